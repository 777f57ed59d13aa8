#!/usr/bin/env python3
"""UMAP of dumped embeddings on MI355X: the `umap.UMAP(...).fit_transform(data)` step of the reference's notebooks
(3.0-Embeddings-inference, 3.1-Embeddings-clustering, 3.2-Embeddings-SSL-categories, 2.0-Figures-MixedWM38) on the HIP
path (ssl_wafermap_amd.manifold).

    python scripts/embedding_umap_amd.py --embeddings tests/golden/simsiam_preds_subset.npz
                                         [--neighbors 15] [--components 2] [--min-dist 0.1] [--epochs N]
                                         [--init spectral|spectral_device|pca|random] [--seed 0] [--no-scale] [--rows N] [--out DIR]
                                         [--densmap [--dens-lambda 2.0] [--dens-frac 0.3] [--dens-var-shift 0.1]]
                                         [--label-frac F] [--holdout N]

What the notebooks do, and where it is here:
  StandardScaler().fit_transform(embeddings)        -> retrieval.StandardScaler (skipped with --no-scale)
  umap.UMAP(n_neighbors, n_components, min_dist, ...).fit_transform(data)
                                                     -> manifold.UMAP: exact kNN graph, fuzzy simplicial set and the
                                                        layout optimisation as HIP kernels
  the 2-D scatter coloured by failure code          -> umap.png (when --components 2)
  umap.UMAP(..., densmap=True, dens_lambda=L)        -> --densmap --dens-lambda L: manifold.DensMAP (the density term in
                                                        the last --dens-frac of the epochs)
  3.0, 2.0-Figures-MixedWM38: labels -1 outside a stratified fraction F, reducer.fit(data, y=labels); reducer.transform(data)
                                                     -> --label-frac F: manifold.InductiveUMAP (with --densmap:
                                                        InductiveDensMAP): the label intersection of the graph before
                                                        the layout, then the transform of the same rows
  fit on some rows, place others                     -> --holdout N: fit on all but the last N rows, transform those
  3.2: HDBSCAN on UMAP(n_neighbors=30, min_dist=0, n_components=50, densmap=True, dens_lambda=0.1).fit_transform(data)
                                                     -> --neighbors 30 --min-dist 0 --components 50 --densmap
                                                        --dens-lambda 0.1, then scripts/embedding_clustering_amd.py
                                                        --embeddings DIR/reduced.npz --no-scale

Outputs under --out: reduced.npz (`embeddings` float32 [n, components], `labels`: the format --embeddings reads; with
--densmap also `rad_orig` and `rad_emb`, the log-radii of the data and of the embedding), umap.png for two components,
summary.json (seconds per stage; sklearn trustworthiness on at most 5 000 seeded rows; with --densmap the Pearson
correlation of the two radii as `radii_correlation`).  With --quality the summary also holds `trustworthiness_full`,
`continuity_full` and `neighbor_preservation` over ALL fitted rows (manifold.embedding_quality: HIP rank kernels, the
same k) with `quality_seconds`, and quality.npz the per-row vectors `trustworthiness_rows`, `continuity_rows` and
`preservation_rows`.  With --label-frac also `transformed` (the fitted rows placed
again by transform) and `labels_kept` in the summary; with --holdout `holdout`, `holdout_labels` (`embeddings` and
`labels` then hold the fitted rows only) and `holdout_recall`: the mean share of a held-out row's 15 nearest fitted rows
in feature space that are among its 15 nearest fitted points in the embedding.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def load_embeddings(path):
    """scripts/embedding_clustering_amd.py's loader (.npz or a reference *_preds_*.pkl.xz)."""
    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", Path(__file__).with_name("embedding_clustering_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_embeddings(path)


def masked_labels(truth, frac: float):
    """The notebook's semi-supervised labels: a stratified fraction `frac` keeps its label
    (sklearn train_test_split(train_size=frac, random_state=42, stratify=labels)), the rest becomes -1.  frac = 1 keeps
    all; a class with a single row cannot be split and keeps its label."""
    truth = np.asarray(truth).astype(np.int64)
    if frac >= 1.0:
        return truth.copy()
    from sklearn.model_selection import train_test_split

    out = np.full(truth.shape, -1, dtype=np.int64)
    single = np.isin(truth, [c for c, cnt in zip(*np.unique(truth, return_counts=True)) if cnt < 2])
    out[single] = truth[single]
    rest = np.flatnonzero(~single)
    keep, _ = train_test_split(rest, train_size=frac, random_state=42, stratify=truth[rest])
    out[keep] = truth[keep]
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--neighbors", type=int, default=15)
    ap.add_argument("--components", type=int, default=2)
    ap.add_argument("--min-dist", type=float, default=0.1)
    ap.add_argument("--epochs", type=int, default=0, help="0: 500 for at most 10 000 rows, 200 above (--densmap: 200 more)")
    ap.add_argument("--densmap", action="store_true", help="DensMAP: add the density-preserving term")
    ap.add_argument("--dens-lambda", type=float, default=2.0)
    ap.add_argument("--dens-frac", type=float, default=0.3)
    ap.add_argument("--dens-var-shift", type=float, default=0.1)
    ap.add_argument("--label-frac", type=float, default=None,
                    help="semi-supervised fit: keep a stratified fraction of the labels, -1 elsewhere; then transform the rows")
    ap.add_argument("--holdout", type=int, default=0, help="fit on all but the last N rows and transform those")
    ap.add_argument("--quality", action="store_true",
                    help="trustworthiness, continuity and neighbour preservation on ALL fitted rows (HIP rank kernels)")
    ap.add_argument("--init", choices=["spectral", "spectral_device", "pca", "random"], default="spectral")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--out", default="umap_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import manifold
    from ssl_wafermap_amd.retrieval import StandardScaler

    common = dict(n_neighbors=a.neighbors, n_components=a.components, min_dist=a.min_dist, n_epochs=a.epochs or None,
                  init=a.init, random_state=a.seed)
    inductive = a.label_frac is not None or a.holdout > 0
    if a.label_frac is not None and not 0.0 < a.label_frac <= 1.0:
        ap.error("--label-frac must be in (0, 1]")
    if a.densmap:
        cls = manifold.InductiveDensMAP if inductive else manifold.DensMAP
        model = cls(dens_lambda=a.dens_lambda, dens_frac=a.dens_frac, dens_var_shift=a.dens_var_shift, **common)
    else:
        model = (manifold.InductiveUMAP if inductive else manifold.UMAP)(**common)
    emb, truth = load_embeddings(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], truth[:a.rows]
    x = torch.from_numpy(emb).to(a.device)
    if not a.no_scale:
        x = StandardScaler().fit_transform(x)
    x_hold = truth_hold = None
    if a.holdout:
        if not 0 < a.holdout < x.shape[0] - 1:
            ap.error("--holdout must leave at least 2 rows to fit")
        x, x_hold = x[:-a.holdout].contiguous(), x[-a.holdout:].contiguous()
        truth, truth_hold = truth[:-a.holdout], truth[-a.holdout:]
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    n = int(x.shape[0])

    # the stages of UMAP.fit, timed one by one (a synchronise closes each)
    seconds = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        seconds[name] = time.perf_counter() - t0
        return res

    k = min(model.n_neighbors, n)
    dist, idx = timed("knn_graph", lambda: manifold.knn_graph(x, k, model.metric))
    graph = timed("fuzzy_set", lambda: manifold.fuzzy_union(idx, manifold.smooth_knn(dist, idx)[2], dist if a.densmap else None))
    if a.densmap:
        graph, dists = graph
    kept = None
    if a.label_frac is not None:
        kept = masked_labels(truth, a.label_frac)
        target = torch.from_numpy(kept.astype(np.int32)).to(x.device)
        graph = timed("label_intersect", lambda: manifold.label_intersect(graph, target, manifold.far_distance(model.target_weight)))
    y0 = timed("init", lambda: model._initial(manifold._prep(x), graph))
    q = manifold.sample_rates(graph.data)
    layout_args = dict(gamma=model.repulsion_strength, learning_rate=model.learning_rate, seed=model.random_state,
                       negative_sample_rate=model.negative_sample_rate)
    extra = {}
    if a.densmap:
        n_epochs = model.default_epochs(n)
        rad_orig = timed("graph_radii", lambda: manifold.graph_radii(graph.indptr, graph.data, dists, q, n_epochs))
        y = timed("layout", lambda: manifold.optimize_layout_densmap(
            y0, graph.indptr, graph.indices, q, graph.data, manifold.standardize_radii(rad_orig), model.a_, model.b_, n_epochs,
            dens_lambda=model.dens_lambda, dens_frac=model.dens_frac, dens_var_shift=model.dens_var_shift, **layout_args))
        rad_emb = manifold.embedding_radii(y, graph.indptr, graph.indices, q, model.a_, model.b_, n_epochs)[0]
        extra = {"rad_orig": rad_orig.cpu().numpy(), "rad_emb": rad_emb.cpu().numpy()}
    else:
        n_epochs = model.n_epochs if model.n_epochs is not None else (500 if n <= 10000 else 200)
        y = timed("layout", lambda: manifold.optimize_layout(y0, graph.indptr, graph.indices, q, model.a_, model.b_, n_epochs,
                                                             **layout_args))
    if inductive:
        # what fit leaves behind, then transform's steps timed one by one
        model._train, model.embedding_, model.graph_ = manifold._prep(x), y, graph

        def place(rows_, tag=""):
            xq = manifold._prep(rows_)
            qd, qi = timed("knn_query" + tag, lambda: manifold.knn_query(xq, model._train, k, model.metric))
            w = timed("memberships" + tag, lambda: manifold.smooth_knn_query(qd)[1])
            start = timed("start" + tag, lambda: model.transform_init(qi, w))
            return timed("transform_layout" + tag, lambda: manifold.optimize_transform(
                start, y, qi, manifold.sample_rates(w), model.a_, model.b_, model.transform_epochs(int(xq.shape[0])),
                seed=model.transform_seed, **{key: v for key, v in layout_args.items() if key != "seed"}))

        if a.label_frac is not None:
            extra["transformed"] = place(x, "" if x_hold is None else "_fitted").cpu().numpy()
        if x_hold is not None:
            held = place(x_hold)
            kk = min(15, n)
            near_x = manifold.knn_query(x_hold, x, kk, model.metric)[1]
            near_y = manifold.knn_query(held, y, kk)[1]
            holdout_recall = float((near_x.unsqueeze(2) == near_y.unsqueeze(1)).any(dim=2).double().mean())
            extra.update(holdout=held.cpu().numpy(), holdout_labels=truth_hold)
    reduced = y.cpu().numpy()
    np.savez(out / "reduced.npz", embeddings=reduced, labels=truth, **extra)

    from sklearn.manifold import trustworthiness

    pick = np.sort(np.random.default_rng(a.seed).permutation(n)[:5000])
    xs = x[torch.from_numpy(pick).to(x.device)].cpu().numpy()
    score = float(trustworthiness(xs, reduced[pick], n_neighbors=min(15, max(1, (pick.size - 1) // 2 - 1))))
    quality = None
    if a.quality:
        # every fitted row, k as the sub-sampled score chooses it (sklearn needs k < n / 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quality = manifold.embedding_quality(x, y, min(15, max(1, (n - 1) // 2 - 1)), metric=model.metric)
        quality_seconds = time.perf_counter() - t0  # (the scores are on the host: nothing is pending)
        np.savez(out / "quality.npz", trustworthiness_rows=quality.trustworthiness_rows, continuity_rows=quality.continuity_rows,
                 preservation_rows=quality.preservation_rows)
    if a.components == 2:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        fig, ax = plt.subplots(figsize=(7, 7))
        sc = ax.scatter(reduced[:, 0], reduced[:, 1], c=truth, cmap="tab10", s=4)
        ax.legend(*sc.legend_elements(), title="failure code", loc="best", fontsize=7)
        ax.set_title(f"{'DensMAP' if a.densmap else 'UMAP'} of {n} embeddings (n_neighbors={k}, min_dist={a.min_dist})")
        fig.savefig(out / "umap.png", dpi=120)
        plt.close(fig)
    summary = {"n": n, "d": int(x.shape[1]), "n_neighbors": k, "n_components": a.components, "min_dist": a.min_dist,
               "n_epochs": n_epochs, "init": a.init, "a": model.a_, "b": model.b_, "graph_entries": int(graph.indices.numel()),
               "seconds": seconds, "trustworthiness": score, "trustworthiness_rows": int(pick.size)}
    if quality is not None:
        summary.update(trustworthiness_full=quality.trustworthiness, continuity_full=quality.continuity,
                       neighbor_preservation=quality.neighbor_preservation, quality_seconds=quality_seconds)
    if a.densmap:
        summary.update(densmap=True, dens_lambda=model.dens_lambda, dens_frac=model.dens_frac, dens_var_shift=model.dens_var_shift,
                       radii_correlation=float(np.corrcoef(extra["rad_orig"].astype(np.float64),
                                                           extra["rad_emb"].astype(np.float64))[0, 1]))
    if kept is not None:
        summary.update(label_frac=a.label_frac, labels_kept=int((kept >= 0).sum()), target_weight=model.target_weight)
    if x_hold is not None:
        summary.update(holdout=int(x_hold.shape[0]), holdout_recall=holdout_recall)
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"UMAP of {n} x {x.shape[1]} -> {a.components}-D in {sum(seconds.values()):.2f} s "
          f"({', '.join(f'{s} {v:.3f}' for s, v in seconds.items())}); trustworthiness {score:.4f} -> {out}")
    return summary


if __name__ == "__main__":
    main()
