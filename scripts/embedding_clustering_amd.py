#!/usr/bin/env python3
"""HDBSCAN hyper-parameter sweep on dumped embeddings on MI355X: the flow of the reference's
notebooks/3.1-Embeddings-clustering.ipynb and 3.2-Embeddings-SSL-categories.ipynb on the HIP path
(ssl_wafermap_amd.cluster).

    python scripts/embedding_clustering_amd.py --embeddings tests/golden/simsiam_preds_subset.npz
                                               [--trials 30] [--design random|grid] [--seed 0] [--rows N]
                                               [--metrics euclidean manhattan] [--no-scale] [--out DIR]
                                               [--holdout N] [--soft] [--validity]

What the notebooks do, and where it is here:
  StandardScaler().fit_transform(embeddings)              -> retrieval.StandardScaler (skipped with --no-scale)
  Ax search, 30 trials, over min_samples 1-60, min_cluster_size 10-100, cluster_selection_epsilon 0.1-1.5, metric
                                                          -> a seeded random set or grid of --trials points over the
                                                             same ranges (no Bayesian model); the trials draw their
                                                             (metric, min_samples) from a few values, and one
                                                             spanning tree serves all trials that share the pair
  hdbscan.HDBSCAN(...).fit(data)                          -> cluster.HDBSCAN.fit / .refit
  homogeneity / silhouette / calinski_harabasz / davies_bouldin on the non-noise rows
                                                          -> cluster.homogeneity_score, silhouette_score, ...
  get_pareto_optimal_parameters()                         -> the non-dominated rows of the table (silhouette,
                                                             calinski_harabasz, homogeneity up; davies_bouldin
                                                             down; and, beyond the notebooks' four scores,
                                                             n_noise down)
  nearest wafers of a member of each cluster              -> retrieval.nearest_neighbors (5 neighbours, L2)
UMAP is a script of its own: scripts/embedding_umap_amd.py writes a reduced.npz that --embeddings reads (add --no-scale),
which is notebook 3.2's reduce-then-cluster flow in two commands.  `min_samples` counts the point itself (sklearn's convention; the `hdbscan` package's
generic path counts one neighbour more).  The canberra and braycurtis metrics of the notebook's search space have
no kernel and are refused.

Outputs under --out: trials.csv (parameters, n_clusters, n_noise, the four scores), pareto.csv, labels.npy (the
chosen trial: the Pareto row with the best silhouette), summary.json.

--holdout N keeps the last N rows out of the scaler and the sweep and asks the chosen trial's model about them
(cluster.approximate_predict / approximate_predict_scores: which cluster, how surely, how anomalous):
holdout_labels.npy, holdout_probabilities.npy, holdout_outlier_scores.npy, and in summary.json `holdout`,
`holdout_noise` and `holdout_homogeneity` (truth against the predicted label over the held-out rows not labelled noise;
null when there are none).

--soft adds the soft clustering of the chosen trial (cluster.all_points_membership_vectors / membership_vector: how
strongly every row, noise rows included, belongs to every cluster): membership.npy [n, n_clusters], exemplars.npz
(`rows`: the exemplar rows of all clusters, `cluster`: the cluster of each), with --holdout also
holdout_membership.npy [N, n_clusters]; and in summary.json `soft_noise_above_half` (the share of the noise rows whose
largest membership exceeds 0.5; null without noise rows) and `soft_mean_row_sum` (the mean probability of belonging
to any cluster).

--validity scores every trial without ground truth, by density and not by convexity (the `hdbscan` package's two scores):
the columns `relative_validity` (HDBSCAN.relative_validity_: from the trial's spanning tree, free) and `dbcv`
(cluster.validity_index: DBCV on the GPU; NaN for a trial with fewer than two clusters) follow the columns above in
trials.csv and pareto.csv, `dbcv` joins the Pareto objectives (up), and summary.json names `chosen_by_dbcv`, the trial with
the best DBCV (null when no trial has one).  Without the flag nothing changes.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

RANGES = {"min_samples": (1, 60), "min_cluster_size": (10, 100), "cluster_selection_epsilon": (0.1, 1.5)}
COLUMNS = ["trial", "metric", "min_samples", "min_cluster_size", "cluster_selection_epsilon", "n_clusters", "n_noise",
           "homogeneity", "silhouette", "calinski_harabasz", "davies_bouldin"]
# (column, +1 when larger is better)
OBJECTIVES = [("silhouette", 1), ("calinski_harabasz", 1), ("homogeneity", 1), ("davies_bouldin", -1), ("n_noise", -1)]
VALIDITY_COLUMNS = ["relative_validity", "dbcv"]  # --validity: after COLUMNS
VALIDITY_OBJECTIVES = [("dbcv", 1)]  # --validity: after OBJECTIVES


def load_embeddings(path):
    """(embeddings float32 [n, d], labels int [n]) from an .npz with `embeddings` / `labels` or a reference
    *_preds_*.pkl.xz (a DataFrame with the feature columns 0..d-1 and failureCode)."""
    path = Path(path)
    if path.suffix == ".npz":
        z = np.load(path)
        return z["embeddings"].astype(np.float32), np.asarray(z["labels"]).astype(np.int64)
    import pandas as pd

    df = pd.read_pickle(path)
    cols = [c for c in df.columns if isinstance(c, (int, np.integer))]
    return df[cols].to_numpy().astype(np.float32), df["failureCode"].to_numpy().astype(np.int64)


def design_trials(trials: int, design: str, seed: int, metrics, max_samples: int):
    """`trials` parameter points.  The (metric, min_samples) pairs come from a pool of about trials / 3 distinct
    values, so that several trials share one spanning tree."""
    rng = np.random.default_rng(seed)
    lo, hi = RANGES["min_samples"]
    hi = min(hi, max_samples)
    n_pairs = max(1, min(-(-trials // 3), (hi - lo + 1) * len(metrics)))
    if design == "grid":
        ms = np.unique(np.linspace(lo, hi, -(-n_pairs // len(metrics))).round().astype(int))
        pairs = [(m, int(s)) for s in ms for m in metrics][:n_pairs]
    else:
        pairs = []
        while len(pairs) < n_pairs:
            cand = (metrics[int(rng.integers(len(metrics)))], int(rng.integers(lo, hi + 1)))
            if cand not in pairs:
                pairs.append(cand)
    out = []
    per = -(-trials // len(pairs))
    for t in range(trials):
        metric, ms = pairs[t // per] if design == "grid" else pairs[t % len(pairs)]
        if design == "grid":
            side = max(1, int(np.ceil(np.sqrt(per))))
            a, b = divmod(t % per, side)
            mcs = int(round(np.linspace(*RANGES["min_cluster_size"], side)[a % side]))
            eps = float(np.linspace(*RANGES["cluster_selection_epsilon"], side)[b])
        else:
            mcs = int(rng.integers(RANGES["min_cluster_size"][0], RANGES["min_cluster_size"][1] + 1))
            eps = float(rng.uniform(*RANGES["cluster_selection_epsilon"]))
        out.append({"metric": metric, "min_samples": ms, "min_cluster_size": mcs, "cluster_selection_epsilon": eps})
    return out


def pareto_rows(rows, objectives=None):
    """Indices of the rows no other row dominates on `objectives` (OBJECTIVES when None; rows without finite scores
    never qualify)."""
    vals = np.array([[s * float(r[c]) for c, s in objectives or OBJECTIVES] for r in rows], dtype=np.float64)
    ok = np.isfinite(vals).all(axis=1)
    keep = []
    for i in np.flatnonzero(ok):
        dominated = any(j != i and (vals[j] >= vals[i]).all() and (vals[j] > vals[i]).any() for j in np.flatnonzero(ok))
        if not dominated:
            keep.append(int(i))
    return keep


def score_trial(x, truth, labels, metric):
    from ssl_wafermap_amd import cluster

    import torch

    n_clusters, n_noise = int(labels.max()) + 1, int((labels == -1).sum())
    row = {"n_clusters": n_clusters, "n_noise": n_noise, "homogeneity": float("nan"), "silhouette": float("nan"),
           "calinski_harabasz": float("nan"), "davies_bouldin": float("nan")}
    keep = labels != -1
    if n_clusters >= 2:  # the scores are defined for 2 <= n_clusters <= n_kept - 1
        xs = x[torch.from_numpy(np.flatnonzero(keep)).to(x.device)].contiguous()
        row["homogeneity"] = cluster.homogeneity_score(truth[keep], labels[keep])
        row["silhouette"] = cluster.silhouette_score(xs, labels[keep], metric)
        row["calinski_harabasz"] = cluster.calinski_harabasz_score(xs, labels[keep])
        row["davies_bouldin"] = cluster.davies_bouldin_score(xs, labels[keep])
    return row


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--trials", type=int, default=30)
    ap.add_argument("--design", choices=["random", "grid"], default="random")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--metrics", nargs="+", default=["euclidean", "manhattan"])
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--out", default="clustering_out")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last N rows out of the sweep and predict them")
    ap.add_argument("--soft", action="store_true", help="write the chosen trial's membership vectors and exemplars")
    ap.add_argument("--validity", action="store_true", help="add the relative_validity and dbcv columns and the dbcv objective")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import cluster
    from ssl_wafermap_amd.retrieval import StandardScaler, nearest_neighbors

    for m in a.metrics:
        cluster.metric_code(m)  # canberra / braycurtis: NotImplementedError naming the metric
    emb, truth = load_embeddings(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], truth[:a.rows]
    if not 0 <= a.holdout < emb.shape[0]:
        raise ValueError(f"--holdout ({a.holdout}) must be in [0, rows = {emb.shape[0]})")
    n_fit = emb.shape[0] - a.holdout
    x, x_hold = torch.from_numpy(emb[:n_fit]).to(a.device), None
    if a.holdout:
        x_hold, truth_hold, truth = torch.from_numpy(emb[n_fit:]).to(a.device), truth[n_fit:], truth[:n_fit]
    if not a.no_scale:
        scaler = StandardScaler()
        x = scaler.fit_transform(x)
        if a.holdout:
            x_hold = scaler.transform(x_hold)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    trials = design_trials(a.trials, a.design, a.seed, list(a.metrics), min(64, x.shape[0]))
    trees, rows, all_labels = {}, [], []
    t0 = time.perf_counter()
    for t, p in enumerate(trials):
        key = (p["metric"], p["min_samples"])
        if key not in trees:
            trees[key] = cluster.HDBSCAN(min_cluster_size=p["min_cluster_size"], min_samples=p["min_samples"],
                                         metric=p["metric"], prediction_data=a.holdout > 0 or a.soft).fit(x)
        model = trees[key].refit(min_cluster_size=p["min_cluster_size"],
                                 cluster_selection_epsilon=p["cluster_selection_epsilon"])
        labels = model.labels_.copy()
        all_labels.append(labels)
        rows.append({"trial": t, **p, **score_trial(x, truth, labels, p["metric"])})
        if a.validity:
            rows[-1]["relative_validity"] = model.relative_validity_
            rows[-1]["dbcv"] = cluster.validity_index(x, labels, p["metric"]) if rows[-1]["n_clusters"] >= 2 else float("nan")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    columns = COLUMNS + VALIDITY_COLUMNS if a.validity else COLUMNS
    with open(out / "trials.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=columns)
        wr.writeheader()
        wr.writerows(rows)
    front = pareto_rows(rows, OBJECTIVES + VALIDITY_OBJECTIVES if a.validity else None)
    with open(out / "pareto.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=columns)
        wr.writeheader()
        wr.writerows(rows[i] for i in front)
    chosen = max(front, key=lambda i: rows[i]["silhouette"]) if front else None
    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "trials": len(rows), "n_trees": len(trees),
               "sweep_seconds": wall, "pareto": front, "chosen": chosen}
    if a.validity:
        scored = [i for i, r in enumerate(rows) if np.isfinite(r["dbcv"])]
        summary["chosen_by_dbcv"] = max(scored, key=lambda i: rows[i]["dbcv"]) if scored else None
    if a.holdout:
        summary.update(holdout=int(a.holdout), holdout_noise=None, holdout_homogeneity=None)  # (filled for a chosen trial)
    if chosen is not None:
        labels = all_labels[chosen]
        np.save(out / "labels.npy", labels)
        print(f"chosen trial {chosen}: {rows[chosen]}")
        members = [int(np.flatnonzero(labels == c)[0]) for c in range(int(labels.max()) + 1)]
        q = x[torch.tensor(members, device=x.device)].contiguous()
        dist, idx = nearest_neighbors(q, x, min(6, x.shape[0]), metric="l2")
        for c, (m, dr, ir) in enumerate(zip(members, dist.cpu().tolist(), idx.cpu().tolist())):
            near = [(j, round(dd, 4), int(truth[j])) for j, dd in zip(ir, dr) if j != m][:5]
            print(f"cluster {c}: member {m} (failure code {int(truth[m])}); nearest (row, L2, failure code): {near}")
        if a.holdout or a.soft:
            p = trials[chosen]
            model = trees[(p["metric"], p["min_samples"])].refit(min_cluster_size=p["min_cluster_size"],
                                                                 cluster_selection_epsilon=p["cluster_selection_epsilon"])
        if a.holdout:
            h_labels, h_prob = cluster.approximate_predict(model, x_hold)
            h_scores = cluster.approximate_predict_scores(model, x_hold)
            np.save(out / "holdout_labels.npy", h_labels)
            np.save(out / "holdout_probabilities.npy", h_prob)
            np.save(out / "holdout_outlier_scores.npy", h_scores)
            keep = h_labels != -1
            summary.update(holdout_noise=int((~keep).sum()),
                           holdout_homogeneity=cluster.homogeneity_score(truth_hold[keep], h_labels[keep]) if keep.any() else None)
            print(f"held-out rows: {int(keep.sum())} of {a.holdout} assigned to a cluster, homogeneity "
                  f"{summary['holdout_homogeneity']}")
        if a.soft:
            member = cluster.all_points_membership_vectors(model)
            np.save(out / "membership.npy", member)
            ex = model.exemplar_indices_
            np.savez(out / "exemplars.npz", rows=np.concatenate(ex) if ex else np.zeros(0, dtype=np.int64),
                     cluster=np.repeat(np.arange(len(ex)), [r.size for r in ex]).astype(np.int64))
            if a.holdout:
                np.save(out / "holdout_membership.npy", cluster.membership_vector(model, x_hold))
            noise = labels == -1
            summary.update(soft_noise_above_half=float((member[noise].max(axis=1) > 0.5).mean()) if noise.any() else None,
                           soft_mean_row_sum=float(member.sum(axis=1).mean()))
            print(f"soft clustering: {sum(r.size for r in ex)} exemplars; mean row sum {summary['soft_mean_row_sum']:.4f}; noise rows "
                  f"with a membership above 0.5: {summary['soft_noise_above_half']}")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(rows)} trials on {x.shape[0]} x {x.shape[1]} in {wall:.2f} s with {len(trees)} spanning trees; "
          f"{len(front)} Pareto-optimal rows -> {out}")
    return summary


if __name__ == "__main__":
    main()
