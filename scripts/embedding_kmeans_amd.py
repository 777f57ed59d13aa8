#!/usr/bin/env python3
"""KMeans sweep over the number of clusters on dumped embeddings on MI355X (ssl_wafermap_amd.cluster.KMeans): "k groups,
every wafer in one", the partition that scripts/embedding_clustering_amd.py (HDBSCAN, which leaves noise rows) does not
give, and the reference's sklearn.cluster.KMeans(n_clusters=k) .fit / .predict of notebooks/1.0-Preprocess-WM811K.ipynb.

    python scripts/embedding_kmeans_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --k 25:50 --n-init 10
                                           [--init k-means++|random] [--seed 0] [--no-scale] [--rows N] [--holdout N]
                                           [--out DIR]

It standardises the rows (retrieval.StandardScaler; skipped with --no-scale), fits every k of --k LO:HI (both ends; a
single number is one k) with --n-init restarts that advance together, one assignment pass per iteration for all of them,
and scores each fit with the scores of the HDBSCAN sweep: silhouette, Calinski-Harabasz, Davies-Bouldin and homogeneity
against the failure codes.

Outputs under --out: trials.csv (k, inertia, n_iter, the four scores, seconds), and for the chosen k (the best
silhouette, the lowest k among equals) labels.npy (int64 [n]), centers.npy (float32 [k, d], in the scaled space) and
summary.json.  The nearest wafers of every centre are printed (retrieval.nearest_neighbors, L2): the centre as the
prototype wafer of its group.

--holdout N keeps the last N rows out of the scaler and the fits and asks the chosen model about them
(KMeans.predict): holdout_labels.npy, and in summary.json `holdout` and `holdout_homogeneity`.
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

COLUMNS = ["k", "inertia", "n_iter", "homogeneity", "silhouette", "calinski_harabasz", "davies_bouldin", "seconds"]


def parse_k(text: str):
    lo, _, hi = text.partition(":")
    lo, hi = int(lo), int(hi or lo)
    if not 2 <= lo <= hi:
        raise ValueError(f"--k {text!r}: LO:HI with 2 <= LO <= HI expected")
    return list(range(lo, hi + 1))


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


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--k", default="25:50", help="LO:HI, both ends, or one number")
    ap.add_argument("--n-init", type=int, default=10)
    ap.add_argument("--init", choices=["k-means++", "random"], default="k-means++")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last N rows out of the fits and predict them")
    ap.add_argument("--out", default="kmeans_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import cluster
    from ssl_wafermap_amd.retrieval import StandardScaler, nearest_neighbors

    ks = parse_k(a.k)
    emb, truth = load_embeddings(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], truth[:a.rows]
    if not 0 <= a.holdout < emb.shape[0]:
        raise ValueError(f"--holdout ({a.holdout}) must be in [0, rows = {emb.shape[0]})")
    n_fit = emb.shape[0] - a.holdout
    if ks[-1] > n_fit - 1:
        raise ValueError(f"--k up to {ks[-1]} needs more than {n_fit} rows")
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

    rows, models = [], {}
    t_all = time.perf_counter()
    for k in ks:
        t0 = time.perf_counter()
        model = cluster.KMeans(k, init=a.init, n_init=a.n_init, random_state=a.seed + k).fit(x)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        labels = model.labels_
        rows.append({"k": k, "inertia": model.inertia_, "n_iter": model.n_iter_,
                     "homogeneity": cluster.homogeneity_score(truth, labels),
                     "silhouette": cluster.silhouette_score(x, labels),
                     "calinski_harabasz": cluster.calinski_harabasz_score(x, labels),
                     "davies_bouldin": cluster.davies_bouldin_score(x, labels), "seconds": seconds})
        models[k] = model
    wall = time.perf_counter() - t_all
    with open(out / "trials.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=COLUMNS)
        wr.writeheader()
        wr.writerows(rows)
    best = max(rows, key=lambda r: (r["silhouette"], -r["k"]))
    model = models[best["k"]]
    labels, centres = model.labels_, model.cluster_centers_
    np.save(out / "labels.npy", labels)
    np.save(out / "centers.npy", centres.cpu().numpy())
    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "k": [ks[0], ks[-1]], "n_init": a.n_init, "init": a.init,
               "sweep_seconds": wall, "fit_seconds": float(sum(r["seconds"] for r in rows)), "chosen_k": best["k"],
               "chosen": {c: best[c] for c in COLUMNS}, "cluster_sizes": np.bincount(labels, minlength=best["k"]).tolist()}
    print(f"chosen k = {best['k']}: {best}")
    dist, idx = nearest_neighbors(centres.contiguous(), x, min(5, x.shape[0]), metric="l2")
    for c, (dr, ir) in enumerate(zip(dist.cpu().tolist(), idx.cpu().tolist())):
        near = [(j, round(dd, 4), int(truth[j])) for j, dd in zip(ir, dr)]
        print(f"centre {c} ({summary['cluster_sizes'][c]} wafers); nearest (row, L2, failure code): {near}")
    if a.holdout:
        h_labels = model.predict(x_hold)
        np.save(out / "holdout_labels.npy", h_labels)
        summary.update(holdout=int(a.holdout), holdout_homogeneity=cluster.homogeneity_score(truth_hold, h_labels))
        print(f"held-out rows: {a.holdout} assigned; homogeneity {summary['holdout_homogeneity']:.4f}")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(ks)} values of k x {a.n_init} restarts on {x.shape[0]} x {x.shape[1]} in {wall:.2f} s "
          f"({summary['fit_seconds']:.2f} s in the fits) -> {out}")
    return summary


if __name__ == "__main__":
    main()
