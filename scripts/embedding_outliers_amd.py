#!/usr/bin/env python3
"""Local outlier factor of dumped embeddings on MI355X (ssl_wafermap_amd.neighbors): "which wafers look like nothing we
have seen", as a local, density-based, model-free score -- sklearn.neighbors.LocalOutlierFactor over the exact kNN lists,
next to the GLOSH scores of scripts/embedding_clustering_amd.py (relative to one HDBSCAN tree) and the log-likelihoods of
scripts/embedding_gmm_amd.py (elliptical clusters).

    python scripts/embedding_outliers_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --neighbors 10:40:10
                                             [--contamination auto|0.05] [--holdout N] [--rows N] [--no-scale] [--top 20]
                                             [--out DIR]

It standardises the rows (retrieval.StandardScaler; skipped with --no-scale) and scores every row for every neighbour
count of --neighbors (one number, or LO:HI[:STEP] with both ends) from ONE kNN graph at the largest count: the counts share
every pass over the lists (neighbors.outlier_scores).  Breunig et al. recommend the maximum LOF over a range of counts: the
combined score of a row is that maximum, and a row is flagged (-1 in labels.npy) where its combined score, negated as
sklearn negates it, lies below the offset: -1.5 for --contamination auto, else the 100 * contamination percentile.

Outputs under --out: negative_outlier_factor.npy (float64 [R + 1, n]: one row per count, then the combined one),
labels.npy (int64 [n], +1 / -1), kdist.npy (float32 [R, n], the distance to the k-th neighbour), indegree.npy (int32 [R, n],
how many lists a row appears in: 0 marks an "anti-hub", the ODIN outlier score) and summary.json: the rows flagged per count
and combined, the hubness (skewness of the in-degrees) per count, the --top most anomalous rows, and, when the file carries
labels, the mean LOF per class.

--holdout N keeps the last N rows out of the scaler and the fit and scores them as NEW rows against the others
(LocalOutlierFactor(novelty=True).score_samples, per count): holdout_negative_outlier_factor.npy ([R + 1, N]),
holdout_labels.npy, and in summary.json `holdout` and `holdout_flagged`.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def parse_neighbors(text: str):
    """'20' -> [20]; '10:40:10' -> [10, 20, 30, 40]; '5:8' -> [5, 6, 7, 8]."""
    parts = text.split(":")
    try:
        nums = [int(p) for p in parts]
    except ValueError:
        nums = []
    if len(nums) == 1 and nums[0] >= 1:
        return nums
    if len(nums) in (2, 3) and 1 <= nums[0] <= nums[1] and (len(nums) == 2 or nums[2] >= 1):
        return list(range(nums[0], nums[1] + 1, nums[2] if len(nums) == 3 else 1))
    raise ValueError(f"--neighbors {text!r}: a number or LO:HI[:STEP] with 1 <= LO <= HI expected")


def parse_contamination(text: str):
    return text if text == "auto" else float(text)


def load(path):
    """(embeddings float32 [n, d], labels int64 [n] or None)."""
    path = Path(path)
    if path.suffix == ".npz":
        z = np.load(path)
        return z["embeddings"].astype(np.float32), (np.asarray(z["labels"]).astype(np.int64) if "labels" in z.files else None)
    from scripts.embedding_kmeans_amd import load_embeddings

    return load_embeddings(path)


def combined(nof: np.ndarray) -> np.ndarray:
    """[R + 1, n]: the rows of nof and under them the negated maximum LOF over the counts (the minimum of the rows)."""
    return np.concatenate([nof, nof.min(axis=0, keepdims=True)], axis=0)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--neighbors", default="20", help="a number, or LO:HI[:STEP] with both ends")
    ap.add_argument("--contamination", default="auto", help="'auto' (offset -1.5) or a share in (0, 0.5]")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last N rows out of the fit and score them as new rows")
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--top", type=int, default=20, help="how many of the most anomalous rows summary.json lists")
    ap.add_argument("--out", default="outliers_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import neighbors
    from ssl_wafermap_amd.retrieval import StandardScaler

    ks = parse_neighbors(a.neighbors)
    contamination = neighbors.check_contamination(parse_contamination(a.contamination))
    emb, truth = load(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], (None if truth is None else truth[:a.rows])
    if not 0 <= a.holdout < emb.shape[0]:
        raise ValueError(f"--holdout ({a.holdout}) must be in [0, rows = {emb.shape[0]})")
    n_fit = emb.shape[0] - a.holdout
    neighbors.check_ks(ks, min(n_fit - 1, neighbors.MAX_K))
    x = torch.from_numpy(emb[:n_fit]).to(a.device)
    x_hold = torch.from_numpy(emb[n_fit:]).to(a.device) if a.holdout else None
    if not a.no_scale:
        scaler = StandardScaler()
        x = scaler.fit_transform(x)
        if a.holdout:
            x_hold = scaler.transform(x_hold)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    t0 = time.perf_counter()
    scores = neighbors.outlier_scores(x, ks)
    nof = combined(-scores.lof.cpu().numpy())
    kdist, indegree = scores.kdist.cpu().numpy(), scores.indegree.cpu().numpy()
    seconds = time.perf_counter() - t0
    offsets = [neighbors.offset_for(row, contamination) for row in nof]
    labels = neighbors.labels_from(nof[-1], offsets[-1])
    np.save(out / "negative_outlier_factor.npy", nof)
    np.save(out / "labels.npy", labels)
    np.save(out / "kdist.npy", kdist)
    np.save(out / "indegree.npy", indegree)

    order = np.argsort(nof[-1], kind="stable")[:max(0, a.top)]
    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "neighbors": ks, "contamination": contamination, "scaled": not a.no_scale,
               "offsets": offsets, "flagged": {str(k): int((nof[r] < offsets[r]).sum()) for r, k in enumerate(ks)},
               "flagged_combined": int((labels == -1).sum()),
               "hubness": {str(k): neighbors.skewness(indegree[r]) for r, k in enumerate(ks)},
               "never_listed": {str(k): int((indegree[r] == 0).sum()) for r, k in enumerate(ks)},
               "most_anomalous_rows": order.tolist(), "most_anomalous_lof": (-nof[-1][order]).tolist(), "seconds": seconds}
    if truth is not None:
        fit_truth = truth[:n_fit]
        summary["mean_lof_per_class"] = {str(int(c)): float(-nof[-1][fit_truth == c].mean()) for c in np.unique(fit_truth)}
        summary["flagged_per_class"] = {str(int(c)): int((labels[fit_truth == c] == -1).sum()) for c in np.unique(fit_truth)}
    for r, k in enumerate(ks):
        print(f"k = {k}: {summary['flagged'][str(k)]} rows below the offset {offsets[r]:.4f}, hubness {summary['hubness'][str(k)]:.3f}, "
              f"{summary['never_listed'][str(k)]} rows in no list")
    print(f"combined (maximum LOF over {len(ks)} counts): {summary['flagged_combined']} of {x.shape[0]} rows flagged; most anomalous rows "
          f"{order[:5].tolist()} with LOF {[round(v, 3) for v in summary['most_anomalous_lof'][:5]]}")

    if a.holdout:
        rows = []
        for k in ks:
            model = neighbors.LocalOutlierFactor(k, contamination=contamination, novelty=True).fit(x)
            rows.append(model.score_samples(x_hold))
        hold = combined(np.stack(rows))
        hold_labels = neighbors.labels_from(hold[-1], offsets[-1])  # the fitted rows' offset judges the new rows
        np.save(out / "holdout_negative_outlier_factor.npy", hold)
        np.save(out / "holdout_labels.npy", hold_labels)
        summary.update(holdout=int(a.holdout), holdout_flagged=int((hold_labels == -1).sum()),
                       holdout_flagged_per_count={str(k): int((hold[r] < offsets[r]).sum()) for r, k in enumerate(ks)})
        print(f"held-out rows: {a.holdout} scored as new rows, {summary['holdout_flagged']} flagged")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(ks)} neighbour counts on {x.shape[0]} x {x.shape[1]} in {seconds:.2f} s (graph, passes and copies) -> {out}")
    return summary


if __name__ == "__main__":
    main()
