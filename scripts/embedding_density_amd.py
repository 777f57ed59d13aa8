#!/usr/bin/env python3
"""Gaussian kernel density of dumped embeddings on MI355X (ssl_wafermap_amd.density): a per-wafer log density that assumes
neither the ellipses of scripts/embedding_gmm_amd.py nor the one neighbour count of scripts/embedding_outliers_amd.py --
sklearn.neighbors.KernelDensity by brute force over ALL rows, for a list of bandwidths in one pass -- with the bandwidth
chosen without labels by the leave-one-out likelihood, the class-conditional classifier when the file carries labels, and
the uniformity of the embedding (Wang & Isola 2020).

    python scripts/embedding_density_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --bandwidths 2:40:7
                                            [--pca 50] [--holdout N] [--by-class] [--contamination 0.05] [--rows N]
                                            [--no-scale] [--out DIR]

It standardises the rows (retrieval.StandardScaler; skipped with --no-scale), reduces them to --pca dimensions
(decomposition.PCA; 0, the default: no reduction) and scores every row under the OTHER rows for every bandwidth of
--bandwidths: LO:HI:COUNT (log-spaced, both ends), one number, or `scott` / `silverman` (sklearn's rules of thumb).  The
chosen bandwidth is the one with the largest leave-one-out log-likelihood.  --by-class (the file must carry labels; rows
labelled -1 are left out of the classifier) adds, per bandwidth, the leave-one-out accuracy and macro F1 of
density.KDEClassifier.

Outputs under --out: trials.csv (per bandwidth: loo_log_likelihood, its mean per row and, with --by-class, loo_accuracy
and loo_macro_f1), log_density.npy (float64 [n]: the leave-one-out log density at the chosen bandwidth), flagged.npy
(int64: the rows of the lowest --contamination share of those, most anomalous first) and summary.json: the chosen
bandwidth, `uniformity` at t = 2 on the rows as the density saw them (normalised to unit length for this figure alone),
the flagged count and, when the file carries labels, the mean log density per class.

--holdout N keeps the last N rows out of the scaler, the PCA and the fit and scores them as NEW rows at the chosen
bandwidth (KernelDensity.score_samples): holdout_log_density.npy ([N]) and, in summary.json, `holdout` and
`holdout_below_threshold` (the new rows below the flagged rows' threshold).
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

from scripts.embedding_outliers_amd import load  # noqa: E402


def parse_bandwidths(text: str):
    """'scott' / 'silverman' -> that name; '1.5' -> [1.5]; '0.5:20:6' -> six log-spaced values from 0.5 to 20."""
    if text in ("scott", "silverman"):
        return text
    parts = text.split(":")
    try:
        if len(parts) == 1 and float(parts[0]) > 0:
            return [float(parts[0])]
        if len(parts) == 3:
            lo, hi, count = float(parts[0]), float(parts[1]), int(parts[2])
            if 0 < lo <= hi and count >= 1 and (count > 1 or lo == hi):
                return [float(v) for v in np.geomspace(lo, hi, count)]
    except ValueError:
        pass
    raise ValueError(f"--bandwidths {text!r}: a positive number, LO:HI:COUNT with 0 < LO <= HI, 'scott' or 'silverman' expected")


def macro_f1(truth: np.ndarray, pred: np.ndarray) -> float:
    """The unweighted mean over the classes of `truth` of 2 tp / (2 tp + fp + fn) (0 for a class never hit)."""
    scores = []
    for c in np.unique(truth):
        tp = float(np.sum((pred == c) & (truth == c)))
        fp, fn = float(np.sum((pred == c) & (truth != c))), float(np.sum((pred != c) & (truth == c)))
        scores.append(0.0 if tp == 0 else 2 * tp / (2 * tp + fp + fn))
    return float(np.mean(scores))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--bandwidths", default="scott", help="LO:HI:COUNT (log-spaced), a number, 'scott' or 'silverman'")
    ap.add_argument("--pca", type=int, default=0, help="reduce to this many dimensions first (0: no reduction)")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last N rows out of the fit and score them as new rows")
    ap.add_argument("--by-class", action="store_true", help="leave-one-out accuracy and macro F1 of the class-conditional classifier")
    ap.add_argument("--contamination", type=float, default=0.05, help="the share of rows flagged as the least dense")
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--out", default="density_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import decomposition, density
    from ssl_wafermap_amd.retrieval import StandardScaler

    bandwidths = parse_bandwidths(a.bandwidths)
    if not 0.0 < a.contamination <= 0.5:
        raise ValueError(f"--contamination ({a.contamination}) must be in (0, 0.5]")
    emb, truth = load(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], (None if truth is None else truth[:a.rows])
    if not 0 <= a.holdout < emb.shape[0] - 1:
        raise ValueError(f"--holdout ({a.holdout}) must leave at least 2 rows of {emb.shape[0]}")
    if a.by_class and truth is None:
        raise ValueError("--by-class needs labels in the embeddings file")
    n_fit = emb.shape[0] - a.holdout
    if a.pca < 0 or a.pca > min(n_fit, emb.shape[1]):
        raise ValueError(f"--pca ({a.pca}) must be in [0, min(rows, features) = {min(n_fit, emb.shape[1])}]")
    x = torch.from_numpy(emb[:n_fit]).to(a.device)
    x_hold = torch.from_numpy(emb[n_fit:]).to(a.device) if a.holdout else None
    if not a.no_scale:
        scaler = StandardScaler()
        x = scaler.fit_transform(x)
        if a.holdout:
            x_hold = scaler.transform(x_hold)
    explained = None
    if a.pca:
        pca = decomposition.PCA(a.pca)
        x = pca.fit_transform(x)
        explained = float(pca.explained_variance_ratio_.sum())
        if a.holdout:
            x_hold = pca.transform(x_hold)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    t0 = time.perf_counter()
    model = density.KernelDensity(bandwidths).fit(x)
    hs = np.atleast_1d(model.bandwidth_)
    loo = model.loo_score_samples()
    ll = loo.sum(axis=1)
    seconds = time.perf_counter() - t0
    chosen = int(np.argmax(ll))
    trials = [{"bandwidth": float(h), "loo_log_likelihood": float(ll[q]), "loo_mean_log_density": float(ll[q] / n_fit)}
              for q, h in enumerate(hs)]
    fit_truth = None if truth is None else truth[:n_fit]
    if a.by_class:
        clf = density.KDEClassifier(hs.tolist()).fit(x, fit_truth)
        pred = clf.loo_predict()
        known = fit_truth[clf.fit_rows_]
        for q in range(len(hs)):
            trials[q].update(loo_accuracy=float((pred[q] == known).mean()), loo_macro_f1=macro_f1(known, pred[q]))
    with open(out / "trials.csv", "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=list(trials[0]))
        w.writeheader()
        w.writerows(trials)

    log_density = loo[chosen]
    flagged_count = max(1, int(np.floor(a.contamination * n_fit)))
    flagged = np.argsort(log_density, kind="stable")[:flagged_count].astype(np.int64)
    threshold = float(log_density[flagged[-1]])
    np.save(out / "log_density.npy", log_density)
    np.save(out / "flagged.npy", flagged)

    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "scaled": not a.no_scale, "pca": a.pca, "pca_explained_variance_ratio": explained,
               "bandwidths": [float(h) for h in hs], "chosen_bandwidth": float(hs[chosen]), "chosen_at_an_end": bool(len(hs) > 1 and chosen in (0, len(hs) - 1)),
               "loo_log_likelihood": float(ll[chosen]), "contamination": a.contamination, "flagged": int(flagged_count), "threshold": threshold,
               "uniformity": density.uniformity(x, t=2.0), "seconds": seconds}
    if fit_truth is not None:
        summary["mean_log_density_per_class"] = {str(int(c)): float(log_density[fit_truth == c].mean()) for c in np.unique(fit_truth)}
        summary["flagged_per_class"] = {str(int(c)): int((fit_truth[flagged] == c).sum()) for c in np.unique(fit_truth)}
    for t in trials:
        extra = f", leave-one-out accuracy {t['loo_accuracy']:.4f}, macro F1 {t['loo_macro_f1']:.4f}" if a.by_class else ""
        print(f"h = {t['bandwidth']:.4g}: leave-one-out log-likelihood {t['loo_log_likelihood']:.6g} ({t['loo_mean_log_density']:.4f} per row){extra}")
    print(f"chosen h = {hs[chosen]:.4g}{' (an end of the list: widen it)' if summary['chosen_at_an_end'] else ''}; {flagged_count} rows flagged below "
          f"log density {threshold:.4f}; uniformity(t = 2) {summary['uniformity']:.4f}")

    if a.holdout:
        hold = (model if np.ndim(model.bandwidth_) == 0 else model[chosen]).score_samples(x_hold)
        np.save(out / "holdout_log_density.npy", hold)
        summary.update(holdout=int(a.holdout), holdout_below_threshold=int((hold < threshold).sum()))
        print(f"held-out rows: {a.holdout} scored as new rows, {summary['holdout_below_threshold']} below the threshold")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(hs)} bandwidths on {x.shape[0]} x {x.shape[1]} in {seconds:.2f} s (fit, leave-one-out pass and copies) -> {out}")
    return summary


if __name__ == "__main__":
    main()
