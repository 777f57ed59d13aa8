#!/usr/bin/env python3
"""Gaussian-mixture sweep over the number of components on dumped embeddings on MI355X
(ssl_wafermap_amd.mixture.GaussianMixture): a per-wafer likelihood, soft assignments with elliptical clusters, and BIC /
AIC as the choice of the cluster count that scripts/embedding_kmeans_amd.py makes by silhouette.

    python scripts/embedding_gmm_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --k 25:50 [--pca 50]
                                        [--covariance-type full|diag|spherical] [--n-init 1] [--seed 0]
                                        [--no-scale] [--rows N] [--holdout N] [--out DIR]

It standardises the rows (retrieval.StandardScaler; skipped with --no-scale), reduces them to --pca dimensions
(decomposition.PCA; 0: no reduction; a full-covariance mixture takes at most 256 features), fits every k of --k LO:HI
(both ends; a single number is one k) and scores the hard labels of each fit with the scores of the other sweeps:
silhouette, Calinski-Harabasz, Davies-Bouldin and homogeneity against the failure codes.

Outputs under --out: trials.csv (k, lower bound, BIC, AIC, n_iter, converged, the four scores, seconds), and for the
model of the lowest BIC (the lowest k among equals) labels.npy (int64 [n]), proba.npy (float64 [n, k]),
score_samples.npy (float64 [n]), weights.npy, means.npy, covariances.npy (in the scaled, reduced space) and summary.json.

--holdout N keeps the last N rows out of the scaler, the PCA and the fits and asks the chosen model about them:
holdout_labels.npy, holdout_score_samples.npy, and in summary.json `holdout`, `holdout_score` and
`holdout_homogeneity`.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from scripts.embedding_kmeans_amd import load_embeddings, parse_k  # noqa: E402

COLUMNS = ["k", "lower_bound", "bic", "aic", "n_iter", "converged", "homogeneity", "silhouette", "calinski_harabasz",
           "davies_bouldin", "seconds"]


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--k", default="25:50", help="LO:HI, both ends, or one number")
    ap.add_argument("--pca", type=int, default=50, help="reduce to this many dimensions first (0: no reduction)")
    ap.add_argument("--covariance-type", choices=["full", "diag", "spherical"], default="full")
    ap.add_argument("--n-init", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last N rows out of the fits and score them")
    ap.add_argument("--out", default="gmm_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import cluster, decomposition, mixture
    from ssl_wafermap_amd.retrieval import StandardScaler

    ks = parse_k(a.k)
    emb, truth = load_embeddings(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], truth[:a.rows]
    if not 0 <= a.holdout < emb.shape[0]:
        raise ValueError(f"--holdout ({a.holdout}) must be in [0, rows = {emb.shape[0]})")
    n_fit = emb.shape[0] - a.holdout
    if ks[-1] > n_fit - 1:
        raise ValueError(f"--k up to {ks[-1]} needs more than {n_fit} rows")
    if a.pca < 0 or a.pca > min(n_fit, emb.shape[1]):
        raise ValueError(f"--pca ({a.pca}) must be in [0, min(rows, features) = {min(n_fit, emb.shape[1])}]")
    x, x_hold = torch.from_numpy(emb[:n_fit]).to(a.device), None
    if a.holdout:
        x_hold, truth_hold, truth = torch.from_numpy(emb[n_fit:]).to(a.device), truth[n_fit:], truth[:n_fit]
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

    rows, models = [], {}
    t_all = time.perf_counter()
    for k in ks:
        t0 = time.perf_counter()
        model = mixture.GaussianMixture(k, covariance_type=a.covariance_type, n_init=a.n_init,
                                        random_state=a.seed + k)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (a fit that ran out of iterations says so in the `converged` column)
            labels = model.fit_predict(x)
        bic, aic = model.bic(x), model.aic(x)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        several = len(np.unique(labels)) > 1
        rows.append({"k": k, "lower_bound": model.lower_bound_, "bic": bic, "aic": aic, "n_iter": model.n_iter_,
                     "converged": int(model.converged_), "homogeneity": cluster.homogeneity_score(truth, labels),
                     "silhouette": cluster.silhouette_score(x, labels) if several else float("nan"),
                     "calinski_harabasz": cluster.calinski_harabasz_score(x, labels) if several else float("nan"),
                     "davies_bouldin": cluster.davies_bouldin_score(x, labels) if several else float("nan"),
                     "seconds": seconds})
        models[k] = (model, labels)
    wall = time.perf_counter() - t_all
    with open(out / "trials.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=COLUMNS)
        wr.writeheader()
        wr.writerows(rows)
    best = min(rows, key=lambda r: (r["bic"], r["k"]))
    model, labels = models[best["k"]]
    np.save(out / "labels.npy", labels.astype(np.int64))
    np.save(out / "proba.npy", model.predict_proba(x).cpu().numpy())
    np.save(out / "score_samples.npy", model.score_samples(x).cpu().numpy())
    np.save(out / "weights.npy", model.weights_)
    np.save(out / "means.npy", model.means_)
    np.save(out / "covariances.npy", model.covariances_)
    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "k": [ks[0], ks[-1]], "covariance_type": a.covariance_type,
               "n_init": a.n_init, "pca": a.pca, "pca_explained_variance_ratio": explained, "sweep_seconds": wall,
               "fit_seconds": float(sum(r["seconds"] for r in rows)), "chosen_k": best["k"],
               "chosen": {c: best[c] for c in COLUMNS}, "chosen_by_aic": min(rows, key=lambda r: (r["aic"], r["k"]))["k"],
               "cluster_sizes": np.bincount(labels, minlength=best["k"]).tolist()}
    print(f"chosen k = {best['k']} (lowest BIC): {best}")
    if a.holdout:
        h_labels = model.predict(x_hold)
        h_scores = model.score_samples(x_hold).cpu().numpy()
        np.save(out / "holdout_labels.npy", h_labels.astype(np.int64))
        np.save(out / "holdout_score_samples.npy", h_scores)
        summary.update(holdout=int(a.holdout), holdout_score=float(h_scores.mean()),
                       holdout_homogeneity=cluster.homogeneity_score(truth_hold, h_labels))
        print(f"held-out rows: {a.holdout}; mean log-likelihood {summary['holdout_score']:.4f} "
              f"(fitted rows: {best['lower_bound']:.4f}); homogeneity {summary['holdout_homogeneity']:.4f}")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(ks)} values of k x {a.n_init} initialisations on {x.shape[0]} x {x.shape[1]} ({a.covariance_type}) in "
          f"{wall:.2f} s -> {out}")
    return summary


if __name__ == "__main__":
    main()
