#!/usr/bin/env python3
"""PCA of dumped embeddings on MI355X (ssl_wafermap_amd.decomposition.PCA) with the rank diagnostics of the covariance
spectrum: the cheap linear reduction in front of the all-pairs kernels (HDBSCAN, KMeans, UMAP: their cost is linear in
the feature count), and the measurement of dimensional collapse of a self-supervised embedding.

    python scripts/embedding_pca_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --variance 0.95 --out pca_out
    python scripts/embedding_pca_amd.py --embeddings F --components 50 [--whiten] [--holdout K] --out DIR

--components N keeps N components, --variance V the smallest count whose cumulative variance ratio exceeds V; without
either all min(n, d) are kept.  --holdout K keeps the last K rows out of the fit, transforms them with the fitted model
and reports their reconstruction error next to the fitted rows'.

Outputs under --out: reduced.npz (`embeddings` float32 [n, m], all rows, the held-out ones last as in the input; `labels`)
-- what scripts/embedding_clustering_amd.py --embeddings ... --no-scale and scripts/embedding_kmeans_amd.py read --,
components.npy (float64 [m, d]), mean.npy (float64 [d]), spectrum.csv (eigenvalue, ratio, cumulative for all min(n, d)
eigenvalues) and summary.json: seconds per stage, n_components, effective_rank (exp of the spectrum's entropy),
participation_ratio, zero_variance_columns, the components needed for 90 / 95 / 99 % of the variance and the relative
reconstruction error |x - inverse_transform(transform(x))|_F / |x - mean|_F.
"""
from __future__ import annotations

import argparse
import csv
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


def components_for(ratio: np.ndarray, fraction: float) -> int:
    """The smallest count whose cumulative ratio exceeds `fraction` (the rule of PCA(n_components=fraction))."""
    return int(min(np.searchsorted(np.cumsum(ratio), fraction, side="right") + 1, ratio.size))


def relative_error(x, back, mean) -> float:
    """|x - back|_F / |x - mean|_F in float64 on the host (x, back: float32 device tensors)."""
    x64 = x.double().cpu().numpy()
    num = np.linalg.norm(x64 - back.double().cpu().numpy())
    den = np.linalg.norm(x64 - mean)
    return float(num / den) if den > 0 else 0.0


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--components", type=int, default=None)
    g.add_argument("--variance", type=float, default=None, help="a fraction in (0, 1)")
    ap.add_argument("--whiten", action="store_true")
    ap.add_argument("--holdout", type=int, default=0, help="keep the last K rows out of the fit and transform them")
    ap.add_argument("--out", default="pca_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import decomposition

    emb, truth = load_embeddings(a.embeddings)
    if not 0 <= a.holdout <= emb.shape[0] - 2:
        raise ValueError(f"--holdout ({a.holdout}) must leave at least 2 of the {emb.shape[0]} rows")
    n_fit = emb.shape[0] - a.holdout
    n_components = a.components if a.components is not None else a.variance
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    seconds = {}
    x, seconds["upload"] = timed(lambda: torch.from_numpy(emb[:n_fit]).to(a.device))
    model = decomposition.PCA(n_components, whiten=a.whiten)
    _, seconds["fit"] = timed(lambda: model.fit(x))
    y, seconds["transform"] = timed(lambda: model.transform(x))
    back, seconds["inverse_transform"] = timed(lambda: model.inverse_transform(y))
    reduced = y.cpu().numpy()

    spectrum = model.spectrum_
    total = spectrum.sum()
    ratio = spectrum / total if total > 0 else np.zeros_like(spectrum)
    with open(out / "spectrum.csv", "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(["eigenvalue", "ratio", "cumulative"])
        wr.writerows(zip(spectrum.tolist(), ratio.tolist(), np.cumsum(ratio).tolist()))
    summary = {
        "n": int(n_fit), "d": int(emb.shape[1]), "whiten": bool(a.whiten), "n_components": int(model.n_components_),
        "seconds": seconds,
        "explained_variance_ratio_kept": float(model.explained_variance_ratio_.sum()),
        "effective_rank": decomposition.effective_rank(spectrum),
        "participation_ratio": decomposition.participation_ratio(spectrum),
        "zero_variance_columns": int((np.diag(model.covariance_) == 0).sum()),
        "components_for_variance": {str(p): components_for(ratio, p / 100.0) for p in (90, 95, 99)},
        "relative_reconstruction_error": relative_error(x, back, model.mean_),
    }
    if a.holdout:
        x_hold = torch.from_numpy(emb[n_fit:]).to(a.device)
        y_hold, seconds["holdout_transform"] = timed(lambda: model.transform(x_hold))
        summary.update(holdout=int(a.holdout),
                       holdout_relative_reconstruction_error=relative_error(x_hold, model.inverse_transform(y_hold), model.mean_))
        reduced = np.concatenate([reduced, y_hold.cpu().numpy()])
    np.savez(out / "reduced.npz", embeddings=reduced.astype(np.float32), labels=truth)
    np.save(out / "components.npy", model.components_)
    np.save(out / "mean.npy", model.mean_)
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    cf = summary["components_for_variance"]
    print(f"{n_fit} x {emb.shape[1]} -> {model.n_components_} components ({100 * summary['explained_variance_ratio_kept']:.2f} % "
          f"of the variance) in {seconds['fit'] + seconds['transform']:.3f} s; effective rank {summary['effective_rank']:.2f}, "
          f"participation ratio {summary['participation_ratio']:.2f}, {summary['zero_variance_columns']} zero-variance columns, "
          f"components for 90 / 95 / 99 %: {cf['90']} / {cf['95']} / {cf['99']}; relative reconstruction error "
          f"{summary['relative_reconstruction_error']:.4g}"
          + (f" (held-out {a.holdout} rows: {summary['holdout_relative_reconstruction_error']:.4g})" if a.holdout else "")
          + f" -> {out}")
    return summary


if __name__ == "__main__":
    main()
