#!/usr/bin/env python3
"""Linear probe of dumped embeddings on MI355X as the convex problem it is
(ssl_wafermap_amd.linear_model.LogisticRegression / MultilabelLogisticRegression): a whole list of regularisation
strengths C in one solve, each to a gradient tolerance, so the number depends on the embedding and not on training knobs.

    python scripts/embedding_probe_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --C 1e-4:1:5
                                          [--class-weight balanced] [--holdout N | --val-frac F] [--multilabel]
                                          [--max-iter 1000] [--tol 1e-4] [--seed 0] [--rows N] [--no-scale] [--out DIR]

--C LO:HI:N is N log-spaced values from LO to HI (both ends; a single number is one C; a comma list is taken as given).
The held-out rows (--holdout N rows or --val-frac of them, drawn with --seed; default a fifth) take no part in the
scaler or the fit.  The rows are standardised (retrieval.StandardScaler; skipped with --no-scale) and the whole list is
fitted in one solve.  Per C the script reports train and held-out accuracy and macro F1 (models.knn.macro_metrics) --
with --multilabel (labels [n, L] of 0 / 1) accuracy, macro F1 and macro AUROC (models.evals.multilabel_metrics,
multilabel_auroc) -- and chooses the C of the best held-out accuracy (macro AUROC with --multilabel; the smallest such
C among equals).

Outputs under --out: trials.csv (one row per C), and for the chosen C coef.npy, intercept.npy, proba.npy (float64, the
held-out rows), confusion.npy (row-normalised, held-out; not with --multilabel) and summary.json (which also lists the
train and held-out row indices).
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

COLUMNS = ["C", "n_iter", "converged", "train_accuracy", "train_f1", "holdout_accuracy", "holdout_f1", "holdout_auroc"]


def parse_c(text: str) -> list:
    """"1e-4:1:5" -> 5 log-spaced values; "0.1" -> [0.1]; "0.01,0.1,1" -> as given."""
    if ":" in text:
        lo, hi, num = text.split(":")
        lo, hi, num = float(lo), float(hi), int(num)
        if not (0 < lo <= hi and num >= 1):
            raise ValueError(f"--C {text!r}: 0 < LO <= HI and N >= 1 expected")
        return [float(v) for v in (np.geomspace(lo, hi, num) if num > 1 else [lo])]
    return [float(v) for v in text.split(",")]


def load_rows(path, multilabel: bool):
    """(embeddings float32 [n, d], labels int64 [n] or [n, L])."""
    path = Path(path)
    if path.suffix == ".npz":
        z = np.load(path)
        emb, labels = z["embeddings"].astype(np.float32), np.asarray(z["labels"]).astype(np.int64)
    else:
        from scripts.embedding_kmeans_amd import load_embeddings

        emb, labels = load_embeddings(path)
    if labels.ndim != (2 if multilabel else 1) or labels.shape[0] != emb.shape[0]:
        raise ValueError(f"labels of shape {labels.shape} do not fit {'--multilabel' if multilabel else 'a single-label probe'}")
    return emb, labels


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--C", default="1e-4:1:5", help="LO:HI:N log-spaced, one number, or a comma list")
    ap.add_argument("--class-weight", choices=["none", "balanced"], default="none",
                    help="balanced: class weights (pos_weight with --multilabel) from the training rows")
    ap.add_argument("--holdout", type=int, default=0, help="hold N rows out")
    ap.add_argument("--val-frac", type=float, default=0.0, help="... or this fraction (default 0.2 when neither is given)")
    ap.add_argument("--multilabel", action="store_true")
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--out", default="probe_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import linear_model
    from ssl_wafermap_amd.models.evals import multilabel_auroc, multilabel_metrics
    from ssl_wafermap_amd.models.knn import macro_metrics
    from ssl_wafermap_amd.retrieval import StandardScaler

    cs = parse_c(a.C)
    emb, labels = load_rows(a.embeddings, a.multilabel)
    if a.rows:
        emb, labels = emb[:a.rows], labels[:a.rows]
    n = emb.shape[0]
    if a.holdout and a.val_frac:
        raise ValueError("--holdout and --val-frac exclude each other")
    n_hold = a.holdout if a.holdout else int(round((a.val_frac or 0.2) * n))
    if not 1 <= n_hold < n:
        raise ValueError(f"{n_hold} held-out rows of {n}: at least one row on each side expected")
    perm = np.random.default_rng(a.seed).permutation(n)
    hold_rows, train_rows = np.sort(perm[:n_hold]), np.sort(perm[n_hold:])
    x, x_hold = torch.from_numpy(emb[train_rows]).to(a.device), torch.from_numpy(emb[hold_rows]).to(a.device)
    y, y_hold = labels[train_rows], labels[hold_rows]
    if not a.no_scale:
        scaler = StandardScaler()
        x, x_hold = scaler.fit_transform(x), scaler.transform(x_hold)
    balanced = a.class_weight == "balanced"
    if a.multilabel:
        model = linear_model.MultilabelLogisticRegression(cs, pos_weight="balanced" if balanced else None, tol=a.tol,
                                                          max_iter=a.max_iter)
    else:
        model = linear_model.LogisticRegression(cs, class_weight="balanced" if balanced else None, tol=a.tol, max_iter=a.max_iter)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a problem that ran out of iterations says so in the `converged` column)
        model.fit(x, y)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0

    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    table, scores = [], []
    for i, c in enumerate(cs):
        one = model[i]
        row = {"C": repr(c), "n_iter": int(np.max(one.n_iter_)), "converged": int(np.all(one.converged_))}
        if a.multilabel:
            for name, rows_x, rows_y in (("train", x, y), ("holdout", x_hold, y_hold)):
                logits, target = one.decision_function(rows_x).float(), torch.from_numpy(rows_y).to(a.device)
                acc, f1 = multilabel_metrics(logits, target)
                row[f"{name}_accuracy"], row[f"{name}_f1"] = acc, f1
                if name == "holdout":
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")  # (a label without positives among the held-out rows counts as 0)
                        row["holdout_auroc"] = multilabel_auroc(logits, target)
            scores.append(row["holdout_auroc"])
        else:
            k = int(one.classes_.size)
            for name, rows_x, rows_y in (("train", x, y), ("holdout", x_hold, y_hold)):
                known = np.isin(rows_y, one.classes_)  # (a held-out class the training rows never showed cannot be scored)
                pred = np.searchsorted(one.classes_, one.predict(rows_x)[known])
                truth = np.searchsorted(one.classes_, rows_y[known])
                _, f1, _ = macro_metrics(torch.from_numpy(pred), torch.from_numpy(truth), k)
                row[f"{name}_accuracy"], row[f"{name}_f1"] = float((pred == truth).mean()), f1
            row["holdout_auroc"] = ""
            scores.append(row["holdout_accuracy"])
        table.append(row)
    with open(out / "trials.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=COLUMNS)
        wr.writeheader()
        wr.writerows(table)

    chosen = int(np.argmax(scores))
    best = model.best(scores)
    proba = best.predict_proba(x_hold).cpu().numpy()
    np.save(out / "coef.npy", best.coef_)
    np.save(out / "intercept.npy", best.intercept_)
    np.save(out / "proba.npy", proba)
    summary = {"embeddings": str(a.embeddings), "n_train": int(len(train_rows)), "n_holdout": int(n_hold), "d": int(emb.shape[1]),
               "multilabel": bool(a.multilabel), "class_weight": a.class_weight, "C": cs, "chosen_C": cs[chosen],
               "chosen_index": chosen, "fit_seconds": seconds, "tol": a.tol, "max_iter": a.max_iter,
               "holdout_accuracy": table[chosen]["holdout_accuracy"], "holdout_f1": table[chosen]["holdout_f1"],
               "train_accuracy": table[chosen]["train_accuracy"], "converged": bool(table[chosen]["converged"]),
               "train_rows": train_rows.tolist(), "holdout_rows": hold_rows.tolist()}
    if a.multilabel:
        summary["holdout_auroc"] = table[chosen]["holdout_auroc"]
    else:
        known = np.isin(y_hold, best.classes_)
        pred = np.searchsorted(best.classes_, best.predict(x_hold)[known])
        truth = np.searchsorted(best.classes_, y_hold[known])
        _, _, cm = macro_metrics(torch.from_numpy(pred), torch.from_numpy(truth), int(best.classes_.size))
        np.save(out / "confusion.npy", cm.numpy())
        summary["classes"] = best.classes_.tolist()
    with open(out / "summary.json", "w") as fh:
        json.dump(summary, fh, indent=1)

    print(f"{len(train_rows)} training rows x {emb.shape[1]} features, {len(cs)} values of C in one solve: {seconds:.2f} s")
    print(f"{'C':>10} {'iter':>6} {'conv':>5} {'train acc':>10} {'train F1':>9} {'held-out acc':>13} {'held-out F1':>12}"
          + (f" {'held-out AUROC':>15}" if a.multilabel else ""))
    for row in table:
        print(f"{float(row['C']):>10.3g} {row['n_iter']:>6} {row['converged']:>5} {row['train_accuracy']:>10.4f} "
              f"{row['train_f1']:>9.4f} {row['holdout_accuracy']:>13.4f} {row['holdout_f1']:>12.4f}"
              + (f" {row['holdout_auroc']:>15.4f}" if a.multilabel else ""))
    print(f"chosen by the held-out rows: C = {cs[chosen]:g} -> {out}/")
    return summary


if __name__ == "__main__":
    main()
