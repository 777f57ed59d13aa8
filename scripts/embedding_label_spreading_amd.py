#!/usr/bin/env python3
"""Label spreading over the kNN graph of dumped embeddings on MI355X (ssl_wafermap_amd.semi_supervised.LabelSpreading):
a few known failure codes pushed through the neighbourhood structure of ALL rows, labelled and unlabelled -- the
`sklearn.semi_supervised` step after the reference's notebooks 3.0 and 3.2 (`fit(x, y=labels with -1)`), next to the
existing kNN vote, which looks at the labelled rows only.

    python scripts/embedding_label_spreading_amd.py --embeddings tests/golden/simsiam_preds_subset.npz --label-frac 0.1
                                                    --alpha 0.2,0.5,0.8,0.95 --neighbors 15 [--max-iter 200] [--tol 1e-3]
                                                    [--affinity connectivity|fuzzy] [--seed 0] [--no-scale] [--rows N]
                                                    [--holdout N] [--out DIR]

It standardises the rows (retrieval.StandardScaler; skipped with --no-scale), hides all but --label-frac of the labels
with a seeded draw, and fits every alpha of --alpha in ONE pass (the alphas share every gather of the graph).  Per alpha:
the number of steps, the accuracy on the hidden rows, the number of rows no label reached (graph components without a
labelled row), and beside them the accuracy of the weighted kNN vote (utils.benchmarking.knn_predict, k = --neighbors,
t = 0.1, L2-normalised rows) of the labelled rows on the same hidden rows.

Outputs under --out: trials.csv (one row per alpha), and for the chosen alpha (the best hidden-row accuracy, the lowest
alpha among equals) labels.npy (int64 [n], -1 for unreached rows), proba.npy (float64 [n, classes]) and summary.json.

--holdout N keeps N rows, drawn with the seed (dumps are often sorted by failure code, so not the last N), out of the scaler
and the fit and asks the chosen model about them (LabelSpreading.predict_proba): holdout_rows.npy, holdout_proba.npy, and in
summary.json `holdout` and `holdout_accuracy`.
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

from scripts.embedding_kmeans_amd import load_embeddings  # noqa: E402

COLUMNS = ["alpha", "n_iter", "accuracy_hidden", "unreached", "accuracy_hidden_reached", "knn_vote_accuracy_hidden"]


def parse_alphas(text: str):
    alphas = [float(t) for t in text.split(",") if t.strip()]
    if not alphas or not all(0.0 < a < 1.0 for a in alphas):
        raise ValueError(f"--alpha {text!r}: numbers in (0, 1), separated by commas, expected")
    return alphas


def hide_labels(truth: np.ndarray, frac: float, seed: int) -> np.ndarray:
    """The labels with -1 on the rows a seeded draw hides: each row keeps its label with probability `frac`."""
    if not 0.0 < frac <= 1.0:
        raise ValueError(f"--label-frac ({frac}) must be in (0, 1]")
    keep = np.random.default_rng(seed).random(truth.shape[0]) < frac
    return np.where(keep, truth, -1).astype(np.int64)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--embeddings", required=True)
    ap.add_argument("--label-frac", type=float, default=0.1)
    ap.add_argument("--alpha", default="0.2,0.5,0.8,0.95")
    ap.add_argument("--neighbors", type=int, default=15)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--affinity", choices=["connectivity", "fuzzy"], default="connectivity")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only")
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--holdout", type=int, default=0, help="keep N rows (a seeded draw) out of the fit and predict them")
    ap.add_argument("--out", default="label_spreading_out")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import functional as F_hip
    from ssl_wafermap_amd.retrieval import StandardScaler
    from ssl_wafermap_amd.semi_supervised import LabelSpreading
    from ssl_wafermap_amd.utils.benchmarking import knn_predict

    alphas = parse_alphas(a.alpha)
    emb, truth = load_embeddings(a.embeddings)
    if a.rows:
        emb, truth = emb[:a.rows], truth[:a.rows]
    if not 0 <= a.holdout < emb.shape[0]:
        raise ValueError(f"--holdout ({a.holdout}) must be in [0, rows = {emb.shape[0]})")
    n_fit = emb.shape[0] - a.holdout
    if a.holdout:  # the held-out rows go to the end, the others keep their order
        held = np.sort(np.random.default_rng(a.seed + 1).choice(emb.shape[0], a.holdout, replace=False))
        order = np.concatenate([np.setdiff1d(np.arange(emb.shape[0]), held), held])
        emb, truth = emb[order], truth[order]
    x, x_hold = torch.from_numpy(emb[:n_fit]).to(a.device), None
    if a.holdout:
        x_hold, truth_hold, truth = torch.from_numpy(emb[n_fit:]).to(a.device), truth[n_fit:], truth[:n_fit]
    if not a.no_scale:
        scaler = StandardScaler()
        x = scaler.fit_transform(x)
        if a.holdout:
            x_hold = scaler.transform(x_hold)
    y = hide_labels(truth, a.label_frac, a.seed)
    hidden = y < 0
    if hidden.all() or not hidden.any():
        raise ValueError("the draw must leave some rows labelled and some hidden")
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    t0 = time.perf_counter()
    model = LabelSpreading(n_neighbors=a.neighbors, alpha=alphas, max_iter=a.max_iter, tol=a.tol, affinity=a.affinity).fit(x, y)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0

    # the existing vote among the labelled rows only, on the same hidden rows
    classes = model.classes_
    codes = torch.from_numpy(np.searchsorted(classes, y[~hidden])).to(a.device)
    unit = F_hip.l2_normalize(x.contiguous(), out_dtype=torch.float32)
    bank = unit[torch.from_numpy(~hidden).to(a.device)].contiguous()
    k = min(a.neighbors, bank.shape[0])
    vote = knn_predict(unit[torch.from_numpy(hidden).to(a.device)].contiguous(), bank.t(), codes, len(classes), k, 0.1)[:, 0]
    knn_acc = float((classes[vote.cpu().numpy()] == truth[hidden]).mean())

    rows = []
    for g, alpha in enumerate(alphas):
        labels, unreached = model.transduction_[g], model.unreached_[g]
        ok = labels == truth
        rows.append({"alpha": alpha, "n_iter": int(model.n_iter_[g]), "accuracy_hidden": float(ok[hidden].mean()),
                     "unreached": int(unreached.sum()),
                     "accuracy_hidden_reached": float(ok[hidden & ~unreached].mean()) if (hidden & ~unreached).any() else float("nan"),
                     "knn_vote_accuracy_hidden": knn_acc})
    with open(out / "trials.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=COLUMNS)
        wr.writeheader()
        wr.writerows(rows)
    best = max(range(len(rows)), key=lambda g: (rows[g]["accuracy_hidden"], -rows[g]["alpha"]))
    labels = np.where(model.unreached_[best], -1, model.transduction_[best]).astype(np.int64)
    np.save(out / "labels.npy", labels)
    np.save(out / "proba.npy", model.label_distributions_[best])
    summary = {"n": int(x.shape[0]), "d": int(x.shape[1]), "neighbors": a.neighbors, "affinity": a.affinity, "label_frac": a.label_frac,
               "labelled": int((~hidden).sum()), "hidden": int(hidden.sum()), "classes": classes.tolist(), "alphas": alphas,
               "fit_seconds": seconds, "chosen_alpha": alphas[best], "chosen": rows[best], "trials": rows,
               "knn_vote_accuracy_hidden": knn_acc}
    for r in rows:
        print(r)
    print(f"chosen alpha = {alphas[best]}: hidden-row accuracy {rows[best]['accuracy_hidden']:.4f} (kNN vote of the labelled rows: "
          f"{knn_acc:.4f}), {rows[best]['unreached']} rows unreached")
    if a.holdout:
        proba = model.predict_proba(x_hold)[best]
        np.save(out / "holdout_proba.npy", proba)
        np.save(out / "holdout_rows.npy", held)
        reached = proba.sum(axis=1) > 0
        pred = classes[np.argmax(proba, axis=1)]
        summary.update(holdout=int(a.holdout), holdout_unreached=int((~reached).sum()), holdout_accuracy=float((pred == truth_hold).mean()))
        print(f"held-out rows: {a.holdout}, accuracy {summary['holdout_accuracy']:.4f}, {summary['holdout_unreached']} with only "
              f"unreached neighbours")
    (out / "summary.json").write_text(json.dumps(summary, indent=1))
    print(f"{len(alphas)} alphas on {x.shape[0]} x {x.shape[1]} in {seconds:.2f} s (graph, fit and copies) -> {out}")
    return summary


if __name__ == "__main__":
    main()
