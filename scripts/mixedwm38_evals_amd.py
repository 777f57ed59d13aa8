#!/usr/bin/env python3
"""MixedWM38 downstream evaluation on MI355X: the reference's scripts/MixedWM38_evals.py -- linear_probe_ssl() (:905-940,
linear_probe() :740-870) and train_supervised() (:663-710) -- on the HIP path.  It produces the numbers of Table 1 of the
reference's report (reports/Mixed_Wafermaps.pdf): test AUC of a linear and a two-layer probe on frozen features of each
pretrained encoder, per label fraction, next to a supervised ResNet-18.

    python scripts/mixedwm38_evals_amd.py --ckpt BYOL=runs/BYOL/checkpoints/last.ckpt [--ckpt MAE=...]
                                          [--data-root /path/to/reference/data] [--max-epochs N] [--patience N]
                                          [--supervised-max-epochs N] [--no-supervised] [--out DIR]

What the reference does, and where it is here:
  :873-903  load_from_checkpoint per model                     -> --ckpt NAME=PATH, utils/checkpoint.load_checkpoint
  :905-940  predict val / test features (inference transforms) -> retrieval.embed_dataset (eval mode, batch 256)
  :752-775  predict the split's training features, StandardScaler fit on them -> retrieval.StandardScaler
  :807-810  pos_weight = negative / positive label frequency  -> models.pos_weight_from_labels
  :811-870  MultilabelLinearClassifier and TwoLayerMultilabelClassifier, batches of 1024, EarlyStopping(val_loss,
            patience 50), up to 1000 epochs, test with the last epoch's weights  -> models.fit_probe / evaluate_multilabel
  :663-710  SupervisedR18 per split: base transforms with denoise, batch 64, drop_last, Adam 1e-3, up to 100 epochs,
            EarlyStopping(patience 5)                          -> models.MultilabelSupervisedR18 + fit_probe
Outputs under --out: results.csv (model x split x probe: test_acc, test_auc, test_f1, epochs_run), one
history_<model>_<split>_<probe>.csv per run, and a printed table shaped like Table 1 (AUC x 100).

Data: `--data-root` = the reference's `data/` directory (processed/MixedWM38/train_{1,5,10,20}_split, val_data,
test_data pickles).  Without it the subset mode runs from the data-only fixture tests/golden/mixedwm38_train_1_split.npz
(381 maps with 8-bit labels), split deterministically into train / val / test (subset_split).
"""
from __future__ import annotations

import argparse
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FIXTURE = ROOT / "tests/golden/mixedwm38_train_1_split.npz"
REFERENCE_SPLITS = ["train_20_split", "train_10_split", "train_5_split", "train_1_split"]   # reference :655-660
PROBES = ("linear", "2layer")


def subset_split(labels: np.ndarray, seed: int = 0, fractions=(0.6, 0.2, 0.2)):
    """Deterministic train / val / test index arrays of the fixture's multi-label maps [N, L]: a seeded permutation cut by
    `fractions`, then, for every label without a positive in the training part, its first positive from val / test moves
    to train (the probes' pos_weight needs a positive of every label).  The parts are disjoint and cover all rows."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    order = np.random.default_rng(seed).permutation(n)
    a = int(round(fractions[0] * n))
    b = a + int(round(fractions[1] * n))
    train, val, test = list(order[:a]), list(order[a:b]), list(order[b:])
    for lab in range(labels.shape[1]):
        if labels[train, lab].any():
            continue
        for part in (val, test):
            hit = [i for i in part if labels[i, lab]]
            if hit:
                part.remove(hit[0])
                train.append(hit[0])
                break
        else:
            raise ValueError(f"subset_split: label {lab} has no positive sample at all")
    return np.array(sorted(train)), np.array(sorted(val)), np.array(sorted(test))


def load_data(data_root):
    """-> (train splits {name: (store, labels [N, 8])}, (val store, labels), (test store, labels))."""
    from ssl_wafermap_amd.data.store import WaferStore

    if data_root:
        import pandas as pd

        base = Path(data_root) / "processed/MixedWM38"

        def read(name):
            df = pd.read_pickle(base / f"{name}.pkl.xz")
            return WaferStore(df.waferMap.tolist()), np.vstack(df.label).astype(np.int64)

        return {name: read(name) for name in REFERENCE_SPLITS}, read("val_data"), read("test_data")
    store, _ = WaferStore.load(FIXTURE)
    with np.load(FIXTURE) as z:
        labels = z["multilabel"].astype(np.int64)
    tr, va, te = subset_split(labels)
    part = lambda idx: (store.subset(idx), labels[idx])   # noqa: E731
    return {"train_subset": part(tr)}, part(va), part(te)


def build_encoder(name: str, path: str, mae_backbone: str, dev):
    import ssl_wafermap_amd.models as zoo
    from ssl_wafermap_amd.utils.checkpoint import load_checkpoint

    kw = {}
    if name == "DINOViT":
        kw["batch_norm"] = False
    if name == "MAE":
        kw["backbone"] = mae_backbone
    if not hasattr(zoo, name):
        raise SystemExit(f"--ckpt {name}=...: no model class {name!r} in ssl_wafermap_amd.models")
    model = getattr(zoo, name)(None, 9, **kw)
    load_checkpoint(model, path)
    return model.to(dev).eval()


def print_table(rows, splits):
    """Table 1 shape: test AUC x 100, one line per model and probe, one column per training split."""
    import pandas as pd

    df = pd.DataFrame(rows)
    df["auc100"] = df["test_auc"] * 100
    table = df.pivot_table(index=["model", "probe"], columns="split", values="auc100", sort=False)
    table = table[[s for s in splits if s in table.columns]]
    print("\nMixedWM38 test AUC x 100 (rows: model / probe, columns: training split)")
    print(table.to_string(float_format=lambda v: f"{v:6.2f}"))
    return table


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", action="append", default=[], metavar="NAME=PATH",
                    help="pretrained model class and Lightning-layout checkpoint; repeatable")
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--max-epochs", type=int, default=1000, help="probe epochs at most (reference 1000)")
    ap.add_argument("--patience", type=int, default=50, help="probe early-stopping patience (reference 50)")
    ap.add_argument("--supervised-max-epochs", type=int, default=100)
    ap.add_argument("--supervised-patience", type=int, default=5)
    ap.add_argument("--no-supervised", action="store_true")
    ap.add_argument("--mae-backbone", default="vit_b_32", choices=["vit_b_32", "vit_small_16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import pandas as pd
    import torch

    from ssl_wafermap_amd import optim
    from ssl_wafermap_amd.data import WaferLoader, WaferMapDataset
    from ssl_wafermap_amd.models import (MultilabelLinearClassifier, MultilabelSupervisedR18, TwoLayerMultilabelClassifier,
                                         evaluate_multilabel, fit_probe, pos_weight_from_labels)
    from ssl_wafermap_amd.retrieval import StandardScaler, embed_dataset
    from ssl_wafermap_amd.transforms import BaseViewTransform, InferenceTransform

    # the reference filters torchmetrics' single-class AUROC warning (MixedWM38_evals.py:43,75)
    warnings.filterwarnings("ignore", message=".*only one class among the targets.*")
    ckpts = []
    for spec in args.ckpt:
        if "=" not in spec:
            raise SystemExit(f"--ckpt expects NAME=PATH, got {spec!r}")
        name, path = spec.split("=", 1)
        ckpts.append((name, path))
    dev = torch.device("cuda", 0)
    out = Path(args.out) if args.out else Path("mixedwm38_evals") / time.strftime("version_%Y%m%d_%H%M%S")
    out.mkdir(parents=True, exist_ok=True)
    splits, (val_store, val_y), (test_store, test_y) = load_data(args.data_root)
    val_y_t, test_y_t = torch.as_tensor(val_y, device=dev), torch.as_tensor(test_y, device=dev)

    def image_loader(store, y, transform, batch_size, shuffle=False, drop_last=False, seed=0):
        ds = WaferMapDataset(store, y, transform=transform, device=dev)
        return WaferLoader(ds, batch_size, shuffle=shuffle, drop_last=drop_last, seed=seed)

    def epochs_of(loader):
        def it(epoch):
            loader.set_epoch(epoch)
            return iter(loader)
        return it

    rows = []

    def record(model_name, split, probe, res, test):
        hist = pd.DataFrame(res["history"])
        hist.to_csv(out / f"history_{model_name}_{split}_{probe}.csv", index=False)
        row = {"model": model_name, "split": split, "probe": probe, **test, "epochs_run": res["epochs_run"]}
        rows.append(row)
        print(row, flush=True)
        pd.DataFrame(rows).to_csv(out / "results.csv", index=False)

    for model_name, path in ckpts:
        encoder = build_encoder(model_name, path, args.mae_backbone, dev)
        print(f"Loaded {model_name} from {path}", flush=True)
        feats = lambda store, y: embed_dataset(encoder, image_loader(store, y, InferenceTransform(), 256))  # noqa: E731
        val_f, test_f = feats(val_store, val_y), feats(test_store, test_y)
        for split, (store, y) in splits.items():
            train_f = feats(store, y)
            scaler = StandardScaler().fit(train_f)
            xtr, xva, xte = scaler.transform(train_f), scaler.transform(val_f), scaler.transform(test_f)
            ytr = torch.as_tensor(y, device=dev)
            pw = pos_weight_from_labels(y)
            for probe in PROBES:
                torch.manual_seed(args.seed)
                if probe == "linear":
                    clf = MultilabelLinearClassifier(xtr.shape[1], 8, pos_weight=pw).to(dev)
                    # the reference's MultilabelLinearClassifier trains with Adam at lr 1e-2 (evals.py:149-152); this
                    # package's class keeps lr 1e-3 in configure_optimizers, so the port builds the reference's optimiser
                    opt = optim.Adam(clf.parameters(), lr=1e-2)
                else:
                    clf = TwoLayerMultilabelClassifier(xtr.shape[1], 8, pos_weight=pw).to(dev)
                    opt = None
                res = fit_probe(clf, (xtr, ytr), (xva, val_y_t), max_epochs=args.max_epochs, patience=args.patience,
                                batch_size=1024, seed=args.seed, optimizer=opt)
                record(model_name, split, probe, res, evaluate_multilabel(clf, (xte, test_y_t)))
        del encoder
        torch.cuda.empty_cache()

    if not args.no_supervised:
        val_loader = image_loader(val_store, val_y, InferenceTransform(), 64)
        test_loader = image_loader(test_store, test_y, InferenceTransform(), 64)
        for split, (store, y) in splits.items():
            torch.manual_seed(args.seed)
            train_loader = image_loader(store, y, BaseViewTransform(denoise=True, n_views=1), 64, shuffle=True,
                                        drop_last=True, seed=args.seed)
            if len(train_loader) == 0:
                raise SystemExit(f"{split}: fewer than 64 training maps, no full supervised batch")
            model = MultilabelSupervisedR18(8, pos_weight=pos_weight_from_labels(y)).to(dev)
            res = fit_probe(model, epochs_of(train_loader), epochs_of(val_loader), max_epochs=args.supervised_max_epochs,
                            patience=args.supervised_patience, seed=args.seed, n_train=len(train_loader) * 64,
                            n_classes=8)
            record("SupervisedR18", split, "supervised", res, evaluate_multilabel(model, epochs_of(test_loader)))
            del model
            torch.cuda.empty_cache()

    if rows:
        print_table(rows, list(splits))
    return rows


if __name__ == "__main__":
    main()
