"""Supervised baseline and linear probes: the reference's SupervisedR18 (scripts/WM811k_benchmark.py:202-225)
and LinearClassifier / MultilabelLinearClassifier (src/ssl_wafermap/models/evals.py:14-165; drivers
scripts/WM811k_linear_probe.py:286-385, scripts/MixedWM38_evals.py:740-870) — SURVEY 8f.4.

The probes train one Linear layer on frozen features (e.g. `retrieval.embed_dataset` output) with Adam;
`fit_linear_probe` is the loop Lightning's Trainer runs for them: epochs over shuffled mini-batches, then
macro accuracy / F1 (multi-class) or per-label accuracy / macro F1 at threshold 0 (multi-label).

The MixedWM38 evaluation (scripts/MixedWM38_evals.py; Table 1 of the reference's report) adds the two-layer probe
(TwoLayerMultilabelClassifier), the multi-label supervised ResNet-18 (MultilabelSupervisedR18), the AUROC its table
reports (multilabel_auroc, csrc/evalops.hip) and `fit_probe`: Lightning's fit / validate / EarlyStopping / test
sequence of those scripts, with per-epoch train and validation metrics.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import nn as hnn
from .. import optim
from ..loss import BCEWithLogitsLoss, CrossEntropyLoss
from ..evalops import multilabel_auroc_per_label
from ..utils import debug
from .knn import KNNBenchmarkModule, macro_metrics
from .resnet import ResNet18, create_model


class SupervisedR18(KNNBenchmarkModule):
    def __init__(self, dataloader_kNN=None, num_classes=9, log_rep_std: bool = True, **kwargs):
        kwargs.pop("batch_size", None)
        kwargs.pop("max_epochs", None)
        super().__init__(dataloader_kNN, num_classes, **kwargs)
        self.backbone = create_model("resnet18", num_classes=0, pretrained=False)
        self.fc = hnn.Linear(self.backbone.num_features, num_classes, bias=True)
        self.criterion = CrossEntropyLoss()
        self.log_rep_std = log_rep_std

    def forward(self, x):
        """Class logits (the reference returns their log-softmax and applies nll_loss: the same loss)."""
        f = self.backbone(x).flatten(start_dim=1)
        if self.log_rep_std:
            self.log("rep_std", debug.std_of_l2_normalized(f.detach()))
        return self.fc(f)

    def training_step(self, batch, batch_idx):
        x, y = batch
        if isinstance(x, (list, tuple)):
            x = x[0]
        loss = self.criterion(self.forward(x), y)
        self.log("train_loss", loss)
        return loss

    def configure_optimizers(self):
        return [optim.AdamW(self.parameters())], []  # torch.optim.AdamW defaults: lr 1e-3, wd 1e-2


class LinearClassifier(nn.Module):
    def __init__(self, num_features: int, num_classes: int = 9, weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.model = hnn.Linear(num_features, num_classes, bias=True)
        self.criterion = CrossEntropyLoss(weight=weight)
        self.num_classes = num_classes

    def forward(self, x):
        return self.model(x)

    def training_step(self, batch, batch_idx):
        x, y = batch
        return self.criterion(self(x), y)

    def configure_optimizers(self):
        return optim.AdamW(self.parameters(), lr=1e-3, weight_decay=0.0)  # == torch.optim.Adam(lr=1e-3)

    @torch.no_grad()
    def evaluate(self, x, y):
        pred = self(x).float().argmax(dim=1)
        acc, f1, cm = macro_metrics(pred, y, self.num_classes)
        return {"acc": acc, "f1": f1, "confusion_matrix": cm}


class MultilabelLinearClassifier(nn.Module):
    def __init__(self, num_features: int, num_classes: int = 8, pos_weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.model = hnn.Linear(num_features, num_classes, bias=True)
        self.criterion = BCEWithLogitsLoss(pos_weight=pos_weight)
        self.num_classes = num_classes

    def forward(self, x):
        return self.model(x)

    def training_step(self, batch, batch_idx):
        x, y = batch
        return self.criterion(self(x), y.float())

    def configure_optimizers(self):
        return optim.AdamW(self.parameters(), lr=1e-3, weight_decay=0.0)

    @torch.no_grad()
    def evaluate(self, x, y):
        acc, f1 = multilabel_metrics(self(x), y)
        return {"acc": acc, "f1": f1}


def fit_linear_probe(model: nn.Module, features: torch.Tensor, labels: torch.Tensor, epochs: int = 10,
                     batch_size: int = 256, seed: int = 0):
    """Train a (Multilabel)LinearClassifier on frozen features [N, D] (any float dtype, on the GPU)."""
    opt = model.configure_optimizers()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n = features.shape[0]
    feats = features.to(torch.bfloat16).contiguous()
    losses = []
    for _ in range(epochs):
        perm = torch.randperm(n, generator=gen).to(features.device)
        total, steps = 0.0, 0
        for s in range(0, n, batch_size):
            idx = perm[s:s + batch_size]
            opt.zero_grad()
            loss = model.training_step((feats[idx], labels[idx]), steps)
            loss.backward()
            opt.step()
            total += float(loss.detach())
            steps += 1
        losses.append(total / max(steps, 1))
    return losses


# ------------------------------------------------------------------------------------ MixedWM38 evaluation
def multilabel_metrics(logits: torch.Tensor, targets: torch.Tensor) -> Tuple[float, float]:
    """MultilabelAccuracy and MultilabelF1Score (macro) of torchmetrics at threshold 0.5 on the sigmoid, i.e. logit > 0:
    (mean per-label accuracy, mean per-label F1 with F1 = 0 for a label without positives and predictions)."""
    pred = (logits.float() > 0).long()
    y = targets.long()
    tp = (pred & y).sum(0).double()
    fp = (pred & (1 - y)).sum(0).double()
    fn = ((1 - pred) & y).sum(0).double()
    f1 = torch.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp_min(1), torch.zeros_like(tp))
    return float((pred == y).double().mean()), float(f1.mean())


def multilabel_auroc(logits: torch.Tensor, targets: torch.Tensor, average: Optional[str] = "macro"):
    """torchmetrics MultilabelAUROC(num_labels, average, thresholds=None) on the device (csrc/evalops.hip): exact
    rank statistic per label; logits outside [0, 1] are ranked by their float32 sigmoid.  average="macro": the mean of
    the per-label values (a label without positives or negatives counts as 0, with a warning, as in torchmetrics);
    None: the per-label float64 tensor."""
    if average not in ("macro", None):
        raise ValueError(f"multilabel_auroc: average must be 'macro' or None, got {average!r}")
    auc, _ = multilabel_auroc_per_label(logits, targets)
    return float(auc.mean()) if average == "macro" else auc


def pos_weight_from_labels(labels) -> torch.Tensor:
    """BCEWithLogitsLoss pos_weight = negative frequency / positive frequency per label of the training labels [N, L]
    (scripts/MixedWM38_evals.py:807-810, :667-670).  A label without positives raises instead of giving an infinite
    weight."""
    y = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels, dtype=np.float64)
    if y.ndim != 2 or y.shape[0] == 0:
        raise ValueError(f"pos_weight_from_labels: expected [samples, labels], got shape {y.shape}")
    pos = y.sum(axis=0) / y.shape[0]
    missing = np.flatnonzero(pos == 0)
    if missing.size:
        raise ValueError(f"pos_weight_from_labels: label(s) {missing.tolist()} have no positive training sample; "
                         "the weight would be infinite")
    return torch.tensor((1.0 - pos) / pos, dtype=torch.float32)


class EarlyStopping:
    """Lightning's EarlyStopping(monitor="val_loss", mode="min", min_delta=0, patience, check_finite=True) as a pure
    rule: `step(value)` returns True when training should stop.  An improvement is a strictly smaller value (a tie
    is not one); after `patience` epochs in a row without one, or on a non-finite value, it stops."""

    def __init__(self, patience: int, min_delta: float = 0.0):
        if patience < 0:
            raise ValueError("patience must be >= 0")
        self.patience, self.min_delta = int(patience), abs(float(min_delta))
        self.best = math.inf
        self.wait = 0
        self.stopped = False

    def step(self, value: float) -> bool:
        value = float(value)
        if not math.isfinite(value):
            self.stopped = True
        elif value < self.best - self.min_delta:
            self.best, self.wait = value, 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped = True
        return self.stopped


class TwoLayerMultilabelClassifier(MultilabelLinearClassifier):
    """Reference evals.py:155-165: Linear(F, 256) -> Mish -> Dropout(0.5) -> Linear(256, C), state_dict keys
    model.0.* / model.3.* as there.  Adam at lr 1e-2: the reference's MultilabelLinearClassifier.configure_optimizers,
    which this class inherits there (evals.py:149-152)."""

    def __init__(self, num_features: int, num_classes: int = 8, pos_weight: Optional[torch.Tensor] = None):
        super().__init__(num_features, num_classes, pos_weight)
        self.model = nn.Sequential(hnn.Linear(num_features, 256, bias=True), hnn.Mish(), hnn.Dropout(p=0.5),
                                   hnn.Linear(256, num_classes, bias=True))

    def configure_optimizers(self):
        return optim.Adam(self.parameters(), lr=1e-2)


class _ResNet18Classifier(ResNet18):
    """timm.create_model("resnet18", num_classes=C): the backbone plus `fc` (keys conv1.* ... fc.weight / fc.bias)."""

    def __init__(self, num_classes: int):
        super().__init__(0)
        self.fc = hnn.Linear(self.num_features, num_classes, bias=True)

    def forward(self, x):
        return self.fc(super().forward(x).flatten(start_dim=1))


class MultilabelSupervisedR18(nn.Module):
    """The multi-label supervised baseline of the MixedWM38 table (scripts/MixedWM38_evals.py SupervisedR18, :93-166):
    `model` = ResNet-18 with C outputs trained with BCEWithLogitsLoss(pos_weight), Adam lr 1e-3; `backbone` = a
    separate headless ResNet-18 used only by predict_step, as in the reference (state_dict keys backbone.* / model.*)."""

    def __init__(self, num_classes: int = 8, pos_weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.backbone = create_model("resnet18", num_classes=0, pretrained=False)
        self.model = _ResNet18Classifier(num_classes)
        self.criterion = BCEWithLogitsLoss(pos_weight=pos_weight)
        self.num_classes = num_classes

    def forward(self, x):
        return self.model(x)

    def training_step(self, batch, batch_idx):
        x, y = batch
        return self.criterion(self(x), y.float())

    def predict_step(self, batch, batch_idx):
        images, _ = batch
        return self.backbone(images)

    def configure_optimizers(self):
        return optim.Adam(self.parameters(), lr=1e-3)


Batches = Union[Tuple[torch.Tensor, torch.Tensor], Callable[[int], Iterable]]


def _tensor_batches(x: torch.Tensor, y: torch.Tensor, batch_size: int, gen: Optional[torch.Generator]):
    """DataLoader(TensorDataset(x, y), batch_size, shuffle=gen is not None, drop_last=False) as a per-epoch iterator."""
    def it(epoch):
        n = x.shape[0]
        order = torch.randperm(n, generator=gen).to(x.device) if gen is not None else None
        for s in range(0, n, batch_size):
            if order is None:
                yield x[s:s + batch_size], y[s:s + batch_size]
            else:
                idx = order[s:s + batch_size]
                yield x[idx], y[idx]
    return it


def _as_batches(data: Batches, batch_size: int, gen: Optional[torch.Generator], bf16: bool):
    if callable(data):
        return data, None
    x, y = data
    if bf16:
        x = x.to(torch.bfloat16).contiguous()
    return _tensor_batches(x, y, batch_size, gen), x.shape[0]


@torch.no_grad()
def predict_logits(model: nn.Module, data: Batches, batch_size: int = 1024) -> Tuple[torch.Tensor, torch.Tensor]:
    """(logits float32 [N, C], targets [N, C]) of an eval-mode pass over `data` (an (x, y) pair or an epoch -> batches
    callable); the model's mode is restored."""
    was = model.training
    model.eval()
    it, _ = _as_batches(data, batch_size, None, True)
    outs, ys = [], []
    for xb, yb in it(0):
        outs.append(model(xb).float())
        ys.append(yb)
    model.train(was)
    return torch.cat(outs), torch.cat(ys)


def evaluate_multilabel(model: nn.Module, data: Batches, batch_size: int = 1024) -> Dict[str, float]:
    """test_acc / test_auc / test_f1 of the reference's test_step (evals.py:133-144) on `data`."""
    logits, y = predict_logits(model, data, batch_size)
    acc, f1 = multilabel_metrics(logits, y)
    return {"test_acc": acc, "test_auc": multilabel_auroc(logits, y), "test_f1": f1}


def fit_probe(model: nn.Module, train: Batches, val: Batches, max_epochs: int = 1000, patience: int = 50,
              batch_size: int = 1024, seed: int = 0, optimizer=None, n_train: Optional[int] = None,
              n_classes: Optional[int] = None) -> Dict[str, object]:
    """Lightning's `Trainer(max_epochs, callbacks=[EarlyStopping("val_loss", patience)]).fit(model, train, val)` for the
    multi-label probes and the supervised baseline (scripts/MixedWM38_evals.py:800-870, :663-710).

    `train` / `val`: (x, y) device tensors -- mini-batches of `batch_size`, shuffled each epoch from a CPU generator
    seeded with `seed` (train) and in order (val), the last one short -- or callables epoch -> iterable of (x, y)
    batches (image loaders; then pass `n_train`, the samples per training epoch, and `n_classes`).  The optimiser is
    `model.configure_optimizers()` unless given.  Per epoch: train() over the training batches, collecting every
    step's logits in a preallocated buffer; eval() over the validation set; history gets train / val loss (batch-size
    weighted means, as Lightning logs on_epoch) and accuracy / F1 / AUC (multilabel_metrics, multilabel_auroc).
    The weights at the end are the final epoch's: `ModelCheckpoint()` without a monitor keeps the last epoch, which
    is what the reference's `test(ckpt_path="best")` then loads.
    Returns {"history": [per-epoch dict], "epochs_run": int, "stopped_early": bool}."""
    opt = optimizer if optimizer is not None else model.configure_optimizers()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    train_it, n = _as_batches(train, batch_size, gen, True)
    val_it, _ = _as_batches(val, batch_size, None, True)
    n = n if n is not None else n_train
    if n is None:
        raise ValueError("fit_probe: pass n_train with a batch-callable training set")
    c = n_classes if n_classes is not None else getattr(model, "num_classes", None)
    if c is None:
        raise ValueError("fit_probe: pass n_classes")
    dev = next(model.parameters()).device
    buf = torch.empty((n, c), dtype=torch.float32, device=dev)
    tbuf = torch.empty((n, c), dtype=torch.int8, device=dev)
    stopper = EarlyStopping(patience)
    history: List[Dict[str, float]] = []
    for epoch in range(max_epochs):
        model.train()
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        seen = 0
        for step, (xb, yb) in enumerate(train_it(epoch)):
            b = xb.shape[0]
            if seen + b > n:
                raise ValueError(f"fit_probe: more than n_train={n} training samples in epoch {epoch}")
            opt.zero_grad()
            logits = model(xb)
            loss = model.criterion(logits, yb.float())
            loss.backward()
            opt.step()
            buf[seen:seen + b].copy_(logits.detach())
            tbuf[seen:seen + b].copy_(yb)
            loss_sum += loss.detach().double() * b
            seen += b
        model.eval()
        with torch.no_grad():
            vl_sum = torch.zeros((), dtype=torch.float64, device=dev)
            vouts, vys = [], []
            for xb, yb in val_it(epoch):
                logits = model(xb)
                vl_sum += model.criterion(logits, yb.float()).double() * xb.shape[0]
                vouts.append(logits.float())
                vys.append(yb)
            vlog, vy = torch.cat(vouts), torch.cat(vys)
        tr_acc, tr_f1 = multilabel_metrics(buf[:seen], tbuf[:seen])
        va_acc, va_f1 = multilabel_metrics(vlog, vy)
        rec = {"epoch": epoch, "train_loss": float(loss_sum) / max(seen, 1), "train_acc": tr_acc, "train_f1": tr_f1,
               "train_auc": multilabel_auroc(buf[:seen], tbuf[:seen]),
               "val_loss": float(vl_sum) / max(vlog.shape[0], 1), "val_acc": va_acc, "val_f1": va_f1,
               "val_auc": multilabel_auroc(vlog, vy)}
        history.append(rec)
        if stopper.step(rec["val_loss"]):
            break
    model.eval()
    return {"history": history, "epochs_run": len(history), "stopped_early": stopper.stopped}
