"""Device ops of the downstream evaluation (csrc/evalops.hip): per-label AUROC of multi-label scores and inverted dropout.

    auc, npos = multilabel_auroc_per_label(logits, targets)   # float64 [L] on the host, int [L]
    y = dropout(x, p, seed)                                   # autograd: the backward regenerates the mask

No CPU fallback: both raise when the HIP library is missing or the tensors are not on the device.
"""
from __future__ import annotations

import warnings
from typing import Tuple

import torch

from . import _lib
from ._lib import check, dtype_code, ptr, require_gpu, stream_ptr


def multilabel_auroc_per_label(scores: torch.Tensor, targets: torch.Tensor, warn: bool = True
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """torchmetrics MultilabelAUROC(num_labels=L, average=None, thresholds=None) of scores [rows, L] (logits or
    probabilities, bf16 / float32) against 0/1 targets [rows, L]: (auc float64 [L], positives per label int64 [L]),
    both on the host.  Scores outside [0, 1] are ranked by their float32 sigmoid.  A label without positives or
    without negatives gets AUC 0 (and one warning per call), as torchmetrics does."""
    if scores.dim() != 2 or scores.shape != targets.shape:
        raise ValueError(f"multilabel_auroc: scores {tuple(scores.shape)} and targets {tuple(targets.shape)} must be "
                         "the same [rows, labels] shape")
    if scores.dtype not in (torch.float32, torch.bfloat16):
        scores = scores.float()
    scores = scores.contiguous()
    t8 = targets.to(torch.int8).contiguous()
    require_gpu(scores, t8)
    rows, L = scores.shape
    lib = _lib.load()
    need = int(lib.wm_multilabel_auroc_workspace_bytes(rows, L))
    if need == 0:
        raise _lib.WaferHipError(f"multilabel_auroc: unsupported shape rows={rows} labels={L}")
    ws = torch.empty(need, dtype=torch.uint8, device=scores.device)
    auc = torch.empty(L, dtype=torch.float64, device=scores.device)
    npos = torch.empty(L, dtype=torch.int32, device=scores.device)
    check(lib.wm_multilabel_auroc(ptr(scores), dtype_code(scores), ptr(t8), rows, L, ptr(auc), ptr(npos), ptr(ws), need,
                                  stream_ptr()), "wm_multilabel_auroc")
    auc, npos = auc.cpu(), npos.cpu().long()
    if warn and bool(((npos == 0) | (npos == rows)).any()):
        warnings.warn("multilabel_auroc: a label has only one class among the targets; its AUC is meaningless and "
                      "reported as 0 (torchmetrics' rule)", UserWarning, stacklevel=2)
    return auc, npos


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(_lib.load().wm_dropout_fwd(ptr(x), dtype_code(x), x.numel(), p, seed, ptr(y), stream_ptr()), "wm_dropout_fwd")
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(_lib.load().wm_dropout_bwd(ptr(dy), dtype_code(dy), dy.numel(), ctx.p, ctx.seed, ptr(dx), stream_ptr()),
              "wm_dropout_bwd")
        return dx, None, None


def dropout(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """Training-mode inverted dropout: element i kept when rand01(seed, i) >= p, scaled by 1 / (1 - p)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    require_gpu(x.contiguous())
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.WaferHipError(f"dropout: unsupported dtype {x.dtype}")
    if x.numel() > 1 << 32:
        raise _lib.WaferHipError("dropout: more than 2^32 elements in one call (the counter is 32-bit)")
    if x.numel() == 0:
        return x
    return _Dropout.apply(x, p, int(seed) & 0xFFFFFFFF)
