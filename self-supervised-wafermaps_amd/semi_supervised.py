"""Graph-based semi-supervised learning on dumped features: sklearn.semi_supervised's LabelSpreading and
LabelPropagation over the exact kNN graph, `fit(x, y)` with -1 for the unknown labels.

WM-811K labels 172 950 of its 811 457 wafers.  models/knn.py votes among the labelled rows only; these estimators push
the labels through the neighbourhood structure of ALL rows and return a soft class distribution per row.

Steps, all on the device:
  1. the affinity graph of the spectral estimators (manifold.affinity_graph: "connectivity" or "fuzzy", or a ready
     manifold.CSR), without its diagonal (sklearn's normalised Laplacian ignores self-loops), and its float64 degrees
     (csrc/spectral.hip: wm_spec_degree);
  2. the label matrix (csrc/propagate.hip: wm_lp_init) and the iteration (wm_lp_iterate), the hot path:
       spreading    F <- alpha S F + (1 - alpha) Y,  S = D^-1/2 G D^-1/2        (Zhou et al. 2004)
       propagation  F <- D^-1 G F, every row divided by its sum, the labelled rows put back to Y, each step
                    (Zhu and Ghahramani 2002, with the renormalisation inside the loop as sklearn has it)
     for a LIST of alphas in one pass: R groups of C class columns share every gather of the graph.  The host reads the
     residuals sum |F_new - F_old| once per `check_every` steps; a group whose residual is below `tol` there is frozen (its
     columns are copied from then on) and the fit ends when every group is frozen or after `max_iter` steps.  A group gives
     the same bits alone as among others at the same `check_every`.  With check_every = 1, `n_iter_` is sklearn's;
  3. per group the normalised distributions, the arg-max labels and the rows no label reached (wm_lp_finalize);
  4. new rows: their exact kNN among the fitted rows (manifold.knn_query) and the normalised mean of the neighbours'
     distributions (wm_lp_neighbor_mean).

Rows in a graph component without a labelled row keep an all-zero distribution.  sklearn reports classes_[0] for them;
`transduction_` does the same and `unreached_` marks them.
"""
from __future__ import annotations

from typing import Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace
from .manifold import CSR, MAX_NEIGHBORS, _check_graph, _checked_labels, _token_ws, _without_diagonal, affinity_graph, \
    knn_query, laplacian_degree
from .cluster import metric_code

MAX_COLUMNS = 256  # alpha groups x classes that one pass of the kernel takes


# ------------------------------------------------------------------------------------------------ host logic (no GPU)


def check_alphas(alpha) -> Tuple[np.ndarray, bool]:
    """(alphas float64 [R], whether a single number was given).  Every alpha lies strictly inside (0, 1)."""
    single = np.ndim(alpha) == 0
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    if a.ndim != 1 or a.size == 0 or not np.all((a > 0.0) & (a < 1.0)):
        raise ValueError(f"alpha must be a number or a sequence of numbers in the open interval (0, 1) ({alpha!r} given)")
    return a.copy(), single


def check_columns(groups: int, classes: int) -> int:
    """groups * classes, which one pass takes up to MAX_COLUMNS of."""
    groups, classes = int(groups), int(classes)
    if groups < 1 or classes < 1:
        raise ValueError(f"at least one group and one class expected ({groups} x {classes} given)")
    if groups * classes > MAX_COLUMNS:
        raise ValueError(f"{groups} alpha groups x {classes} classes = {groups * classes} columns: one pass takes at most "
                         f"{MAX_COLUMNS} (fit fewer alphas at a time)")
    return groups * classes


def check_label_codes(labels, classes: int) -> None:
    """labels (numpy array or tensor) must lie in -1 .. classes - 1."""
    if len(labels) and (int(labels.min()) < -1 or int(labels.max()) >= int(classes)):
        raise ValueError(f"labels must lie in -1 .. {int(classes) - 1} (-1: unknown)")


def encode_labels(y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(classes_ sorted, codes int32 [n] in -1 .. C - 1) of integer labels with -1 for unknown."""
    y = np.asarray(y)
    known = y >= 0
    if not known.any():
        raise ValueError("y holds no known label (every entry is -1)")
    classes, codes = np.unique(y[known], return_inverse=True)
    out = np.full(y.shape[0], -1, dtype=np.int32)
    out[known] = codes.astype(np.int32)
    return classes, out


class ChunkPlan:
    """The bookkeeping of a fit: how many steps to enqueue next, which groups are still active, and what a chunk's
    residuals mean.  Steps come in chunks of `check_every` (the last one shorter); after a chunk the residual of its LAST
    step decides, per active group, whether the group is frozen (residual < tol) -- the steps in between are not looked at,
    the group has taken them anyway.  `n_iter[g]` is the number of steps group g took."""

    def __init__(self, groups: int, max_iter: int, tol: float, check_every: int):
        if int(max_iter) < 1 or int(check_every) < 1 or not float(tol) >= 0.0:
            raise ValueError("max_iter >= 1, check_every >= 1 and tol >= 0 required")
        self.groups, self.max_iter, self.tol, self.check_every = int(groups), int(max_iter), float(tol), int(check_every)
        self.done = 0
        self.active = np.ones(self.groups, dtype=np.int32)
        self.n_iter = np.zeros(self.groups, dtype=np.int64)
        self.history = []

    def next_chunk(self) -> int:
        """Steps of the next chunk; 0 when the fit is over."""
        if not self.active.any():
            return 0
        return min(self.check_every, self.max_iter - self.done)

    def record(self, resid: np.ndarray) -> None:
        """Takes the residual table [steps, groups] of the chunk just run."""
        resid = np.array(resid, dtype=np.float64)
        if resid.ndim != 2 or resid.shape[1] != self.groups or resid.shape[0] != self.next_chunk():
            raise ValueError(f"a residual table [{self.next_chunk()}, {self.groups}] expected")
        on = self.active != 0
        resid[:, ~on] = np.nan  # a frozen group takes no step: its columns are copied
        self.history.append(resid)
        self.done += resid.shape[0]
        self.n_iter[on] = self.done
        self.active[on & (resid[-1] < self.tol)] = 0

    @property
    def residuals(self) -> np.ndarray:
        """float64 [steps taken, groups], NaN where a group was frozen already."""
        return np.concatenate(self.history, axis=0) if self.history else np.zeros((0, self.groups))


# ------------------------------------------------------------------------------------------------ the four entry points


def _f_matrix(name: str, F, n: int, cols: int):
    import torch

    require_gpu(F)
    if F.dtype != torch.float64 or F.dim() != 2 or F.shape[0] != n or F.shape[1] < cols:
        raise ValueError(f"{name}: float64 [{n}, >= {cols}] expected")


def _device_labels(labels, n: int, classes: int, checked: bool = False):
    """dtype and shape always; the range of the codes (two reductions and two reads by the host) unless `checked`."""
    import torch

    require_gpu(labels)
    if labels.dtype != torch.int32 or labels.shape != (n,):
        raise ValueError(f"labels int32 [{n}] expected")
    if not checked:
        check_label_codes(labels, classes)


def label_matrix(labels, classes: int, groups: int = 1, out=None, checked: bool = False, ws=None):
    """F float64 [n, groups * classes] on the device (wm_lp_init): column g * classes + c of row i is 1.0 where
    labels[i] == c, else 0.0.  labels int32 [n] in -1 .. classes - 1 on the device; `out` may be wider (its other columns
    are left alone).  `checked`: the caller has validated the range of the labels already."""
    import torch

    cols = check_columns(groups, classes)
    n = int(labels.shape[0]) if hasattr(labels, "shape") and len(labels.shape) == 1 else -1
    _device_labels(labels, n, classes, checked)
    out = torch.empty((n, cols), dtype=torch.float64, device=labels.device) if out is None else out
    _f_matrix("out", out, n, cols)
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_lp_init_workspace_bytes(n, int(classes), int(groups)),
                         f"label_matrix: unsupported sizes n={n} classes={classes} groups={groups}", labels.device, ws)
    check(lib.wm_lp_init(ptr(labels), n, int(classes), int(groups), ptr(out), out.shape[1], ptr(ws), need, stream_ptr()), "wm_lp_init")
    return out


def propagate_workspace(n: int, classes: int, groups: int, device):
    """The workspace of `propagate` for these sizes, allocated once per fit."""
    need = _lib.load().wm_lp_iterate_workspace_bytes(int(n), int(classes), int(groups))
    return workspace(need, f"propagate: unsupported sizes n={n} classes={classes} groups={groups}", device)


def propagate(graph: CSR, dinv, labels, classes: int, alpha, active, Fa, Fb, iters: int, hard: bool = False, resid=None,
              checked: bool = False, ws=None):
    """`iters` steps Fa -> Fb -> Fa ... on the device (wm_lp_iterate); returns (the buffer that holds the result,
    resid float64 [iters, groups] on the device).  alpha float64 [groups] and active int32 [groups] are device tensors
    (a group with active 0 is copied); Fa, Fb float64 [n, >= groups * classes] of one pitch; hard: label propagation with
    clamped labelled rows and every other row divided by its sum (alpha is not read).
    `checked`: the caller has validated the graph and the range of the labels already; the call then enqueues its launches
    and reads nothing back."""
    import torch

    n = graph.indptr.numel() - 1 if checked else _check_graph(graph)
    require_gpu(dinv, alpha, active)
    if alpha.dtype != torch.float64 or alpha.dim() != 1 or active.dtype != torch.int32 or active.shape != alpha.shape:
        raise ValueError("alpha float64 [groups] and active int32 [groups] expected")
    groups = alpha.shape[0]
    cols = check_columns(groups, classes)
    _device_labels(labels, n, classes, checked)
    if dinv.dtype != torch.float64 or dinv.shape != (n,):
        raise ValueError(f"dinv float64 [{n}] expected")
    _f_matrix("Fa", Fa, n, cols)
    _f_matrix("Fb", Fb, n, cols)
    if Fa.shape != Fb.shape or Fa.data_ptr() == Fb.data_ptr():
        raise ValueError("Fa and Fb must be two buffers of one shape")
    iters = int(iters)
    if iters < 1:
        raise ValueError("iters >= 1 required")
    resid = torch.empty((iters, groups), dtype=torch.float64, device=Fa.device) if resid is None else resid
    require_gpu(resid)
    if resid.dtype != torch.float64 or resid.numel() < iters * groups:
        raise ValueError(f"resid float64 with at least {iters * groups} cells expected")
    ws = propagate_workspace(n, classes, groups, Fa.device) if ws is None else ws
    check(_lib.load().wm_lp_iterate(ptr(graph.indptr), ptr(graph.indices), ptr(graph.data), ptr(dinv), ptr(labels), n, int(classes),
                                    groups, ptr(alpha), ptr(active), 1 if hard else 0, iters, ptr(Fa), ptr(Fb), Fa.shape[1],
                                    ptr(resid), ptr(ws), ws.numel(), stream_ptr()), "wm_lp_iterate")
    return (Fb if iters % 2 else Fa), resid.view(-1)[:iters * groups].view(iters, groups)


def finalize_labels(F, classes: int, group: int = 0, ws=None):
    """(dist float64 [n, classes], rowsum float64 [n], pred int32 [n], unreached bool [n]) of one group's columns of F
    (wm_lp_finalize): dist = F / rowsum with all-zero rows left zero, pred the first maximum, unreached = (rowsum == 0)."""
    import torch

    classes, group = int(classes), int(group)
    require_gpu(F)
    if F.dtype != torch.float64 or F.dim() != 2 or classes < 1 or group < 0 or (group + 1) * classes > F.shape[1]:
        raise ValueError("F float64 [n, ld] with the group's columns inside it expected")
    n, ld = F.shape
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_lp_finalize_workspace_bytes(n, classes), f"finalize_labels: unsupported sizes n={n} classes={classes}",
                         F.device, ws)
    dist = torch.empty((n, classes), dtype=torch.float64, device=F.device)
    rowsum = torch.empty(n, dtype=torch.float64, device=F.device)
    pred = torch.empty(n, dtype=torch.int32, device=F.device)
    unreached = torch.empty(n, dtype=torch.uint8, device=F.device)
    check(lib.wm_lp_finalize(ptr(F) + 8 * group * classes, ld, n, classes, ptr(dist), ptr(rowsum), ptr(pred), ptr(unreached), ptr(ws),
                             need, stream_ptr()), "wm_lp_finalize")
    return dist, rowsum, pred, unreached.bool()


def neighbor_mean(idx, dist, ws=None):
    """out float64 [m, C] on the device (wm_lp_neighbor_mean): the sum of dist[idx[r][t]] over t, divided by its total;
    rows whose neighbours are all unreached stay zero.  idx int32 [m, k] in [0, n), dist float64 [n, C]."""
    import torch

    require_gpu(idx, dist)
    if idx.dtype != torch.int32 or idx.dim() != 2 or dist.dtype != torch.float64 or dist.dim() != 2:
        raise ValueError("idx int32 [m, k] and dist float64 [n, C] expected")
    (m, k), (n, classes) = idx.shape, dist.shape
    if m < 1 or not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"at least one row and 1 .. {MAX_NEIGHBORS} neighbours expected")
    if int(idx.min()) < 0 or int(idx.max()) >= n:
        raise ValueError("idx must lie in [0, n)")
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_lp_neighbor_mean_workspace_bytes(m, k, classes),
                         f"neighbor_mean: unsupported sizes m={m} k={k} classes={classes}", dist.device, ws)
    out = torch.empty((m, classes), dtype=torch.float64, device=dist.device)
    check(lib.wm_lp_neighbor_mean(ptr(idx), m, k, ptr(dist), n, classes, ptr(out), ptr(ws), need, stream_ptr()), "wm_lp_neighbor_mean")
    return out


# ------------------------------------------------------------------------------------------------ estimators


class _GraphSSL:
    """What LabelSpreading and LabelPropagation share: the graph, the chunked iteration and the attributes."""

    _hard = False

    def __init__(self, n_neighbors: int, alphas: np.ndarray, single: bool, max_iter: int, tol: float, affinity, metric: str,
                 check_every: int):
        metric_code(metric)
        if not isinstance(affinity, CSR) and affinity not in ("connectivity", "fuzzy"):
            raise ValueError(f"affinity must be 'connectivity', 'fuzzy' or a manifold.CSR ({affinity!r} given)")
        if not 1 <= int(n_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors in [1, {MAX_NEIGHBORS}] required")
        ChunkPlan(len(alphas), max_iter, tol, check_every)  # (its checks)
        self.n_neighbors, self.metric, self.affinity = int(n_neighbors), metric, affinity
        self.max_iter, self.tol, self.check_every = int(max_iter), float(tol), int(check_every)
        self._alphas, self._single = alphas, single
        self.classes_ = self.label_distributions_ = self.transduction_ = self.unreached_ = self.n_iter_ = self.residuals_ = None
        self.affinity_matrix_ = self._x = self._dist = None

    def fit(self, x, y):
        import torch

        require_gpu(x)
        n = x.shape[0]
        y_dev = _checked_labels(y, n)
        self.classes_, codes = encode_labels(y_dev.cpu().numpy())
        C, R = len(self.classes_), len(self._alphas)
        cols = check_columns(R, C)
        if isinstance(self.affinity, CSR):
            graph = self.affinity
            if _check_graph(graph) != n:
                raise ValueError(f"the affinity graph has {graph.indptr.numel() - 1} rows, x has {n}")
        else:
            graph = affinity_graph(x, min(self.n_neighbors, n), self.metric, self.affinity)
        graph = _without_diagonal(graph)
        dev = graph.data.device
        _, dinv = laplacian_degree(graph)
        check_label_codes(codes, C)  # once, on the host: the calls below pass checked=True and never wait for the device
        labels = torch.from_numpy(codes).to(dev)
        alpha = torch.from_numpy(self._alphas).to(dev)
        Fa = label_matrix(labels, C, R, checked=True)
        Fb = torch.empty_like(Fa)
        ws = propagate_workspace(n, C, R, dev)
        plan = ChunkPlan(R, self.max_iter, self.tol, self.check_every)
        resid = torch.empty((min(self.check_every, self.max_iter), R), dtype=torch.float64, device=dev)
        cur, other = Fa, Fb
        sent = plan.active.copy()
        active = torch.from_numpy(sent).to(dev)
        while True:
            steps = plan.next_chunk()
            if steps == 0:
                break
            if not np.array_equal(sent, plan.active):  # a group was frozen at the last boundary
                sent = plan.active.copy()
                active = torch.from_numpy(sent).to(dev)
            out, table = propagate(graph, dinv, labels, C, alpha, active, cur, other, steps, hard=self._hard, resid=resid,
                                   checked=True, ws=ws)
            if out is other:
                cur, other = other, cur
            plan.record(table.cpu().numpy())  # the chunk's only synchronisation
        dists, preds, masks = [], [], []
        for g in range(R):
            dist, _, pred, unreached = finalize_labels(cur, C, g)
            dists.append(dist)
            preds.append(pred)
            masks.append(unreached)
        self._x, self._dist, self.affinity_matrix_ = x, dists, graph
        pick = (lambda seq: seq[0]) if self._single else (lambda seq: np.stack(seq))
        self.label_distributions_ = pick([d.cpu().numpy() for d in dists])
        self.transduction_ = pick([self.classes_[p.cpu().numpy()] for p in preds])
        self.unreached_ = pick([m.cpu().numpy() for m in masks])
        self.n_iter_ = int(plan.n_iter[0]) if self._single else plan.n_iter.copy()
        self.residuals_ = plan.residuals[:, 0] if self._single else plan.residuals
        return self

    def predict_proba(self, x):
        """float64 [m, C] (numpy; [R, m, C] for a list of alphas): the normalised mean of the fitted distributions of each
        row's `n_neighbors` nearest fitted rows; all zeros where none of them was reached."""
        if self._dist is None:
            raise RuntimeError("fit first")
        _, idx = knn_query(x, self._x, min(self.n_neighbors, self._x.shape[0]), self.metric)
        out = [neighbor_mean(idx, d).cpu().numpy() for d in self._dist]
        return out[0] if self._single else np.stack(out)

    def predict(self, x):
        """classes_[argmax predict_proba] (classes_[0] for an all-zero row, as in `transduction_`)."""
        return self.classes_[np.argmax(self.predict_proba(x), axis=-1)]


class LabelSpreading(_GraphSSL):
    """sklearn.semi_supervised.LabelSpreading over the exact kNN graph of device rows.  `fit(x, y)`: x a device tensor
    [n, d], y integer labels with -1 for unknown.  alpha: a number, or a sequence of numbers fitted in one pass (every
    attribute then gains a leading axis of that length).  Sets `classes_`, `label_distributions_` (float64 [n, C]),
    `transduction_`, `unreached_` (rows no label reached: their distribution is zero and their transduction_ is
    classes_[0], sklearn's rule), `n_iter_`, `residuals_` ([steps], NaN once a group is frozen) and `affinity_matrix_`
    (the CSR without its diagonal)."""

    def __init__(self, n_neighbors: int = 7, alpha: Union[float, Sequence[float]] = 0.2, max_iter: int = 30, tol: float = 1e-3,
                 affinity="connectivity", metric: str = "euclidean", check_every: int = 8):
        alphas, single = check_alphas(alpha)
        super().__init__(n_neighbors, alphas, single, max_iter, tol, affinity, metric, check_every)
        self.alpha = alpha


class LabelPropagation(_GraphSSL):
    """sklearn.semi_supervised.LabelPropagation over the exact kNN graph: the row-normalised graph, the labelled rows
    clamped to their labels at every step.  Arguments and attributes as LabelSpreading's, without alpha."""

    _hard = True

    def __init__(self, n_neighbors: int = 7, max_iter: int = 30, tol: float = 1e-3, affinity="connectivity",
                 metric: str = "euclidean", check_every: int = 8):
        super().__init__(n_neighbors, np.array([0.5]), True, max_iter, tol, affinity, metric, check_every)
