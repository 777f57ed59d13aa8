"""Non-parametric densities of dumped features: sklearn.neighbors.KernelDensity with the Gaussian kernel, the
class-conditional classifier on top of it, and the uniformity / alignment pair of Wang & Isola (2020).

Everything here is one sum, over ALL other rows and not over the k nearest:

    logsum_h(i) = log sum_j exp(-s_ij / (2 h^2)),        s_ij = ||x_i - x_j||^2,

computed for a LIST of bandwidths h in one all-pairs pass (csrc/kde.hip: wm_kde_logsum, float64 exponent arithmetic and
sums over the float32 squared distances of the all-pairs kernels).
  KernelDensity     log density = logsum - log n - (d / 2) log(2 pi h^2); new rows as well as the fitted ones; the
                    leave-one-out values (self excluded, normaliser n - 1) and their sum, the leave-one-out likelihood
                    by which a bandwidth is chosen without labels;
  KDEClassifier     Bayes' rule on one density per class: the rows sorted by class once, one pass per class on that
                    class's column range (single-writer results, no grouped kernel);
  uniformity        log mean_{i != j} exp(-t s_ij) on the normalised rows: the leave-one-out pass with 1 / (2 h^2) = t,
                    then a float64 log-sum-exp of the n row values on the host -- on all rows, not a sample;
  alignment         mean_i ||z1_i - z2_i||^alpha, through manifold.pair_distances (no kernel of its own).

Conventions as in neighbors.py: device tensors in, the functional layer (`gaussian_log_sums`) returns device tensors,
estimator results are host numpy arrays, host-only logic is plain functions that need no GPU; a CPU tensor or a missing
library raises, there is no fallback.  `ref_gaussian_log_sums` restates the kernel in numpy float64 on a given matrix of
squared distances: the CPU tests check it against sklearn, the GPU tests check the kernel against it.  A list of
bandwidths follows linear_model.LogisticRegression with a list of C: results gain a leading axis, `model[i]` is the model
of `bandwidth_[i]`, `best()` picks one.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace
from .cluster import _prep
from .manifold import pair_distances

MAX_BANDWIDTHS = 4  # WM_KDE_MAX_BANDWIDTHS: bandwidths per launch; a longer list goes in chunks
MAX_ROWS = 1 << 24


# ------------------------------------------------------------------------------------------------ host logic (no GPU)


def check_bandwidths(bandwidth) -> Tuple[np.ndarray, bool]:
    """(h float64 [B], whether a single number was given).  Every h is finite and > 0, and so is 1 / (2 h^2)."""
    single = np.ndim(bandwidth) == 0
    try:
        h = np.atleast_1d(np.asarray(bandwidth, dtype=np.float64))
    except (TypeError, ValueError):
        h = np.empty(0)
    if h.ndim != 1 or h.size == 0 or not np.all(np.isfinite(h) & (h > 0.0)):
        raise ValueError(f"bandwidth must be a positive finite number or a sequence of them ({bandwidth!r} given)")
    scales_of(h)
    return h, single


def scales_of(h: np.ndarray) -> np.ndarray:
    """a = 1 / (2 h^2) float64 [B]: what the kernel multiplies the squared distances with."""
    with np.errstate(over="ignore", divide="ignore"):
        a = 1.0 / (2.0 * np.asarray(h, dtype=np.float64) ** 2)
    check_scales(a)
    return a


def check_scales(a) -> np.ndarray:
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    if a.ndim != 1 or a.size == 0 or not np.all(np.isfinite(a) & (a > 0.0)):
        raise ValueError("1 / (2 h^2) must be finite and positive for every bandwidth")
    return np.ascontiguousarray(a)


def rule_of_thumb(rule: str, n: int, d: int) -> float:
    """sklearn 1.7's bandwidth_ for bandwidth="scott" / "silverman" (no data scale in either: sklearn has none)."""
    if rule == "scott":
        return float(n ** (-1.0 / (d + 4)))
    if rule == "silverman":
        return float((n * (d + 2) / 4.0) ** (-1.0 / (d + 4)))
    raise ValueError(f"bandwidth must be a number, a sequence, 'scott' or 'silverman' ({rule!r} given)")


def log_normaliser(h, d: int) -> np.ndarray:
    """(d / 2) log(2 pi h^2): the log of the Gaussian kernel's integral, per bandwidth."""
    h = np.asarray(h, dtype=np.float64)
    return 0.5 * d * np.log(2.0 * np.pi * h * h)


def host_logsumexp(v, axis: int = -1) -> np.ndarray:
    """float64 log-sum-exp along an axis; -inf where every entry is -inf (never NaN)."""
    v = np.asarray(v, dtype=np.float64)
    top = np.max(v, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        out = np.log(np.sum(np.exp(v - safe), axis=axis, keepdims=True)) + safe
    return np.squeeze(out, axis=axis)


def exclusion_mask(m: int, n: int, self_offset: Optional[int]) -> Optional[np.ndarray]:
    """bool [m, n]: column j is excluded for row i when j + self_offset == i (None: nothing is)."""
    if self_offset is None or self_offset < 0:
        return None
    return (np.arange(n)[None, :] + int(self_offset)) == np.arange(m)[:, None]


def ref_gaussian_log_sums(sq, bandwidths=None, exclude=None, *, inv_two_h2=None) -> np.ndarray:
    """float64 [B, m]: wm_kde_logsum in numpy on a matrix sq [m, n] of squared distances.  out[q][i] =
    log sum_j exp(-sq[i][j] / (2 h_q^2)) over the columns not excluded; `exclude`: None, a self offset (an int: column j is
    excluded for row i when j + exclude == i) or a bool mask [m, n].  The shift is the row's smallest included sq, the
    same for every bandwidth; a row without an included column gives -inf.  `inv_two_h2` replaces `bandwidths` by the
    factors themselves."""
    sq = np.asarray(sq, dtype=np.float64)
    if sq.ndim != 2:
        raise ValueError("sq [m, n] expected")
    a = check_scales(inv_two_h2) if inv_two_h2 is not None else scales_of(check_bandwidths(bandwidths)[0])
    m, n = sq.shape
    mask = exclusion_mask(m, n, int(exclude)) if exclude is not None and np.ndim(exclude) == 0 else exclude
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != sq.shape:
            raise ValueError("exclude: an offset or a bool mask [m, n] expected")
        sq = np.where(mask, np.inf, sq)
    out = np.full((a.size, m), -np.inf)
    if n == 0:
        return out
    smin = sq.min(axis=1)
    have = np.isfinite(smin)
    gap = sq[have] - smin[have, None]  # >= 0; +inf for an excluded column: its term is exp(-inf) = 0
    for q, aq in enumerate(a):
        out[q, have] = -aq * smin[have] + np.log(np.exp(-aq * gap).sum(axis=1))
    return out


def squared_distances(xq, x) -> np.ndarray:
    """float64 [m, n]: the exact squared distances of float32 rows, by differences (near-duplicates keep their digits)."""
    xq, x = np.asarray(xq, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = np.empty((xq.shape[0], x.shape[0]))
    for i in range(xq.shape[0]):
        diff = x - xq[i]
        out[i] = np.einsum("jk,jk->j", diff, diff)
    return out


# ------------------------------------------------------------------------------------------------ the entry point


def gaussian_log_sums(xq, x, bandwidths=None, self_offset: Optional[int] = None, out=None, ws=None, *, inv_two_h2=None):
    """float64 [B, m] on the device (wm_kde_logsum): out[q][i] = log sum_j exp(-||xq_i - x_j||^2 / (2 h_q^2)) over the rows
    j of x [n, d] for the rows i of xq [m, d] (device tensors), for a number or a sequence of bandwidths of any length
    (cut into launches of MAX_BANDWIDTHS; a bandwidth has the same bits wherever it stands).  self_offset: None excludes
    nothing; an int >= 0 excludes column j for row i when j + self_offset == i (0 with x = xq: leave-one-out; `lo` with
    x = xq[lo:hi]: leave-one-out against those rows).  `inv_two_h2` gives the factors 1 / (2 h^2) themselves in place of
    `bandwidths`.  A row without an included column gives -inf."""
    import torch

    a = check_scales(inv_two_h2) if inv_two_h2 is not None else scales_of(check_bandwidths(bandwidths)[0])
    xq, x = _prep(xq), _prep(x)
    if xq.shape[1] != x.shape[1]:
        raise ValueError(f"xq has {xq.shape[1]} features, x has {x.shape[1]}")
    (m, d), n = xq.shape, x.shape[0]
    if not (1 <= m <= MAX_ROWS and 1 <= n <= MAX_ROWS):
        raise ValueError(f"1 .. {MAX_ROWS} rows expected on either side ({m} and {n} given)")
    if self_offset is None:
        so = -1
    else:
        so = int(self_offset)
        if not 0 <= so <= MAX_ROWS:
            raise ValueError(f"self_offset: None or an int in [0, {MAX_ROWS}] expected ({self_offset!r} given)")
    if out is None:
        out = torch.empty((a.size, m), dtype=torch.float64, device=x.device)
    else:
        require_gpu(out)
        if out.dtype != torch.float64 or tuple(out.shape) != (a.size, m):
            raise ValueError(f"gaussian_log_sums: out float64 [{a.size}, {m}] expected")
    lib = _lib.load()
    for g in range(0, a.size, MAX_BANDWIDTHS):
        part = np.ascontiguousarray(a[g:g + MAX_BANDWIDTHS])
        need = lib.wm_kde_logsum_workspace_bytes(m, n, d, part.size)
        if ws is None or need == 0 or ws.numel() < need:
            ws = workspace(need, f"gaussian_log_sums: unsupported sizes m={m} n={n} d={d}", x.device)
        check(lib.wm_kde_logsum(ptr(xq), m, ptr(x), n, d, part.ctypes.data, part.size, so, ptr(out) + 8 * g * m, ptr(ws), need,
                                stream_ptr()), "wm_kde_logsum")
    return out


def normalize_rows(z):
    """The rows of z scaled to unit length ONCE, the result rounded to float32 once (functional.l2_normalize): what the
    device passes and a reference both read."""
    from .functional import l2_normalize

    require_gpu(z)
    return l2_normalize(z.float().contiguous()).detach()


# ------------------------------------------------------------------------------------------------ estimators


def _bandwidth_arg(bandwidth):
    if isinstance(bandwidth, str):
        if bandwidth not in ("scott", "silverman"):
            rule_of_thumb(bandwidth, 2, 1)
        return None, True
    return check_bandwidths(bandwidth)


class KernelDensity:
    """sklearn.neighbors.KernelDensity(kernel="gaussian", metric="euclidean") by brute force on the device.

    bandwidth: a number, a sequence of numbers, "scott" or "silverman" (sklearn 1.7's factors n^(-1 / (d + 4)) and
    (n (d + 2) / 4)^(-1 / (d + 4))).  `fit(x)`: x a device tensor [n, d]; sets `bandwidth_` (a float, or float64 [B] for
    a sequence), `n_samples_fit_`, `n_features_in_`.  `score_samples(x)`: sklearn's log densities logsum - log n -
    (d / 2) log(2 pi h^2) as float64 numpy [m] (the fitted rows given back include themselves, as in sklearn);
    `score(x)` their sum.  `loo_score_samples()`: [B, n], every fitted row against the OTHER rows (normaliser n - 1);
    `loo_log_likelihood()`: [B], their sums -- the label-free criterion for the bandwidth.  With a sequence the results
    of score_samples and score gain a leading axis, `model[i]` is the model of bandwidth_[i] and `best()` the one with
    the largest leave-one-out likelihood (the first maximum wins a tie).
    Other kernels and metrics raise NotImplementedError.  Not implemented: sample_weight, sample(), the tree options
    (algorithm, leaf_size, atol, rtol, breadth_first: the sums are exact up to rounding) and mean shift."""

    def __init__(self, bandwidth: Union[float, Sequence[float], str] = 1.0, kernel: str = "gaussian", metric: str = "euclidean"):
        if kernel != "gaussian":
            raise NotImplementedError(f"kernel {kernel!r} is not implemented (available: gaussian)")
        if metric != "euclidean":
            raise NotImplementedError(f"metric {metric!r} is not implemented (available: euclidean)")
        self._h_given, self._single = _bandwidth_arg(bandwidth)
        self.bandwidth, self.kernel, self.metric = bandwidth, kernel, metric
        self._x = self._h = self._loo = None

    # ---- fitting

    def fit(self, x, y=None) -> "KernelDensity":
        require_gpu(x)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("x [n >= 1, d >= 1] expected")
        n, d = int(x.shape[0]), int(x.shape[1])
        h = self._h_given if self._h_given is not None else np.array([rule_of_thumb(self.bandwidth, n, d)])
        return self._store(_prep(x), h, n, d)

    def _store(self, x, h: np.ndarray, n: int, d: int, loo=None) -> "KernelDensity":
        self._x, self._h, self._loo = x, np.asarray(h, dtype=np.float64), loo
        self.n_samples_fit_, self.n_features_in_ = n, d
        self.bandwidth_ = float(self._h[0]) if self._single else self._h.copy()
        return self

    def _fitted(self):
        if self._x is None:
            raise RuntimeError("KernelDensity: call fit first")

    # ---- one bandwidth of a list

    def __len__(self):
        h = self._h if self._h is not None else self._h_given
        return 1 if h is None else h.size

    def __getitem__(self, i: int) -> "KernelDensity":
        """The fitted model of bandwidth_[i] alone (its results without the leading axis)."""
        self._fitted()
        if self._single:
            raise TypeError("this model was fitted for a single bandwidth")
        i = int(i)
        one = KernelDensity(float(self._h[i]), kernel=self.kernel, metric=self.metric)
        return one._store(self._x, self._h[i:i + 1], self.n_samples_fit_, self.n_features_in_,
                          None if self._loo is None else self._loo[i:i + 1])

    def best(self, scores=None) -> "KernelDensity":
        """model[argmax(scores)]; scores default to the leave-one-out log-likelihoods."""
        self._fitted()
        scores = self.loo_log_likelihood() if scores is None else np.asarray(scores, dtype=np.float64)
        if scores.shape != (self._h.size,):
            raise ValueError(f"best: one score per bandwidth expected ({self._h.size})")
        return self[int(np.argmax(scores))]

    # ---- densities

    def _densities(self, logsum: np.ndarray, count: int) -> np.ndarray:
        with np.errstate(divide="ignore"):
            return logsum - np.log(float(count)) - log_normaliser(self._h, self.n_features_in_)[:, None]

    def score_samples(self, x) -> np.ndarray:
        """The log density of the rows of x [m, d] (device tensor): float64 numpy [m], or [B, m] for a list."""
        self._fitted()
        require_gpu(x)
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        logsum = gaussian_log_sums(x, self._x, self._h).cpu().numpy()
        out = self._densities(logsum, self.n_samples_fit_)
        return out[0] if self._single else out

    def score(self, x, y=None):
        """The total log-likelihood of x: a float, or float64 [B] for a list."""
        s = self.score_samples(x)
        return float(s.sum()) if self._single else s.sum(axis=1)

    def loo_score_samples(self) -> np.ndarray:
        """float64 [B, n]: the log density of every fitted row under the other n - 1 rows (an exact duplicate of the row
        is another row and counts)."""
        self._fitted()
        if self.n_samples_fit_ < 2:
            raise ValueError("leave-one-out needs at least 2 fitted rows")
        if self._loo is None:
            logsum = gaussian_log_sums(self._x, self._x, self._h, self_offset=0).cpu().numpy()
            self._loo = self._densities(logsum, self.n_samples_fit_ - 1)
        return self._loo.copy()

    def loo_log_likelihood(self) -> np.ndarray:
        """float64 [B]: the sum of the leave-one-out log densities per bandwidth."""
        return self.loo_score_samples().sum(axis=1)


def _host_ints(y) -> np.ndarray:
    if hasattr(y, "detach"):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1 or not np.issubdtype(y.dtype, np.integer):
        raise ValueError("y: integer labels [n] expected")
    return y.astype(np.int64)


class KDEClassifier:
    """The class-conditional generative classifier on Gaussian kernel densities: p(c | x) proportional to
    prior_c * (1 / n_c) sum_{j in c} exp(-||x - x_j||^2 / (2 h^2)) (the kernel's normaliser is the same for every class
    and cancels), a non-parametric probe beside kNN and logistic regression.

    bandwidth: a number or a sequence (results gain a leading axis).  priors: None (the class frequencies) or positive
    numbers [n_classes] (scaled to sum 1).  `fit(x, y)`: x a device tensor [n, d], y integer labels [n] (host or
    device); rows with y == -1 are ignored.  The labelled rows are sorted by class once (stable); `classes_`, `class_count_`,
    `priors_`, `fit_rows_` (the labelled rows' indices in x, in their original order).  `predict_log_proba(x)`,
    `predict_proba(x)` float64 numpy [m, n_classes], `predict(x)` labels [m] (the first maximum wins a tie).
    `loo_predict_proba()` / `loo_predict()`: the same for the labelled fitted rows, in the order of `fit_rows_`, every
    row left out of its own class (that class is then normalised by n_c - 1; a class of one row has no density left for
    its own row and gets probability 0 there)."""

    def __init__(self, bandwidth: Union[float, Sequence[float]] = 1.0, priors=None):
        if isinstance(bandwidth, str):
            raise ValueError("KDEClassifier: a number or a sequence of bandwidths expected")
        self._h, self._single = check_bandwidths(bandwidth)
        self.bandwidth, self.priors = bandwidth, priors
        self._x = None

    def fit(self, x, y) -> "KDEClassifier":
        import torch

        require_gpu(x)
        if x.dim() != 2:
            raise ValueError("x [n, d] expected")
        y = _host_ints(y)
        if y.shape[0] != x.shape[0]:
            raise ValueError(f"y: {x.shape[0]} labels expected ({y.shape[0]} given)")
        rows = np.flatnonzero(y != -1)
        if rows.size == 0:
            raise ValueError("no labelled row (every y is -1)")
        classes, idx = np.unique(y[rows], return_inverse=True)
        order = np.argsort(idx, kind="stable")
        counts = np.bincount(idx, minlength=classes.size)
        if self.priors is None:
            priors = counts / float(rows.size)
        else:
            priors = np.asarray(self.priors, dtype=np.float64)
            if priors.shape != (classes.size,) or not np.all(np.isfinite(priors) & (priors > 0.0)):
                raise ValueError(f"priors: positive numbers [{classes.size}] expected")
            priors = priors / priors.sum()
        take = torch.from_numpy(rows[order]).to(x.device)
        self._x = _prep(x).index_select(0, take).contiguous()  # the labelled rows, sorted by class
        self._inverse = np.argsort(order, kind="stable")        # sorted position of the labelled row r: _inverse[r]
        self._sorted_class = idx[order]
        self.classes_, self.class_count_, self.priors_, self.fit_rows_ = classes, counts, priors, rows
        self._lo = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        self.n_features_in_ = int(x.shape[1])
        return self

    def _fitted(self):
        if self._x is None:
            raise RuntimeError("KDEClassifier: call fit first")

    def _class_log_sums(self, xq, leave_out: bool) -> np.ndarray:
        """float64 [B, m, C]: one gaussian_log_sums call per class on that class's rows of the sorted matrix."""
        cols = []
        for c in range(self.classes_.size):
            lo, hi = int(self._lo[c]), int(self._lo[c] + self.class_count_[c])
            cols.append(gaussian_log_sums(xq, self._x[lo:hi], self._h, self_offset=lo if leave_out else None).cpu().numpy())
        return np.stack(cols, axis=2)

    def _posterior(self, logsum: np.ndarray, counts: np.ndarray) -> np.ndarray:
        """log p(c | row) [B, m, C] from the classes' log-sums and the per-(row, class) normalising counts [m, C]."""
        with np.errstate(divide="ignore", invalid="ignore"):
            joint = np.where(counts[None] > 0, logsum - np.log(np.maximum(counts, 1).astype(np.float64))[None], -np.inf)
        joint = joint + np.log(self.priors_)[None, None, :]
        total = host_logsumexp(joint, axis=2)
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(total)[..., None], joint - np.where(np.isfinite(total), total, 0.0)[..., None], -np.inf)

    def _shape(self, v: np.ndarray) -> np.ndarray:
        return v[0] if self._single else v

    def predict_log_proba(self, x) -> np.ndarray:
        self._fitted()
        require_gpu(x)
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        logsum = self._class_log_sums(x, leave_out=False)
        counts = np.broadcast_to(self.class_count_[None, :], logsum.shape[1:])
        return self._shape(self._posterior(logsum, counts))

    def predict_proba(self, x) -> np.ndarray:
        return np.exp(self.predict_log_proba(x))

    def predict(self, x) -> np.ndarray:
        return self.classes_[np.argmax(self.predict_log_proba(x), axis=-1)]

    def loo_predict_log_proba(self) -> np.ndarray:
        self._fitted()
        logsum = self._class_log_sums(self._x, leave_out=True)  # rows in sorted order
        counts = np.tile(self.class_count_[None, :], (self._x.shape[0], 1))
        counts[np.arange(counts.shape[0]), self._sorted_class] -= 1  # a row is not one of its own class's columns
        return self._shape(self._posterior(logsum, counts)[:, self._inverse])

    def loo_predict_proba(self) -> np.ndarray:
        return np.exp(self.loo_predict_log_proba())

    def loo_predict(self) -> np.ndarray:
        return self.classes_[np.argmax(self.loo_predict_log_proba(), axis=-1)]


# ------------------------------------------------------------------------------------------------ Wang & Isola (2020)


def uniformity_from_row_sums(logsum, n: int) -> np.ndarray:
    """log((1 / (n (n - 1))) sum_i exp(logsum[..., i])) in float64: the last step of `uniformity`, on the host."""
    return host_logsumexp(logsum, axis=-1) - math.log(float(n) * float(n - 1))


def uniformity(z, t: Union[float, Sequence[float]] = 2.0, normalize: bool = True):
    """log mean_{i != j} exp(-t ||z_i - z_j||^2) over ALL ordered pairs of the rows of z [n >= 2, d] (device tensor):
    a float, or float64 [T] for a sequence of t.  0 for collapsed rows, more negative the more evenly the rows cover the
    sphere.  normalize: scale the rows to unit length first (`normalize_rows`)."""
    single = np.ndim(t) == 0
    a = check_scales(t)
    require_gpu(z)
    if z.dim() != 2 or z.shape[0] < 2:
        raise ValueError("z [n >= 2, d] expected")
    rows = normalize_rows(z) if normalize else z
    logsum = gaussian_log_sums(rows, rows, inv_two_h2=a, self_offset=0).cpu().numpy()
    out = uniformity_from_row_sums(logsum, int(z.shape[0]))
    return float(out[0]) if single else out


def alignment(z1, z2, alpha: float = 2.0, normalize: bool = True) -> float:
    """mean_i ||z1_i - z2_i||^alpha of two views' rows [n, d] (device tensors), the distances by the all-pairs kernels'
    distance function (manifold.pair_distances with idx = arange), the power and the mean in float64 on the host."""
    import torch

    require_gpu(z1, z2)
    if z1.dim() != 2 or z1.shape != z2.shape or z1.shape[0] < 1:
        raise ValueError("z1 and z2 [n >= 1, d] of one shape expected")
    if not float(alpha) > 0.0:
        raise ValueError(f"alpha > 0 expected ({alpha!r} given)")
    a, b = (normalize_rows(z1), normalize_rows(z2)) if normalize else (z1, z2)
    idx = torch.arange(z1.shape[0], dtype=torch.int32, device=z1.device).unsqueeze(1).contiguous()
    dist = pair_distances(a, b, idx).cpu().numpy().astype(np.float64)[:, 0]
    return float(np.mean(dist ** float(alpha)))
