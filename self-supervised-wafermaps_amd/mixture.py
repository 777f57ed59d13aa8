"""Gaussian mixture of dumped embeddings: a per-row likelihood, soft assignments with elliptical clusters, BIC / AIC.

The probabilistic model next to `cluster.KMeans` (hard, convex) and `cluster.HDBSCAN` (density tree): `score_samples` of
a fitted mixture is the usual novelty score of new rows, `predict_proba` the soft assignment, and `bic` / `aic` the usual
way to choose the number of clusters.  A full-covariance mixture on `decomposition.PCA(50)` output is the intended use.

`GaussianMixture` has sklearn.mixture.GaussianMixture's surface and its attributes' meaning (sklearn 1.7), for
covariance_type "full", "diag" and "spherical".  The passes over the rows are HIP kernels in float64 on the float32 rows
(csrc/gmm.hip; f64 MFMA tiles for the full-covariance log-probabilities, the weighted sums and the weighted scatter), each
with a stated summation order, so two fits give the same bits.  Two things differ from sklearn's arithmetic on purpose:
the row is centred before it is multiplied in the E-step (sklearn: x P - mu P), and the M-step is two passes, the scatter
centred on the new mean (sklearn's diag form avg_X2 - 2 avg_X mu + mu^2 cancels).  What runs on the host, in numpy /
scipy float64, and why: the Cholesky factor of the k covariance matrices, its triangular inverse and the
log-determinants (`precision_cholesky`: scipy.linalg.cholesky and solve_triangular, sklearn's own calls; k d^3 / 3
flops, small next to one E-step), the divisions by nk and the convergence test.  One host synchronisation per half-step.

Not implemented: covariance_type="tied", init_params="random", warm_start, sample(), the Bayesian variant.  The random
stream is numpy.random.default_rng(random_state) and not sklearn's: the same seed starts elsewhere.  DESIGN.md states
the definitions and the error bounds.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace

MAX_FEATURES = 1024       # diag, spherical
MAX_FEATURES_FULL = 256   # full
MAX_COMPONENTS = 1024
COVARIANCE_TYPES = ("full", "diag", "spherical")
INIT_PARAMS = ("kmeans", "k-means++", "random_from_data")
_EPS10 = 10.0 * np.finfo(np.float64).eps
_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for "
                "instance caused by singleton or collapsed samples). Try to decrease the number of components, increase "
                "reg_covar, or scale the input data.")


def _check_covariance_type(covariance_type):
    if covariance_type == "tied":
        raise NotImplementedError('covariance_type="tied" is not implemented (available: ' + ", ".join(COVARIANCE_TYPES) + ")")
    if covariance_type not in COVARIANCE_TYPES:
        raise ValueError(f"unknown covariance_type {covariance_type!r} (available: " + ", ".join(COVARIANCE_TYPES) + ")")


def _prep(x, covariance_type: str = "diag"):
    """(contiguous float32 [n, ld] on the device with ld = d rounded up to a multiple of 4, d).  The kernels take the true
    d and never load the padding columns.  Shapes are checked before the device is."""
    import torch

    if x.dim() != 2:
        raise ValueError("expected [n_samples, n_features]")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 1 or d < 1:
        raise ValueError("at least one row and one feature expected")
    limit = MAX_FEATURES_FULL if covariance_type == "full" else MAX_FEATURES
    if d > limit:
        raise ValueError(f"at most {limit} features with covariance_type={covariance_type!r} ({d} given): reduce the matrix first")
    if n > 1 << 24:
        raise ValueError(f"at most {1 << 24} rows ({n} given)")
    require_gpu(x)
    x = x.float()
    if d % 4:
        x = torch.nn.functional.pad(x, (0, 4 - d % 4))
    return x.contiguous(), d


def _f64(v, device, shape=None, what: str = "array"):
    """v (numpy, list or tensor) as a contiguous float64 tensor on `device`; `shape` is checked."""
    import torch

    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(shape)} expected, {tuple(t.shape)} given")
    return t.to(device=device, dtype=torch.float64).contiguous()


# ------------------------------------------------------------------------------------------------ kernel wrappers
# They take the padded rows xp [n, ld], the true d and raw float64 device operands.


def _sizes(xp, d: int, k: int, what: str):
    n, ld = xp.shape
    if not (1 <= d <= ld and ld % 4 == 0):
        raise ValueError(f"{what}: 1 <= d <= the row pitch, a multiple of 4, expected")
    if not 1 <= k <= MAX_COMPONENTS:
        raise ValueError(f"{what}: 1 <= n_components <= {MAX_COMPONENTS} expected ({k} given)")
    return n, ld


def _logprob_diag(xp, d: int, mean, inv_var, cst):
    """out[i][c] = cst[c] - 0.5 * sum_f (x[i][f] - mean[c][f])^2 * inv_var[c][f]; float64 [n, k]."""
    import torch

    k = mean.shape[0]
    n, ld = _sizes(xp, d, k, "logprob_diag")
    require_gpu(xp, mean, inv_var, cst)
    if mean.shape != (k, d) or inv_var.shape != (k, d) or cst.shape != (k,):
        raise ValueError("logprob_diag: mean [k, d], inv_var [k, d], cst [k] expected")
    lib = _lib.load()
    need = lib.wm_gmm_logprob_diag_workspace_bytes(n, d, ld, k)
    ws = workspace(need, f"logprob_diag n={n} d={d} k={k}: unsupported sizes (reduce the matrix first)", xp.device)
    out = torch.empty((n, k), dtype=torch.float64, device=xp.device)
    check(lib.wm_gmm_logprob_diag(ptr(xp), n, d, ld, ptr(mean), ptr(inv_var), ptr(cst), k, ptr(out), ptr(ws), need,
                                  stream_ptr()), "wm_gmm_logprob_diag")
    return out


def _logprob_full(xp, d: int, mean, pchol, cst):
    """out[i][c] = cst[c] - 0.5 * ||(x_i - mean_c) pchol_c||^2, only the upper triangle of pchol_c read; float64 [n, k]."""
    import torch

    k = mean.shape[0]
    n, ld = _sizes(xp, d, k, "logprob_full")
    require_gpu(xp, mean, pchol, cst)
    if mean.shape != (k, d) or pchol.shape != (k, d, d) or cst.shape != (k,):
        raise ValueError("logprob_full: mean [k, d], pchol [k, d, d], cst [k] expected")
    lib = _lib.load()
    need = lib.wm_gmm_logprob_full_workspace_bytes(n, d, ld, k)
    ws = workspace(need, f"logprob_full n={n} d={d} k={k}: unsupported sizes (reduce the matrix first)", xp.device)
    out = torch.empty((n, k), dtype=torch.float64, device=xp.device)
    check(lib.wm_gmm_logprob_full(ptr(xp), n, d, ld, ptr(mean), ptr(pchol), ptr(cst), k, ptr(out), ptr(ws), need,
                                  stream_ptr()), "wm_gmm_logprob_full")
    return out


def _normalize(wlp):
    """In place on wlp float64 [n, k]: the rows become responsibilities.  Returns (lpn [n], labels int32 [n], lpn_sum
    [1]), device tensors."""
    import torch

    require_gpu(wlp)
    if wlp.dim() != 2 or wlp.dtype != torch.float64:
        raise ValueError("normalize: float64 [n, k] expected")
    n, k = wlp.shape
    lib = _lib.load()
    need = lib.wm_gmm_normalize_workspace_bytes(n, k)
    ws = workspace(need, f"normalize n={n} k={k}: unsupported sizes", wlp.device)
    lpn = torch.empty(n, dtype=torch.float64, device=wlp.device)
    label = torch.empty(n, dtype=torch.int32, device=wlp.device)
    total = torch.empty(1, dtype=torch.float64, device=wlp.device)
    check(lib.wm_gmm_normalize(ptr(wlp), n, k, ptr(lpn), ptr(label), ptr(total), ptr(ws), need, stream_ptr()),
          "wm_gmm_normalize")
    return lpn, label, total


def _check_resp(xp, resp, what: str) -> int:
    import torch

    require_gpu(xp, resp)
    if resp.dim() != 2 or resp.shape[0] != xp.shape[0] or resp.dtype != torch.float64:
        raise ValueError(f"{what}: resp float64 [n_samples, n_components] expected")
    return int(resp.shape[1])


def _weighted_sums(xp, d: int, resp):
    """(nk [k] = sum_i resp[i], sx [k, d] = resp^T x), float64 device tensors."""
    import torch

    k = _check_resp(xp, resp, "weighted_sums")
    n, ld = _sizes(xp, d, k, "weighted_sums")
    lib = _lib.load()
    need = lib.wm_gmm_weighted_sums_workspace_bytes(n, d, ld, k)
    ws = workspace(need, f"weighted_sums n={n} d={d} k={k}: unsupported sizes (reduce the matrix first)", xp.device)
    nk = torch.empty(k, dtype=torch.float64, device=xp.device)
    sx = torch.empty((k, d), dtype=torch.float64, device=xp.device)
    check(lib.wm_gmm_weighted_sums(ptr(xp), n, d, ld, ptr(resp), k, ptr(nk), ptr(sx), ptr(ws), need, stream_ptr()),
          "wm_gmm_weighted_sums")
    return nk, sx


def _scatter(xp, d: int, resp, mean, full: bool):
    import torch

    name = "scatter_full" if full else "scatter_diag"
    k = _check_resp(xp, resp, name)
    n, ld = _sizes(xp, d, k, name)
    require_gpu(mean)
    if mean.shape != (k, d) or mean.dtype != torch.float64:
        raise ValueError(f"{name}: mean float64 [k, d] expected")
    lib = _lib.load()
    need = getattr(lib, f"wm_gmm_{name}_workspace_bytes")(n, d, ld, k)
    ws = workspace(need, f"{name} n={n} d={d} k={k}: unsupported sizes (reduce the matrix first)", xp.device)
    out = torch.empty((k, d, d) if full else (k, d), dtype=torch.float64, device=xp.device)
    check(getattr(lib, f"wm_gmm_{name}")(ptr(xp), n, d, ld, ptr(resp), k, ptr(mean), ptr(out), ptr(ws), need, stream_ptr()),
          f"wm_gmm_{name}")
    return out


def _scatter_diag(xp, d: int, resp, mean):
    """out[c][f] = sum_i resp[i][c] * (x[i][f] - mean[c][f])^2; float64 [k, d]."""
    return _scatter(xp, d, resp, mean, False)


def _scatter_full(xp, d: int, resp, mean):
    """out[c] = sum_i resp[i][c] (x_i - mean_c)(x_i - mean_c)^T; float64 [k, d, d], symmetric bit for bit."""
    return _scatter(xp, d, resp, mean, True)


# ------------------------------------------------------------------------------------------------ host helpers


def precision_cholesky(covariances, covariance_type: str) -> np.ndarray:
    """sklearn's _compute_precision_cholesky in numpy / scipy float64.  full: per component the upper triangular P with
    Sigma^-1 = P P^T (the transposed inverse of the lower Cholesky factor of Sigma); diag / spherical: 1 / sqrt(cov).  A
    matrix that is not positive definite raises ValueError with sklearn's message."""
    from scipy import linalg

    _check_covariance_type(covariance_type)
    cov = np.asarray(covariances, dtype=np.float64)
    if covariance_type == "full":
        if cov.ndim != 3 or cov.shape[1] != cov.shape[2]:
            raise ValueError("covariances [n_components, n_features, n_features] expected")
        k, d, _ = cov.shape
        out = np.empty((k, d, d), dtype=np.float64)
        eye = np.eye(d)
        for c in range(k):
            try:
                low = linalg.cholesky(cov[c], lower=True)
            except (linalg.LinAlgError, ValueError):
                raise ValueError(_ILL_DEFINED) from None
            out[c] = linalg.solve_triangular(low, eye, lower=True).T
        return out
    if not np.isfinite(cov).all() or np.any(cov <= 0.0):
        raise ValueError(_ILL_DEFINED)
    return 1.0 / np.sqrt(cov)


def _log_det_cholesky(pchol: np.ndarray, covariance_type: str, d: int) -> np.ndarray:
    if covariance_type == "full":
        return np.log(np.diagonal(pchol, axis1=1, axis2=2)).sum(axis=1)
    if covariance_type == "diag":
        return np.log(pchol).sum(axis=1)
    return d * np.log(pchol)


def n_parameters(k: int, d: int, covariance_type: str) -> int:
    """The number of free parameters of a k-component mixture in d dimensions (sklearn's _n_parameters)."""
    _check_covariance_type(covariance_type)
    cov = {"full": k * d * (d + 1) / 2.0, "diag": k * d, "spherical": k}[covariance_type]
    return int(cov + d * k + k - 1)


def gmm_converged(lb: float, prev: float, tol: float) -> bool:
    """sklearn's stopping rule: abs(lb - prev) < tol (never true on the first iteration, where prev is -inf)."""
    return bool(abs(lb - prev) < tol)


def _cov_shape(k: int, d: int, covariance_type: str):
    return {"full": (k, d, d), "diag": (k, d), "spherical": (k,)}[covariance_type]


# ------------------------------------------------------------------------------------------------ the two half-steps


def _e_step(xp, d: int, weights: np.ndarray, means: np.ndarray, pchol: np.ndarray, covariance_type: str):
    """(lpn [n], resp [n, k], labels int32 [n], lpn_sum [1]) on the device from host float64 parameters."""
    k = means.shape[0]
    cst = np.log(weights) - 0.5 * d * math.log(2.0 * math.pi) + _log_det_cholesky(pchol, covariance_type, d)
    dev = xp.device
    if covariance_type == "full":
        wlp = _logprob_full(xp, d, _f64(means, dev), _f64(pchol, dev), _f64(cst, dev))
    else:
        inv_var = pchol ** 2 if covariance_type == "diag" else np.broadcast_to((pchol ** 2)[:, None], (k, d))
        wlp = _logprob_diag(xp, d, _f64(means, dev), _f64(inv_var, dev), _f64(cst, dev))
    lpn, labels, total = _normalize(wlp)
    return lpn, wlp, labels, total


def _estimate(xp, d: int, resp, covariance_type: str, reg_covar: float):
    """(nk [k] with sklearn's 10 eps added, means [k, d], covariances) as float64 device tensors: the weighted sums, then
    the scatter centred on the new means."""
    nk, sx = _weighted_sums(xp, d, resp)
    nk = nk + _EPS10
    means = (sx / nk[:, None]).contiguous()
    if covariance_type == "full":
        cov = _scatter_full(xp, d, resp, means) / nk[:, None, None]
        cov.diagonal(dim1=1, dim2=2).add_(reg_covar)
    else:
        cov = _scatter_diag(xp, d, resp, means) / nk[:, None] + reg_covar
        if covariance_type == "spherical":
            cov = cov.mean(dim=1)
    return nk, means, cov.contiguous()


def gmm_e_step(x, weights, means, covariances, covariance_type: str, precisions_cholesky=None):
    """One E-step on the rows x [n, d] (device tensor; fitted or new rows): (log_prob_norm float64 [n], resp float64
    [n, k], labels int32 [n]) on the device.  The parameters are numpy arrays or tensors, used as float64; with
    `precisions_cholesky` the covariances are not looked at."""
    _check_covariance_type(covariance_type)
    xp, d = _prep(x, covariance_type)

    def host(v):
        return v.detach().cpu().numpy().astype(np.float64) if hasattr(v, "detach") else np.asarray(v, dtype=np.float64)

    w, mu = host(weights), host(means)
    if mu.ndim != 2 or mu.shape[1] != d or w.shape != (mu.shape[0],):
        raise ValueError(f"weights [k] and means [k, {d}] expected")
    k = mu.shape[0]
    pchol = precision_cholesky(host(covariances), covariance_type) if precisions_cholesky is None else host(precisions_cholesky)
    if pchol.shape != _cov_shape(k, d, covariance_type):
        raise ValueError(f"covariances / precisions_cholesky: shape {_cov_shape(k, d, covariance_type)} expected")
    lpn, resp, labels, _ = _e_step(xp, d, w, mu, pchol, covariance_type)
    return lpn, resp, labels


def gmm_m_step(x, resp, covariance_type: str, reg_covar: float = 1e-6):
    """One M-step: (weights [k], means [k, d], covariances) as float64 device tensors from the rows x [n, d] and the
    responsibilities resp float64 [n, k] (device tensors).  weights = nk / n divided by their sum."""
    import torch

    _check_covariance_type(covariance_type)
    if float(reg_covar) < 0:
        raise ValueError("reg_covar >= 0 required")
    xp, d = _prep(x, covariance_type)
    nk, means, cov = _estimate(xp, d, resp.contiguous(), covariance_type, float(reg_covar))
    w = nk / torch.tensor(float(xp.shape[0]), dtype=torch.float64, device=xp.device)
    return w / w.sum(), means, cov


# ------------------------------------------------------------------------------------------------ the estimator


class GaussianMixture:
    """sklearn.mixture.GaussianMixture on device tensors: `fit`, `fit_predict`, `predict`, `predict_proba`,
    `score_samples`, `score`, `bic`, `aic` and the attributes `weights_`, `means_`, `covariances_`, `precisions_`,
    `precisions_cholesky_` (numpy float64), `converged_`, `n_iter_`, `lower_bound_`, `lower_bounds_` (the kept run's
    list), `n_features_in_`, and (an extension) `lower_bounds_all_`, the last bound of every initialisation.  `predict`
    returns numpy labels; `predict_proba` and `score_samples` float64 device tensors.

    The loop is sklearn's fit_predict: per initialisation lb = -inf, then E-step (which gives lb), M-step, stop when
    abs(lb - prev) < tol; `lower_bound_` is the bound of the last E-step, computed with the parameters before the last
    M-step.  The kept initialisation is the one of the largest bound.  Initial responsibilities: "kmeans" one-hot labels
    of cluster.KMeans(k, n_init=1); "k-means++" one-hot only at the k rows cluster.kmeans_plusplus returns;
    "random_from_data" one-hot only at k rows drawn without replacement; one M-step from them, then `weights_init`,
    `means_init` and `precisions_init` override their parts (sklearn's _initialize)."""

    def __init__(self, n_components: int = 1, *, covariance_type: str = "full", tol: float = 1e-3, reg_covar: float = 1e-6,
                 max_iter: int = 100, n_init: int = 1, init_params: str = "kmeans", weights_init=None, means_init=None,
                 precisions_init=None, random_state=None):
        _check_covariance_type(covariance_type)
        if int(n_components) < 1:
            raise ValueError("n_components must be at least 1")
        if int(n_components) > MAX_COMPONENTS:
            raise ValueError(f"n_components must be at most {MAX_COMPONENTS}")
        if init_params not in INIT_PARAMS:
            raise ValueError(f"init_params={init_params!r} is not available (available: " + ", ".join(INIT_PARAMS) + ")")
        if float(tol) < 0 or float(reg_covar) < 0:
            raise ValueError("tol >= 0 and reg_covar >= 0 required")
        if int(max_iter) < 1 or int(n_init) < 1:
            raise ValueError("max_iter >= 1 and n_init >= 1 required")
        self.n_components, self.covariance_type = int(n_components), covariance_type
        self.tol, self.reg_covar, self.max_iter, self.n_init = float(tol), float(reg_covar), int(max_iter), int(n_init)
        self.init_params, self.random_state = init_params, random_state
        k = self.n_components
        self.weights_init = None if weights_init is None else np.asarray(weights_init, dtype=np.float64)
        self.means_init = None if means_init is None else np.asarray(means_init, dtype=np.float64)
        self.precisions_init = None if precisions_init is None else np.asarray(precisions_init, dtype=np.float64)
        if self.weights_init is not None and self.weights_init.shape != (k,):
            raise ValueError(f"weights_init: shape ({k},) expected, {self.weights_init.shape} given")
        if self.means_init is not None and (self.means_init.ndim != 2 or self.means_init.shape[0] != k):
            raise ValueError(f"means_init: shape ({k}, n_features) expected, {self.means_init.shape} given")
        if self.precisions_init is not None:
            p = self.precisions_init
            ok = {"full": p.ndim == 3 and p.shape[0] == k and p.shape[1] == p.shape[2],
                  "diag": p.ndim == 2 and p.shape[0] == k, "spherical": p.shape == (k,)}[covariance_type]
            if not ok:
                raise ValueError(f"precisions_init: shape {_cov_shape(k, 'n_features', covariance_type)} expected, {p.shape} given")

    # ---- initialisation

    def _check_init_shapes(self, d: int):
        k = self.n_components
        if self.means_init is not None and self.means_init.shape != (k, d):
            raise ValueError(f"means_init: shape ({k}, {d}) expected, {self.means_init.shape} given")
        if self.precisions_init is not None and self.precisions_init.shape != _cov_shape(k, d, self.covariance_type):
            raise ValueError(f"precisions_init: shape {_cov_shape(k, d, self.covariance_type)} expected, "
                             f"{self.precisions_init.shape} given")

    def _initial_resp(self, x, xp, rng):
        import torch

        from . import cluster

        n, k = xp.shape[0], self.n_components
        resp = torch.zeros((n, k), dtype=torch.float64, device=xp.device)
        cols = torch.arange(k, device=xp.device)
        if self.init_params == "kmeans":
            labels = cluster.KMeans(k, n_init=1, random_state=int(rng.integers(1 << 31))).fit(x).labels_
            resp[torch.arange(n, device=xp.device), torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(xp.device)] = 1.0
        elif self.init_params == "k-means++":
            _, rows = cluster.kmeans_plusplus(x, k, random_state=int(rng.integers(1 << 31)))
            resp[torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(xp.device), cols] = 1.0
        else:
            rows = rng.choice(n, size=k, replace=False)
            resp[torch.from_numpy(rows.astype(np.int64)).to(xp.device), cols] = 1.0
        return resp

    def _initialize(self, x, xp, d: int, rng):
        """(weights, means, covariances or None, precisions_cholesky), numpy float64."""
        ct = self.covariance_type
        if self.weights_init is None or self.means_init is None or self.precisions_init is None:
            nk, means, cov = _estimate(xp, d, self._initial_resp(x, xp, rng), ct, self.reg_covar)
            weights, means, cov = nk.cpu().numpy() / float(xp.shape[0]), means.cpu().numpy(), cov.cpu().numpy()
        else:
            weights = means = cov = None
        if self.weights_init is not None:
            weights = self.weights_init.copy()
        if self.means_init is not None:
            means = self.means_init.copy()
        if self.precisions_init is None:
            return weights, means, cov, precision_cholesky(cov, ct)
        if ct == "full":  # sklearn's _compute_precision_cholesky_from_precisions: U with precision = U U^T
            from scipy import linalg

            pchol = np.empty_like(self.precisions_init)
            for c, prec in enumerate(self.precisions_init):
                try:
                    pchol[c] = linalg.cholesky(prec[::-1, ::-1], lower=True)[::-1, ::-1]
                except (linalg.LinAlgError, ValueError):
                    raise ValueError(_ILL_DEFINED) from None
        else:
            if np.any(self.precisions_init <= 0.0):
                raise ValueError(_ILL_DEFINED)
            pchol = np.sqrt(self.precisions_init)
        return weights, means, None, pchol

    # ---- fitting

    def fit(self, x, y=None) -> "GaussianMixture":
        self.fit_predict(x)
        return self

    def fit_predict(self, x, y=None) -> np.ndarray:
        ct, k = self.covariance_type, self.n_components
        xp, d = _prep(x, ct)
        n = xp.shape[0]
        if n < 2:
            raise ValueError("GaussianMixture needs at least 2 rows")
        if n < k:
            raise ValueError(f"Expected n_samples >= n_components but got n_components = {k}, n_samples = {n}")
        self._check_init_shapes(d)
        rng = np.random.default_rng(self.random_state)
        best = None
        max_lb = -np.inf
        self.converged_ = False
        self.lower_bounds_all_ = []
        for _ in range(self.n_init):
            weights, means, cov, pchol = self._initialize(x, xp, d, rng)
            lb, bounds, converged, n_iter = -np.inf, [], False, 0
            for n_iter in range(1, self.max_iter + 1):
                prev = lb
                _, resp, _, total = _e_step(xp, d, weights, means, pchol, ct)
                nk, means_d, cov_d = _estimate(xp, d, resp, ct, self.reg_covar)
                lb = float(total.cpu()[0]) / n
                bounds.append(lb)
                weights = nk.cpu().numpy() / float(n)
                weights = weights / weights.sum()
                means, cov = means_d.cpu().numpy(), cov_d.cpu().numpy()
                pchol = precision_cholesky(cov, ct)
                if gmm_converged(lb, prev, self.tol):
                    converged = True
                    break
            self.lower_bounds_all_.append(lb)
            if lb > max_lb or max_lb == -np.inf:
                max_lb = lb
                best = (weights, means, cov, pchol, n_iter, bounds, converged)
        weights, means, cov, pchol, n_iter, bounds, converged = best
        self.converged_ = converged
        if not converged:
            try:
                from sklearn.exceptions import ConvergenceWarning as category
            except Exception:  # sklearn is optional
                category = UserWarning
            warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase "
                          "max_iter, tol, or check for degenerate data.", category)
        self.weights_, self.means_, self.covariances_, self.precisions_cholesky_ = weights, means, cov, pchol
        if ct == "full":
            self.precisions_ = np.stack([p @ p.T for p in pchol])
        else:
            self.precisions_ = pchol ** 2
        self.n_iter_, self.lower_bound_, self.lower_bounds_ = n_iter, max_lb, bounds
        self.n_features_in_ = d
        return self._e(xp, d)[2].cpu().numpy()

    # ---- the fitted model on any rows

    def _e(self, xp, d: int):
        return _e_step(xp, d, self.weights_, self.means_, self.precisions_cholesky_, self.covariance_type)

    def _rows(self, x):
        if not hasattr(self, "means_"):
            raise RuntimeError("GaussianMixture: call fit first")
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        return _prep(x, self.covariance_type)

    def predict(self, x) -> np.ndarray:
        return self._e(*self._rows(x))[2].cpu().numpy()

    def predict_proba(self, x):
        return self._e(*self._rows(x))[1]

    def score_samples(self, x):
        return self._e(*self._rows(x))[0]

    def score(self, x, y=None) -> float:
        xp, d = self._rows(x)
        return float(self._e(xp, d)[3].cpu()[0]) / xp.shape[0]

    def _n_parameters(self) -> int:
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    def bic(self, x) -> float:
        n = x.shape[0]
        return -2.0 * self.score(x) * n + self._n_parameters() * math.log(n)

    def aic(self, x) -> float:
        return -2.0 * self.score(x) * x.shape[0] + 2.0 * self._n_parameters()
