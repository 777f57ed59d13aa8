"""PCA of dumped embeddings and the rank diagnostics of their covariance spectrum.

The linear reducer next to `manifold.UMAP`: the tool for "reduce the matrix first" that the all-pairs kernels of
`cluster` and `manifold` ask for (their cost is linear in the feature count), and the measurement of dimensional
collapse of self-supervised embeddings (the covariance spectrum is what the Barlow Twins and VICReg losses act on).

PCA needs only the d x d covariance, one streaming pass over the rows.  The passes over the rows are HIP kernels
(csrc/pca.hip, float64 MFMA tiles with a stated summation order): `column_means`, `covariance`, `project`,
`reconstruct`.  The covariance is centred before it is multiplied (never X^T X - n mu mu^T), accumulated in double, and
symmetric bit for bit.  What runs on the host, in numpy float64, and why: the eigendecomposition of the d x d matrix
(`pca_from_covariance`: numpy.linalg.eigh, small, done once), the sign rule, the choice of the component count and the
diagnostics `effective_rank` / `participation_ratio`.

`PCA` has sklearn.decomposition.PCA's surface and its attributes' meaning (sklearn 1.7): eigenvalues descending and
clipped at 0, signs by svd_flip(u_based_decision=False) (the entry of largest magnitude of every component is
positive), a float `n_components` keeps the smallest count whose cumulative ratio exceeds it.  Whitening scales the
projection matrix on the host, so the kernel has no whitening mode.  `n_components="mle"`, randomised / truncated
solvers and `partial_fit` are not implemented.  `manifold._pca_init` (UMAP's init="pca") does not use this module.
DESIGN.md states the definitions and the error bounds.
"""
from __future__ import annotations

import numbers
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace

MAX_FEATURES = 4096


def _prep(x):
    """Contiguous float32 [n, d padded to a multiple of 4] on the device (zero columns centre to exact zeros)."""
    import torch

    require_gpu(x)
    if x.dim() != 2:
        raise ValueError("expected [n_samples, n_features]")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("at least one row and one feature expected")
    x = x.float()
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))
    if x.shape[1] > MAX_FEATURES:
        raise ValueError(f"at most {MAX_FEATURES} features ({x.shape[1]} given)")
    return x.contiguous()


def _f64_on(v, device, cols: Optional[int] = None):
    """v (numpy or tensor, [d] or [m, d]) as a contiguous float64 tensor on `device`, zero-padded to `cols` columns."""
    import torch

    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)))
    t = t.to(device=device, dtype=torch.float64)
    if cols is not None and t.shape[-1] != cols:
        if t.shape[-1] > cols:
            raise ValueError(f"{t.shape[-1]} features given, {cols} expected")
        t = torch.nn.functional.pad(t, (0, cols - t.shape[-1]))
    return t.contiguous()


def _means(xp):
    import torch

    n, d = xp.shape
    lib = _lib.load()
    need = lib.wm_pca_mean_workspace_bytes(n, d)
    ws = workspace(need, f"column_means n={n} d={d}: unsupported sizes", xp.device)
    mean = torch.empty(d, dtype=torch.float64, device=xp.device)
    check(lib.wm_pca_mean(ptr(xp), n, d, ptr(mean), ptr(ws), need, stream_ptr()), "wm_pca_mean")
    return mean


def _gram(xp, mean):
    import torch

    n, d = xp.shape
    lib = _lib.load()
    need = lib.wm_pca_gram_workspace_bytes(n, d)
    ws = workspace(need, f"covariance n={n} d={d}: unsupported sizes", xp.device)
    out = torch.empty((d, d), dtype=torch.float64, device=xp.device)
    check(lib.wm_pca_gram(ptr(xp), n, d, ptr(mean), ptr(out), ptr(ws), need, stream_ptr()), "wm_pca_gram")
    return out


def _project(xp, w, mean):
    import torch

    (n, d), m = xp.shape, w.shape[0]
    lib = _lib.load()
    need = lib.wm_pca_project_workspace_bytes(n, d, m)
    ws = workspace(need, f"project n={n} d={d} m={m}: unsupported sizes", xp.device)
    out = torch.empty((n, m), dtype=torch.float32, device=xp.device)
    check(lib.wm_pca_project(ptr(xp), n, d, ptr(mean), ptr(w), m, ptr(out), ptr(ws), need, stream_ptr()), "wm_pca_project")
    return out


def column_means(x):
    """Column means of x [n, d] (device tensor, any float dtype, used as float32): float64 [d] on the device, summed in
    double in a fixed order (csrc/pca.hip)."""
    d = x.shape[1] if x.dim() == 2 else 0
    return _means(_prep(x))[:d].contiguous()


def gram(x, mean=None):
    """sum_i (x_i - mean)(x_i - mean)^T as float64 [d, d] on the device; mean None: the raw second-moment matrix."""
    d = x.shape[1] if x.dim() == 2 else 0
    xp = _prep(x)
    mp = None if mean is None else _f64_on(mean, xp.device, xp.shape[1])
    if mp is not None and mp.shape != (xp.shape[1],):
        raise ValueError("mean [n_features] expected")
    return _gram(xp, mp)[:d, :d].contiguous()


def covariance(x, center: bool = True, ddof: int = 1) -> Tuple[object, object]:
    """(mean float64 [d], cov float64 [d, d]) of the rows of x on the device: cov = gram(x, mean) / (n - ddof), exactly
    symmetric.  center=False: mean is zeros and cov the second-moment matrix over n - ddof."""
    import torch

    d = x.shape[1] if x.dim() == 2 else 0
    xp = _prep(x)
    n = xp.shape[0]
    if n - int(ddof) <= 0:
        raise ValueError(f"n_samples ({n}) must exceed ddof ({ddof})")
    mean = _means(xp) if center else None
    # (a tensor divisor: torch divides by a Python scalar on the device as a multiplication by its reciprocal, which is
    # one more rounding than the correctly rounded quotient this returns)
    cov = _gram(xp, mean)[:d, :d] / torch.tensor(float(n - int(ddof)), dtype=torch.float64, device=xp.device)
    if mean is None:
        mean = torch.zeros(xp.shape[1], dtype=torch.float64, device=xp.device)
    return mean[:d].contiguous(), cov.contiguous()


def project(x, components, mean=None):
    """(x - mean) W^T as float32 [n, m] on the device: x [n, d], W = components [m, d] (numpy or tensor, used as float64),
    accumulated in double and rounded once."""
    xp = _prep(x)
    d = xp.shape[1]
    w = _f64_on(components, xp.device, d)
    if w.dim() != 2 or not 1 <= w.shape[0] <= d:
        raise ValueError(f"components [m, n_features] with 1 <= m <= {d} expected")
    return _project(xp, w, None if mean is None else _f64_on(mean, xp.device, d))


def reconstruct(y, components, mean=None):
    """y W + mean as float32 [n, d] on the device: y [n, m], W = components [m, d] as float64."""
    import torch

    require_gpu(y)
    if y.dim() != 2:
        raise ValueError("expected [n_samples, n_components]")
    y = y.float().contiguous()
    n, m = y.shape
    comp = components if isinstance(components, torch.Tensor) else np.asarray(components)
    if comp.ndim != 2 or comp.shape[0] != m:
        raise ValueError(f"components [{m}, n_features] expected")
    d = int(comp.shape[1])
    dp = d + (-d) % 4
    if dp > MAX_FEATURES:
        raise ValueError(f"at most {MAX_FEATURES} features ({dp} given)")
    w = _f64_on(comp, y.device, dp)
    mp = None if mean is None else _f64_on(mean, y.device, dp)
    lib = _lib.load()
    need = lib.wm_pca_reconstruct_workspace_bytes(n, m, dp)
    ws = workspace(need, f"reconstruct n={n} m={m} d={dp}: unsupported sizes", y.device)
    out = torch.empty((n, dp), dtype=torch.float32, device=y.device)
    check(lib.wm_pca_reconstruct(ptr(y), n, m, ptr(w), dp, ptr(mp), ptr(out), ptr(ws), need, stream_ptr()),
          "wm_pca_reconstruct")
    return out if dp == d else out[:, :d].contiguous()


# ------------------------------------------------------------------------------------------------ host


class PCAResult(NamedTuple):
    components: np.ndarray                # [m, d], rows of unit length, largest-magnitude entry positive
    explained_variance: np.ndarray        # [m], descending, >= 0
    explained_variance_ratio: np.ndarray  # [m], of the total variance
    singular_values: np.ndarray           # [m], sqrt(explained_variance * (n - 1))
    noise_variance: float                 # mean of the eigenvalues left out (0 when none is)
    n_components: int
    all_variances: np.ndarray             # the min(n, d) leading eigenvalues, for spectra and diagnostics


def _check_n_components(n_components, limit: int):
    if isinstance(n_components, str):
        if n_components == "mle":
            raise NotImplementedError('n_components="mle" is not implemented (an int, a float in (0, 1) or None)')
        raise ValueError(f"n_components={n_components!r}: an int, a float in (0, 1) or None expected")
    if n_components is None:
        return
    if isinstance(n_components, (bool, np.bool_)):
        raise ValueError("n_components must be an int, a float in (0, 1) or None")
    if isinstance(n_components, numbers.Integral):
        if limit and not 1 <= n_components <= limit:
            raise ValueError(f"n_components={n_components} must be in [1, min(n_samples, n_features) = {limit}]")
        if n_components < 1:
            raise ValueError(f"n_components={n_components} must be at least 1")
        return
    if isinstance(n_components, numbers.Real):
        if not 0.0 < n_components < 1.0:
            raise ValueError(f"n_components={n_components}: a float must be in (0, 1)")
        return
    raise ValueError(f"n_components={n_components!r}: an int, a float in (0, 1) or None expected")


def pca_from_covariance(cov, n_samples: int, n_components=None) -> PCAResult:
    """Principal components from a covariance matrix (numpy float64 [d, d], symmetric, divided by n_samples - 1), by
    numpy.linalg.eigh.  Eigenvalues descending, clipped at 0; the largest-magnitude entry of every component positive
    (the first such entry where several tie).  n_components: an int in [1, min(n_samples, d)], a float in (0, 1) (the
    smallest count whose cumulative variance ratio exceeds it), or None (min(n_samples, d))."""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
        raise ValueError("a square covariance matrix expected")
    n = int(n_samples)
    if n < 2:
        raise ValueError(f"n_samples ({n_samples}) must be at least 2")
    d = cov.shape[0]
    limit = min(n, d)
    _check_n_components(n_components, limit)
    vals, vecs = np.linalg.eigh(cov)
    vals, vecs = vals[::-1], vecs[:, ::-1]
    vals = np.where(vals > 0.0, vals, 0.0)[:limit]
    comps = np.ascontiguousarray(vecs.T[:limit])
    lead = np.argmax(np.abs(comps), axis=1)
    signs = np.sign(comps[np.arange(limit), lead])
    signs[signs == 0] = 1.0
    comps *= signs[:, None]
    total = vals.sum()
    ratio = vals / total if total > 0 else np.zeros_like(vals)
    if n_components is None:
        m = limit
    elif isinstance(n_components, numbers.Integral):
        m = int(n_components)
    else:
        m = min(int(np.searchsorted(np.cumsum(ratio), n_components, side="right")) + 1, limit)
    noise = float(vals[m:].mean()) if m < limit else 0.0
    return PCAResult(comps[:m].copy(), vals[:m].copy(), ratio[:m].copy(), np.sqrt(vals[:m] * (n - 1)), noise, m, vals)


def _positive_spectrum(explained_variance) -> np.ndarray:
    v = np.asarray(explained_variance, dtype=np.float64).ravel()
    if v.size == 0 or not np.isfinite(v).all() or (v < 0).any():
        raise ValueError("a non-empty spectrum of finite, non-negative eigenvalues expected")
    v = v[v > 0]
    if v.size == 0:
        raise ValueError("the spectrum has no positive eigenvalue")
    return v


def effective_rank(explained_variance) -> float:
    """exp of the entropy of the normalised positive eigenvalues (Roy & Vetterli's effective rank; RankMe): k equal
    eigenvalues give k, a single one gives 1."""
    v = _positive_spectrum(explained_variance)
    p = v / v.sum()
    return float(np.exp(-(p * np.log(p)).sum()))


def participation_ratio(explained_variance) -> float:
    """(sum l)^2 / sum l^2 of the eigenvalues: k equal ones give k, a single one gives 1."""
    v = _positive_spectrum(explained_variance)
    return float(v.sum() ** 2 / (v * v).sum())


class PCA:
    """sklearn.decomposition.PCA on device tensors: `fit`, `transform`, `fit_transform`, `inverse_transform` and the
    attributes `components_`, `explained_variance_`, `explained_variance_ratio_`, `singular_values_`, `mean_` (numpy
    float64), `n_components_`, `n_samples_`, `n_features_in_`, `noise_variance_`, and `get_covariance()`.  `spectrum_`
    holds all min(n, d) eigenvalues and `covariance_` the sample covariance [d, d] they were taken from.  transform /
    inverse_transform return float32 device tensors."""

    def __init__(self, n_components=None, whiten: bool = False):
        _check_n_components(n_components, 0)
        self.n_components = n_components
        self.whiten = bool(whiten)

    def fit(self, x, y=None) -> "PCA":
        self._fit(x)
        return self

    def _fit(self, x):
        xp = _prep(x)
        d = x.shape[1]
        n = xp.shape[0]
        if n < 2:
            raise ValueError("PCA needs at least 2 rows")
        mean = _means(xp)
        cov = _gram(xp, mean)[:d, :d].cpu().numpy() / float(n - 1)  # (the host divides: the correctly rounded quotient)
        res = pca_from_covariance(cov, n, self.n_components)
        self.components_ = res.components
        self.explained_variance_ = res.explained_variance
        self.explained_variance_ratio_ = res.explained_variance_ratio
        self.singular_values_ = res.singular_values
        self.noise_variance_ = res.noise_variance
        self.n_components_ = res.n_components
        self.spectrum_ = res.all_variances
        self.covariance_ = cov
        self.mean_ = mean[:d].cpu().numpy()
        self.n_samples_, self.n_features_in_ = n, d
        dp = xp.shape[1]
        self._mean_dev = mean  # (padded; the padding columns are exact zeros)
        self._w_dev = _f64_on(self._forward_matrix(), xp.device, dp)
        self._w_back_dev = _f64_on(self._backward_matrix(), xp.device, dp)
        return xp

    def _scale(self) -> np.ndarray:
        s = np.sqrt(self.explained_variance_)
        return np.maximum(s, np.finfo(np.float64).eps)  # sklearn's floor

    def _forward_matrix(self) -> np.ndarray:
        return self.components_ / self._scale()[:, None] if self.whiten else self.components_

    def _backward_matrix(self) -> np.ndarray:
        return np.sqrt(self.explained_variance_)[:, None] * self.components_ if self.whiten else self.components_

    def _check_fitted(self):
        if not hasattr(self, "components_"):
            raise RuntimeError("PCA: call fit before transform / inverse_transform")

    def transform(self, x):
        self._check_fitted()
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        xp = _prep(x)
        if xp.device != self._w_dev.device:
            raise _lib.WaferHipError("the rows are not on the device the model was fitted on")
        return _project(xp, self._w_dev, self._mean_dev)

    def fit_transform(self, x, y=None):
        return _project(self._fit(x), self._w_dev, self._mean_dev)

    def inverse_transform(self, y):
        self._check_fitted()
        require_gpu(y)
        if y.dim() != 2 or y.shape[1] != self.n_components_:
            raise ValueError(f"[n_samples, {self.n_components_}] expected")
        d = self.n_features_in_
        out = reconstruct(y, self._w_back_dev, self._mean_dev)
        return out if out.shape[1] == d else out[:, :d].contiguous()

    def get_covariance(self) -> np.ndarray:
        """components_^T diag(max(explained_variance_ - noise_variance_, 0)) components_ + noise_variance_ I, as
        sklearn computes it (with whiten=True sklearn scales the components by sqrt(explained_variance_) first; so
        does this)."""
        self._check_fitted()
        comps, ev = self.components_, self.explained_variance_
        if self.whiten:
            comps = comps * np.sqrt(ev)[:, None]
        diff = np.where(ev > self.noise_variance_, ev - self.noise_variance_, 0.0)
        cov = (comps.T * diff) @ comps
        cov.flat[:: cov.shape[0] + 1] += self.noise_variance_
        return cov
