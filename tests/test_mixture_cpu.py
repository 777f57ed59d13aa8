"""CPU checks of mixture.py: the C entry points refuse bad arguments without a launch, Python validates before the
library is touched, the host helpers against float64 restatements (and sklearn's private ones where importable), and
`em64`, the straight-line numpy restatement of the EM loop that the GPU tests compare whole fits with.

`em64` against sklearn.mixture.GaussianMixture, started from the same weights, means and precisions: per quantity q the
difference, relative to max |q|, is bounded by
    16 * |em64(float64) - em64(long double)| / max |q|  +  n_iter * (d + k + 8) * 2^-53.
The long-double run measures how far float64 rounding moves THIS trajectory (EM amplifies a rounding through every later
iteration, so no a-priori figure exists); 16 covers another summation order of the same float64 arithmetic (BLAS
products, sklearn's uncentred x P - mu P and one-pass diag covariances); the floor is one rounding per term of the
longest sum, per iteration, for quantities the two float64 runs happen to agree on.  Measured here (k = 5, d = 16, 2000
rows; relative differences over weights, means, covariances, bound; diag and full, 5 and 20 iterations):
    em64 float64 vs long double   6e-17 .. 1e-12, and 5.7e-10 for the bound of full at 5 iterations
    sklearn vs em64 float64       0     .. 8e-13, and 4.7e-10 for that bound
(full at 5 iterations passes through a badly conditioned covariance, which both float64 runs feel alike and have left
behind by iteration 20: 4e-14 there.)  The largest ratio of the second to the first is 6.5, the diag covariances at 5
iterations (1.0e-14 against 1.6e-15: sklearn's one-pass form against the centred one).
"""
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
KERNELS = ["wm_gmm_logprob_diag", "wm_gmm_logprob_full", "wm_gmm_normalize", "wm_gmm_weighted_sums", "wm_gmm_scatter_diag",
           "wm_gmm_scatter_full"]
EPS10 = 10.0 * np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ the restatement


def chol_inv_upper(cov):
    """P upper triangular with cov^-1 = P P^T, in cov's dtype (numpy.linalg has no long double): the lower Cholesky
    factor by columns, its inverse by forward substitution, transposed.  Raises ValueError on a non-positive pivot."""
    d = cov.shape[0]
    low = np.zeros_like(cov)
    for j in range(d):
        s = cov[j, j] - (low[j, :j] * low[j, :j]).sum()
        if not s > 0:
            raise ValueError("not positive definite")
        low[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            low[i, j] = (cov[i, j] - (low[i, :j] * low[j, :j]).sum()) / low[j, j]
    inv = np.zeros_like(cov)
    for c in range(d):
        for i in range(c, d):
            rhs = (1 if i == c else 0) - (low[i, c:i] * inv[c:i, c]).sum()
            inv[i, c] = rhs / low[i, i]
    return inv.T


def ref_pchol(cov, ct):
    if ct == "full":
        return np.stack([chol_inv_upper(c) for c in cov])
    return 1 / np.sqrt(cov)


def ref_e_step(x, w, mu, cov, ct):
    """(lpn [n], resp [n, k]) in x's dtype; the row is centred before it is multiplied."""
    n, d = x.shape
    k = mu.shape[0]
    p = ref_pchol(cov, ct)
    wlp = np.empty((n, k), dtype=x.dtype)
    two_pi = 2 * np.arccos(x.dtype.type(-1))
    for c in range(k):
        diff = x - mu[c]
        if ct == "full":
            y = diff @ p[c]
            maha, logdet = (y * y).sum(1), np.log(np.diagonal(p[c])).sum()
        elif ct == "diag":
            maha, logdet = (diff * diff * (p[c] * p[c])).sum(1), np.log(p[c]).sum()
        else:
            maha, logdet = (diff * diff).sum(1) * (p[c] * p[c]), d * np.log(p[c])
        wlp[:, c] = np.log(w[c]) - (d * np.log(two_pi) + maha) / 2 + logdet
    m = wlp.max(1)
    lpn = m + np.log(np.exp(wlp - m[:, None]).sum(1))
    return lpn, np.exp(wlp - lpn[:, None])


def ref_m_step(x, resp, ct, reg_covar):
    """(weights, means, covariances): sums first, then the scatter centred on the new mean."""
    n, d = x.shape
    nk = resp.sum(0) + x.dtype.type(EPS10)
    mu = (resp.T @ x) / nk[:, None]
    k = nk.shape[0]
    if ct == "full":
        cov = np.empty((k, d, d), dtype=x.dtype)
        for c in range(k):
            diff = x - mu[c]
            cov[c] = (resp[:, c, None] * diff).T @ diff / nk[c]
            cov[c].flat[:: d + 1] += x.dtype.type(reg_covar)
    else:
        cov = np.stack([(resp[:, c, None] * (x - mu[c]) ** 2).sum(0) / nk[c] for c in range(k)]) + x.dtype.type(reg_covar)
        if ct == "spherical":
            cov = cov.mean(1)
    w = nk / n
    return w / w.sum(), mu, cov


def em64(x, weights, means, covariances, covariance_type, n_iter, reg_covar, dtype, tol=None):
    """The loop of mixture.GaussianMixture for one initialisation, straight-line numpy in `dtype`.  Returns a dict:
    weights, means, covariances after the last M-step; lower_bounds, one per E-step (the last one belongs to the
    parameters BEFORE the last M-step); n_iter.  With `tol` the loop stops as sklearn's does."""
    x = np.asarray(x, dtype=dtype)
    w, mu, cov = (np.asarray(v, dtype=dtype) for v in (weights, means, covariances))
    lb, bounds, done = -np.inf, [], 0
    for done in range(1, n_iter + 1):
        prev = lb
        lpn, resp = ref_e_step(x, w, mu, cov, covariance_type)
        lb = lpn.mean()
        bounds.append(lb)
        w, mu, cov = ref_m_step(x, resp, covariance_type, reg_covar)
        if tol is not None and abs(lb - prev) < tol:
            break
    return {"weights": w, "means": mu, "covariances": cov, "lower_bounds": bounds, "n_iter": done}


def fit_input(rows=2000, dims=16):
    """The shared input of the whole-fit comparisons: the golden embeddings standardised, PCA to `dims` dimensions in
    numpy float64, rounded to float32 (what the device gets), the first `rows` rows; returned as float64."""
    e = np.load(GOLDEN / "simsiam_preds_subset.npz")["embeddings"].astype(np.float64)
    s = e.std(0)
    e = (e - e.mean(0)) / np.where(s > 0, s, 1.0)  # (a constant column keeps scale 1, as StandardScaler does)
    vals, vecs = np.linalg.eigh(np.cov(e, rowvar=False))
    y = (e @ vecs[:, ::-1][:, :dims]).astype(np.float32)
    return y[:rows].astype(np.float64), y[rows:rows + 100].astype(np.float64)


def fit_init(x, k, ct):
    """(weights, means, covariances, precisions): k spread rows as means, the global per-feature variances."""
    n, d = x.shape
    means = x[np.linspace(0, n - 1, k).astype(int)].copy()
    var = x.var(0)
    weights = np.full(k, 1.0 / k)
    if ct == "full":
        cov = np.stack([np.diag(var)] * k)
        prec = np.stack([np.diag(1.0 / var)] * k)
    elif ct == "diag":
        cov = np.stack([var] * k)
        prec = 1.0 / cov
    else:
        cov = np.full(k, var.mean())
        prec = 1.0 / cov
    return weights, means, cov, prec


def stop_input():
    """Three separated blobs of unequal spread (600 x 5, float32 values as float64): from `fit_init` the loop stops on
    tol = 1e-3 at an iteration whose change is far below tol while every earlier change is far above it."""
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((3, 5)) * 6.0
    lab = np.arange(600) % 3
    return (centres[lab] + rng.standard_normal((600, 5)) * (1 + 0.5 * lab[:, None])).astype(np.float32).astype(np.float64)


def stop_reference(ct):
    """(n_iter at which em64 in float64 stops with tol = 1e-3, the |changes| of its bounds from iteration 2 on)."""
    x = stop_input()
    w, mu, cov, _ = fit_init(x, 3, ct)
    run = em64(x, w, mu, cov, ct, 40, 1e-6, np.float64, tol=1e-3)
    return run["n_iter"], np.abs(np.diff([float(b) for b in run["lower_bounds"]]))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / np.abs(b).max())


def fit_bound(f64, ld, key, n_iter, d, k):
    """The bound rule of this file's docstring for quantity `key` (lower_bound: the last E-step's)."""
    pick = (lambda r: r["lower_bounds"][-1]) if key == "lower_bound" else (lambda r: r[key])
    return 16.0 * rel(pick(f64), pick(ld)) + n_iter * (d + k + 8) * 2.0 ** -53


_CACHE = {}


def reference_runs(ct, n_iter):
    """em64 in float64 and in long double on the shared input, computed once per session."""
    key = (ct, n_iter)
    if key not in _CACHE:
        x, _ = fit_input()
        w, mu, cov, _ = fit_init(x, 5, ct)
        _CACHE[key] = tuple(em64(x, w, mu, cov, ct, n_iter, 1e-6, dt) for dt in (np.float64, np.longdouble))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the C boundary


def test_new_symbols_are_declared_and_typed():
    from ssl_wafermap_amd import _lib

    header = (ROOT / "include" / "wafer_hip.h").read_text()
    lib = _lib.load()
    for name in KERNELS:
        for sym in (name, name + "_workspace_bytes"):
            assert re.search(rf"\b{sym}\s*\(", header), f"{sym} is not declared in wafer_hip.h"
            assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        assert _lib.SIGNATURES[name][1][-3:] == [_lib.c_void_p, _lib.c_size_t, _lib.c_void_p]
    assert lib.wm_version() == 4


def test_entry_points_refuse_without_a_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    ws = {n: getattr(lib, n + "_workspace_bytes") for n in KERNELS}
    for name in KERNELS:
        if name == "wm_gmm_normalize":
            continue
        fn, dmax = ws[name], 256 if name.endswith("_full") else 1024
        assert fn(1, 1, 4, 1) > 0 and fn(12449, 50, 52, 50) > 0 and fn(1 << 24, dmax, dmax, 1024) > 0
        assert fn(0, 50, 52, 5) == 0 and fn((1 << 24) + 1, 50, 52, 5) == 0          # n
        assert fn(100, 0, 4, 5) == 0 and fn(100, dmax + 1, dmax + 4, 5) == 0        # d
        assert fn(100, 50, 50, 5) == 0 and fn(100, 50, 48, 5) == 0                  # ld % 4, ld >= d
        assert fn(100, 50, 52, 0) == 0 and fn(100, 50, 52, 1025) == 0               # k
        assert fn(1 << 24, dmax, dmax, 1024) <= 256 << 20                           # the workspace cap
    fn = ws["wm_gmm_normalize"]
    assert fn(1, 1) == 8 and fn(257, 50) == 16 and fn(1 << 24, 1024) > 0
    assert fn(0, 5) == 0 and fn((1 << 24) + 1, 5) == 0 and fn(10, 0) == 0 and fn(10, 1025) == 0
    # the slice rules are functions of (n, d) alone: the same planes per component for every k
    assert ws["wm_gmm_weighted_sums"](65600, 4, 4, 7) == 7 * ws["wm_gmm_weighted_sums"](65600, 4, 4, 1)
    assert ws["wm_gmm_scatter_diag"](65600, 4, 4, 7) == 7 * ws["wm_gmm_scatter_diag"](65600, 4, 4, 1)
    assert ws["wm_gmm_scatter_full"](65600, 4, 4, 7) == 7 * ws["wm_gmm_scatter_full"](65600, 4, 4, 1)
    # null pointers and bad sizes: WM_EINVAL before any launch (a fake non-null pointer where sizes are probed)
    p = 4096
    assert lib.wm_gmm_logprob_diag(None, 8, 4, 4, None, None, None, 2, None, None, 0, None) == -1
    assert lib.wm_gmm_logprob_diag(p, 0, 4, 4, p, p, p, 2, p, p, 256, None) == -1
    assert lib.wm_gmm_logprob_diag(p, 8, 4, 0, p, p, p, 2, p, p, 256, None) == -1
    assert lib.wm_gmm_logprob_full(None, 8, 4, 4, None, None, None, 2, None, None, 0, None) == -1
    assert lib.wm_gmm_logprob_full(p, 8, 4, 4, p, p, p, 0, p, p, 256, None) == -1
    assert lib.wm_gmm_normalize(None, 8, 2, None, None, None, None, 0, None) == -1
    assert lib.wm_gmm_normalize(p, 8, 0, p, p, p, p, 8, None) == -1
    for name in ("wm_gmm_scatter_diag", "wm_gmm_scatter_full"):
        assert getattr(lib, name)(None, 8, 4, 4, None, 2, None, None, None, 0, None) == -1
        assert getattr(lib, name)(p, 8, 0, 4, p, 2, p, p, p, 1 << 20, None) == -1
    assert lib.wm_gmm_weighted_sums(None, 8, 4, 4, None, 2, None, None, None, 0, None) == -1
    assert lib.wm_gmm_weighted_sums(p, -1, 4, 4, p, 2, p, p, p, 1 << 20, None) == -1
    # the other codes, still without a launch: unsupported sizes, a short workspace, a misaligned pointer
    assert lib.wm_gmm_logprob_full(p, 8, 300, 300, p, p, p, 2, p, p, 256, None) == -2
    assert lib.wm_gmm_scatter_diag(p, 8, 1025, 1028, p, 2, p, p, p, 1 << 20, None) == -2
    assert lib.wm_gmm_scatter_full(p, 8, 4, 4, p, 2, p, p, p, 8, None) == -3
    assert lib.wm_gmm_normalize(p, 300, 2, p, p, p, p, 8, None) == -3
    assert lib.wm_gmm_weighted_sums(p + 4, 8, 4, 4, p, 2, p, p, p, 1 << 20, None) == -4
    assert lib.wm_gmm_logprob_diag(p, 8, 4, 4, p + 4, p, p, 2, p, p, 256, None) == -4


# ------------------------------------------------------------------------------------------------ Python validation


def test_argument_errors_come_before_the_library(monkeypatch):
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd import mixture as M

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(NotImplementedError, match="tied"):
        M.GaussianMixture(2, covariance_type="tied")
    with pytest.raises(NotImplementedError, match="tied"):
        M.n_parameters(2, 3, "tied")
    with pytest.raises(ValueError, match="available"):
        M.GaussianMixture(2, covariance_type="oval")
    with pytest.raises(ValueError, match="kmeans.*k-means\\+\\+.*random_from_data"):
        M.GaussianMixture(2, init_params="random")
    for kw in ({"n_components": 0}, {"n_components": -3}, {"tol": -1e-3}, {"reg_covar": -1e-6}, {"max_iter": 0}, {"n_init": 0},
               {"n_components": 1025}):
        with pytest.raises(ValueError):
            M.GaussianMixture(**{"n_components": 2, **kw})
    for kw in ({"weights_init": np.ones(3) / 3}, {"means_init": np.zeros((3, 4))}, {"means_init": np.zeros(4)},
               {"precisions_init": np.ones((3, 4))}, {"precisions_init": np.ones((2, 4, 5))}):
        with pytest.raises(ValueError, match="_init"):
            M.GaussianMixture(2, covariance_type="full" if kw.get("precisions_init", np.zeros(0)).ndim == 3 else "diag", **kw)
    with pytest.raises(ValueError, match="precisions_init"):
        M.GaussianMixture(2, covariance_type="spherical", precisions_init=np.ones((2, 4)))
    x = torch.zeros(8, 4)
    with pytest.raises(ValueError, match="reduce the matrix first"):
        M.GaussianMixture(2, covariance_type="full").fit(torch.zeros(8, 257))
    with pytest.raises(ValueError, match="reduce the matrix first"):
        M.GaussianMixture(2, covariance_type="diag").fit(torch.zeros(8, 1025))
    with pytest.raises(ValueError):
        M.GaussianMixture(2).fit(torch.zeros(8))
    w, mu = np.ones(2) / 2, np.zeros((2, 4))
    calls = [lambda: M.GaussianMixture(2).fit(x), lambda: M.GaussianMixture(2, covariance_type="diag").fit_predict(x),
             lambda: M.gmm_e_step(x, w, mu, np.ones((2, 4)), "diag"), lambda: M.gmm_e_step(x, w, mu, np.stack([np.eye(4)] * 2), "full"),
             lambda: M.gmm_m_step(x, torch.zeros(8, 2, dtype=torch.float64), "full"),
             lambda: M._logprob_diag(x, 4, torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2)),
             lambda: M._normalize(torch.zeros(8, 2, dtype=torch.float64)),
             lambda: M._weighted_sums(x, 4, torch.zeros(8, 2, dtype=torch.float64))]
    for call in calls:
        with pytest.raises(_lib.WaferHipError):  # CPU tensors: no fallback, as the rest of the package
            call()
    with pytest.raises(RuntimeError, match="fit"):
        M.GaussianMixture(2).predict(x)
    m = M.GaussianMixture()
    assert (m.n_components, m.covariance_type, m.tol, m.reg_covar, m.max_iter, m.n_init, m.init_params) == \
        (1, "full", 1e-3, 1e-6, 100, 1, "kmeans")


def test_init_shapes_are_checked_against_the_rows(monkeypatch):
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd import mixture as M

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(M, "require_gpu", lambda *t: None)  # (let CPU rows through the device check: nothing is launched)
    monkeypatch.setattr(_lib, "load", no_library)
    x = torch.zeros(8, 4)
    with pytest.raises(ValueError, match="means_init"):
        M.GaussianMixture(2, means_init=np.zeros((2, 5))).fit(x)
    with pytest.raises(ValueError, match="precisions_init"):
        M.GaussianMixture(2, covariance_type="diag", precisions_init=np.ones((2, 5))).fit(x)
    with pytest.raises(ValueError, match="n_samples >= n_components"):
        M.GaussianMixture(9).fit(x)
    with pytest.raises(ValueError, match="weights"):
        M.gmm_e_step(x, np.ones(3) / 3, np.zeros((2, 4)), np.ones((2, 4)), "diag")
    with pytest.raises(ValueError, match="shape"):
        M.gmm_e_step(x, np.ones(2) / 2, np.zeros((2, 4)), np.ones((2, 5)), "diag")


# ------------------------------------------------------------------------------------------------ host helpers


def test_precision_cholesky_and_n_parameters():
    from ssl_wafermap_amd import mixture as M

    rng = np.random.default_rng(3)
    k, d = 4, 7
    a = rng.standard_normal((k, d, 2 * d))
    cov = a @ a.transpose(0, 2, 1) / (2 * d) + 0.1 * np.eye(d)
    p = M.precision_cholesky(cov, "full")
    assert p.shape == (k, d, d) and p.dtype == np.float64
    for c in range(k):
        assert np.array_equal(p[c], np.triu(p[c]))  # upper triangular, exact zeros below
        # Sigma^-1 = P P^T: P^T Sigma P = I within cond(Sigma) * a few eps (cond < 1e3 here)
        assert np.abs(p[c].T @ cov[c] @ p[c] - np.eye(d)).max() <= 1e3 * d * 2.0 ** -52
        ref = chol_inv_upper(cov[c].astype(np.longdouble))
        assert np.abs(p[c] - ref).max() <= 1e3 * d * 2.0 ** -52 * np.abs(ref).max()
    var = rng.uniform(0.5, 2.0, (k, d))
    assert np.array_equal(M.precision_cholesky(var, "diag"), 1.0 / np.sqrt(var))
    assert np.array_equal(M.precision_cholesky(var[:, 0], "spherical"), 1.0 / np.sqrt(var[:, 0]))
    for kk, dd in ((1, 1), (5, 16), (50, 50), (1024, 256)):
        assert M.n_parameters(kk, dd, "full") == kk * dd * (dd + 1) // 2 + kk * dd + kk - 1
        assert M.n_parameters(kk, dd, "diag") == 2 * kk * dd + kk - 1
        assert M.n_parameters(kk, dd, "spherical") == kk + kk * dd + kk - 1
    assert M.gmm_converged(1.0005, 1.0, 1e-3) and not M.gmm_converged(1.002, 1.0, 1e-3)
    assert not M.gmm_converged(-3.0, -np.inf, 1e-3) and not M.gmm_converged(1.0, 1.0, 0.0)
    try:
        from sklearn.mixture import GaussianMixture as Sk
        from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky
    except Exception:
        pytest.skip("sklearn's private helpers are not importable; the restatements above were checked")
    for ct, c in (("full", cov), ("diag", var), ("spherical", var[:, 0])):
        assert np.array_equal(M.precision_cholesky(c, ct), _compute_precision_cholesky(c, ct))  # the same scipy calls
        sk = Sk(k, covariance_type=ct)
        sk.means_ = np.zeros((k, d))
        assert M.n_parameters(k, d, ct) == sk._n_parameters()


def test_ill_defined_covariance_raises_sklearns_message():
    from ssl_wafermap_amd import mixture as M

    bad = np.stack([np.eye(3), np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])])
    for call in (lambda: M.precision_cholesky(bad, "full"), lambda: M.precision_cholesky(np.array([[1.0, 0.0]]), "diag"),
                 lambda: M.precision_cholesky(np.array([1.0, -1.0]), "spherical")):
        with pytest.raises(ValueError, match="ill-defined empirical covariance.*increase reg_covar"):
            call()


# ------------------------------------------------------------------------------------------------ em64 against sklearn


@pytest.mark.parametrize("n_iter", [5, 20])
@pytest.mark.parametrize("ct", ["diag", "full"])
def test_em64_against_sklearn(ct, n_iter):
    from sklearn.mixture import GaussianMixture as Sk

    x, _ = fit_input()
    n, d = x.shape
    k = 5
    w, mu, cov, prec = fit_init(x, k, ct)
    f64, ld = reference_runs(ct, n_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = Sk(k, covariance_type=ct, tol=0.0, max_iter=n_iter, reg_covar=1e-6, weights_init=w, means_init=mu,
                precisions_init=prec).fit(x)
    assert sk.n_iter_ == n_iter == f64["n_iter"] == len(f64["lower_bounds"])
    got = {"weights": sk.weights_, "means": sk.means_, "covariances": sk.covariances_, "lower_bound": sk.lower_bound_}
    for key, val in got.items():
        want = f64["lower_bounds"][-1] if key == "lower_bound" else f64[key]  # the bound BEFORE the last M-step
        err, bound = rel(val, want), fit_bound(f64, ld, key, n_iter, d, k)
        print(f"{ct} it={n_iter} {key}: sklearn vs em64 {err:.3g}, float64 vs long double "
              f"{(bound - n_iter * (d + k + 8) * 2.0 ** -53) / 16:.3g}, bound {bound:.3g}")
        assert err <= bound, (key, err, bound)
    # the bound of the last E-step is NOT the bound of the returned parameters
    after = ref_e_step(x, f64["weights"], f64["means"], f64["covariances"], ct)[0].mean()
    assert abs(after - sk.lower_bound_) > 100 * abs(f64["lower_bounds"][-1] - sk.lower_bound_)


@pytest.mark.parametrize("ct", ["diag", "spherical", "full"])
def test_stop_input_is_far_from_the_tolerance(ct):
    """The GPU test of the stopping rule needs an input on which a rounding cannot move the stop: the change at the stop
    is at least 10 x below tol = 1e-3 and every change before it at least 10 x above."""
    n_iter, changes = stop_reference(ct)
    assert 3 <= n_iter < 40 and len(changes) == n_iter - 1
    assert changes[-1] <= 1e-4 and (changes[:-1] >= 1e-2).all(), changes


def test_fit_input_leaves_no_label_to_chance():
    """The GPU tests compare `predict` with the argmax of the reference responsibilities and may leave out rows whose
    two largest differ by less than 1e-9: on this input the reference leaves out none."""
    x, held = fit_input()
    for ct in ("diag", "spherical", "full"):
        for n_iter in (5, 20):
            ld = reference_runs(ct, n_iter)[1]
            for rows in (x, held):
                resp = ref_e_step(rows.astype(np.longdouble), ld["weights"], ld["means"], ld["covariances"], ct)[1]
                top = np.sort(resp, axis=1)
                assert (top[:, -1] - top[:, -2] >= 1e-9).all()
