"""GPU checks of csrc/gmm.hip and mixture.py.

Exact: on integer lattices (rows and means small integers, inv_var powers of two, P small-integer upper triangular,
responsibilities multiples of 1/8) every product and sum is exact in float64, so numpy restates the results bit for
bit: fragment maps, masks, slice and slab edges, the true-d rule (1e30 in the padding columns of x changes nothing) and
the triangle rule of logprob_full (NaN below the diagonal of P changes nothing).

Against float64 (references in numpy long double), with u = 2^-53, one rounding per centring, product and accumulation
step, and sums of non-negative terms unless said otherwise:
  logprob_diag   a term (x - m)^2 v carries 3 roundings, the d-term sum d more, the final cst - acc / 2 one:
                 |err| <= (d + 3) u S / 2 + u |out|,  S = sum_f (x - m)^2 v.
  logprob_full   y_j = sum_f (x_f - m_f) P_fj over at most d terms, each with the centring's rounding and the
                 accumulation's: |dy_j| <= E_j = (d + 1) u sum_f |x_f - m_f| |P_fj| (cancellation: bounded by the sum
                 of magnitudes, not by y_j); the square one more, the sum over j d more:
                 |err| <= (sum_j (2 |y_j| E_j + E_j^2) + (d + 1) u S) / 2 + u |out|,  S = sum_j y_j^2.
  normalize      the device exp and log in double: no accuracy table of ROCm's device library was at hand, so
                 2 ulp = 4 u is ASSUMED for both.  s = sum_c exp(a_c), a_c = wlp_c - m <= 0: the subtraction moves
                 exp(a_c) by u |a_c| relative and |a| exp(a) <= 1 / e, the k - 1 additions by (k - 1) u, s >= 1:
                 |ds| / s <= (4 + k - 1 + k) u.  lpn = m + log s: |dlpn| <= (2 k + 3) u + 4 u log k + u |lpn| =: L.
                 resp = exp(wlp - lpn): relative error <= L + u |wlp - lpn| + 4 u.
                 lpn_sum: n additions, |err| <= n u sum |lpn| (+ the lpn's own errors, n L).
  weighted_sums  sums over n rows with cancellation: |err| <= (n + 1) u sum_i resp |x| (any order of n additions, one
                 rounding per product; the count is the rows', whatever the slices); nk: n u sum_i resp.
  scatter_diag   resp (x - m)^2: 3 roundings per term: |err| <= (n + 3) u out.
  scatter_full   A = resp (x_r - m_r) two roundings (centring, product), B one, the product and the sum:
                 |err| <= (n + 4) u sum_i resp |x_r - m_r| |x_c - m_c|.
Near-duplicate rows are among the random data (rows 3, 5, 7 and the last are row 0 plus 1e-6 noise).

Whole fits against `em64` of tests/test_mixture_cpu.py in long double, with that file's bound rule per quantity:
16 x the relative difference between em64 in float64 and in long double, plus n_iter (d + k + 8) 2^-53.  What the model
returns for held-out rows is compared with the long-double restatement at the MODEL's parameters: the kernels' bounds
above plus, for full, the host Cholesky factor's backward error (4 d u cond(Sigma) relative on the Mahalanobis term).
"""
import math
import warnings

import numpy as np
import pytest
import torch

import test_mixture_cpu as R
from parity_log import parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
LD = np.longdouble


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def padded(x, limit, poison=1e30):
    """x float32 [n, d] as the device rows [n, ld]: d rounded up to a multiple of 4 -- and 4 more columns where d is one
    already and the limit allows -- with `poison` in the padding.  Returns (xp, d)."""
    n, d = x.shape
    ld = d + (-d) % 4
    if ld == d and d + 4 <= limit:
        ld = d + 4
    xp = np.full((n, ld), poison, dtype=np.float32)
    xp[:, :d] = x
    return dev(xp), d


def lattice(n, d, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (n, d)).astype(np.float32)
    mean = rng.integers(-3, 4, (k, d)).astype(np.float64)
    resp = rng.integers(0, 9, (n, k)).astype(np.float64) / 8.0
    return rng, x, mean, resp


def rows(n, d, seed):
    """float32 rows with near-duplicates among them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    for i in (3, 5, 7, n - 1):
        if 0 < i < n:
            x[i] = x[0] + 1e-6 * rng.standard_normal(d).astype(np.float32)
    return x


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


DIAG_SHAPES = [(1, 1, 1), (33, 5, 7), (65, 17, 65), (257, 130, 2), (31, 1024, 3), (1000, 512, 130), (64, 3, 300), (4097, 4, 63),
               (255, 15, 64), (63, 16, 2), (32, 65, 7), (65600, 4, 2)]
FULL_SHAPES = [(1, 1, 1), (33, 5, 7), (65, 17, 2), (63, 64, 3), (255, 65, 2), (64, 130, 2), (32, 256, 2), (1000, 50, 63),
               (31, 16, 65), (257, 15, 130), (4097, 4, 7), (64, 3, 300), (65600, 4, 2)]


# ------------------------------------------------------------------------------------------------ exact


@pytest.mark.parametrize("n, d, k", DIAG_SHAPES)
def test_logprob_diag_exact(n, d, k):
    from ssl_wafermap_amd import mixture as M

    rng, x, mean, _ = lattice(n, d, k, 1000 * n + d + k)
    inv_var = 2.0 ** rng.integers(-2, 3, (k, d))
    cst = rng.integers(-5, 6, k).astype(np.float64)
    diff = x.astype(np.float64)[:, None, :] - mean[None] if n * k * d <= 1 << 24 else None
    if diff is not None:
        want = cst[None] - 0.5 * (diff * diff * inv_var[None]).sum(2)
    else:
        want = np.stack([cst[c] - 0.5 * ((x - mean[c]) ** 2 * inv_var[c]).sum(1) for c in range(k)], axis=1)
    xp, _ = padded(x, 1024)
    got = host(M._logprob_diag(xp, d, dev(mean), dev(inv_var), dev(cst)))
    assert np.array_equal(got, want)
    clean, _ = padded(x, 1024, poison=0.0)
    assert same_bytes(got, host(M._logprob_diag(clean, d, dev(mean), dev(inv_var), dev(cst))))  # padding, and a second call


@pytest.mark.parametrize("n, d, k", FULL_SHAPES)
def test_logprob_full_exact(n, d, k):
    from ssl_wafermap_amd import mixture as M

    rng, x, mean, _ = lattice(n, d, k, 2000 * n + d + k)
    p = np.triu(rng.integers(-2, 3, (k, d, d))).astype(np.float64)
    cst = rng.integers(-5, 6, k).astype(np.float64)
    want = np.stack([cst[c] - 0.5 * (((x.astype(np.float64) - mean[c]) @ p[c]) ** 2).sum(1) for c in range(k)], axis=1)
    xp, _ = padded(x, 256)
    got = host(M._logprob_full(xp, d, dev(mean), dev(p), dev(cst)))
    assert np.array_equal(got, want)
    dirty = p.copy()
    dirty[:, np.tril_indices(d, -1)[0], np.tril_indices(d, -1)[1]] = np.nan  # below the diagonal: never read
    clean, _ = padded(x, 256, poison=0.0)
    assert same_bytes(got, host(M._logprob_full(clean, d, dev(mean), dev(dirty), dev(cst))))


M_SHAPES = [(1, 1, 1), (33, 5, 7), (65, 63, 65), (257, 64, 2), (1000, 130, 63), (4097, 17, 130), (65600, 4, 2), (255, 1024, 3),
            (64, 512, 300), (31, 3, 64), (63, 15, 1), (32, 16, 7)]


@pytest.mark.parametrize("n, d, k", M_SHAPES)
def test_weighted_sums_and_scatter_diag_exact(n, d, k):
    from ssl_wafermap_amd import mixture as M

    _, x, mean, resp = lattice(n, d, k, 3000 * n + d + k)
    x64 = x.astype(np.float64)
    xp, _ = padded(x, 1024)
    clean, _ = padded(x, 1024, poison=0.0)
    nk, sx = M._weighted_sums(xp, d, dev(resp))
    assert np.array_equal(host(nk), resp.sum(0)) and np.array_equal(host(sx), resp.T @ x64)
    nk2, sx2 = M._weighted_sums(clean, d, dev(resp))
    assert same_bytes(host(nk), host(nk2)) and same_bytes(host(sx), host(sx2))
    want = np.stack([(resp[:, c, None] * (x64 - mean[c]) ** 2).sum(0) for c in range(k)])
    got = host(M._scatter_diag(xp, d, dev(resp), dev(mean)))
    assert np.array_equal(got, want)
    assert same_bytes(got, host(M._scatter_diag(clean, d, dev(resp), dev(mean))))


SCATTER_FULL_SHAPES = [(1, 1, 1), (33, 5, 7), (65, 64, 2), (257, 65, 3), (1000, 130, 2), (4097, 17, 7), (65600, 4, 2),
                       (63, 256, 2), (31, 15, 65), (64, 3, 300), (255, 50, 63), (32, 16, 130)]


@pytest.mark.parametrize("n, d, k", SCATTER_FULL_SHAPES)
def test_scatter_full_exact(n, d, k):
    from ssl_wafermap_amd import mixture as M

    _, x, mean, resp = lattice(n, d, k, 4000 * n + d + k)
    x64 = x.astype(np.float64)
    want = np.stack([((x64 - mean[c]) * resp[:, c, None]).T @ (x64 - mean[c]) for c in range(k)])
    xp, _ = padded(x, 256)
    got = host(M._scatter_full(xp, d, dev(resp), dev(mean)))
    assert np.array_equal(got, want)
    assert same_bytes(got, np.ascontiguousarray(got.transpose(0, 2, 1)))  # symmetric bit for bit
    clean, _ = padded(x, 256, poison=0.0)
    assert same_bytes(got, host(M._scatter_full(clean, d, dev(resp), dev(mean))))


# ------------------------------------------------------------------------------------------------ against float64


@pytest.mark.parametrize("n, d, k", [(1000, 50, 7), (257, 17, 65), (65, 130, 3)])
def test_logprob_against_long_double(n, d, k):
    from ssl_wafermap_amd import mixture as M

    rng = np.random.default_rng(n + d + k)
    x = rows(n, d, n * d)
    mean = rng.standard_normal((k, d))
    inv_var = 1.0 / rng.uniform(0.2, 3.0, (k, d))
    cst = rng.standard_normal(k)
    xl = x.astype(LD)
    xp, _ = padded(x, 256)
    got = host(M._logprob_diag(xp, d, dev(mean), dev(inv_var), dev(cst)))
    worst = 0.0
    for c in range(k):
        s = ((xl - mean[c].astype(LD)) ** 2 * inv_var[c].astype(LD)).sum(1)
        want = cst[c] - s / 2
        bound = (d + 3) * U * s / 2 + U * np.abs(want)
        worst = max(worst, float((np.abs(got[:, c] - want) / bound).max()))
    parity(f"logprob_diag n={n} d={d} k={k}: error / derived bound", worst, 1.0)
    p = np.triu(rng.standard_normal((k, d, d))) / math.sqrt(d)
    got = host(M._logprob_full(xp, d, dev(mean), dev(p), dev(cst)))
    worst = 0.0
    for c in range(k):
        diff = xl - mean[c].astype(LD)
        y = diff @ p[c].astype(LD)
        e = (d + 1) * U * (np.abs(diff) @ np.abs(p[c]).astype(LD))
        s = (y * y).sum(1)
        want = cst[c] - s / 2
        bound = ((2 * np.abs(y) * e + e * e).sum(1) + (d + 1) * U * s) / 2 + U * np.abs(want)
        worst = max(worst, float((np.abs(got[:, c] - want) / bound).max()))
    parity(f"logprob_full n={n} d={d} k={k}: error / derived bound", worst, 1.0)


def normalize_bounds(wlp):
    """(lpn, resp, L, resp's relative bound) of the docstring, in long double."""
    k = wlp.shape[1]
    w = wlp.astype(LD)
    m = w.max(1)
    lpn = m + np.log(np.exp(w - m[:, None]).sum(1))
    big_l = (2 * k + 3) * U + 4 * U * math.log(k) + U * np.abs(lpn)
    resp = np.exp(w - lpn[:, None])
    return lpn, resp, big_l, big_l[:, None] + U * np.abs(w - lpn[:, None]) + 4 * U


@pytest.mark.parametrize("n, k", [(1, 1), (33, 2), (255, 7), (257, 65), (1000, 300), (4097, 63), (65600, 2), (64, 130)])
def test_normalize_against_long_double(n, k):
    from ssl_wafermap_amd import mixture as M

    rng = np.random.default_rng(n + k)
    wlp = rng.standard_normal((n, k)) * 5.0 - 40.0
    wlp[::7] *= 20.0  # rows whose spread makes most responsibilities underflow
    lpn_ref, resp_ref, big_l, resp_rel = normalize_bounds(wlp)
    t = dev(wlp)
    lpn, label, total = M._normalize(t)
    lpn, resp, label, total = host(lpn), host(t), host(label), float(host(total)[0])
    parity(f"normalize n={n} k={k}: lpn error / derived bound", float((np.abs(lpn - lpn_ref) / big_l).max()), 1.0)
    parity(f"normalize n={n} k={k}: resp error / derived bound",
           float((np.abs(resp - resp_ref) / (resp_rel * resp_ref + 1e-300)).max()), 1.0)
    assert np.array_equal(label, wlp.argmax(1).astype(np.int32)) and label.dtype == np.int32
    want = math.fsum(lpn.tolist())  # the sum of the lpn the kernel itself stored
    parity(f"normalize n={n} k={k}: lpn_sum error / (n u sum |lpn|)", abs(total - want) / (n * U * np.abs(lpn).sum()), 1.0)
    if k == 1:
        assert np.array_equal(resp, np.ones((n, 1))) and np.array_equal(lpn, wlp[:, 0])
    t2 = dev(wlp)
    lpn2, label2, total2 = M._normalize(t2)
    assert same_bytes(host(t2), resp) and same_bytes(host(lpn2), lpn) and same_bytes(host(total2), np.array([total]))


def test_normalize_edges():
    from ssl_wafermap_amd import mixture as M

    wlp = np.array([[-900.0, -3.0, -2000.0, -3.0],       # spread above 800: exact zeros, lpn = log 2 - 3
                    [-5.0, -900.0, -1e4, -1e5],          # ... and lpn equals the maximum
                    [-7.0, -7.0, -7.0, -7.0],            # an exact tie: the lowest index
                    [-1e300, -1e300, -3.0, -3.0],
                    [2.0, 1.0, 2.0, 0.0]])
    t = dev(wlp)
    lpn, label, total = M._normalize(t)
    lpn, resp, label = host(lpn), host(t), host(label)
    assert np.isfinite(lpn).all() and np.isfinite(resp).all()
    assert lpn[1] == -5.0 and resp[1].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert resp[0, 0] == 0.0 and resp[0, 2] == 0.0 and resp[0, 1] == resp[0, 3] and abs(resp[0, 1] - 0.5) <= 8 * U
    assert abs(lpn[0] - (math.log(2.0) - 3.0)) <= 16 * U * 3 and abs(lpn[2] - (math.log(4.0) - 7.0)) <= 16 * U * 7
    assert label.tolist() == [1, 0, 0, 2, 0]
    assert resp[3, 0] == 0.0 and resp[3, 1] == 0.0
    one = dev(np.array([[-1234.5], [0.0], [7e5]]))
    lpn1, label1, total1 = M._normalize(one)
    assert host(one).tolist() == [[1.0], [1.0], [1.0]] and host(lpn1).tolist() == [-1234.5, 0.0, 7e5]
    assert host(label1).tolist() == [0, 0, 0] and float(host(total1)[0]) == (-1234.5 + 0.0) + 7e5


@pytest.mark.parametrize("n, d, k", [(1000, 50, 7), (257, 17, 65), (4097, 130, 3)])
def test_m_step_kernels_against_long_double(n, d, k):
    from ssl_wafermap_amd import mixture as M

    rng = np.random.default_rng(7 * n + d + k)
    x = rows(n, d, n + d) + 3.0  # (an offset: the sums of resp * x cancel less than their magnitudes)
    resp = rng.dirichlet(np.full(k, 0.3), n)
    xl, rl = x.astype(LD), resp.astype(LD)
    xp, _ = padded(x, 256)
    nk, sx = M._weighted_sums(xp, d, dev(resp))
    nk, sx = host(nk), host(sx)
    parity(f"weighted_sums n={n} d={d} k={k}: nk error / derived bound",
           float((np.abs(nk - rl.sum(0)) / (n * U * rl.sum(0))).max()), 1.0)
    parity(f"weighted_sums n={n} d={d} k={k}: sx error / derived bound",
           float((np.abs(sx - rl.T @ xl) / ((n + 1) * U * (rl.T @ np.abs(xl)))).max()), 1.0)
    mean = sx / nk[:, None]
    sd = host(M._scatter_diag(xp, d, dev(resp), dev(mean)))
    sf = host(M._scatter_full(xp, d, dev(resp), dev(mean)))
    worst_d = worst_f = 0.0
    for c in range(k):
        diff = xl - mean[c].astype(LD)
        want = (rl[:, c, None] * diff * diff).sum(0)
        worst_d = max(worst_d, float((np.abs(sd[c] - want) / ((n + 3) * U * want)).max()))
        want = (rl[:, c, None] * diff).T @ diff
        mag = (rl[:, c, None] * np.abs(diff)).T @ np.abs(diff)
        worst_f = max(worst_f, float((np.abs(sf[c] - want) / ((n + 4) * U * mag)).max()))
    parity(f"scatter_diag n={n} d={d} k={k}: error / derived bound", worst_d, 1.0)
    parity(f"scatter_full n={n} d={d} k={k}: error / derived bound", worst_f, 1.0)


def test_two_passes_survive_cancellation():
    """Rows 1000 + 1e-3 noise: the centred scatter keeps the variances, the one-pass float64 form
    avg_X2 - 2 avg_X mu + mu^2 (sklearn's diag form) loses them."""
    from ssl_wafermap_amd import mixture as M

    n, d, k = 1000, 52, 7
    rng = np.random.default_rng(11)
    x = (1000.0 + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    resp = rng.dirichlet(np.full(k, 0.5), n)
    xp, _ = padded(x, 256)
    nk, sx = M._weighted_sums(xp, d, dev(resp))
    mean_t = sx / nk[:, None]
    nk, mean = host(nk), host(mean_t)
    var_d = host(M._scatter_diag(xp, d, dev(resp), mean_t.contiguous())) / nk[:, None]
    var_f = host(M._scatter_full(xp, d, dev(resp), mean_t.contiguous())) / nk[:, None, None]
    xl, rl = x.astype(LD), resp.astype(LD)
    x64 = x.astype(np.float64)
    worst_kernel = worst_one_pass = worst_full = 0.0
    for c in range(k):
        diff = xl - mean[c].astype(LD)
        exact = (rl[:, c, None] * diff * diff).sum(0) / nk[c]
        exact_full = (rl[:, c, None] * diff).T @ diff / nk[c]
        one_pass = (resp[:, c] @ (x64 * x64)) / nk[c] - 2 * ((resp[:, c] @ x64) / nk[c]) * mean[c] + mean[c] ** 2
        worst_kernel = max(worst_kernel, float((np.abs(var_d[c] - exact) / exact).max()))
        worst_one_pass = max(worst_one_pass, float((np.abs(one_pass - exact) / exact).max()))
        mag = (rl[:, c, None] * np.abs(diff)).T @ np.abs(diff) / nk[c]
        worst_full = max(worst_full, float((np.abs(var_f[c] - exact_full) / mag).max()))
    parity("cancellation: scatter_diag variance, relative error / ((n + 4) u)", worst_kernel / ((n + 4) * U), 1.0)
    parity("cancellation: scatter_full covariance, error / ((n + 5) u sum |.||.|)", worst_full / ((n + 5) * U), 1.0)
    parity("cancellation: one-pass float64 error / two-pass kernel error", worst_one_pass / max(worst_kernel, U), 100.0, higher=True)


# ------------------------------------------------------------------------------------------------ determinism


def test_a_component_does_not_depend_on_the_others():
    from ssl_wafermap_amd import mixture as M

    n, d, k = 4097, 17, 7
    rng = np.random.default_rng(5)
    x = rows(n, d, 9)
    resp = rng.dirichlet(np.full(k, 0.3), n)
    mean = rng.standard_normal((k, d))
    xp, _ = padded(x, 256)
    nk, sx = M._weighted_sums(xp, d, dev(resp))
    sd = M._scatter_diag(xp, d, dev(resp), dev(mean))
    sf = M._scatter_full(xp, d, dev(resp), dev(mean))
    for c in (0, 4, 6):
        one = dev(resp[:, c:c + 1])
        nk1, sx1 = M._weighted_sums(xp, d, one)
        assert same_bytes(host(nk1), host(nk)[c:c + 1]) and same_bytes(host(sx1), host(sx)[c:c + 1])
        assert same_bytes(host(M._scatter_diag(xp, d, one, dev(mean[c:c + 1]))), host(sd)[c:c + 1])
        assert same_bytes(host(M._scatter_full(xp, d, one, dev(mean[c:c + 1]))), host(sf)[c:c + 1])
    # and a second call of everything gives the same bytes
    nk2, sx2 = M._weighted_sums(xp, d, dev(resp))
    assert same_bytes(host(nk2), host(nk)) and same_bytes(host(sx2), host(sx))
    assert same_bytes(host(M._scatter_diag(xp, d, dev(resp), dev(mean))), host(sd))
    assert same_bytes(host(M._scatter_full(xp, d, dev(resp), dev(mean))), host(sf))


# ------------------------------------------------------------------------------------------------ whole fits


@pytest.fixture(scope="module")
def fit_rows():
    x, held = R.fit_input()
    return x, held, dev(x.astype(np.float32)), dev(held.astype(np.float32))


def model_lpn_bound(x, w, mu, cov, ct):
    """(lpn, resp) of the long-double restatement at the given parameters and the bound of the module docstring on the
    model's lpn: the log-probability kernel's, the Cholesky factor's for full, normalize's."""
    n, d = x.shape
    k = mu.shape[0]
    xl = x.astype(LD)
    lpn, resp = R.ref_e_step(xl, w.astype(LD), mu.astype(LD), cov.astype(LD), ct)
    p = R.ref_pchol(cov.astype(LD), ct)
    worst = np.zeros(n, dtype=LD)
    for c in range(k):
        diff = xl - mu[c].astype(LD)
        if ct == "full":
            y = diff @ p[c]
            e = (d + 1) * U * (np.abs(diff) @ np.abs(p[c]))
            s = (y * y).sum(1)
            b = ((2 * np.abs(y) * e + e * e).sum(1) + (d + 1) * U * s) / 2 + 4 * d * U * np.linalg.cond(cov[c]) * s / 2
        else:
            s = (diff * diff * (p[c] * p[c] if ct == "diag" else p[c] * p[c] * np.ones(d))).sum(1)
            b = (d + 3 + 4) * U * s / 2  # (+ 4: 1 / sqrt, its square and the host's two roundings of inv_var)
        cst = abs(float(np.log(w[c]))) + 0.5 * d * math.log(2 * math.pi) + d * float(np.abs(np.log(np.abs(np.diagonal(p[c]) if ct == "full" else p[c]))).max())
        worst = np.maximum(worst, b + (d + 4) * U * cst + U * s / 2)
    return lpn, resp, worst + (2 * k + 3) * U + 4 * U * math.log(k) + U * np.abs(lpn)


@pytest.mark.parametrize("n_iter", [5, 20])
@pytest.mark.parametrize("ct", ["diag", "spherical", "full"])
def test_fit_against_em64(fit_rows, ct, n_iter):
    from ssl_wafermap_amd import mixture as M

    x, held, x_dev, held_dev = fit_rows
    n, d = x.shape
    k = 5
    w, mu, cov, prec = R.fit_init(x, k, ct)
    f64, ld = R.reference_runs(ct, n_iter)
    model = M.GaussianMixture(k, covariance_type=ct, tol=0.0, max_iter=n_iter, weights_init=w, means_init=mu, precisions_init=prec)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        labels = model.fit_predict(x_dev)
    assert any("did not converge" in str(c.message) for c in caught)  # tol = 0 never converges: the warning is sklearn's
    assert model.n_iter_ == n_iter == len(model.lower_bounds_) and not model.converged_ and model.n_features_in_ == d
    got = {"weights": model.weights_, "means": model.means_, "covariances": model.covariances_, "lower_bound": model.lower_bound_}
    for key, val in got.items():
        want = ld["lower_bounds"][-1] if key == "lower_bound" else ld[key]  # the bound BEFORE the last M-step
        parity(f"fit {ct} it={n_iter} {key}: relative to em64 long double / bound", R.rel(val, want) / R.fit_bound(f64, ld, key, n_iter, d, k), 1.0)
    lbs = np.array(model.lower_bounds_)
    assert (np.diff(lbs) >= -1e-12 * np.abs(lbs[1:])).all() and model.lower_bound_ == lbs[-1]
    # labels: the argmax of the reference responsibilities (no row of this input is within 1e-9 of a tie:
    # test_mixture_cpu.test_fit_input_leaves_no_label_to_chance)
    for rows_h, rows_d, lab in ((x, x_dev, labels), (held, held_dev, model.predict(held_dev))):
        ref = R.ref_e_step(rows_h.astype(LD), ld["weights"], ld["means"], ld["covariances"], ct)[1]
        top = np.sort(ref, axis=1)
        clear = top[:, -1] - top[:, -2] >= 1e-9
        assert clear.mean() >= 0.999 and np.array_equal(lab[clear], ref.argmax(1)[clear])
    # the fitted model on 100 held-out rows against the restatement at the model's own parameters
    lpn_ref, resp_ref, lpn_bound = model_lpn_bound(held, model.weights_, model.means_, model.covariances_, ct)
    lpn = host(model.score_samples(held_dev))
    proba = host(model.predict_proba(held_dev))
    assert lpn.dtype == np.float64 and proba.shape == (100, k)
    parity(f"fit {ct} it={n_iter}: score_samples error / bound", float((np.abs(lpn - lpn_ref) / lpn_bound).max()), 1.0)
    parity(f"fit {ct} it={n_iter}: predict_proba error / bound",
           float((np.abs(proba - resp_ref) / (resp_ref * (2 * lpn_bound[:, None] + 4 * U) + 1e-300)).max()), 1.0)
    score_ref = float(lpn_ref.mean())
    tol = float(lpn_bound.mean()) + 100 * U * float(np.abs(lpn_ref).mean())
    assert abs(model.score(held_dev) - score_ref) <= tol
    npar = M.n_parameters(k, d, ct)
    assert abs(model.bic(held_dev) - (-2 * score_ref * 100 + npar * math.log(100))) <= 2 * 100 * tol + 8 * U * abs(npar * math.log(100))
    assert abs(model.aic(held_dev) - (-2 * score_ref * 100 + 2 * npar)) <= 2 * 100 * tol + 8 * U * 2 * npar
    if ct == "full":
        for c in range(k):
            assert np.abs(model.precisions_[c] @ model.covariances_[c] - np.eye(d)).max() <= 16 * d * U * np.linalg.cond(model.covariances_[c])
    else:
        assert np.allclose(model.precisions_ * model.covariances_, 1.0, rtol=8 * U, atol=0)


def test_steps_and_initialisations(fit_rows):
    from ssl_wafermap_amd import mixture as M

    x, held, x_dev, held_dev = fit_rows
    n, d = x.shape
    k = 5
    # the public half-steps against the restatement: one E-step and one M-step from the init arrays
    for ct in ("diag", "spherical", "full"):
        w, mu, cov, _ = R.fit_init(x, k, ct)
        lpn, resp, labels = M.gmm_e_step(x_dev, w, mu, cov, ct)
        lpn_ref, resp_ref, bound = model_lpn_bound(x, w, mu, cov, ct)
        parity(f"gmm_e_step {ct}: lpn error / bound", float((np.abs(host(lpn) - lpn_ref) / bound).max()), 1.0)
        assert np.array_equal(host(labels), host(resp).argmax(1)) and labels.dtype == torch.int32
        w1, mu1, cov1 = M.gmm_m_step(x_dev, resp, ct)
        wr, mur, covr = R.ref_m_step(x.astype(LD), host(resp).astype(LD), ct, 1e-6)
        # weights and covariances are sums over n rows of non-negative terms (an off-diagonal covariance is bounded by
        # the diagonal's magnitudes): (n + 5) u of the largest entry.  The means cancel: (n + 2) u of resp^T |x| / nk.
        r = host(resp).astype(LD)
        mean_mag = float(((r.T @ np.abs(x).astype(LD)) / r.sum(0)[:, None]).max() / np.abs(mur).max())
        for name, a, b, scale in (("weights", w1, wr, 1.0), ("means", mu1, mur, mean_mag), ("covariances", cov1, covr, 1.0)):
            parity(f"gmm_m_step {ct} {name}: relative error / derived bound", R.rel(host(a), b) / ((n + 5) * U * scale), 1.0)
    # n_init: the kept run is the one of the largest bound; every init_params runs and improves on its first bound
    for init in ("kmeans", "k-means++", "random_from_data"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = M.GaussianMixture(3, covariance_type="diag", n_init=3, max_iter=4, tol=0.0, init_params=init, random_state=7).fit(x_dev)
        assert len(model.lower_bounds_all_) == 3 and model.lower_bound_ == max(model.lower_bounds_all_)
        assert model.lower_bounds_[-1] == model.lower_bound_ and model.lower_bounds_[-1] > model.lower_bounds_[0]
        assert abs(model.weights_.sum() - 1.0) <= 8 * U and model.means_.shape == (3, d) and model.covariances_.shape == (3, d)
        again = M.GaussianMixture(3, covariance_type="diag", n_init=3, max_iter=4, tol=0.0, init_params=init, random_state=7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            again.fit(x_dev)
        assert same_bytes(again.means_, model.means_) and again.lower_bounds_ == model.lower_bounds_  # the same bits


@pytest.mark.parametrize("ct", ["diag", "spherical", "full"])
def test_convergence_stop(ct):
    from ssl_wafermap_amd import mixture as M

    x = R.stop_input()
    want_iter, changes = R.stop_reference(ct)
    assert changes[-1] <= 1e-4 and (changes[:-1] >= 1e-2).all()  # (10 x from tol on both sides: a rounding cannot move the stop)
    w, mu, cov, prec = R.fit_init(x, 3, ct)
    model = M.GaussianMixture(3, covariance_type=ct, tol=1e-3, max_iter=40, weights_init=w, means_init=mu, precisions_init=prec)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*did not converge.*")  # a converged fit does not warn
        model.fit(dev(x.astype(np.float32)))
    assert model.converged_ and model.n_iter_ == want_iter == len(model.lower_bounds_)


# ------------------------------------------------------------------------------------------------ the script


def test_sweep_script_on_wafer_embeddings(tmp_path, capsys):
    import csv
    import importlib.util

    spec = importlib.util.spec_from_file_location("embedding_gmm_amd", R.ROOT / "scripts" / "embedding_gmm_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    summary = mod.main(["--embeddings", str(R.GOLDEN / "simsiam_preds_subset.npz"), "--rows", "1536", "--pca", "8", "--k", "2:4",
                        "--holdout", "36", "--seed", "0", "--out", str(tmp_path)])
    with open(tmp_path / "trials.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == 3 and list(table[0]) == mod.COLUMNS and [int(r["k"]) for r in table] == [2, 3, 4]
    for row in table:
        assert all(np.isfinite(float(row[c])) for c in mod.COLUMNS), row
        assert float(row["bic"]) > float(row["aic"]) and 1 <= int(row["n_iter"]) <= 100 and 0 <= float(row["homogeneity"]) <= 1
    k = summary["chosen_k"]
    assert float(table[k - 2]["bic"]) == min(float(r["bic"]) for r in table) and (summary["n"], summary["d"]) == (1500, 8)
    labels, proba, scores = (np.load(tmp_path / f) for f in ("labels.npy", "proba.npy", "score_samples.npy"))
    assert labels.shape == (1500,) and proba.shape == (1500, k) and scores.shape == (1500,) and proba.dtype == np.float64
    assert np.array_equal(labels, proba.argmax(1))
    # a row of responsibilities sums to 1 within normalize's bound on lpn (module docstring: every entry of the row moves
    # by that relative amount), the entries' own 4 u + u |wlp - lpn| (weighted: at most 1 / e per entry) and numpy's k adds
    assert (np.abs(proba.sum(1) - 1.0) <= ((2 * k + 3) + 4 * math.log(k) + np.abs(scores) + 4 + k + k) * U).all()
    assert abs(scores.mean() - float(table[k - 2]["lower_bound"])) <= 0.5  # (the kept parameters, one M-step later)
    assert np.load(tmp_path / "weights.npy").shape == (k,) and np.load(tmp_path / "means.npy").shape == (k, 8)
    assert np.load(tmp_path / "covariances.npy").shape == (k, 8, 8)
    assert np.load(tmp_path / "holdout_labels.npy").shape == (36,) and np.load(tmp_path / "holdout_score_samples.npy").shape == (36,)
    assert summary["holdout"] == 36 and np.isfinite(summary["holdout_score"])
    assert "lowest BIC" in capsys.readouterr().out
