"""GPU checks of csrc/logreg.hip and linear_model.py.  The reference (`lr64`, long double), the bounds (`bounds64`) and
the generators are tests/test_linear_model_cpu.py's.

Exact: on integer lattices (x in [-4, 4], w and b small integers, residuals multiples of 1/8) every product and sum of
the two matrix products is exact in float64, so numpy restates z_out and the gradient bit for bit: fragment maps, masks,
tile and slice edges, the true-d rule (1e30 in the padding columns of x changes nothing).

Against long double, with u = 2^-53, one rounding per product and per accumulation step (first order; `bounds64`
multiplies by 1 + 1e-3 for the second-order terms), and for the device exp / log / log1p in double the 2 ulp = 4 u that
tests/test_gpu_mixture.py ASSUMES (no accuracy table of ROCm's device library was at hand):
  logits     z = sum_f x_f w_f + b: d products, d additions, the intercept's addition, in any order:
             |dz| <= E_z = (d + 2) u (sum_f |x_f w_f| + |b|).
  mode 0     lse is 1-Lipschitz in the max norm: the logits' errors move it by E = max_c E_z at most; computed from
             the stored logits it carries wm_gmm_normalize's L = (2 K + 3) u + 4 u log K + u |lse| (sum of exp(a_c),
             a_c <= 0, in class order; the log; the addition of the maximum).  p_c = exp(z_c - lse): the argument is off by
             E_z,c + E + L + u |z_c - lse| (its own subtraction), the exp by 4 u relative:
             |dp_c| <= p_c rho_c,  rho_c = E_z,c + E + L + u |z_c - lse| + 4 u.
             resid = s (p - onehot): the subtraction and the product add 2 u |p - onehot|:
             |dresid| <= s (p rho + 2 u |p - onehot|).
             loss_i = s (lse - z_y): |dloss_i| <= s (E + L + E_z,y + u |lse - z_y|) + u loss_i.
  mode 1     e = exp(-|z|) (4 u), sigma = 1 / (1 + e) or e / (1 + e): an addition, a division, a product: 7 u relative
             with e's; the logit's error moves sigma by sigma (1 - sigma) E_z <= sigma E_z; the products with a and s
             2 u more: |dresid| <= |resid| (E_z + 9 u).
             softplus = max(+-z, 0) + log1p(e) is 1-Lipschitz in z; e's 4 u moves log1p(e) by at most 4 u log1p(e)
             (e / (1 + e) <= log1p(e)), log1p itself 4 u, the addition u, the products with a and s 2 u:
             |dloss_i| <= s a (E_z + 11 u softplus).
  loss       n non-negative terms added in a fixed order: |dloss| <= sum_i |dloss_i| + n u sum_i loss_i.
  gradient   resid^T [x | 1] from the residuals the kernel stored, one rounding per product, n additions with
             cancellation: |dgrad| <= (n + 1) u sum_i |resid_i| |x_i| (wm_gmm_weighted_sums' bound); against lr64 the
             residuals' own bounds are added, sum_i |dresid_i| |x_i|.
Every ratio error / bound is taken with 1e-300 added to the bound: a float64 result below the normal range (a sigmoid
or a probability of exp(-1000)) is a zero or a subnormal, whose absolute error is the format's, not the derivation's.
A fit stops at max |grad f| <= tol of the DEVICE's gradient; the long-double gradient at the returned parameters is
therefore within tol + (the gradient bound above) / S + 3 u |w| / (C S) (the penalty's product, addition and the
division by S).  Against sklearn: the strong-convexity bound of tests/test_linear_model_cpu.py.

cols <= 256 is the contract, so K = 65 runs with 1 and 3 groups (195 columns, straddling 64 and 128) and its 4-group
form (260 columns) is checked to be refused.
"""
import csv
import importlib.util
import json
import warnings

import numpy as np
import pytest
import torch

import test_linear_model_cpu as R
from parity_log import parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = R.U
LD = R.LD


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def padded(x, poison=1e30, limit=1024):
    """x float32 [n, d] as device rows [n, ld]: d rounded up to a multiple of 4 -- and 4 more columns where d is one
    already and the limit allows -- with `poison` in the padding."""
    n, d = x.shape
    ld = d + (-d) % 4
    if ld == d and d + 4 <= limit:
        ld = d + 4
    xp = np.full((n, ld), poison, dtype=np.float32)
    xp[:, :d] = x
    return dev(xp)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SHAPES = [(1, 1, 1), (63, 16, 3), (65, 17, 27), (257, 130, 65), (64, 1024, 2), (1000, 512, 256), (4097, 4, 9)]


# ------------------------------------------------------------------------------------------------ exact


@pytest.mark.parametrize("n, d, cols", SHAPES)
def test_logits_exact(n, d, cols):
    from ssl_wafermap_amd import linear_model as L

    x, w, _ = R.lattice(n, d, cols, 100 * n + d + cols)
    want = x.astype(np.float64) @ w[:, :d].T + w[:, d][None, :]
    xp = padded(x)
    _, _, z = L._residual(xp, d, dev(w), 1, 1, want_z=True)
    z = host(z)
    assert np.array_equal(z, want)
    _, _, z2 = L._residual(padded(x, poison=0.0), d, dev(w), 1, 1, want_z=True)  # the padding, and a second call
    assert same_bytes(z, host(z2))
    # the softmax form (labels given) stores the same logits
    y = np.random.default_rng(n).integers(-1, cols, n).astype(np.int32)
    _, loss, z3 = L._residual(xp, d, dev(w), 0, cols, dev(y), want_z=True)
    assert same_bytes(z, host(z3)) and np.isfinite(host(loss)).all()


def wsum_slices(n, d):
    """csrc/gmm.hip's cut of the rows of the weighted sums (f64_cut), restated."""
    tn = (d + 1 + 63) // 64
    want = min((1024 + tn - 1) // tn, (n + 255) // 256, (256 << 20) // (1024 * (d + 1) * 8))
    want = max(want, 1)
    rows = (n + want - 1) // want
    slice_rows = (rows + 31) // 32 * 32
    return (n + slice_rows - 1) // slice_rows


def first_two_slice_n(d):
    n = 1
    while wsum_slices(n, d) < 2:
        n += 1
    return n


GRAD_SHAPES = SHAPES + [(first_two_slice_n(d) + e, d, cols) for d, cols in ((17, 27), (130, 65), (512, 256)) for e in (-1, 0, 1)]


@pytest.mark.parametrize("n, d, cols", GRAD_SHAPES)
def test_gradient_exact_and_shared_with_weighted_sums(n, d, cols):
    from ssl_wafermap_amd import linear_model as L
    from ssl_wafermap_amd import mixture as M

    x, _, resid = R.lattice(n, d, cols, 200 * n + d + cols)
    x64 = x.astype(np.float64)
    xp = padded(x)
    grad = host(L._gradient(xp, d, dev(resid)))
    assert grad.shape == (cols, d + 1)
    assert np.array_equal(grad[:, :d], resid.T @ x64) and np.array_equal(grad[:, d], resid.sum(0))
    assert same_bytes(grad, host(L._gradient(padded(x, poison=0.0), d, dev(resid))))
    nk, sx = M._weighted_sums(xp, d, dev(resid))  # the same launch path: the same bytes
    assert same_bytes(np.ascontiguousarray(grad[:, :d]), host(sx)) and same_bytes(np.ascontiguousarray(grad[:, d]), host(nk))


def test_the_slice_boundary_is_where_the_test_says():
    assert first_two_slice_n(17) == first_two_slice_n(512) == 257 and wsum_slices(256, 130) == 1 and wsum_slices(258, 130) == 2


# ------------------------------------------------------------------------------------------------ against long double


def labels_for(n, mode, classes, rng):
    if mode == 0:
        y = rng.integers(0, classes, n).astype(np.int32)
        y[::11] = -1
        return y
    return (rng.random((n, classes)) < 0.4).astype(np.int8)


def check_against_lr64(tag, x, y, w, sw, mode, pw, classes):
    """The kernels' resid, loss and gradient against lr64 within bounds64; returns the device arrays."""
    from ssl_wafermap_amd import linear_model as L

    n, d = x.shape
    resid, loss, _ = L._residual(padded(x), d, dev(w), mode, classes, dev(y), None if sw is None else dev(sw),
                                 None if pw is None else dev(pw))
    grad = host(L._gradient(padded(x), d, resid))
    resid, loss = host(resid), host(loss)
    assert np.isfinite(resid).all() and np.isfinite(loss).all() and np.isfinite(grad).all()
    loss_ref, resid_ref, grad_ref = R.lr64(x, y, w, sw, mode, pw, classes)
    _, rb, lb = R.bounds64(x, y, w, sw, mode, pw, classes)
    tiny = LD(1e-300)
    parity(f"{tag}: resid error / derived bound", float((np.abs(resid - resid_ref) / (rb + tiny)).max()), 1.0)
    parity(f"{tag}: loss error / derived bound", float((np.abs(loss - loss_ref) / (lb + tiny)).max()), 1.0)
    x1 = np.concatenate([np.abs(x).astype(LD), np.ones((n, 1), dtype=LD)], axis=1)
    gb = rb.T @ x1 + (n + 1) * U * (np.abs(resid).astype(LD).T @ x1)
    parity(f"{tag}: gradient error / derived bound", float((np.abs(grad - grad_ref) / (gb + tiny)).max()), 1.0)
    return resid, loss, grad


@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("k", [2, 3, 9, 65])
@pytest.mark.parametrize("mode", [0, 1])
def test_residual_loss_gradient_against_long_double(mode, k, groups):
    from ssl_wafermap_amd import _lib

    n, d = 321, 37  # five full tiles and one row; two slabs of the loss; two slices of the gradient
    if k * groups > 256:
        assert _lib.load().wm_logreg_residual_workspace_bytes(n, d, 40, k * groups, mode, k) == 0  # 260 columns: refused
        groups = 3
    cols = k * groups
    rng = np.random.default_rng(1000 * mode + 10 * k + groups)
    x = R.rows(n, d, 7 * k + groups)
    w = rng.standard_normal((cols, d + 1)) * 0.5
    y = labels_for(n, mode, k, rng)
    sw = rng.uniform(0.1, 3.0, n)
    sw[::13] = 0.0  # zero-weight rows
    pw = rng.uniform(0.3, 4.0, k) if mode == 1 else None
    tag = f"logreg mode={mode} K={k} groups={groups}"
    r0, _, _ = check_against_lr64(tag + " plain", x, y, w, None, mode, None, k)
    r1, _, _ = check_against_lr64(tag + " weighted", x, y, w, sw, mode, pw, k)
    assert (r1[::13] == 0).all()  # a zero-weight row's residuals are zeros
    if mode == 0:
        assert (r0[::11] == 0).all() and (r1[::11] == 0).all()  # y == -1: an exact zero row
        assert (np.abs(r1) <= sw[:, None]).all()
    else:
        assert (np.abs(r1) <= sw[:, None] * np.maximum(np.tile(pw, groups), 1.0)[None, :]).all()


@pytest.mark.parametrize("scale", [1e3, 1e4])
@pytest.mark.parametrize("mode", [0, 1])
def test_extreme_logits(mode, scale):
    n, d, k = 130, 8, 5
    rng = np.random.default_rng(int(scale) + mode)
    x = R.rows(n, d, 3)
    x[10] = 0.0                            # all logits of the row equal (the intercepts are equal below)
    w = rng.standard_normal((k, d + 1))
    w[:, d] = 0.25
    big = float(np.abs(x.astype(np.float64) @ w[:, :d].T).max())
    w[:, :d] *= scale / big                # |z| reaches `scale`
    z = x.astype(np.float64) @ w[:, :d].T + w[:, d]
    assert scale * 0.99 <= np.abs(z).max() <= scale * 1.01 + 1
    if mode == 0:
        y = z.argmax(1).astype(np.int32)
        y[::2] = z.argmin(1)[::2]          # rows whose true class has p underflowing to 0
        assert (np.exp(z.min(1) - z.max(1))[::2] == 0).sum() >= 5
    else:
        y = (z < 0).astype(np.int8)        # every label as wrong as it can be
        y[::3] = 1 - y[::3]
    sw = rng.uniform(0.5, 2.0, n)
    resid, loss, grad = check_against_lr64(f"logreg extreme mode={mode} |z|~{scale:g}", x, y, w, sw, mode, None, k)
    assert not np.isnan(resid).any() and (np.abs(resid) <= sw[:, None]).all()
    if mode == 0:
        assert np.abs(resid[10] - sw[10] * (0.2 - (np.arange(k) == y[10]))).max() <= 8 * U * sw[10]
        assert loss[0] >= scale  # the wrong rows cost about |z| each
    else:
        assert np.abs(np.abs(resid[10]) - sw[10] * np.where(y[10] == 1, 1 - 1 / (1 + np.exp(-0.25)), 1 / (1 + np.exp(-0.25)))).max() <= 16 * U * sw[10]


# ------------------------------------------------------------------------------------------------ independence


@pytest.mark.parametrize("mode", [0, 1])
def test_a_problem_does_not_depend_on_its_company(mode):
    from ssl_wafermap_amd import linear_model as L

    n, d = 1000, 50
    k = 9 if mode == 0 else 3
    rng = np.random.default_rng(40 + mode)
    x = R.rows(n, d, 21)
    xp = padded(x)
    y = labels_for(n, mode, k, rng)
    sw = dev(rng.uniform(0.1, 2.0, n))
    pw = dev(rng.uniform(0.5, 3.0, k)) if mode == 1 else None
    w = rng.standard_normal((4, k, d + 1))
    y_d = dev(y)
    resid, loss, _ = L._residual(xp, d, dev(w.reshape(4 * k, d + 1)), mode, k, y_d, sw, pw)
    grad = host(L._gradient(xp, d, resid))
    resid, loss = host(resid), host(loss)
    if mode == 0:  # a problem is a group of k columns
        for g in range(4):
            r1, l1, _ = L._residual(xp, d, dev(w[g]), 0, k, y_d, sw)
            assert same_bytes(host(r1), np.ascontiguousarray(resid[:, g * k:(g + 1) * k])) and same_bytes(host(l1), loss[g:g + 1])
            assert same_bytes(host(L._gradient(xp, d, r1)), np.ascontiguousarray(grad[g * k:(g + 1) * k]))
        # ... and may move: problem 3 first
        r2, l2, _ = L._residual(xp, d, dev(w[[3, 0, 1, 2]].reshape(4 * k, d + 1)), 0, k, y_d, sw)
        assert same_bytes(np.ascontiguousarray(host(r2)[:, :k]), np.ascontiguousarray(resid[:, 3 * k:])) and host(l2)[0] == loss[3]
    else:  # a problem is one column
        for q in (0, 4, 7, 11):
            g, l = divmod(q, k)
            r1, l1, _ = L._residual(xp, d, dev(w[g, l:l + 1]), 1, 1, dev(y[:, l:l + 1]), sw, pw[l:l + 1].contiguous())
            assert same_bytes(host(r1), np.ascontiguousarray(resid[:, q:q + 1])) and same_bytes(host(l1), loss[q:q + 1])
            assert same_bytes(host(L._gradient(xp, d, r1)), np.ascontiguousarray(grad[q:q + 1]))
    # a second call of everything gives the same bytes
    resid2, loss2, _ = L._residual(xp, d, dev(w.reshape(4 * k, d + 1)), mode, k, y_d, sw, pw)
    assert same_bytes(host(resid2), resid) and same_bytes(host(loss2), loss) and same_bytes(host(L._gradient(xp, d, resid2)), grad)


# ------------------------------------------------------------------------------------------------ whole fits


def fit_problem(name):
    """(train x, y, held-out x, list of C, tol, max_iter)."""
    if name == "blobs":
        x, y = R.blobs()  # the CPU tests' problem; held-out rows around the same centres
        return x, y, R.blobs(n=100)[0], R.C_LIST, 1e-8, 2000
    x, y = R.golden_rows(2100)
    return x[:2000], y[:2000], x[2000:], [1e-4, 1e-3], 1e-7, 2000


def gradient_slack(x, y, w, c, total, mode, classes):
    """What the device's gradient of f may differ from the long-double one by at w (module docstring)."""
    n, d = x.shape
    _, rb, _ = R.bounds64(x, y, w, None, mode, None, classes)
    _, resid, _ = R.lr64(x, y, w, None, mode, None, classes)
    x1 = np.concatenate([np.abs(x).astype(LD), np.ones((n, 1), dtype=LD)], axis=1)
    gb = (rb.T @ x1 + (n + 1) * U * (np.abs(resid).T @ x1)) / total
    return float((gb + 3 * U * np.abs(w) / (c * total) + U * gb).max())


@pytest.mark.parametrize("name", ["blobs", "golden"])
def test_fit(name):
    from ssl_wafermap_amd.linear_model import LogisticRegression

    x, y, held, cs, tol, max_iter = fit_problem(name)
    n, d = x.shape
    x_dev, held_dev = dev(x), dev(held)
    classes = np.unique(y)
    k = len(classes)
    idx = np.searchsorted(classes, y).astype(np.int32)

    def fit(c, intercept):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # converges: no warning
            return LogisticRegression(c, fit_intercept=intercept, tol=tol, max_iter=max_iter).fit(x_dev, y)

    # two classes are the sigmoid form: one column, label 1 = classes_[1] (the first 2 000 golden rows hold two classes)
    if k == 2:
        mode, k_cols, target = 1, 1, (idx == 1).astype(np.int8)[:, None]
    else:
        mode, k_cols, target = 0, k, idx
    plain = fit(cs, False)
    assert plain.coef_.shape == (len(cs), k_cols, d) and plain.converged_.all() and (plain.n_iter_ >= 1).all()
    for i, c in enumerate(cs):
        w = R.with_zero_intercept(plain.coef_[i])
        g = R.objective64(x, target, w, None, c, mode, total=float(n))[1][:, :d]
        slack = gradient_slack(x, target, w, c, float(n), mode, k_cols)
        parity(f"fit {name} C={c:g}: long-double max |grad f| / (tol + the gradient kernel's bound)",
               float(np.abs(g).max()) / (tol + slack), 1.0)
        sk = R.sk_fit(x, y, c, False)
        dist, bound = R.strong_convexity_gap(x, target, w, R.with_zero_intercept(sk.coef_), None, c, mode, total=float(n))
        parity(f"fit {name} C={c:g}: ||W - W_sklearn|| / strong-convexity bound", dist / bound, 1.0)
    full = fit(cs, True)
    for i, c in enumerate(cs):
        sk = R.sk_fit(x, y, c, True)
        one = full[i]
        assert one.coef_.shape == sk.coef_.shape and one.intercept_.shape == sk.intercept_.shape
        assert np.array_equal(one.classes_, sk.classes_)
        assert np.array_equal(one.predict(x_dev), sk.predict(x.astype(np.float64)))
        assert one.score(x_dev, y) == float((sk.predict(x.astype(np.float64)) == y).mean())
    # the fitted model on held-out rows against lr64 at the model's own parameters
    one = full[len(cs) - 1]
    w = np.concatenate([one.coef_, one.intercept_[:, None]], axis=1)
    _, p_ref, _ = R.lr64(held, None, w, None, mode)
    dummy = np.zeros(len(held), dtype=np.int64) if mode == 0 else np.zeros((len(held), 1), dtype=np.int8)
    ez, _, _ = R.bounds64(held, dummy, w, None, mode)
    z_ref = held.astype(LD) @ w[:, :d].T.astype(LD) + w[:, d].astype(LD)
    z = host(one.decision_function(held_dev))
    proba = host(one.predict_proba(held_dev))
    assert proba.dtype == np.float64 and proba.shape == (len(held), k)
    if mode == 1:  # sklearn's shapes: decision_function [n], predict_proba [1 - p, p]
        assert z.shape == (len(held),)
        z = z[:, None]
    parity(f"fit {name}: decision_function error / E_z", float((np.abs(z - z_ref) / ez).max()), 1.0)
    if mode == 0:
        lse = np.log(np.exp(z_ref - z_ref.max(1, keepdims=True)).sum(1, keepdims=True)) + z_ref.max(1, keepdims=True)
        rho = ez + ez.max(1, keepdims=True) + (2 * k + 3) * U + 4 * U * np.log(LD(k)) + U * np.abs(lse) + U * np.abs(z_ref - lse) + 4 * U
        pb = p_ref * rho * (1 + 1e-3)
    else:  # sigma's bound (module docstring: E_z + 7 u relative); 1 - p is one more subtraction
        pb1 = p_ref * (ez + 7 * U) * (1 + 1e-3)
        p_ref, pb = np.concatenate([1 - p_ref, p_ref], axis=1), np.concatenate([pb1 + U * (1 - p_ref), pb1], axis=1)
    parity(f"fit {name}: predict_proba error / bound", float((np.abs(proba - p_ref) / (pb + LD(1e-300))).max()), 1.0)
    # a C fitted alone equals the same C in the list, and two fits give the same bits
    alone = fit(cs[-1], True)
    assert same_bytes(alone.coef_, one.coef_) and same_bytes(alone.intercept_, one.intercept_)
    assert np.array_equal(alone.n_iter_, one.n_iter_)
    again = fit(cs, True)
    assert same_bytes(again.coef_, full.coef_) and same_bytes(again.intercept_, full.intercept_)
    assert np.array_equal(again.n_iter_, full.n_iter_)


def test_two_class_and_multilabel_fits():
    from ssl_wafermap_amd.linear_model import ConvergenceWarning, LogisticRegression, MultilabelLogisticRegression

    x, y3 = R.blobs(n=500, d=12, k=3, seed=4)
    y = np.array([-5, 2])[(y3 > 0).astype(int)]
    y[::17] = -1
    x_dev = dev(x)
    model = LogisticRegression(0.5, class_weight="balanced", tol=1e-8, max_iter=2000).fit(x_dev, y)
    keep = y != -1
    sk = R.sk_fit(x[keep], y[keep], 0.5, True, "balanced")
    assert model.coef_.shape == (1, 12) == sk.coef_.shape and model.classes_.tolist() == [-5, 2]
    assert np.abs(model.coef_ - sk.coef_).max() <= 1e-5 and np.abs(model.intercept_ - sk.intercept_).max() <= 1e-5
    assert np.array_equal(model.predict(x_dev), sk.predict(x.astype(np.float64)))
    proba = host(model.predict_proba(x_dev))
    assert proba.shape == (500, 2) and np.abs(proba - sk.predict_proba(x.astype(np.float64))).max() <= 1e-5
    assert host(model.decision_function(x_dev)).shape == (500,)
    # multilabel: one sigmoid problem per (C, label), sklearn's with the equivalent sample_weight
    rng = np.random.default_rng(6)
    yl = ((x @ rng.standard_normal((12, 3)) + rng.standard_normal((500, 3))) > np.array([0.0, 0.8, -0.5])).astype(np.int64)
    cs = [0.1, 1.0]
    ml = MultilabelLogisticRegression(cs, pos_weight="balanced", fit_intercept=False, tol=1e-9, max_iter=2000).fit(x_dev, yl)
    pos = yl.mean(0)
    pw = (1 - pos) / pos
    for i, c in enumerate(cs):
        for l in range(3):
            sw = np.where(yl[:, l] == 1, pw[l], 1.0)
            sk = R.sk_fit(x, yl[:, l], c, False, None, sw)
            dist, bound = R.strong_convexity_gap(x, yl[:, l:l + 1], R.with_zero_intercept(ml.coef_[i, l:l + 1]),
                                                 R.with_zero_intercept(sk.coef_), sw, c, 1)
            parity(f"multilabel fit C={c:g} label {l}: ||w - w_sklearn|| / strong-convexity bound", dist / bound, 1.0)
    one = ml[1]
    pr = host(one.predict_proba(x_dev))
    assert pr.shape == (500, 3) and np.array_equal(one.predict(x_dev), (pr > 0.5).astype(np.int8))
    alone = MultilabelLogisticRegression(1.0, pos_weight="balanced", fit_intercept=False, tol=1e-9, max_iter=2000).fit(x_dev, yl)
    assert same_bytes(alone.coef_, one.coef_) and np.array_equal(alone.n_iter_, one.n_iter_)
    with pytest.warns(ConvergenceWarning):
        short = LogisticRegression(1.0, tol=1e-12, max_iter=3).fit(x_dev, y3)
    assert short.n_iter_.tolist() == [3] and not short.converged_.any()
    with pytest.raises(TypeError):
        ml.predict(x_dev)
    with pytest.raises(ValueError):
        one.predict(dev(x[:, :5]))


# ------------------------------------------------------------------------------------------------ the script


def test_probe_script_on_wafer_embeddings(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("embedding_probe_amd", R.ROOT / "scripts" / "embedding_probe_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # 60 iterations do not converge the largest C: the script says so itself
        summary = mod.main(["--embeddings", str(R.GOLDEN / "simsiam_preds_subset.npz"), "--C", "1e-4:1e-2:3", "--holdout", "1000",
                            "--max-iter", "60", "--out", str(tmp_path)])
    with open(tmp_path / "trials.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == 3 and list(table[0]) == mod.COLUMNS
    assert [float(r["C"]) for r in table] == pytest.approx([1e-4, 1e-3, 1e-2])
    for name in ("coef.npy", "intercept.npy", "proba.npy", "summary.json"):
        assert (tmp_path / name).exists(), name
    with open(tmp_path / "summary.json") as fh:
        assert json.load(fh)["chosen_C"] == summary["chosen_C"]
    best = max(table, key=lambda r: float(r["holdout_accuracy"]))
    assert float(best["C"]) == pytest.approx(summary["chosen_C"])
    labels = np.load(R.GOLDEN / "simsiam_preds_subset.npz")["labels"].astype(np.int64)
    held = labels[summary["holdout_rows"]]
    majority = float(np.bincount(held).max()) / len(held)
    assert len(held) == 1000 and summary["holdout_accuracy"] > majority  # a sanity floor, not a benchmark
    k = len(np.unique(labels[summary["train_rows"]]))
    assert np.load(tmp_path / "coef.npy").shape == (k, 512) and np.load(tmp_path / "intercept.npy").shape == (k,)
    proba = np.load(tmp_path / "proba.npy")
    assert proba.shape == (1000, k) and np.abs(proba.sum(1) - 1).max() <= 1e-12
    assert "held-out" in capsys.readouterr().out
