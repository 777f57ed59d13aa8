"""GPU checks of the label spreading / propagation kernels (csrc/propagate.hip) and the estimators built on them
(semi_supervised.LabelSpreading, LabelPropagation) against numpy float64, the restatement in
tests/test_label_spreading_cpu.py and sklearn.

Bounds are derived, not tuned.  u = 2^-53.
  (a) Exact cases.  A circulant graph of degree 4 or 16 with unit weights has dinv = 1/2 or 1/4; with alpha = 1/2 and
      one-hot labels every product and partial sum of three steps is a dyadic number of fewer than 30 bits: any order gives
      numpy's bits, for F and for the residuals alike.
  (b) One step.  The gather of a row of K entries adds K terms, each the product of three factors (2 roundings), with
      K - 1 additions: within (K + 1) u sum|terms| of the exact sum.  The row factor (dinv_i, or dinv_i^2) and alpha add
      2 u, the final addition of (1 - alpha) y one more u on the whole and 2 u on that term (1 - alpha and the product).
      Two computations (device, numpy): per entry 2 (K + 5) u a_i r_i sum_p |w_p cs_j F_jq| + 2 u |b_i y|, with a_i = alpha
      (1 in propagation), b_i = 1 - alpha (0 in propagation) and r_i the row factor.  In propagation the row factor
      includes the division by the row's sum over the classes, r_i = dinv_i^2 / sum_c t_c; every term is non-negative
      there, so the sum over C classes and the division add (C + 1) u relative, which the derivation would put on top
      ((2 K + C + 6) u per side); the test asserts the smaller figure above all the same.  An empty row has no terms: the
      result is (1 - alpha) y, or 0, exactly; a labelled row of a propagation step is y exactly (bound 0).
  (c) The residual is a sum of n C non-negative numbers, each within one rounding of the difference of the two F: within
      (n C + 1) u of the exact sum in any order; two computations: 2 (n C + 2) u sum|Fout - Fin|.
  (e) Division and comparison are exact operations on equal operands: bit equality.
  (f) A sum of k non-negative terms, then a sum of C of them and a division: per side (k - 1) u + (C - 1) u + u relative;
      two computations: 2 (k + C) u times the reference value.
  (g) The fit.  The affine map contracts with factor alpha, so the error of t steps is at most t times the error of one
      (a first-order statement: the constants of the weighted norm in which S contracts are left out): E = t (2 (K_max + 5) u M + 2 u) with M = alpha max_i dinv_i sum_p w_p dinv_j >= any a_i r_i
      sum|terms| for F in [0, 1].  A distribution is F / rowsum: |d dist| <= (1 + C) E / rowsum + 2 u per entry.  Labels are
      compared on the rows whose two largest reference probabilities are further apart than that bound; the others (at
      most 1 % of the rows, asserted on the reference alone) are too close to call.
"""
import numpy as np
import pytest
import torch
from parity_log import parity

from test_gpu_spectral import bits, circulant, dev, host, random_symmetric, to_csr, worst
from test_label_spreading_cpu import (golden_case, one_hot, ref_degree, ref_finalize, ref_propagate, ref_step, sklearn_fit)
from test_spectral_cpu import golden_labels, golden_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
SENTINEL = -7.25


def S():
    from ssl_wafermap_amd import semi_supervised

    return semi_supervised


def M():
    from ssl_wafermap_amd import manifold

    return manifold


def padded(F, pad):
    """F on the device inside a wider buffer whose extra columns hold the sentinel."""
    buf = np.full((F.shape[0], F.shape[1] + pad), SENTINEL)
    buf[:, :F.shape[1]] = F
    return dev(buf)


def run_steps(csr, dinv, labels, classes, alphas, F0, iters, hard=False, active=None, pad=3):
    """`iters` steps from F0 through semi_supervised.propagate on padded buffers: (F [n, cols], resid [iters, groups],
    the two raw buffers)."""
    groups = len(alphas)
    Fa = padded(F0, pad)
    Fb = torch.full_like(Fa, SENTINEL)
    act = dev(np.ones(groups, dtype=np.int32) if active is None else np.asarray(active, dtype=np.int32))
    out, resid = S().propagate(csr, dinv, dev(labels), classes, dev(np.asarray(alphas, dtype=np.float64)), act, Fa, Fb, iters, hard=hard)
    assert out is (Fb if iters % 2 else Fa)
    return host(out)[:, :classes * groups], host(resid), (host(Fa), host(Fb))


def ref_steps(g, labels, classes, alphas, F0, iters, hard=False, active=None):
    _, dinv = ref_degree(g)
    F, resids = F0, []
    for _ in range(iters):
        F, r, _ = ref_step(g, dinv, labels, classes, alphas, F, hard, active)
        resids.append(r)
    return F, np.array(resids)


# ------------------------------------------------------------------------------------------------ (a) exact cases


@pytest.mark.parametrize("C", [1, 2, 9, 16, 17, 64, 65, 256])
@pytest.mark.parametrize("n", [1, 3, 17, 255, 256, 257])
def test_three_steps_are_exact_on_circulant_graphs(n, C):
    degree = 16 if (n + C) % 2 else 4
    g = circulant(n, degree)
    csr = to_csr(g)
    _, dinv = M().laplacian_degree(csr)
    assert np.array_equal(host(dinv), np.full(n, 1.0 / np.sqrt(degree)))
    rows = np.arange(n)
    labels = np.where(rows % 3 == 0, (rows // 3) % C, -1).astype(np.int32)
    pad = 3
    init = torch.full((n, C + pad), SENTINEL, dtype=torch.float64, device=DEV)
    S().label_matrix(dev(labels), C, 1, out=init)
    F0 = one_hot(labels, C)
    assert np.array_equal(host(init)[:, :C], F0) and (host(init)[:, C:] == SENTINEL).all()
    got, resid, (Fa, Fb) = run_steps(csr, dinv, labels, C, [0.5], F0, 3, pad=pad)
    want, want_resid = ref_steps(g, labels, C, [0.5], F0, 3)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(resid), bits(want_resid))
    assert (Fa[:, C:] == SENTINEL).all() and (Fb[:, C:] == SENTINEL).all()  # the padding columns are never written


@pytest.mark.parametrize("n, groups, C", [(17, 15, 9), (257, 1, 130), (256, 3, 64)])
def test_three_column_slots_per_lane_are_exact(n, groups, C):
    """129 .. 192 columns: the instantiation with three columns per lane, which the sizes above do not reach; several
    groups at once with alpha = 1/2, 1/4, 1/8, ... (dyadic, so every value stays exact)."""
    g = circulant(n, 4)
    csr = to_csr(g)
    _, dinv = M().laplacian_degree(csr)
    rows = np.arange(n)
    labels = np.where(rows % 3 == 0, (rows // 3) % C, -1).astype(np.int32)
    alphas = [0.5 ** (1 + k % 3) for k in range(groups)]
    assert 128 < groups * C <= 192
    F0 = one_hot(labels, C, groups)
    got, resid, (Fa, Fb) = run_steps(csr, dinv, labels, C, alphas, F0, 3)
    want, want_resid = ref_steps(g, labels, C, alphas, F0, 3)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(resid), bits(want_resid))
    assert (Fa[:, groups * C:] == SENTINEL).all() and (Fb[:, groups * C:] == SENTINEL).all()


def test_label_matrix_repeats_per_group():
    labels = np.array([2, -1, 0, 1, -1, 2, 2], dtype=np.int32)
    got = host(S().label_matrix(dev(labels), 3, 4))
    assert np.array_equal(got, one_hot(labels, 3, 4))


# ------------------------------------------------------------------------------------------------ (b), (c) one step

_RANDOM = {}


def random_case():
    """(graph, csr, dinv on the device, labels, F0 [n, 27]) at n = 700: rows of 0, 1, 15, 16, 17 and 300 entries, the empty
    row labelled; F0 random in [0, 1)."""
    if not _RANDOM:
        n = 700
        g = random_symmetric(n, 41, lengths=(0, 1, 15, 16, 17, 300))
        assert np.diff(g.indptr)[:6].tolist() == [0, 1, 15, 16, 17, 300]
        rng = np.random.default_rng(8)
        labels = np.where(rng.random(n) < 0.3, rng.integers(0, 9, size=n), -1).astype(np.int32)
        labels[0], labels[1], labels[5] = 2, -1, -1
        csr = to_csr(g)
        _, dinv = M().laplacian_degree(csr)
        _RANDOM.update(g=g, csr=csr, dinv=dinv, labels=labels, F0=rng.random((n, 27)))
    return _RANDOM


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("alphas", [[0.3], [0.2, 0.5, 0.9]])
def test_one_step_against_float64(alphas, hard):
    c = random_case()
    g, labels = c["g"], c["labels"]
    cols = 9 * len(alphas)
    F0 = c["F0"][:, :cols].copy()
    got, resid, _ = run_steps(c["csr"], c["dinv"], labels, 9, alphas, F0, 1, hard=hard)
    want, want_resid, mag = ref_step(g, ref_degree(g)[1], labels, 9, alphas, F0, hard)
    K = np.diff(g.indptr)[:, None]
    b = 0.0 if hard else (1.0 - np.repeat(np.asarray(alphas), 9))[None, :]
    bound = 2 * (K + 5) * U * mag + 2 * U * np.abs(b * one_hot(labels, 9, len(alphas)))
    name = f"lp step {'hard' if hard else 'soft'} R={len(alphas)}"
    parity(f"{name} / bound", worst(np.abs(got - want), bound), 1.0)
    empty = np.diff(g.indptr) == 0
    assert empty[0] and np.array_equal(bits(got[empty]), bits(want[empty]))
    assert np.array_equal(got[0], one_hot(labels, 9, len(alphas))[0] * (1.0 if hard else 1.0 - np.repeat(np.asarray(alphas), 9)))
    if hard:
        known = labels >= 0
        assert np.array_equal(got[known], one_hot(labels, 9, len(alphas))[known])
        rs = got[~known].reshape(-1, len(alphas), 9).sum(axis=2)  # propagation keeps every reached row a distribution
        assert np.all((np.abs(rs - 1.0) <= 2 * (9 + 1) * U) | (rs == 0.0))
    # (c) the residual, and two calls give the same bits
    total = np.abs(want - F0).reshape(700, len(alphas), 9).sum(axis=(0, 2))
    parity(f"{name} residual / bound", worst(np.abs(resid[0] - want_resid), 2 * (700 * 9 + 2) * U * total), 1.0)
    again, resid2, _ = run_steps(c["csr"], c["dinv"], labels, 9, alphas, F0, 1, hard=hard)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(bits(resid), bits(resid2))


# ------------------------------------------------------------------------------------------------ (d) frozen groups


@pytest.mark.parametrize("hard", [False, True])
def test_frozen_groups_are_copied_and_leave_the_others_alone(hard):
    c = random_case()
    alphas, labels = [0.2, 0.5, 0.9], c["labels"]
    F0 = c["F0"].copy()
    got, resid, _ = run_steps(c["csr"], c["dinv"], labels, 9, alphas, F0, 5, hard=hard, active=[1, 0, 1])
    assert np.array_equal(bits(got[:, 9:18]), bits(F0[:, 9:18])) and (resid[:, 1] == 0.0).all()
    two = np.concatenate([F0[:, :9], F0[:, 18:]], axis=1)
    alone, resid_alone, _ = run_steps(c["csr"], c["dinv"], labels, 9, [0.2, 0.9], two, 5, hard=hard)
    assert np.array_equal(bits(got[:, :9]), bits(alone[:, :9])) and np.array_equal(bits(got[:, 18:]), bits(alone[:, 9:]))
    assert np.array_equal(bits(resid[:, [0, 2]]), bits(resid_alone))  # the residual's order does not depend on the group count


# ------------------------------------------------------------------------------------------------ (e) finalize


@pytest.mark.parametrize("C", [1, 9, 38])
def test_finalize_is_exact(C):
    n, groups, g = 300, 3, 1
    rng = np.random.default_rng(C)
    F = rng.random((n, groups * C + 2))
    block = F[:, g * C:(g + 1) * C]
    block[::7] = 0.0  # unreached rows
    if C > 1:
        block[1::7, C - 1] = block[1::7, 0] = 2.0  # ties: the first maximum wins
        block[2::7] = 0.25  # every class equal
    dist, rowsum, pred, unreached = S().finalize_labels(dev(F), C, g)
    want_dist, want_sum, want_pred, want_un = ref_finalize(block)
    assert np.array_equal(bits(host(rowsum)), bits(want_sum)) and np.array_equal(bits(host(dist)), bits(want_dist))
    assert np.array_equal(host(pred), want_pred) and host(pred).dtype == np.int32
    assert np.array_equal(host(unreached), want_un) and want_un[::7].all() and (host(pred)[::7] == 0).all()
    assert (host(dist)[::7] == 0.0).all()


# ------------------------------------------------------------------------------------------------ (f) neighbour mean


@pytest.mark.parametrize("k", [1, 7, 15])
def test_neighbor_mean_against_float64(k):
    n, m, C = 200, 77, 9
    rng = np.random.default_rng(k)
    dist = rng.random((n, C))
    dist[:20] = 0.0  # unreached fitted rows
    dist /= np.where(dist.sum(axis=1, keepdims=True) == 0, 1.0, dist.sum(axis=1, keepdims=True))
    idx = rng.integers(0, n, size=(m, k)).astype(np.int32)
    idx[0] = rng.integers(0, 20, size=k)  # only unreached neighbours
    idx[1, 0] = 5  # one unreached neighbour among reached ones (k > 1)
    got = host(S().neighbor_mean(dev(idx), dev(dist)))
    sums = np.cumsum(dist[idx], axis=1)[:, -1]  # t order
    tot = np.cumsum(sums, axis=1)[:, -1:]
    want = np.where(tot == 0, 0.0, sums / np.where(tot == 0, 1.0, tot))
    parity(f"lp neighbor mean k={k} / bound", worst(np.abs(got - want), 2 * (k + C) * U * want), 1.0)
    rs = got.sum(axis=1)
    assert (got[0] == 0.0).all() and np.all((np.abs(rs - 1.0) <= 2 * (C + 1) * U) | (rs == 0.0))


# ------------------------------------------------------------------------------------------------ (g), (h) estimators


def fit_bound(g, alpha, steps, C, F_ref):
    """Per-row bound of |dist - reference dist| after `steps` steps, docstring (g)."""
    _, dinv = ref_degree(g)
    K = int(np.diff(g.indptr).max())
    M_ = alpha * float((dinv * (g.astype(np.float64) @ dinv)).max())
    E = steps * (2 * (K + 5) * U * M_ + 2 * U)
    rowsum = F_ref.sum(axis=1)
    return np.where(rowsum > 0, (1 + C) * E / np.where(rowsum > 0, rowsum, 1.0) + 2 * U, 0.0)


@pytest.mark.parametrize("alpha", [0.2, 0.8])
def test_label_spreading_matches_sklearn(alpha):
    x, g, labels, _, classes = golden_case()
    C, n = len(classes), x.shape[0]
    F_ref, n_ref, hist = ref_propagate(g, labels, C, [alpha], max_iter=100, tol=1e-3)
    assert (np.abs(hist[:, 0] - 1e-3) > 1e-9 * 1e-3).all()  # no residual sits on the threshold
    sk = sklearn_fit("spreading", g, x, labels, alpha=alpha, max_iter=100, tol=1e-3)
    assert n_ref[0] == sk.n_iter_ and 1 < sk.n_iter_ < 100
    model = S().LabelSpreading(alpha=alpha, max_iter=100, tol=1e-3, affinity=to_csr(g), check_every=1).fit(dev(x), labels)
    assert model.n_iter_ == sk.n_iter_ and np.array_equal(model.classes_, np.arange(C))
    bound = fit_bound(g, alpha, sk.n_iter_, C, F_ref)
    ref_sorted = np.sort(sk.label_distributions_, axis=1)
    gap = ref_sorted[:, -1] - (ref_sorted[:, -2] if C > 1 else 0.0)
    reached = F_ref.sum(axis=1) > 0
    compare = ~reached | (gap > bound)
    assert (~compare).sum() <= 0.01 * n  # the reference alone: few rows are too close to call
    assert np.array_equal(model.transduction_[compare], sk.transduction_[compare])
    assert np.array_equal(model.unreached_, ~reached)
    diff = np.abs(model.label_distributions_ - sk.label_distributions_).max(axis=1)
    parity(f"lp fit alpha={alpha} vs sklearn / bound", worst(diff, bound), 1.0)
    assert model.residuals_.shape == hist[:, 0].shape
    assert (np.abs(model.residuals_ - hist[:, 0]) <= 1e-9 * hist[:, 0]).all()  # far inside the margin asserted above


def test_label_propagation_matches_sklearn():
    x, g, labels, _, classes = golden_case()
    C = len(classes)
    F_ref, n_ref, hist = ref_propagate(g, labels, C, [0.5], hard=True, max_iter=300, tol=0.1)
    assert (np.abs(hist[:, 0] - 0.1) > 1e-9 * 0.1).all()
    sk = sklearn_fit("propagation", g, x, labels, max_iter=300, tol=0.1)
    model = S().LabelPropagation(max_iter=300, tol=0.1, affinity=to_csr(g), check_every=1).fit(dev(x), labels)
    assert model.n_iter_ == sk.n_iter_ == n_ref[0] and 1 < sk.n_iter_ < 300
    known = labels >= 0
    assert np.array_equal(model.label_distributions_[known], one_hot(labels, C)[known])  # clamped
    # the renormalised map is no contraction with a known factor: the steps' bounds add up with the factor 1 per step
    bound = fit_bound(g, 1.0, sk.n_iter_, C, F_ref)
    diff = np.abs(model.label_distributions_ - sk.label_distributions_).max(axis=1)
    parity("lp propagation fit vs sklearn / bound", worst(diff, bound), 1.0)


def test_a_list_of_alphas_equals_the_single_fits():
    x, g, labels, _, classes = golden_case()
    csr, xd = to_csr(g), dev(x)
    both = S().LabelSpreading(alpha=[0.2, 0.8], max_iter=100, affinity=csr).fit(xd, labels)
    assert both.label_distributions_.shape == (2, x.shape[0], len(classes)) and both.n_iter_.shape == (2,)
    assert both.n_iter_[0] < both.n_iter_[1] and both.n_iter_[0] % 8 == 0  # per group, at a chunk boundary
    for k, alpha in enumerate([0.2, 0.8]):
        one = S().LabelSpreading(alpha=alpha, max_iter=100, affinity=csr).fit(xd, labels)
        assert one.n_iter_ == both.n_iter_[k]
        assert np.array_equal(bits(one.label_distributions_), bits(both.label_distributions_[k]))
        assert np.array_equal(one.transduction_, both.transduction_[k]) and np.array_equal(one.unreached_, both.unreached_[k])
        assert np.array_equal(bits(one.residuals_), bits(both.residuals_[:one.n_iter_, k]))
        assert np.isnan(both.residuals_[one.n_iter_:, k]).all()


# ------------------------------------------------------------------------------------------------ (i) unreached, new rows


def test_unreached_rows_and_new_rows():
    n_fit, n_new, n_far = 400, 40, 20
    rows, truth = golden_rows(n_fit + n_new), golden_labels(n_fit + n_new).astype(np.int64)
    far = rows[:n_far] * 0.01 + 100.0  # a tight clump far away: a component of its own, without a label
    x = np.concatenate([rows[:n_fit], far]).astype(np.float32)
    y = np.concatenate([truth[:n_fit] + 10, np.full(n_far, -1)])  # (labels that are not their own codes)
    y[np.random.default_rng(2).random(n_fit + n_far) > 0.15] = -1
    model = S().LabelSpreading(n_neighbors=7, alpha=0.5, max_iter=40, check_every=1).fit(dev(x), y)
    g = model.affinity_matrix_.to_scipy().copy()
    g.sort_indices()
    classes, codes = np.unique(y[y >= 0], return_inverse=True)
    labels = np.full(y.shape[0], -1, dtype=np.int32)
    labels[y >= 0] = codes
    assert np.array_equal(model.classes_, classes) and g.diagonal().sum() == 0
    F_ref, n_ref, _ = ref_propagate(g, labels, len(classes), [0.5], max_iter=40, tol=1e-3)
    want_dist, _, want_pred, want_un = ref_finalize(F_ref)
    assert want_un[n_fit:].all()  # the clump is its own component
    assert model.n_iter_ == n_ref[0]
    assert np.array_equal(model.unreached_, want_un) and (model.label_distributions_[want_un] == 0.0).all()
    parity("lp fit (device graph) vs restatement / bound",
           worst(np.abs(model.label_distributions_ - want_dist).max(axis=1), fit_bound(g, 0.5, n_ref[0], len(classes), F_ref)), 1.0)
    sk = sklearn_fit("spreading", g, x, labels, alpha=0.5, max_iter=40, tol=1e-3)
    assert np.array_equal(model.transduction_[want_un], classes[sk.transduction_[want_un]])
    assert (model.transduction_[want_un] == classes[0]).all()
    # new rows: golden rows the fit has not seen, and one next to the clump (all its neighbours unreached)
    new = np.concatenate([rows[n_fit:], far[:1] + 0.001]).astype(np.float32)
    proba = model.predict_proba(dev(new))
    _, idx = M().knn_query(dev(new), dev(x), 7)
    sums = np.cumsum(model.label_distributions_[host(idx)], axis=1)[:, -1]
    tot = np.cumsum(sums, axis=1)[:, -1:]
    want = np.where(tot == 0, 0.0, sums / np.where(tot == 0, 1.0, tot))
    parity("lp predict_proba / bound", worst(np.abs(proba - want), 2 * (7 + len(classes)) * U * want), 1.0)
    assert (proba[-1] == 0.0).all() and model.predict(dev(new))[-1] == classes[0]
    assert np.array_equal(model.predict(dev(new)), classes[np.argmax(want, axis=1)])
