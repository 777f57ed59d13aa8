"""CPU checks of label spreading / propagation (ssl_wafermap_amd.semi_supervised, csrc/propagate.hip) and the float64 numpy
restatement `ref_propagate` that tests/test_gpu_label_spreading.py compares the kernels against.  No GPU: nothing here
launches a kernel.

Bounds, u = 2^-53.
  1. The restatement against sklearn.  Both iterate the same map in float64 from the same graph; they differ in how the
     normalised weights are formed (sklearn divides each weight by sqrt(deg_i) and by sqrt(deg_j), or by deg_i; the
     restatement multiplies sums by dinv) and in the order of each row's sum.  A step of a row of K <= 40 entries is within
     (K + 5) u of the exact one relative to sum |terms|, which is at most sqrt(deg_max / deg_min) < 3 for distributions in
     [0, 1]; the map contracts with alpha, so the t <= 30 steps to tol = 1e-3 leave at most t (K + 5) 3 u < 5e-13 in F per
     side in the worst case, and far less in fact because roundings do not line up.  The test asserts 1e-14 on the
     normalised distributions, tighter than that worst case: about 90 u, what a few dozen roundings that do not line up
     leave (measured: 4e-16), so that a lost term or a wrong factor cannot hide.  n_iter_ must be equal.  sklearn's
     LabelPropagation renormalises every row inside its loop, which the restatement (and the kernel) therefore do too; its
     sparse branch divides every weight by the degree of row 0, so it is given the dense matrix of the same graph.
  2. The closed form F* = (1 - alpha) (I - alpha S)^-1 Y: after t steps |F_t - F*| <= alpha^t |F_0 - F*| in the norm in
     which S is a contraction (S is similar to the row-stochastic D^-1 G: factor sqrt(deg_max / deg_min) between the
     norms); t is chosen so that alpha^t sqrt(deg_max / deg_min) n < 1e-13, and numpy's solve adds cond(I - alpha S) n u
     <= n u / (1 - alpha).
"""
import warnings

import numpy as np
import pytest

from test_spectral_cpu import golden_labels, golden_rows, ref_knn

U = 2.0 ** -53
EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -4


# ------------------------------------------------------------------------------------------------ float64 restatement


def ref_connectivity(x, k):
    """manifold.connectivity_graph without its diagonal, float32 scipy CSR: 0.5 (A + A^T) of the kNN indicator (the row
    itself among the k), entries 1.0 where two rows list each other and 0.5 where one does."""
    from scipy.sparse import coo_matrix

    n = x.shape[0]
    _, idx = ref_knn(x, k)
    a = coo_matrix((np.ones(n * k), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n)).tocsr()
    g = (0.5 * (a + a.T)).tolil()
    g.setdiag(0.0)
    g = g.tocsr()
    g.eliminate_zeros()
    g.sort_indices()
    return g.astype(np.float32)


def ref_degree(g):
    """(deg, dinv) in wm_spec_degree's order: the row's entries in storage order, one accumulator."""
    d64 = g.data.astype(np.float64)
    deg = np.array([np.cumsum(d64[g.indptr[i]:g.indptr[i + 1]])[-1] if g.indptr[i + 1] > g.indptr[i] else 0.0
                    for i in range(g.shape[0])])
    return deg, np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)


def one_hot(labels, classes, groups=1):
    y = np.zeros((labels.shape[0], classes))
    known = labels >= 0
    y[np.flatnonzero(known), labels[known]] = 1.0
    return np.tile(y, (1, groups))


def ref_residual(diff, classes, groups):
    """sum |Fout - Fin| per group in the kernel's order: a row's classes in class order, quads of rows as
    ((r0 + r1) + r2) + r3, thread t of 256 adds the quads t, t + 256, ..., then s[t] += s[t + h] for h = 128 .. 1."""
    n = diff.shape[0]
    out = np.zeros(groups)
    for g in range(groups):
        d = diff[:, g * classes:(g + 1) * classes]
        rows = np.cumsum(d, axis=1)[:, -1]
        rows = np.concatenate([rows, np.zeros(-n % 4)]).reshape(-1, 4)
        quads = ((rows[:, 0] + rows[:, 1]) + rows[:, 2]) + rows[:, 3]
        s = np.zeros(256)
        for t in range(min(256, quads.shape[0])):
            s[t] = np.cumsum(quads[t::256])[-1]
        h = 128
        while h >= 1:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
        out[g] = s[0]
    return out


def ref_step(g, dinv, labels, classes, alphas, F, hard=False, active=None):
    """One step of wm_lp_iterate in its stated order: (Fout, resid [groups], mag) -- mag[i][q] = the row factor times
    sum_p |w_p cs_j F_jq|, the quantity the rounding bound of the gather is relative to (the row factor of a propagation
    step includes the division by the row's sum)."""
    n, groups = g.shape[0], len(alphas)
    cols = classes * groups
    d64 = g.data.astype(np.float64)
    cs = np.ones(n) if hard else dinv
    terms = d64[:, None] * (cs[g.indices][:, None] * F[g.indices, :cols])
    s = np.zeros((n, cols))
    mag = np.zeros((n, cols))
    for i in range(n):
        b, e = g.indptr[i], g.indptr[i + 1]
        if e > b:
            s[i] = np.cumsum(terms[b:e], axis=0)[-1]
            mag[i] = np.abs(terms[b:e]).sum(axis=0)
    y = one_hot(labels, classes, groups)
    a = np.repeat(np.asarray(alphas, dtype=np.float64), classes)[None, :]
    if hard:  # t = dinv^2 s, divided by its sum over the group's classes in class order (1 where that is 0)
        t = (dinv * dinv)[:, None] * s
        tot = np.concatenate([np.repeat(np.cumsum(t[:, k * classes:(k + 1) * classes], axis=1)[:, -1:], classes, axis=1)
                              for k in range(groups)], axis=1)
        tot = np.where(tot == 0, 1.0, tot)
        out = np.where((labels >= 0)[:, None], y, t / tot)
        mag = np.where((labels >= 0)[:, None], 0.0, ((dinv * dinv)[:, None] * mag) / tot)
    else:
        out = a * (dinv[:, None] * s) + (1.0 - a) * y
        mag = a * (dinv[:, None] * mag)
    if active is not None:
        frozen = np.repeat(np.asarray(active) == 0, classes)
        out[:, frozen] = F[:, :cols][:, frozen]
        mag[:, frozen] = 0.0
    return out, ref_residual(np.abs(out - F[:, :cols]), classes, groups), mag


def ref_propagate(g, labels, classes, alphas, hard=False, max_iter=30, tol=1e-3, check_every=1):
    """The estimator's fit in numpy float64: (F [n, groups * classes], n_iter [groups], residual history [steps, groups]
    with NaN once a group is frozen).  Chunks of `check_every` steps; a group whose residual is below tol at a chunk
    boundary is frozen."""
    groups = len(alphas)
    _, dinv = ref_degree(g)
    F = one_hot(labels, classes, groups)
    active = np.ones(groups, dtype=np.int32)
    n_iter = np.zeros(groups, dtype=np.int64)
    hist, done = [], 0
    while active.any() and done < max_iter:
        for _ in range(min(check_every, max_iter - done)):
            F, r, _ = ref_step(g, dinv, labels, classes, alphas, F, hard, active)
            hist.append(np.where(active != 0, r, np.nan))
            done += 1
        n_iter[active != 0] = done
        active[(active != 0) & (hist[-1] < tol)] = 0
    return F, n_iter, np.array(hist)


def ref_finalize(F):
    """(dist, rowsum, pred, unreached) of one group's columns, sklearn's rule for all-zero rows."""
    rowsum = np.cumsum(F, axis=1)[:, -1]
    dist = np.where(rowsum[:, None] == 0, 0.0, F / np.where(rowsum == 0, 1.0, rowsum)[:, None])
    return dist, rowsum, np.argmax(F, axis=1), rowsum == 0


_CASE = {}


def golden_case(n=600, k=7, frac=0.1, seed=0):
    """(x float32 [n, d], graph, label codes with -1 on the hidden rows, true codes, classes): `n` golden rows, their
    k-neighbour connectivity graph and a seeded draw that keeps `frac` of the labels.  Computed once."""
    key = (n, k, frac, seed)
    if key not in _CASE:
        x, truth = golden_rows(n), golden_labels(n).astype(np.int64)
        keep = np.random.default_rng(seed).random(n) < frac
        classes, codes = np.unique(truth[keep], return_inverse=True)
        labels = np.full(n, -1, dtype=np.int32)
        labels[keep] = codes
        _CASE[key] = (x, ref_connectivity(x, k), labels, truth, classes)
    return _CASE[key]


def sklearn_fit(kind, g, x, labels, **kw):
    from sklearn.semi_supervised import LabelPropagation, LabelSpreading

    # (sklearn's sparse branch of LabelPropagation divides every weight by the degree of row 0, not by its row's: the dense
    # matrix of the same graph takes the row-normalising branch)
    dense = g.astype(np.float64).toarray()
    if kind == "spreading":
        model = LabelSpreading(kernel=lambda a, b=None: g.astype(np.float64), **kw)
    else:
        model = LabelPropagation(kernel=lambda a, b=None: dense, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit(x.astype(np.float64), labels)
    return model


# ------------------------------------------------------------------------------------------------ 1, 2: the restatement


@pytest.mark.parametrize("kind, alpha", [("spreading", 0.2), ("spreading", 0.8), ("propagation", None)])
def test_restatement_matches_sklearn(kind, alpha):
    x, g, labels, _, classes = golden_case()
    C = len(classes)
    kw = {"alpha": alpha} if kind == "spreading" else {}
    tol = 1e-3 if kind == "spreading" else 0.1  # (propagation takes 721 steps to 1e-3 on this graph)
    sk = sklearn_fit(kind, g, x, labels, max_iter=300, tol=tol, **kw)
    F, n_iter, hist = ref_propagate(g, labels, C, [alpha or 0.5], hard=kind == "propagation", max_iter=300, tol=tol)
    dist, _, pred, _ = ref_finalize(F)
    assert n_iter[0] == sk.n_iter_ and 1 < n_iter[0] < 300
    assert np.abs(dist - sk.label_distributions_).max() <= 1e-14
    assert np.array_equal(np.arange(C)[pred], sk.transduction_)
    assert hist.shape == (n_iter[0], 1)


@pytest.mark.parametrize("alpha", [0.2, 0.8])
def test_restatement_reaches_the_closed_form(alpha):
    from test_gpu_spectral import random_symmetric

    n, C = 60, 4
    g = random_symmetric(n, 7, lengths=(1, 5))
    assert np.diff(g.indptr).min() >= 1
    rng = np.random.default_rng(3)
    labels = np.where(rng.random(n) < 0.3, rng.integers(0, C, size=n), -1).astype(np.int32)
    deg, dinv = ref_degree(g)
    S = dinv[:, None] * g.astype(np.float64).toarray() * dinv[None, :]
    want = (1.0 - alpha) * np.linalg.solve(np.eye(n) - alpha * S, one_hot(labels, C))
    ratio = np.sqrt(deg.max() / deg.min())
    steps = int(np.ceil(np.log(1e-13 / (ratio * n)) / np.log(alpha)))
    F, n_iter, _ = ref_propagate(g, labels, C, [alpha], max_iter=steps, tol=0.0)
    assert n_iter[0] == steps
    assert np.abs(F - want).max() <= 1e-13 + n * U / (1.0 - alpha)


# ------------------------------------------------------------------------------------------------ 3: host logic


def S():
    from ssl_wafermap_amd import semi_supervised

    return semi_supervised


@pytest.mark.parametrize("alpha", [0.0, 1.0, -0.1, 1.5, [0.2, 1.0], [], float("nan")])
def test_alpha_outside_the_open_interval_is_refused(alpha):
    with pytest.raises(ValueError):
        S().check_alphas(alpha)
    with pytest.raises(ValueError):
        S().LabelSpreading(alpha=alpha)


def test_alpha_forms():
    a, single = S().check_alphas(0.2)
    assert single and a.tolist() == [0.2]
    a, single = S().check_alphas([0.2, 0.8])
    assert not single and a.tolist() == [0.2, 0.8] and a.dtype == np.float64
    assert S().LabelPropagation()._hard and not S().LabelSpreading()._hard


def test_labels_and_column_limits():
    s = S()
    s.check_label_codes(np.array([-1, 0, 8]), 9)
    for bad in ([-2, 0], [0, 9]):
        with pytest.raises(ValueError):
            s.check_label_codes(np.array(bad), 9)
    assert s.check_columns(4, 9) == 36 and s.check_columns(1, 256) == 256
    for groups, classes in ((29, 9), (1, 257), (0, 9), (2, 0)):
        with pytest.raises(ValueError):
            s.check_columns(groups, classes)
    classes, codes = s.encode_labels(np.array([7, -1, 3, 7, -1]))
    assert classes.tolist() == [3, 7] and codes.tolist() == [1, -1, 0, 1, -1] and codes.dtype == np.int32
    with pytest.raises(ValueError):
        s.encode_labels(np.array([-1, -1]))
    with pytest.raises(ValueError):
        s.LabelSpreading(affinity="rbf")
    with pytest.raises(ValueError):
        s.LabelSpreading(n_neighbors=0)
    with pytest.raises(ValueError):
        s.LabelPropagation(check_every=0)


def test_chunks_and_freezing_follow_the_residual_table():
    """A fake residual table: group 0 falls below tol at step 3, group 1 at step 9, group 2 never (max_iter 20)."""
    steps = np.arange(1, 21)
    table = np.stack([np.where(steps >= 3, 1e-4, 1.0), np.where(steps >= 9, 1e-4, 1.0), np.ones(20)], axis=1)

    def run(check_every, tol=1e-3, max_iter=20):
        plan = S().ChunkPlan(3, max_iter, tol, check_every)
        chunks, actives = [], []
        while plan.next_chunk():
            k = plan.next_chunk()
            chunks.append(k)
            actives.append(plan.active.tolist())
            plan.record(table[plan.done:plan.done + k])
        return plan, chunks, actives

    plan, chunks, actives = run(1)
    assert chunks == [1] * 20 and plan.n_iter.tolist() == [3, 9, 20]  # sklearn's n_iter_: the first step below tol
    assert actives[2] == [1, 1, 1] and actives[3] == [0, 1, 1] and actives[9] == [0, 0, 1]
    res = plan.residuals
    assert res.shape == (20, 3) and np.isnan(res[3:, 0]).all() and np.array_equal(res[:3, 0], table[:3, 0])
    assert np.isnan(res[9:, 1]).all() and not np.isnan(res[:, 2]).any()

    plan, chunks, actives = run(8)  # boundaries at 8, 16, 20: frozen at the first boundary at or behind the crossing
    assert chunks == [8, 8, 4] and plan.n_iter.tolist() == [8, 16, 20]
    assert actives == [[1, 1, 1], [0, 1, 1], [0, 0, 1]]

    plan, chunks, _ = run(8, max_iter=10)  # the last chunk is cut to max_iter
    assert chunks == [8, 2] and plan.n_iter.tolist() == [8, 10, 10]

    plan, chunks, _ = run(4, tol=10.0)  # everything below tol at the first boundary: the fit ends there
    assert chunks == [4] and plan.n_iter.tolist() == [4, 4, 4] and plan.next_chunk() == 0

    plan = S().ChunkPlan(3, 20, 1e-3, 8)
    with pytest.raises(ValueError):
        plan.record(table[:3])  # not the chunk that was asked for
    for bad in ((0, 1e-3, 8), (20, -1.0, 8), (20, 1e-3, 0)):
        with pytest.raises(ValueError):
            S().ChunkPlan(3, *bad)


# ------------------------------------------------------------------------------------------------ 4: the library


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_argument_validation_needs_no_gpu(lib):
    """Every wm_lp_* refuses null pointers, sizes beyond its limits, misaligned pointers and a short workspace before any
    launch (the pointers below are never dereferenced: no call here passes its checks)."""
    P, ODD = 0x10000, 0x10004  # aligned to 16 / to 4 only
    BIG = 1 << 30
    # companions: 0 for what they refuse
    assert lib.wm_lp_init_workspace_bytes(100, 9, 4) == 256
    assert lib.wm_lp_iterate_workspace_bytes(100, 9, 4) == 4 * 25 * 8 and lib.wm_lp_iterate_workspace_bytes(101, 9, 1) == 26 * 8
    assert lib.wm_lp_finalize_workspace_bytes(100, 9) == 256 and lib.wm_lp_neighbor_mean_workspace_bytes(10, 7, 9) == 256
    for n, classes, groups in ((0, 9, 1), ((1 << 24) + 1, 9, 1), (100, 0, 1), (100, 9, 0), (100, 9, 29), (100, 257, 1)):
        assert lib.wm_lp_init_workspace_bytes(n, classes, groups) == 0
        assert lib.wm_lp_iterate_workspace_bytes(n, classes, groups) == 0
    assert lib.wm_lp_iterate_workspace_bytes(1 << 24, 1, 256) == 256 * (1 << 22) * 8  # (size_t arithmetic)
    assert lib.wm_lp_finalize_workspace_bytes(100, 257) == 0 and lib.wm_lp_finalize_workspace_bytes((1 << 24) + 1, 9) == 0
    assert lib.wm_lp_neighbor_mean_workspace_bytes(10, 65, 9) == 0 and lib.wm_lp_neighbor_mean_workspace_bytes(10, 0, 9) == 0
    assert lib.wm_lp_neighbor_mean_workspace_bytes(10, 7, 257) == 0

    # wm_lp_init(labels, n, classes, groups, F, ldf, ws, bytes, stream)
    assert lib.wm_lp_init(None, 100, 9, 1, P, 9, P, BIG, None) == EINVAL
    assert lib.wm_lp_init(P, 100, 9, 1, None, 9, P, BIG, None) == EINVAL
    assert lib.wm_lp_init(P, 100, 9, 1, P, 9, None, BIG, None) == EINVAL
    assert lib.wm_lp_init(P, 0, 9, 1, P, 9, P, BIG, None) == EINVAL
    assert lib.wm_lp_init(P, 100, 9, 2, P, 17, P, BIG, None) == EINVAL  # ldf < cols
    assert lib.wm_lp_init(P, 100, 9, 29, P, 261, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_init(P, (1 << 24) + 1, 9, 1, P, 9, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_init(P, 100, 9, 1, ODD, 9, P, BIG, None) == EALIGN
    assert lib.wm_lp_init(P + 2, 100, 9, 1, P, 9, P, BIG, None) == EALIGN
    assert lib.wm_lp_init(P, 100, 9, 1, P, 9, P, 255, None) == EWORKSPACE

    # wm_lp_iterate(indptr, indices, data, dinv, labels, n, classes, groups, alpha, active, hard, iters, Fa, Fb, ldf, resid,
    #               ws, bytes, stream)
    def iterate(**kw):
        a = dict(indptr=P, indices=P, data=P, dinv=P, labels=P, n=100, classes=9, groups=4, alpha=P, active=P, hard=0, iters=3,
                 Fa=P, Fb=P + 0x100000, ldf=36, resid=P, ws=P, bytes=BIG, stream=None)
        a.update(kw)
        return lib.wm_lp_iterate(*a.values())

    for name in ("indptr", "indices", "data", "dinv", "labels", "alpha", "active", "Fa", "Fb", "resid", "ws"):
        assert iterate(**{name: None}) == EINVAL, name
    assert iterate(n=0) == EINVAL and iterate(iters=0) == EINVAL and iterate(Fb=P) == EINVAL and iterate(ldf=35) == EINVAL
    assert iterate(groups=29, ldf=261) == EUNSUPPORTED and iterate(n=(1 << 24) + 1) == EUNSUPPORTED
    assert iterate(classes=257, groups=1, ldf=257) == EUNSUPPORTED
    for name in ("dinv", "alpha", "Fa", "Fb", "resid"):
        assert iterate(**{name: ODD + (0x100000 if name == "Fb" else 0)}) == EALIGN, name
    for name in ("indptr", "indices", "data", "labels", "active"):
        assert iterate(**{name: P + 2}) == EALIGN, name
    assert iterate(ws=P + 8) == EALIGN
    assert iterate(bytes=4 * 25 * 8 - 1) == EWORKSPACE and iterate(hard=1, bytes=0) == EWORKSPACE

    # wm_lp_finalize(F, ldf, n, classes, dist, rowsum, pred, unreached, ws, bytes, stream)
    Q = P + 0x100000
    assert lib.wm_lp_finalize(None, 9, 100, 9, Q, P, P, P, P, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 9, 100, 9, None, P, P, P, P, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, None, P, P, P, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, P, None, P, P, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, P, P, None, P, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, P, P, P, None, BIG, None) == EINVAL
    assert lib.wm_lp_finalize(P, 8, 100, 9, Q, P, P, P, P, BIG, None) == EINVAL  # ldf < classes
    assert lib.wm_lp_finalize(P, 9, 100, 9, P, P, P, P, P, BIG, None) == EINVAL  # in place
    assert lib.wm_lp_finalize(P, 257, 100, 257, Q, P, P, P, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_finalize(P, 9, (1 << 24) + 1, 9, Q, P, P, P, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_finalize(ODD, 9, 100, 9, Q, P, P, P, P, BIG, None) == EALIGN
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, P, P + 2, P, P, BIG, None) == EALIGN
    assert lib.wm_lp_finalize(P, 9, 100, 9, Q, P, P, P, P, 0, None) == EWORKSPACE

    # wm_lp_neighbor_mean(idx, m, k, dist, n, classes, out, ws, bytes, stream)
    assert lib.wm_lp_neighbor_mean(None, 10, 7, P, 100, 9, Q, P, BIG, None) == EINVAL
    assert lib.wm_lp_neighbor_mean(P, 10, 7, None, 100, 9, Q, P, BIG, None) == EINVAL
    assert lib.wm_lp_neighbor_mean(P, 10, 7, P, 100, 9, None, P, BIG, None) == EINVAL
    assert lib.wm_lp_neighbor_mean(P, 10, 7, P, 100, 9, Q, None, BIG, None) == EINVAL
    assert lib.wm_lp_neighbor_mean(P, 10, 0, P, 100, 9, Q, P, BIG, None) == EINVAL
    assert lib.wm_lp_neighbor_mean(P, 10, 65, P, 100, 9, Q, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_neighbor_mean(P, 10, 7, P, 100, 257, Q, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_neighbor_mean(P, 10, 7, P, (1 << 24) + 1, 9, Q, P, BIG, None) == EUNSUPPORTED
    assert lib.wm_lp_neighbor_mean(P + 2, 10, 7, P, 100, 9, Q, P, BIG, None) == EALIGN
    assert lib.wm_lp_neighbor_mean(P, 10, 7, ODD, 100, 9, Q, P, BIG, None) == EALIGN
    assert lib.wm_lp_neighbor_mean(P, 10, 7, P, 100, 9, Q, P, 100, None) == EWORKSPACE


def test_product_path_fails_loudly_without_gpu_tensors():
    import torch

    from ssl_wafermap_amd import _lib

    with pytest.raises(_lib.WaferHipError):
        S().label_matrix(torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(_lib.WaferHipError):
        S().LabelSpreading().fit(torch.zeros(8, 4), np.array([0, 1, -1, -1, -1, -1, -1, -1]))
