"""CPU checks of neighbors.py: the numpy restatements of the LOF kernels (ref_lrd, ref_lof, ref_in_degree) against
sklearn.neighbors.LocalOutlierFactor on float64 distances, the host logic of the estimator, and the argument checks of the
entry points, which return before any launch.

Both sides get the SAME float64 distance matrix (sklearn through metric="precomputed"), so the neighbour sets and the
distances are identical and only the order of the float64 operations differs.  With u = 2^-53 and every summand >= 0:
  lrd  a sum of k terms is within (k - 1) u relative of exact in any order; the division by k, the added 1e-10 and the
       reciprocal add one rounding each: (k + 2) u per side, 2 (k + 2) u between the two;
  LOF  sklearn takes the mean of the k ratios lrd_j / lrd_i, the restatement the ratio of the mean: either way k lrd values
       ((k + 2) u each), k - 1 additions, the division by k, and a division by lrd_i (u + (k + 2) u): (3 k + 5) u per side,
       2 (3 k + 5) u between the two.
"""
import warnings

import numpy as np
import pytest

U = 2.0 ** -53
KS = (1, 5, 20, 40)


def N():
    from ssl_wafermap_amd import neighbors

    return neighbors


def lrd_bound(k):
    return 2 * (k + 2) * U


def lof_bound(k):
    return 2 * (3 * k + 5) * U


def exact_distances(a, b):
    """float64 [len(a), len(b)] Euclidean distances by direct differences (no dot-product trick)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def host_lists(D, k, remove_self):
    """(dist float64 [m, k], idx int64 [m, k]) of a distance matrix, every row ordered by (distance, index); remove_self
    drops column i from row i first (by index, as manifold.neighbor_lists does)."""
    m, n = D.shape
    dist, idx = np.empty((m, k)), np.empty((m, k), dtype=np.int64)
    for i in range(m):
        order = np.lexsort((np.arange(n), D[i]))
        if remove_self:
            order = order[order != i]
        idx[i] = order[:k]
        dist[i] = D[i, idx[i]]
    return dist, idx


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


_CASE = {}


def normal_case():
    """The 300 x 16 input of the issue, its float64 distance matrix and its lists at 63 columns, computed once."""
    if not _CASE:
        x = np.random.default_rng(0).standard_normal((300, 16))
        x[:3] *= 6
        D = exact_distances(x, x)
        dist, idx = host_lists(D, 63, True)
        _CASE.update(x=x, D=D, dist=dist, idx=idx)
    return _CASE


def sk_fit(D, k, **kw):
    from sklearn.neighbors import LocalOutlierFactor

    return LocalOutlierFactor(n_neighbors=k, metric="precomputed", **kw).fit(D)


# ------------------------------------------------------------------------------------------------ restatements vs sklearn


@pytest.mark.parametrize("k", KS)
def test_restatements_match_sklearn(k):
    c = normal_case()
    dist, idx = c["dist"][:, :k], c["idx"][:, :k]
    lrd = N().ref_lrd(dist, idx, dist, [k])
    lof = N().ref_lof(idx, lrd, lrd, [k])
    sk = sk_fit(c["D"], k)
    assert np.array_equal(np.sort(sk._fit_X[np.arange(300)[:, None], idx], axis=1), np.sort(sk._distances_fit_X_, axis=1))
    assert rel(lrd[0], sk._lrd) <= lrd_bound(k)
    assert rel(-lof[0], sk.negative_outlier_factor_) <= lof_bound(k)
    assert lof[0, :3].min() > 1.5 and np.median(lof[0]) < 1.2  # the three scaled rows are the outliers


def test_a_list_of_ks_equals_the_single_ks_and_ignores_further_columns():
    c = normal_case()
    lrd = N().ref_lrd(c["dist"], c["idx"], c["dist"], KS)
    lof = N().ref_lof(c["idx"], lrd, lrd, KS)
    deg = N().ref_in_degree(c["idx"], KS)
    assert lrd.shape == lof.shape == deg.shape == (4, 300)
    for r, k in enumerate(KS):
        dist, idx = c["dist"][:, :k], c["idx"][:, :k]
        one = N().ref_lrd(dist, idx, dist, k)
        assert np.array_equal(one[0], lrd[r])
        assert np.array_equal(N().ref_lof(idx, one, one, k)[0], lof[r])
        assert np.array_equal(N().ref_in_degree(idx, k)[0], deg[r])


def test_duplicates_have_lrd_1e10_and_lof_1():
    x = np.random.default_rng(1).standard_normal((40, 4))
    x[10:16] = x[10]  # 6 identical rows, more than k = 3
    D = exact_distances(x, x)
    dist, idx = host_lists(D, 3, True)
    lrd = N().ref_lrd(dist, idx, dist, 3)
    lof = N().ref_lof(idx, lrd, lrd, 3)
    assert np.array_equal(lrd[0, 10:16], np.full(6, 1e10)) and np.array_equal(lof[0, 10:16], np.ones(6))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (sklearn remarks on the duplicates)
        sk = sk_fit(D, 3)
    assert rel(lrd[0], sk._lrd) <= lrd_bound(3)
    assert rel(-lof[0], sk.negative_outlier_factor_) <= lof_bound(3)


@pytest.mark.parametrize("k", [1, 20])
def test_novelty_path_matches_sklearn(k):
    c = normal_case()
    new = np.random.default_rng(2).standard_normal((7, 16))
    new[0] *= 6
    new[1] = c["x"][5]  # a fitted row given back: it finds itself at distance 0
    Dn = exact_distances(new, c["x"])
    dist_fit, idx_fit = c["dist"][:, :k], c["idx"][:, :k]
    lrd_fit = N().ref_lrd(dist_fit, idx_fit, dist_fit, k)
    dq, iq = host_lists(Dn, k, False)
    assert iq[1, 0] == 5 and dq[1, 0] == 0.0
    lrd_q = N().ref_lrd(dq, iq, dist_fit, k)
    lof_q = N().ref_lof(iq, lrd_q, lrd_fit, k)
    sk = sk_fit(c["D"], k, novelty=True)
    assert rel(-lof_q[0], sk.score_samples(Dn)) <= lof_bound(k)
    assert lof_q[0, 0] > 1.5
    fitted = N().ref_lof(idx_fit, lrd_fit, lrd_fit, k)
    assert k == 1 or lof_q[0, 1] != fitted[0, 5]  # self is not removed for a new row (at k = 1 both can be exactly 1)


def test_offset_and_labels_follow_sklearn():
    c = normal_case()
    auto, tenth = sk_fit(c["D"], 20), sk_fit(c["D"], 20, contamination=0.1)
    nof = auto.negative_outlier_factor_
    assert N().offset_for(nof, "auto") == auto.offset_ == -1.5
    assert N().offset_for(nof, 0.1) == tenth.offset_
    from sklearn.neighbors import LocalOutlierFactor

    for model, cont in ((auto, "auto"), (tenth, 0.1)):
        want = LocalOutlierFactor(n_neighbors=20, metric="precomputed", contamination=cont).fit_predict(c["D"])
        got = N().labels_from(nof, N().offset_for(nof, cont))
        assert np.array_equal(got, want) and got.dtype == want.dtype
    assert (N().labels_from(nof, tenth.offset_) == -1).sum() == 30


def test_in_degree_is_a_bincount():
    c = normal_case()
    for k in (1, 7, 63):
        want = np.bincount(c["idx"][:, :k].ravel(), minlength=300)
        got = N().ref_in_degree(c["idx"], k)
        assert got.dtype == np.int32 and np.array_equal(got[0], want) and got.sum() == 300 * k
    rect = np.array([[0, 4], [4, 1], [4, 0]])
    assert np.array_equal(N().ref_in_degree(rect, [1, 2], n=6), [[1, 0, 0, 0, 2, 0], [2, 1, 0, 0, 3, 0]])


def test_skewness_matches_scipy():
    from scipy import stats

    counts = N().ref_in_degree(normal_case()["idx"], 10)[0]
    assert abs(N().skewness(counts) - stats.skew(counts.astype(np.float64))) <= 1e-12
    assert N().skewness(counts) > 0.0 and N().skewness([3, 3, 3]) == 0.0
    with pytest.raises(ValueError):
        N().skewness([])


# ------------------------------------------------------------------------------------------------ host logic, refusals


def test_check_ks():
    ks, single = N().check_ks(20)
    assert single and ks.dtype == np.int32 and ks.tolist() == [20]
    ks, single = N().check_ks(range(10, 50, 10))
    assert not single and ks.tolist() == [10, 20, 30, 40]
    assert N().check_ks([63])[0].tolist() == [63]
    for bad in (0, 64, [], [5, 0], [5, 64], 2.5, [[1, 2]], -1):
        with pytest.raises(ValueError):
            N().check_ks(bad)
    with pytest.raises(ValueError):
        N().check_ks(7, limit=6)


def test_clipped_neighbors_warns_as_sklearn_and_names_the_limit():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert N().clipped_neighbors(20, 300) == 20
        assert N().clipped_neighbors(63, 64) == 63
    with pytest.warns(UserWarning, match="n_neighbors"):
        assert N().clipped_neighbors(20, 5) == 4
    with pytest.raises(ValueError, match="63"):
        N().clipped_neighbors(64, 1000)
    with pytest.warns(UserWarning), pytest.raises(ValueError, match="63"):
        N().clipped_neighbors(500, 100)
    for bad in ((0, 10), (3, 1)):
        with pytest.raises(ValueError):
            N().clipped_neighbors(*bad)


def test_contamination_range():
    assert N().check_contamination("auto") == "auto" and N().check_contamination(0.5) == 0.5
    for bad in (0.0, 0.51, -0.1, "all"):
        with pytest.raises(ValueError):
            N().check_contamination(bad)
        with pytest.raises(ValueError):
            N().LocalOutlierFactor(contamination=bad)


def test_driver_script_options():
    from scripts import embedding_outliers_amd as script

    assert script.parse_neighbors("20") == [20]
    assert script.parse_neighbors("10:40:10") == [10, 20, 30, 40]
    assert script.parse_neighbors("5:8") == [5, 6, 7, 8]
    for bad in ("0", "40:10", "a", "1:2:0", "1:2:3:4", ""):
        with pytest.raises(ValueError):
            script.parse_neighbors(bad)
    assert script.parse_contamination("auto") == "auto" and script.parse_contamination("0.05") == 0.05
    nof = np.array([[-1.0, -3.0, -1.2], [-2.0, -1.1, -1.2]])
    assert np.array_equal(script.combined(nof), [[-1.0, -3.0, -1.2], [-2.0, -1.1, -1.2], [-2.0, -3.0, -1.2]])


def test_estimator_refusals_need_no_gpu():
    import torch

    from ssl_wafermap_amd import _lib

    LOF = N().LocalOutlierFactor
    with pytest.raises(NotImplementedError):
        LOF(metric="canberra")
    with pytest.raises(ValueError):
        LOF(metric="cosine")
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError):
            LOF(n_neighbors=bad)
    x = torch.zeros(8, 4)
    with pytest.raises(AttributeError, match="novelty=True"):
        LOF(novelty=True).fit_predict(x)
    for name in ("score_samples", "decision_function", "predict"):
        with pytest.raises(AttributeError, match="novelty=False"):
            getattr(LOF(), name)(x)
        with pytest.raises(RuntimeError):
            getattr(LOF(novelty=True), name)(x)
    # a CPU tensor is an error, never a fallback
    with pytest.raises(_lib.WaferHipError):
        LOF(3).fit(x)
    with pytest.raises(_lib.WaferHipError):
        N().outlier_scores(x, 3)
    with pytest.raises(_lib.WaferHipError):
        N().in_degree(torch.zeros((8, 3), dtype=torch.int32), 3)
    with pytest.raises(_lib.WaferHipError):
        N().local_reachability_density(torch.zeros(8, 3), torch.zeros((8, 3), dtype=torch.int32), torch.zeros(8, 3), 3)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers and bad sizes come back as WM_EINVAL (-1) / WM_EUNSUPPORTED (-2); the pointers below are host
    addresses that no code path dereferences before the refusal (ks is read on the host by design)."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert N().MAX_GROUPS == 64 and N().MAX_K == 63
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    ks = np.array([1, 5], dtype=np.int32)
    for fn in (lib.wm_lof_lrd_workspace_bytes, lib.wm_lof_factor_workspace_bytes, lib.wm_lof_indegree_workspace_bytes):
        assert fn(300, 63, 64) == 256
        assert fn(300, 64, 1) == 0 and fn(300, 5, 65) == 0 and fn((1 << 24) + 1, 5, 1) == 0 and fn(0, 5, 1) == 0
    lrd = lambda **kw: lib.wm_lof_lrd(*[kw.get(k, v) for k, v in dict(dq=p, iq=p, rows=8, ld=5, df=p, n=8, ldf=5, ks=ks.ctypes.data, g=2,
                                                                      out=p, ws=p, wsb=256, st=None).items()])  # noqa: E731
    fac = lambda **kw: lib.wm_lof_factor(*[kw.get(k, v) for k, v in dict(iq=p, rows=8, ld=5, lq=p, lf=p + 64, n=8, ks=ks.ctypes.data, g=2,
                                                                         out=p + 128, ws=p, wsb=256, st=None).items()])  # noqa: E731
    deg = lambda **kw: lib.wm_lof_indegree(*[kw.get(k, v) for k, v in dict(iq=p, rows=8, ld=5, n=8, ks=ks.ctypes.data, g=2, out=p, ws=p,
                                                                           wsb=256, st=None).items()])  # noqa: E731
    for call, pointers in ((lrd, ("dq", "iq", "df", "ks", "out", "ws")), (fac, ("iq", "lq", "lf", "ks", "out", "ws")),
                           (deg, ("iq", "ks", "out", "ws"))):
        for name in pointers:
            assert call(**{name: None}) == -1, name
        assert call(rows=0) == -1 and call(g=0) == -1 and call(ld=0) == -1
        assert call(ld=4) == -1  # ks holds a 5
        assert call(ks=np.array([0, 5], dtype=np.int32).ctypes.data) == -1
        assert call(ld=64) == -2 and call(g=65) == -2 and call(rows=(1 << 24) + 1) == -2
        assert call(wsb=8) == -3
        assert call(out=p + 1) == -4
    assert lrd(ldf=4) == -1 and lrd(ldf=64) == -2 and lrd(n=0) == -1
    assert fac(out=p) == -1  # lof must be a third buffer
