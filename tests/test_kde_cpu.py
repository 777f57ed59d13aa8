"""CPU checks of density.py: the numpy float64 restatement of the Gaussian log-sum kernel against
sklearn.neighbors.KernelDensity, the leave-one-out values against n refits, the rules of thumb, uniformity and alignment
against their formulas, the classifier against a hand-written Bayes rule, the list conventions, and the argument checks of
the C entry point, which need no GPU.

Tolerance against sklearn: 1e-10 absolute.  Both sides are float64 log-sum-exps of at most 300 terms on the same float64
rows; sklearn builds its distances in its tree, the restatement by differences, and the two agree to rounding (5.5e-12 was
measured on 2 000 standardised golden rows, h in [0.5, 20]).  sklearn is asked for one leaf (`sk_kde` says why).

The helpers at the end (`log_sum_reference`, `float64_slack`) are what tests/test_gpu_kde.py judges the kernel by; the
derivation stands in that file's docstring.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -53


def D():
    from ssl_wafermap_amd import density

    return density


# ------------------------------------------------------------------------------------------------ helpers (shared with the GPU tests)


def exact_sq(xq, x):
    """float64 [m, n]: the exact squared distances of float32 rows, widened first."""
    return D().squared_distances(np.asarray(xq, dtype=np.float32), np.asarray(x, dtype=np.float32))


def float64_slack(sq_min, logsum, a, n: int, weighted_arg):
    """The float64 rounding of kernel and restatement together, absolute in the log-sum (derivation: test_gpu_kde.py).
    sq_min [m], logsum and weighted_arg [m] for one factor a; n the number of columns."""
    rescales = math.ceil(n / 64) + 2
    rel_sum = (2 * (n - 1) + 16 + 9 * rescales) * U
    return rel_sum + 4 * U * weighted_arg + 16 * U * math.log(max(n, 2)) + 2 * U * np.abs(a * sq_min) + 2 * U * np.abs(logsum)


def log_sum_reference(sq, a, d: int, exclude=None, exact: bool = False):
    """(reference [B, m], bound [B, m]) for factors a [B] on exact squared distances sq [m, n] of rows with d features:
    the restatement, and per row and factor the distance part log sum_j w_ij exp(eps a s_ij), eps = (d + 2) 2^-24, plus
    `float64_slack`.  exact: the rows are such that the float32 chain is exact (small integers), eps = 0.  Rows without
    an included column: reference -inf, bound 0 (the kernel must give -inf)."""
    dens = D()
    a = np.asarray(a, dtype=np.float64)
    sq = np.asarray(sq, dtype=np.float64)
    ref = dens.ref_gaussian_log_sums(sq, exclude=exclude, inv_two_h2=a)
    mask = dens.exclusion_mask(sq.shape[0], sq.shape[1], exclude)
    s = sq if mask is None else np.where(mask, np.inf, sq)
    eps = 0.0 if exact else (d + 2) * 2.0 ** -24
    bound = np.zeros_like(ref)
    smin = s.min(axis=1)
    have = np.isfinite(smin)
    gap = np.where(np.isfinite(s[have]), s[have] - smin[have, None], np.inf)
    fin = np.isfinite(gap)
    for q, aq in enumerate(a):
        t = np.exp(-aq * gap)
        w = t / t.sum(axis=1, keepdims=True)
        arg = np.where(fin, aq * np.where(fin, s[have], 0.0), 0.0)
        dist_part = np.log((w * np.exp(eps * arg)).sum(axis=1))
        weighted_arg = (w * np.where(fin, aq * np.where(fin, gap, 0.0), 0.0)).sum(axis=1)
        bound[q, have] = dist_part + float64_slack(smin[have], ref[q, have], aq, sq.shape[1], weighted_arg)
    return ref, bound


def propagate(logv, bound, axis=-1):
    """The bound of logsumexp(logv) along an axis when every entry moves by at most its `bound`: log sum softmax(logv)
    exp(bound) (convexity, as for the rows themselves)."""
    logv = np.asarray(logv, dtype=np.float64)
    top = np.max(logv, axis=axis, keepdims=True)
    w = np.exp(logv - np.where(np.isfinite(top), top, 0.0))
    return np.log((w * np.exp(bound)).sum(axis=axis) / w.sum(axis=axis))


def uniformity_formula(rows, t):
    """log mean_{i < j} exp(-t ||z_i - z_j||^2) on scipy's pdist, float64."""
    from scipy.spatial.distance import pdist

    sq = pdist(np.asarray(rows, dtype=np.float64), "sqeuclidean")
    return float(np.log(np.mean(np.exp(-t * sq))))


def bayes_log_posterior(x, y, h, priors=None, leave_out=False):
    """Hand-written rule: log p(c | x_i) [n_labelled, C] for the labelled rows of x themselves (leave_out) or as queries."""
    keep = y != -1
    xs, ys = x[keep], y[keep]
    classes = np.unique(ys)
    sq = exact_sq(xs, xs)
    out = np.full((xs.shape[0], classes.size), -np.inf)
    pri = np.array([(ys == c).mean() for c in classes]) if priors is None else np.asarray(priors, dtype=np.float64) / np.sum(priors)
    for i in range(xs.shape[0]):
        for k, c in enumerate(classes):
            members = np.flatnonzero(ys == c)
            if leave_out:
                members = members[members != i]
            if members.size:
                dens = np.mean(np.exp(-sq[i, members] / (2.0 * h * h)))
                out[i, k] = np.log(pri[k]) + np.log(dens)
    return out - np.log(np.exp(out).sum(axis=1, keepdims=True)), classes


@pytest.fixture
def on_host(monkeypatch):
    """density.py with its device steps replaced by numpy on CPU tensors: the restatement for the kernel, a float32
    normalisation, row-wise distances for pair_distances."""
    dens = D()

    def fake_log_sums(xq, x, bandwidths=None, self_offset=None, out=None, ws=None, *, inv_two_h2=None):
        sq = exact_sq(xq.numpy(), x.numpy())
        return torch.from_numpy(dens.ref_gaussian_log_sums(sq, bandwidths, exclude=self_offset, inv_two_h2=inv_two_h2))

    def fake_normalize(z):
        z = z.numpy().astype(np.float64)
        return torch.from_numpy((z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32))

    def fake_pairs(a, b, idx):
        diff = a.numpy().astype(np.float64) - b.numpy().astype(np.float64)[idx.numpy()[:, 0]]
        return torch.from_numpy(np.sqrt((diff * diff).sum(axis=1)).astype(np.float32)[:, None])

    monkeypatch.setattr(dens, "gaussian_log_sums", fake_log_sums)
    monkeypatch.setattr(dens, "require_gpu", lambda *t: None)
    monkeypatch.setattr(dens, "_prep", lambda x: x.float().contiguous())
    monkeypatch.setattr(dens, "normalize_rows", fake_normalize)
    monkeypatch.setattr(dens, "pair_distances", fake_pairs)
    return dens


def sk_kde(bandwidth, x):
    """sklearn's estimator, exact (rtol = atol = 0), fitted on the float64 copy of x.  leaf_size above n makes the tree ONE
    leaf, whose kernel sum sklearn evaluates directly: with inner nodes it carries lower and upper bounds in log space and
    subtracts them, which loses digits for rows of low density (1.6e-5 absolute on the d = 6, h = 0.3 case below, against
    1.4e-14 for the single leaf, both judged by a long-double sum)."""
    from sklearn.neighbors import KernelDensity

    x = np.asarray(x, dtype=np.float64)
    return KernelDensity(bandwidth=bandwidth, rtol=0, atol=0, leaf_size=x.shape[0] + 1).fit(x)


def rows(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ against sklearn


@pytest.mark.parametrize("d", [1, 6, 50])
def test_restatement_matches_sklearn(d):
    dens = D()
    x, xq = rows(300, d, 1), rows(40, d, 2)
    hs = [0.3, 1.0, 4.0]
    for query in (x, xq):
        got = dens.ref_gaussian_log_sums(exact_sq(query, x), hs) - math.log(300) - dens.log_normaliser(hs, d)[:, None]
        for q, h in enumerate(hs):
            want = sk_kde(h, x).score_samples(query.astype(np.float64))
            assert np.abs(got[q] - want).max() <= 1e-10


def test_leave_one_out_equals_refits(on_host):
    x = rows(40, 6, 3)
    hs = [0.5, 1.5]
    model = on_host.KernelDensity(hs).fit(torch.from_numpy(x))
    got = model.loo_score_samples()
    assert got.shape == (2, 40)
    x64 = x.astype(np.float64)
    for q, h in enumerate(hs):
        for i in range(40):
            want = sk_kde(h, np.delete(x64, i, axis=0)).score_samples(x64[i:i + 1])[0]
            assert abs(got[q, i] - want) <= 1e-10
    assert np.allclose(model.loo_log_likelihood(), got.sum(axis=1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("rule", ["scott", "silverman"])
def test_rules_of_thumb_are_sklearns(rule, on_host):
    from sklearn.neighbors import KernelDensity

    x = rows(57, 5, 4)
    want = KernelDensity(bandwidth=rule).fit(x.astype(np.float64)).bandwidth_
    got = on_host.KernelDensity(rule).fit(torch.from_numpy(x))
    assert got.bandwidth_ == pytest.approx(want, rel=1e-15)
    ref = sk_kde(rule, x).score_samples(x.astype(np.float64))
    assert np.abs(got.score_samples(torch.from_numpy(x)) - ref).max() <= 1e-10
    assert got.score(torch.from_numpy(x)) == pytest.approx(ref.sum(), abs=1e-9)


def test_estimator_refuses_what_is_not_built():
    dens = D()
    with pytest.raises(NotImplementedError):
        dens.KernelDensity(kernel="tophat")
    with pytest.raises(NotImplementedError):
        dens.KernelDensity(metric="manhattan")
    for bad in (0.0, -1.0, float("nan"), float("inf"), [], [1.0, 0.0], "scot", 1e-200, 1e200):
        with pytest.raises(ValueError):
            dens.KernelDensity(bad)
    from ssl_wafermap_amd import neighbors

    assert neighbors.KernelDensity is dens.KernelDensity


# ------------------------------------------------------------------------------------------------ uniformity, alignment


def test_uniformity_matches_the_pdist_formula(on_host):
    z = rows(120, 8, 5)
    zn = on_host.normalize_rows(torch.from_numpy(z)).numpy()
    got = on_host.uniformity(torch.from_numpy(z), t=[0.5, 2.0, 7.0])
    assert got.shape == (3,)
    for q, t in enumerate([0.5, 2.0, 7.0]):
        assert got[q] == pytest.approx(uniformity_formula(zn, t), abs=1e-12)
    assert on_host.uniformity(torch.from_numpy(z)) == pytest.approx(got[1], abs=0)
    assert on_host.uniformity(torch.from_numpy(z), normalize=False) == pytest.approx(uniformity_formula(z, 2.0), abs=1e-12)
    same = np.tile(rows(1, 8, 6), (9, 1))
    assert on_host.uniformity(torch.from_numpy(same)) == pytest.approx(0.0, abs=1e-12)  # collapsed rows


def test_alignment_matches_numpy(on_host):
    z1, z2 = rows(90, 7, 7), rows(90, 7, 8)
    for alpha in (1.0, 2.0, 3.5):
        want = np.mean(np.linalg.norm(z1.astype(np.float64) - z2.astype(np.float64), axis=1) ** alpha)
        assert on_host.alignment(torch.from_numpy(z1), torch.from_numpy(z2), alpha, normalize=False) == pytest.approx(want, rel=1e-6)
    n1 = on_host.normalize_rows(torch.from_numpy(z1)).numpy().astype(np.float64)
    n2 = on_host.normalize_rows(torch.from_numpy(z2)).numpy().astype(np.float64)
    want = np.mean(np.linalg.norm(n1 - n2, axis=1) ** 2)
    assert on_host.alignment(torch.from_numpy(z1), torch.from_numpy(z2)) == pytest.approx(want, rel=1e-6)
    with pytest.raises(ValueError):
        on_host.alignment(torch.from_numpy(z1), torch.from_numpy(z2[:5]))


# ------------------------------------------------------------------------------------------------ the classifier


def labelled_case():
    """60 rows of three shifted blobs, labels 3 / 7 / 9 with one class of a single row and a few unlabelled rows."""
    rng = np.random.default_rng(9)
    y = rng.choice([3, 7], size=60)
    y[17] = 9  # a class of one row
    y[[4, 30, 31]] = -1
    x = rng.standard_normal((60, 5)).astype(np.float32)
    x[y == 7] += 1.5
    x[y == 9] -= 2.0
    return x, y.astype(np.int64)


@pytest.mark.parametrize("priors", [None, [0.2, 0.5, 0.3]])
def test_classifier_is_bayes_rule(on_host, priors):
    x, y = labelled_case()
    hs = [0.7, 2.0]
    clf = on_host.KDEClassifier(hs, priors=priors).fit(torch.from_numpy(x), y)
    assert list(clf.classes_) == [3, 7, 9] and list(clf.class_count_) == [int((y == c).sum()) for c in (3, 7, 9)]
    assert np.array_equal(clf.fit_rows_, np.flatnonzero(y != -1))
    labelled = torch.from_numpy(x[y != -1])
    logp, loo = clf.predict_log_proba(labelled), clf.loo_predict_log_proba()
    assert logp.shape == loo.shape == (2, 57, 3)
    for q, h in enumerate(hs):
        want, classes = bayes_log_posterior(x, y, h, priors)
        assert np.abs(logp[q] - want).max() <= 1e-10
        want_loo, _ = bayes_log_posterior(x, y, h, priors, leave_out=True)
        fin = np.isfinite(want_loo)
        assert np.array_equal(np.isfinite(loo[q]), fin) and np.abs(loo[q][fin] - want_loo[fin]).max() <= 1e-10
        assert np.array_equal(clf.loo_predict()[q], classes[np.argmax(want_loo, axis=1)])
    proba = clf.loo_predict_proba()
    assert not np.isnan(proba).any() and np.abs(proba.sum(axis=2) - 1.0).max() <= 1e-12
    own = np.flatnonzero(y[y != -1] == 9)[0]
    assert np.all(proba[:, own, 2] == 0.0)  # the single row of class 9 has no density left for itself
    one = on_host.KDEClassifier(0.7, priors=priors).fit(torch.from_numpy(x), torch.from_numpy(y))
    assert np.array_equal(one.predict_log_proba(labelled), logp[0]) and one.predict(labelled).shape == (57,)
    assert np.array_equal(one.predict(labelled), clf.predict(labelled)[0])


def test_classifier_argument_checks(on_host):
    x, y = labelled_case()
    with pytest.raises(ValueError):
        on_host.KDEClassifier(1.0).fit(torch.from_numpy(x), np.full(60, -1))
    with pytest.raises(ValueError):
        on_host.KDEClassifier(1.0, priors=[0.5, 0.5]).fit(torch.from_numpy(x), y)
    with pytest.raises(ValueError):
        on_host.KDEClassifier("scott")
    with pytest.raises(RuntimeError):
        on_host.KDEClassifier(1.0).loo_predict_proba()


# ------------------------------------------------------------------------------------------------ a list of bandwidths


def test_list_semantics(on_host):
    x = torch.from_numpy(rows(80, 4, 11))
    hs = [0.05, 0.4, 1.0, 3.0, 9.0]
    many = on_host.KernelDensity(hs).fit(x)
    assert len(many) == 5 and np.array_equal(many.bandwidth_, hs)
    s, loo, ll = many.score_samples(x), many.loo_score_samples(), many.loo_log_likelihood()
    assert s.shape == loo.shape == (5, 80) and ll.shape == (5,) and many.score(x).shape == (5,)
    for i, h in enumerate(hs):
        one = many[i]
        alone = on_host.KernelDensity(h).fit(x)
        assert one.bandwidth_ == alone.bandwidth_ == h
        assert np.array_equal(one.score_samples(x), s[i]) and np.array_equal(alone.score_samples(x), s[i])
        assert np.array_equal(one.loo_score_samples(), loo[i:i + 1]) and np.array_equal(alone.loo_log_likelihood(), ll[i:i + 1])
        assert isinstance(alone.score(x), float)
    best = many.best()
    assert best.bandwidth_ == hs[int(np.argmax(ll))] and 0 < int(np.argmax(ll)) < 4  # an interior maximum
    assert many.best([0, 0, 5, 5, 1]).bandwidth_ == 1.0  # the first maximum wins
    with pytest.raises(TypeError):
        many[0][0]
    with pytest.raises(ValueError):
        many.best([1.0, 2.0])
    with pytest.raises(RuntimeError):
        on_host.KernelDensity(hs).score_samples(x)
    with pytest.raises(ValueError):
        on_host.KernelDensity(1.0).fit(x[:1]).loo_score_samples()


def test_restatement_edges():
    dens = D()
    sq = np.array([[0.0, 4.0, 4.0], [4.0, 0.0, 1.0]])
    # nothing excluded, an offset, a mask; a row with every column excluded gives -inf, not NaN
    assert np.allclose(dens.ref_gaussian_log_sums(sq, inv_two_h2=[0.5])[0], np.log([1 + 2 * np.exp(-2.0), np.exp(-2.0) + 1 + np.exp(-0.5)]))
    assert np.allclose(dens.ref_gaussian_log_sums(sq, inv_two_h2=[0.5], exclude=0)[0], [np.log(2.0) - 2.0, np.log(np.exp(-2.0) + np.exp(-0.5))])
    out = dens.ref_gaussian_log_sums(sq, 1.0, exclude=np.array([[True, True, True], [False, True, True]]))
    assert out[0, 0] == -np.inf and out[0, 1] == pytest.approx(-2.0)
    assert np.array_equal(dens.ref_gaussian_log_sums(sq[:, :1], 1.0, exclude=0)[0], [-np.inf, -2.0])
    # a tiny bandwidth keeps the nearest columns: -a s_min + log(multiplicity), exactly
    tiny = dens.ref_gaussian_log_sums(sq, inv_two_h2=[1e9], exclude=0)[0]
    assert tiny[0] == -4e9 + np.log(2.0) and tiny[1] == -1e9
    assert dens.host_logsumexp(np.array([-np.inf, -np.inf])) == -np.inf


# ------------------------------------------------------------------------------------------------ the C entry point, no GPU


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_size_function(lib):
    cap = D().MAX_BANDWIDTHS
    assert lib.wm_kde_logsum_workspace_bytes(100, 200, 8, 1) > 0
    assert lib.wm_kde_logsum_workspace_bytes(100, 200, 8, cap) > lib.wm_kde_logsum_workspace_bytes(100, 200, 8, 1)
    # three column tiles of 129 columns are three slices of [m] minima and [b][m] sums
    assert lib.wm_kde_logsum_workspace_bytes(129, 129, 8, 3) == 3 * 129 * 4 * 8 + 256
    for bad in ((0, 200, 8, 1), (100, 0, 8, 1), (100, 200, 0, 1), (100, 200, 6, 1), (100, 200, 1028, 1), (100, 200, 8, 0),
                (100, 200, 8, cap + 1), ((1 << 24) + 1, 200, 8, 1), (100, (1 << 24) + 1, 8, 1), (-1, 200, 8, 1)):
        assert lib.wm_kde_logsum_workspace_bytes(*bad) == 0, bad


def test_entry_point_refuses_before_any_launch(lib):
    """Host buffers stand in for the device pointers: every call below must be refused before a kernel is launched."""
    cap = D().MAX_BANDWIDTHS
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = (ctypes.c_double * 8)(*([0.5] * 8))
    ga = ctypes.addressof(good)

    def call(xr=p, x=p, a=ga, b=1, so=0, out=p, ws=p, m=4, n=4, d=4):
        return lib.wm_kde_logsum(xr, m, x, n, d, a, b, so, out, ws, 1 << 20, None)

    einval = -1
    for null in ("xr", "x", "a", "out", "ws"):
        assert call(**{null: None}) == einval, null
    assert call(b=0) == einval and call(b=cap + 1) == einval and call(b=-3) == einval
    assert call(m=0) == einval and call(n=0) == einval and call(d=0) == einval and call(so=-2) == einval
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for b in range(1, cap + 1):
            vals = [0.5] * 8
            vals[b - 1] = bad  # the last of b bandwidths
            arr = (ctypes.c_double * 8)(*vals)
            assert call(a=ctypes.addressof(arr), b=b) == einval, (bad, b)
    assert call(d=6) == -2  # unsupported: d is no multiple of 4


# ------------------------------------------------------------------------------------------------ the script's host logic


def test_script_host_logic():
    from scripts.embedding_density_amd import macro_f1, parse_bandwidths

    assert parse_bandwidths("scott") == "scott" and parse_bandwidths("silverman") == "silverman"
    assert parse_bandwidths("1.5") == [1.5] and parse_bandwidths("2:2:1") == [2.0]
    assert np.allclose(parse_bandwidths("0.5:8:5"), [0.5, 1.0, 2.0, 4.0, 8.0], rtol=1e-15, atol=0)
    for bad in ("", "0", "-1", "2:1:3", "1:2", "1:2:0", "1:2:1", "a:b:c", "scot"):
        with pytest.raises(ValueError):
            parse_bandwidths(bad)
    from sklearn.metrics import f1_score

    rng = np.random.default_rng(12)
    truth, pred = rng.integers(0, 4, 200), rng.integers(0, 5, 200)
    assert macro_f1(truth, pred) == pytest.approx(f1_score(truth, pred, labels=np.unique(truth), average="macro"), abs=1e-15)
