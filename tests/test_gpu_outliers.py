"""GPU checks of the local-outlier-factor kernels (csrc/lof.hip) and of neighbors.py built on them, against the numpy
float64 restatements (neighbors.ref_lrd, ref_lof, ref_in_degree; tests/test_outliers_cpu.py checks those against sklearn)
and, end to end, against sklearn.

Bounds are derived, not tuned.  u = 2^-53.  Kernel and restatement are float64 computations on IDENTICAL float32
distances, widened exactly, and every summand is non-negative.
  (a) lrd.  A sum of k non-negative terms, in any order (the kernel's balanced tree, numpy's), is within (k - 1) u
      relative of the exact sum.  The division by k, the added 1e-10 and the reciprocal add one rounding each (the sum of
      two non-negative numbers keeps a relative error relative): (k + 2) u per side, 2 (k + 2) u between the two.
  (b) LOF, each side from its own lrd.  The k summands carry lrd's error, (k + 2) u each; their sum adds (k - 1) u, the
      division by k one u, and the final division u plus the divisor's (k + 2) u: (3 k + 5) u per side, 2 (3 k + 5) u
      between the two.
  (c) The in-degree is an integer: equality.
  (d) Bits.  The order of a sum depends on k alone: two calls, a k alone and the same k inside a list, a list cut into
      launches of 64 groups, and lists with further columns behind max(ks) give equal bits.
  (e) The fit against sklearn on the same float32 values (given to sklearn as float64).  The project's distance is within
      eps = (d + 3) 2^-24 relative of the exact one (manifold.knn_graph).  Where a row and every row of its list have the
      same neighbour sets in both computations, each reach term moves by at most eps relative, so does each lrd, and the
      ratio by 2 eps / (1 - eps).  The sets are the same where the relative gap between the k-th and the (k + 1)-th
      reference distance exceeds 2 eps; rows that fail this, or list a row that fails it, are left out, and their share is
      capped at 0 for this input (asserted on the reference alone: the smallest gap is 5.5e-5 against 2 eps = 2.3e-6).
      Labels are compared on the rows whose reference score is further from offset_ than that bound.
"""
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch
from parity_log import parity

from test_outliers_cpu import exact_distances, host_lists, lof_bound, lrd_bound, normal_case
from test_spectral_cpu import golden_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53


def N():
    from ssl_wafermap_amd import neighbors

    return neighbors


def M():
    from ssl_wafermap_amd import manifold

    return manifold


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def worst(got, want, bound):
    """max |got - want| / (bound |want|) per group of a [R, rows] pair; bound: one relative figure per group."""
    frac = np.abs(got - want) / (np.asarray(bound, dtype=np.float64)[:, None] * np.abs(want))
    return float(frac.max())


_LISTS = {}


def lists(n, d=6):
    """(dist float32, idx int32) [n, min(n - 1, 63)]: the exact lists of seeded rows without the row itself, the distances
    rounded to float32 once -- what both sides are fed."""
    if n not in _LISTS:
        x = normal_case()["x"] if n == 300 else np.random.default_rng(n).standard_normal((n, d))
        dist, idx = host_lists(exact_distances(x, x), min(n - 1, 63), True)
        _LISTS[n] = (x, dist.astype(np.float32), idx.astype(np.int32))
    return _LISTS[n]


def device_passes(dist_q, idx_q, dist_fit, ks, lrd_fit=None):
    """(lrd, lof) [R, rows] on the host through the two kernels; lrd_fit None: the query lists are the fitted lists."""
    lrd = N().local_reachability_density(dev(dist_q), dev(idx_q), dev(dist_fit), ks)
    lof = N().local_outlier_factor(dev(idx_q), lrd, lrd if lrd_fit is None else dev(lrd_fit), ks)
    return host(lrd), host(lof)


def check_against_restatement(name, dist, idx, ks):
    """The three passes of square lists against numpy; returns the device results."""
    lrd, lof = device_passes(dist, idx, dist, ks)
    want_lrd = N().ref_lrd(dist, idx, dist, ks)
    want_lof = N().ref_lof(idx, want_lrd, want_lrd, ks)
    assert lrd.shape == lof.shape == (len(ks), idx.shape[0]) and lrd.dtype == lof.dtype == np.float64
    parity(f"lof lrd {name} / bound", worst(lrd, want_lrd, [lrd_bound(k) for k in ks]), 1.0)
    parity(f"lof factor {name} / bound", worst(lof, want_lof, [lof_bound(k) for k in ks]), 1.0)
    deg = host(N().in_degree(dev(idx), ks))
    assert deg.dtype == np.int32 and np.array_equal(deg, N().ref_in_degree(idx, ks))
    return lrd, lof, deg


# ------------------------------------------------------------------------------------------------ (a) - (c) the kernels


@pytest.mark.parametrize("n, ks", [(2, [1]), (4, [3, 1]), (5, [1, 2, 4]), (64, [1, 2, 63]), (65, [1, 2, 63]),
                                   (300, [1, 5, 20, 40, 63])])
def test_passes_match_the_restatement(n, ks):
    """n = 5: one row past a workgroup of four waves (one row each); 64, 65: lists of 63 columns, every lane but the last
    busy, and 65 * 63 cells, past a multiple of the 256 threads of the in-degree pass; 300: the counts of the issue."""
    _, dist, idx = lists(n)
    assert dist.shape[1] == min(n - 1, 63)
    _, lof, deg = check_against_restatement(f"n={n}", dist, idx, ks)
    assert np.array_equal(deg.sum(axis=1), n * np.asarray(ks))
    if n == 300:
        assert lof[2, :3].min() > 1.5  # the three scaled rows, k = 20


def test_columns_behind_the_largest_k_are_never_read_into_a_sum():
    """ld = 63 with ks up to 20: the 43 further columns hold +inf distances (any use would make a sum infinite) and the
    in-range index 0 (any use would change row 0's in-degree and the lrd sums).  Equal bits to the lists cut at 20."""
    _, dist, idx = lists(300)
    ks = [1, 5, 20]
    cut_d, cut_i = np.ascontiguousarray(dist[:, :20]), np.ascontiguousarray(idx[:, :20])
    pad_d, pad_i = dist.copy(), idx.copy()
    pad_d[:, 20:], pad_i[:, 20:] = np.inf, 0
    lrd, lof = device_passes(pad_d, pad_i, pad_d, ks)
    lrd_cut, lof_cut = device_passes(cut_d, cut_i, cut_d, ks)
    assert np.isfinite(lrd).all() and np.isfinite(lof).all()
    assert np.array_equal(bits(lrd), bits(lrd_cut)) and np.array_equal(bits(lof), bits(lof_cut))
    assert np.array_equal(host(N().in_degree(dev(pad_i), ks)), N().ref_in_degree(cut_i, ks))
    # the fitted side narrower than the query side: ld_fit = 20 under ld = 63
    lrd_mixed = host(N().local_reachability_density(dev(pad_d), dev(pad_i), dev(cut_d), ks))
    assert np.array_equal(bits(lrd_mixed), bits(lrd_cut))


@pytest.mark.parametrize("m", [1, 7])
def test_rectangular_passes_match_the_restatement(m):
    x, dist_fit, idx_fit = lists(300)
    ks = [1, 5, 20, 40, 63]
    new = np.random.default_rng(100 + m).standard_normal((m, 16))
    new[0] *= 6
    dq, iq = host_lists(exact_distances(new, x), 63, False)
    dq, iq = dq.astype(np.float32), iq.astype(np.int32)
    lrd_fit = N().ref_lrd(dist_fit, idx_fit, dist_fit, ks)
    lrd_fit_dev, _ = device_passes(dist_fit, idx_fit, dist_fit, ks)
    lrd, lof = device_passes(dq, iq, dist_fit, ks, lrd_fit=lrd_fit_dev)
    want_lrd = N().ref_lrd(dq, iq, dist_fit, ks)
    want_lof = N().ref_lof(iq, want_lrd, lrd_fit, ks)
    assert lrd.shape == lof.shape == (5, m)
    parity(f"lof lrd rectangular m={m} / bound", worst(lrd, want_lrd, [lrd_bound(k) for k in ks]), 1.0)
    parity(f"lof factor rectangular m={m} / bound", worst(lof, want_lof, [lof_bound(k) for k in ks]), 1.0)
    deg = host(N().in_degree(dev(iq), ks, n=300))
    assert np.array_equal(deg, N().ref_in_degree(iq, ks, n=300)) and deg.shape == (5, 300)


def test_duplicates_give_lrd_1e10_and_lof_1():
    x = np.random.default_rng(1).standard_normal((40, 4))
    x[10:16] = x[10]
    dist, idx = host_lists(exact_distances(x, x), 3, True)
    dist, idx = dist.astype(np.float32), idx.astype(np.int32)
    lrd, lof, _ = check_against_restatement("duplicates", dist, idx, [3])
    assert np.array_equal(lrd[0, 10:16], np.full(6, 1e10)) and np.array_equal(lof[0, 10:16], np.ones(6))
    # end to end: the graph's own lists keep the duplicates and drop the row by index
    scores = N().outlier_scores(dev(x.astype(np.float32)), 3)
    assert np.array_equal(host(scores.lrd)[0, 10:16], np.full(6, 1e10)) and np.array_equal(host(scores.lof)[0, 10:16], np.ones(6))
    assert (host(scores.kdist)[0, 10:16] == 0.0).all()


# ------------------------------------------------------------------------------------------------ (d) bits


def test_two_calls_and_every_k_alone_give_the_same_bits():
    _, dist, idx = lists(300)
    ks = [1, 5, 20, 40, 63]
    lrd, lof = device_passes(dist, idx, dist, ks)
    deg = host(N().in_degree(dev(idx), ks))
    again = device_passes(dist, idx, dist, ks)
    assert np.array_equal(bits(lrd), bits(again[0])) and np.array_equal(bits(lof), bits(again[1]))
    assert np.array_equal(deg, host(N().in_degree(dev(idx), ks)))
    for r, k in enumerate(ks):
        one_lrd, one_lof = device_passes(dist, idx, dist, k)
        assert np.array_equal(bits(one_lrd[0]), bits(lrd[r])) and np.array_equal(bits(one_lof[0]), bits(lof[r]))
        assert np.array_equal(host(N().in_degree(dev(idx), k))[0], deg[r])


def test_a_list_longer_than_one_launch_goes_in_chunks():
    """70 neighbour counts: a launch of 64 groups and one of 6, written into one output."""
    _, dist, idx = lists(65)
    ks = list(range(1, 64)) + [5, 63, 1, 20, 7, 2, 40]
    assert len(ks) > N().MAX_GROUPS
    lrd, lof, deg = check_against_restatement("70 groups", dist, idx, ks)
    for r in (64, 65, 69):
        first = ks.index(ks[r])
        assert np.array_equal(bits(lrd[r]), bits(lrd[first])) and np.array_equal(bits(lof[r]), bits(lof[first]))
        assert np.array_equal(deg[r], deg[first])


def test_wrappers_refuse_bad_lists():
    _, dist, idx = lists(65)
    d, i = dev(dist), dev(idx)
    with pytest.raises(ValueError):
        N().local_reachability_density(d, i, d, 64)
    with pytest.raises(ValueError):
        N().local_reachability_density(d, i, d[:, :10].contiguous(), 11)  # k beyond the fitted side's columns
    with pytest.raises(ValueError):
        N().local_reachability_density(d.double(), i, d, 3)
    with pytest.raises(ValueError):
        N().local_reachability_density(d, i, d[:40].contiguous(), 3)  # an index beyond the fitted rows
    with pytest.raises(ValueError):
        N().in_degree(i, 3, n=10)
    with pytest.raises(ValueError):
        N().in_degree(i.long(), 3)
    lrd = N().local_reachability_density(d, i, d, [3, 5])
    with pytest.raises(ValueError):
        N().local_outlier_factor(i, lrd, lrd, [3])
    with pytest.raises(ValueError):
        N().local_outlier_factor(i, lrd, lrd, [3, 5], out=lrd)
    with pytest.raises(ValueError):
        N().outlier_scores(dev(np.zeros((10, 4), dtype=np.float32)), 10)  # k <= n - 1


# ------------------------------------------------------------------------------------------------ (e) against sklearn


def test_fit_matches_sklearn_on_the_same_float32_values():
    from sklearn.neighbors import LocalOutlierFactor

    k, x32 = 20, normal_case()["x"].astype(np.float32)
    n, d = x32.shape
    eps = (d + 3) * 2.0 ** -24
    bound = 2 * eps / (1 - eps)
    sk = LocalOutlierFactor(n_neighbors=k).fit(x32.astype(np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # nothing is clipped here
        model = N().LocalOutlierFactor(k).fit(dev(x32))
    # the reference alone: every row's neighbour set is settled beyond the distance error
    ref_d, ref_i = host_lists(exact_distances(x32, x32), k + 1, True)
    settled = (ref_d[:, k] - ref_d[:, k - 1]) > 2 * eps * ref_d[:, k - 1]
    compare = settled & settled[ref_i[:, :k]].all(axis=1)
    assert (~compare).sum() == 0
    assert model.n_neighbors_ == sk.n_neighbors_ == k and model.n_samples_fit_ == n and model.offset_ == sk.offset_ == -1.5
    _, got_i = N().fitted_lists(dev(x32), k)
    assert np.array_equal(np.sort(host(got_i), axis=1), np.sort(ref_i[:, :k], axis=1))
    want = sk.negative_outlier_factor_
    got = model.negative_outlier_factor_
    assert got.dtype == np.float64 and got.shape == (n,)
    parity("lof fit vs sklearn / bound", float((np.abs(got - want)[compare] / (bound * np.abs(want[compare]))).max()), 1.0)
    for cont in ("auto", 0.1):
        sk_c = LocalOutlierFactor(n_neighbors=k, contamination=cont)
        want_labels = sk_c.fit_predict(x32.astype(np.float64))
        mine = N().LocalOutlierFactor(k, contamination=cont)
        labels = mine.fit_predict(dev(x32))
        # "auto": offset_ is -1.5 on both sides.  0.1: offset_ is an interpolation of two order statistics of the scores,
        # all of one sign, so it moves by at most `bound` relative as well, and a label is settled beyond both movements
        assert abs(mine.offset_ - sk_c.offset_) <= (0.0 if cont == "auto" else bound * abs(sk_c.offset_))
        margin = bound * np.abs(want) + (0.0 if cont == "auto" else bound * abs(sk_c.offset_))
        clear = np.abs(want - sk_c.offset_) > margin
        assert clear.sum() >= n - 2  # (the reference alone; the percentile lies between two scores)
        assert np.array_equal(labels[clear], want_labels[clear]) and labels.dtype == want_labels.dtype
    assert (labels == -1).sum() == 30  # strictly below the interpolated 10th percentile of 300 scores


def test_estimator_clips_and_warns_and_new_rows_follow_the_restatement():
    x, _, _ = lists(300)
    x32 = x.astype(np.float32)
    with pytest.warns(UserWarning, match="n_neighbors"):
        small = N().LocalOutlierFactor(20).fit(dev(x32[:5]))
    assert small.n_neighbors_ == 4 and small.n_samples_fit_ == 5
    k = 20
    model = N().LocalOutlierFactor(k, novelty=True, contamination=0.1).fit(dev(x32))
    dist_fit, idx_fit = (host(t) for t in N().fitted_lists(dev(x32), k))
    lrd_fit = N().ref_lrd(dist_fit, idx_fit, dist_fit, k)
    assert np.array_equal(model.kdist_, dist_fit[:, k - 1])
    # fitted rows given back as new rows find themselves at distance 0: not the fitted scores, but the restatement's
    new = np.concatenate([x32[:50], (x32[50:57] + 0.25).astype(np.float32)])
    dq, iq = (host(t) for t in M().knn_query(dev(new), dev(x32), k))
    assert np.array_equal(iq[:50, 0], np.arange(50)) and (dq[:50, 0] == 0.0).all()
    lrd_q = N().ref_lrd(dq, iq, dist_fit, k)
    want = -N().ref_lof(iq, lrd_q, lrd_fit, k)[0]
    got = model.score_samples(dev(new))
    parity("lof score_samples vs restatement / bound", float((np.abs(got - want) / (lof_bound(k) * np.abs(want))).max()), 1.0)
    assert not np.array_equal(got[:50], model.negative_outlier_factor_[:50])
    assert np.array_equal(model.decision_function(dev(new)), got - model.offset_)
    assert np.array_equal(model.predict(dev(new)), np.where(got - model.offset_ < 0, -1, 1))


# ------------------------------------------------------------------------------------------------ golden embeddings

_GOLDEN = {}


def golden():
    if not _GOLDEN:
        _GOLDEN["x"] = golden_rows(12449)
    return _GOLDEN["x"]


def test_golden_embeddings_against_the_restatement_of_the_device_lists():
    x, k = golden(), 20
    assert x.shape == (12449, 512)
    scores = N().outlier_scores(dev(x), k)
    dist, idx = (host(t) for t in N().fitted_lists(dev(x), k))
    assert (idx != np.arange(len(x))[:, None]).all() and (np.diff(dist, axis=1) >= 0).all()
    want_lrd = N().ref_lrd(dist, idx, dist, k)
    want_lof = N().ref_lof(idx, want_lrd, want_lrd, k)
    parity("lof lrd golden / bound", worst(host(scores.lrd), want_lrd, [lrd_bound(k)]), 1.0)
    parity("lof factor golden / bound", worst(host(scores.lof), want_lof, [lof_bound(k)]), 1.0)
    deg = host(scores.indegree)
    assert np.array_equal(deg, N().ref_in_degree(idx, k)) and deg.sum() == k * len(x)
    assert np.array_equal(host(scores.kdist)[0], dist[:, k - 1])
    assert N().hubness(dev(x), k) == N().skewness(deg[0]) > 0.0


def test_golden_holdout_through_the_novelty_path():
    x, k = golden(), 20
    fit, hold = x[:-1000], x[-1000:]
    model = N().LocalOutlierFactor(k, novelty=True).fit(dev(fit))
    dist_fit, idx_fit = (host(t) for t in N().fitted_lists(dev(fit), k))
    lrd_fit = N().ref_lrd(dist_fit, idx_fit, dist_fit, k)
    parity("lof golden fitted lrd / bound", worst(model.local_reachability_density_[None], lrd_fit, [lrd_bound(k)]), 1.0)
    dq, iq = (host(t) for t in M().knn_query(dev(hold), dev(fit), k))
    want = -N().ref_lof(iq, N().ref_lrd(dq, iq, dist_fit, k), lrd_fit, k)[0]
    got = model.score_samples(dev(hold))
    assert got.shape == (1000,)
    parity("lof golden holdout vs restatement / bound", float((np.abs(got - want) / (lof_bound(k) * np.abs(want))).max()), 1.0)
    assert np.array_equal(model.predict(dev(hold)), np.where(got < -1.5, -1, 1))


# ------------------------------------------------------------------------------------------------ the driver script


def test_driver_script_writes_its_files(tmp_path):
    import json

    from scripts import embedding_outliers_amd as script

    golden_file = str(Path(__file__).resolve().parent / "golden" / "simsiam_preds_subset.npz")
    summary = script.main(["--embeddings", golden_file, "--rows", "700", "--neighbors", "5:15:5", "--contamination", "0.05",
                           "--holdout", "100", "--out", str(tmp_path)])
    nof, labels = np.load(tmp_path / "negative_outlier_factor.npy"), np.load(tmp_path / "labels.npy")
    kdist, indegree = np.load(tmp_path / "kdist.npy"), np.load(tmp_path / "indegree.npy")
    assert nof.shape == (4, 600) and nof.dtype == np.float64 and np.array_equal(nof[3], nof[:3].min(axis=0))
    assert labels.shape == (600,) and (labels == -1).sum() == 30 == summary["flagged_combined"]  # 5 % of 600, strictly below
    assert np.array_equal(labels == -1, nof[3] < summary["offsets"][3])
    assert kdist.shape == (3, 600) and kdist.dtype == np.float32 and (np.diff(kdist, axis=0) >= 0).all()
    assert indegree.shape == (3, 600) and indegree.dtype == np.int32 and indegree.sum(axis=1).tolist() == [3000, 6000, 9000]
    assert summary["neighbors"] == [5, 10, 15] and summary["most_anomalous_rows"][0] == int(np.argmin(nof[3]))
    assert set(summary["hubness"]) == {"5", "10", "15"} and "mean_lof_per_class" in summary
    hold, hold_labels = np.load(tmp_path / "holdout_negative_outlier_factor.npy"), np.load(tmp_path / "holdout_labels.npy")
    assert hold.shape == (4, 100) and np.array_equal(hold[3], hold[:3].min(axis=0)) and np.isfinite(hold).all()
    assert np.array_equal(hold_labels == -1, hold[3] < summary["offsets"][3]) and summary["holdout"] == 100
    assert json.loads((tmp_path / "summary.json").read_text())["flagged_combined"] == 30
