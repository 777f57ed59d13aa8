"""CPU checks of HDBSCAN's prediction for new rows and of the GLOSH outlier scores (ssl_wafermap_amd.cluster: glosh,
assign_from_tree, labels_from_mst(return_selected=True), approximate_predict's refusals, the wm_mreach_query entry
point's argument checks).  No GPU: the spanning trees come from numpy (test_cluster_cpu.prim_mst), the nearest fitted
row in mutual reachability from the float64 brute force below, which restates what the kernel computes."""
import math

import numpy as np
import pytest
from sklearn.datasets import make_blobs

from test_cluster_cpu import pairwise64, prim_mst, selected_cluster

# ------------------------------------------------------------------------------------------------ a tree built by hand
#
#   13 (root) -- points 0, 1 leave at 0.25; splits at 0.5 into
#     14 (A, 4 points) -- points 2, 3 leave at 1.0; 4, 5 at 2.0
#     15 (B, 7 points) -- point 6 leaves at 0.8; splits at 1.0 into
#       16 (B1, 3 points) -- point 7 leaves at 2.0; 8, 9 at 4.0
#       17 (B2, 3 points) -- point 10 leaves at 1.25; 11 at 2.5; 12 at 5.0
#
# own-row deaths:   13: 0.5   14: 2.0   15: 1.0   16: 4.0   17: 5.0
# propagated D:     13: 5.0   14: 2.0   15: 5.0   16: 4.0   17: 5.0
N_HAND = 13
HAND_ROWS = [(13, 0, 0.25, 1), (13, 1, 0.25, 1), (13, 14, 0.5, 4), (13, 15, 0.5, 7),
             (14, 2, 1.0, 1), (14, 3, 1.0, 1), (14, 4, 2.0, 1), (14, 5, 2.0, 1),
             (15, 6, 0.8, 1), (15, 16, 1.0, 3), (15, 17, 1.0, 3),
             (16, 7, 2.0, 1), (16, 8, 4.0, 1), (16, 9, 4.0, 1),
             (17, 10, 1.25, 1), (17, 11, 2.5, 1), (17, 12, 5.0, 1)]


def hand_tree():
    from ssl_wafermap_amd.cluster import CONDENSED_DTYPE

    return np.array(HAND_ROWS, dtype=CONDENSED_DTYPE)


def assign(selected, neighbor, weight, **kw):
    from ssl_wafermap_amd.cluster import assign_from_tree

    labels, prob, score = assign_from_tree(hand_tree(), N_HAND, selected, np.array(neighbor), np.array(weight, dtype=np.float64), **kw)
    assert labels.dtype == np.int64 and prob.dtype == np.float64 and score.dtype == np.float64
    return labels.tolist(), prob.tolist(), score.tolist()


def test_glosh_on_the_hand_built_tree():
    from ssl_wafermap_amd.cluster import glosh

    got = glosh(hand_tree(), N_HAND)
    want = [(5.0 - 0.25) / 5.0, (5.0 - 0.25) / 5.0,  # the root's D is the deepest leaf's
            0.5, 0.5, 0.0, 0.0,  # A: (2 - 1) / 2, and 0 for the last to leave
            (5.0 - 0.8) / 5.0,  # B's own point against B's propagated D
            0.5, 0.0, 0.0,  # B1: (4 - 2) / 4
            (5.0 - 1.25) / 5.0, 0.5, 0.0]  # B2
    assert got.dtype == np.float64 and got.tolist() == want


def test_assign_both_branches_of_the_walk():
    sel = [14, 16, 17]  # A, B1, B2 -> labels 0, 1, 2
    # neighbour 4 (A, lambda 2): weight 0.25 -> lam 4 >= 2: the neighbour left first, the row joins A itself, at A's death
    # weight 1.0 -> lam 1 < 2: climb, but A was born at 0.5 < 1, so the row still joins A, half way to its death
    labels, prob, score = assign(sel, [4, 4], [0.25, 1.0])
    assert labels == [0, 0] and prob == [1.0, 0.5] and score == [0.0, 0.5]
    # neighbour 11 (B2, lambda 2.5), weight 0.5 -> lam 2: B2 was born at 1 < 2: B2 itself
    labels, prob, score = assign(sel, [11], [0.5])
    assert labels == [2] and prob == [2.0 / 5.0] and score == [(5.0 - 2.0) / 5.0]


def test_assign_a_climb_past_a_selected_cluster_gives_noise():
    sel = [14, 16, 17]
    # neighbour 12 (B2, lambda 5): weight 4 -> lam 0.25: B2 (born 1.0) and B (born 0.5) are younger: the root, past
    # the selected B2; weight 1.25 -> lam 0.8: past B2 to B, which is not selected and has no selected ancestor
    labels, prob, score = assign(sel, [12, 12], [4.0, 1.25])
    assert labels == [-1, -1] and prob == [0.0, 0.0]
    assert score == [(5.0 - 0.25) / 5.0, (5.0 - 0.8) / 5.0]
    # with B selected instead of its children, the second climb ends in a labelled cluster: death[B] = 1.0, own rows only
    labels, prob, score = assign([14, 15], [12, 12, 11], [4.0, 1.25, 0.5])
    assert labels == [-1, 1, 1] and prob == [0.0, 0.8, 1.0]
    assert score == [(5.0 - 0.25) / 5.0, (5.0 - 0.8) / 5.0, (5.0 - 2.0) / 5.0]  # (the score is C's, B2 for the third)


def test_assign_weight_zero_is_lambda_infinity():
    labels, prob, score = assign([14, 16, 17], [8, 0], [0.0, 0.0])
    assert labels == [1, -1] and prob == [1.0, 0.0] and score == [0.0, 0.0]


def test_assign_root_selected_on_both_sides_of_the_threshold():
    # without an epsilon the threshold is the largest lambda among the root's own rows: 0.5
    labels, prob, score = assign([13], [0, 0, 12], [2.0, 2.5, 0.25], allow_single_cluster=True)
    assert labels == [0, -1, 0] and prob == [1.0, 0.0, 1.0]
    assert score == [(5.0 - 0.5) / 5.0, (5.0 - 0.4) / 5.0, (5.0 - 4.0) / 5.0]
    # with an epsilon it is 1 / epsilon = 0.25: lam 0.4 now belongs, lam 0.2 does not
    labels, prob, _ = assign([13], [0, 0], [2.5, 5.0], cluster_selection_epsilon=4.0, allow_single_cluster=True)
    assert labels == [0, -1] and prob == [0.4 / 0.5, 0.0]
    # the root in `selected` without the flag labels nothing, as in labels_from_mst
    labels, prob, _ = assign([13], [0, 12], [2.0, 0.25])
    assert labels == [-1, -1] and prob == [0.0, 0.0]


def test_assign_argument_errors():
    from ssl_wafermap_amd.cluster import assign_from_tree

    t = hand_tree()
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [14], np.array([13]), np.array([1.0]))  # neighbour out of range
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [14], np.array([1]), np.array([-1.0]))
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [14], np.array([1]), np.array([np.nan]))
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [16, 14], np.array([1]), np.array([1.0]))  # unsorted
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [18], np.array([1]), np.array([1.0]))  # no such cluster
    with pytest.raises(ValueError):
        assign_from_tree(t, N_HAND, [14], np.array([1, 2]), np.array([1.0]))
    empty = assign_from_tree(t, N_HAND, [14], np.zeros(0, dtype=np.int64), np.zeros(0))
    assert all(a.shape == (0,) for a in empty)


# ------------------------------------------------------------------------------------------------ blobs

CASES = [(5, 15, 0.0, "euclidean", 1.0), (1, 5, 0.0, "euclidean", 1.0), (10, 40, 2.0, "euclidean", 1.0),
         (5, 15, 0.0, "manhattan", 2.0)]  # (min_samples, min_cluster_size, epsilon, metric, alpha)


@pytest.fixture(scope="module")
def blobs_far():
    """The blobs of test_cluster_cpu (no duplicate rows) and one row planted far from all of them (the last)."""
    x, _ = make_blobs(600, 16, centers=5, cluster_std=1.0, random_state=3)
    assert np.unique(x, axis=0).shape[0] == 600
    return np.concatenate([x, np.full((1, 16), 80.0)])


_FITS = {}


def fitted(x, case, allow_single_cluster=False):
    """(labels, probabilities, condensed tree, selected) once per case; shared and left unchanged."""
    from ssl_wafermap_amd.cluster import labels_from_mst

    key = (x.shape, case, allow_single_cluster)
    if key not in _FITS:
        ms, mcs, eps, metric, alpha = case
        _FITS[key] = labels_from_mst(*prim_mst(x, ms, metric, alpha), x.shape[0], mcs, eps,
                                     allow_single_cluster=allow_single_cluster, return_selected=True)
    return _FITS[key]


def brute_query(xq, x, min_samples, metric="euclidean", alpha=1.0):
    """Float64 restatement of the device path: the core distance of a fitted row is the min_samples-th smallest of its
    row of distances, itself included; that of a new row the min_samples-th smallest of {0} and its distances to the
    fitted rows; w_ic = max(core_q[i], core[c], dist_ic / alpha); the answer is the c that minimises (w, dist, c)."""
    x, xq = np.asarray(x, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    core = np.sort(pairwise64(x, metric), axis=1)[:, min_samples - 1]
    if metric == "euclidean":
        dq = np.stack([np.sqrt(((x - row) ** 2).sum(axis=1)) for row in xq])
    else:
        dq = np.stack([np.abs(x - row).sum(axis=1) for row in xq])
    core_q = np.sort(np.concatenate([np.zeros((xq.shape[0], 1)), dq], axis=1), axis=1)[:, min_samples - 1]
    w = np.maximum(np.maximum(core_q[:, None], core[None, :]), dq / alpha)
    j = np.array([np.lexsort((np.arange(x.shape[0]), dq[i], w[i]))[0] for i in range(xq.shape[0])])
    return j, w[np.arange(xq.shape[0]), j]


@pytest.mark.parametrize("case", CASES)
def test_return_selected_lists_the_clusters_in_label_order(blobs_far, case):
    from ssl_wafermap_amd.cluster import labels_from_mst

    ms, mcs, eps, metric, alpha = case
    n = blobs_far.shape[0]
    labels, prob, tree, selected = fitted(blobs_far, case)
    three = labels_from_mst(*prim_mst(blobs_far, ms, metric, alpha), n, mcs, eps)
    assert len(three) == 3 and np.array_equal(three[0], labels) and np.array_equal(three[1], prob)
    assert selected.dtype == np.int64 and selected.shape == (labels.max() + 1,) and (np.diff(selected) > 0).all()
    pts = tree[tree["child_size"] == 1]
    parent_of = np.empty(n, dtype=np.int64)
    parent_of[pts["child"]] = pts["parent"]
    for c in range(labels.max() + 1):
        assert selected_cluster(tree, parent_of[labels == c]) == selected[c]


@pytest.mark.parametrize("case", CASES)
def test_glosh_on_blobs(blobs_far, case):
    from ssl_wafermap_amd.cluster import glosh

    n = blobs_far.shape[0]
    _, _, tree, _ = fitted(blobs_far, case)
    score = glosh(tree, n)
    assert score.shape == (n,) and ((score >= 0) & (score <= 1)).all()
    cl = tree[tree["child_size"] > 1]
    leaves = set(tree["parent"].tolist()) - set(cl["parent"].tolist())
    assert leaves
    for leaf in leaves:
        rows = tree[tree["parent"] == leaf]
        last = rows["child"][rows["lambda_val"] == rows["lambda_val"].max()]
        assert (score[last] == 0).all()
    assert int(np.argmax(score)) == n - 1 and (score[:-1] < score[-1]).all()  # the planted row


def check_self_prediction(labels, prob, score, got):
    """A fitted row that belongs to a cluster, presented as a new row, is assigned its own label, at least as surely
    and at most as anomalous as in the fit.  Under the (w, dist, j) order the query's nearest fitted row is its twin
    (distance 0) unless another has a strictly smaller w, and either way the walk cannot leave the twin's cluster.
    Noise rows may be promoted (the query sees its twin as a neighbour): nothing is asserted for them."""
    got_labels, got_prob, got_score = got
    own = labels >= 0
    assert own.any()
    assert np.array_equal(got_labels[own], labels[own])
    assert (got_prob[own] >= prob[own]).all()
    assert (got_score[own] <= score[own]).all()
    return int((got_labels[~own] >= 0).sum())


@pytest.mark.parametrize("case", CASES)
def test_fitted_rows_predict_their_own_cluster(blobs_far, case):
    from ssl_wafermap_amd.cluster import assign_from_tree, glosh

    ms, _, eps, metric, alpha = case
    n = blobs_far.shape[0]
    labels, prob, tree, selected = fitted(blobs_far, case)
    assert labels[-1] == -1  # the planted row is noise
    j, w = brute_query(blobs_far, blobs_far, ms, metric, alpha)
    got = assign_from_tree(tree, n, selected, j, w, eps)
    check_self_prediction(labels, prob, glosh(tree, n), got)
    assert ((got[1] >= 0) & (got[1] <= 1)).all() and ((got[2] >= 0) & (got[2] <= 1)).all()
    assert (got[1][got[0] == -1] == 0).all()


@pytest.mark.parametrize("eps", [0.0, 3.0])
def test_fitted_rows_predict_the_single_cluster(eps):
    from ssl_wafermap_amd.cluster import assign_from_tree, glosh

    x, _ = make_blobs(300, 8, centers=1, cluster_std=1.0, random_state=5)
    case = (5, 20, eps, "euclidean", 1.0)
    labels, prob, tree, selected = fitted(x, case, allow_single_cluster=True)
    assert selected.tolist() == [300] and set(labels.tolist()) == {-1, 0}  # the root is the one cluster
    j, w = brute_query(x, x, 5)
    check_self_prediction(labels, prob, glosh(tree, 300), assign_from_tree(tree, 300, selected, j, w, eps, allow_single_cluster=True))
    none = assign_from_tree(tree, 300, selected, j, w, eps)
    assert (none[0] == -1).all() and (none[1] == 0).all()


def test_new_rows_near_a_blob_join_it_and_far_rows_are_noise(blobs_far):
    from ssl_wafermap_amd.cluster import assign_from_tree

    case = CASES[0]
    labels, _, tree, selected = fitted(blobs_far, case)
    rng = np.random.default_rng(0)
    near = blobs_far[[0, 100, 200, 300]] + 0.05 * rng.standard_normal((4, 16))
    far = np.full((2, 16), -90.0) + rng.standard_normal((2, 16))
    j, w = brute_query(np.concatenate([near, far]), blobs_far, case[0])
    got_labels, got_prob, got_score = assign_from_tree(tree, blobs_far.shape[0], selected, j, w)
    assert np.array_equal(got_labels[:4], labels[[0, 100, 200, 300]]) and (got_prob[:4] > 0).all()
    assert (got_labels[4:] == -1).all() and (got_prob[4:] == 0).all() and (got_score[4:] > got_score[:4].max()).all()


# ------------------------------------------------------------------------------------------------ model state, refusals


def host_model(x, **kw):
    """An HDBSCAN whose tree comes from numpy: what `fit` stores short of the device tensors."""
    from ssl_wafermap_amd import cluster

    model = cluster.HDBSCAN(**kw)
    k = model.min_cluster_size if model.min_samples is None else model.min_samples
    u, v, w = prim_mst(x, k)
    model.minimum_spanning_tree_ = np.stack([u.astype(np.float64), v.astype(np.float64), w], axis=1)
    model._n, model._k = x.shape[0], k
    return model.refit()


def test_refit_sets_selected_clusters_and_outlier_scores(blobs_far):
    from ssl_wafermap_amd import cluster

    model = host_model(blobs_far, min_cluster_size=15, min_samples=5)
    labels, _, tree, selected = fitted(blobs_far, CASES[0])
    assert np.array_equal(model.labels_, labels) and np.array_equal(model.selected_clusters_, selected)
    assert np.array_equal(model.outlier_scores_, cluster.glosh(tree, blobs_far.shape[0]))
    model.refit(min_cluster_size=40, cluster_selection_epsilon=2.0)
    ref = cluster.labels_from_mst(*prim_mst(blobs_far, 5), blobs_far.shape[0], 40, 2.0, return_selected=True)
    assert np.array_equal(model.selected_clusters_, ref[3])
    assert np.array_equal(model.outlier_scores_, cluster.glosh(ref[2], blobs_far.shape[0]))


def test_prediction_refusals_and_stored_state(blobs_far):
    import torch

    from ssl_wafermap_amd import _lib, cluster

    rows = torch.zeros(3, 16)
    plain = cluster.HDBSCAN()
    assert plain.prediction_data is False and plain._train is None and plain._core is None
    assert plain.selected_clusters_ is None and plain.outlier_scores_ is None
    for fn in (cluster.approximate_predict, cluster.approximate_predict_scores):
        with pytest.raises(RuntimeError):
            fn(cluster.HDBSCAN(prediction_data=True), rows)  # before fit
        with pytest.raises(ValueError, match="prediction_data"):
            fn(host_model(blobs_far, min_cluster_size=15, min_samples=5), rows)
        keeps = host_model(blobs_far, min_cluster_size=15, min_samples=5, prediction_data=True)
        keeps._train, keeps._core = torch.zeros(blobs_far.shape[0], 16), torch.zeros(blobs_far.shape[0])  # (stand-ins: not reached)
        with pytest.raises(_lib.WaferHipError):
            fn(keeps, rows)  # a CPU tensor
    assert cluster.HDBSCAN(prediction_data=True).prediction_data is True
    with pytest.raises(_lib.WaferHipError):
        cluster.HDBSCAN(prediction_data=True).fit(torch.zeros(8, 4))
    with pytest.raises(_lib.WaferHipError):
        cluster.mreach_query(torch.zeros(3, 4), torch.zeros(3), torch.zeros(8, 4), torch.zeros(8))
    with pytest.raises(_lib.WaferHipError):
        cluster.query_core_distances(torch.zeros(3, 4), torch.zeros(8, 4), 2)


def test_mreach_query_validates_before_any_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_mreach_query(None, None, 4, None, None, 8, 4, 0, 1.0, None, None, None, None, 0, None) == -1
    assert lib.wm_mreach_query_workspace_bytes(0, 100, 8) == 0 and lib.wm_mreach_query_workspace_bytes(10, 0, 8) == 0
    assert lib.wm_mreach_query_workspace_bytes(10, 100, 0) == 0
    assert lib.wm_mreach_query_workspace_bytes((1 << 24) + 1, 100, 8) == 0
    assert lib.wm_mreach_query_workspace_bytes(10, 100, 8) >= 10 * 12
    assert math.isfinite(lib.wm_mreach_query_workspace_bytes(4096, 60000, 52))
