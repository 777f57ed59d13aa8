"""CPU checks of HDBSCAN's soft clustering (ssl_wafermap_amd.cluster: exemplars_from_tree, membership_from_tree,
HDBSCAN.exemplar_indices_, the refusals of all_points_membership_vectors / membership_vector, the argument checks of
the wm_group_min_dist entry point).  No GPU: the trees come from the hand-built tree of test_hdbscan_predict_cpu and
from numpy (test_cluster_cpu.prim_mst), the exemplar distances from float64 brute force (test_cluster_cpu.pairwise64)."""
import math

import numpy as np
import pytest

from test_cluster_cpu import pairwise64, prim_mst
from test_hdbscan_predict_cpu import HAND_ROWS, N_HAND, hand_tree, host_model

INF = math.inf
SEL = [14, 16, 17]  # A, B1, B2
D = {14: 2.0, 16: 4.0, 17: 5.0}  # the propagated deaths of the three


def soft(selected, at, lam, dist, tree=None):
    from ssl_wafermap_amd.cluster import membership_from_tree

    out, parts = membership_from_tree(hand_tree() if tree is None else tree, N_HAND, selected, np.array(at), np.array(lam, dtype=np.float64),
                                      np.array(dist, dtype=np.float64).reshape(len(at), len(selected)), return_parts=True)
    assert out.dtype == np.float64 and out.shape == (len(at), len(selected))
    return out, parts


def combine(a, s, p):
    """The result from a row's distance vector, scores and probability, by the formulas of the specification."""
    a, s = np.array(a, dtype=np.float64), np.array(s, dtype=np.float64)
    outlier = np.isinf(s) / np.isinf(s).sum() if np.isinf(s).any() else np.exp(s - s.max()) / np.exp(s - s.max()).sum()
    prod = a * outlier
    return prod / prod.sum() * p


# ------------------------------------------------------------------------------------------------ the hand-built tree


def test_exemplars_on_the_hand_built_tree():
    from ssl_wafermap_amd.cluster import exemplars_from_tree

    got = exemplars_from_tree(hand_tree(), N_HAND, SEL)
    assert [g.tolist() for g in got] == [[4, 5], [8, 9], [12]] and all(g.dtype == np.int64 for g in got)
    assert [g.tolist() for g in exemplars_from_tree(hand_tree(), N_HAND, [14, 15])] == [[4, 5], [8, 9, 12]]  # B: both leaves
    assert [g.tolist() for g in exemplars_from_tree(hand_tree(), N_HAND, [13])] == [[4, 5, 8, 9, 12]]  # the root: every leaf
    assert exemplars_from_tree(hand_tree(), N_HAND, []) == []
    with pytest.raises(ValueError):
        exemplars_from_tree(hand_tree(), N_HAND, [16, 14])
    with pytest.raises(ValueError):
        exemplars_from_tree(hand_tree(), N_HAND, [18])


def test_merge_heights_scores_and_probability_of_the_worked_rows():
    """Row 7 (in B1 at lambda 2), row 6 (B's own point, noise under this selection, lambda 0.8) and row 0 (the root's,
    lambda 0.25), with exemplar distances given by hand."""
    dist = [[4.0, 1.0, 2.0], [2.0, 1.0, 1.0], [1.0, 2.0, 4.0]]
    out, parts = soft(SEL, [16, 15, 13], [2.0, 0.8, 0.25], dist)
    assert parts["h"].tolist() == [[0.5, 2.0, 1.0], [0.5, 0.8, 0.8], [0.25, 0.25, 0.25]]
    want_s = [[2.0 / (2.0 - 0.5), 4.0 / (4.0 - 2.0), 5.0 / (5.0 - 1.0)],
              [2.0 / (2.0 - 0.5), 4.0 / (4.0 - 0.8), 5.0 / (5.0 - 0.8)],
              [2.0 / (2.0 - 0.25), 4.0 / (4.0 - 0.25), 5.0 / (5.0 - 0.25)]]
    assert parts["s"].tolist() == want_s and want_s[0] == [4.0 / 3.0, 2.0, 1.25]
    assert parts["p"].tolist() == [2.0 / 4.0, 0.8 / 4.0, 0.25 / 2.0]  # c* = B1, B1 (the first of two), A (the first of three)
    want_a = [[1 / 7, 4 / 7, 2 / 7], [0.2, 0.4, 0.4], [4 / 7, 2 / 7, 1 / 7]]
    assert np.allclose(parts["a"], want_a, rtol=1e-15, atol=0)
    for i in range(3):
        assert np.allclose(out[i], combine(parts["a"][i], want_s[i], parts["p"][i]), rtol=4e-16, atol=0)
        assert abs(out[i].sum() - parts["p"][i]) <= 1e-15
    assert out[0].argmax() == 1 and out[2].argmax() == 0


def test_zero_distance_infinite_distance_and_infinite_lambda():
    # row 4, an exemplar of A: at distance 0 from A the distance vector is one-hot, and the last row to leave A has an
    # infinite score there; B2 at an infinite distance
    out, parts = soft(SEL, [14], [2.0], [[0.0, 3.0, INF]])
    assert parts["a"].tolist() == [[1.0, 0.0, 0.0]] and parts["h"].tolist() == [[2.0, 0.5, 0.5]]
    assert parts["s"][0, 0] == INF and parts["outlier"].tolist() == [[1.0, 0.0, 0.0]] and parts["p"].tolist() == [1.0]
    assert out.tolist() == [[1.0, 0.0, 0.0]]
    # two zero distances share the distance vector
    _, parts = soft(SEL, [16], [2.0], [[0.0, 0.0, 1.0]])
    assert parts["a"].tolist() == [[0.5, 0.5, 0.0]]
    # a cluster at an infinite distance gets nothing; the others keep their proportions
    out, parts = soft(SEL, [16], [2.0], [[1.0, 2.0, INF]])
    assert np.allclose(parts["a"], [[2 / 3, 1 / 3, 0.0]], rtol=1e-15, atol=0) and out[0, 2] == 0.0
    assert np.allclose(out[0], combine(parts["a"][0], [4.0 / 3.0, 2.0, 1.25], 0.5), rtol=4e-16, atol=0)
    # every cluster at an infinite distance: zeros, not NaN
    out, _ = soft(SEL, [16], [2.0], [[INF, INF, INF]])
    assert out.tolist() == [[0.0, 0.0, 0.0]]
    # an infinite lambda in B2 becomes B2's propagated death, 5: the row behaves like row 12, the last to leave
    out, parts = soft(SEL, [17], [INF], [[3.0, 2.0, 0.0]])
    assert parts["lam"].tolist() == [5.0] and parts["h"].tolist() == [[0.5, 1.0, 5.0]]
    assert parts["s"][0, 2] == INF and parts["p"].tolist() == [1.0] and out.tolist() == [[0.0, 0.0, 1.0]]
    # where that death is infinite too (row 12 a duplicate: lambda inf), the largest finite lambda of the tree: 4
    rows = list(HAND_ROWS)
    rows[-1] = (17, 12, INF, 1)
    from ssl_wafermap_amd.cluster import CONDENSED_DTYPE

    # and so do the infinite deaths of B2, B and the root: D = 2, 4, 4 for A, B1, B2.  Every score stays a ratio of finite
    # numbers and every row sums to its p, the rows of the other clusters included
    dup = np.array(rows, dtype=CONDENSED_DTYPE)
    dist = [[3.0, 2.0, 0.0], [4.0, 1.0, 2.0], [1.0, 2.0, 4.0], [1.0, 2.0, 4.0]]
    out, parts = soft(SEL, [17, 16, 14, 13], [INF, 2.0, 1.0, 0.25], dist, tree=dup)
    assert parts["lam"].tolist() == [4.0, 2.0, 1.0, 0.25]
    assert parts["h"].tolist() == [[0.5, 1.0, 4.0], [0.5, 2.0, 1.0], [1.0, 0.5, 0.5], [0.25, 0.25, 0.25]]
    want_s = [[4.0 / 3.5, 4.0 / 3.0, INF], [2.0 / 1.5, 4.0 / 2.0, 4.0 / 3.0], [2.0 / 1.0, 4.0 / 3.5, 4.0 / 3.5],
              [2.0 / 1.75, 4.0 / 3.75, 4.0 / 3.75]]
    assert parts["s"].tolist() == want_s and parts["p"].tolist() == [1.0, 0.5, 0.5, 0.125]
    assert out[0].tolist() == [0.0, 0.0, 1.0]  # the duplicate itself: the last to leave B2
    for i in (1, 2, 3):
        assert np.allclose(out[i], combine(parts["a"][i], want_s[i], parts["p"][i]), rtol=4e-16, atol=0)
        assert (out[i] > 0).all() and abs(out[i].sum() - parts["p"][i]) <= 1e-15
    # a new row that lands deeper than every finite lambda keeps its own lambda: in B1 at 8, D[B1] = 4: s = 8 / 0 = inf
    out, parts = soft(SEL, [16], [8.0], [[4.0, 1.0, 2.0]], tree=dup)
    assert parts["h"].tolist() == [[0.5, 8.0, 1.0]] and parts["p"].tolist() == [1.0] and out.tolist() == [[0.0, 1.0, 0.0]]


def test_selected_parent_and_root_and_no_cluster():
    # B selected instead of its children: rows in B1 and B2 are on B's lineage; A against them splits at 0.5.
    # D[B] = 5: row 7 scores 5 / (5 - 2) for B, 2 / (2 - 0.5) for A; p = 2 / 5
    out, parts = soft([14, 15], [16, 14], [2.0, 1.0], [[2.0, 1.0], [1.0, 2.0]])
    assert parts["h"].tolist() == [[0.5, 2.0], [1.0, 0.5]] and parts["p"].tolist() == [2.0 / 5.0, 1.0 / 2.0]
    assert parts["s"].tolist() == [[2.0 / 1.5, 5.0 / 3.0], [2.0 / 1.0, 5.0 / 4.5]]
    # the root as the single cluster: one column, lam / max(lam, the largest lambda of the tree)
    out, parts = soft([13], [16, 13, 17], [2.0, 0.25, 5.0], [[1.0], [3.0], [0.0]])
    assert out.tolist() == [[2.0 / 5.0], [0.25 / 5.0], [1.0]]
    # no cluster at all
    from ssl_wafermap_amd.cluster import membership_from_tree

    none = membership_from_tree(hand_tree(), N_HAND, [], np.array([16, 13]), np.array([2.0, 0.25]), np.zeros((2, 0)))
    assert none.shape == (2, 0) and none.dtype == np.float64
    with pytest.raises(ValueError):
        membership_from_tree(hand_tree(), N_HAND, SEL, np.array([16]), np.array([2.0]), np.zeros((1, 2)))
    with pytest.raises(ValueError):
        membership_from_tree(hand_tree(), N_HAND, SEL, np.array([12]), np.array([2.0]), np.zeros((1, 3)))  # a point id
    with pytest.raises(ValueError):
        membership_from_tree(hand_tree(), N_HAND, SEL, np.array([16]), np.array([-1.0]), np.zeros((1, 3)))


def test_assign_from_tree_shares_the_walk():
    """The walk factored out of assign_from_tree gives the (C, lam) its docstring states."""
    from ssl_wafermap_amd.cluster import _tree_tables, _walk

    _, cl_parent, birth, _, _, pt_parent, pt_lam = _tree_tables(hand_tree(), N_HAND)
    at, lam = _walk(N_HAND, cl_parent, birth, pt_parent, pt_lam, np.array([4, 4, 12, 12, 8]), np.array([0.25, 1.0, 4.0, 1.25, 0.0]))
    assert at.tolist() == [14, 14, 13, 15, 16] and lam.tolist() == [4.0, 1.0, 0.25, 0.8, INF]


# ------------------------------------------------------------------------------------------------ blobs

N_BLOB, PER, DIM, SPACING = 3, 80, 8, 12.0


@pytest.fixture(scope="module")
def noisy_blobs():
    """300 rows: three unit Gaussian blobs of 80 rows, SPACING = 12 standard deviations apart on three axes of R^8,
    and 60 rows uniform in the box [-18, 30]^8 (sparse: noise); min_samples 5, min_cluster_size 15.  At this spacing
    the host path puts the largest membership of every clustered row on its own label (asserted below)."""
    from ssl_wafermap_amd.cluster import _tree_tables, exemplars_from_tree, labels_from_mst

    rng = np.random.default_rng(7)
    blob = np.repeat(np.arange(N_BLOB), PER)
    x = np.concatenate([SPACING * np.eye(DIM)[blob] + rng.standard_normal((N_BLOB * PER, DIM)), rng.uniform(-18.0, 30.0, (60, DIM))])
    n = x.shape[0]
    labels, prob, tree, selected = labels_from_mst(*prim_mst(x, 5), n, 15, return_selected=True)
    assert selected.size == N_BLOB and (labels == -1).sum() >= 30
    for b in range(N_BLOB):
        of_blob = labels[:N_BLOB * PER][blob == b]
        assert np.unique(of_blob[of_blob >= 0]).size == 1  # one cluster per blob
    ex = exemplars_from_tree(tree, n, selected)
    dist = pairwise64(x)
    ex_dist = np.stack([dist[:, e].min(axis=1) for e in ex], axis=1)
    _, _, _, _, _, pt_parent, pt_lam = _tree_tables(tree, n)
    return x, labels, tree, selected, ex, ex_dist, pt_parent, pt_lam


def test_membership_properties_on_blobs(noisy_blobs):
    from ssl_wafermap_amd.cluster import membership_from_tree

    x, labels, tree, selected, ex, ex_dist, pt_parent, pt_lam = noisy_blobs
    n = x.shape[0]
    out, parts = membership_from_tree(tree, n, selected, pt_parent, pt_lam, ex_dist, return_parts=True)
    assert out.shape == (n, N_BLOB) and np.isfinite(out).all() and (out >= 0).all() and (out <= 1).all()
    assert (parts["p"] <= 1).all() and (parts["p"] >= 0).all()
    assert np.abs(out.sum(axis=1) - parts["p"]).max() <= 1e-12
    for c, rows in enumerate(ex):
        assert rows.size and (np.diff(rows) > 0).all() and (labels[rows] == c).all()
        assert (out[rows].argmax(axis=1) == c).all() and (parts["a"][rows, c] == 1).all()  # one-hot in the distance factor
    own = labels >= 0
    assert np.array_equal(out[own].argmax(axis=1), labels[own])
    assert np.array_equal(membership_from_tree(tree, n, selected, pt_parent, pt_lam, ex_dist), out)


def test_membership_with_a_cluster_of_exact_duplicates():
    """Three blobs of 80 rows, 20 rows of the first identical (more than min_cluster_size = 15): the duplicates leave at
    lambda inf, and their cluster and all its ancestors have an infinite death.  Every score must still be a number,
    every row must sum to its p, and the rows of the other blobs must be scored as without the duplicates."""
    from ssl_wafermap_amd.cluster import _tree_tables, exemplars_from_tree, labels_from_mst, membership_from_tree

    rng = np.random.default_rng(7)
    blob = np.repeat(np.arange(N_BLOB), PER)
    x = SPACING * np.eye(DIM)[blob] + rng.standard_normal((N_BLOB * PER, DIM))
    x[:20] = x[0]
    n = x.shape[0]
    labels, _, tree, selected = labels_from_mst(*prim_mst(x, 5), n, 15, return_selected=True)
    assert np.isinf(tree["lambda_val"]).sum() >= 20 and selected.size >= N_BLOB
    _, _, _, _, spread, pt_parent, pt_lam = _tree_tables(tree, n)
    assert np.isinf(spread[selected]).any() and np.isinf(spread[n])  # the case is what it claims
    ex = exemplars_from_tree(tree, n, selected)
    dist = pairwise64(x)
    ex_dist = np.stack([dist[:, e].min(axis=1) for e in ex], axis=1)
    out, parts = membership_from_tree(tree, n, selected, pt_parent, pt_lam, ex_dist, return_parts=True)
    assert not np.isnan(parts["s"]).any() and not np.isnan(parts["outlier"]).any() and np.isfinite(parts["lam"]).all()
    assert np.isfinite(out).all() and (out >= 0).all() and (out <= 1).all() and (parts["p"] <= 1).all()
    assert np.abs(out.sum(axis=1) - parts["p"]).max() <= 1e-12
    own = labels >= 0
    assert own.sum() >= 200 and (parts["p"][own] > 0).all() and np.array_equal(out[own].argmax(axis=1), labels[own])
    c_dup = labels[0]
    assert c_dup >= 0 and (labels[:20] == c_dup).all()
    assert (parts["p"][:20] == 1).all() and (out[:20, c_dup] == 1).all()  # the duplicates are the last to leave
    top = float(tree["lambda_val"][np.isfinite(tree["lambda_val"])].max())
    assert (parts["lam"][:20] == top).all()


def test_exemplar_indices_follow_a_refit(noisy_blobs):
    x = noisy_blobs[0]
    model = host_model(x, min_cluster_size=15, min_samples=5)
    first = model.exemplar_indices_
    assert [e.tolist() for e in first] == [e.tolist() for e in noisy_blobs[4]]
    assert model.exemplar_indices_ is first  # computed once
    model.refit(min_cluster_size=60)
    again = model.exemplar_indices_
    assert again is not first and len(again) == model.selected_clusters_.size
    assert [e.tolist() for e in again] != [e.tolist() for e in first]
    from ssl_wafermap_amd import cluster

    assert [e.tolist() for e in again] == [e.tolist() for e in cluster.exemplars_from_tree(model.condensed_tree_, x.shape[0], model.selected_clusters_)]
    assert cluster.HDBSCAN().exemplar_indices_ is None


# ------------------------------------------------------------------------------------------------ refusals, ABI


def test_soft_clustering_refusals(noisy_blobs, monkeypatch):
    import torch

    from ssl_wafermap_amd import _lib, cluster

    x = noisy_blobs[0]
    rows = torch.zeros(3, DIM)
    with pytest.raises(RuntimeError):
        cluster.all_points_membership_vectors(cluster.HDBSCAN(prediction_data=True))  # before fit
    with pytest.raises(RuntimeError):
        cluster.membership_vector(cluster.HDBSCAN(prediction_data=True), rows)
    plain = host_model(x, min_cluster_size=15, min_samples=5)
    with pytest.raises(ValueError, match="prediction_data"):
        cluster.all_points_membership_vectors(plain)
    with pytest.raises(ValueError, match="prediction_data"):
        cluster.membership_vector(plain, rows)
    keeps = host_model(x, min_cluster_size=15, min_samples=5, prediction_data=True)
    keeps._train, keeps._core = torch.zeros(x.shape[0], DIM), torch.zeros(x.shape[0])  # (stand-ins: no kernel is reached)
    with pytest.raises(_lib.WaferHipError):
        cluster.membership_vector(keeps, rows)  # a CPU tensor
    with pytest.raises(_lib.WaferHipError):
        cluster.all_points_membership_vectors(keeps)
    with pytest.raises(_lib.WaferHipError):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32), 1)
    # the checks behind the device check, which no CPU tensor passes: let them through to reach the others
    monkeypatch.setattr(cluster, "require_gpu", lambda *t: None)
    with pytest.raises(ValueError, match="features"):
        cluster.membership_vector(keeps, torch.zeros(3, DIM + 4))
    assert cluster.membership_vector(keeps, torch.zeros(0, DIM)).shape == (0, keeps.selected_clusters_.size)
    with pytest.raises(ValueError, match="features"):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 8), torch.zeros(8, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="group"):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 4), torch.zeros(7, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="group"):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 4), torch.zeros(8), 1)  # float ids
    with pytest.raises(ValueError, match="n_groups"):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 4), torch.full((8,), 2, dtype=torch.int32), 2)
    with pytest.raises(NotImplementedError):
        cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32), 1, "canberra")
    dist, j = cluster.group_min_distances(torch.zeros(3, 4), torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), 2)  # no column
    assert dist.shape == j.shape == (3, 2) and torch.isinf(dist).all() and (j == -1).all()


def test_group_min_dist_validates_before_any_launch():
    """The entry point's argument checks, in the order of test_mreach_query_argument_errors.  The pointers are stand-ins
    (16-byte aligned numbers): every call here returns before it would touch them."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    a = 4096
    need = lib.wm_group_min_dist_workspace_bytes(9, 65, 8, 3)
    assert need >= 2 * 9 * 3 * 8  # (65 columns against 9 rows: two column slices, merged from the workspace)

    def call(xq=a, m=9, xe=a, group=a, e=65, d=8, metric=0, g=3, out_d=a, out_j=a, ws=a, ws_bytes=need):
        return lib.wm_group_min_dist(xq, m, xe, group, e, d, metric, g, out_d, out_j, ws, ws_bytes, None)

    assert call(xq=None) == -1 and call(xe=None) == -1 and call(group=None) == -1 and call(out_d=None) == -1
    assert call(out_j=None) == -1 and call(ws=None) == -1
    assert call(m=0) == -1 and call(e=0) == -1 and call(d=0) == -1 and call(g=0) == -1
    assert call(m=(1 << 24) + 1) == -2 and call(e=(1 << 24) + 1) == -2 and call(d=6) == -2 and call(d=1028) == -2
    assert call(metric=2) == -2 and call(metric=-1) == -2
    assert call(ws_bytes=16) == -3
    assert lib.wm_group_min_dist_workspace_bytes(0, 65, 8, 3) == 0 and lib.wm_group_min_dist_workspace_bytes(9, 0, 8, 3) == 0
    assert lib.wm_group_min_dist_workspace_bytes(9, 65, 0, 3) == 0 and lib.wm_group_min_dist_workspace_bytes(9, 65, 8, 0) == 0
    assert lib.wm_group_min_dist_workspace_bytes((1 << 24) + 1, 65, 8, 3) == 0
    assert lib.wm_group_min_dist_workspace_bytes(811457, 2000, 52, 100) == 256  # one slice: straight into the outputs
