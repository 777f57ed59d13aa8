"""CPU checks of the clustering host code (ssl_wafermap_amd.cluster): labels_from_mst on a float64 Prim spanning tree
of the dense mutual-reachability matrix against sklearn.cluster.HDBSCAN(algorithm="brute"), the selection variants,
exact weight ties, the edge sizes and the argument errors.  No GPU: the tree here comes from numpy."""
import numpy as np
import pytest
from sklearn.cluster import HDBSCAN as SkHDBSCAN
from sklearn.datasets import make_blobs
from sklearn.metrics import adjusted_rand_score

BLOB_PARAMS = [(5, 15, 0.0), (1, 5, 0.0), (10, 40, 2.0)]  # (min_samples, min_cluster_size, epsilon)


def pairwise64(x, metric="euclidean"):
    x = np.asarray(x, dtype=np.float64)
    if metric == "euclidean":
        return np.stack([np.sqrt(((x - row) ** 2).sum(axis=1)) for row in x])
    return np.stack([np.abs(x - row).sum(axis=1) for row in x])


def prim_mst(x, min_samples, metric="euclidean", alpha=1.0):
    """(u, v, w) of the mutual-reachability MST in float64, u < v, sorted by (w, u, v); the core distance is the
    min_samples-th smallest of the row including the zero self-distance."""
    dist = pairwise64(x, metric)
    n = dist.shape[0]
    core = np.sort(dist, axis=1)[:, min_samples - 1]
    mr = np.maximum(np.maximum(core[:, None], core[None, :]), dist / alpha)
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    best, src = mr[0].copy(), np.zeros(n, dtype=np.int64)
    best[0] = np.inf
    u, v, w = [], [], []
    for _ in range(n - 1):
        j = int(np.argmin(best))
        u.append(min(j, int(src[j])))
        v.append(max(j, int(src[j])))
        w.append(best[j])
        in_tree[j] = True
        closer = (mr[j] < best) & ~in_tree
        best[closer], src[closer] = mr[j][closer], j
        best[j] = np.inf
    u, v, w = np.array(u), np.array(v), np.array(w)
    order = np.lexsort((v, u, w))
    return u[order], v[order], w[order]


def same_clustering(ours, theirs):
    assert np.array_equal(ours == -1, theirs == -1), "noise sets differ"
    assert adjusted_rand_score(theirs, ours) == 1.0


@pytest.fixture(scope="module")
def blobs():
    x, _ = make_blobs(600, 16, centers=5, cluster_std=1.0, random_state=3)
    return x


@pytest.fixture(scope="module")
def blob_trees(blobs):
    return {ms: prim_mst(blobs, ms) for ms in {p[0] for p in BLOB_PARAMS}}


@pytest.mark.parametrize("min_samples,min_cluster_size,eps", BLOB_PARAMS)
def test_labels_match_sklearn_on_blobs(blobs, blob_trees, min_samples, min_cluster_size, eps):
    from ssl_wafermap_amd.cluster import CONDENSED_DTYPE, labels_from_mst

    ref = SkHDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, cluster_selection_epsilon=eps,
                    algorithm="brute", copy=True).fit(blobs)
    labels, prob, tree = labels_from_mst(*blob_trees[min_samples], 600, min_cluster_size, eps)
    same_clustering(labels, ref.labels_)
    assert tree.dtype == CONDENSED_DTYPE and tree.dtype.names == ("parent", "child", "lambda_val", "child_size")
    assert sorted(tree["child"][tree["child_size"] == 1].tolist()) == list(range(600))  # every point leaves once
    assert prob.shape == (600,) and ((prob >= 0) & (prob <= 1)).all()
    assert (prob[labels == -1] == 0).all() and (prob[labels >= 0] > 0).all()


@pytest.mark.parametrize("method,eps", [("leaf", 0.0), ("leaf", 2.0), ("eom", 0.5)])
def test_selection_variants_match_sklearn(blobs, blob_trees, method, eps):
    from ssl_wafermap_amd.cluster import labels_from_mst

    ref = SkHDBSCAN(min_cluster_size=15, min_samples=5, cluster_selection_epsilon=eps, cluster_selection_method=method,
                    algorithm="brute", copy=True).fit(blobs)
    labels, _, _ = labels_from_mst(*blob_trees[5], 600, 15, eps, cluster_selection_method=method)
    same_clustering(labels, ref.labels_)


def selected_cluster(tree, point_parents):
    """Condensed-tree id of the cluster that owns points whose rows have these parents: their deepest common
    ancestor (ids grow downwards, and a selected cluster either loses points itself or splits in two)."""
    cl = tree[tree["child_size"] > 1]
    up = dict(zip(cl["child"].tolist(), cl["parent"].tolist()))

    def chain(c):
        out = {c}
        while c in up:
            c = up[c]
            out.add(c)
        return out

    return max(set.intersection(*(chain(int(c)) for c in set(point_parents.tolist()))))


def check_probabilities(labels, prob, tree, sk_prob):
    """The membership strength is min(lambda_point, death) / death with death = the largest lambda over ALL condensed
    rows of the point's cluster, so the last point to leave a cluster has strength exactly 1.  sklearn takes the
    largest lambda of the LAST contiguous run of the cluster's rows only: where the cluster's rows form one run the
    two definitions agree and the values equal sklearn's (float64 arithmetic on trees whose weights agree to
    rounding: 1e-9 relative); elsewhere sklearn's death is no larger, so its strengths are no smaller.  Returns the
    number of clusters whose rows form one run."""
    n = labels.size
    pts = tree[tree["child_size"] == 1]
    lam_of, parent_of = np.empty(n), np.empty(n, dtype=np.int64)
    lam_of[pts["child"]], parent_of[pts["child"]] = pts["lambda_val"], pts["parent"]
    one_run = 0
    for c in range(labels.max() + 1):
        members = np.flatnonzero(labels == c)
        rows = np.flatnonzero(tree["parent"] == selected_cluster(tree, parent_of[members]))
        death = tree["lambda_val"][rows].max()
        assert np.isfinite(death) and death > 0
        assert np.array_equal(prob[members], np.minimum(lam_of[members], death) / death)
        assert prob[members].max() == 1.0
        if rows[-1] - rows[0] + 1 == rows.size:
            one_run += 1
            np.testing.assert_allclose(prob[members], sk_prob[members], rtol=1e-9, atol=0)
        else:
            assert (sk_prob[members] >= prob[members] * (1 - 1e-9)).all()
    return one_run


@pytest.mark.parametrize("min_samples,min_cluster_size,eps", BLOB_PARAMS)
def test_probabilities_take_the_largest_lambda_of_the_cluster(blobs, blob_trees, min_samples, min_cluster_size, eps):
    from ssl_wafermap_amd.cluster import labels_from_mst

    ref = SkHDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, cluster_selection_epsilon=eps,
                    algorithm="brute", copy=True).fit(blobs)
    labels, prob, tree = labels_from_mst(*blob_trees[min_samples], 600, min_cluster_size, eps)
    assert np.array_equal(labels, ref.labels_)  # (clusters are numbered in the same order)
    check_probabilities(labels, prob, tree, ref.probabilities_)


def test_probabilities_equal_sklearn_where_the_clusters_rows_are_contiguous():
    """One blob with allow_single_cluster: the root is the one cluster and all its condensed rows form one run, so the
    membership strengths are sklearn's (sibling clusters interleave their rows level by level: none of the blobs' clusters forms one run)."""
    from ssl_wafermap_amd.cluster import labels_from_mst

    x, _ = make_blobs(300, 8, centers=1, cluster_std=1.0, random_state=5)
    ref = SkHDBSCAN(min_cluster_size=20, min_samples=5, allow_single_cluster=True, algorithm="brute", copy=True).fit(x)
    labels, prob, tree = labels_from_mst(*prim_mst(x, 5), 300, 20, allow_single_cluster=True)
    assert np.array_equal(labels, ref.labels_) and labels.max() == 0
    assert check_probabilities(labels, prob, tree, ref.probabilities_) == 1
    assert (prob[labels == -1] == 0).all() and (ref.probabilities_[labels == -1] == 0).all()


@pytest.mark.parametrize("eps", [0.0, 3.0])
def test_allow_single_cluster_on_one_blob(eps):
    from ssl_wafermap_amd.cluster import labels_from_mst

    x, _ = make_blobs(300, 8, centers=1, cluster_std=1.0, random_state=5)
    ref = SkHDBSCAN(min_cluster_size=20, min_samples=5, allow_single_cluster=True, cluster_selection_epsilon=eps,
                    algorithm="brute", copy=True).fit(x)
    labels, _, _ = labels_from_mst(*prim_mst(x, 5), 300, 20, eps, allow_single_cluster=True)
    assert set(ref.labels_.tolist()) == {-1, 0}  # the case is what it claims to be: the root is the one cluster
    assert np.array_equal(labels, ref.labels_)
    # without the flag the same tree gives what sklearn gives
    ref2 = SkHDBSCAN(min_cluster_size=20, min_samples=5, cluster_selection_epsilon=eps, algorithm="brute", copy=True).fit(x)
    same_clustering(labels_from_mst(*prim_mst(x, 5), 300, 20, eps)[0], ref2.labels_)


def lattice_points():
    """Three 6 x 6 integer grids far apart plus four far points: every distance inside a grid is one of a
    few exactly representable values, so the spanning tree is full of equal weights."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    pts = np.concatenate([g, g + [40, 0], g + [0, 40], [[20, 20], [70, 70], [-30, 10], [10, -30]]])
    return np.concatenate([pts, np.zeros((pts.shape[0], 2))], axis=1)


@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
def test_exact_weight_ties_on_a_lattice(metric):
    from ssl_wafermap_amd.cluster import labels_from_mst

    x = lattice_points()
    n = x.shape[0]
    u, v, w = prim_mst(x, 4, metric)
    assert np.unique(w).size < n // 4  # ties indeed
    labels, prob, _ = labels_from_mst(u, v, w, n, 10)
    # the clustering is decided by the geometry, whatever order equal edges take: the three grids are the clusters
    # (a far point may hang on to the grid it joins first, with a small membership strength)
    assert (prob[108:] < 0.2).all()
    for g in range(3):
        assert np.unique(labels[36 * g:36 * (g + 1)]).size == 1 and labels[36 * g] >= 0
    assert np.unique(labels[:108]).size == 3
    ref = SkHDBSCAN(min_cluster_size=10, min_samples=4, metric=metric, algorithm="brute", copy=True).fit(x)
    same_clustering(labels, ref.labels_)
    # any order of the equal-weight edges gives the same labels
    rng = np.random.default_rng(0)
    order = np.lexsort((rng.permutation(n - 1), w))
    again, _, _ = labels_from_mst(u[order], v[order], w[order], n, 10)
    assert np.array_equal(again, labels)


def test_n_equal_to_min_cluster_size_and_tiny_inputs():
    from ssl_wafermap_amd.cluster import labels_from_mst

    x, _ = make_blobs(12, 4, centers=1, random_state=1)
    tree = prim_mst(x, 3)
    labels, prob, cond = labels_from_mst(*tree, 12, 12)
    ref = SkHDBSCAN(min_cluster_size=12, min_samples=3, algorithm="brute", copy=True).fit(x)
    assert np.array_equal(labels, ref.labels_) and (labels == -1).all() and (prob == 0).all()
    assert (cond["parent"] == 12).all() and len(cond) == 12
    one, _, _ = labels_from_mst(*tree, 12, 12, allow_single_cluster=True)
    ref1 = SkHDBSCAN(min_cluster_size=12, min_samples=3, allow_single_cluster=True, algorithm="brute", copy=True).fit(x)
    assert np.array_equal(one, ref1.labels_)
    two, _, _ = labels_from_mst(np.array([0]), np.array([1]), np.array([1.5]), 2, 2)
    assert two.tolist() == [-1, -1]
    # duplicated points: zero-weight edges (lambda = inf) do not break the stabilities' arithmetic
    xd = np.concatenate([x, x, x + 50.0, x + 50.0])
    ld, pd_, _ = labels_from_mst(*prim_mst(xd, 2), 48, 8)
    refd = SkHDBSCAN(min_cluster_size=8, min_samples=2, algorithm="brute", copy=True).fit(xd)
    same_clustering(ld, refd.labels_)
    assert np.isfinite(pd_).all()


def test_argument_errors():
    from ssl_wafermap_amd import cluster

    u, v, w = np.array([0, 1]), np.array([1, 2]), np.array([1.0, 2.0])
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, v, w, 4, 2)  # n - 1 edges
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, v, w, 3, 1)  # min_cluster_size
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, v, w[::-1], 3, 2)  # unsorted
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, np.array([1, 3]), w, 3, 2)  # endpoint out of range
    with pytest.raises(ValueError):
        cluster.labels_from_mst(np.array([0, 0]), np.array([1, 1]), w, 3, 2)  # a cycle
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, v, w, 3, 2, cluster_selection_method="best")
    with pytest.raises(ValueError):
        cluster.labels_from_mst(u, v, w, 3, 2, cluster_selection_epsilon=-1.0)
    with pytest.raises(ValueError):
        cluster.HDBSCAN(min_cluster_size=1)
    with pytest.raises(ValueError):
        cluster.HDBSCAN(min_samples=0)
    with pytest.raises(ValueError):
        cluster.HDBSCAN(metric="chebyshev")
    with pytest.raises(ValueError):
        cluster.HDBSCAN(alpha=0.0)
    with pytest.raises(RuntimeError):
        cluster.HDBSCAN().refit(min_cluster_size=10)


@pytest.mark.parametrize("metric", ["canberra", "braycurtis"])
def test_listed_but_unbuilt_metrics_say_so(metric):
    import torch

    from ssl_wafermap_amd import cluster

    with pytest.raises(NotImplementedError, match=metric):
        cluster.HDBSCAN(metric=metric)
    with pytest.raises(NotImplementedError, match=metric):
        cluster.core_distances(torch.zeros(8, 4), 2, metric=metric)
    with pytest.raises(NotImplementedError, match=metric):
        cluster.silhouette_samples(torch.zeros(8, 4), np.arange(8) % 2, metric=metric)


def test_kernels_have_no_cpu_fallback():
    import torch

    from ssl_wafermap_amd import _lib, cluster

    with pytest.raises(_lib.WaferHipError):
        cluster.core_distances(torch.zeros(8, 4), 2)
    with pytest.raises(_lib.WaferHipError):
        cluster.HDBSCAN().fit(torch.zeros(8, 4))
    with pytest.raises(_lib.WaferHipError):
        cluster.silhouette_samples(torch.zeros(8, 4), np.arange(8) % 2)


def test_entry_points_validate_before_any_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_core_distance(None, 8, 4, 0, 1, None, None, 0, None) == -1
    assert lib.wm_mreach_min_edge(None, None, None, 8, 4, 0, 1.0, None, None, None, 0, None) == -1
    assert lib.wm_cluster_dist_sums(None, None, 8, 4, 0, 2, None, None) == -1
    assert lib.wm_core_distance_workspace_bytes(100, 512, 65) == 0
    assert lib.wm_core_distance_workspace_bytes(100, 512, 64) >= 100 * 64 * 4
    assert lib.wm_mreach_min_edge_workspace_bytes(100, 512) >= 100 * 8
    assert lib.wm_mreach_min_edge_workspace_bytes(0, 512) == 0


def test_every_entry_point_checks_in_one_order_against_its_own_size_function():
    """Invalid, then unsupported, then misaligned, then workspace too small, for every entry point of cluster.hip; and
    every size function is exactly its entry point's requirement plus 256.  9 or 65 rows against 65 columns are two
    column slices, so every mode needs its planes.  The pointers are stand-ins: every call returns before a launch."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    a, cols, k, g = 4096, 65, 2, 3
    # name -> (rows of the first matrix, the size function of (rows, d) or None, the call of (x, rows, d, ws_bytes))
    table = {
        "wm_core_distance": (65, lambda r, d: lib.wm_core_distance_workspace_bytes(r, d, k),
                             lambda x, r, d, wb: lib.wm_core_distance(x, r, d, 0, k, a, a, wb, None)),
        "wm_knn_graph": (65, lambda r, d: lib.wm_knn_graph_workspace_bytes(r, d, k),
                         lambda x, r, d, wb: lib.wm_knn_graph(x, r, d, 0, k, a, a, a, wb, None)),
        "wm_knn_query": (9, lambda r, d: lib.wm_knn_query_workspace_bytes(r, cols, d, k),
                         lambda x, r, d, wb: lib.wm_knn_query(x, r, a, cols, d, 0, k, a, a, a, wb, None)),
        "wm_rank_query": (9, lambda r, d: lib.wm_rank_query_workspace_bytes(r, cols, d, k),
                          lambda x, r, d, wb: lib.wm_rank_query(x, r, a, cols, d, 0, a, a, a, k, a, a, wb, None)),
        "wm_mreach_min_edge": (65, lambda r, d: lib.wm_mreach_min_edge_workspace_bytes(r, d),
                               lambda x, r, d, wb: lib.wm_mreach_min_edge(x, a, a, r, d, 0, 1.0, a, a, a, wb, None)),
        "wm_mreach_min_edge_grouped": (65, lambda r, d: lib.wm_mreach_min_edge_grouped_workspace_bytes(r, d, g),
                                       lambda x, r, d, wb: lib.wm_mreach_min_edge_grouped(x, a, a, a, r, d, 0, g, a, a, a, wb, None)),
        "wm_allpoints_core": (65, lambda r, d: lib.wm_allpoints_core_workspace_bytes(r, d, g),
                              lambda x, r, d, wb: lib.wm_allpoints_core(x, a, r, d, 0, g, 8.0, a, a, wb, None)),
        "wm_mreach_query": (9, lambda r, d: lib.wm_mreach_query_workspace_bytes(r, cols, d),
                            lambda x, r, d, wb: lib.wm_mreach_query(x, a, r, a, a, cols, d, 0, 1.0, a, a, a, a, wb, None)),
        "wm_group_min_dist": (9, lambda r, d: lib.wm_group_min_dist_workspace_bytes(r, cols, d, g),
                              lambda x, r, d, wb: lib.wm_group_min_dist(x, r, a, a, cols, d, 0, g, a, a, a, wb, None)),
        "wm_group_min_mreach": (9, lambda r, d: lib.wm_group_min_mreach_workspace_bytes(r, cols, d, g),
                                lambda x, r, d, wb: lib.wm_group_min_mreach(x, a, r, a, a, a, cols, d, 0, g, a, a, a, wb, None)),
        "wm_pair_dist": (9, None, lambda x, r, d, wb: lib.wm_pair_dist(x, r, a, cols, d, 0, a, k, a, None)),
        "wm_cluster_dist_sums": (65, None, lambda x, r, d, wb: lib.wm_cluster_dist_sums(x, a, r, d, 0, g, a, None)),
    }
    assert len(table) == 12 and sum(size is not None for _, size, _ in table.values()) == 10
    for name, (rows, size, call) in table.items():
        need = size(rows, 8) if size else 0
        if size:
            assert need > 257, name
            assert call(a, rows, 8, need - 257) == -3, name  # one byte short of need - 256
        assert call(a + 8, rows, 8, need) == -4, name  # misaligned first matrix, everything else valid
        assert call(a + 8, rows, 6, need) == -2, name  # d = 6 wins over the misaligned pointer
        assert call(a + 8, 0, 6, need) == -1, name  # no rows wins over both


def test_host_scores_match_sklearn(blobs):
    from sklearn import metrics

    from ssl_wafermap_amd import cluster

    rng = np.random.default_rng(0)
    labels = rng.integers(0, 7, 600) * 3 - 1  # arbitrary label values, -1 among them
    truth = rng.integers(0, 4, 600)
    for ours, theirs in ((cluster.calinski_harabasz_score(blobs, labels), metrics.calinski_harabasz_score(blobs, labels)),
                         (cluster.davies_bouldin_score(blobs, labels), metrics.davies_bouldin_score(blobs, labels)),
                         (cluster.homogeneity_score(truth, labels), metrics.homogeneity_score(truth, labels)),
                         (cluster.homogeneity_score(truth, truth), 1.0)):
        assert abs(ours - theirs) <= 1e-10 * abs(theirs)
