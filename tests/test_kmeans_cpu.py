"""CPU checks of cluster.KMeans' host side: argument validation and refusals, the n_init="auto" rule, the stopping rule and
the empty-cluster rule as pure host functions on numpy inputs, and the size limits of the entry points (no launch)."""
import numpy as np
import pytest
import torch


def test_refusals_name_the_feature():
    from ssl_wafermap_amd import cluster

    with pytest.raises(NotImplementedError, match="elkan"):
        cluster.KMeans(4, algorithm="elkan")
    with pytest.raises(ValueError, match="algorithm"):
        cluster.KMeans(4, algorithm="hamerly")
    for call in ("fit", "fit_predict", "fit_transform", "score"):
        with pytest.raises(NotImplementedError, match="sample_weight"):
            getattr(cluster.KMeans(2), call)(torch.zeros(8, 4), sample_weight=np.ones(8))


def test_argument_validation():
    from ssl_wafermap_amd import _lib, cluster

    for kw in ({"n_clusters": 0}, {"init": "farthest"}, {"n_init": 0}, {"n_init": "many"}, {"max_iter": 0}, {"tol": -1.0}):
        with pytest.raises(ValueError):
            cluster.KMeans(**{"n_clusters": 3, **kw})
    with pytest.raises(_lib.WaferHipError):  # CPU tensors: as the rest of the module
        cluster.KMeans(2).fit(torch.zeros(8, 4))
    with pytest.raises(_lib.WaferHipError):
        cluster.kmeans_plusplus(torch.zeros(8, 4), 2)
    with pytest.raises(_lib.WaferHipError):
        cluster.kmeans_step(torch.zeros(8, 4), torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="before fit"):
        cluster.KMeans(2).predict(torch.zeros(8, 4))
    m = cluster.KMeans()
    assert (m.n_clusters, m.init, m.n_init, m.max_iter, m.tol, m.algorithm) == (8, "k-means++", "auto", 300, 1e-4, "lloyd")


def test_n_init_auto_rule():
    from ssl_wafermap_amd import cluster

    assert cluster.KMeans(3)._n_init == 1
    assert cluster.KMeans(3, init="k-means++", n_init="auto")._n_init == 1
    assert cluster.KMeans(3, init="random")._n_init == 10
    assert cluster.KMeans(3, init=np.zeros((3, 4), dtype=np.float32))._n_init == 1
    assert cluster.KMeans(3, init="random", n_init=4)._n_init == 4
    assert cluster.KMeans(3, n_init=7)._n_init == 7


def test_stopping_rule():
    from ssl_wafermap_amd.cluster import kmeans_stop

    assert kmeans_stop(0, 5.0, 1e-3) == "labels"  # strict convergence comes first
    assert kmeans_stop(0, 0.0, 0.0) == "labels"
    assert kmeans_stop(3, 1e-3, 1e-3) == "tol"  # at most the tolerance
    assert kmeans_stop(3, 0.0, 0.0) == "tol"  # tol = 0 still stops centres that do not move
    assert kmeans_stop(3, np.nextafter(1e-3, 1), 1e-3) is None
    assert kmeans_stop(np.int32(1), np.float64(2.0), 1.0) is None


def test_empty_cluster_rule():
    from ssl_wafermap_amd.cluster import kmeans_relocation_plan

    #          row:  0    1    2    3    4    5    6
    labels = np.array([0, 0, 0, 2, 2, 4, 0])
    dist = np.array([1.0, 5.0, 5.0, 9.0, 0.5, 7.0, 2.0])
    counts = np.array([4, 0, 2, 0, 1, 0])
    clusters, rows = kmeans_relocation_plan(counts, labels, dist)
    # descending distance, ascending index: 3 (9.0), 5 (7.0: alone in cluster 4, passed over), 1 (5.0), 2 (5.0), ...
    assert clusters.tolist() == [1, 3, 5] and rows.tolist() == [3, 1, 2]
    # a cluster that has given rows down to one member gives no more
    clusters, rows = kmeans_relocation_plan(np.array([2, 0, 0, 1]), np.array([0, 0, 3]), np.array([3.0, 2.0, 1.0]))
    assert clusters.tolist() == [1] and rows.tolist() == [0]
    # nothing empty: nothing moves
    clusters, rows = kmeans_relocation_plan(np.array([2, 1]), np.array([0, 0, 1]), np.array([3.0, 2.0, 1.0]))
    assert clusters.size == 0 and rows.size == 0
    with pytest.raises(ValueError):
        kmeans_relocation_plan(np.array([1, 0]), np.array([0, 0]), np.array([1.0]))


def test_entry_points_refuse_without_a_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_kmeans_update_workspace_bytes(1000, 52, 7, 3) > 0
    assert lib.wm_kmeans_update_workspace_bytes(1000, 50, 7, 3) == 0  # d % 4
    assert lib.wm_kmeans_update_workspace_bytes(1000, 1028, 7, 3) == 0
    assert lib.wm_kmeans_update_workspace_bytes(1000, 52, 0, 3) == 0
    assert lib.wm_kmeans_update_workspace_bytes(1000, 52, 7, 2000) == 0
    assert lib.wm_kmeans_seed_workspace_bytes(1000, 52, 7, 3) > 0
    assert lib.wm_kmeans_seed_workspace_bytes(5, 52, 7, 3) == 0  # k > n
    assert lib.wm_kmeans_seed_workspace_bytes(1000, 52, 7, 17) == 0
    assert lib.wm_kmeans_update(None, 8, 4, None, None, None, 1, 2, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.wm_kmeans_seed(None, 8, 4, 2, 2, None, None, None, None, None, None, 0, None) == -1
    # the slab count is a function of (n, d, k) alone: R restarts need R times the bytes of one, up to the padding
    one = lib.wm_kmeans_update_workspace_bytes(12449, 512, 50, 1)
    ten = lib.wm_kmeans_update_workspace_bytes(12449, 512, 50, 10)
    assert abs(ten - 10 * one) <= 10 * 5 * 256
