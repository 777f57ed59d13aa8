"""CPU checks of the DBCV cluster validity (ssl_wafermap_amd.cluster: validity_from_parts, relative_validity,
validity_index's refusals, the three entry points' argument checks; scripts/embedding_clustering_amd.py's column list).
No GPU: `brute_dbcv` below restates the definition of DESIGN.md ("DBCV") in float64 with dense matrices and Kruskal
under the total order (w, min(i, j), max(i, j)); test_gpu_dbcv checks the device path against it."""
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest

from test_cluster_cpu import pairwise64

ROOT = Path(__file__).resolve().parent.parent

# ------------------------------------------------------------------------------------------------ float64 restatements


def allpoints_core64(dist, p):
    """The all-points core distance of every row of one cluster from its float64 distance matrix, in the log domain:
    exp(-(logsumexp_j(-p log dist_ij) - log(n_c - 1)) / p) over dist_ij > 0; 0 for a row without a positive distance."""
    n = dist.shape[0]
    out = np.zeros(n)
    for i in range(n):
        pos = dist[i][dist[i] > 0]
        if pos.size:
            out[i] = math.exp(-(np.logaddexp.reduce(-p * np.log(pos)) - math.log(n - 1)) / p)
    return out


def kruskal(w):
    """Edges (i, j, w_ij), i < j, of the minimum spanning tree of the dense symmetric matrix w under (w, i, j)."""
    n = w.shape[0]
    iu, ju = np.triu_indices(n, 1)
    order = np.lexsort((ju, iu, w[iu, ju]))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    edges = []
    for e in order:
        ra, rb = find(int(iu[e])), find(int(ju[e]))
        if ra != rb:
            parent[ra] = rb
            edges.append((int(iu[e]), int(ju[e]), float(w[iu[e], ju[e]])))
    return edges


def cross_dist64(a, b, metric):
    a, b = a.astype(np.float64), b.astype(np.float64)
    if metric == "euclidean":
        return np.stack([np.sqrt(((b - row) ** 2).sum(axis=1)) for row in a])
    return np.stack([np.abs(b - row).sum(axis=1) for row in a])


def brute_dbcv(x, labels, metric="euclidean", p=None, forests=None):
    """DBCV of DESIGN.md, straight line, float64.  Clusters of fewer than two rows take no part.  `forests`: per kept
    cluster a list of (i, j) tree edges in the cluster's own row numbering to use in place of Kruskal's (their weights
    are recomputed here).  Returns a dict: score, v, sizes, n_total, sparseness, sep, cores, edges, internal, clusters."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    p = float(x.shape[1] if p is None else p)
    clusters = [c for c in sorted(set(labels[labels >= 0].tolist())) if (labels == c).sum() >= 2]
    members = [np.flatnonzero(labels == c) for c in clusters]
    cores, trees, internal, sparseness = [], [], [], []
    for k, rows in enumerate(members):
        dist = pairwise64(x[rows], metric)
        core = allpoints_core64(dist, p)
        mr = np.maximum(np.maximum(core[:, None], core[None, :]), dist)
        edges = kruskal(mr) if forests is None else [(int(i), int(j), float(mr[i, j])) for i, j in forests[k]]
        degree = np.zeros(rows.size, dtype=int)
        for i, j, _ in edges:
            degree[i] += 1
            degree[j] += 1
        inner = np.flatnonzero(degree > 1)
        if inner.size == 0:
            inner = np.array([0])
        inner_edges = [w for i, j, w in edges if degree[i] > 1 and degree[j] > 1]
        if not inner_edges:
            inner_edges = [w for _, _, w in edges]
        cores.append(core)
        trees.append(edges)
        internal.append(inner)
        sparseness.append(max(inner_edges))
    c = len(clusters)
    sep = np.full((c, c), np.inf)
    for a in range(c):
        for b in range(c):
            if a != b:
                da = cross_dist64(x[members[a][internal[a]]], x[members[b][internal[b]]], metric)
                sep[a, b] = np.maximum(np.maximum(cores[a][internal[a]][:, None], cores[b][internal[b]][None, :]), da).min()
    n_total = labels.shape[0]
    score, v = 0.0, []
    for a in range(c):
        s_a = min(sep[a, b] for b in range(c) if b != a)
        top = max(s_a, sparseness[a])
        v.append((s_a - sparseness[a]) / top if top > 0 else 0.0)
        score += members[a].size / float(n_total) * v[-1]
    return {"score": score, "v": np.array(v), "sizes": np.array([m.size for m in members]), "n_total": n_total,
            "sparseness": np.array(sparseness), "sep": sep, "cores": cores, "edges": trees, "internal": internal,
            "clusters": clusters, "members": members}


def relative_validity64(mst, labels):
    """The edge walk of DESIGN.md ("relative_validity_"), one edge at a time."""
    labels = [int(t) for t in labels]
    n = len(labels)
    n_clusters = max(labels) + 1 if n else 0
    if n_clusters <= 0:
        return 0.0
    dsc, dspc = [0.0] * n_clusters, [math.inf] * n_clusters
    max_w, min_outlier = 0.0, math.inf
    for u, v, w in mst:
        a, b = labels[int(u)], labels[int(v)]
        max_w = max(max_w, w)
        if a < 0 and b < 0:
            continue
        if a < 0 or b < 0:
            min_outlier = min(min_outlier, w)
            continue
        if a == b:
            dsc[a] = max(dsc[a], w)
        else:
            dspc[a] = min(dspc[a], w)
            dspc[b] = min(dspc[b], w)
    if math.isinf(min_outlier):
        min_outlier = max_w
    total = 0.0
    for c in range(n_clusters):
        if math.isinf(dspc[c]):
            dspc[c] = 2.0 * (max_w if n_clusters > 1 else min_outlier)
        top = max(dspc[c], dsc[c])
        v_c = (dspc[c] - dsc[c]) / top if top > 0 else 0.0
        total += labels.count(c) * v_c
    return total / n


# ------------------------------------------------------------------------------------------------ relative validity

# A spanning tree built by hand on the 13 points of test_hdbscan_predict_cpu's tree (weights = 1 / lambda there):
# A = {2, 3, 4, 5}, B1 = {7, 8, 9}, B2 = {10, 11, 12}; 0, 1 and 6 fall out as noise.  A hangs on the rest through the
# noise point 6 only, so no edge joins it to another cluster.
HAND_MST = np.array([(4, 5, 0.5), (2, 4, 1.0), (3, 4, 1.0), (8, 9, 0.25), (7, 8, 0.5), (11, 12, 0.2), (10, 11, 0.8),
                     (7, 10, 1.0), (6, 7, 1.25), (5, 6, 2.0), (0, 2, 4.0), (0, 1, 4.0)])
HAND_LABELS = np.array([-1, -1, 0, 0, 0, 0, -1, 1, 1, 1, 2, 2, 2])


def labelled(**groups):
    lab = np.full(13, -1)
    for c, rows in groups.items():
        lab[list(rows)] = int(c[1:])
    return lab


RV_CASES = {
    "island": HAND_LABELS,  # A's DSPC stays infinite: 2 * max_w
    "no_noise": labelled(c0=range(0, 6), c1=range(6, 10), c2=range(10, 13)),
    "noise_edges_only": labelled(c0=[2], c1=[12]),  # every edge has a noise end
    "one_cluster": labelled(c0=[2, 3, 4, 5]),  # DSPC = 2 * min_outlier
    "one_cluster_no_noise": labelled(c0=range(13)),  # min_outlier falls back on max_w
    "all_noise": np.full(13, -1),
    "empty_id": labelled(c0=[2, 3, 4, 5], c2=[10, 11, 12]),  # label 1 has no row
}


@pytest.mark.parametrize("case", sorted(RV_CASES))
def test_relative_validity_against_the_edge_walk(case):
    from ssl_wafermap_amd.cluster import relative_validity

    lab = RV_CASES[case]
    got = relative_validity(HAND_MST, lab)
    assert isinstance(got, float) and got == relative_validity64(HAND_MST.tolist(), lab)
    assert -1.0 <= got <= 1.0
    shuffled = HAND_MST[np.random.default_rng(3).permutation(12)]  # the edge order does not matter (max / min only)
    assert relative_validity(shuffled, lab) == got


def test_relative_validity_worked_values():
    from ssl_wafermap_amd.cluster import relative_validity

    # island: A: DSC 1, DSPC 2 * 4 = 8; B1: DSC 0.5, DSPC 1; B2: DSC 0.8, DSPC 1
    want = (4 * (8 - 1) / 8 + 3 * (1 - 0.5) / 1 + 3 * (1 - 0.8) / 1) / 13
    assert relative_validity(HAND_MST, RV_CASES["island"]) == pytest.approx(want, rel=1e-15)
    # one cluster: DSC 1, min_outlier = min(2, 4) = 2, DSPC = 4
    assert relative_validity(HAND_MST, RV_CASES["one_cluster"]) == pytest.approx(4 * 0.75 / 13, rel=1e-15)
    assert relative_validity(HAND_MST, RV_CASES["one_cluster_no_noise"]) == pytest.approx((8 - 4) / 8, rel=1e-15)
    assert relative_validity(HAND_MST, RV_CASES["noise_edges_only"]) == pytest.approx(2 / 13, rel=1e-15)
    assert relative_validity(HAND_MST, RV_CASES["all_noise"]) == 0.0
    assert relative_validity(np.zeros((0, 3)), np.array([0])) == 0.0  # one row: no edge, DSC = DSPC = 0
    with pytest.raises(ValueError):
        relative_validity(HAND_MST[:5], HAND_LABELS)


def test_relative_validity_property_follows_fit_and_refit():
    """Host only: the model's tree comes from numpy (as test_hdbscan_predict_cpu.host_model builds it)."""
    from sklearn.datasets import make_blobs

    from test_cluster_cpu import prim_mst
    from ssl_wafermap_amd import cluster

    x, _ = make_blobs(300, 4, centers=4, cluster_std=1.0, random_state=5)
    model = cluster.HDBSCAN(min_cluster_size=10, min_samples=5)
    assert model.relative_validity_ is None
    u, v, w = prim_mst(x, 5)
    model._n, model._k = 300, 5
    model.minimum_spanning_tree_ = np.stack([u.astype(np.float64), v.astype(np.float64), w], axis=1)
    model._label()
    first = model.relative_validity_
    assert first == relative_validity64(model.minimum_spanning_tree_.tolist(), model.labels_) and -1 <= first <= 1
    labels = model.labels_.copy()
    model.refit(min_cluster_size=120)
    assert not np.array_equal(labels, model.labels_)
    assert model.relative_validity_ == relative_validity64(model.minimum_spanning_tree_.tolist(), model.labels_) != first


# ------------------------------------------------------------------------------------------------ validity from parts


def test_validity_from_parts_worked_values():
    from ssl_wafermap_amd.cluster import validity_from_parts

    score, v = validity_from_parts([3, 2], 6, [1.0, 0.0], [[9.0, 2.0], [2.0, 9.0]])  # (the diagonal is ignored)
    assert v.tolist() == [0.5, 1.0] and score == 3 / 6 * 0.5 + 2 / 6 * 1.0
    score, v = validity_from_parts([2, 2, 2], 6, [0.0, 4.0, 1.0], [[0, 0.0, 3.0], [0.0, 0, 2.0], [3.0, 2.0, 0]])
    assert v.tolist() == [0.0, -1.0, 0.5] and score == 2 / 6 * 0.0 + 2 / 6 * -1.0 + 2 / 6 * 0.5  # both zero: 0
    for bad in (([3], 3, [1.0], [[0.0]]), ([3, 2], 4, [1.0, 1.0], np.ones((2, 2))), ([3, 2], 5, [1.0], np.ones((2, 2))),
                ([3, 2], 5, [1.0, -1.0], np.ones((2, 2))), ([3, 2], 5, [1.0, 1.0], np.ones((2, 3)))):
        with pytest.raises(ValueError):
            validity_from_parts(*bad)


def small_inputs():
    """(name, x, labels, metric, p): at most 40 rows; blobs with noise, a singleton cluster and an absent id; two-row
    clusters; exact duplicates inside a cluster; a cluster of identical rows; a large power."""
    rng = np.random.default_rng(7)
    blobs = np.concatenate([rng.standard_normal((12, 3)), rng.standard_normal((15, 3)) + 8, rng.standard_normal((9, 3)) - 8])
    lab = np.repeat([0, 1, 3], [12, 15, 9])
    noisy = lab.copy()
    noisy[[0, 13, 30]] = -1
    noisy[5] = 7  # a singleton cluster
    dup = blobs.copy()
    dup[3] = dup[1]
    dup[14] = dup[12]
    same = blobs.copy()
    same[27:] = same[27]
    pairs = np.concatenate([rng.standard_normal((2, 5)), rng.standard_normal((2, 5)) + 6, rng.standard_normal((3, 5)) - 6])
    return [("blobs", blobs, lab, "euclidean", None), ("noisy", blobs, noisy, "manhattan", None),
            ("duplicates", dup, lab, "euclidean", None), ("identical", same, lab, "euclidean", None),
            ("pairs", pairs, np.repeat([0, 1, 2], [2, 2, 3]), "euclidean", None), ("power", blobs, noisy, "euclidean", 512.0)]


@pytest.mark.parametrize("case", small_inputs(), ids=lambda c: c[0])
def test_brute_force_parts_reproduce_its_score(case):
    from ssl_wafermap_amd.cluster import validity_from_parts

    _, x, lab, metric, p = case
    ref = brute_dbcv(x, lab, metric, p)
    score, v = validity_from_parts(ref["sizes"], ref["n_total"], ref["sparseness"], ref["sep"])
    assert score == ref["score"] and np.array_equal(v, ref["v"]) and -1.0 <= score <= 1.0
    assert all(len(e) == m.size - 1 for e, m in zip(ref["edges"], ref["members"]))


def test_brute_force_on_worked_cases():
    # two rows per cluster: the all-points core of a row is its one distance (the mean over n_c - 1 = 1 term)
    x = np.array([[0.0], [1.0], [10.0], [12.0]])
    ref = brute_dbcv(x, [0, 0, 1, 1], p=3.0)
    assert np.allclose(ref["cores"][0], [1.0, 1.0], rtol=1e-15) and np.allclose(ref["cores"][1], [2.0, 2.0], rtol=1e-15)
    assert np.allclose(ref["sparseness"], [1.0, 2.0], rtol=1e-15)
    assert ref["sep"][0, 1] == ref["sep"][1, 0] == 10.0  # first rows only: |0 - 10|
    assert ref["score"] == pytest.approx(0.5 * 9 / 10 + 0.5 * 8 / 10, rel=1e-14)
    # a cluster of identical rows: every core distance and the sparseness are 0
    ref = brute_dbcv(np.array([[0.0], [0.0], [0.0], [5.0], [6.0]]), [0, 0, 0, 1, 1])
    assert (ref["cores"][0] == 0).all() and ref["sparseness"][0] == 0 and ref["v"][0] == 1.0
    # the log form where the plain float64 power leaves the range
    dist = np.array([[0.0, 1e-3, 1e3], [1e-3, 0.0, 1e3], [1e3, 1e3, 0.0]])
    got = allpoints_core64(dist, 1024.0)
    with np.errstate(over="ignore", divide="ignore"):
        assert np.isinf((dist[0][1:] ** -1024.0).sum()) and (dist[2][:2] ** -1024.0).sum() == 0.0
    assert got[0] == pytest.approx(1e-3 * 2 ** (1 / 1024), rel=1e-12) and got[2] == pytest.approx(1e3, rel=1e-12)


# ------------------------------------------------------------------------------------------------ refusals


def test_validity_index_refusals():
    import torch

    from ssl_wafermap_amd import _lib, cluster

    x = torch.zeros(6, 4)
    good = np.array([0, 0, 1, 1, -1, 2])
    for lab in (np.array([0, 0, 0, 0, -1, -1]), np.array([0, 0, 1, 2, 3, -1]), np.full(6, -1)):  # < 2 usable clusters
        with pytest.raises(ValueError, match="two clusters"):
            cluster.validity_index(x, lab)
    with pytest.raises(ValueError):
        cluster.validity_index(x, good[:5])
    with pytest.raises(ValueError):
        cluster.validity_index(x, good.astype(np.float64))
    for d in (0, -1.0, math.inf):
        with pytest.raises(ValueError, match="d must"):
            cluster.validity_index(x, good, d=d)
        with pytest.raises(ValueError, match="d must"):
            cluster.allpoints_core_distances(x, good, d=d)
    with pytest.raises(NotImplementedError, match="mst_raw_dist"):
        cluster.validity_index(x, good, mst_raw_dist=True)
    with pytest.raises(NotImplementedError, match="canberra"):
        cluster.validity_index(x, good, metric="canberra")
    with pytest.raises(NotImplementedError, match="canberra"):
        cluster.allpoints_core_distances(x, good, metric="canberra")
    with pytest.raises(ValueError):
        cluster.validity_index(x, good, metric="cosine")
    for call in (lambda: cluster.validity_index(x, good), lambda: cluster.allpoints_core_distances(x, good),
                 lambda: cluster.grouped_min_outgoing_edges(x, torch.zeros(6), torch.zeros(6, dtype=torch.int32), good // 2 + 1, 3),
                 lambda: cluster.group_min_mreach(x, torch.zeros(6), x, torch.zeros(6), np.zeros(6, dtype=np.int64), 1)):
        with pytest.raises(_lib.WaferHipError):  # a CPU tensor: there is no fallback
            call()


def test_wrappers_validate_their_groups(monkeypatch):
    import torch

    from ssl_wafermap_amd import cluster

    monkeypatch.setattr(cluster, "require_gpu", lambda *t: None)  # (the checks behind the device check)
    x, core, comp = torch.zeros(6, 4), torch.zeros(6), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="group"):
        cluster.grouped_min_outgoing_edges(x, core, comp, torch.zeros(5, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="n_groups"):
        cluster.grouped_min_outgoing_edges(x, core, comp, torch.full((6,), 2), 2)
    with pytest.raises(ValueError, match="core"):
        cluster.grouped_min_outgoing_edges(x, core.double(), comp, torch.zeros(6, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="features"):
        cluster.group_min_mreach(x, core, torch.zeros(6, 8), core, torch.zeros(6, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="core_q"):
        cluster.group_min_mreach(x, core[:5], x, core, torch.zeros(6, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="group"):
        cluster.group_min_mreach(x, core, x, core, torch.zeros(6), 1)  # float ids
    with pytest.raises(ValueError, match="n_groups"):
        cluster.group_min_mreach(x, core, x, core, torch.zeros(6, dtype=torch.int32), 0)


def test_entry_points_validate_before_any_launch():
    """The pointers are stand-ins (16-byte aligned numbers): every call here returns before it would touch them."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    a = 4096
    need_c = lib.wm_allpoints_core_workspace_bytes(300, 8, 3)
    need_e = lib.wm_mreach_min_edge_grouped_workspace_bytes(300, 8, 3)
    need_g = lib.wm_group_min_mreach_workspace_bytes(9, 65, 8, 3)
    assert need_c >= 300 * 16 + 3 * 8 and need_e >= 300 * 8 + 3 * 8 and need_g == lib.wm_group_min_dist_workspace_bytes(9, 65, 8, 3)

    def core(x=a, group=a, n=300, d=8, metric=0, g=3, p=8.0, out=a, ws=a, ws_bytes=need_c):
        return lib.wm_allpoints_core(x, group, n, d, metric, g, p, out, ws, ws_bytes, None)

    assert core(x=None) == -1 and core(group=None) == -1 and core(out=None) == -1 and core(ws=None) == -1
    assert core(n=0) == -1 and core(d=0) == -1 and core(g=0) == -1 and core(p=0.0) == -1 and core(p=-2.0) == -1
    assert core(p=math.inf) == -1 and core(p=math.nan) == -1
    assert core(n=(1 << 24) + 1) == -2 and core(d=6) == -2 and core(d=1028) == -2 and core(metric=2) == -2
    assert core(ws_bytes=16) == -3

    def edge(x=a, cr=a, comp=a, group=a, n=300, d=8, metric=0, g=3, out_w=a, out_j=a, ws=a, ws_bytes=need_e):
        return lib.wm_mreach_min_edge_grouped(x, cr, comp, group, n, d, metric, g, out_w, out_j, ws, ws_bytes, None)

    assert edge(x=None) == -1 and edge(cr=None) == -1 and edge(comp=None) == -1 and edge(group=None) == -1
    assert edge(out_w=None) == -1 and edge(out_j=None) == -1 and edge(ws=None) == -1
    assert edge(n=0) == -1 and edge(d=0) == -1 and edge(g=0) == -1
    assert edge(n=(1 << 24) + 1) == -2 and edge(d=6) == -2 and edge(metric=-1) == -2
    assert edge(ws_bytes=16) == -3

    def gmin(xq=a, cq=a, m=9, xe=a, cr=a, group=a, e=65, d=8, metric=0, g=3, out_w=a, out_j=a, ws=a, ws_bytes=need_g):
        return lib.wm_group_min_mreach(xq, cq, m, xe, cr, group, e, d, metric, g, out_w, out_j, ws, ws_bytes, None)

    assert gmin(xq=None) == -1 and gmin(cq=None) == -1 and gmin(xe=None) == -1 and gmin(cr=None) == -1
    assert gmin(group=None) == -1 and gmin(out_w=None) == -1 and gmin(out_j=None) == -1 and gmin(ws=None) == -1
    assert gmin(m=0) == -1 and gmin(e=0) == -1 and gmin(d=0) == -1 and gmin(g=0) == -1
    assert gmin(m=(1 << 24) + 1) == -2 and gmin(e=(1 << 24) + 1) == -2 and gmin(d=6) == -2 and gmin(metric=2) == -2
    assert gmin(ws_bytes=16) == -3

    for size in (lib.wm_allpoints_core_workspace_bytes, lib.wm_mreach_min_edge_grouped_workspace_bytes):
        assert size(0, 8, 3) == 0 and size(300, 0, 3) == 0 and size(300, 8, 0) == 0 and size((1 << 24) + 1, 8, 3) == 0
        assert size(300, 8, 3) > 0 and size(1 << 24, 1024, 1 << 24) > 0
    size = lib.wm_group_min_mreach_workspace_bytes
    assert size(0, 65, 8, 3) == 0 and size(9, 0, 8, 3) == 0 and size(9, 65, 0, 3) == 0 and size(9, 65, 8, 0) == 0
    assert size((1 << 24) + 1, 65, 8, 3) == 0 and size(9, (1 << 24) + 1, 8, 3) == 0 and size(9, 65, 8, 3) > 0


# ------------------------------------------------------------------------------------------------ the script


def test_script_columns_without_the_flag():
    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", ROOT / "scripts" / "embedding_clustering_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.COLUMNS == ["trial", "metric", "min_samples", "min_cluster_size", "cluster_selection_epsilon", "n_clusters",
                           "n_noise", "homogeneity", "silhouette", "calinski_harabasz", "davies_bouldin"]
    assert mod.OBJECTIVES == [("silhouette", 1), ("calinski_harabasz", 1), ("homogeneity", 1), ("davies_bouldin", -1),
                              ("n_noise", -1)]
    assert mod.VALIDITY_COLUMNS == ["relative_validity", "dbcv"] and mod.VALIDITY_OBJECTIVES == [("dbcv", 1)]
    rows = [{"silhouette": 0.5, "calinski_harabasz": 10.0, "homogeneity": 0.5, "davies_bouldin": 1.0, "n_noise": 3, "dbcv": 0.1},
            {"silhouette": 0.5, "calinski_harabasz": 10.0, "homogeneity": 0.5, "davies_bouldin": 1.0, "n_noise": 3, "dbcv": 0.4}]
    assert mod.pareto_rows(rows) == [0, 1]  # equal on the old objectives: neither dominates
    assert mod.pareto_rows(rows, mod.OBJECTIVES + mod.VALIDITY_OBJECTIVES) == [1]
