"""CPU checks of the embedding-quality scores (ssl_wafermap_amd.manifold: quality_from_ranks and the argument rules;
the two entry points' argument checks).  No GPU: `ranks64` and `quality64` below restate the definitions of DESIGN.md
("Trustworthiness and continuity") with dense float64 matrices; test_gpu_embedding_quality checks the device path
against them.

The restatement is pinned to sklearn.manifold.trustworthiness on tie-free data, where the arbitrary tie order of
sklearn's argsort cannot show: the penalty sum is an exact integer below 2^53, followed by one multiply and one
subtract, so 1e-12 is generous by four orders."""
import numpy as np
import pytest

from test_cluster_cpu import pairwise64

SHAPES = [(300, 8, 15), (130, 52, 5), (65, 4, 31)]  # (n, d, k)


# ------------------------------------------------------------------------------------------------ float64 restatements


def ranks64(dist):
    """r(i, j) for every pair of a distance matrix [m, n]: 1 + #{ l != skip_i : (dist(i, l), l) < (dist(i, j), j) } with
    skip_i = i when the matrix is square (the row itself is no candidate; its own entry is 0).  int64 [m, n]."""
    m, n = dist.shape
    out = np.zeros((m, n), dtype=np.int64)
    for i in range(m):
        order = np.lexsort((np.arange(n), dist[i]))
        if m == n:
            order = order[order != i]
        out[i, order] = np.arange(1, order.size + 1)
    return out


def neighbours64(dist, k):
    """N_k of every row of a square distance matrix: the first k rows other than the row itself by (distance, index)."""
    n = dist.shape[0]
    out = np.empty((n, k), dtype=np.int64)
    for i in range(n):
        order = np.lexsort((np.arange(n), dist[i]))
        out[i] = order[order != i][:k]
    return out


def quality64(dist_a, dist_b, k, near_a=None, near_b=None):
    """(trustworthiness, continuity, preservation, their per-row vectors) of the definitions from the two spaces'
    distance matrices; near_a / near_b: neighbour lists [n, >= k] to use in place of the matrices' own."""
    n = dist_a.shape[0]
    near_a = neighbours64(dist_a, k) if near_a is None else np.asarray(near_a)[:, :k]
    near_b = neighbours64(dist_b, k) if near_b is None else np.asarray(near_b)[:, :k]
    ra, rb = ranks64(dist_a), ranks64(dist_b)
    rows = np.arange(n)[:, None]
    pen_t = np.maximum(ra[rows, near_b] - k, 0).sum(axis=1)
    pen_c = np.maximum(rb[rows, near_a] - k, 0).sum(axis=1)
    norm = k * (2.0 * n - 3.0 * k - 1.0)
    keep = np.array([np.intersect1d(near_a[i], near_b[i]).size for i in range(n)]) / k
    return {"trustworthiness": 1.0 - float(pen_t.sum()) * (2.0 / (n * norm)), "continuity": 1.0 - float(pen_c.sum()) * (2.0 / (n * norm)),
            "preservation": float(keep.mean()), "trustworthiness_rows": 1.0 - pen_t * (2.0 / norm),
            "continuity_rows": 1.0 - pen_c * (2.0 / norm), "preservation_rows": keep,
            "ranks_a": ra[rows, near_b], "ranks_b": rb[rows, near_a]}


def two_spaces(n, d, seed=0):
    """Tie-free normal rows and a 2-D picture of them that keeps some of the structure."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, d))
    b = a[:, :2] + 0.5 * rng.standard_normal((n, 2))
    return a, b


# ------------------------------------------------------------------------------------------------ against sklearn


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_restatement_against_sklearn(n, d, k):
    from sklearn.manifold import trustworthiness

    a, b = two_spaces(n, d)
    got = quality64(pairwise64(a), pairwise64(b), k)
    assert abs(got["trustworthiness"] - trustworthiness(a, b, n_neighbors=k)) <= 1e-12
    assert abs(got["continuity"] - trustworthiness(b, a, n_neighbors=k)) <= 1e-12
    assert abs(got["trustworthiness_rows"].mean() - got["trustworthiness"]) <= 1e-12
    assert 0.0 < got["preservation"] < 1.0 and 0.0 < got["trustworthiness"] < 1.0 and 0.0 < got["continuity"] < 1.0


def test_restatement_on_worked_cases():
    # five points on a line; the picture swaps the two ends' order of rows 3 and 4 as seen from row 0
    a = np.array([[0.0], [1.0], [2.0], [3.0], [4.5]])
    d = pairwise64(a)
    r = ranks64(d)
    assert r[0].tolist() == [0, 1, 2, 3, 4] and r[2].tolist() == [3, 1, 0, 2, 4]  # row 2: 1 and 3 tie at 1.0, index order
    assert neighbours64(d, 2).tolist() == [[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]]
    same = quality64(d, d, 2)
    assert same["trustworthiness"] == same["continuity"] == same["preservation"] == 1.0
    # duplicates of a row are its neighbours (removed by index, not by distance)
    dup = pairwise64(np.array([[0.0], [0.0], [0.0], [5.0], [6.0]]))
    assert neighbours64(dup, 2).tolist() == [[1, 2], [0, 2], [0, 1], [4, 0], [3, 0]]
    assert ranks64(dup)[1].tolist() == [1, 0, 2, 3, 4]
    # rectangular: no row is skipped
    assert ranks64(np.array([[2.0, 1.0, 1.0]])).tolist() == [[3, 1, 2]]


# ------------------------------------------------------------------------------------------------ the host arithmetic


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_quality_from_ranks_against_the_restatement(n, d, k):
    from ssl_wafermap_amd.manifold import quality_from_ranks

    a, b = two_spaces(n, d, seed=1)
    da, db = pairwise64(a), pairwise64(b)
    ref = quality64(da, db, k)
    got = quality_from_ranks(ref["ranks_a"].astype(np.int32), ref["ranks_b"].astype(np.int32), k)
    assert got.n_neighbors == k
    assert got.trustworthiness == ref["trustworthiness"] and got.continuity == ref["continuity"]
    assert got.neighbor_preservation == ref["preservation"]
    assert np.array_equal(got.trustworthiness_rows, ref["trustworthiness_rows"])
    assert np.array_equal(got.continuity_rows, ref["continuity_rows"])
    assert np.array_equal(got.preservation_rows, ref["preservation_rows"])
    # a sequence of k from the ranks at the largest equals the separate calls (the first k entries of a list are N_k)
    ks = sorted({1, 2, k // 2 + 1, k})
    many = quality_from_ranks(ref["ranks_a"], ref["ranks_b"], ks)
    assert [q.n_neighbors for q in many] == ks
    for q in many:
        one = quality64(da, db, q.n_neighbors)
        assert q.trustworthiness == one["trustworthiness"] and q.continuity == one["continuity"]
        assert q.neighbor_preservation == one["preservation"]
        assert np.array_equal(q.continuity_rows, one["continuity_rows"])
        single = quality_from_ranks(ref["ranks_a"], ref["ranks_b"], q.n_neighbors)
        assert single.trustworthiness == q.trustworthiness and np.array_equal(single.trustworthiness_rows, q.trustworthiness_rows)


def test_argument_rules():
    import torch

    from ssl_wafermap_amd import _lib, manifold

    ranks = np.ones((10, 6), dtype=np.int32)
    for k in (5, 6, 0):  # k >= n / 2 as sklearn refuses it; k < 1
        with pytest.raises(ValueError):
            manifold.quality_from_ranks(ranks, ranks, k)
    with pytest.raises(ValueError):
        manifold.quality_from_ranks(ranks, ranks, [2, 5])
    with pytest.raises(ValueError):
        manifold.quality_from_ranks(np.ones((20, 6), dtype=np.int32), np.ones((20, 6), dtype=np.int32), 7)  # wider than the lists
    with pytest.raises(ValueError):
        manifold.quality_from_ranks(ranks.astype(np.float64), ranks, 2)
    with pytest.raises(ValueError):
        manifold.quality_from_ranks(ranks, ranks[:, :5], 2)
    assert manifold.quality_from_ranks(ranks, ranks, 4).trustworthiness == 1.0
    with pytest.raises(ValueError, match="n_samples / 2"):
        manifold.check_quality_k(128, 64)
    with pytest.raises(ValueError, match="at most 63"):
        manifold.check_quality_k(1000, 64)
    assert manifold.check_quality_k(1000, 63) == 63
    x, y = torch.zeros(10, 4), torch.zeros(10, 2)
    idx = torch.zeros(10, 3, dtype=torch.int32)
    for call in (lambda: manifold.trustworthiness(x, y, 2), lambda: manifold.continuity(x, y, 2),
                 lambda: manifold.embedding_quality(x, y, 2), lambda: manifold.pair_distances(x, x, idx),
                 lambda: manifold.neighbor_ranks(x, x, idx)):
        with pytest.raises(_lib.WaferHipError):  # a CPU tensor: there is no fallback
            call()


def test_wrappers_validate_their_lists(monkeypatch):
    import torch

    from ssl_wafermap_amd import cluster, manifold

    monkeypatch.setattr(cluster, "require_gpu", lambda *t: None)  # (the checks behind the device check)
    monkeypatch.setattr(manifold, "require_gpu", lambda *t: None)
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="features"):
        manifold.pair_distances(x, torch.zeros(10, 8), torch.zeros(10, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="idx"):
        manifold.pair_distances(x, x, torch.zeros(9, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="idx"):
        manifold.neighbor_ranks(x, x, torch.zeros(10, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="k "):
        manifold.neighbor_ranks(x, x, torch.zeros(10, 65, dtype=torch.int32))
    with pytest.raises(ValueError, match="exclude_self"):
        manifold.neighbor_ranks(x[:4], x, torch.zeros(4, 3, dtype=torch.int32), exclude_self=True)
    with pytest.raises(ValueError, match="unknown metric"):
        manifold.neighbor_ranks(x, x, torch.zeros(10, 3, dtype=torch.int32), metric="cosine")
    with pytest.raises(ValueError, match="n_samples / 2"):
        manifold.trustworthiness(x, x, 5)
    with pytest.raises(ValueError, match="rows"):
        manifold.embedding_quality(x, torch.zeros(9, 2), 2)


# ------------------------------------------------------------------------------------------------ the entry points


def test_entry_points_validate_before_any_launch():
    """The pointers are stand-ins (16-byte aligned numbers): every call here returns before it would touch them."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    a = 4096
    need = lib.wm_rank_query_workspace_bytes(9, 650, 8, 15)  # 1 row tile, 11 column tiles: 11 slices of [9][15] counts
    assert need >= 11 * 9 * 15 * 4

    def rank(xq=a, m=9, x=a, n=650, d=8, metric=0, t=a, tj=a, skip=a, k=15, count=a, ws=a, ws_bytes=need):
        return lib.wm_rank_query(xq, m, x, n, d, metric, t, tj, skip, k, count, ws, ws_bytes, None)

    assert rank(xq=None) == -1 and rank(x=None) == -1 and rank(t=None) == -1 and rank(tj=None) == -1
    assert rank(skip=None) == -1 and rank(count=None) == -1 and rank(ws=None) == -1
    assert rank(m=0) == -1 and rank(n=0) == -1 and rank(d=0) == -1 and rank(k=0) == -1
    assert rank(k=65) == -2 and rank(m=(1 << 24) + 1) == -2 and rank(n=(1 << 24) + 1) == -2
    assert rank(d=6) == -2 and rank(d=1028) == -2 and rank(metric=2) == -2 and rank(metric=-1) == -2
    assert rank(xq=a + 4) == -4 and rank(x=a + 8) == -4 and rank(ws=a + 4) == -4
    assert rank(ws_bytes=16) == -3
    assert rank(k=65, xq=a + 4, ws_bytes=0) == -2 and rank(xq=a + 4, ws_bytes=0) == -4  # the order of the checks

    def pair(xq=a, m=9, x=a, n=650, d=8, metric=0, idx=a, k=15, out=a):
        return lib.wm_pair_dist(xq, m, x, n, d, metric, idx, k, out, None)

    assert pair(xq=None) == -1 and pair(x=None) == -1 and pair(idx=None) == -1 and pair(out=None) == -1
    assert pair(m=0) == -1 and pair(n=0) == -1 and pair(d=0) == -1 and pair(k=0) == -1
    assert pair(k=65) == -2 and pair(d=6) == -2 and pair(d=1028) == -2 and pair(metric=2) == -2 and pair(m=(1 << 24) + 1) == -2
    assert pair(xq=a + 4) == -4 and pair(x=a + 8) == -4

    size = lib.wm_rank_query_workspace_bytes
    assert size(0, 650, 8, 15) == 0 and size(9, 0, 8, 15) == 0 and size(9, 650, 0, 15) == 0 and size(9, 650, 8, 0) == 0
    assert size(9, 650, 8, 65) == 0 and size((1 << 24) + 1, 650, 8, 15) == 0 and size(9, (1 << 24) + 1, 8, 15) == 0
    assert size(9, 650, 8, 64) > 0 and size(1 << 24, 1 << 24, 1024, 64) > 0
    assert size(70000, 650, 8, 15) == 256  # 1094 row tiles: one slice, which stores straight into the output
