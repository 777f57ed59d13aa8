"""CPU checks of the UMAP host code (ssl_wafermap_amd.manifold): the curve fit of (a, b), the sampling schedule, the
negative-sample hash, argument validation and the refusals.  No GPU: nothing here launches a kernel.  The float64
reference of the whole algorithm that the GPU tests compare against (tests/test_gpu_umap.py) lives here too, so that
its own pieces are checked without a GPU."""
import numpy as np
import pytest

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ float64 reference


def ref_mix(x):
    """lowbias32 on numpy uint64 arrays holding 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def ref_sampled(q, ep):
    q = np.asarray(q, dtype=np.uint64)
    return ((np.uint64(ep + 1) * q) >> np.uint64(16)) > ((np.uint64(ep) * q) >> np.uint64(16))


def ref_negatives(seed, ep, entries, rate, n):
    """[len(entries), rate] negative-sample vertices of the given CSR entry positions."""
    key0 = ref_mix(np.uint64((seed ^ (ep * 0x9E3779B9)) & M32))
    key = ref_mix((key0 + np.asarray(entries, dtype=np.uint64)) & np.uint64(M32))
    h = ref_mix((key[:, None] + np.arange(rate, dtype=np.uint64)[None, :]) & np.uint64(M32))
    return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def ref_smooth_knn(dist, idx):
    """umap-learn's smooth_knn_dist / compute_membership_strengths (local_connectivity = 1) in float64 on a sorted
    kNN graph: (rho, sigma, weights, floor) with floor the value sigma may not fall below."""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    target = np.log2(k)
    rho, sigma, floor = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        pos = dist[i][dist[i] > 0]
        rho[i] = pos[0] if pos.size else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            d = dist[i, 1:] - rho[i]
            psum = np.where(d > 0, np.exp(-np.maximum(d, 0) / mid), 1.0).sum()
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2
        floor[i] = 1e-3 * (dist[i].mean() if rho[i] > 0 else dist.mean())
        sigma[i] = max(mid, floor[i])
    return rho, sigma, ref_weights(dist, idx, rho, sigma), floor


def ref_weights(dist, idx, rho, sigma):
    d = np.asarray(dist, dtype=np.float64) - np.asarray(rho, dtype=np.float64)[:, None]
    with np.errstate(under="ignore"):
        w = np.where(d > 0, np.exp(-np.maximum(d, 0) / np.asarray(sigma, dtype=np.float64)[:, None]), 1.0)
    return np.where(np.asarray(idx) == np.arange(d.shape[0])[:, None], 0.0, w)


def ref_union(idx, w):
    """scipy's P + P^T - P o P^T in float64 (CSR, sorted columns, explicit zeros dropped)."""
    from scipy.sparse import csr_matrix

    n, k = idx.shape
    p = csr_matrix((np.asarray(w, dtype=np.float64).ravel(), (np.repeat(np.arange(n), k), np.asarray(idx).ravel())), shape=(n, n))
    p.eliminate_zeros()
    g = p + p.T - p.multiply(p.T)
    g = csr_matrix(g)
    g.eliminate_zeros()
    g.sort_indices()
    return g


def ref_rates(data):
    data = np.asarray(data, dtype=np.float64)
    return np.rint(65536.0 * data / data.max()).astype(np.int64)


def ref_layout_epoch(y, indptr, indices, q, a, b, gamma, alpha, seed, ep, rate):
    """One epoch of the deterministic gather in float64 from the positions y: (y', sum over the vertex's terms of
    |term| per component, number of sampled entries per vertex, number of term components that clip).  `alpha` is
    the epoch's step (the caller passes the float32 value the kernel uses)."""
    y = np.asarray(y, dtype=np.float64)
    n, dim = y.shape
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    head = np.repeat(np.arange(n), np.diff(indptr))
    e = np.flatnonzero(ref_sampled(q, ep))
    total, mag = np.zeros((n, dim)), np.zeros((n, dim))
    clipped = 0
    if e.size:
        i, j = head[e], indices[e]
        d = y[i] - y[j]
        r = (d * d).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(r > 0, -2.0 * a * b * r ** (b - 1.0) / (a * r ** b + 1.0), 0.0)
        clipped += int((np.abs(coef[:, None] * d) > 4.0).sum())
        g = 2.0 * np.clip(coef[:, None] * d, -4.0, 4.0)
        np.add.at(total, i, g)
        np.add.at(mag, i, np.abs(g))
        neg = ref_negatives(seed, ep, e, rate, n)
        for t in range(rate):
            k = neg[:, t]
            d = y[i] - y[k]
            r = (d * d).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where((r > 0) & (k != i), 2.0 * gamma * b / ((0.001 + r) * (a * r ** b + 1.0)), 0.0)
            clipped += int((np.abs(coef[:, None] * d) > 4.0).sum())
            g = np.clip(coef[:, None] * d, -4.0, 4.0)
            np.add.at(total, i, g)
            np.add.at(mag, i, np.abs(g))
    hits = np.bincount(head[e], minlength=n) if e.size else np.zeros(n, dtype=np.int64)
    return y + float(alpha) * total, mag, hits, clipped


def ref_alpha(learning_rate, ep, n_epochs):
    return float(np.float32(learning_rate * (1.0 - ep / n_epochs)))


def ref_knn(x, k):
    """(dist, idx) float64 / int64 [n, k] of the exact Euclidean kNN graph, ordered by (distance, index), from the Gram
    form in float64 (no n x n x d broadcast), the self-distance set to exactly 0."""
    x = np.asarray(x, dtype=np.float64)
    sq = (x * x).sum(axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)
    np.fill_diagonal(d2, 0.0)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def ref_random_init(n, dim, seed):
    """init="random" of manifold.UMAP: uniform in [-10, 10], every dimension rescaled to [0, 10], as float32."""
    y = np.random.default_rng(seed).uniform(-10.0, 10.0, (n, dim))
    lo, hi = y.min(axis=0), y.max(axis=0)
    return (10.0 * (y - lo) / (hi - lo)).astype(np.float32)


def ref_fit(x, k, dim, a, b, n_epochs, seed, rate=5, gamma=1.0, learning_rate=1.0):
    """The whole algorithm in float64 with init="random": kNN graph, fuzzy simplicial set, `n_epochs` layout epochs."""
    dist, idx = ref_knn(x, k)
    _, _, w, _ = ref_smooth_knn(dist, idx)
    g = ref_union(idx, w)
    q = ref_rates(g.data)
    y = ref_random_init(x.shape[0], dim, seed).astype(np.float64)
    for ep in range(n_epochs):
        y = ref_layout_epoch(y, g.indptr, g.indices, q, a, b, gamma, ref_alpha(learning_rate, ep, n_epochs), seed, ep, rate)[0]
    return y


# ------------------------------------------------------------------------------------------------ tests


def test_find_ab_params():
    from ssl_wafermap_amd.manifold import find_ab_params

    a, b = find_ab_params(1.0, 0.1)
    assert abs(a - 1.57694) <= 1e-4 and abs(b - 0.89506) <= 1e-4
    a, b = find_ab_params(1.0, 0.0)
    assert abs(a - 1.93281) <= 1e-4 and abs(b - 0.79049) <= 1e-4


@pytest.mark.parametrize("epochs", [1, 200, 500])
@pytest.mark.parametrize("q", [65536, 32768, 21845, 1, 0])
def test_schedule_samples_an_entry_floor_of_its_rate(q, epochs):
    from ssl_wafermap_amd.manifold import is_sampled

    count = sum(is_sampled(q, ep) for ep in range(epochs))
    assert count == (epochs * q) >> 16
    # the GPU tests' reference takes the same decisions
    assert [bool(ref_sampled(q, ep)) for ep in range(epochs)] == [is_sampled(q, ep) for ep in range(epochs)]


def test_hash_against_hand_computed_values():
    from ssl_wafermap_amd.manifold import mix32, negative_index

    # 1 -> ^>>16: 1; * 0x7feb352d: 0x7feb352d; ^>>15: 0x7febcafb; * 0x846ca68b mod 2^32; ^>>16
    assert mix32(0) == 0
    assert mix32(1) == 0x688990C0
    assert mix32(0x9E3779B9) == 0x01FCE552
    assert mix32(0xFFFFFFFF) == 0x6768824A
    assert [int(v) for v in ref_mix([0, 1, 0x9E3779B9, 0xFFFFFFFF])] == [0, 0x688990C0, 0x01FCE552, 0x6768824A]
    # seed = 0, epoch = 0, entry = 0, t = 0: every mix sees 0
    assert negative_index(0, 0, 0, 0, 1000) == 0
    assert negative_index(42, 7, 123, 3, 172950) == 153715
    assert negative_index(0xFFFFFFFF, 499, 2 ** 22, 4, 65) == 41  # (epoch * 0x9e3779b9 and the sums wrap)
    assert int(ref_negatives(42, 7, [123], 4, 172950)[0, 3]) == 153715
    assert int(ref_negatives(0xFFFFFFFF, 499, [2 ** 22], 5, 65)[0, 4]) == 41
    draws = ref_negatives(3, 11, np.arange(4096), 5, 65)
    assert draws.min() == 0 and draws.max() == 64  # the multiply-shift covers [0, n) and nothing else


def test_reference_epoch_moves_a_pair_as_the_formulas_say():
    """Two vertices one unit apart, both directions sampled, no negatives: y_0' = y_0 + alpha * 2 att."""
    a, b = 1.5, 0.9
    y = np.array([[0.0, 0.0], [1.0, 0.0]])
    out, mag, hits, _ = ref_layout_epoch(y, [0, 1, 2], [1, 0], [65536, 65536], a, b, 1.0, 0.5, 0, 0, 0)
    att = -2.0 * a * b / (a + 1.0)  # r = 1
    assert np.allclose(out, [[-0.5 * 2 * att, 0.0], [1.0 + 0.5 * 2 * att, 0.0]], rtol=1e-15, atol=0)
    assert hits.tolist() == [1, 1] and np.allclose(mag[:, 0], 2 * abs(att))
    # coincident points exert nothing; an unsampled entry exerts nothing
    same, _, hits, _ = ref_layout_epoch(np.zeros((2, 2)), [0, 1, 2], [1, 0], [65536, 65536], a, b, 1.0, 0.5, 0, 0, 3)
    assert (same == 0).all() and hits.tolist() == [1, 1]
    out, _, hits, _ = ref_layout_epoch(y, [0, 1, 2], [1, 0], [1, 1], a, b, 1.0, 0.5, 0, 0, 3)
    assert np.array_equal(out, y) and hits.tolist() == [0, 0]
    # a close pair: the repulsion clips at 4 per component (vertex 1 draws vertex 0 as a negative at epoch 0)
    near = np.array([[0.0, 0.0], [0.02, 0.0]])
    assert 0 in ref_negatives(0, 0, [1], 3, 2)[0]
    out, _, _, clipped = ref_layout_epoch(near, [0, 1, 2], [1, 0], [65536, 65536], a, b, 1.0, 1.0, 0, 0, 3)
    assert clipped >= 1 and out[1, 0] - near[1, 0] > 3.5


def test_argument_validation_needs_no_gpu():
    from ssl_wafermap_amd.manifold import UMAP

    model = UMAP()
    assert abs(model.a_ - 1.57694) <= 1e-4 and abs(model.b_ - 0.89506) <= 1e-4 and model.embedding_ is None
    for bad in ({"n_neighbors": 1}, {"n_neighbors": 65}, {"n_components": 0}, {"n_components": 65}, {"n_epochs": 0},
                {"min_dist": -0.1}, {"min_dist": 2.0}, {"spread": 0.0}, {"learning_rate": 0.0}, {"negative_sample_rate": -1},
                {"init": "tsne"}, {"metric": "cosine"}, {"local_connectivity": 2.0}, {"set_op_mix_ratio": 0.5}):
        with pytest.raises(ValueError):
            UMAP(**bad)
    with pytest.raises(NotImplementedError, match="canberra"):
        UMAP(metric="canberra")


def test_features_not_built_are_named():
    import torch

    from ssl_wafermap_amd.manifold import UMAP

    with pytest.raises(NotImplementedError, match="densmap"):
        UMAP(densmap=True)
    with pytest.raises(NotImplementedError, match="semi-supervised"):
        UMAP().fit(torch.zeros(8, 4), y=np.zeros(8))
    with pytest.raises(NotImplementedError, match="transform"):
        UMAP().transform(torch.zeros(8, 4))


def test_cpu_tensors_are_refused():
    import torch

    from ssl_wafermap_amd import _lib, manifold

    x = torch.zeros(8, 4)
    with pytest.raises(_lib.WaferHipError):
        manifold.UMAP(n_neighbors=3).fit(x)
    with pytest.raises(_lib.WaferHipError):
        manifold.knn_graph(x, 3)
    with pytest.raises(_lib.WaferHipError):
        manifold.smooth_knn(torch.zeros(8, 3), torch.zeros(8, 3, dtype=torch.int32))
    with pytest.raises(_lib.WaferHipError):
        manifold.optimize_layout(torch.zeros(8, 2), torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                                 torch.zeros(0, dtype=torch.int32), 1.5, 0.9, 10)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_knn_graph_workspace_bytes(100, 8, 65) == 0 and lib.wm_knn_graph_workspace_bytes(100, 8, 64) > 0
    assert lib.wm_knn_graph(None, 4, 4, 0, 2, None, None, None, 0, None) == -1
    assert lib.wm_umap_smooth_knn(None, None, 4, 2, None, None, None, None, None) == -1
    assert lib.wm_umap_layout(None, None, None, None, None, 4, 2, 1.5, 0.9, 1.0, 1.0, 0, 0, 1, 1, 5, None, None) == -1
