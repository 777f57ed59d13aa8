"""CPU checks of the semi-supervised fit and the transform of new rows (ssl_wafermap_amd.manifold: InductiveUMAP,
InductiveDensMAP, label_intersect, knn_query, smooth_knn_query, optimize_transform): the float64 restatement of
umap-learn 0.5's discrete_metric_simplicial_set_intersection + reset_local_connectivity and of UMAP.transform
(smooth_knn_dist with local_connectivity 0, init_transform, optimize_layout_euclidean(move_other=False)) that the GPU
tests compare against (tests/test_gpu_umap_transform.py), its own pieces checked on hand-computed cases, and the
argument validation and refusals of the new names.  No GPU: nothing here launches a kernel."""
import numpy as np
import pytest

from test_umap_cpu import (ref_alpha, ref_knn, ref_layout_epoch, ref_negatives, ref_random_init, ref_rates, ref_sampled,
                           ref_smooth_knn, ref_union)

# ------------------------------------------------------------------------------------------------ float64 reference


def ref_far_dist(target_weight):
    return 2.5 / (1.0 - target_weight) if target_weight < 1.0 else 1.0e12


def ref_label_intersect(g, labels, far_dist, unknown_dist=1.0):
    """umap-learn's categorical intersection of the scipy CSR graph g with `labels` (-1: unknown), then
    reset_local_connectivity (rows divided by their maximum, A + A^T - A o A^T), in float64.  Returns the values at g's
    own entries, in g's order (an entry the scipy result drops is an exact 0)."""
    from scipy.sparse import csr_matrix

    g = csr_matrix(g).astype(np.float64)
    g.sort_indices()
    n = g.shape[0]
    labels = np.asarray(labels)
    rows = np.repeat(np.arange(n), np.diff(g.indptr))
    li, lj = labels[rows], labels[g.indices]
    f = np.where((li == -1) | (lj == -1), np.exp(-unknown_dist), np.where(li != lj, np.exp(-far_dist), 1.0))
    a = csr_matrix((g.data * f, g.indices.copy(), g.indptr.copy()), shape=g.shape)
    a.eliminate_zeros()
    top = np.asarray(a.max(axis=1).todense()).ravel() if a.nnz else np.zeros(n)
    a = _row_divide(a, top)
    r = csr_matrix(a + a.T - a.multiply(a.T))
    return np.asarray(r[rows, g.indices]).ravel() if g.nnz else np.zeros(0)


def _row_divide(a, top):
    """normalize(norm="max"): every row divided by its maximum (a true division, as sklearn does); zero rows stay."""
    a = a.copy()
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    a.data = a.data / np.where(top > 0, top, 1.0)[rows]
    return a


def pairwise64_rect(xq, x, metric="euclidean"):
    """float64 distances [m, n] of the rows of xq to the rows of x from the differences themselves, one query row at a
    time (equal rows are at exactly 0)."""
    xq, x = np.asarray(xq, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = np.empty((xq.shape[0], x.shape[0]))
    for i in range(xq.shape[0]):
        diff = x - xq[i]
        out[i] = np.sqrt((diff * diff).sum(axis=1)) if metric == "euclidean" else np.abs(diff).sum(axis=1)
    return out


def ref_knn_query(xq, x, k, metric="euclidean"):
    """(dist, idx) float64 / int64 [m, k] of the exact kNN of the rows of xq among the rows of x, ordered by
    (distance, index)."""
    dist = pairwise64_rect(xq, x, metric)
    idx = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(dist, idx, axis=1), idx


def ref_smooth_knn_query(dist):
    """smooth_knn_dist(local_connectivity = 0) + compute_membership_strengths(bipartite=True) in float64:
    (sigma, weights, floor); rho = 0 for every row, the bisection runs over j >= 1, the floor is 1e-3 * the mean of all
    distances."""
    dist = np.asarray(dist, dtype=np.float64)
    m, k = dist.shape
    target = np.log2(k)
    sigma = np.zeros(m)
    floor = 1e-3 * dist.mean()
    for i in range(m):
        lo, hi, mid = 0.0, np.inf, 1.0
        d = dist[i, 1:]
        for _ in range(64):
            with np.errstate(under="ignore"):
                psum = np.where(d > 0, np.exp(-np.maximum(d, 0) / mid), 1.0).sum()
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2
        sigma[i] = max(mid, floor)
    return sigma, ref_query_weights(dist, sigma), floor


def ref_query_weights(dist, sigma):
    dist = np.asarray(dist, dtype=np.float64)
    with np.errstate(under="ignore"):
        return np.where(dist > 0, np.exp(-np.maximum(dist, 0) / np.asarray(sigma, dtype=np.float64)[:, None]), 1.0)


def ref_transform_alpha(learning_rate, ep, n_epochs):
    return float(np.float32((learning_rate / 4.0) * (1.0 - ep / n_epochs)))


def ref_transform_epoch(y_new, y_train, idx, q, a, b, gamma, alpha, seed, ep, rate):
    """One epoch of the transform layout in float64 from the positions y_new among the fixed y_train: (y', sum over the
    point's terms of |term| per component, number of sampled entries per point, number of term components that clip).
    The attraction counts once; negatives come from the fitted points; the force is 0 at r = 0."""
    y, t = np.asarray(y_new, dtype=np.float64), np.asarray(y_train, dtype=np.float64)
    m, dim = y.shape
    n = t.shape[0]
    idx, q = np.asarray(idx, dtype=np.int64), np.asarray(q, dtype=np.int64)
    k = idx.shape[1]
    head = np.repeat(np.arange(m), k)
    e = np.flatnonzero(ref_sampled(q.ravel(), ep))
    total, mag = np.zeros((m, dim)), np.zeros((m, dim))
    clipped = 0
    if e.size:
        i, j = head[e], idx.ravel()[e]
        d = y[i] - t[j]
        r = (d * d).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(r > 0, -2.0 * a * b * r ** (b - 1.0) / (a * r ** b + 1.0), 0.0)
        clipped += int((np.abs(coef[:, None] * d) > 4.0).sum())
        g = np.clip(coef[:, None] * d, -4.0, 4.0)
        np.add.at(total, i, g)
        np.add.at(mag, i, np.abs(g))
        neg = ref_negatives(seed, ep, e, rate, n)
        for s in range(rate):
            d = y[i] - t[neg[:, s]]
            r = (d * d).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where(r > 0, 2.0 * gamma * b / ((0.001 + r) * (a * r ** b + 1.0)), 0.0)
            clipped += int((np.abs(coef[:, None] * d) > 4.0).sum())
            g = np.clip(coef[:, None] * d, -4.0, 4.0)
            np.add.at(total, i, g)
            np.add.at(mag, i, np.abs(g))
    hits = np.bincount(head[e], minlength=m) if e.size else np.zeros(m, dtype=np.int64)
    return y + float(alpha) * total, mag, hits, clipped


def ref_transform_start(y_train, idx, w):
    """init_transform of umap-learn 0.5.3: the weighted average of the neighbours' positions."""
    w = np.asarray(w, dtype=np.float64)
    return (w[:, :, None] * np.asarray(y_train, dtype=np.float64)[idx]).sum(axis=1) / w.sum(axis=1, keepdims=True)


def ref_transform(xq, x, y_train, k, a, b, n_epochs, seed=42, rate=5, gamma=1.0, learning_rate=1.0):
    """UMAP.transform in float64: (final positions, start positions)."""
    dist, idx = ref_knn_query(xq, x, k)
    _, w, _ = ref_smooth_knn_query(dist)
    q = ref_rates(w)
    start = ref_transform_start(y_train, idx, w)
    y = start.astype(np.float32).astype(np.float64)
    for ep in range(n_epochs):
        y = ref_transform_epoch(y, y_train, idx, q, a, b, gamma, ref_transform_alpha(learning_rate, ep, n_epochs), seed, ep,
                                rate)[0]
    return y, start


def ref_fit_labels(x, labels, k, dim, a, b, n_epochs, seed, target_weight=0.5, rate=5, gamma=1.0, learning_rate=1.0):
    """test_umap_cpu.ref_fit with the label intersection between the union and the rates (labels None: ref_fit)."""
    dist, idx = ref_knn(x, k)
    _, _, w, _ = ref_smooth_knn(dist, idx)
    g = ref_union(idx, w)
    data = g.data if labels is None else ref_label_intersect(g, labels, ref_far_dist(target_weight))
    q = ref_rates(data)
    y = ref_random_init(x.shape[0], dim, seed).astype(np.float64)
    for ep in range(n_epochs):
        y = ref_layout_epoch(y, g.indptr, g.indices, q, a, b, gamma, ref_alpha(learning_rate, ep, n_epochs), seed, ep, rate)[0]
    return y


def recall_at_k(x_new, x_fit, y_new, y_fit, k=15):
    """The mean share of a new row's k nearest fitted rows in feature space that are among its k nearest fitted points
    in the embedding."""
    near_x = ref_knn_query(x_new, x_fit, k)[1]
    near_y = ref_knn_query(y_new, y_fit, k)[1]
    return float(np.mean([np.intersect1d(p, q).size / k for p, q in zip(near_x, near_y)]))


def loo_knn_accuracy(y, labels, k=15):
    """Leave-one-out k-NN label accuracy in the embedding y: every point takes the majority label of its k nearest
    other points (ties to the lowest label)."""
    idx = ref_knn(y, k + 1)[1]
    labels = np.asarray(labels)
    right = 0
    for i in range(y.shape[0]):
        near = [j for j in idx[i] if j != i][:k]
        right += int(np.bincount(labels[near]).argmax() == labels[i])
    return right / y.shape[0]


# ------------------------------------------------------------------------------------------------ the reference's pieces


def path_graph(w01, w12):
    from scipy.sparse import csr_matrix

    return csr_matrix(np.array([[0.0, w01, 0.0], [w01, 0.0, w12], [0.0, w12, 0.0]]))


def test_reference_intersection_on_a_path_by_hand():
    """0 - 1 - 2 with labels (0, 1, -1), weights 0.5 and 0.25, far_dist 5: v_01 = 0.5 e^-5, v_12 = 0.25 e^-1.  Rows 0 and 2
    have one entry each, which the max-normalisation makes 1; row 1 keeps (v_01 / v_12, 1); the union with a 1 is 1."""
    g = path_graph(0.5, 0.25)
    assert g.indices.tolist() == [1, 0, 2, 1]
    out = ref_label_intersect(g, [0, 1, -1], 5.0)
    x = (0.5 * np.exp(-5.0)) / (0.25 * np.exp(-1.0))
    assert np.allclose(out, [(1.0 + x) - x, (x + 1.0) - x, 1.0, 1.0], rtol=1e-15, atol=0)
    # a triangle's far edge survives below 1: add 0 - 2 (labels 0 and -1: unknown) with weight 1
    from scipy.sparse import csr_matrix

    tri = csr_matrix(np.array([[0.0, 0.5, 1.0], [0.5, 0.0, 0.25], [1.0, 0.25, 0.0]]))
    out = ref_label_intersect(tri, [0, 1, -1], 5.0)
    v01, v02, v12 = 0.5 * np.exp(-5.0), np.exp(-1.0), 0.25 * np.exp(-1.0)
    m01, m10 = v01 / v02, v01 / v12  # row maxima: v02, v12, v02
    want01 = m01 + m10 - m01 * m10
    assert tri.indices.tolist() == [1, 2, 0, 2, 0, 1]
    assert np.allclose(out, [want01, 1.0, want01, 1.0, 1.0, 1.0], rtol=1e-14, atol=0) and 0 < want01 < 0.1
    # target_weight = 1: far_dist = 1e12, the cross-label entry is exactly 0, vertex 0's row is all zeros, no NaN
    out = ref_label_intersect(g, [0, 1, -1], ref_far_dist(1.0))
    assert out.tolist() == [0.0, 0.0, 1.0, 1.0]
    # equal labels change nothing but the normalisation; all unknown likewise (the factor cancels in the division)
    assert np.allclose(ref_label_intersect(g, [3, 3, 3], 5.0), [1.0, 1.0, 1.0, 1.0], rtol=1e-15)
    assert np.allclose(ref_label_intersect(g, [-1, -1, -1], 5.0), [1.0, 1.0, 1.0, 1.0], rtol=1e-15)
    assert ref_far_dist(0.5) == 5.0 and ref_far_dist(0.0) == 2.5 and ref_far_dist(1.0) == 1e12


def test_reference_transform_epoch_by_hand():
    """One new point at the origin, one neighbour at unit distance, no negatives: y' = y + alpha att, att once."""
    a, b = 1.5, 0.9
    y, t = np.zeros((1, 2)), np.array([[1.0, 0.0]])
    out, mag, hits, _ = ref_transform_epoch(y, t, [[0]], [[65536]], a, b, 1.0, 0.25, 42, 0, 0)
    att = -2.0 * a * b / (a + 1.0) * (0.0 - 1.0)  # r = 1, d = y_i - y_j = -1: towards the neighbour
    assert np.allclose(out, [[0.25 * att, 0.0]], rtol=1e-15, atol=0) and att > 0
    assert hits.tolist() == [1] and np.allclose(mag, [[abs(att), 0.0]])
    # the fit's epoch on the same pair moves the head twice as far
    fit, _, _, _ = ref_layout_epoch(np.array([[0.0, 0.0], [1.0, 0.0]]), [0, 1, 2], [1, 0], [65536, 65536], a, b, 1.0, 0.25, 42, 0, 0)
    assert np.allclose(fit[0], [2 * 0.25 * att, 0.0], rtol=1e-15, atol=0)
    # a coincident neighbour exerts nothing, negatives at the same place neither
    same, _, hits, _ = ref_transform_epoch(np.ones((1, 2)), np.ones((1, 2)), [[0]], [[65536]], a, b, 1.0, 0.25, 42, 0, 3)
    assert (same == 1).all() and hits.tolist() == [1]
    # an entry with q = 1 is not sampled at epoch 0 (nor in any of the first 65535 epochs)
    out, _, hits, _ = ref_transform_epoch(y, t, [[0]], [[1]], a, b, 1.0, 0.25, 42, 0, 3)
    assert np.array_equal(out, y) and hits.tolist() == [0]
    # negatives come from the fitted points and repel: with one fitted point every negative is that point
    out, _, _, clipped = ref_transform_epoch(np.array([[0.98, 0.0]]), t, [[0]], [[65536]], a, b, 1.0, 1.0, 42, 0, 3)
    assert clipped >= 3 and out[0, 0] < 0.98 - 3 * 3.5
    assert ref_transform_alpha(1.0, 0, 100) == 0.25 and ref_transform_alpha(1.0, 50, 100) == 0.125


def test_reference_query_memberships_and_start():
    """rho = 0: the weights are exp(-d / sigma) with the sum over j >= 1 at log2 k; an all-duplicate row has weights 1
    and sigma at the floor; the start is the weighted mean."""
    rng = np.random.default_rng(0)
    dist = np.sort(rng.uniform(0.5, 2.0, (6, 15)), axis=1)
    dist[5] = 0.0
    sigma, w, floor = ref_smooth_knn_query(dist)
    assert np.allclose(w[:5, 1:].sum(axis=1), np.log2(15), atol=1e-5) and (w[5] == 1).all() and sigma[5] == floor
    assert np.allclose(w[:5], np.exp(-dist[:5] / sigma[:5, None]))
    start = ref_transform_start(np.array([[0.0, 0.0], [2.0, 4.0]]), np.array([[0, 1]]), np.array([[3.0, 1.0]]))
    assert np.allclose(start, [[0.5, 1.0]])
    d, i = ref_knn_query(np.array([[0.0, 0.0], [1.0, 1.0]]), np.array([[3.0, 4.0], [1.0, 1.0], [0.0, 1.0], [1.0, 1.0]]), 3)
    assert i.tolist() == [[2, 1, 3], [1, 3, 2]] and np.allclose(d, [[1.0, np.sqrt(2), np.sqrt(2)], [0.0, 0.0, 1.0]])
    assert d[1, 0] == 0 and d[1, 1] == 0
    assert recall_at_k(np.eye(3), np.eye(3), np.eye(3), np.eye(3), k=1) == 1.0
    assert loo_knn_accuracy(np.array([[0.0], [0.1], [0.2], [5.0], [5.1], [5.2]]), [0, 0, 0, 1, 1, 1], k=2) == 1.0


# ------------------------------------------------------------------------------------------------ the new names


@pytest.mark.parametrize("name", ["InductiveUMAP", "InductiveDensMAP"])
def test_argument_validation_and_refusals(name):
    import torch

    from ssl_wafermap_amd import _lib, manifold

    cls = getattr(manifold, name)
    model = cls()
    assert model.target_weight == 0.5 and model.target_metric == "categorical" and model.transform_seed == 42
    assert isinstance(model, manifold.DensMAP if name == "InductiveDensMAP" else manifold.UMAP)
    cls(target_weight=0.0), cls(target_weight=1.0, transform_seed=7, n_neighbors=30, n_components=50, min_dist=0.0)
    for bad in ({"target_weight": -0.1}, {"target_weight": 1.1}, {"n_neighbors": 1}, {"n_components": 65}, {"n_epochs": 0}):
        with pytest.raises(ValueError):
            cls(**bad)
    with pytest.raises(NotImplementedError, match="l2"):
        cls(target_metric="l2")
    with pytest.raises(NotImplementedError, match="densmap|DensMAP") if name == "InductiveUMAP" else pytest.raises(ValueError):
        cls(densmap=True)
    x = torch.zeros(8, 4)
    for bad_y in (np.zeros(8), np.zeros(7, dtype=np.int64), np.full(8, -2), np.zeros((8, 1), dtype=np.int64), torch.zeros(8),
                  torch.zeros(9, dtype=torch.int64), torch.full((8,), -2, dtype=torch.int32), ["a"] * 8):
        with pytest.raises(ValueError):
            model.fit(x, y=bad_y)
    # good labels pass the label check; the CPU tensor x is then refused like everywhere else
    for good_y in (np.zeros(8, dtype=np.int64), np.full(8, -1, dtype=np.int32), torch.arange(8), list(range(8))):
        with pytest.raises(_lib.WaferHipError):
            model.fit(x, y=good_y)
    with pytest.raises(ValueError, match="fit"):
        model.transform(x)
    assert model.transform_epochs(10) == 100 and model.transform_epochs(10001) == 30
    assert cls(n_epochs=200).transform_epochs(10) == 66 and cls(n_epochs=2).transform_epochs(10) == 1
    assert manifold.far_distance(0.5) == 5.0 and manifold.far_distance(1.0) == 1e12


def test_parents_keep_raising_and_name_the_new_classes():
    import torch

    from ssl_wafermap_amd.manifold import UMAP, DensMAP

    for cls in (UMAP, DensMAP):
        with pytest.raises(NotImplementedError, match=f"semi-supervised.*Inductive{cls.__name__}"):
            cls().fit(torch.zeros(8, 4), y=np.zeros(8))
        with pytest.raises(NotImplementedError, match=f"transform.*Inductive{cls.__name__}"):
            cls().transform(torch.zeros(8, 4))


def test_cpu_tensors_are_refused():
    import torch

    from ssl_wafermap_amd import _lib, manifold

    with pytest.raises(_lib.WaferHipError):
        manifold.knn_query(torch.zeros(3, 4), torch.zeros(8, 4), 3)
    with pytest.raises(_lib.WaferHipError):
        manifold.smooth_knn_query(torch.zeros(8, 3))
    g = manifold.CSR(torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    with pytest.raises(_lib.WaferHipError):
        manifold.label_intersect(g, torch.zeros(8, dtype=torch.int32), 5.0)
    with pytest.raises(_lib.WaferHipError):
        manifold.optimize_transform(torch.zeros(3, 2), torch.zeros(8, 2), torch.zeros(3, 2, dtype=torch.int32),
                                    torch.zeros(3, 2, dtype=torch.int32), 1.5, 0.9, 10)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_knn_query_workspace_bytes(10, 100, 8, 65) == 0 and lib.wm_knn_query_workspace_bytes(0, 100, 8, 5) == 0
    assert lib.wm_knn_query_workspace_bytes(10, 100, 8, 64) > 0
    assert lib.wm_knn_query(None, 4, None, 4, 4, 0, 2, None, None, None, 0, None) == -1
    assert lib.wm_umap_label_intersect(None, None, None, None, 4, 0.5, 0.5, None, None, None) == -1
    assert lib.wm_umap_smooth_knn_query(None, 4, 2, None, None, None, None) == -1
    assert lib.wm_umap_transform_layout(None, None, None, None, None, 4, 4, 2, 2, 1.5, 0.9, 1.0, 1.0, 42, 0, 1, 1, 5, None) == -1
