"""UMAP embedding of dumped features.

The reference's flow (notebooks 3.0-Embeddings-inference, 3.1-Embeddings-clustering, 3.2-Embeddings-SSL-categories,
2.0-Figures-MixedWM38 and, through its dumped features, 2.0-Figures-nearest-neighbors):
`umap.UMAP(...).fit_transform(data)`, for the 2-D pictures and, in 3.2, as the 50-dimensional reduction that HDBSCAN
then clusters.

Three steps, the GPU-shaped ones as HIP kernels:
  1. the exact k-nearest-neighbour graph with indices (csrc/cluster.hip: wm_knn_graph; umap-learn approximates it with
     NN-descent above 4096 rows, here it is exact at every size);
  2. the fuzzy simplicial set: rho, sigma and the membership weights per row (csrc/umap.hip: wm_umap_smooth_knn), then
     the union G = P + P^T - P o P^T as CSR, a one-off index build with torch sort / unique on int64 keys;
  3. the layout optimisation (csrc/umap.hip: wm_umap_layout), the hot path: umap-learn's racy in-place loop restated
     as a deterministic double-buffered gather -- the kernel file states every formula.  Two fits give the same bits.

What runs on the host: the curve fit of (a, b) (scipy, 300 points, as umap-learn's find_ab_params) and the spectral
initialisation (scipy eigsh on the normalised Laplacian, as umap-learn itself does).

DensMAP (`umap.UMAP(densmap=True, dens_lambda=...)` of notebooks 3.0, 3.1 and 3.2) is its own estimator, `DensMAP`:
the same three steps, plus
  4. the graph's radii ro_i = log(eps + sum w d^2 / sum w) once per fit (csrc/umap.hip: wm_densmap_graph_radii) over the
     graph distances max(d_ij, d_ji) that `fuzzy_simplicial_set(..., return_dists=True)` returns, and, in the last
     `dens_frac` of the epochs, the density term: per epoch the embedding's radii, their statistics and the per-vertex
     terms by fixed-order kernels, then the layout kernel with the term compiled in (wm_densmap_layout).
`UMAP(densmap=True)` itself keeps raising and names `DensMAP`.

Semi-supervised fits and the transform of new rows (`reducer.fit(x, y=labels); reducer.transform(x)` of notebooks
3.0-Embeddings-inference and 2.0-Figures-MixedWM38, labels -1 where unknown) are the estimators `InductiveUMAP` and
`InductiveDensMAP`: the parents' steps, plus
  5. with y: the categorical-target intersection of the fuzzy graph (csrc/umap.hip: wm_umap_label_intersect), applied
     between `fuzzy_simplicial_set` and the initialisation;
  6. transform: the exact kNN of the new rows among the fitted ones (csrc/cluster.hip: wm_knn_query), their
     memberships (wm_umap_smooth_knn_query), the weighted-average start, and the layout in which only the new points
     move -- all epochs in one launch, one wave per point (wm_umap_transform_layout).
`UMAP` and `DensMAP` themselves keep raising for y= and transform and name these classes.

How far a picture can be believed (`trustworthiness`, `continuity`, `embedding_quality`; sklearn.manifold.trustworthiness
and its converse) is scored on ALL rows:
  7. the neighbour lists of both spaces (wm_knn_graph at k + 1, the row removed by index), the distances of the listed
     pairs in the other space (csrc/cluster.hip: wm_pair_dist) and the rank of every listed row in the other space's
     (distance, index) order (wm_rank_query, one all-pairs pass with integer counts); the scores are float64 arithmetic
     on those integer ranks on the host (`quality_from_ranks`).

Not built: target_metric other than "categorical", inverse_transform, update (NotImplementedError naming the feature).
Only local_connectivity = 1 and set_op_mix_ratio = 1 are supported.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace
from .cluster import _prep, metric_code

MAX_NEIGHBORS = 64
MAX_COMPONENTS = 64
_MASK32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ host restatements


def find_ab_params(spread: float, min_dist: float) -> Tuple[float, float]:
    """umap-learn's find_ab_params: fit 1 / (1 + a x^(2b)) to the offset exponential exp(-(x - min_dist) / spread)
    (1 below min_dist) on 300 points of [0, 3 spread]."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def mix32(x: int) -> int:
    """The kernels' 32-bit finaliser (csrc/common.h: lowbias32)."""
    x &= _MASK32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _MASK32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _MASK32
    x ^= x >> 16
    return x


def negative_index(seed: int, epoch: int, entry: int, t: int, n: int) -> int:
    """The t-th negative sample of CSR entry `entry` at `epoch` (csrc/umap.hip)."""
    h = mix32(mix32(mix32((seed ^ (epoch * 0x9E3779B9)) & _MASK32) + entry) + t)
    return (h * n) >> 32


def is_sampled(q: int, epoch: int) -> bool:
    """Whether an entry of rate q (of 65536) is sampled at `epoch`: (E q) >> 16 times in E epochs."""
    return (((epoch + 1) * q) >> 16) > ((epoch * q) >> 16)


class EmbeddingQuality(NamedTuple):
    """The neighbourhood scores of an embedding at one k ("Trustworthiness and continuity"); the per-row
    vectors are float64 [n] and the scores are their means."""
    n_neighbors: int
    trustworthiness: float
    continuity: float
    neighbor_preservation: float
    trustworthiness_rows: np.ndarray
    continuity_rows: np.ndarray
    preservation_rows: np.ndarray


def check_quality_k(n: int, k: int) -> int:
    """sklearn's rule (n_neighbors < n_samples / 2, else the normaliser 2n - 3k - 1 can vanish) and the kNN kernels' (64
    candidates, the row itself one of them)."""
    k = int(k)
    if k < 1:
        raise ValueError(f"n_neighbors ({k}) must be at least 1")
    if 2 * k >= n:
        raise ValueError(f"n_neighbors ({k}) should be less than n_samples / 2 ({n / 2})")
    if k > MAX_NEIGHBORS - 1:
        raise ValueError(f"n_neighbors ({k}) must be at most {MAX_NEIGHBORS - 1}")
    return k


def _penalty_score(ranks, n: int, k: int):
    """(1 - 2 / (n k (2n - 3k - 1)) * sum_i pen_i, the per-row values 1 - 2 / (k (2n - 3k - 1)) * pen_i float64 [n]) with
    pen_i = sum_j max(0, rank - k) over the first k entries of row i.  The sums are exact integers (int64), followed by
    one multiply and one subtract."""
    pen = np.maximum(ranks[:, :k].astype(np.int64) - k, 0).sum(axis=1)
    norm = k * (2.0 * n - 3.0 * k - 1.0)
    return 1.0 - float(pen.sum()) * (2.0 / (n * norm)), 1.0 - pen.astype(np.float64) * (2.0 / norm)


def quality_from_ranks(ranks_x, ranks_emb, n_neighbors):
    """Trustworthiness, continuity and neighbour preservation from integer ranks, in float64 on the host.
    ranks_x int [n, K]: r_x(i, j), the 1-based rank (self excluded, ties by index) in the INPUT space of the j that is
    the q-th neighbour of row i in the EMBEDDING; ranks_emb int [n, K]: the rank in the embedding of the q-th neighbour
    in the input space.  Both lists are ordered, so their first k columns belong to N_k for every k <= K: `n_neighbors`
    may be one k (an EmbeddingQuality is returned) or a sequence of them (a list, equal to the separate calls).  A
    neighbour of one space is one of the other exactly when its rank there is at most k, which gives the preservation
    from either matrix (the trustworthiness side is used)."""
    ranks_x, ranks_emb = np.asarray(ranks_x), np.asarray(ranks_emb)
    if ranks_x.ndim != 2 or ranks_x.shape != ranks_emb.shape or ranks_x.dtype.kind not in "iu" or ranks_emb.dtype.kind not in "iu":
        raise ValueError("two integer rank matrices [n, K] of one shape expected")
    if np.ndim(n_neighbors) > 0:
        return [quality_from_ranks(ranks_x, ranks_emb, int(k)) for k in n_neighbors]
    n, width = ranks_x.shape
    k = check_quality_k(n, n_neighbors)
    if k > width:
        raise ValueError(f"n_neighbors ({k}) exceeds the {width} ranks per row")
    t, t_rows = _penalty_score(ranks_x, n, k)
    c, c_rows = _penalty_score(ranks_emb, n, k)
    p_rows = (ranks_x[:, :k] <= k).sum(axis=1).astype(np.float64) / k
    return EmbeddingQuality(k, t, c, float(p_rows.mean()), t_rows, c_rows, p_rows)


# ------------------------------------------------------------------------------------------------ GPU steps


def knn_graph(x, k: int, metric: str = "euclidean"):
    """The k nearest rows of every row of x [n, d] (device tensor), the row itself among them: (dist float32 [n, k],
    idx int32 [n, k]) on the device, every row ordered by (distance, index).  1 <= k <= min(n, 64).  Exact; the distance
    function is cluster.py's (relative error at most (d + 3) 2^-24, duplicates at exactly 0)."""
    import torch

    code = metric_code(metric)
    x = _prep(x)
    n, d = x.shape
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"k ({k}) must be in [1, n_samples = {n}]")
    lib = _lib.load()
    need = lib.wm_knn_graph_workspace_bytes(n, d, k)
    ws = workspace(need, f"knn_graph: unsupported sizes n={n} d={d} k={k} (k <= {MAX_NEIGHBORS})", x.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
    check(lib.wm_knn_graph(ptr(x), n, d, code, k, ptr(dist), ptr(idx), ptr(ws), need, stream_ptr()), "wm_knn_graph")
    return dist, idx


def smooth_knn(dist, idx):
    """(rho [n], sigma [n], weights [n, k]) float32 of a kNN graph as `knn_graph` returns it: umap-learn's
    smooth_knn_dist and compute_membership_strengths with local_connectivity = 1."""
    import torch

    require_gpu(dist, idx)
    if dist.dim() != 2 or idx.shape != dist.shape or dist.dtype != torch.float32 or idx.dtype != torch.int32:
        raise ValueError("dist float32 [n, k] and idx int32 [n, k] expected")
    n, k = dist.shape
    if not 1 <= k <= min(n, MAX_NEIGHBORS):
        raise ValueError(f"k ({k}) must be in [1, min(n_samples, {MAX_NEIGHBORS})]")
    mean = dist.double().mean().reshape(1).contiguous()
    rho = torch.empty(n, dtype=torch.float32, device=dist.device)
    sigma = torch.empty(n, dtype=torch.float32, device=dist.device)
    w = torch.empty((n, k), dtype=torch.float32, device=dist.device)
    check(_lib.load().wm_umap_smooth_knn(ptr(dist), ptr(idx), n, k, ptr(mean), ptr(rho), ptr(sigma), ptr(w), stream_ptr()),
          "wm_umap_smooth_knn")
    return rho, sigma, w


def knn_query(xq, x, k: int, metric: str = "euclidean"):
    """The k nearest rows of x [n, d] for every row of xq [m, d] (device tensors): (dist float32 [m, k], idx int32
    [m, k]) on the device, every row ordered by (distance, index), by `knn_graph`'s distance function (a query equal to
    a row of x leads with exactly 0).  1 <= k <= min(n, 64), m >= 1.  `knn_query(x, x, k)` is `knn_graph(x, k)` in bits."""
    import torch

    code = metric_code(metric)
    xq, x = _prep(xq), _prep(x)
    if xq.shape[1] != x.shape[1]:
        raise ValueError(f"xq has {xq.shape[1]} features, x has {x.shape[1]}")
    (m, d), n = xq.shape, x.shape[0]
    k = int(k)
    if m < 1:
        raise ValueError("at least one query row expected")
    if not 1 <= k <= n:
        raise ValueError(f"k ({k}) must be in [1, n_samples = {n}]")
    lib = _lib.load()
    need = lib.wm_knn_query_workspace_bytes(m, n, d, k)
    ws = workspace(need, f"knn_query: unsupported sizes m={m} n={n} d={d} k={k} (k <= {MAX_NEIGHBORS})", x.device)
    dist = torch.empty((m, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((m, k), dtype=torch.int32, device=x.device)
    check(lib.wm_knn_query(ptr(xq), m, ptr(x), n, d, code, k, ptr(dist), ptr(idx), ptr(ws), need, stream_ptr()), "wm_knn_query")
    return dist, idx


def _pair_args(name: str, xq, x, idx):
    import torch

    xq, x = _prep(xq), _prep(x)
    require_gpu(idx)
    if xq.shape[1] != x.shape[1]:
        raise ValueError(f"xq has {xq.shape[1]} features, x has {x.shape[1]}")
    if xq.shape[0] < 1 or x.shape[0] < 1:
        raise ValueError("at least one row expected on either side")
    if idx.dim() != 2 or idx.shape[0] != xq.shape[0] or idx.dtype != torch.int32:
        raise ValueError(f"idx int32 [m = {xq.shape[0]}, k] expected")
    if not 1 <= idx.shape[1] <= MAX_NEIGHBORS:
        raise ValueError(f"{name}: k ({idx.shape[1]}) must be in [1, {MAX_NEIGHBORS}]")
    return xq, x


def pair_distances(xq, x, idx, metric: str = "euclidean"):
    """out[i, q] = dist(xq[i], x[idx[i, q]]) float32 [m, k] on the device for idx int32 [m, k] (device tensors): the bits
    `knn_graph` / `knn_query` give that pair (their own lists come back with their own distances).  An entry of -1 (or any
    index outside [0, n)) gives +inf.  1 <= k <= 64."""
    import torch

    code = metric_code(metric)
    xq, x = _pair_args("pair_distances", xq, x, idx)
    (m, d), n, k = xq.shape, x.shape[0], idx.shape[1]
    out = torch.empty((m, k), dtype=torch.float32, device=x.device)
    check(_lib.load().wm_pair_dist(ptr(xq), m, ptr(x), n, d, code, ptr(idx), k, ptr(out), stream_ptr()), "wm_pair_dist")
    return out


def neighbor_ranks(xq, x, idx, metric: str = "euclidean", exclude_self: bool = False):
    """The 1-based rank of x[idx[i, q]] among the rows of x as seen from xq[i], int32 [m, k] on the device:
    1 + #{ l : (dist(i, l), l) < (dist(i, j), j) }, j = idx[i, q] -- the candidates ordered by (distance, index) as
    `knn_query` orders them, so the q-th entry of that row's kNN list has rank q + 1.  exclude_self (xq is x, m = n):
    column i is never counted for row i (the rank among the other rows).  An entry of -1 ranks behind every column.
    The distances of the listed pairs come from `pair_distances`, the counts from wm_rank_query (one all-pairs pass)."""
    import torch

    code = metric_code(metric)
    xq, x = _pair_args("neighbor_ranks", xq, x, idx)
    (m, d), n, k = xq.shape, x.shape[0], idx.shape[1]
    if exclude_self and m != n:
        raise ValueError(f"exclude_self needs the rows of x themselves as queries (m = {m}, n = {n})")
    lib = _lib.load()
    need = lib.wm_rank_query_workspace_bytes(m, n, d, k)
    ws = workspace(need, f"neighbor_ranks: unsupported sizes m={m} n={n} d={d} k={k} (k <= {MAX_NEIGHBORS})", x.device)
    thr = pair_distances(xq, x, idx, metric)
    # the kernel wants every row's thresholds sorted by (distance, index): a stable sort by the index, then by the distance
    by_j = torch.sort(idx, dim=1, stable=True).indices
    order = by_j.gather(1, torch.sort(thr.gather(1, by_j), dim=1, stable=True).indices)
    t_sorted, j_sorted = thr.gather(1, order).contiguous(), idx.gather(1, order).contiguous()
    skip = (torch.arange(m, dtype=torch.int32, device=x.device) if exclude_self
            else torch.full((m,), -1, dtype=torch.int32, device=x.device))
    count = torch.empty((m, k), dtype=torch.int32, device=x.device)
    check(lib.wm_rank_query(ptr(xq), m, ptr(x), n, d, code, ptr(t_sorted), ptr(j_sorted), ptr(skip), k, ptr(count), ptr(ws),
                            need, stream_ptr()), "wm_rank_query")
    ranks = torch.empty_like(count)
    ranks.scatter_(1, order, count + 1)
    return ranks


def neighbor_lists(x, k: int, metric: str = "euclidean"):
    """N_k of every row: the first k rows OTHER than the row itself in its (distance, index) order, int32 [n, k] on the
    device.  `knn_graph` at k + 1 with the row removed by index, not by distance: exact duplicates of the row stay, and
    when more than k duplicates with lower indices push the row out of its own list the last entry goes instead."""
    import torch

    idx = knn_graph(x, k + 1, metric)[1]
    own = idx == torch.arange(idx.shape[0], dtype=torch.int32, device=idx.device).unsqueeze(1)
    keep = torch.sort(own.to(torch.int8), dim=1, stable=True).indices[:, :k]  # (the row itself moves to the end)
    return idx.gather(1, keep).contiguous()


def embedding_quality(x, embedding, n_neighbors=5, metric: str = "euclidean", embedding_metric: str = "euclidean"):
    """Trustworthiness, continuity and neighbour preservation of `embedding` [n, Db] for the rows x [n, Da] (device
    tensors) on ALL rows: an EmbeddingQuality, or a list of them when n_neighbors is a sequence (one pass at the largest
    k serves every smaller one).  Two `knn_graph` calls (k + 1, the row removed by index) give the neighbour lists of
    both spaces, two rank passes (`neighbor_ranks`) the rank of every neighbour of one space in the other; the scores
    are `quality_from_ranks` of those integers, float64 on the host.  n_neighbors < n / 2 and <= 63."""
    x, embedding = _prep(x), _prep(embedding)
    n = x.shape[0]
    if embedding.shape[0] != n:
        raise ValueError(f"x has {n} rows, the embedding {embedding.shape[0]}")
    ks = [int(k) for k in n_neighbors] if np.ndim(n_neighbors) > 0 else [int(n_neighbors)]
    if not ks:
        raise ValueError("at least one n_neighbors expected")
    for k in ks:
        check_quality_k(n, k)
    near_x = neighbor_lists(x, max(ks), metric)
    near_e = neighbor_lists(embedding, max(ks), embedding_metric)
    ranks_x = neighbor_ranks(x, x, near_e, metric, exclude_self=True).cpu().numpy()
    ranks_e = neighbor_ranks(embedding, embedding, near_x, embedding_metric, exclude_self=True).cpu().numpy()
    res = quality_from_ranks(ranks_x, ranks_e, ks)
    return res if np.ndim(n_neighbors) > 0 else res[0]


def trustworthiness(x, embedding, n_neighbors: int = 5, metric: str = "euclidean", embedding_metric: str = "euclidean",
                    return_rows: bool = False):
    """sklearn.manifold.trustworthiness on every row, on the device: 1 - 2 / (n k (2n - 3k - 1)) * the sum over the
    rows i and their k nearest rows j IN THE EMBEDDING of max(0, r_x(i, j) - k), r_x the rank of j in the input space.
    Ties are resolved by the index (sklearn: arbitrarily).  return_rows: (score, per-row values float64 [n])."""
    x, embedding = _prep(x), _prep(embedding)
    n = x.shape[0]
    if embedding.shape[0] != n:
        raise ValueError(f"x has {n} rows, the embedding {embedding.shape[0]}")
    k = check_quality_k(n, n_neighbors)
    ranks = neighbor_ranks(x, x, neighbor_lists(embedding, k, embedding_metric), metric, exclude_self=True).cpu().numpy()
    score, rows_ = _penalty_score(ranks, n, k)
    return (score, rows_) if return_rows else score


def continuity(x, embedding, n_neighbors: int = 5, metric: str = "euclidean", embedding_metric: str = "euclidean",
               return_rows: bool = False):
    """Trustworthiness with the two spaces exchanged: the neighbours of the input space, ranked in the embedding (how
    many true neighbours the embedding tore apart).  continuity(a, b) is trustworthiness(b, a) in bits."""
    return trustworthiness(embedding, x, n_neighbors, embedding_metric, metric, return_rows)


def smooth_knn_query(dist):
    """(sigma [m], weights [m, k]) float32 of the distances of new rows to their nearest fitted rows as `knn_query`
    returns them: umap-learn's smooth_knn_dist with local_connectivity = 0 (rho = 0) and
    compute_membership_strengths(bipartite=True), as UMAP.transform calls them."""
    import torch

    require_gpu(dist)
    if dist.dim() != 2 or dist.dtype != torch.float32:
        raise ValueError("dist float32 [m, k] expected")
    m, k = dist.shape
    if m < 1 or not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"m >= 1 and k in [1, {MAX_NEIGHBORS}] expected")
    mean = dist.double().mean().reshape(1).contiguous()
    sigma = torch.empty(m, dtype=torch.float32, device=dist.device)
    w = torch.empty((m, k), dtype=torch.float32, device=dist.device)
    check(_lib.load().wm_umap_smooth_knn_query(ptr(dist), m, k, ptr(mean), ptr(sigma), ptr(w), stream_ptr()),
          "wm_umap_smooth_knn_query")
    return sigma, w


class CSR(NamedTuple):
    """A square sparse matrix on the device: indptr int32 [n + 1], indices int32 [nnz] (columns sorted within a row),
    data float32 [nnz]."""

    indptr: "object"
    indices: "object"
    data: "object"

    @property
    def shape(self):
        return (self.indptr.numel() - 1,) * 2

    def to_scipy(self):
        from scipy.sparse import csr_matrix

        return csr_matrix((self.data.cpu().numpy(), self.indices.cpu().numpy(), self.indptr.cpu().numpy()), shape=self.shape)


def fuzzy_union(idx, weights, dist=None):
    """G = P + P^T - P o P^T of the directed membership matrix P[i, idx[i, j]] = weights[i, j] (zeros dropped), as CSR
    on the device.  The value of an entry is formed in double from the two float32 memberships and rounded once, by
    the same expression for (i, j) and (j, i): G is symmetric in bits and within 2^-24 relative of the exact union.
    With `dist` (the kNN distances float32 [n, k]) the result is (G, dists): dists float32 [nnz], aligned with G's
    entries, max(d_ij, d_ji) over the kNN graph with a missing direction counting 0 (umap-learn's dmat.maximum(dmat.T))."""
    import torch

    require_gpu(idx, weights)
    n, k = idx.shape
    dev = idx.device
    rows = torch.arange(n, device=dev, dtype=torch.int64).unsqueeze(1).expand(n, k)
    cols = idx.long()
    keep = weights > 0
    key = (rows * n + cols)[keep]
    val = weights[keep].double()
    key, order = torch.sort(key)
    val = val[order]
    both = torch.unique(torch.cat([key, (key % n) * n + key // n]))  # sorted: row-major, columns ascending

    def lookup(want):
        if key.numel() == 0:
            return torch.zeros(want.shape, dtype=torch.float64, device=dev)
        at = torch.searchsorted(key, want).clamp_(max=key.numel() - 1)
        return torch.where(key[at] == want, val[at], torch.zeros((), dtype=torch.float64, device=dev))

    p, pt = lookup(both), lookup((both % n) * n + both // n)
    data = ((p + pt) - p * pt).float()
    r = both // n
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    graph = CSR(indptr.to(torch.int32), (both % n).to(torch.int32).contiguous(), data.contiguous())
    if dist is None:
        return graph
    require_gpu(dist)
    # every kNN entry carries a distance, also one whose membership is 0
    key, order = torch.sort((rows * n + cols).reshape(-1))
    val = dist.reshape(-1).double()[order]
    return graph, torch.maximum(lookup(both), lookup((both % n) * n + both // n)).float().contiguous()


def fuzzy_simplicial_set(x, n_neighbors: int, metric: str = "euclidean", return_dists: bool = False):
    """umap-learn's fuzzy_simplicial_set (local_connectivity = 1, set_op_mix_ratio = 1) of the rows of x; with
    `return_dists` also the graph distances aligned with its entries (`fuzzy_union`)."""
    dist, idx = knn_graph(x, n_neighbors, metric)
    _, _, w = smooth_knn(dist, idx)
    return fuzzy_union(idx, w, dist if return_dists else None)


def far_distance(target_weight: float) -> float:
    """umap-learn's far_dist of a categorical target: 2.5 / (1 - target_weight), 1e12 at target_weight = 1."""
    return 2.5 / (1.0 - target_weight) if target_weight < 1.0 else 1.0e12


def label_intersect(graph: CSR, labels, far_dist: float, unknown_dist: float = 1.0) -> CSR:
    """umap-learn's discrete_metric_simplicial_set_intersection + reset_local_connectivity of the symmetric-pattern
    CSR `graph` (`fuzzy_union`) with `labels` int32 [n] on the device (-1: unknown): entries across two labels are
    scaled by exp(-far_dist), entries with an unknown end by exp(-unknown_dist), rows are divided by their maximum and
    the result is symmetrised again (csrc/umap.hip: wm_umap_label_intersect).  Same pattern, symmetric in bits; an
    entry that becomes 0 stays as an explicit zero."""
    import math

    import torch

    require_gpu(graph.indptr, graph.indices, graph.data, labels)
    n = graph.shape[0]
    if graph.indptr.dtype != torch.int32 or graph.indices.dtype != torch.int32 or graph.data.dtype != torch.float32:
        raise ValueError("graph: indptr, indices int32 and data float32 expected")
    if graph.indices.shape != graph.data.shape or graph.indices.dim() != 1:
        raise ValueError("graph: indices [nnz] and data [nnz] expected")
    if labels.dtype != torch.int32 or labels.shape != (n,):
        raise ValueError(f"labels int32 [{n}] expected")
    if n < 1 or not (far_dist >= 0 and unknown_dist >= 0):
        raise ValueError("a graph of at least one vertex and far_dist, unknown_dist >= 0 expected")
    _check_csr(graph.indptr, graph.indices.numel())
    if graph.indices.numel() and (int(graph.indices.min()) < 0 or int(graph.indices.max()) >= n):
        raise ValueError("indices must lie in [0, n)")
    out = torch.empty_like(graph.data)
    ws = torch.empty(n, dtype=torch.float64, device=graph.data.device)
    check(_lib.load().wm_umap_label_intersect(ptr(graph.indptr), ptr(graph.indices), ptr(graph.data), ptr(labels), n,
                                              math.exp(-float(far_dist)), math.exp(-float(unknown_dist)), ptr(out), ptr(ws),
                                              stream_ptr()), "wm_umap_label_intersect")
    return CSR(graph.indptr, graph.indices, out)


def sample_rates(data):
    """q_e = rint(65536 w_e / max w) of the graph's weights, in float64, as the int32 tensor the layout kernel reads
    (0 <= q_e <= 65536)."""
    import torch

    if data.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=data.device)
    w = data.double()
    return torch.round(65536.0 * w / w.max()).to(torch.int32).contiguous()


def _check_csr(indptr, nnz: int):
    """The kernels trust a graph's row pointers: check once on the host that they rise from 0 to nnz."""
    ip = indptr.long()
    if int(ip[0]) != 0 or int(ip[-1]) != nnz or bool((ip[1:] < ip[:-1]).any()):
        raise ValueError("indptr must rise from 0 to nnz")


def _check_schedule(a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate, negative_sample_rate):
    """The epoch range and the parameters of a layout call, as the three layout entry points of csrc/umap.hip require them."""
    if not 0 <= epoch_begin <= epoch_end <= n_epochs or n_epochs < 1:
        raise ValueError("0 <= epoch_begin <= epoch_end <= n_epochs expected")
    if not (a > 0 and b > 0 and gamma >= 0 and learning_rate >= 0 and 0 <= int(negative_sample_rate) <= 64):
        raise ValueError("a, b > 0, gamma, learning_rate >= 0 and 0 <= negative_sample_rate <= 64 expected")


def _check_layout_args(y, indptr, indices, q, a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate,
                       negative_sample_rate):
    """The validation `optimize_layout` and `optimize_layout_densmap` share; returns (n, dim)."""
    import torch

    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("y float32 [n, dim] expected")
    n, dim = y.shape
    if not 1 <= dim <= MAX_COMPONENTS:
        raise ValueError(f"1 <= dim <= {MAX_COMPONENTS} expected ({dim} given)")
    if indptr.dtype != torch.int32 or indices.dtype != torch.int32 or q.dtype != torch.int32:
        raise ValueError("indptr, indices and q must be int32")
    if indptr.shape != (n + 1,) or q.shape != indices.shape or indices.dim() != 1:
        raise ValueError("indptr [n + 1], indices [nnz] and q [nnz] expected")
    _check_csr(indptr, indices.numel())
    if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= n or int(q.min()) < 0 or int(q.max()) > 65536):
        raise ValueError("indices must lie in [0, n) and q in [0, 65536]")
    _check_schedule(a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate, negative_sample_rate)
    return n, dim


def _double_buffered(name: str, y, call):
    """The layout entry point `name` run as `call(buf_a, buf_b, result)` on a copy of y and a second buffer; returns the
    buffer that the int at `result` names as the one holding the new positions."""
    import torch

    bufs = (y.clone(), torch.empty_like(y))
    which = ctypes.c_int(0)
    check(call(ptr(bufs[0]), ptr(bufs[1]), ctypes.addressof(which)), name)
    return bufs[which.value]


def optimize_layout(y, indptr, indices, q, a: float, b: float, n_epochs: int, epoch_begin: int = 0,
                    epoch_end: Optional[int] = None, gamma: float = 1.0, learning_rate: float = 1.0, seed: int = 0,
                    negative_sample_rate: int = 5):
    """Epochs [epoch_begin, epoch_end) of `n_epochs` of the layout optimisation (csrc/umap.hip) from the positions
    y float32 [n, dim] over the symmetric CSR graph (indptr, indices int32) with sampling rates q (`sample_rates`).
    Returns the new positions; y is left unchanged.  Splitting the epoch range over several calls changes no bit."""
    require_gpu(y, indptr, indices, q)
    epoch_end = n_epochs if epoch_end is None else epoch_end
    n, dim = _check_layout_args(y, indptr, indices, q, a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate,
                                negative_sample_rate)
    return _double_buffered("wm_umap_layout", y, lambda buf_a, buf_b, result: _lib.load().wm_umap_layout(
        buf_a, buf_b, ptr(indptr), ptr(indices), ptr(q), n, dim, float(a), float(b), float(gamma), float(learning_rate),
        int(seed) & _MASK32, int(epoch_begin), int(epoch_end), int(n_epochs), int(negative_sample_rate), result, stream_ptr()))


def optimize_transform(y_new, y_train, idx, q, a: float, b: float, n_epochs: int, epoch_begin: int = 0,
                       epoch_end: Optional[int] = None, gamma: float = 1.0, learning_rate: float = 1.0, seed: int = 42,
                       negative_sample_rate: int = 5):
    """Epochs [epoch_begin, epoch_end) of `n_epochs` of the transform layout (csrc/umap.hip: wm_umap_transform_layout):
    the new points y_new float32 [m, dim] move among the fixed y_train float32 [n, dim] along their entries idx int32
    [m, k] in [0, n) with rates q int32 [m, k] in [0, 65536]; k <= 64.  All epochs of the call run in one launch.  Returns
    the new positions; both inputs are left unchanged.  Splitting the epoch range over several calls changes no bit."""
    import torch

    require_gpu(y_new, y_train, idx, q)
    epoch_end = n_epochs if epoch_end is None else epoch_end
    if y_new.dim() != 2 or y_train.dim() != 2 or y_new.dtype != torch.float32 or y_train.dtype != torch.float32:
        raise ValueError("y_new float32 [m, dim] and y_train float32 [n, dim] expected")
    (m, dim), n = y_new.shape, y_train.shape[0]
    if y_train.shape[1] != dim or not 1 <= dim <= MAX_COMPONENTS:
        raise ValueError(f"y_new and y_train must share 1 <= dim <= {MAX_COMPONENTS}")
    if m < 1 or n < 1:
        raise ValueError("at least one new and one fitted point expected")
    if idx.dtype != torch.int32 or q.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != m or q.shape != idx.shape:
        raise ValueError("idx int32 [m, k] and q int32 [m, k] expected")
    k = idx.shape[1]
    if not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"1 <= k <= {MAX_NEIGHBORS} expected ({k} given)")
    # the kernel trusts the entries: check once here that none points outside y_train
    if int(idx.min()) < 0 or int(idx.max()) >= n or int(q.min()) < 0 or int(q.max()) > 65536:
        raise ValueError("idx must lie in [0, n) and q in [0, 65536]")
    _check_schedule(a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate, negative_sample_rate)
    out = torch.empty_like(y_new)
    check(_lib.load().wm_umap_transform_layout(ptr(y_new), ptr(out), ptr(y_train), ptr(idx), ptr(q), m, n, k, dim, float(a),
                                               float(b), float(gamma), float(learning_rate), int(seed) & _MASK32,
                                               int(epoch_begin), int(epoch_end), int(n_epochs), int(negative_sample_rate),
                                               stream_ptr()), "wm_umap_transform_layout")
    return out


# ------------------------------------------------------------------------------------------------ DensMAP steps


def in_density_phase(epoch: int, n_epochs: int, dens_lambda: float, dens_frac: float) -> bool:
    """Whether 0-based `epoch` of `n_epochs` carries the density term (csrc/umap.hip evaluates the same expression)."""
    return bool(dens_lambda > 0 and (epoch + 1) / n_epochs > 1.0 - dens_frac)


def graph_radii(indptr, data, dists, q, n_epochs: int):
    """ro float32 [n]: the log of the weighted mean squared graph distance over each row's live entries (those sampled
    at least once in `n_epochs`), log 1e-8 for a row without one (csrc/umap.hip: wm_densmap_graph_radii)."""
    import torch

    require_gpu(indptr, data, dists, q)
    if indptr.dtype != torch.int32 or q.dtype != torch.int32 or data.dtype != torch.float32 or dists.dtype != torch.float32:
        raise ValueError("indptr, q int32 and data, dists float32 expected")
    if indptr.dim() != 1 or indptr.numel() < 2 or data.dim() != 1 or dists.shape != data.shape or q.shape != data.shape:
        raise ValueError("indptr [n + 1] and data, dists, q [nnz] expected")
    _check_csr(indptr, data.numel())
    if int(n_epochs) < 1:
        raise ValueError("n_epochs must be positive")
    n = indptr.numel() - 1
    ro = torch.empty(n, dtype=torch.float32, device=data.device)
    check(_lib.load().wm_densmap_graph_radii(ptr(indptr), ptr(data.contiguous()), ptr(dists.contiguous()), ptr(q.contiguous()), n,
                                             int(n_epochs), ptr(ro), stream_ptr()), "wm_densmap_graph_radii")
    return ro


def standardize_radii(ro):
    """R = (ro - mean) / std in double (population std), 0 when std = 0, as float32."""
    import torch

    r = ro.double()
    std = r.std(unbiased=False) if r.numel() > 1 else torch.zeros((), dtype=torch.float64, device=ro.device)
    if float(std) == 0.0:
        return torch.zeros_like(ro)
    return ((r - r.mean()) / std).float().contiguous()


def embedding_radii(y, indptr, indices, q, a: float, b: float, n_epochs: int):
    """(re, D) float32 [n] of the positions y float32 [n, dim] over the graph's live entries:
    D_i = 2 sum 1 / (1 + a r^b), re_i = log(1e-8 + N_i / D_i) with N_i = 2 sum r / (1 + a r^b), r the squared distance
    (csrc/umap.hip: wm_densmap_embedding_radii)."""
    import torch

    require_gpu(y, indptr, indices, q)
    n, dim = _check_layout_args(y, indptr, indices, q, a, b, n_epochs, 0, n_epochs, 0.0, 0.0, 0)
    re = torch.empty(n, dtype=torch.float32, device=y.device)
    d = torch.empty(n, dtype=torch.float32, device=y.device)
    check(_lib.load().wm_densmap_embedding_radii(ptr(y.contiguous()), ptr(indptr), ptr(indices), ptr(q), n, dim, float(a), float(b),
                                                 int(n_epochs), ptr(re), ptr(d), stream_ptr()), "wm_densmap_embedding_radii")
    return re, d


class DensityTerms(NamedTuple):
    """What the last density-phase epoch of an `optimize_layout_densmap` call computed from the positions before it:
    per vertex float32 [n] 1 / D, 1 / (1e-8 + N / D), W and re, the float32 scalar `scale` =
    dens_lambda mu_tot / (std n) the layout kernel multiplies with, and mu_tot, mean, var, cov, std in float64."""

    inv_d: "object"
    inv_den: "object"
    w: "object"
    re: "object"
    scale: float
    mu_tot: float
    mean: float
    var: float
    cov: float
    std: float


# Where wm_densmap_layout leaves them in its workspace (csrc/umap.hip, "Workspace of wm_densmap_layout"), in bytes:
_WS_SCALARS = 0  # float64 mu_tot, mean, var, cov, std
_WS_SCALE = 40  # float32 s
_WS_VERTEX = 64 + 4 * 128 * 8  # float32 [n][4], behind the scalars and the four rows of 128 float64 slots


def optimize_layout_densmap(y, indptr, indices, q, data, R, a: float, b: float, n_epochs: int, epoch_begin: int = 0,
                            epoch_end: Optional[int] = None, gamma: float = 1.0, learning_rate: float = 1.0, seed: int = 0,
                            negative_sample_rate: int = 5, dens_lambda: float = 2.0, dens_frac: float = 0.3,
                            dens_var_shift: float = 0.1, return_terms: bool = False):
    """`optimize_layout` with DensMAP's density term in the epochs of the density phase (`in_density_phase`): `data`
    float32 [nnz] > 0 are the graph's weights and `R` float32 [n] the standardised graph radii (`graph_radii`,
    `standardize_radii`).  Epochs outside the phase, and every epoch when dens_lambda = 0, are `optimize_layout`'s bit for
    bit; splitting the epoch range over several calls changes no bit.  With `return_terms` the result is
    (positions, DensityTerms or None when the call ran no phase epoch)."""
    import torch

    require_gpu(y, indptr, indices, q, data, R)
    epoch_end = n_epochs if epoch_end is None else epoch_end
    n, dim = _check_layout_args(y, indptr, indices, q, a, b, n_epochs, epoch_begin, epoch_end, gamma, learning_rate,
                                negative_sample_rate)
    if n < 2:
        raise ValueError("at least 2 vertices expected")
    if data.dtype != torch.float32 or R.dtype != torch.float32 or data.shape != indices.shape or R.shape != (n,):
        raise ValueError("data float32 [nnz] and R float32 [n] expected")
    # (an explicit zero of a label-intersected graph has rate 0: it is never sampled and never live, so never divided by)
    if data.numel() and not bool((torch.isfinite(data) & ((data > 0) | ((data == 0) & (q == 0)))).all()):
        raise ValueError("data must be positive and finite (0 only where the rate is 0)")
    if not bool(torch.isfinite(R).all()):
        raise ValueError("R must be finite")
    if not (dens_lambda >= 0 and 0 <= dens_frac <= 1 and dens_var_shift >= 0):
        raise ValueError("dens_lambda >= 0, 0 <= dens_frac <= 1 and dens_var_shift >= 0 expected")
    lib = _lib.load()
    need = lib.wm_densmap_layout_workspace_bytes(n)
    if need == 0:
        raise ValueError(f"optimize_layout_densmap: unsupported n = {n}")
    ws = torch.zeros(need, dtype=torch.uint8, device=y.device)
    out = _double_buffered("wm_densmap_layout", y, lambda buf_a, buf_b, result: lib.wm_densmap_layout(
        buf_a, buf_b, ptr(indptr), ptr(indices), ptr(q), ptr(data.contiguous()), ptr(R.contiguous()), n, int(indices.numel()), dim,
        float(a), float(b), float(gamma), float(learning_rate), float(dens_lambda), float(dens_frac), float(dens_var_shift),
        int(seed) & _MASK32, int(epoch_begin), int(epoch_end), int(n_epochs), int(negative_sample_rate), ptr(ws), need, result,
        stream_ptr()))
    if not return_terms:
        return out
    if not any(in_density_phase(ep, n_epochs, dens_lambda, dens_frac) for ep in range(epoch_begin, epoch_end)):
        return out, None
    vert = ws[_WS_VERTEX:_WS_VERTEX + 16 * n].view(torch.float32).view(n, 4)
    scal = ws[_WS_SCALARS:_WS_SCALARS + 40].view(torch.float64).cpu().tolist()
    scale = float(ws[_WS_SCALE:_WS_SCALE + 4].view(torch.float32).cpu()[0])
    return out, DensityTerms(*(vert[:, c].contiguous() for c in range(4)), scale, *scal)


# ------------------------------------------------------------------------------------------------ initialisation


def _spectral_init(graph: CSR, dim: int):
    """umap-learn's spectral_layout for a connected graph: the eigenvectors 1 .. dim of the normalised Laplacian
    (scipy eigsh on the host).  None when the graph is disconnected or eigsh does not converge."""
    import scipy.sparse
    import scipy.sparse.csgraph
    import scipy.sparse.linalg

    g = graph.to_scipy().astype(np.float64)
    g.eliminate_zeros()  # (the explicit zeros a label intersection leaves are no edges)
    n = g.shape[0]
    if n <= dim + 1 or scipy.sparse.csgraph.connected_components(g, directed=False)[0] != 1:
        return None
    deg = np.asarray(g.sum(axis=0)).ravel()
    d_inv = scipy.sparse.diags(1.0 / np.sqrt(deg))
    lap = scipy.sparse.identity(n, dtype=np.float64) - d_inv @ g @ d_inv
    k = dim + 1
    try:
        vals, vecs = scipy.sparse.linalg.eigsh(lap, k, which="SM", ncv=min(n - 1, max(2 * k + 1, int(np.sqrt(n)))), tol=1e-4,
                                               v0=np.ones(n), maxiter=n * 5)
    except (scipy.sparse.linalg.ArpackError, scipy.sparse.linalg.ArpackNoConvergence):
        return None
    return vecs[:, np.argsort(vals)[1:k]]


def _pca_init(x, dim: int):
    import torch

    xc = x.double() - x.double().mean(dim=0, keepdim=True)
    u, s, _ = torch.linalg.svd(xc, full_matrices=False)
    out = torch.zeros((x.shape[0], dim), dtype=torch.float64, device=x.device)
    m = min(dim, s.numel())
    out[:, :m] = u[:, :m] * s[:m]
    return out


# ------------------------------------------------------------------------------------------------ estimator


class UMAP:
    """umap.UMAP on device tensors: `.fit(x)` / `.fit_transform(x)` give float32 [n, n_components] on the device and
    set `embedding_`, `graph_` (CSR), `a_`, `b_`.  `n_epochs=None` means 500 for at most 10 000 rows and 200 above.
    `init`: "spectral" (falls back to "pca" with a warning when the graph is disconnected or eigsh does not
    converge), "pca", "random" or an [n, n_components] array."""

    def __init__(self, n_neighbors: int = 15, n_components: int = 2, metric: str = "euclidean", n_epochs: Optional[int] = None,
                 learning_rate: float = 1.0, init="spectral", min_dist: float = 0.1, spread: float = 1.0,
                 negative_sample_rate: int = 5, repulsion_strength: float = 1.0, random_state: int = 0,
                 local_connectivity: float = 1.0, set_op_mix_ratio: float = 1.0, densmap: bool = False):
        metric_code(metric)
        if densmap:
            raise NotImplementedError("densmap=True is not a switch of this class: use manifold.DensMAP")
        if float(local_connectivity) != 1.0 or float(set_op_mix_ratio) != 1.0:
            raise ValueError("only local_connectivity=1.0 and set_op_mix_ratio=1.0 are supported")
        if not 2 <= int(n_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors must be in [2, {MAX_NEIGHBORS}]")
        if not 1 <= int(n_components) <= MAX_COMPONENTS:
            raise ValueError(f"n_components must be in [1, {MAX_COMPONENTS}]")
        if n_epochs is not None and int(n_epochs) < 1:
            raise ValueError("n_epochs must be positive")
        if not (min_dist >= 0 and spread > 0 and min_dist <= spread):
            raise ValueError("0 <= min_dist <= spread and spread > 0 required")
        if not (learning_rate > 0 and repulsion_strength >= 0 and 0 <= int(negative_sample_rate) <= 64):
            raise ValueError("learning_rate > 0, repulsion_strength >= 0 and 0 <= negative_sample_rate <= 64 required")
        if isinstance(init, str) and init not in ("spectral", "pca", "random"):
            raise ValueError("init must be 'spectral', 'pca', 'random' or an array")
        self.n_neighbors, self.n_components, self.metric = int(n_neighbors), int(n_components), metric
        self.n_epochs = None if n_epochs is None else int(n_epochs)
        self.learning_rate, self.init, self.min_dist, self.spread = float(learning_rate), init, float(min_dist), float(spread)
        self.negative_sample_rate, self.repulsion_strength = int(negative_sample_rate), float(repulsion_strength)
        self.random_state = int(random_state)
        self.a_, self.b_ = find_ab_params(self.spread, self.min_dist)
        self.embedding_ = self.graph_ = None

    def _initial(self, x, graph: CSR):
        import torch

        n, dim = x.shape[0], self.n_components
        rng = np.random.default_rng(self.random_state)
        init = self.init
        if not isinstance(init, str):
            y = torch.as_tensor(np.asarray(init.cpu() if hasattr(init, "cpu") else init), dtype=torch.float64)
            if y.shape != (n, dim):
                raise ValueError(f"init array must be [{n}, {dim}]")
            y = y.to(x.device)
        elif init == "random":
            y = torch.from_numpy(rng.uniform(-10.0, 10.0, (n, dim))).to(x.device)
        else:
            y = None
            if init == "spectral":
                vecs = _spectral_init(graph, dim)
                if vecs is None:
                    warnings.warn("UMAP: spectral initialisation failed (the graph is disconnected or eigsh did not "
                                  "converge); falling back to init='pca'")
                else:
                    y = torch.from_numpy(vecs).to(x.device)
            if y is None:
                y = _pca_init(x, dim)
            top = float(y.abs().max())
            y = y * (10.0 / top if top > 0 else 1.0) + torch.from_numpy(rng.normal(0.0, 1e-4, (n, dim))).to(x.device)
        lo, hi = y.min(dim=0).values, y.max(dim=0).values
        span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
        return (10.0 * (y - lo) / span).float().contiguous()

    def _checked(self, x, y):
        if y is not None:
            raise NotImplementedError(f"y= (semi-supervised UMAP) is not implemented by this class: use manifold.Inductive{type(self).__name__}")
        x = _prep(x)
        if x.shape[0] < 2:
            raise ValueError("UMAP needs at least 2 rows")
        return x

    def _target_graph(self, graph: CSR) -> CSR:
        """The graph the layout sees: the fuzzy simplicial set itself (the Inductive classes intersect it with y)."""
        return graph

    def fit(self, x, y=None) -> "UMAP":
        x = self._checked(x, y)
        n = x.shape[0]
        graph = self._target_graph(fuzzy_simplicial_set(x, min(self.n_neighbors, n), self.metric))
        n_epochs = self.n_epochs if self.n_epochs is not None else (500 if n <= 10000 else 200)
        self.graph_ = graph
        self.embedding_ = optimize_layout(self._initial(x, graph), graph.indptr, graph.indices, sample_rates(graph.data),
                                          self.a_, self.b_, n_epochs, gamma=self.repulsion_strength,
                                          learning_rate=self.learning_rate, seed=self.random_state,
                                          negative_sample_rate=self.negative_sample_rate)
        return self

    def fit_transform(self, x, y=None):
        return self.fit(x, y).embedding_

    def transform(self, x):
        raise NotImplementedError("transform of new rows is not implemented by this class (fit_transform embeds the fitted "
                                  f"rows): use manifold.Inductive{type(self).__name__}")


class DensMAP(UMAP):
    """umap.UMAP(densmap=True, ...): UMAP whose last `dens_frac` of the epochs also pull the embedding's local radii
    towards the data's (`optimize_layout_densmap`).  `UMAP`'s arguments plus umap-learn's dens_lambda = 2.0,
    dens_frac = 0.3, dens_var_shift = 0.1; `n_epochs=None` means 700 for at most 10 000 rows and 400 above (umap-learn adds
    200 epochs for densmap).  After `fit`, `rad_orig_` holds the graph's radii ro and `rad_emb_` the embedding's radii re
    at the final positions, float32 [n] on the device."""

    def __init__(self, *args, dens_lambda: float = 2.0, dens_frac: float = 0.3, dens_var_shift: float = 0.1, **kwargs):
        if "densmap" in kwargs or len(args) > 13:
            raise ValueError("DensMAP takes no densmap= argument: the class is the switch")
        super().__init__(*args, **kwargs)
        if not (dens_lambda >= 0 and 0 <= dens_frac <= 1 and dens_var_shift >= 0):
            raise ValueError("dens_lambda >= 0, 0 <= dens_frac <= 1 and dens_var_shift >= 0 required")
        self.dens_lambda, self.dens_frac, self.dens_var_shift = float(dens_lambda), float(dens_frac), float(dens_var_shift)
        self.rad_orig_ = self.rad_emb_ = None

    def default_epochs(self, n: int) -> int:
        return self.n_epochs if self.n_epochs is not None else (700 if n <= 10000 else 400)

    def fit(self, x, y=None) -> "DensMAP":
        x = self._checked(x, y)
        n = x.shape[0]
        graph, dists = fuzzy_simplicial_set(x, min(self.n_neighbors, n), self.metric, return_dists=True)
        graph = self._target_graph(graph)  # (the pattern is kept: dists stay aligned)
        n_epochs = self.default_epochs(n)
        q = sample_rates(graph.data)
        self.graph_ = graph
        self.rad_orig_ = graph_radii(graph.indptr, graph.data, dists, q, n_epochs)
        self.embedding_ = optimize_layout_densmap(
            self._initial(x, graph), graph.indptr, graph.indices, q, graph.data, standardize_radii(self.rad_orig_), self.a_,
            self.b_, n_epochs, gamma=self.repulsion_strength, learning_rate=self.learning_rate, seed=self.random_state,
            negative_sample_rate=self.negative_sample_rate, dens_lambda=self.dens_lambda, dens_frac=self.dens_frac,
            dens_var_shift=self.dens_var_shift)
        self.rad_emb_ = embedding_radii(self.embedding_, graph.indptr, graph.indices, q, self.a_, self.b_, n_epochs)[0]
        return self


# ------------------------------------------------------------------------------------------------ y= and transform


def _checked_labels(y, n: int):
    """y= of a fit as an int32 [n] tensor where it lives: a numpy array or a tensor (host or device) of integer values
    >= -1."""
    import torch

    t = y.detach() if isinstance(y, torch.Tensor) else None
    if t is None:
        arr = np.asarray(y)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"y must hold integers (-1: unknown), not {arr.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64)))
    elif t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"y must hold integers (-1: unknown), not {t.dtype}")
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"y must have one label per row ([{n}]), not {tuple(t.shape)}")
    t = t.to(torch.int64)
    if n and (int(t.min()) < -1 or int(t.max()) > 2 ** 31 - 1):
        raise ValueError("labels must be >= -1 (-1: unknown) and fit int32")
    return t.to(torch.int32).contiguous()


class _Inductive:
    """What `InductiveUMAP` and `InductiveDensMAP` add to their parents (mixed in before them): the target arguments,
    the label intersection of the graph that the parents' `fit(x, y)` lays out, and `transform`."""

    def __init__(self, *args, target_weight: float = 0.5, target_metric: str = "categorical", transform_seed: int = 42, **kwargs):
        super().__init__(*args, **kwargs)
        if target_metric != "categorical":
            raise NotImplementedError(f"target_metric {target_metric!r} is not implemented (available: 'categorical')")
        if not 0.0 <= float(target_weight) <= 1.0:
            raise ValueError("0 <= target_weight <= 1 required")
        self.target_weight, self.target_metric, self.transform_seed = float(target_weight), target_metric, int(transform_seed)
        self._labels = self._train = None

    def _checked(self, x, y):
        # labels first: a bad y is a ValueError whatever x is; an x that is no 2-D device tensor is refused right after
        labels = _checked_labels(y, x.shape[0]) if y is not None and getattr(x, "ndim", 0) == 2 else None
        x = super()._checked(x, None)
        self._labels = None if labels is None else labels.to(x.device)
        self._train = x
        return x

    def _target_graph(self, graph: CSR) -> CSR:
        if self._labels is None:
            return graph
        return label_intersect(graph, self._labels, far_distance(self.target_weight))

    def transform_epochs(self, m: int) -> int:
        if self.n_epochs is not None:
            return max(1, self.n_epochs // 3)
        return 100 if m <= 10000 else 30

    def transform_graph(self, x):
        """(idx int32 [m, k], weights float32 [m, k]) of the new rows x among the fitted rows."""
        if self.embedding_ is None or self._train is None:
            raise ValueError("transform needs a fitted model: call fit first")
        if not hasattr(x, "is_cuda") or not x.is_cuda:
            raise ValueError("transform needs a device tensor")
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("expected [n_samples >= 1, n_features]")
        x = _prep(x)
        if x.shape[1] != self._train.shape[1]:
            raise ValueError(f"x has {x.shape[1]} (padded) features, the model was fitted on {self._train.shape[1]}")
        dist, idx = knn_query(x, self._train, min(self.n_neighbors, self._train.shape[0]), self.metric)
        return idx, smooth_knn_query(dist)[1]

    def transform_init(self, idx, w):
        """umap-learn 0.5.3's init_transform: sum_j w_j Y_j / sum_j w_j, in double, rounded once (the plain mean of the
        neighbours where every weight underflowed to 0)."""
        import torch

        wd = w.double()
        tot = wd.sum(dim=1, keepdim=True)
        wd = torch.where(tot > 0, wd / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.full_like(wd, 1.0 / w.shape[1]))
        return (wd.unsqueeze(2) * self.embedding_.double()[idx.long()]).sum(dim=1).float().contiguous()

    def transform(self, x):
        """Positions float32 [m, n_components] of new rows x [m, d] (device tensor) in the fitted embedding, which does
        not move: umap-learn's UMAP.transform (exact kNN among the fitted rows, rho = 0 memberships, weighted-average
        start, n_epochs // 3 -- or 100, 30 above 10 000 rows -- layout epochs at a quarter of the learning rate with
        seed `transform_seed`).  Two calls give the same bits."""
        idx, w = self.transform_graph(x)
        return optimize_transform(self.transform_init(idx, w), self.embedding_, idx, sample_rates(w), self.a_, self.b_,
                                  self.transform_epochs(idx.shape[0]), gamma=self.repulsion_strength,
                                  learning_rate=self.learning_rate, seed=self.transform_seed,
                                  negative_sample_rate=self.negative_sample_rate)


class InductiveUMAP(_Inductive, UMAP):
    """`UMAP` with `fit(x, y)` and `transform(x)`: `UMAP`'s arguments plus umap-learn's target_weight = 0.5,
    target_metric = "categorical" and transform_seed = 42.  y: one integer label per row, -1 where unknown (numpy array
    or tensor); the fuzzy graph is intersected with the labels (`label_intersect`) before the initialisation, so the
    spectral start and the layout see the intersected graph.  With y=None the fit is `UMAP`'s bit for bit."""


class InductiveDensMAP(_Inductive, DensMAP):
    """`DensMAP` with `fit(x, y)` and `transform(x)` (see `InductiveUMAP`); the graph distances stay aligned with the
    intersected graph because its pattern is kept.  `transform` places new rows into the DensMAP embedding by the plain
    transform layout, without a density term: recent umap-learn releases refuse transform for densmap=True, but notebook
    3.0-Embeddings-inference calls it on such a model, so it is provided."""
