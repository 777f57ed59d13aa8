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

Laplacian eigenmaps of a graph (`laplacian_eigenpairs`, `spectral_layout`, `SpectralEmbedding`, and
`cluster.SpectralClustering` on top of them; `init="spectral_device"` of the estimators above):
  8. a thick-restart Lanczos eigensolver with full reorthogonalisation on N = D^-1/2 G D^-1/2 in float64
     (csrc/spectral.hip: wm_spec_degree, wm_spec_matvec, wm_spec_orthonormalise, wm_spec_rotate); the eigenvalue-0 pairs of
     the connected components (found by scipy on the host) are deflated in closed form; the host takes numpy's eigh of the
     small matrix T once per restart cycle, the cycle's only synchronisation.  Two solves give the same bits.
`init="spectral"` keeps the host path below.

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


# ------------------------------------------------------------------------------------------------ Laplacian eigenmaps

SPEC_MAX_BASIS = 255  # Lanczos steps per cycle the kernels take (the basis has one more column, 256 at most)
SPEC_MAX_COMPONENTS = 256  # connected components whose trivial vectors the device solver deflates
SPEC_DENSE_ROWS = 512  # graphs of at most this many rows are solved densely on the host


def _check_graph(graph: CSR) -> int:
    """What the spectral kernels trust about a graph, checked once on the host; returns n."""
    import torch

    require_gpu(graph.indptr, graph.indices, graph.data)
    if graph.indptr.dtype != torch.int32 or graph.indices.dtype != torch.int32 or graph.data.dtype != torch.float32:
        raise ValueError("graph: indptr, indices int32 and data float32 expected")
    if graph.indptr.dim() != 1 or graph.indptr.numel() < 2 or graph.indices.dim() != 1 or graph.indices.shape != graph.data.shape:
        raise ValueError("graph: indptr [n + 1], indices [nnz] and data [nnz] expected")
    n = graph.indptr.numel() - 1
    _check_csr(graph.indptr, graph.indices.numel())
    if graph.indices.numel() and (int(graph.indices.min()) < 0 or int(graph.indices.max()) >= n):
        raise ValueError("indices must lie in [0, n)")
    return n


def _token_ws(need: int, what: str, device, ws=None):
    """(workspace, byte count) of an entry point that stores nothing in its workspace: `ws` when the caller keeps one
    (`token_workspace`, once per solve), else a new tensor.  ValueError(what) for sizes the kernel does not take."""
    if ws is None or need == 0 or ws.numel() < need:
        ws = workspace(need, what, device)
    return ws, need


def token_workspace(device):
    """The 256 bytes that `laplacian_degree`, `laplacian_matvec` and `basis_rotate` ask for and never touch; a caller
    that issues many of them allocates it once and passes it as `ws`."""
    return workspace(256, "token workspace", device)


def laplacian_degree(graph: CSR, ws=None):
    """(deg, dinv) float64 [n] on the device: the row sums of `graph` in column order and 1 / sqrt(deg), 0 for an empty
    row (csrc/spectral.hip: wm_spec_degree)."""
    import torch

    n = _check_graph(graph)
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_spec_degree_workspace_bytes(n), f"laplacian_degree: unsupported n = {n}", graph.data.device, ws)
    deg = torch.empty(n, dtype=torch.float64, device=graph.data.device)
    dinv = torch.empty_like(deg)
    check(lib.wm_spec_degree(ptr(graph.indptr), ptr(graph.data), n, ptr(deg), ptr(dinv), ptr(ws), need, stream_ptr()),
          "wm_spec_degree")
    return deg, dinv


def _basis_column(v, col: int):
    """(pointer, pitch) of column `col` of a row-major float64 basis [n, ld], or of a plain vector [n] (col = 0)."""
    import torch

    require_gpu(v)
    if v.dtype != torch.float64 or v.dim() not in (1, 2):
        raise ValueError("a float64 vector [n] or basis [n, ld] expected")
    ld = 1 if v.dim() == 1 else v.shape[1]
    if not 0 <= col < ld:
        raise ValueError(f"column {col} outside the basis of {ld}")
    return ptr(v) + 8 * col, ld


def laplacian_matvec(graph: CSR, dinv, v, col: int = 0, out=None, checked: bool = False, ws=None):
    """w = D^-1/2 G D^-1/2 v float64 [n] on the device (wm_spec_matvec); v is a vector [n] or column `col` of a basis
    [n, ld].  `checked`: the caller has validated the graph already; `ws`: the caller's `token_workspace`."""
    import torch

    n = graph.indptr.numel() - 1 if checked else _check_graph(graph)
    vp, ld = _basis_column(v, col)
    require_gpu(dinv)
    if dinv.dtype != torch.float64 or dinv.shape != (n,) or v.shape[0] != n:
        raise ValueError(f"dinv float64 [{n}] and v with {n} rows expected")
    out = torch.empty(n, dtype=torch.float64, device=v.device) if out is None else out
    if out.dtype != torch.float64 or out.shape != (n,) or not out.is_contiguous():
        raise ValueError(f"out float64 [{n}] expected")
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_spec_matvec_workspace_bytes(n), f"laplacian_matvec: unsupported n = {n}", v.device, ws)
    check(lib.wm_spec_matvec(ptr(graph.indptr), ptr(graph.indices), ptr(graph.data), ptr(dinv), vp, ld, n, ptr(out), ptr(ws),
                             need, stream_ptr()), "wm_spec_matvec")
    return out


def lanczos_workspace(n: int, ldv: int, ncomp: int, device):
    """The workspace of `lanczos_orthonormalise` for these sizes, allocated once per solve."""
    need = _lib.load().wm_spec_orthonormalise_workspace_bytes(int(n), int(ldv), int(ncomp))
    return workspace(need, f"lanczos: unsupported sizes n={n} basis={ldv} (<= {SPEC_MAX_BASIS + 1}) components={ncomp} "
                           f"(<= {SPEC_MAX_COMPONENTS})", device)


def lanczos_orthonormalise(w, V, j: int, comp, ncomp: int, u, T, m: int, ws=None):
    """The tail of Lanczos step j in place (wm_spec_orthonormalise): w float64 [n] is orthogonalised twice against the
    unit trivial vectors u float64 [n] (component labels comp int32 [n] in [0, ncomp)) and against V[:, :j + 1] (V float64
    [n, ldv], m < ldv); the summed coefficients go to T[:j + 1, j], |w| to T[j + 1, j] and T.flat[m m], w / |w| to
    V[:, j + 1].  T float64 [m m + 2]: the flag word T[m m + 1] (int64) is set to j + 1 on a breakdown."""
    import torch

    require_gpu(w, V, comp, u, T)
    if V.dim() != 2 or V.dtype != torch.float64 or w.dtype != torch.float64 or u.dtype != torch.float64 or T.dtype != torch.float64:
        raise ValueError("w, u float64 [n], V float64 [n, ldv] and T float64 expected")
    n, ldv = V.shape
    if w.shape != (n,) or u.shape != (n,) or comp.shape != (n,) or comp.dtype != torch.int32:
        raise ValueError(f"w, u float64 [{n}] and comp int32 [{n}] expected")
    if not (0 <= j < m < ldv) or T.numel() != m * m + 2:
        raise ValueError("0 <= j < m < ldv and T of m m + 2 cells expected")
    ws = lanczos_workspace(n, ldv, ncomp, V.device) if ws is None else ws
    check(_lib.load().wm_spec_orthonormalise(ptr(w), ptr(V), n, ldv, int(j), ptr(comp), int(ncomp), ptr(u), ptr(T), int(m), ptr(ws),
                                             ws.numel(), stream_ptr()), "wm_spec_orthonormalise")


def basis_rotate(V, S, m: Optional[int] = None, out=None, ws=None):
    """out[:, :q] = V[:, :m] @ S float64 on the device (wm_spec_rotate): V [n, ldv], S [m, q] (tensor or numpy array);
    `out` a second buffer [n, ldo >= q] (a new [n, q] when None).  Returns out."""
    import torch

    S = torch.as_tensor(np.ascontiguousarray(S) if isinstance(S, np.ndarray) else S, dtype=torch.float64).to(V.device).contiguous()
    require_gpu(V, S)
    if V.dim() != 2 or S.dim() != 2 or V.dtype != torch.float64:
        raise ValueError("V float64 [n, ldv] and S float64 [m, q] expected")
    m = S.shape[0] if m is None else int(m)
    (n, ldv), q = V.shape, S.shape[1]
    if S.shape[0] != m or not 1 <= m <= ldv or q < 1:
        raise ValueError(f"S [{m}, q >= 1] with m <= {ldv} expected")
    out = torch.empty((n, q), dtype=torch.float64, device=V.device) if out is None else out
    require_gpu(out)
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] != n or out.shape[1] < q or out.data_ptr() == V.data_ptr():
        raise ValueError(f"out float64 [{n}, >= {q}], not V itself, expected")
    lib = _lib.load()
    ws, need = _token_ws(lib.wm_spec_rotate_workspace_bytes(n, m, q), f"basis_rotate: unsupported sizes n={n} m={m} q={q}", V.device, ws)
    check(lib.wm_spec_rotate(ptr(V), ldv, ptr(S), q, n, m, q, ptr(out), out.shape[1], ptr(ws), need, stream_ptr()), "wm_spec_rotate")
    return out


def graph_components(graph: CSR):
    """(ncomp, labels int32 [n]) of the graph's connected components on the host (scipy), explicit zeros being no edges;
    the labels are numbered by each component's smallest row."""
    import scipy.sparse.csgraph

    g = graph.to_scipy().copy()  # (host tensors share their memory with scipy's arrays: never edit the caller's graph)
    g.eliminate_zeros()
    ncomp, labels = scipy.sparse.csgraph.connected_components(g, directed=False)
    first = np.unique(labels, return_index=True)[1]
    rank = np.empty(ncomp, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(ncomp)
    return int(ncomp), rank[labels].astype(np.int32)


def trivial_vectors(deg, labels, ncomp: int):
    """u float64 [n] (numpy): sqrt(deg) normalised within each component -- the eigenvalue-0 vectors of the normalised
    Laplacian, all in one array because their supports are disjoint."""
    deg = np.asarray(deg, dtype=np.float64)
    return np.sqrt(deg) / np.sqrt(np.bincount(labels, weights=deg, minlength=ncomp))[labels]


def lanczos_start(labels, ncomp: int, u):
    """The fixed start vector float64 [n] (numpy): 1 + frac(i phi), a low-discrepancy function of the row index alone, made
    orthogonal to every component's u and normalised.  It has mass in every component of at least two rows."""
    n = labels.shape[0]
    x = 1.0 + np.modf(np.arange(n, dtype=np.float64) * 0.6180339887498949)[0]
    for _ in range(2):
        x = x - u * np.bincount(labels, weights=u * x, minlength=ncomp)[labels]
    return x / np.linalg.norm(x)


class Eigenpairs(NamedTuple):
    """What `laplacian_eigenpairs` returns: the k smallest NONTRIVIAL eigenvalues of I - D^-1/2 G D^-1/2 ascending (numpy
    float64 [k]) with their unit eigenvectors (float64 [n, k] on the device) and the residuals |N y - theta y| the solver
    stopped on (numpy [k]); the trivial pairs (eigenvalue 0, one per component) as `trivial` float64 [n] on the device
    with `labels` int32 [n] -- column c of the trivial vectors is `trivial` on the rows labelled c, components numbered by
    their smallest row (`trivial_matrix`); the counts; `converged`."""
    eigenvalues: np.ndarray
    eigenvectors: "object"
    residuals: np.ndarray
    trivial: "object"
    labels: "object"
    n_components: int
    cycles: int
    matvecs: int
    converged: bool

    def trivial_matrix(self):
        """The trivial eigenvectors as float64 [n, n_components] on the device."""
        return _trivial_matrix(self.trivial, self.labels, self.n_components)


def _trivial_matrix(u, comp, ncomp: int):
    """u float64 [n] spread over the columns its labels comp int32 [n] name: float64 [n, ncomp] on u's device."""
    import torch

    out = torch.zeros((u.shape[0], ncomp), dtype=torch.float64, device=u.device)
    out.scatter_(1, comp.long().unsqueeze(1), u.unsqueeze(1))
    return out


def _dense_eigenpairs(graph: CSR, k: int, labels, ncomp: int, u):
    """The host solve of small problems: numpy eigh of the float64 N with the trivial vectors shifted to -3, below its
    spectrum [-1, 1].  (theta descending [k], vectors [n, k])."""
    g = graph.to_scipy().astype(np.float64)
    deg = np.asarray(g.sum(axis=1)).ravel()
    dinv = 1.0 / np.sqrt(deg)
    dense = dinv[:, None] * g.toarray() * dinv[None, :]
    dense = 0.5 * (dense + dense.T)
    um = np.zeros((labels.shape[0], ncomp))
    um[np.arange(labels.shape[0]), labels] = u
    theta, vecs = np.linalg.eigh(dense - 3.0 * (um @ um.T))
    return theta[::-1][:k].copy(), np.ascontiguousarray(vecs[:, ::-1][:, :k])


def laplacian_eigenpairs(graph: CSR, k: int, tol: float = 1e-6, ncv: Optional[int] = None, max_cycles: int = 300) -> Eigenpairs:
    """The k smallest nontrivial eigenpairs of the normalised Laplacian I - N, N = D^-1/2 G D^-1/2, of the symmetric CSR
    `graph`: thick-restart Lanczos with full reorthogonalisation on the device in float64 (csrc/spectral.hip).  The trivial
    pairs (one per connected component, found on the host) are known in closed form and deflated, so one Krylov sequence
    serves a disconnected graph.  A cycle runs Lanczos steps up to m = ncv or max(2k + 2, 64) basis vectors, reads T, beta
    and the breakdown flag in one copy (the only synchronisation), takes numpy's eigh of T, and stops when the first k
    residuals |beta S[m - 1, i]| are at most `tol` (absolute: |N| = 1); otherwise it keeps q = k + (m - k) // 2 Ritz
    vectors (wm_spec_rotate) and the residual vector, resets T to diag(theta) and goes on from column q, whose step
    computes the arrow coefficients itself.  The start vector is a fixed function of
    the row index: two calls give the same bits.  Graphs of at most 512 rows, and sizes with n - components <= m + 1, are
    solved densely on the host.  `converged` is False when `max_cycles` ran out (the pairs are the current Ritz pairs)."""
    import torch

    n = _check_graph(graph)
    k, max_cycles = int(k), int(max_cycles)
    if k < 1 or max_cycles < 1 or not tol >= 0:
        raise ValueError("k >= 1, max_cycles >= 1 and tol >= 0 expected")
    m = int(ncv) if ncv is not None else max(2 * k + 2, 64)
    if m <= k:
        raise ValueError(f"ncv ({m}) must exceed k ({k})")
    dev = graph.data.device
    ncomp, labels = graph_components(graph)
    if k > n - ncomp:
        raise ValueError(f"k ({k}) exceeds the {n - ncomp} nontrivial eigenpairs of {n} rows in {ncomp} components")
    token = token_workspace(dev)  # what degree, matvec and rotate ask for and never touch: once per solve
    deg, dinv = laplacian_degree(graph, token)
    deg_h = deg.cpu().numpy()
    if not (deg_h > 0).all():
        raise ValueError("every row of the graph needs a positive degree")
    u_h = trivial_vectors(deg_h, labels, ncomp)
    u, comp = torch.from_numpy(u_h).to(dev), torch.from_numpy(labels).to(dev)
    if n <= SPEC_DENSE_ROWS or n - ncomp <= m + 1:
        theta, vecs = _dense_eigenpairs(graph, k, labels, ncomp, u_h)
        return Eigenpairs(1.0 - theta, torch.from_numpy(vecs).to(dev), np.zeros(k), u, comp, ncomp, 0, 0, True)
    if m > SPEC_MAX_BASIS or ncomp > SPEC_MAX_COMPONENTS:
        raise ValueError(f"the device solver takes at most {SPEC_MAX_BASIS} basis vectors ({m} asked for: lower k or ncv) and "
                         f"{SPEC_MAX_COMPONENTS} connected components ({ncomp} found: raise n_neighbors)")
    ldv = m + 1
    V, spare = torch.zeros((n, ldv), dtype=torch.float64, device=dev), torch.zeros((n, ldv), dtype=torch.float64, device=dev)
    V[:, 0] = torch.from_numpy(lanczos_start(labels, ncomp, u_h)).to(dev)
    w = torch.empty(n, dtype=torch.float64, device=dev)
    T = torch.zeros(m * m + 2, dtype=torch.float64, device=dev)
    ws = lanczos_workspace(n, ldv, ncomp, dev)
    begin, matvecs = 0, 0
    for cycle in range(1, max_cycles + 1):
        for j in range(begin, m):
            laplacian_matvec(graph, dinv, V, j, out=w, checked=True, ws=token)
            lanczos_orthonormalise(w, V, j, comp, ncomp, u, T, m, ws)
        matvecs += m - begin
        t_h = T.cpu().numpy()  # the cycle's one synchronisation
        flag = int(t_h[m * m + 1:].view(np.int64)[0])
        mm, beta = (flag, 0.0) if flag else (m, float(t_h[m * m]))  # a breakdown at step flag - 1: an invariant subspace
        theta, S = np.linalg.eigh(t_h[:m * m].reshape(m, m)[:mm, :mm], UPLO="U")
        theta, S = theta[::-1], S[:, ::-1]
        kk = min(k, mm)
        resid = np.abs(beta * S[mm - 1, :kk])
        done = bool(flag) or bool((resid <= tol).all())
        if done or cycle == max_cycles:
            break
        q = k + (m - k) // 2
        basis_rotate(V, S[:, :q], m, out=spare, ws=token)
        spare[:, q] = V[:, m]
        V, spare = spare, V
        # T restarts as diag(theta); the arrow beta S[m - 1, :q] is not filled in: step q's full orthogonalisation computes
        # V[:, :q]^T N v_q, which is that arrow, into column q above the diagonal, the triangle eigh reads
        t_new = np.zeros(m * m + 2)
        t_new[:m * m].reshape(m, m)[np.arange(q), np.arange(q)] = theta[:q]
        T.copy_(torch.from_numpy(t_new))
        begin = q
    vecs = basis_rotate(V, S[:, :kk], mm, ws=token)
    return Eigenpairs(1.0 - theta[:kk], vecs, resid, u, comp, ncomp, cycle, matvecs, done and kk == k)


def meta_positions(ncomp: int, dim: int, centroids=None):
    """umap-learn's component_layout: where each of `ncomp` > 1 connected components goes, float64 [ncomp, dim] (numpy).
    Up to 2 dim components sit on the axes: the rows of vstack([B, -B])[:ncomp], B = hstack([eye(ceil(ncomp / 2)), zeros]).
    More than that: the eigenvectors 1 .. dim of the dense normalised Laplacian of exp(-d^2) (no self-loops), d the
    Euclidean distances of the components' centroids (float64 [ncomp, features]), divided by their maximum; each vector's
    sign is fixed so that its entry of largest magnitude is positive."""
    if ncomp <= 2 * dim:
        half = -(-ncomp // 2)
        base = np.hstack([np.eye(half), np.zeros((half, dim - half))])
        return np.vstack([base, -base])[:ncomp]
    c = np.asarray(centroids, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != ncomp:
        raise ValueError(f"centroids [{ncomp}, features] expected")
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    off = ~np.eye(ncomp, dtype=bool)
    # scipy's normalised Laplacian (which umap-learn reaches through sklearn) ignores self-loops, and a / sqrt(w_i w_j) does
    # not change when every affinity is scaled: exp(-(d^2 - min d^2)) is the same matrix without the underflow of far centroids
    aff = np.where(off, np.exp(-(d2 - d2[off].min())), 0.0)
    w = aff.sum(axis=1)
    alone = w == 0
    dinv = 1.0 / np.sqrt(np.where(alone, 1.0, w))
    lap = np.diag(1.0 - alone) - dinv[:, None] * aff * dinv[None, :]
    vecs = np.linalg.eigh(0.5 * (lap + lap.T))[1][:, 1:dim + 1]
    vecs = vecs * np.sign(vecs[np.abs(vecs).argmax(axis=0), np.arange(dim)])
    return vecs / vecs.max()


def component_ranges(meta):
    """data_range float64 [ncomp]: half the smallest positive distance from a component's meta position to another's
    (1 when every meta position coincides with it)."""
    meta = np.asarray(meta, dtype=np.float64)
    d = np.sqrt(((meta[:, None, :] - meta[None, :, :]) ** 2).sum(axis=2))
    return np.array([row[row > 0].min() / 2.0 if (row > 0).any() else 1.0 for row in d])


def component_is_small(size: int, dim: int) -> bool:
    """Whether a component is placed at random around its meta position and not by its own eigenvectors."""
    return size < 2 * dim or size <= dim + 1


def component_plan(x, labels, ncomp: int, dim: int):
    """(meta positions [ncomp, dim], data_range [ncomp]) of a disconnected graph's components; x [n, d] on the device
    gives the centroids when there are more than 2 dim components."""
    import torch

    centroids = None
    if ncomp > 2 * dim:
        lab = torch.from_numpy(labels).to(x.device)
        centroids = np.stack([x[lab == c].double().mean(dim=0).cpu().numpy() for c in range(ncomp)])
    meta = meta_positions(ncomp, dim, centroids)
    return meta, component_ranges(meta)


def _entry_rows(graph: CSR):
    """The row of every stored entry, int64 [nnz] on the graph's device."""
    import torch

    n = graph.indptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=graph.data.device), (graph.indptr[1:] - graph.indptr[:-1]).long())


def _select_entries(graph: CSR, head, keep) -> CSR:
    """The graph with only the stored entries that `keep` (bool [nnz]) marks; `head`: `_entry_rows(graph)`."""
    import torch

    if bool(keep.all()):
        return graph
    n = graph.indptr.numel() - 1
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=graph.data.device)
    indptr[1:] = torch.cumsum(torch.bincount(head[keep], minlength=n), 0)
    return CSR(indptr.to(torch.int32), graph.indices[keep].contiguous(), graph.data[keep].contiguous())


def _without_zeros(graph: CSR) -> CSR:
    """The graph without its explicit zeros: the entries a label intersection leaves are no edges (`graph_components`
    does not follow them either), so the two ends of every entry that stays share a component."""
    return _select_entries(graph, _entry_rows(graph), graph.data != 0)


def _component_subgraph(graph: CSR, comp, head, c: int):
    """(rows int64 ascending, the CSR of component c in its own numbering), by torch indexing on the device.  comp: the
    labels of `graph_components`; head: `_entry_rows(graph)`.  An entry is kept when both its ends are in the component
    and it is no explicit zero, and the row pointers are counted from the kept entries."""
    import torch

    n = graph.indptr.numel() - 1
    rows = torch.nonzero(comp == c).squeeze(1)
    renumber = torch.full((n,), -1, dtype=torch.int64, device=comp.device)
    renumber[rows] = torch.arange(rows.numel(), device=comp.device)
    cols = graph.indices.long()
    keep = (comp[head] == c) & (comp[cols] == c) & (graph.data != 0)
    indptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=comp.device)
    indptr[1:] = torch.cumsum(torch.bincount(head[keep], minlength=n)[rows], 0)
    return rows, CSR(indptr.to(torch.int32), renumber[cols[keep]].to(torch.int32).contiguous(), graph.data[keep].contiguous())


def spectral_layout(x, graph: CSR, dim: int, random_state: int = 0, tol: float = 1e-4):
    """umap-learn's spectral_layout with multi_component_layout, float64 [n, dim] on the device, or None when a solve did
    not converge.  One component: the eigenvectors 1 .. dim of the normalised Laplacian (`laplacian_eigenpairs`).  More:
    every component gets a meta position and a data_range (`component_plan`); a small one (`component_is_small`) is
    drawn uniformly within its data_range around its meta position from default_rng(random_state), in component order; any
    other gets its own eigenvectors 1 .. dim from its sub-graph, scaled to data_range / max|.| and moved to its meta
    position.  Components are numbered by their smallest row."""
    import torch

    n = _check_graph(graph)
    dim = int(dim)
    graph = _without_zeros(graph)  # (a label-intersected graph: its explicit zeros are no edges)
    ncomp, labels = graph_components(graph)
    if ncomp == 1:
        if n <= dim + 1:
            return None
        res = laplacian_eigenpairs(graph, dim, tol)
        return res.eigenvectors if res.converged else None
    dev = graph.data.device
    meta, ranges = component_plan(x, labels, ncomp, dim)
    rng = np.random.default_rng(random_state)
    comp = torch.from_numpy(labels).to(dev)
    head = _entry_rows(graph)
    out = torch.empty((n, dim), dtype=torch.float64, device=dev)
    sizes = np.bincount(labels, minlength=ncomp)
    for c in range(ncomp):
        centre = torch.from_numpy(meta[c]).to(dev)
        if component_is_small(int(sizes[c]), dim):
            out[comp == c] = torch.from_numpy(rng.uniform(-ranges[c], ranges[c], (int(sizes[c]), dim))).to(dev) + centre
            continue
        rows, sub = _component_subgraph(graph, comp, head, c)
        res = laplacian_eigenpairs(sub, dim, tol)
        if not res.converged:
            return None
        vecs = res.eigenvectors
        out[rows] = vecs * (float(ranges[c]) / float(vecs.abs().max())) + centre
    return out


def _sign_flip(vecs):
    """sklearn's _deterministic_vector_sign_flip on columns: the entry of largest magnitude of every column is positive."""
    import torch

    top = vecs.abs().argmax(dim=0)
    sign = torch.sign(vecs[top, torch.arange(vecs.shape[1], device=vecs.device)])
    return vecs * torch.where(sign == 0, torch.ones_like(sign), sign)


def connectivity_graph(x, n_neighbors: int, metric: str = "euclidean") -> CSR:
    """sklearn's kneighbors_graph(include_self=True) symmetrised, 0.5 (A + A^T), as CSR on the device: entries 1.0 where
    both rows list each other (the diagonal among them) and 0.5 where one does."""
    import torch

    _, idx = knn_graph(x, n_neighbors, metric)
    n, k = idx.shape
    dev = idx.device
    key = torch.unique(torch.arange(n, device=dev, dtype=torch.int64).unsqueeze(1) * n + idx.long())
    both = torch.unique(torch.cat([key, (key % n) * n + key // n]))

    def has(want):
        at = torch.searchsorted(key, want).clamp_(max=key.numel() - 1)
        return (key[at] == want).float()

    data = 0.5 * (has(both) + has((both % n) * n + both // n))
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(both // n, minlength=n), 0)
    return CSR(indptr.to(torch.int32), (both % n).to(torch.int32).contiguous(), data.contiguous())


def affinity_graph(x, n_neighbors: int, metric: str, affinity: str) -> CSR:
    """The affinity matrix of the spectral estimators: "fuzzy" (`fuzzy_simplicial_set`) or "connectivity"
    (`connectivity_graph`)."""
    if affinity not in ("fuzzy", "connectivity"):
        raise ValueError(f"affinity must be 'fuzzy' or 'connectivity' ({affinity!r} given)")
    x = _prep(x)
    k = int(n_neighbors)
    if not 1 <= k <= min(x.shape[0], MAX_NEIGHBORS):
        raise ValueError(f"n_neighbors ({k}) must be in [1, min(n_samples, {MAX_NEIGHBORS})]")
    return fuzzy_simplicial_set(x, k, metric) if affinity == "fuzzy" else connectivity_graph(x, k, metric)


def _without_diagonal(graph: CSR) -> CSR:
    """The graph without its diagonal entries (scipy's normalised Laplacian, which sklearn uses, ignores self-loops)."""
    head = _entry_rows(graph)
    return _select_entries(graph, head, head != graph.indices.long())


def spectral_embedding(graph: CSR, n_components: int, tol: float = 1e-6, drop_first: bool = True):
    """sklearn.manifold.spectral_embedding (norm_laplacian=True) of an affinity CSR: (embedding float64 [n, n_components]
    on the device, eigenvalues numpy, n_connected_components, converged).  Self-loops are dropped first, as scipy's
    normalised Laplacian does.  The columns are the trivial vectors (one per component, ordered by its smallest row) and
    then the nontrivial ones ascending, the first column dropped with `drop_first`; every eigenvector is divided by
    sqrt(deg) (sklearn's recovery) and its sign fixed by `_sign_flip`."""
    import torch

    n = _check_graph(graph)
    want = int(n_components) + (1 if drop_first else 0)
    if not 1 <= int(n_components) or want > n:
        raise ValueError(f"n_components ({n_components}) must be at least 1 and leave room in {n} rows")
    graph = _without_diagonal(graph)
    ncomp, labels = graph_components(graph)
    deg, _ = laplacian_degree(graph)
    if want <= ncomp:  # the closed-form vectors fill every column: nothing to iterate, nothing that could fail to converge
        deg_h = deg.cpu().numpy()
        if not (deg_h > 0).all():
            raise ValueError("every row of the graph needs a positive degree")
        u = torch.from_numpy(trivial_vectors(deg_h, labels, ncomp)).to(deg.device)
        full, vals, converged = _trivial_matrix(u, torch.from_numpy(labels).to(deg.device), ncomp)[:, :want], np.zeros(want), True
    else:
        res = laplacian_eigenpairs(graph, want - ncomp, tol)
        full = torch.cat([res.trivial_matrix(), res.eigenvectors], dim=1)
        vals, converged = np.concatenate([np.zeros(ncomp), res.eigenvalues]), bool(res.converged)
    full = _sign_flip(full / torch.sqrt(deg).unsqueeze(1))
    first = 1 if drop_first else 0
    return full[:, first:].contiguous(), vals[first:], ncomp, converged


class SpectralEmbedding:
    """sklearn.manifold.SpectralEmbedding on device tensors, with the exact kNN graph: `fit(x)` / `fit_transform(x)` give
    `embedding_` float32 [n, n_components] on the device and set `eigenvalues_` (numpy, of the kept columns),
    `n_connected_components_`, `converged_` and `affinity_matrix_` (CSR).  affinity: "fuzzy" (UMAP's fuzzy simplicial
    set) or "connectivity" (sklearn's nearest_neighbors affinity, self included)."""

    def __init__(self, n_components: int = 2, n_neighbors: int = 15, metric: str = "euclidean", affinity: str = "fuzzy",
                 tol: float = 1e-6):
        metric_code(metric)
        if affinity not in ("fuzzy", "connectivity"):
            raise ValueError(f"affinity must be 'fuzzy' or 'connectivity' ({affinity!r} given)")
        if int(n_components) < 1 or not 1 <= int(n_neighbors) <= MAX_NEIGHBORS or not tol >= 0:
            raise ValueError(f"n_components >= 1, n_neighbors in [1, {MAX_NEIGHBORS}] and tol >= 0 required")
        self.n_components, self.n_neighbors, self.metric = int(n_components), int(n_neighbors), metric
        self.affinity, self.tol = affinity, float(tol)
        self.embedding_ = self.eigenvalues_ = self.n_connected_components_ = self.converged_ = self.affinity_matrix_ = None

    def fit(self, x, y=None) -> "SpectralEmbedding":
        graph = affinity_graph(x, min(self.n_neighbors, x.shape[0]), self.metric, self.affinity)
        emb, self.eigenvalues_, self.n_connected_components_, self.converged_ = spectral_embedding(graph, self.n_components,
                                                                                                  self.tol)
        self.affinity_matrix_ = graph
        self.embedding_ = emb.float().contiguous()
        return self

    def fit_transform(self, x, y=None):
        return self.fit(x).embedding_


# ------------------------------------------------------------------------------------------------ estimator

_INITS = ("spectral", "spectral_device", "pca", "random")


class UMAP:
    """umap.UMAP on device tensors: `.fit(x)` / `.fit_transform(x)` give float32 [n, n_components] on the device and
    set `embedding_`, `graph_` (CSR), `a_`, `b_`.  `n_epochs=None` means 500 for at most 10 000 rows and 200 above.
    `init`: "spectral" (falls back to "pca" with a warning when the graph is disconnected or eigsh does not
    converge), "spectral_device" (`spectral_layout`: the same start from the device eigensolver, every connected
    component of a disconnected graph laid out on its own; falls back to "pca" with a warning only when the solver does
    not converge), "pca", "random" or an [n, n_components] array."""

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
        if isinstance(init, str) and init not in _INITS:
            raise ValueError("init must be 'spectral', 'spectral_device', 'pca', 'random' or an array")
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
            elif init == "spectral_device":
                y = spectral_layout(x, graph, dim, self.random_state)
                if y is None:
                    warnings.warn("UMAP: the device eigensolver of init='spectral_device' did not converge; falling back to "
                                  "init='pca'")
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
