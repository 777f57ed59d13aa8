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

Not built (NotImplementedError naming the feature): densmap=True, y= (semi-supervised fits), transform of new rows.
Only local_connectivity = 1 and set_op_mix_ratio = 1 are supported.
"""
from __future__ import annotations

import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr
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
    if need == 0:
        raise ValueError(f"knn_graph: unsupported sizes n={n} d={d} k={k} (k <= {MAX_NEIGHBORS})")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
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


def fuzzy_union(idx, weights) -> CSR:
    """G = P + P^T - P o P^T of the directed membership matrix P[i, idx[i, j]] = weights[i, j] (zeros dropped), as CSR
    on the device.  The value of an entry is formed in double from the two float32 memberships and rounded once, by
    the same expression for (i, j) and (j, i): G is symmetric in bits and within 2^-24 relative of the exact union."""
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
    return CSR(indptr.to(torch.int32), (both % n).to(torch.int32).contiguous(), data.contiguous())


def fuzzy_simplicial_set(x, n_neighbors: int, metric: str = "euclidean") -> CSR:
    """umap-learn's fuzzy_simplicial_set (local_connectivity = 1, set_op_mix_ratio = 1) of the rows of x."""
    dist, idx = knn_graph(x, n_neighbors, metric)
    _, _, w = smooth_knn(dist, idx)
    return fuzzy_union(idx, w)


def sample_rates(data):
    """q_e = rint(65536 w_e / max w) of the graph's weights, in float64, as the int32 tensor the layout kernel reads
    (0 <= q_e <= 65536)."""
    import torch

    if data.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=data.device)
    w = data.double()
    return torch.round(65536.0 * w / w.max()).to(torch.int32).contiguous()


def optimize_layout(y, indptr, indices, q, a: float, b: float, n_epochs: int, epoch_begin: int = 0,
                    epoch_end: Optional[int] = None, gamma: float = 1.0, learning_rate: float = 1.0, seed: int = 0,
                    negative_sample_rate: int = 5):
    """Epochs [epoch_begin, epoch_end) of `n_epochs` of the layout optimisation (csrc/umap.hip) from the positions
    y float32 [n, dim] over the symmetric CSR graph (indptr, indices int32) with sampling rates q (`sample_rates`).
    Returns the new positions; y is left unchanged.  Splitting the epoch range over several calls changes no bit."""
    import torch

    require_gpu(y, indptr, indices, q)
    epoch_end = n_epochs if epoch_end is None else epoch_end
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("y float32 [n, dim] expected")
    n, dim = y.shape
    if not 1 <= dim <= MAX_COMPONENTS:
        raise ValueError(f"1 <= dim <= {MAX_COMPONENTS} expected ({dim} given)")
    if indptr.dtype != torch.int32 or indices.dtype != torch.int32 or q.dtype != torch.int32:
        raise ValueError("indptr, indices and q must be int32")
    if indptr.shape != (n + 1,) or q.shape != indices.shape or indices.dim() != 1:
        raise ValueError("indptr [n + 1], indices [nnz] and q [nnz] expected")
    # the kernel trusts the graph: check once here that no entry points outside y
    ip = indptr.long()
    if int(ip[0]) != 0 or int(ip[-1]) != indices.numel() or bool((ip[1:] < ip[:-1]).any()):
        raise ValueError("indptr must rise from 0 to nnz")
    if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= n or int(q.min()) < 0 or int(q.max()) > 65536):
        raise ValueError("indices must lie in [0, n) and q in [0, 65536]")
    if not 0 <= epoch_begin <= epoch_end <= n_epochs or n_epochs < 1:
        raise ValueError("0 <= epoch_begin <= epoch_end <= n_epochs expected")
    if not (a > 0 and b > 0 and gamma >= 0 and learning_rate >= 0 and 0 <= int(negative_sample_rate) <= 64):
        raise ValueError("a, b > 0, gamma, learning_rate >= 0 and 0 <= negative_sample_rate <= 64 expected")
    import ctypes

    bufs = (y.clone(), torch.empty_like(y))
    which = ctypes.c_int(0)
    check(_lib.load().wm_umap_layout(ptr(bufs[0]), ptr(bufs[1]), ptr(indptr), ptr(indices), ptr(q), n, dim, float(a), float(b),
                                     float(gamma), float(learning_rate), int(seed) & _MASK32, int(epoch_begin), int(epoch_end),
                                     int(n_epochs), int(negative_sample_rate), ctypes.addressof(which), stream_ptr()),
          "wm_umap_layout")
    return bufs[which.value]


# ------------------------------------------------------------------------------------------------ initialisation


def _spectral_init(graph: CSR, dim: int):
    """umap-learn's spectral_layout for a connected graph: the eigenvectors 1 .. dim of the normalised Laplacian
    (scipy eigsh on the host).  None when the graph is disconnected or eigsh does not converge."""
    import scipy.sparse
    import scipy.sparse.csgraph
    import scipy.sparse.linalg

    g = graph.to_scipy().astype(np.float64)
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
            raise NotImplementedError("densmap=True is not implemented (the density term of DensMAP has no kernel)")
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

    def fit(self, x, y=None) -> "UMAP":
        if y is not None:
            raise NotImplementedError("y= (semi-supervised UMAP) is not implemented")
        x = _prep(x)
        n = x.shape[0]
        if n < 2:
            raise ValueError("UMAP needs at least 2 rows")
        graph = fuzzy_simplicial_set(x, min(self.n_neighbors, n), self.metric)
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
        raise NotImplementedError("transform of new rows is not implemented (fit_transform embeds the fitted rows)")
