"""Local, density-based outlier scores of dumped features: sklearn.neighbors.LocalOutlierFactor (Breunig et al. 2000)
over the exact kNN lists, for the fitted rows and, with `novelty=True`, for new rows against them; and the in-degree of
the kNN graph (the ODIN score) with its skewness, the hubness of the embedding.

"Which wafers look like nothing we have seen" without a clustering behind it: GLOSH (`cluster.HDBSCAN.outlier_scores_`)
is relative to one condensed tree and its min_cluster_size, `mixture.GaussianMixture.score_samples` assumes elliptical
clusters; LOF compares the density around a row with the density around its neighbours and needs the lists alone.

Steps, all on the device:
  1. the lists: manifold.knn_graph at max(k) + 1 with the row itself removed by index (manifold.neighbor_lists' rule,
     the distances kept), or manifold.knn_query of new rows against the fitted rows (nothing removed).  Rows are ordered
     by (distance, index), so the first k columns are the k-neighbourhood: one graph serves a LIST of neighbour counts;
  2. the local reachability density (csrc/lof.hip: wm_lof_lrd), with kdist_k(j) = dist_fit[j][k - 1]:
         lrd_k(i) = 1 / (mean_{t < k} max(dist(i, j_t), kdist_k(j_t)) + 1e-10)
     (the 1e-10 is sklearn's: a row with more than k exact duplicates has lrd = 1e10 and LOF = 1);
  3. the factor (wm_lof_factor):  LOF_k(i) = (mean_{t < k} lrd_k(j_t)) / lrd_k(i);
  4. the in-degree (wm_lof_indegree):  N_k(j) = #{ i : j among the first k columns of row i }.
Every group of a list shares the loads of the lists; a k gives the same bits alone as inside any list, and two calls give
the same bits (a fixed tree per sum, no float atomics).  Breunig et al. recommend the maximum of LOF over a range of k.

Conventions as in semi_supervised.py: device tensors in, the functional layer returns device tensors, estimator
attributes are host numpy arrays, host-only logic is plain functions that need no GPU; a CPU tensor or a missing library
raises, there is no fallback.  `ref_lrd`, `ref_lof` and `ref_in_degree` restate the kernels in numpy float64 over the same
(dist, idx) arrays: the CPU tests check them against sklearn, the GPU tests check the kernels against them.
"""
from __future__ import annotations

import warnings
from typing import NamedTuple, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr
from .cluster import metric_code
from .density import KernelDensity  # noqa: F401  (sklearn's class lives in neighbors: neighbors.KernelDensity is density's)
from .manifold import _token_ws, knn_graph, knn_query

MAX_K = 63  # columns of a list: one wave64 lane each, the last lane idle (csrc/lof.hip)
MAX_GROUPS = 64  # WM_LOF_MAX_GROUPS: neighbour counts per launch; a longer list goes in chunks
MAX_ROWS = 1 << 24
LRD_EPS = 1e-10  # sklearn's


# ------------------------------------------------------------------------------------------------ host logic (no GPU)


def check_ks(n_neighbors, limit: int = MAX_K) -> Tuple[np.ndarray, bool]:
    """(ks int32 [R], whether a single number was given).  Every k lies in [1, limit]."""
    single = np.ndim(n_neighbors) == 0
    k = np.atleast_1d(np.asarray(n_neighbors))
    if k.ndim != 1 or k.size == 0 or not np.issubdtype(k.dtype, np.integer) or not np.all((k >= 1) & (k <= limit)):
        raise ValueError(f"n_neighbors must be an integer or a sequence of integers in [1, {limit}] ({n_neighbors!r} given)")
    return k.astype(np.int32), single


def _lists(name: str, dist, idx):
    """Shapes of a pair of host lists (dist may be None)."""
    idx = np.asarray(idx)
    if idx.ndim != 2 or not np.issubdtype(idx.dtype, np.integer) or (dist is not None and np.shape(dist) != idx.shape):
        raise ValueError(f"{name}: dist [rows, ld] and integer idx [rows, ld] of one shape expected")
    return (None if dist is None else np.asarray(dist, dtype=np.float64)), idx.astype(np.int64)


def ref_lrd(dist_q, idx_q, dist_fit, ks) -> np.ndarray:
    """float64 [R, rows]: wm_lof_lrd in numpy.  dist_q, idx_q [rows, ld] the query lists, dist_fit [n_fit, ld_fit] the
    fitted lists' distances (any float dtype: widened first), ks the neighbour counts."""
    dist_q, idx_q = _lists("ref_lrd", dist_q, idx_q)
    dist_fit = np.asarray(dist_fit, dtype=np.float64)
    ks, _ = check_ks(ks, min(idx_q.shape[1], dist_fit.shape[1]))
    out = np.empty((len(ks), idx_q.shape[0]))
    for r, k in enumerate(ks):
        reach = np.maximum(dist_q[:, :k], dist_fit[idx_q[:, :k], k - 1])
        out[r] = 1.0 / (reach.sum(axis=1) / float(k) + LRD_EPS)
    return out


def ref_lof(idx_q, lrd_q, lrd_fit, ks) -> np.ndarray:
    """float64 [R, rows]: wm_lof_factor in numpy.  lrd_q [R, rows], lrd_fit [R, n_fit]."""
    _, idx_q = _lists("ref_lof", None, idx_q)
    ks, _ = check_ks(ks, idx_q.shape[1])
    lrd_q, lrd_fit = np.asarray(lrd_q, dtype=np.float64), np.asarray(lrd_fit, dtype=np.float64)
    if lrd_q.shape != (len(ks), idx_q.shape[0]) or lrd_fit.ndim != 2 or lrd_fit.shape[0] != len(ks):
        raise ValueError("lrd_q [R, rows] and lrd_fit [R, n_fit] expected")
    out = np.empty_like(lrd_q)
    for r, k in enumerate(ks):
        out[r] = (lrd_fit[r][idx_q[:, :k]].sum(axis=1) / float(k)) / lrd_q[r]
    return out


def ref_in_degree(idx, ks, n: int = None) -> np.ndarray:
    """int32 [R, n]: wm_lof_indegree in numpy (n defaults to the number of rows)."""
    _, idx = _lists("ref_in_degree", None, idx)
    ks, _ = check_ks(ks, idx.shape[1])
    n = idx.shape[0] if n is None else int(n)
    out = np.zeros((len(ks), n), dtype=np.int32)
    for r, k in enumerate(ks):
        np.add.at(out[r], idx[:, :k].ravel(), 1)
    return out


def skewness(counts) -> float:
    """The (biased, Fisher-Pearson) skewness m3 / m2^1.5 of integer counts in float64; 0 when they are all equal."""
    c = np.asarray(counts, dtype=np.float64).ravel()
    if c.size == 0:
        raise ValueError("at least one count expected")
    dev = c - c.mean()
    m2, m3 = float((dev * dev).mean()), float((dev * dev * dev).mean())
    return 0.0 if m2 == 0.0 else m3 / m2 ** 1.5


def clipped_neighbors(n_neighbors: int, n: int) -> int:
    """sklearn's n_neighbors_ = max(1, min(n_neighbors, n - 1)), with its warning when the request is clipped, and the
    kernels' limit on the result."""
    n_neighbors, n = int(n_neighbors), int(n)
    if n < 2:
        raise ValueError(f"at least 2 rows expected ({n} given)")
    if n_neighbors < 1:
        raise ValueError(f"n_neighbors >= 1 required ({n_neighbors} given)")
    k = max(1, min(n_neighbors, n - 1))
    if k < n_neighbors:
        warnings.warn(f"n_neighbors ({n_neighbors}) is greater than the total number of samples ({n}) minus one. n_neighbors will be "
                      f"set to (n_samples - 1) for estimation.", UserWarning, stacklevel=3)
    if k > MAX_K:
        raise ValueError(f"n_neighbors_ = {k}: the neighbour lists of the kernels hold at most {MAX_K} columns")
    return k


def check_contamination(contamination):
    """'auto' or a number in (0, 0.5]."""
    if isinstance(contamination, str):
        if contamination != "auto":
            raise ValueError(f"contamination must be 'auto' or a number in (0, 0.5] ({contamination!r} given)")
        return contamination
    c = float(contamination)
    if not 0.0 < c <= 0.5:
        raise ValueError(f"contamination must be 'auto' or a number in (0, 0.5] ({contamination!r} given)")
    return c


def offset_for(negative_outlier_factor: np.ndarray, contamination) -> float:
    """sklearn's offset_: -1.5 for 'auto', else the 100 * contamination percentile of the fitted scores."""
    if contamination == "auto":
        return -1.5
    return float(np.percentile(negative_outlier_factor, 100.0 * float(contamination)))


def labels_from(scores: np.ndarray, offset: float) -> np.ndarray:
    """+1, and -1 where a score lies below the offset (int64, as sklearn's)."""
    out = np.ones(np.shape(scores), dtype=np.int64)
    out[np.asarray(scores) < offset] = -1
    return out


# ------------------------------------------------------------------------------------------------ the three entry points


def _device_lists(name: str, dist, idx):
    import torch

    require_gpu(dist, idx)
    if idx.dim() != 2 or idx.dtype != torch.int32 or (dist is not None and (dist.dtype != torch.float32 or dist.shape != idx.shape)):
        raise ValueError(f"{name}: dist float32 [rows, ld] and idx int32 [rows, ld] expected")
    rows, ld = idx.shape
    if not (1 <= rows <= MAX_ROWS and 1 <= ld <= MAX_K):
        raise ValueError(f"{name}: 1 .. {MAX_ROWS} rows of 1 .. {MAX_K} columns expected ({rows} x {ld} given)")
    return rows, ld


def _check_range(name: str, idx, n: int) -> None:
    """(one reduction pair read by the host; the kernels themselves skip an index outside [0, n))"""
    if int(idx.min()) < 0 or int(idx.max()) >= n:
        raise ValueError(f"{name}: idx must lie in [0, {n})")


def _out(name: str, out, shape, dtype, device):
    import torch

    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    require_gpu(out)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name}: out {dtype} {list(shape)} expected")
    return out


def _chunks(ks: np.ndarray):
    """(first group, the host array of its neighbour counts) per launch."""
    for g in range(0, len(ks), MAX_GROUPS):
        yield g, np.ascontiguousarray(ks[g:g + MAX_GROUPS])


def local_reachability_density(dist_q, idx_q, dist_fit, ks, out=None, checked: bool = False, ws=None):
    """lrd float64 [R, rows] on the device (wm_lof_lrd) of the query lists (dist_q float32, idx_q int32, [rows, ld]) against
    the fitted lists' distances dist_fit float32 [n_fit, ld_fit]; ks: a number or a sequence, every k <= min(ld, ld_fit).
    For the fitted rows themselves pass their own lists as both.  Columns behind max(ks) are never read into a sum.
    `checked`: the caller vouches for idx in [0, n_fit) and the call reads nothing back."""
    import torch

    rows, ld = _device_lists("local_reachability_density", dist_q, idx_q)
    require_gpu(dist_fit)
    if dist_fit.dim() != 2 or dist_fit.dtype != torch.float32 or not 1 <= dist_fit.shape[1] <= MAX_K or not 1 <= dist_fit.shape[0] <= MAX_ROWS:
        raise ValueError(f"dist_fit float32 [n_fit <= {MAX_ROWS}, ld_fit <= {MAX_K}] expected")
    n_fit, ld_fit = dist_fit.shape
    ks, _ = check_ks(ks, min(ld, ld_fit))
    if not checked:
        _check_range("local_reachability_density", idx_q, n_fit)
    out = _out("local_reachability_density", out, (len(ks), rows), torch.float64, idx_q.device)
    lib = _lib.load()
    for g, part in _chunks(ks):
        ws, need = _token_ws(lib.wm_lof_lrd_workspace_bytes(rows, ld, len(part)),
                             f"local_reachability_density: unsupported sizes rows={rows} ld={ld}", idx_q.device, ws)
        check(lib.wm_lof_lrd(ptr(dist_q), ptr(idx_q), rows, ld, ptr(dist_fit), n_fit, ld_fit, part.ctypes.data, len(part),
                             ptr(out) + 8 * g * rows, ptr(ws), need, stream_ptr()), "wm_lof_lrd")
    return out


def local_outlier_factor(idx_q, lrd_q, lrd_fit, ks, out=None, checked: bool = False, ws=None):
    """lof float64 [R, rows] on the device (wm_lof_factor): the mean lrd of each query row's first k neighbours over the
    row's own.  idx_q int32 [rows, ld]; lrd_q [R, rows] and lrd_fit [R, n_fit] as `local_reachability_density` returns them
    for the same ks (the same tensor for the fitted rows themselves)."""
    import torch

    rows, ld = _device_lists("local_outlier_factor", None, idx_q)
    ks, _ = check_ks(ks, ld)
    require_gpu(lrd_q, lrd_fit)
    if lrd_q.dtype != torch.float64 or tuple(lrd_q.shape) != (len(ks), rows) or lrd_fit.dtype != torch.float64 or lrd_fit.dim() != 2 \
            or lrd_fit.shape[0] != len(ks) or not 1 <= lrd_fit.shape[1] <= MAX_ROWS:
        raise ValueError(f"lrd_q float64 [{len(ks)}, {rows}] and lrd_fit float64 [{len(ks)}, n_fit] expected")
    n_fit = lrd_fit.shape[1]
    if not checked:
        _check_range("local_outlier_factor", idx_q, n_fit)
    out = _out("local_outlier_factor", out, (len(ks), rows), torch.float64, idx_q.device)
    if out.data_ptr() in (lrd_q.data_ptr(), lrd_fit.data_ptr()):
        raise ValueError("out must be a buffer of its own")
    lib = _lib.load()
    for g, part in _chunks(ks):
        ws, need = _token_ws(lib.wm_lof_factor_workspace_bytes(rows, ld, len(part)),
                             f"local_outlier_factor: unsupported sizes rows={rows} ld={ld}", idx_q.device, ws)
        check(lib.wm_lof_factor(ptr(idx_q), rows, ld, ptr(lrd_q) + 8 * g * rows, ptr(lrd_fit) + 8 * g * n_fit, n_fit, part.ctypes.data,
                                len(part), ptr(out) + 8 * g * rows, ptr(ws), need, stream_ptr()), "wm_lof_factor")
    return out


def in_degree(idx, ks, n: int = None, out=None, checked: bool = False, ws=None):
    """int32 [R, n] on the device (wm_lof_indegree): how many rows list j among their first k columns.  idx int32
    [rows, ld] in [0, n); n defaults to rows (the lists of a set against itself)."""
    import torch

    rows, ld = _device_lists("in_degree", None, idx)
    ks, _ = check_ks(ks, ld)
    n = rows if n is None else int(n)
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(f"n in [1, {MAX_ROWS}] expected ({n} given)")
    if not checked:
        _check_range("in_degree", idx, n)
    out = _out("in_degree", out, (len(ks), n), torch.int32, idx.device)
    lib = _lib.load()
    for g, part in _chunks(ks):
        ws, need = _token_ws(lib.wm_lof_indegree_workspace_bytes(rows, ld, len(part)), f"in_degree: unsupported sizes rows={rows} ld={ld}",
                             idx.device, ws)
        check(lib.wm_lof_indegree(ptr(idx), rows, ld, n, part.ctypes.data, len(part), ptr(out) + 4 * g * n, ptr(ws), need, stream_ptr()),
              "wm_lof_indegree")
    return out


# ------------------------------------------------------------------------------------------------ scores of a matrix


class OutlierScores(NamedTuple):
    """Device tensors [R, n], one row per neighbour count.  lof, lrd float64; kdist float32 (the distance to the k-th
    neighbour, the row itself not counted: a column of the graph, copied); indegree int32."""
    lof: object
    lrd: object
    kdist: object
    indegree: object


def fitted_lists(x, k: int, metric: str = "euclidean"):
    """(dist float32 [n, k], idx int32 [n, k]) on the device: `knn_graph` at k + 1 with the row itself removed by index,
    exactly as manifold.neighbor_lists removes it (exact duplicates stay; a row that more than k duplicates with lower
    indices pushed out of its own list loses its last entry instead), the distances kept beside the indices."""
    import torch

    dist, idx = knn_graph(x, int(k) + 1, metric)
    own = idx == torch.arange(idx.shape[0], dtype=torch.int32, device=idx.device).unsqueeze(1)
    keep = torch.sort(own.to(torch.int8), dim=1, stable=True).indices[:, :int(k)]  # (the row itself moves to the end)
    return dist.gather(1, keep).contiguous(), idx.gather(1, keep).contiguous()


def _scores_of_lists(dist, idx, ks: np.ndarray) -> OutlierScores:
    import torch

    lrd = local_reachability_density(dist, idx, dist, ks, checked=True)
    lof = local_outlier_factor(idx, lrd, lrd, ks, checked=True)
    indeg = in_degree(idx, ks, checked=True)
    cols = torch.from_numpy(ks.astype(np.int64) - 1).to(dist.device)
    return OutlierScores(lof, lrd, dist.index_select(1, cols).t().contiguous(), indeg)


def outlier_scores(x, n_neighbors: Union[int, Sequence[int]], metric: str = "euclidean") -> OutlierScores:
    """LOF, lrd, k-distance and in-degree of every row of x [n, d] (device tensor) for each neighbour count of
    `n_neighbors` (an int or a sequence, 1 .. min(n - 1, 63)): one kNN graph at max + 1, the row removed by index, then the
    three passes, each one launch for all counts.  An OutlierScores of [R, n] device tensors (R = 1 for an int)."""
    metric_code(metric)
    require_gpu(x)
    if x.dim() != 2 or x.shape[0] < 2:
        raise ValueError("x [n >= 2, d] expected")
    ks, _ = check_ks(n_neighbors, min(x.shape[0] - 1, MAX_K))
    dist, idx = fitted_lists(x, int(ks.max()), metric)
    return _scores_of_lists(dist, idx, ks)


def hubness(x, k: int, metric: str = "euclidean") -> float:
    """The skewness of the k-occurrence counts N_k (the in-degrees of the kNN graph of x without self-loops): near 0 for
    an embedding whose rows are listed about equally often, large and positive when a few hubs appear in very many lists
    (Radovanovic et al. 2010).  The counts are integers from the device; the moments are float64 on the host."""
    scores = outlier_scores(x, int(k), metric)
    return skewness(scores.indegree[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------ estimator


class LocalOutlierFactor:
    """sklearn.neighbors.LocalOutlierFactor over the exact kNN lists of device rows.

    `fit(x)`: x a device tensor [n, d].  Sets `n_neighbors_` (= min(n_neighbors, n - 1), with sklearn's warning when that
    clips; above 63 is a ValueError), `n_samples_fit_`, `negative_outlier_factor_` (float64 [n], -LOF; near -1 for
    inliers), `local_reachability_density_`, `kdist_` (float32) and `offset_` (-1.5 for contamination="auto", else the
    100 * contamination percentile of the fitted scores; contamination in (0, 0.5]).
    novelty=False: `fit_predict(x)` returns +1 / -1 for the fitted rows; `score_samples`, `decision_function` and `predict`
    raise AttributeError, as sklearn's are not available.  novelty=True: those three take NEW rows (their kNN among the
    fitted rows, nothing removed, then the two passes against the fitted lists), and `fit_predict` raises.  A fitted row
    given back as a new row finds itself at distance 0 and so does not get its fitted score, as in sklearn."""

    def __init__(self, n_neighbors: int = 20, metric: str = "euclidean", contamination="auto", novelty: bool = False):
        metric_code(metric)
        if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)) or n_neighbors < 1:
            raise ValueError(f"n_neighbors must be an integer >= 1 ({n_neighbors!r} given)")
        self.n_neighbors, self.metric, self.novelty = int(n_neighbors), metric, bool(novelty)
        self.contamination = check_contamination(contamination)
        self.negative_outlier_factor_ = self.local_reachability_density_ = self.kdist_ = None
        self.n_neighbors_ = self.n_samples_fit_ = self.offset_ = None
        self._x = self._dist = self._lrd = None

    def fit(self, x, y=None):
        require_gpu(x)
        if x.dim() != 2:
            raise ValueError("x [n, d] expected")
        n = int(x.shape[0])
        k = clipped_neighbors(self.n_neighbors, n)
        ks = np.array([k], dtype=np.int32)
        dist, idx = fitted_lists(x, k, self.metric)
        scores = _scores_of_lists(dist, idx, ks)
        self._x, self._dist, self._lrd = x, dist, scores.lrd
        self.n_neighbors_, self.n_samples_fit_ = k, n
        self.negative_outlier_factor_ = -scores.lof[0].cpu().numpy()
        self.local_reachability_density_ = scores.lrd[0].cpu().numpy()
        self.kdist_ = scores.kdist[0].cpu().numpy()
        self.offset_ = offset_for(self.negative_outlier_factor_, self.contamination)
        return self

    def fit_predict(self, x, y=None):
        if self.novelty:
            raise AttributeError("fit_predict is not available when novelty=True. Use novelty=False if you want to predict on the "
                                 "training set.")
        return labels_from(self.fit(x).negative_outlier_factor_, self.offset_)

    def _for_new_rows(self, name: str) -> None:
        if not self.novelty:
            raise AttributeError(f"{name} is not available when novelty=False. Use novelty=True if you want to use LOF for novelty "
                                 f"detection and compute {name} for new unseen data. Note that the opposite LOF of the training "
                                 f"samples is always available by considering the negative_outlier_factor_ attribute.")
        if self._lrd is None:
            raise RuntimeError("fit first")

    def score_samples(self, x):
        """-LOF of new rows x [m, d] (device tensor) against the fitted rows: float64 [m] (numpy)."""
        self._for_new_rows("score_samples")
        ks = np.array([self.n_neighbors_], dtype=np.int32)
        dist_q, idx_q = knn_query(x, self._x, self.n_neighbors_, self.metric)
        lrd_q = local_reachability_density(dist_q, idx_q, self._dist, ks, checked=True)
        return -local_outlier_factor(idx_q, lrd_q, self._lrd, ks, checked=True)[0].cpu().numpy()

    def decision_function(self, x):
        """score_samples(x) - offset_: negative for an outlier."""
        self._for_new_rows("decision_function")
        return self.score_samples(x) - self.offset_

    def predict(self, x):
        """+1 / -1 (int64 numpy) of new rows: -1 where decision_function < 0."""
        self._for_new_rows("predict")
        return labels_from(self.decision_function(x), 0.0)
