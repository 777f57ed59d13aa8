"""HDBSCAN clustering and cluster scores for dumped embeddings.

The reference's flow (notebooks/3.1-Embeddings-clustering.ipynb, 3.2-Embeddings-SSL-categories.ipynb): HDBSCAN on
the embedding matrix inside a hyper-parameter search over `min_cluster_size`, `min_samples`,
`cluster_selection_epsilon` and `metric`, every trial scored with homogeneity, silhouette, Calinski-Harabasz and
Davies-Bouldin.

Here the O(N^2 D) parts are HIP kernels (csrc/cluster.hip): the core distances, the Boruvka rounds of the
mutual-reachability spanning tree and the all-pairs pass of the silhouette.  The spanning tree depends on
`(metric, min_samples, alpha)` only, so `HDBSCAN.refit` / `labels_from_mst` serve every
`(min_cluster_size, cluster_selection_epsilon)` trial that shares them without touching the GPU again.

What runs on the host, in numpy float64, and why: the per-component minimum and the union-find between Boruvka rounds
(at most ceil(log2 n) rounds of O(n) work), and everything from the sorted tree edges to the labels (single-linkage
tree, condensed tree, stabilities, selection: O(n log n) pointer chasing with no arithmetic to speak of).

Semantics follow `sklearn.cluster.HDBSCAN`: `min_samples` counts the point itself (the core distance is the
`min_samples`-th smallest distance with the zero self-distance as the first), which is one neighbour fewer than the
generic path of the `hdbscan` package uses for the same number.  `alpha` divides the pairwise distance inside the
mutual reachability, max(core_i, core_j, dist_ij / alpha), with the core distances unscaled.

New rows (`HDBSCAN(prediction_data=True)`, `approximate_predict`, `approximate_predict_scores`): one more all-pairs
pass (wm_mreach_query) finds, for every new row, the fitted row nearest in mutual reachability; the walk from that
row through the condensed tree to a label, a membership strength and a GLOSH outlier score is host code
(`assign_from_tree`), as is `outlier_scores_` of the fitted rows (`glosh`).

Soft clustering (`exemplar_indices_`, `all_points_membership_vectors`, `membership_vector`): one rectangular pass
(wm_group_min_dist) gives every row its distance to the nearest exemplar of every cluster; the merge heights in the
condensed tree and the membership vectors themselves are host code (`exemplars_from_tree`, `membership_from_tree`).

Cluster validity without ground truth (`validity_index`, `relative_validity`, `HDBSCAN.relative_validity_`): DBCV of
Moulavi et al. 2014 under the names of the `hdbscan` package's validity module.  With the rows sorted by label its three
all-pairs parts are block-diagonal passes of the same kernels (wm_allpoints_core, wm_mreach_min_edge_grouped: one
Boruvka round of every cluster's own tree per launch, wm_group_min_mreach); which rows and edges of a cluster's tree are
internal and the score itself are host code (`validity_from_parts`).  `relative_validity` is the package's cheap
approximation from the fitted spanning tree and uses no GPU.  DESIGN.md states the definition and what differs from the
package.

KMeans (`KMeans`, `kmeans_step`, `kmeans_plusplus`; the reference's sklearn.cluster.KMeans(n_clusters=k) of notebook
1.0-Preprocess-WM811K): a partition of ALL rows into a chosen number of clusters, the baseline that silhouette,
Calinski-Harabasz and Davies-Bouldin were designed for.  The assignment is wm_group_min_dist again, with the centres of
R restarts laid out as R groups of k columns, so one pass over the rows assigns them for every restart; the update
(wm_kmeans_update: float64 sums in a fixed order, no atomics) and the k-means++ seeding (wm_kmeans_seed, driven by a
host-drawn table of uniforms) are csrc/kmeans.hip.  The stopping rule (`kmeans_stop`) and the empty-cluster rule
(`kmeans_relocation_plan`) are host functions on numpy values.  DESIGN.md states the definitions.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr, workspace

METRICS = {"euclidean": 0, "l2": 0, "manhattan": 1, "l1": 1, "cityblock": 1}
_LISTED_NOT_BUILT = ("canberra", "braycurtis")  # in the notebook's search space; no kernel here

CONDENSED_DTYPE = np.dtype([("parent", np.intp), ("child", np.intp), ("lambda_val", np.float64), ("child_size", np.intp)])


def metric_code(metric: str) -> int:
    """The kernels' code of a metric name (0 Euclidean, 1 Manhattan).  A metric the notebook lists but no kernel
    computes raises NotImplementedError naming it; any other unknown name raises ValueError."""
    if metric in _LISTED_NOT_BUILT:
        raise NotImplementedError(f"metric {metric!r} is not implemented (available: euclidean, manhattan)")
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r} (available: euclidean, manhattan)")
    return METRICS[metric]


def _prep(x):
    import torch

    require_gpu(x)
    if x.dim() != 2:
        raise ValueError("expected [n_samples, n_features]")
    x = x.float()
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))  # zero columns change no distance
    if x.shape[1] > 1024:
        raise ValueError(f"at most 1024 features ({x.shape[1]} given): reduce the matrix first")
    return x.contiguous()


def _check_core_comp(core, comp, n: int):
    """The per-row operands of the min-edge kernels."""
    import torch

    if core.shape != (n,) or comp.shape != (n,) or core.dtype != torch.float32 or comp.dtype != torch.int32:
        raise ValueError("core float32 [n] and comp int32 [n] expected")


def _check_core_pair(core_q, m: int, core, n: int, n_name: str):
    """The core distances of the two sides of a mutual-reachability query; `n_name`: what the message calls n."""
    import torch

    if core_q.shape != (m,) or core.shape != (n,) or core_q.dtype != torch.float32 or core.dtype != torch.float32:
        raise ValueError(f"core_q float32 [m] and core float32 [{n_name}] expected")


def _through_order(order, j):
    """Column indices j (int32, -1 = none) into rows sorted by `order`, as indices into the rows as the caller gave them."""
    import torch

    return torch.where(j >= 0, order.to(torch.int32)[j.clamp(min=0).long()], j)


# ------------------------------------------------------------------------------------------------ GPU: tree


def core_distances(x, min_samples: int, metric: str = "euclidean"):
    """Distance of every row of x [n, d] (device tensor) to its `min_samples`-th nearest row, itself included
    (sklearn's convention): float32 [n] on the device.  1 <= min_samples <= min(n, 64)."""
    import torch

    code = metric_code(metric)
    x = _prep(x)
    n, d = x.shape
    k = int(min_samples)
    if not 1 <= k <= n:
        raise ValueError(f"min_samples ({k}) must be in [1, n_samples = {n}]")
    lib = _lib.load()
    need = lib.wm_core_distance_workspace_bytes(n, d, k)
    ws = workspace(need, f"core_distances: unsupported sizes n={n} d={d} min_samples={k} (min_samples <= 64)", x.device)
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib.wm_core_distance(ptr(x), n, d, code, k, ptr(out), ptr(ws), need, stream_ptr()), "wm_core_distance")
    return out


def min_outgoing_edges(x, core, comp, metric: str = "euclidean", alpha: float = 1.0):
    """One Boruvka round: per row the lightest mutual-reachability edge to a row of another component
    (`comp` int32 [n]) as (weight float32 [n], j int32 [n]); j = -1 / weight = inf when there is none."""
    import torch

    code = metric_code(metric)
    x = _prep(x)
    require_gpu(core, comp)
    n, d = x.shape
    _check_core_comp(core, comp, n)
    lib = _lib.load()
    need = lib.wm_mreach_min_edge_workspace_bytes(n, d)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    w = torch.empty(n, dtype=torch.float32, device=x.device)
    j = torch.empty(n, dtype=torch.int32, device=x.device)
    check(lib.wm_mreach_min_edge(ptr(x), ptr(core), ptr(comp), n, d, code, 1.0 / float(alpha), ptr(w), ptr(j), ptr(ws),
                                 need, stream_ptr()), "wm_mreach_min_edge")
    return w, j


def _find_all(parent: np.ndarray) -> np.ndarray:
    """Root of every element (pointer jumping: O(log depth) vectorised passes)."""
    root = parent.copy()
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            return root
        root = nxt


def mutual_reachability_mst(x, min_samples: int, metric: str = "euclidean", alpha: float = 1.0, return_rounds: bool = False):
    """Minimum spanning tree of the mutual-reachability graph max(core_i, core_j, dist_ij / alpha) of x [n, d]
    (device tensor): (u, v, w) numpy arrays of the n - 1 edges, u < v, sorted by (w, u, v); w float64 holding the
    kernels' float32 weights.

    Boruvka: every round the kernel gives each row its lightest edge out of its component (ties to the lowest j);
    the host takes the per-component minimum under the total order (w, min(i, j), max(i, j)) -- which the lowest-j
    rule agrees with, and under which no round can close a cycle since an edge has the same weight bits from both
    ends -- merges, and renumbers the components.  At most ceil(log2 n) rounds."""
    if not alpha > 0:
        raise ValueError("alpha must be positive")
    x = _prep(x)
    out = _boruvka(x, core_distances(x, min_samples, metric), metric, alpha)
    return out if return_rounds else out[:3]


def _boruvka(x, core, metric: str, alpha: float, group=None, n_groups: int = 1):
    """mutual_reachability_mst's rounds on a prepared matrix and its core distances: (u, v, w, rounds).  With `group`
    (int32 device tensor [n], non-decreasing, every id in [0, n_groups) present; alpha 1) the rounds run on every
    group's own graph at once (wm_mreach_min_edge_grouped) and end at one component per group: a spanning forest of
    n - n_groups edges, found in at most ceil(log2 of the largest group) rounds."""
    import torch

    n = x.shape[0]
    parent = np.arange(n, dtype=np.int64)
    eu, ev, ew = [], [], []
    n_comp, rounds = n, 0
    comp = parent.copy()
    while n_comp > (1 if group is None else n_groups):
        comp_d = torch.from_numpy(comp.astype(np.int32)).to(x.device)
        if group is None:
            w_d, j_d = min_outgoing_edges(x, core, comp_d, metric, alpha)
        else:
            w_d, j_d = grouped_min_outgoing_edges(x, core, comp_d, group, n_groups, metric)
        w, j = w_d.cpu().numpy(), j_d.cpu().numpy().astype(np.int64)
        rounds += 1
        i = np.flatnonzero(j >= 0)
        if i.size == 0:
            raise _lib.WaferHipError("mutual_reachability_mst: no outgoing edge although several components remain")
        lo, hi = np.minimum(i, j[i]), np.maximum(i, j[i])
        order = np.lexsort((hi, lo, w[i], comp[i]))
        first = np.ones(order.size, dtype=bool)
        first[1:] = comp[i][order][1:] != comp[i][order][:-1]
        pick = order[first]  # one edge per component
        edges = np.unique(np.stack([lo[pick], hi[pick]], axis=1), axis=0)  # two components may pick the same edge
        for a, b in edges:
            ra, rb = a, b
            while parent[ra] != ra:
                ra = parent[ra]
            while parent[rb] != rb:
                rb = parent[rb]
            if ra == rb:
                raise _lib.WaferHipError("mutual_reachability_mst: a Boruvka round closed a cycle")
            parent[max(ra, rb)] = min(ra, rb)
            eu.append(a)
            ev.append(b)
            ew.append(float(w[a]) if j[a] == b else float(w[b]))
        comp = _find_all(parent)
        parent = comp.copy()
        n_comp = int(np.unique(comp).size)
    u, v, wt = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64), np.asarray(ew, dtype=np.float64)
    order = np.lexsort((v, u, wt))
    return u[order], v[order], wt[order], rounds


# ------------------------------------------------------------------------------------------------ host: tree -> labels


def _single_linkage(u, v, w, n):
    """scipy-format hierarchy (left, right, value, size as Python lists) from edges sorted by weight."""
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    left, right = [0] * (n - 1), [0] * (n - 1)
    for e in range(n - 1):
        a, b = int(u[e]), int(v[e])
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a == b:
            raise ValueError("labels_from_mst: the edges contain a cycle")
        node = n + e
        left[e], right[e] = a, b
        size[node] = size[a] + size[b]
        parent[a] = parent[b] = node
    return left, right, [float(t) for t in w], size


def _bfs(left, right, n, root):
    """Level order of the hierarchy below `root` (sklearn's bfs_from_hierarchy)."""
    out, level = [], [root]
    while level:
        out.extend(level)
        nxt = []
        for node in level:
            if node >= n:
                nxt.append(left[node - n])
                nxt.append(right[node - n])
        level = nxt
    return out


def _condense(left, right, value, size, n, min_cluster_size):
    root = 2 * n - 2
    relabel = {root: n}
    next_label = n + 1
    ignore = bytearray(2 * n - 1)
    rows = []
    for node in _bfs(left, right, n, root):
        if node < n or ignore[node]:
            continue
        l, r, dist = left[node - n], right[node - n], value[node - n]
        lam = 1.0 / dist if dist > 0.0 else math.inf
        lc, rc = size[l], size[r]
        me = relabel[node]
        if lc >= min_cluster_size and rc >= min_cluster_size:
            for child, cnt in ((l, lc), (r, rc)):
                relabel[child] = next_label
                rows.append((me, next_label, lam, cnt))
                next_label += 1
            continue
        fall = []
        if lc < min_cluster_size:
            fall.append(l)
        else:
            relabel[l] = me
        if rc < min_cluster_size:
            fall.append(r)
        else:
            relabel[r] = me
        for sub_root in fall:
            for sub in _bfs(left, right, n, sub_root):
                if sub < n:
                    rows.append((me, sub, lam, 1))
                ignore[sub] = 1
    return np.array(rows, dtype=CONDENSED_DTYPE)


def labels_from_mst(u, v, w, n: int, min_cluster_size: int, cluster_selection_epsilon: float = 0.0,
                    cluster_selection_method: str = "eom", allow_single_cluster: bool = False,
                    return_selected: bool = False) -> Tuple[np.ndarray, ...]:
    """Flat HDBSCAN clustering from the n - 1 spanning-tree edges (u, v, w), sorted by weight: single-linkage tree,
    condensed tree, stabilities, excess-of-mass or leaf selection, epsilon merge.  Pure numpy / Python on float64.

    Returns (labels int64 [n] with -1 for noise, probabilities float64 [n], condensed_tree): the condensed tree is
    a structured array (parent, child, lambda_val, child_size) in sklearn's row order.  Semantics are
    sklearn.cluster.HDBSCAN's (_tree.pyx) with one deliberate difference in `probabilities`: a cluster's death is
    the largest lambda over ALL its condensed rows, where sklearn takes the last contiguous run of them.  With
    `return_selected` a fourth value follows: the condensed-tree ids of the selected clusters, sorted, so that a
    cluster's position is its label."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    n, mcs = int(n), int(min_cluster_size)
    if n < 2 or u.shape != (n - 1,) or v.shape != (n - 1,) or w.shape != (n - 1,):
        raise ValueError("labels_from_mst needs n >= 2 and n - 1 edges")
    if mcs < 2:
        raise ValueError("min_cluster_size must be at least 2")
    if cluster_selection_epsilon < 0:
        raise ValueError("cluster_selection_epsilon must not be negative")
    if cluster_selection_method not in ("eom", "leaf"):
        raise ValueError("cluster_selection_method must be 'eom' or 'leaf'")
    if u.min() < 0 or v.min() < 0 or max(u.max(), v.max()) >= n:
        raise ValueError("edge endpoints must lie in [0, n)")
    if np.isnan(w).any() or (np.diff(w) < 0).any():
        raise ValueError("edge weights must be sorted ascending")
    eps = float(cluster_selection_epsilon)

    tree = _condense(*_single_linkage(u, v, w, n), n, mcs)
    parent, child, lam, csize = tree["parent"], tree["child"], tree["lambda_val"], tree["child_size"]
    root = n  # == parent.min()
    n_nodes = int(parent.max()) + 1
    is_cl = csize > 1
    # ---- stabilities, summed in row order as sklearn does
    births = np.full(max(int(child.max()), root) + 1, np.nan)
    births[child] = lam
    births[root] = 0.0
    stab_arr = np.zeros(n_nodes)
    with np.errstate(invalid="ignore"):
        np.add.at(stab_arr, parent, (lam - births[parent]) * csize)
    stability = {c: float(stab_arr[c]) for c in range(root, n_nodes)}
    children = {c: [] for c in stability}
    birth_lambda, cl_parent = {}, {}
    for p_, c_, l_ in zip(parent[is_cl].tolist(), child[is_cl].tolist(), lam[is_cl].tolist()):
        children[p_].append(c_)
        birth_lambda[c_] = l_
        cl_parent[c_] = p_

    def descendants(c):
        out, level = [], [c]
        while level:
            out.extend(level)
            level = [g for p_ in level for g in children[p_]]
        return out

    def traverse_upwards(leaf):
        p_ = cl_parent[leaf]
        if p_ == root:
            return p_ if allow_single_cluster else leaf
        with np.errstate(divide="ignore"):
            parent_eps = 1.0 / birth_lambda[p_] if birth_lambda[p_] != 0 else math.inf
        return p_ if parent_eps > eps else traverse_upwards(p_)

    def epsilon_search(leaves):
        selected, processed = [], set()
        for leaf in sorted(leaves):
            leaf_eps = 1.0 / birth_lambda[leaf] if birth_lambda[leaf] != 0 else math.inf
            if leaf_eps < eps:
                if leaf not in processed:
                    top = traverse_upwards(leaf)
                    selected.append(top)
                    processed.update(s for s in descendants(top) if s != top)
            else:
                selected.append(leaf)
        return set(selected)

    node_list = sorted(stability, reverse=True)
    if not allow_single_cluster:
        node_list = node_list[:-1]
    is_cluster = {c: True for c in node_list}
    has_cluster_rows = bool(is_cl.any())
    if cluster_selection_method == "eom":
        for node in node_list:
            subtree = float(np.sum([stability[c] for c in children[node]]))
            if subtree > stability[node]:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in descendants(node):
                    if sub != node:
                        is_cluster[sub] = False
        if eps != 0.0 and has_cluster_rows:
            eom = [c for c in is_cluster if is_cluster[c]]
            if len(eom) == 1 and eom[0] == root:
                selected = set(eom) if allow_single_cluster else set()
            else:
                selected = epsilon_search(set(eom))
            for c in is_cluster:
                is_cluster[c] = c in selected
    else:
        leaves = {c for c in children if not children[c]} if has_cluster_rows else set()
        if not leaves:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[root] = True
            selected = set()
        elif eps != 0.0:
            selected = epsilon_search(leaves)
        else:
            selected = leaves
        if leaves:
            for c in is_cluster:
                is_cluster[c] = c in selected
    clusters = sorted(c for c in is_cluster if is_cluster[c])
    label_of = {c: i for i, c in enumerate(clusters)}

    # ---- labels: the nearest selected cluster on the way up from the point's condensed parent
    top = np.full(n_nodes, root, dtype=np.int64)
    selected_set = set(clusters)
    for c in range(root + 1, n_nodes):  # (ids grow downwards: a parent is numbered before its children)
        top[c] = c if c in selected_set else top[cl_parent[c]]
    pts = ~is_cl
    p_child, p_top, p_lam = child[pts], top[parent[pts]], lam[pts]
    lab_map = np.full(n_nodes, -1, dtype=np.int64)
    for c, i in label_of.items():
        lab_map[c] = i
    labels = np.full(n, -1, dtype=np.int64)
    under = p_top != root
    labels[p_child[under]] = lab_map[p_top[under]]
    if len(clusters) == 1 and allow_single_cluster and (~under).any():
        threshold = 1.0 / eps if eps != 0.0 else float(lam[parent == root].max())
        keep = ~under & (p_lam >= threshold)
        labels[p_child[keep]] = label_of.get(root, -1)
    # ---- membership strengths
    deaths = np.zeros(n_nodes)
    np.maximum.at(deaths, parent, lam)
    prob = np.zeros(n)
    lab_pts = labels[p_child]
    has = lab_pts >= 0
    death = deaths[np.asarray(clusters, dtype=np.int64)[lab_pts[has]]] if clusters else np.zeros(0)
    lam_h = p_lam[has]
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where((death == 0.0) | np.isinf(lam_h), 1.0, np.minimum(lam_h, death) / death)
    prob[p_child[has]] = val
    if return_selected:
        return labels, prob, tree, np.asarray(clusters, dtype=np.int64)
    return labels, prob, tree


# ------------------------------------------------------------------------------------------------ host: outliers, new rows


def _tree_tables(tree, n: int):
    """Per-node tables of a condensed tree: (n_nodes, cluster parent [n_nodes] (the root is its own), birth lambda
    [n_nodes] (0 at the root), death [n_nodes] = the largest lambda over the cluster's own rows, D [n_nodes] = the
    death propagated upwards over cluster children, per point its parent [n] and its lambda [n])."""
    parent, child, lam, csize = tree["parent"], tree["child"], tree["lambda_val"], tree["child_size"]
    n_nodes = int(parent.max()) + 1
    is_cl = csize > 1
    cl_parent = np.arange(n_nodes, dtype=np.int64)
    cl_parent[child[is_cl]] = parent[is_cl]
    birth = np.zeros(n_nodes)
    birth[child[is_cl]] = lam[is_cl]
    death = np.zeros(n_nodes)
    np.maximum.at(death, parent, lam)
    spread = death.copy()
    for c in range(n_nodes - 1, n, -1):  # (ids grow downwards: every child is visited before its parent)
        spread[cl_parent[c]] = max(spread[cl_parent[c]], spread[c])
    pt_parent, pt_lam = np.full(n, n, dtype=np.int64), np.zeros(n)
    pt_parent[child[~is_cl]], pt_lam[child[~is_cl]] = parent[~is_cl], lam[~is_cl]
    return n_nodes, cl_parent, birth, death, spread, pt_parent, pt_lam


def _glosh_ratio(spread, lam):
    """(spread - lam) / spread, clipped below at 0: 0 where spread == 0 or lam is not finite, and the limit 1 where
    only spread is infinite (a cluster that holds exact duplicates)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.maximum((spread - lam) / spread, 0.0)
    val = np.where(np.isinf(spread), 1.0, val)
    return np.where((spread == 0.0) | ~np.isfinite(lam), 0.0, val)


def glosh(condensed_tree, n: int) -> np.ndarray:
    """GLOSH outlier scores of the n fitted rows (the `hdbscan` package's `outlier_scores_`), float64 [n] in [0, 1].
    D[c] is the largest lambda among cluster c's own condensed rows, propagated upwards so that a parent's D is at
    least each cluster child's; a point that leaves cluster P at lambda l scores (D[P] - l) / D[P], and 0 where
    D[P] == 0 or l is not finite."""
    n = int(n)
    _, _, _, _, spread, pt_parent, pt_lam = _tree_tables(condensed_tree, n)
    return _glosh_ratio(spread[pt_parent], pt_lam)


def _walk(root, cl_parent, birth, pt_parent, pt_lam, neighbor, weight):
    """The walk of a new row into the condensed tree (assign_from_tree states the rule): (C int64 [m], the cluster the
    row would fall out of; lam float64 [m] = 1 / weight, inf at weight 0)."""
    with np.errstate(divide="ignore"):
        lam = 1.0 / weight
    at = pt_parent[neighbor]
    climb = pt_lam[neighbor] > lam
    while True:
        move = climb & (at != root) & (birth[at] >= lam)
        if not move.any():
            break
        at = np.where(move, cl_parent[at], at)
    return at, lam


def assign_from_tree(condensed_tree, n: int, selected, neighbor, weight, cluster_selection_epsilon: float = 0.0,
                     allow_single_cluster: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Labels, membership strengths and outlier scores of new rows from the fitted condensed tree: (labels int64 [m],
    probabilities float64 [m], outlier_scores float64 [m]).  Pure numpy on float64.

    `selected`: the sorted condensed-tree ids of the flat clustering (labels_from_mst(..., return_selected=True));
    `neighbor` [m]: per new row the fitted row nearest in mutual reachability; `weight` [m]: that mutual
    reachability.  Per row, with lam = 1 / weight (inf at weight 0) and (P, l_nb) the neighbour's condensed row: the
    row joins C = P when l_nb <= lam (the neighbour has left P before the row would), otherwise the first cluster
    on the way up from P that was born before lam (or the root).  The label is that of S, the nearest selected
    cluster on the way up from C, C included; none: -1 with probability 0.  Where the root itself is the selected
    cluster (allow_single_cluster) a row that ends at it belongs when lam reaches the threshold of labels_from_mst's
    branch for that case: 1 / epsilon, or without an epsilon the largest lambda among the root's own rows.  The
    probability is min(lam, death[S]) / death[S] with labels_from_mst's death, and 1 where death[S] == 0 or lam is
    infinite; the outlier score is max(0, (D[C] - lam) / D[C]) with glosh's D, and 0 where D[C] == 0 or lam is
    infinite."""
    n = int(n)
    selected = np.asarray(selected, dtype=np.int64)
    neighbor = np.asarray(neighbor, dtype=np.int64)
    weight = np.asarray(weight, dtype=np.float64)
    if neighbor.ndim != 1 or weight.shape != neighbor.shape:
        raise ValueError("neighbor [m] and weight [m] expected")
    if neighbor.size and (neighbor.min() < 0 or neighbor.max() >= n):
        raise ValueError("neighbor must lie in [0, n)")
    if np.isnan(weight).any() or (weight < 0).any():
        raise ValueError("weight must not be negative")
    if (np.diff(selected) <= 0).any():
        raise ValueError("selected must be sorted condensed-tree ids")
    eps = float(cluster_selection_epsilon)
    n_nodes, cl_parent, birth, death, spread, pt_parent, pt_lam = _tree_tables(condensed_tree, n)
    root = n
    if selected.size and (selected.min() < root or selected.max() >= n_nodes):
        raise ValueError("selected must hold cluster ids of the condensed tree")
    at, lam = _walk(root, cl_parent, birth, pt_parent, pt_lam, neighbor, weight)
    # ---- S: the nearest selected cluster from C upwards (the root stands for "none", as in labels_from_mst)
    label_at = np.full(n_nodes, -1, dtype=np.int64)
    label_at[selected] = np.arange(selected.size)
    top = np.full(n_nodes, root, dtype=np.int64)
    for c in range(root + 1, n_nodes):
        top[c] = c if label_at[c] >= 0 else top[cl_parent[c]]
    s = top[at]
    labels = np.where(s != root, label_at[s], -1)
    if selected.size == 1 and selected[0] == root and allow_single_cluster:
        tree = condensed_tree
        threshold = 1.0 / eps if eps != 0.0 else float(tree["lambda_val"][tree["parent"] == root].max())
        labels = np.where(lam >= threshold, 0, -1)  # (every walk ends at the root here: nothing else is selected)
    has = labels >= 0
    d_s = death[s]
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = np.where((d_s == 0.0) | np.isinf(lam), 1.0, np.minimum(lam, d_s) / d_s)
    prob = np.where(has, prob, 0.0)
    return labels.astype(np.int64), prob, _glosh_ratio(spread[at], lam)


def _checked_selected(selected, root: int, n_nodes: int) -> np.ndarray:
    selected = np.asarray(selected, dtype=np.int64)
    if selected.ndim != 1 or (np.diff(selected) <= 0).any():
        raise ValueError("selected must be sorted condensed-tree ids")
    if selected.size and (selected.min() < root or selected.max() >= n_nodes):
        raise ValueError("selected must hold cluster ids of the condensed tree")
    return selected


def exemplars_from_tree(condensed_tree, n: int, selected) -> list:
    """The exemplar rows of every selected cluster (the `hdbscan` package's `exemplars_`, as row indices): a list of
    ascending int64 arrays, one per entry of `selected`.  For every leaf cluster L of the condensed tree below S (S
    itself when it has no cluster child) the exemplars are L's own rows that leave last, those whose lambda equals
    death[L], the largest lambda among L's rows.  A leaf counts for the nearest selected cluster from it upwards (the
    flat clusterings of labels_from_mst never select a cluster below another one)."""
    n = int(n)
    n_nodes, cl_parent, _, death, _, pt_parent, pt_lam = _tree_tables(condensed_tree, n)
    selected = _checked_selected(selected, n, n_nodes)
    is_leaf = np.ones(n_nodes, dtype=bool)
    is_leaf[cl_parent[n + 1:]] = False  # (the root is its own parent: only real children are listed)
    cand = np.flatnonzero(is_leaf[pt_parent] & (pt_lam == death[pt_parent]))
    under = np.full(n_nodes, -1, dtype=np.int64)  # position in `selected` of the nearest selected cluster from a node up
    under[selected] = np.arange(selected.size)
    for c in range(n + 1, n_nodes):  # (ids grow downwards: a parent is numbered before its children)
        if under[c] < 0:
            under[c] = under[cl_parent[c]]
    owner = under[pt_parent[cand]]
    return [cand[owner == s].astype(np.int64) for s in range(selected.size)]


def membership_from_tree(condensed_tree, n: int, selected, at, lam, exemplar_dist, return_parts: bool = False):
    """Soft-clustering membership vectors from the fitted condensed tree: float64 [m, C], one column per entry of
    `selected`, every entry in [0, 1] and every row summing to the row's probability of belonging to any cluster.  Pure
    numpy on float64; the formulas are the `hdbscan` package's prediction module's, with two deliberate differences
    marked below.

    `at` [m]: the condensed cluster a row sits in; `lam` [m]: the lambda at which it leaves it (an infinite one is
    replaced by the largest lambda below `at`, or where that is infinite too by the largest finite lambda of the
    tree); `exemplar_dist` [m, C]: the distance to the nearest exemplar of every selected cluster (inf: none).
    Infinite lambdas of the tree itself (exact duplicates: a cluster that holds min_cluster_size of them has an
    infinite death, and so have its ancestors) count as the largest finite lambda of the tree throughout, the value
    an infinite `lam` gets: every score and probability stays a ratio of finite numbers, a duplicate is the last to
    leave its cluster (p = 1 there), and the other rows of the model are scored against a finite depth.  (The limit of
    the formulas at an infinite death would instead give every row under such a cluster p = 0.)  Per row i and selected
    cluster S_c, with D = glosh's propagated death, capped so:
      distance vector   a_c = 1 / exemplar_dist[i, c], normalised to sum 1; with a zero distance the indicator of the
                        zero entries, normalised; 0 at an infinite distance;
      merge height      h_c = lam_i when S_c is at_i, above it or below it; otherwise the lambda at which their lowest
                        common ancestor split (the birth of its children);
      score             s_c = m_c / (m_c - h_c) with m_c = max(lam_i, D[S_c]), +inf at a zero denominator (deliberate:
                        the package adds a small constant to the denominator instead);
      outlier vector    the softmax of s over c; with an infinite s the indicator of the infinite ones, normalised;
      probability       p_i = h* / max(lam_i, D[S_c*]) with h* the largest h_c and c* the first cluster that attains
                        it; 0 at a zero denominator;
      result            a * outlier, normalised to sum 1, times p_i (deliberate: the same formula for fitted and for
                        new rows, where the package raises the two factors to different powers in its two functions).
    A row whose product vanishes everywhere (every distance infinite) is all zeros.  Where the root is the only selected
    cluster (allow_single_cluster) the one column holds p_i = lam_i / max(lam_i, the largest lambda of the tree): how far
    down the tree the row stays, 1 for the last rows to leave.  C == 0 gives [m, 0].  With `return_parts` a dict of the
    intermediate arrays (a, h, s, outlier [m, C]; p, lam [m]) follows."""
    n = int(n)
    n_nodes, cl_parent, birth, _, spread, _, _ = _tree_tables(condensed_tree, n)
    selected = _checked_selected(selected, n, n_nodes)
    at = np.asarray(at, dtype=np.int64)
    lam = np.asarray(lam, dtype=np.float64).copy()
    dist = np.asarray(exemplar_dist, dtype=np.float64)
    m, n_sel = at.shape[0], selected.size
    if at.ndim != 1 or lam.shape != (m,) or dist.shape != (m, n_sel):
        raise ValueError("at [m], lam [m] and exemplar_dist [m, C] expected")
    if m and (at.min() < n or at.max() >= n_nodes):
        raise ValueError("at must hold cluster ids of the condensed tree")
    if np.isnan(lam).any() or (lam < 0).any() or np.isnan(dist).any() or (dist < 0).any():
        raise ValueError("lam and exemplar_dist must not be negative")
    if n_sel == 0:
        out = np.zeros((m, 0))
        return (out, {"a": out, "h": out, "s": out, "outlier": out, "p": np.zeros(m), "lam": lam}) if return_parts else out
    all_lam = condensed_tree["lambda_val"]
    top_lam = float(all_lam[np.isfinite(all_lam)].max()) if np.isfinite(all_lam).any() else 0.0
    spread, birth = np.minimum(spread, top_lam), np.minimum(birth, top_lam)  # (unchanged where the tree is finite)
    inf_lam = np.isinf(lam)
    lam[inf_lam] = spread[at[inf_lam]]
    # ---- per (tree cluster k, selected cluster c): on one lineage or not, and where not the split lambda of their
    # lowest common ancestor.  Ids grow downwards, so one pass in id order sees every parent before its children.
    k_nodes = n_nodes - n
    par = cl_parent[n:] - n
    sel = selected - n
    above = np.zeros((k_nodes, n_sel), dtype=bool)  # S_c is k or an ancestor of k
    above[sel, np.arange(n_sel)] = True
    below = np.zeros((k_nodes, n_sel), dtype=bool)  # S_c is a descendant of k
    for k in range(1, k_nodes):
        above[k] |= above[par[k]]
    for k in range(k_nodes - 1, 0, -1):
        below[par[k]] |= below[k] | (sel == k)
    lineage = above | below
    split = np.zeros((k_nodes, n_sel))
    for k in range(1, k_nodes):  # (off the lineage the parent is either the common ancestor or off it as well)
        split[k] = np.where(lineage[par[k]], birth[n + k], split[par[k]])
    big = spread[selected]  # D[S_c]
    # ---- per row
    lam_c = lam[:, None]
    h = np.where(lineage[at - n], lam_c, split[at - n])
    m_c = np.maximum(lam_c, big[None, :])
    den = m_c - h
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den == 0.0, np.inf, m_c / den)
        inv = np.where(np.isinf(dist), 0.0, 1.0 / dist)
    zero = dist == 0.0
    a = np.where(zero.any(axis=1, keepdims=True), zero.astype(np.float64), inv)
    a_sum = a.sum(axis=1, keepdims=True)
    a = np.divide(a, a_sum, out=np.zeros_like(a), where=a_sum > 0)
    s_inf = np.isinf(s)
    with np.errstate(invalid="ignore", over="ignore"):
        soft = np.exp(np.where(s_inf, -np.inf, s) - np.where(s_inf, -np.inf, s).max(axis=1, keepdims=True))
    soft = np.where(s_inf.any(axis=1, keepdims=True), s_inf.astype(np.float64), soft)
    outlier = soft / soft.sum(axis=1, keepdims=True)
    c_star = np.argmax(h, axis=1)
    h_star = h[np.arange(m), c_star]
    p_den = np.maximum(lam, big[c_star])
    p = np.divide(h_star, p_den, out=np.zeros(m), where=p_den != 0.0)
    prod = a * outlier
    p_sum = prod.sum(axis=1, keepdims=True)
    out = np.divide(prod, p_sum, out=np.zeros_like(prod), where=p_sum > 0) * p[:, None]
    if return_parts:
        return out, {"a": a, "h": h, "s": s, "outlier": outlier, "p": p, "lam": lam}
    return out


class HDBSCAN:
    """sklearn.cluster.HDBSCAN on device tensors: `.fit(x)` / `.fit_predict(x)` set `labels_`, `probabilities_`,
    `condensed_tree_` and `minimum_spanning_tree_` (numpy [n - 1, 3]: u, v, weight; kept whether or not
    `gen_min_span_tree` is set, since `refit` needs it).  `min_samples=None` means `min_cluster_size`.
    `refit(min_cluster_size=..., cluster_selection_epsilon=...)` relabels from the stored tree: the tree depends on
    (metric, min_samples, alpha) only.  `fit` and `refit` also set `selected_clusters_` (the sorted condensed-tree ids
    of the clusters: position = label) and `outlier_scores_` (`glosh`); `relative_validity_` scores the labelling from the
    tree alone.  With `prediction_data=True`, `fit` keeps the
    prepared device matrix and the device core distances, which `approximate_predict` needs."""

    def __init__(self, min_cluster_size: int = 5, min_samples: Optional[int] = None, cluster_selection_epsilon: float = 0.0,
                 metric: str = "euclidean", alpha: float = 1.0, cluster_selection_method: str = "eom",
                 allow_single_cluster: bool = False, gen_min_span_tree: bool = False, prediction_data: bool = False):
        metric_code(metric)
        if cluster_selection_method not in ("eom", "leaf"):
            raise ValueError("cluster_selection_method must be 'eom' or 'leaf'")
        if int(min_cluster_size) < 2:
            raise ValueError("min_cluster_size must be at least 2")
        if min_samples is not None and int(min_samples) < 1:
            raise ValueError("min_samples must be at least 1")
        if cluster_selection_epsilon < 0 or not alpha > 0:
            raise ValueError("cluster_selection_epsilon >= 0 and alpha > 0 required")
        self.min_cluster_size, self.min_samples = int(min_cluster_size), min_samples
        self.cluster_selection_epsilon, self.metric, self.alpha = float(cluster_selection_epsilon), metric, float(alpha)
        self.cluster_selection_method, self.allow_single_cluster = cluster_selection_method, bool(allow_single_cluster)
        self.gen_min_span_tree, self.prediction_data = bool(gen_min_span_tree), bool(prediction_data)
        self.labels_ = self.probabilities_ = self.condensed_tree_ = self.minimum_spanning_tree_ = None
        self.selected_clusters_ = self.outlier_scores_ = None
        self._n = self._k = self._train = self._core = self._exemplars = self._relative_validity = None

    def fit(self, x) -> "HDBSCAN":
        k = self.min_cluster_size if self.min_samples is None else int(self.min_samples)
        if k > x.shape[0]:
            raise ValueError(f"min_samples ({k}) must be at most the number of samples ({x.shape[0]})")
        xp = _prep(x)
        core = core_distances(xp, k, self.metric)
        u, v, w, _ = _boruvka(xp, core, self.metric, self.alpha)
        self._n, self._k = int(x.shape[0]), k
        self._train, self._core = (xp, core) if self.prediction_data else (None, None)
        self.minimum_spanning_tree_ = np.stack([u.astype(np.float64), v.astype(np.float64), w], axis=1)
        return self._label()

    def refit(self, min_cluster_size: Optional[int] = None, cluster_selection_epsilon: Optional[float] = None) -> "HDBSCAN":
        if self.minimum_spanning_tree_ is None:
            raise RuntimeError("HDBSCAN.refit before fit")
        if min_cluster_size is not None:
            self.min_cluster_size = int(min_cluster_size)
        if cluster_selection_epsilon is not None:
            self.cluster_selection_epsilon = float(cluster_selection_epsilon)
        return self._label()

    def _label(self) -> "HDBSCAN":
        t = self.minimum_spanning_tree_
        self.labels_, self.probabilities_, self.condensed_tree_, self.selected_clusters_ = labels_from_mst(
            t[:, 0].astype(np.int64), t[:, 1].astype(np.int64), t[:, 2], self._n, self.min_cluster_size,
            self.cluster_selection_epsilon, self.cluster_selection_method, self.allow_single_cluster, return_selected=True)
        self.outlier_scores_ = glosh(self.condensed_tree_, self._n)
        self._exemplars = self._relative_validity = None
        return self

    @property
    def relative_validity_(self):
        """`relative_validity` of the fitted tree under the current labels (a float; no GPU work); None before `fit`.
        Computed on first access after a `fit` / `refit`."""
        if self.labels_ is None:
            return None
        if self._relative_validity is None:
            self._relative_validity = relative_validity(self.minimum_spanning_tree_, self.labels_)
        return self._relative_validity

    @property
    def exemplar_indices_(self):
        """The exemplar rows of every cluster (`exemplars_from_tree`), a list in label order; None before `fit`.
        Computed on first access after a `fit` / `refit`."""
        if self.condensed_tree_ is None:
            return None
        if self._exemplars is None:
            self._exemplars = exemplars_from_tree(self.condensed_tree_, self._n, self.selected_clusters_)
        return self._exemplars

    def fit_predict(self, x) -> np.ndarray:
        return self.fit(x).labels_


# ------------------------------------------------------------------------------------------------ GPU: new rows


def query_core_distances(xq, x, min_samples: int, metric: str = "euclidean"):
    """Core distances of new rows xq [m, d] against the fitted rows x [n, d] (device tensors) under this module's
    convention, the row counting itself: the `min_samples`-th smallest of {0} and the distances to the fitted rows,
    that is the distance to the (min_samples - 1)-th nearest fitted row (wm_knn_query with min_samples - 1
    neighbours).  float32 [m] on the device; min_samples == 1 gives zeros and launches nothing."""
    import torch

    from .manifold import knn_query  # (manifold imports this module)

    metric_code(metric)
    xq, x = _prep(xq), _prep(x)
    m, n = xq.shape[0], x.shape[0]
    k = int(min_samples) - 1
    if not 0 <= k <= n:
        raise ValueError(f"min_samples ({k + 1}) must be in [1, n_samples + 1 = {n + 1}]")
    if k == 0 or m == 0:
        return torch.zeros(m, dtype=torch.float32, device=xq.device)
    return knn_query(xq, x, k, metric)[0][:, k - 1].contiguous()


def mreach_query(xq, core_q, x, core, metric: str = "euclidean", alpha: float = 1.0):
    """Per row of xq [m, d] the fitted row of x [n, d] nearest in mutual reachability
    max(core_q[i], core[c], dist_ic / alpha), equal weights resolved by the smaller distance and then the lower
    index: (weight float32 [m], dist float32 [m], j int32 [m]) on the device (wm_mreach_query; an exact search over
    all fitted rows)."""
    import torch

    code = metric_code(metric)
    if not alpha > 0:
        raise ValueError("alpha must be positive")
    xq, x = _prep(xq), _prep(x)
    require_gpu(core_q, core)
    (m, d), n = xq.shape, x.shape[0]
    if x.shape[1] != d:
        raise ValueError(f"the new rows have {d} features (padded), the fitted rows {x.shape[1]}")
    _check_core_pair(core_q, m, core, n, "n")
    if m < 1 or n < 1:
        raise ValueError("mreach_query needs at least one row on either side")
    lib = _lib.load()
    need = lib.wm_mreach_query_workspace_bytes(m, n, d)
    ws = workspace(need, f"mreach_query: unsupported sizes m={m} n={n} d={d}", xq.device)
    w = torch.empty(m, dtype=torch.float32, device=xq.device)
    dist = torch.empty(m, dtype=torch.float32, device=xq.device)
    j = torch.empty(m, dtype=torch.int32, device=xq.device)
    check(lib.wm_mreach_query(ptr(xq), ptr(core_q), m, ptr(x), ptr(core), n, d, code, 1.0 / float(alpha), ptr(w), ptr(dist),
                              ptr(j), ptr(ws), need, stream_ptr()), "wm_mreach_query")
    return w, dist, j


def _require_prediction_data(model: "HDBSCAN"):
    if model.minimum_spanning_tree_ is None:
        raise RuntimeError("HDBSCAN prediction before fit")
    if model._train is None or model._core is None:
        raise ValueError("this model keeps no prediction data: construct it with HDBSCAN(..., prediction_data=True)")


def _nearest_fitted(model: "HDBSCAN", rows):
    """What every prediction for new rows starts from: (prepared rows, neighbor int64 [m], weight float64 [m]), the
    fitted row nearest in mutual reachability and that mutual reachability; (rows, None, None) when there are none."""
    _require_prediction_data(model)
    xq = _prep(rows)
    if xq.shape[1] != model._train.shape[1]:
        raise ValueError(f"rows have {rows.shape[1]} features, the model was fitted on {model._train.shape[1]} (after padding)")
    if xq.shape[0] == 0:
        return xq, None, None
    core_q = query_core_distances(xq, model._train, model._k, model.metric)
    w, _, j = mreach_query(xq, core_q, model._train, model._core, model.metric, model.alpha)
    return xq, j.cpu().numpy().astype(np.int64), w.cpu().numpy().astype(np.float64)


def _predict(model: "HDBSCAN", rows):
    _, j, w = _nearest_fitted(model, rows)
    if j is None:
        return np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0)
    return assign_from_tree(model.condensed_tree_, model._n, model.selected_clusters_, j, w, model.cluster_selection_epsilon,
                            model.allow_single_cluster)


def approximate_predict(model: "HDBSCAN", rows) -> Tuple[np.ndarray, np.ndarray]:
    """Cluster labels and membership strengths of new rows [m, d] (device tensor with the fitted feature count) under
    a model fitted with `prediction_data=True`: (labels int64 [m], probabilities float64 [m]), numpy like `labels_`.
    The fitted clustering does not change.  The name is the `hdbscan` package's; two deliberate differences:
    the nearest fitted row in mutual reachability is found by an exact search over all fitted rows (wm_mreach_query)
    where `hdbscan` looks among the 2 * min_samples nearest only; and the core distance of a new row counts the row
    itself, as `fit` does here (the min_samples-th smallest of zero and the distances to the fitted rows), where
    `hdbscan` counts one neighbour further.  A model that follows a `refit` predicts under the relabelling."""
    labels, prob, _ = _predict(model, rows)
    return labels, prob


def approximate_predict_scores(model: "HDBSCAN", rows) -> np.ndarray:
    """GLOSH outlier scores of new rows under a model fitted with `prediction_data=True`: float64 [m] in [0, 1]
    (see `assign_from_tree`; the search and the core-distance convention are `approximate_predict`'s)."""
    return _predict(model, rows)[2]


# ------------------------------------------------------------------------------------------------ GPU: soft clustering


def group_min_distances(xq, xe, group, n_groups: int, metric: str = "euclidean"):
    """Per row of xq [m, d] and per group c in [0, n_groups) the nearest row of xe [e, d] among those with
    group[j] == c: (dist float32 [m, n_groups], j int32 [m, n_groups]) on the device (wm_group_min_dist); j is the lowest
    index into xe that attains the distance, and a group without a row gives inf / -1.  `group`: e integers in
    [0, n_groups) in any order (a tensor or an array): the columns are sorted by (group, index) for the kernel, which
    wants the groups in runs, and the indices mapped back.  The distances are `manifold.knn_query`'s bits."""
    import torch

    code = metric_code(metric)
    xq, xe = _prep(xq), _prep(xe)
    (m, d), e, g = xq.shape, xe.shape[0], int(n_groups)
    if xe.shape[1] != d:
        raise ValueError(f"the rows have {d} features (padded), the grouped rows {xe.shape[1]}")
    group = torch.as_tensor(group)
    if group.shape != (e,) or group.dtype not in (torch.int32, torch.int64):
        raise ValueError("group: one int32 / int64 id per row of xe expected")
    if g < 0 or (e and (int(group.min()) < 0 or int(group.max()) >= g)):
        raise ValueError(f"group ids must lie in [0, n_groups = {g})")
    dist = torch.full((m, g), float("inf"), dtype=torch.float32, device=xq.device)
    j = torch.full((m, g), -1, dtype=torch.int32, device=xq.device)
    if m == 0 or e == 0 or g == 0:
        return dist, j  # (nothing to compare)
    order = torch.argsort(group.to(xq.device), stable=True)  # by (group, index)
    xs = xe[order].contiguous()
    gs = group.to(xq.device)[order].to(torch.int32).contiguous()
    lib = _lib.load()
    need = lib.wm_group_min_dist_workspace_bytes(m, e, d, g)
    ws = workspace(need, f"group_min_distances: unsupported sizes m={m} e={e} d={d} n_groups={g}", xq.device)
    check(lib.wm_group_min_dist(ptr(xq), m, ptr(xs), ptr(gs), e, d, code, g, ptr(dist), ptr(j), ptr(ws), need, stream_ptr()),
          "wm_group_min_dist")
    return dist, _through_order(order, j)


def _exemplar_distances(model: "HDBSCAN", xq) -> np.ndarray:
    """float64 [m, C]: the distance of every prepared row to the nearest exemplar of every cluster of the model."""
    import torch

    ex = model.exemplar_indices_
    rows = np.concatenate(ex) if ex else np.zeros(0, dtype=np.int64)
    group = np.repeat(np.arange(len(ex)), [r.size for r in ex]) if ex else np.zeros(0, dtype=np.int64)
    xe = model._train[torch.from_numpy(rows).to(model._train.device)]
    return group_min_distances(xq, xe, torch.from_numpy(group), len(ex), model.metric)[0].cpu().numpy().astype(np.float64)


def all_points_membership_vectors(model: "HDBSCAN") -> np.ndarray:
    """Soft clustering of the fitted rows under a model fitted with `prediction_data=True`: float64 [n, C], one column
    per cluster in label order (`membership_from_tree`, which states the formulas and what the one column of a
    single root cluster holds).  A row sits in its own condensed parent at its own lambda; the distances to the
    clusters' nearest exemplars (`exemplar_indices_`) are one pass of wm_group_min_dist over the stored matrix.  The
    name is the `hdbscan` package's.  A model that follows a `refit` answers under the relabelling."""
    _require_prediction_data(model)
    _, _, _, _, _, pt_parent, pt_lam = _tree_tables(model.condensed_tree_, model._n)
    return membership_from_tree(model.condensed_tree_, model._n, model.selected_clusters_, pt_parent, pt_lam,
                                _exemplar_distances(model, model._train))


def membership_vector(model: "HDBSCAN", rows) -> np.ndarray:
    """Soft clustering of new rows [m, d] under a model fitted with `prediction_data=True`: float64 [m, C].  A new row
    sits in the cluster C and at the lambda 1 / weight of `approximate_predict`'s walk (the same search, the same
    code); the rest is `all_points_membership_vectors`'.  The refusals are `approximate_predict`'s."""
    xq, j, w = _nearest_fitted(model, rows)
    if j is None:
        return np.zeros((0, model.selected_clusters_.size))
    n = model._n
    _, cl_parent, birth, _, _, pt_parent, pt_lam = _tree_tables(model.condensed_tree_, n)
    at, lam = _walk(n, cl_parent, birth, pt_parent, pt_lam, j, w)
    return membership_from_tree(model.condensed_tree_, n, model.selected_clusters_, at, lam, _exemplar_distances(model, xq))


# ------------------------------------------------------------------------------------------------ GPU: DBCV


def _sorted_groups(group, n: int, g: int, device):
    """(order or None, group int32 on the device in non-decreasing order): `order` sorts the rows by (group, index) and is
    None when they already are."""
    import torch

    group = torch.as_tensor(group)
    if group.shape != (n,) or group.dtype not in (torch.int32, torch.int64):
        raise ValueError("group: one int32 / int64 id per row expected")
    if g < 1 or (n and (int(group.min()) < 0 or int(group.max()) >= g)):
        raise ValueError(f"group ids must lie in [0, n_groups = {g})")
    group = group.to(device)
    if n < 2 or bool((group[1:] >= group[:-1]).all()):
        return None, group.to(torch.int32).contiguous()
    order = torch.argsort(group, stable=True)
    return order, group[order].to(torch.int32).contiguous()


def allpoints_core_distances(x, labels, d: Optional[float] = None, metric: str = "euclidean"):
    """DBCV's all-points core distance of every row of x [n, D] (device tensor) inside its own cluster:
    ((1 / (n_c - 1)) * sum_j dist_ij^-p)^(-1 / p) over the rows j of the cluster at a positive distance, with p = `d`,
    or D as passed (before the padding to a multiple of 4) when `d` is None.  float64 [n] on the device
    (wm_allpoints_core: the sum is a log-sum-exp, so no p overflows); NaN on the noise rows (label -1), 0 for a row
    whose cluster holds nothing but copies of it.  `labels`: any integer array or tensor [n]."""
    import torch

    code = metric_code(metric)
    p = float(x.shape[1] if d is None else d)
    if not 0 < p < math.inf:
        raise ValueError(f"d must be positive and finite (got {d})")
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)
    if lab.shape != (x.shape[0],) or lab.dtype.kind not in "iu":
        raise ValueError("one integer label per row expected")
    x = _prep(x)
    n, dim = x.shape
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=x.device)
    keep = np.flatnonzero(lab >= 0)
    if keep.size == 0:
        return out
    _, enc = np.unique(lab[keep], return_inverse=True)
    order = np.argsort(enc, kind="stable")  # by (cluster, index)
    rows = torch.from_numpy(keep[order]).to(x.device)
    xs = x[rows].contiguous()
    gs = torch.from_numpy(enc[order].astype(np.int32)).to(x.device)
    m, g = int(keep.size), int(enc.max()) + 1
    lib = _lib.load()
    need = lib.wm_allpoints_core_workspace_bytes(m, dim, g)
    ws = workspace(need, f"allpoints_core_distances: unsupported sizes n={m} d={dim} clusters={g}", x.device)
    res = torch.empty(m, dtype=torch.float64, device=x.device)
    check(lib.wm_allpoints_core(ptr(xs), ptr(gs), m, dim, code, g, p, ptr(res), ptr(ws), need, stream_ptr()), "wm_allpoints_core")
    out[rows] = res
    return out


def grouped_min_outgoing_edges(x, core, comp, group, n_groups: int, metric: str = "euclidean"):
    """`min_outgoing_edges` (alpha 1) inside every group at once: per row the lightest mutual-reachability edge to a row
    of its own group in another component, as (weight float32 [n], j int32 [n]); -1 / inf where the row's component
    holds its whole group (wm_mreach_min_edge_grouped).  `group`: n integers in [0, n_groups) in any order; rows that
    are not in runs are sorted by (group, index) for the kernel and the indices mapped back."""
    import torch

    code = metric_code(metric)
    x = _prep(x)
    require_gpu(core, comp)
    n, d = x.shape
    _check_core_comp(core, comp, n)
    g = int(n_groups)
    order, gs = _sorted_groups(group, n, g, x.device)
    if order is not None:
        x, core, comp = x[order].contiguous(), core[order].contiguous(), comp[order].contiguous()
    lib = _lib.load()
    need = lib.wm_mreach_min_edge_grouped_workspace_bytes(n, d, g)
    ws = workspace(need, f"grouped_min_outgoing_edges: unsupported sizes n={n} d={d} n_groups={g}", x.device)
    w = torch.empty(n, dtype=torch.float32, device=x.device)
    j = torch.empty(n, dtype=torch.int32, device=x.device)
    check(lib.wm_mreach_min_edge_grouped(ptr(x), ptr(core), ptr(comp), ptr(gs), n, d, code, g, ptr(w), ptr(j), ptr(ws), need,
                                         stream_ptr()), "wm_mreach_min_edge_grouped")
    if order is None:
        return w, j
    w_out, j_out = torch.empty_like(w), torch.empty_like(j)
    w_out[order], j_out[order] = w, _through_order(order, j)
    return w_out, j_out


def group_min_mreach(xq, core_q, xe, core, group, n_groups: int, metric: str = "euclidean"):
    """`group_min_distances` with the mutual reachability max(core_q[i], core[j], dist_ij) in place of the distance:
    (weight float32 [m, n_groups], j int32 [m, n_groups]) on the device (wm_group_min_mreach), j the lowest index into xe
    that attains the weight, inf / -1 for a group without a row.  core_q float32 [m], core float32 [e]."""
    import torch

    code = metric_code(metric)
    xq, xe = _prep(xq), _prep(xe)
    require_gpu(core_q, core)
    (m, d), e, g = xq.shape, xe.shape[0], int(n_groups)
    if xe.shape[1] != d:
        raise ValueError(f"the rows have {d} features (padded), the grouped rows {xe.shape[1]}")
    _check_core_pair(core_q, m, core, e, "e")
    if m < 1 or e < 1:
        raise ValueError("group_min_mreach needs at least one row on either side")
    order, gs = _sorted_groups(group, e, g, xq.device)
    if order is not None:
        xe, core = xe[order].contiguous(), core[order].contiguous()
    w = torch.empty((m, g), dtype=torch.float32, device=xq.device)
    j = torch.empty((m, g), dtype=torch.int32, device=xq.device)
    lib = _lib.load()
    need = lib.wm_group_min_mreach_workspace_bytes(m, e, d, g)
    ws = workspace(need, f"group_min_mreach: unsupported sizes m={m} e={e} d={d} n_groups={g}", xq.device)
    check(lib.wm_group_min_mreach(ptr(xq), ptr(core_q), m, ptr(xe), ptr(core), ptr(gs), e, d, code, g, ptr(w), ptr(j), ptr(ws),
                                  need, stream_ptr()), "wm_group_min_mreach")
    if order is None:
        return w, j
    return w, _through_order(order, j)


def validity_from_parts(sizes, n_total: int, sparseness, sep) -> Tuple[float, np.ndarray]:
    """DBCV from its parts, in float64: `sizes` [C] the clusters' row counts, `n_total` the number of rows the labelling
    covers (noise included), `sparseness` [C] the largest internal edge of every cluster's tree, `sep` [C, C] the
    clusters' pairwise separations (the diagonal is ignored).  Returns (score, V [C]) with sep_c = the smallest entry
    of row c off the diagonal, V_c = (sep_c - sparseness_c) / max(sep_c, sparseness_c) (0 when both are 0) and
    score = sum_c sizes_c / n_total * V_c."""
    sizes = np.asarray(sizes, dtype=np.float64)
    sparse = np.asarray(sparseness, dtype=np.float64)
    sep = np.array(sep, dtype=np.float64)
    c = sizes.shape[0]
    if sizes.ndim != 1 or sparse.shape != (c,) or sep.shape != (c, c) or c < 2:
        raise ValueError("sizes [C], sparseness [C] and sep [C, C] with C >= 2 expected")
    if not n_total >= sizes.sum() or (sizes < 0).any():
        raise ValueError("n_total must cover the clusters, and no size may be negative")
    sep[np.arange(c), np.arange(c)] = np.inf
    nearest = sep.min(axis=1)
    if not (np.isfinite(sparse).all() and np.isfinite(nearest).all() and (sparse >= 0).all() and (nearest >= 0).all()):
        raise ValueError("sparseness and the separations must be finite and not negative")
    top = np.maximum(nearest, sparse)
    v = np.divide(nearest - sparse, top, out=np.zeros(c), where=top > 0.0)
    return float(np.cumsum(sizes / float(n_total) * v)[-1]), v  # (added in cluster order, one at a time)


def _internal_parts(u, v, w, group: np.ndarray, starts: np.ndarray):
    """From the spanning forest (one tree per group; rows sorted by group, `starts` [g + 1] the groups' first rows):
    (internal bool [n], sparseness float64 [g]).  Internal rows have degree > 1 in their tree, or are the group's first
    row where no row has (two rows or fewer); internal edges join two internal rows, or are all the group's edges where
    none does; the sparseness is the largest internal edge weight (0 for a group without an edge)."""
    n, g = group.shape[0], starts.shape[0] - 1
    degree = np.bincount(u, minlength=n) + np.bincount(v, minlength=n)
    internal = degree > 1
    none = np.bincount(group[internal], minlength=g) == 0
    internal[starts[:-1][none]] = True
    eg = group[u]
    inner = (degree[u] > 1) & (degree[v] > 1)
    use = inner | (np.bincount(eg[inner], minlength=g) == 0)[eg]
    sparse = np.zeros(g)
    np.maximum.at(sparse, eg[use], w[use])
    return internal, sparse


def _validity_parts(x, lab: np.ndarray, metric: str, d):
    """validity_index's device work: (sizes [C'], sparseness [C'], sep [C', C'], kept label values [C'], detail) over the
    C' clusters of at least two rows.  `detail` holds what a check needs to restate the score on the same trees: rows
    (the kept rows in (label, index) order), group, core (float64), u, v, w (the forest, indices into `rows`), internal
    and rounds."""
    import torch

    values, counts = np.unique(lab[lab >= 0], return_counts=True)
    values = values[counts >= 2]
    keep = np.flatnonzero(np.isin(lab, values))
    enc = np.searchsorted(values, lab[keep])
    order = np.argsort(enc, kind="stable")
    rows, group = keep[order], enc[order]
    g = int(values.size)
    sizes = np.bincount(group, minlength=g)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    xp = _prep(x)
    xs = xp[torch.from_numpy(rows).to(xp.device)].contiguous()
    core64 = allpoints_core_distances(xs, group, float(x.shape[1] if d is None else d), metric)
    core = core64.float().contiguous()  # rounded once: both mutual-reachability passes use these bits
    u, v, w, rounds = _boruvka(xs, core, metric, 1.0, torch.from_numpy(group.astype(np.int32)).to(xp.device), g)
    internal, sparse = _internal_parts(u, v, w, group, starts)
    at = np.flatnonzero(internal)
    at_d = torch.from_numpy(at).to(xp.device)
    xi, ci = xs[at_d].contiguous(), core[at_d].contiguous()
    wmin = group_min_mreach(xi, ci, xi, ci, torch.from_numpy(group[at]), g, metric)[0].cpu().numpy().astype(np.float64)
    sep = np.minimum.reduceat(wmin, np.searchsorted(group[at], np.arange(g)), axis=0)  # (every group has an internal row)
    detail = {"rows": rows, "group": group, "core": core64.cpu().numpy(), "u": u, "v": v, "w": w, "internal": internal,
              "rounds": rounds}
    return sizes, sparse, sep, values, detail


def validity_index(x, labels, metric: str = "euclidean", d: Optional[float] = None, per_cluster_scores: bool = False,
                   mst_raw_dist: bool = False, return_parts: bool = False):
    """DBCV, the density-based cluster validity of a labelling (`hdbscan.validity.validity_index`): a float in [-1, 1],
    larger is better; with `per_cluster_scores` also float64 [labels.max() + 1], every cluster's V_c.  x [n, D] device
    tensor, `labels` [n] integers with -1 for noise, `d` the power of the all-points core distance (default D).
    DESIGN.md ("DBCV") states the definition.  Noise rows take no part but count in n, so they lower the score.
    Deliberate differences from the package: a cluster of a single row scores 0 and takes no part in the other clusters'
    separations; fewer than two clusters of at least two rows raise ValueError (as `silhouette_samples` does);
    `mst_raw_dist` is not built; the power sums are taken in the log domain, so p = 50 .. 1024 neither overflows nor
    underflows (the package's float64 powers do).  With `return_parts` a dict of the intermediate arrays follows."""
    if mst_raw_dist:
        raise NotImplementedError("mst_raw_dist is not implemented: the trees are always built on the mutual reachability")
    metric_code(metric)
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)
    if x.ndim != 2 or lab.shape != (x.shape[0],) or lab.dtype.kind not in "iu":
        raise ValueError("x [n, D] and one integer label per row expected")
    if d is not None and not 0 < float(d) < math.inf:
        raise ValueError(f"d must be positive and finite (got {d})")
    usable = int((np.unique(lab[lab >= 0], return_counts=True)[1] >= 2).sum())
    if usable < 2:
        raise ValueError(f"validity_index needs at least two clusters of at least two rows (got {usable})")
    sizes, sparse, sep, kept, detail = _validity_parts(x, lab, metric, d)
    score, v = validity_from_parts(sizes, lab.shape[0], sparse, sep)
    out = (score,)
    if per_cluster_scores:
        per = np.zeros(int(lab.max()) + 1)
        per[kept] = v
        out += (per,)
    if return_parts:
        out += ({"sizes": sizes, "n_total": int(lab.shape[0]), "sparseness": sparse, "sep": sep, "clusters": kept, **detail},)
    return out[0] if len(out) == 1 else out


def relative_validity(mst, labels) -> float:
    """The `hdbscan` package's `relative_validity_`: a cheap stand-in for DBCV from the fitted spanning tree `mst`
    [n - 1, 3] (u, v, weight: `HDBSCAN.minimum_spanning_tree_`) and `labels` [n].  Host only, float64.  Over the edges:
    the largest weight inside cluster c is its sparseness DSC_c, the smallest weight between c and another cluster its
    separation DSPC_c; an edge with one noise end only lowers `min_outlier`, one with two is skipped.  A cluster that
    no edge joins to another one gets DSPC_c = 2 * (the largest weight of the tree, or with a single cluster
    `min_outlier`, itself the largest weight when no edge has a noise end).  V_c = (DSPC_c - DSC_c) / max(DSPC_c, DSC_c)
    (0 when both are 0) and the score is sum_c n_c V_c / n, n counting the noise rows.  No cluster: 0.0."""
    mst = np.asarray(mst, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = lab.shape[0]
    if lab.ndim != 1 or mst.shape != (max(n - 1, 0), 3):
        raise ValueError("mst [n - 1, 3] and labels [n] expected")
    n_clusters = int(lab.max()) + 1 if n else 0
    if n_clusters <= 0:
        return 0.0
    a, b, w = lab[mst[:, 0].astype(np.int64)], lab[mst[:, 1].astype(np.int64)], mst[:, 2]
    max_w = float(w.max()) if w.size else 0.0
    one_noise = (a < 0) != (b < 0)
    min_outlier = float(w[one_noise].min()) if one_noise.any() else max_w
    dsc, dspc = np.zeros(n_clusters), np.full(n_clusters, np.inf)
    both = (a >= 0) & (b >= 0)
    same, cross = both & (a == b), both & (a != b)
    np.maximum.at(dsc, a[same], w[same])
    np.minimum.at(dspc, a[cross], w[cross])
    np.minimum.at(dspc, b[cross], w[cross])
    dspc[np.isinf(dspc)] = 2.0 * (max_w if n_clusters > 1 else min_outlier)
    top = np.maximum(dspc, dsc)
    v = np.divide(dspc - dsc, top, out=np.zeros(n_clusters), where=top > 0.0)
    return float(np.cumsum(np.bincount(lab[lab >= 0], minlength=n_clusters) * v)[-1] / n)  # (added in cluster order)


# ------------------------------------------------------------------------------------------------ scores


def cluster_distance_sums(x, labels, n_clusters: int, metric: str = "euclidean"):
    """out[i, c] = sum of dist(i, j) over the rows j with labels[j] == c: float64 [n, n_clusters] on the device
    (wm_cluster_dist_sums).  labels: int32 device tensor in [-1, n_clusters)."""
    import torch

    code = metric_code(metric)
    x = _prep(x)
    require_gpu(labels)
    n, d = x.shape
    if labels.shape != (n,) or labels.dtype != torch.int32:
        raise ValueError("labels int32 [n] expected")
    out = torch.empty((n, n_clusters), dtype=torch.float64, device=x.device)
    check(_lib.load().wm_cluster_dist_sums(ptr(x), ptr(labels), n, d, code, int(n_clusters), ptr(out), stream_ptr()),
          "wm_cluster_dist_sums")
    return out


def silhouette_samples(x, labels, metric: str = "euclidean"):
    """sklearn.metrics.silhouette_samples of x [n, d] (device tensor) under `labels` (any integer array or tensor;
    every distinct value is a cluster, so drop noise rows first as the notebook does): float64 [n] on the device.
    The all-pairs part is the kernel (rows sorted by label so that each cluster is one run of columns); the
    per-sample arithmetic on the [n, n_clusters] sums is float64.  Singleton clusters score 0."""
    import torch

    metric_code(metric)
    x = _prep(x)
    n = x.shape[0]
    lab = torch.as_tensor(np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)).to(x.device)
    if lab.shape != (n,):
        raise ValueError("one label per row expected")
    _, enc = torch.unique(lab, return_inverse=True)
    c = int(enc.max()) + 1
    if not 2 <= c <= n - 1:
        raise ValueError(f"silhouette needs 2 <= n_clusters <= n_samples - 1 (got {c} clusters, {n} samples)")
    order = torch.argsort(enc, stable=True)
    enc_s = enc[order].to(torch.int32).contiguous()
    sums = cluster_distance_sums(x[order].contiguous(), enc_s, c, metric)
    counts = torch.bincount(enc_s.long(), minlength=c).double()
    own = enc_s.long().unsqueeze(1)
    intra = sums.gather(1, own).squeeze(1)
    a = intra / (counts[enc_s.long()] - 1.0)
    other = sums / counts.unsqueeze(0)
    other.scatter_(1, own, float("inf"))
    b = other.min(dim=1).values
    s = (b - a) / torch.maximum(a, b)
    s = torch.where(counts[enc_s.long()] == 1, torch.zeros_like(s), torch.nan_to_num(s))
    out = torch.empty_like(s)
    out[order] = s
    return out


def silhouette_score(x, labels, metric: str = "euclidean") -> float:
    return float(silhouette_samples(x, labels, metric).mean())


def _host64(x) -> np.ndarray:
    return (x.detach().cpu().double().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float64))


def _encode(labels) -> Tuple[np.ndarray, int]:
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)
    uniq, enc = np.unique(lab, return_inverse=True)
    return enc, uniq.size


def _cluster_means(x: np.ndarray, enc: np.ndarray, c: int):
    counts = np.bincount(enc, minlength=c).astype(np.float64)
    sums = np.zeros((c, x.shape[1]))
    np.add.at(sums, enc, x)
    return sums / counts[:, None], counts


def calinski_harabasz_score(x, labels) -> float:
    """sklearn.metrics.calinski_harabasz_score.  O(N D): float64 on the host from per-cluster sums (no kernel)."""
    x = _host64(x)
    enc, c = _encode(labels)
    n = x.shape[0]
    if not 2 <= c <= n - 1:
        raise ValueError("calinski_harabasz_score needs 2 <= n_clusters <= n_samples - 1")
    means, counts = _cluster_means(x, enc, c)
    extra = float((counts * ((means - x.mean(axis=0)) ** 2).sum(axis=1)).sum())
    intra = float(((x - means[enc]) ** 2).sum())
    return 1.0 if intra == 0.0 else extra * (n - c) / (intra * (c - 1.0))


def davies_bouldin_score(x, labels) -> float:
    """sklearn.metrics.davies_bouldin_score (Euclidean).  O(N D): float64 on the host from per-cluster sums."""
    x = _host64(x)
    enc, c = _encode(labels)
    if not 2 <= c <= x.shape[0] - 1:
        raise ValueError("davies_bouldin_score needs 2 <= n_clusters <= n_samples - 1")
    means, counts = _cluster_means(x, enc, c)
    spread = np.bincount(enc, weights=np.sqrt(((x - means[enc]) ** 2).sum(axis=1)), minlength=c) / counts
    sep = np.sqrt(((means[:, None, :] - means[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(spread, 0) or np.allclose(sep, 0):
        return 0.0
    sep[sep == 0] = np.inf
    ratio = (spread[:, None] + spread[None, :]) / sep
    return float(ratio.max(axis=1).mean())


def homogeneity_score(labels_true, labels_pred) -> float:
    """sklearn.metrics.homogeneity_score: 1 - H(C | K) / H(C), float64 on the host from the contingency table."""
    t, nt = _encode(labels_true)
    p, npred = _encode(labels_pred)
    if t.shape != p.shape:
        raise ValueError("labels_true and labels_pred differ in length")
    if t.size == 0:
        return 1.0
    table = np.zeros((nt, npred))
    np.add.at(table, (t, p), 1.0)
    n = float(t.size)
    pc = table.sum(axis=1) / n
    h_c = float(-(pc[pc > 0] * np.log(pc[pc > 0])).sum())
    if h_c == 0.0:
        return 1.0
    pk = table.sum(axis=0)
    nz = table > 0
    h_ck = float(-(table[nz] / n * np.log(table[nz] / np.broadcast_to(pk, table.shape)[nz])).sum())
    return 1.0 - h_ck / h_c


# ------------------------------------------------------------------------------------------------ KMeans


class KMeansStep(NamedTuple):
    """What `kmeans_step` returns.  With centres [k, d] the restart axis is dropped: labels / distances [n], centres
    [k, d], counts [k], and inertia / n_changed / shift2 are 0-d tensors."""
    labels: object      # int32 [n, R] on the device: the nearest centre of every restart, in [0, k)
    distances: object   # float32 [n, R] on the device: the distance to it
    centres: object     # float32 [R, k, d] on the device: the updated centres
    counts: object      # int32 [R, k] on the device
    inertia: object     # float64 [R] on the device
    n_changed: object   # int32 [R] on the device
    shift2: object      # float64 [R] on the device


def _kmeans_n_init(n_init, init) -> int:
    """sklearn's rule: n_init="auto" is 1 for k-means++ or an array of centres and 10 for "random"."""
    if isinstance(n_init, str):
        if n_init != "auto":
            raise ValueError(f"n_init must be 'auto' or a positive integer ({n_init!r} given)")
        return 10 if isinstance(init, str) and init == "random" else 1
    if int(n_init) < 1:
        raise ValueError(f"n_init must be 'auto' or a positive integer ({n_init!r} given)")
    return int(n_init)


def kmeans_stop(n_changed: int, shift2: float, tol_scaled: float) -> Optional[str]:
    """The stopping rule of one restart after one iteration (sklearn's `_kmeans_single_lloyd`): "labels" when no row
    changed its centre (strict convergence), otherwise "tol" when the squared centre shift is at most the scaled
    tolerance, otherwise None.  Pure host code."""
    if int(n_changed) == 0:
        return "labels"
    if float(shift2) <= float(tol_scaled):
        return "tol"
    return None


def kmeans_relocation_plan(counts, labels, distances):
    """This module's empty-cluster rule as pure numpy (no parity with sklearn's relocation is claimed): the empty
    clusters (counts == 0) in ascending id take, one each, the rows farthest from their assigned centres, in the order
    (distance descending, index ascending).  A taken row leaves its old cluster's sum and count, so a row whose cluster
    would be left without a member is passed over.  Returns (clusters int64 [e], rows int64 [e]): cluster clusters[q]
    takes row rows[q]; fewer pairs than empty clusters when the rows run out."""
    counts = np.asarray(counts, dtype=np.int64).copy()
    labels = np.asarray(labels, dtype=np.int64)
    distances = np.asarray(distances, dtype=np.float64)
    if labels.ndim != 1 or distances.shape != labels.shape or counts.ndim != 1:
        raise ValueError("counts [k], labels [n] and distances [n] expected")
    empty = np.flatnonzero(counts == 0)
    order = np.lexsort((np.arange(labels.size), -distances))
    clusters, rows, at = [], [], 0
    for c in empty:
        while at < order.size and counts[labels[order[at]]] <= 1:
            at += 1
        if at == order.size:
            break
        i = int(order[at])
        at += 1
        counts[labels[i]] -= 1
        clusters.append(int(c))
        rows.append(i)
    return np.asarray(clusters, dtype=np.int64), np.asarray(rows, dtype=np.int64)


def kmeans_relocate(x, labels, centres_old, centres_new, counts, clusters, rows):
    """Apply a `kmeans_relocation_plan` to one restart's update on the host: (centres float32 [k, d], counts int64 [k],
    shift2 float).  Cluster clusters[q] becomes row rows[q] with count 1; every cluster that gave a row is recomputed
    from its remaining members as the exactly rounded float64 sum (math.fsum) divided by the count and rounded to
    float32 once; shift2 is math.fsum of the squared moves against centres_old.  x: the prepared device matrix; the
    other arguments numpy."""
    import torch

    labels = np.asarray(labels, dtype=np.int64)
    centres = np.array(centres_new, dtype=np.float32)
    counts = np.asarray(counts, dtype=np.int64).copy()
    taken = np.zeros(labels.size, dtype=bool)
    taken[rows] = True
    take = x[torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(x.device)].cpu().numpy()
    for q, c in enumerate(clusters):
        centres[c] = take[q]
        counts[c] = 1
    for donor in np.unique(labels[rows]):
        keep = np.flatnonzero((labels == donor) & ~taken)
        member = x[torch.from_numpy(keep).to(x.device)].cpu().numpy().astype(np.float64)
        centres[donor] = np.array([math.fsum(col) for col in member.T]) / float(keep.size)
        counts[donor] = keep.size
    move = centres.astype(np.float64) - np.asarray(centres_old, dtype=np.float64)
    return centres, counts, math.fsum((move * move).ravel().tolist())


def _kmeans_update(x, cols, dist, prev_cols, centres):
    """wm_kmeans_update on prepared operands: cols / dist [n, R] as wm_group_min_dist wrote them for centres [R, k, d];
    (centres_new, counts, inertia, n_changed, shift2) on the device."""
    import torch

    (n, d), (r, k, _) = x.shape, centres.shape
    lib = _lib.load()
    need = lib.wm_kmeans_update_workspace_bytes(n, d, k, r)
    ws = workspace(need, f"kmeans update: unsupported sizes n={n} d={d} n_clusters={k} restarts={r}", x.device)
    new = torch.empty_like(centres)
    counts = torch.empty((r, k), dtype=torch.int32, device=x.device)
    inertia = torch.empty(r, dtype=torch.float64, device=x.device)
    changed = torch.empty(r, dtype=torch.int32, device=x.device)
    shift2 = torch.empty(r, dtype=torch.float64, device=x.device)
    check(lib.wm_kmeans_update(ptr(x), n, d, ptr(cols), ptr(dist), ptr(prev_cols), r, k, ptr(centres), ptr(new), ptr(counts),
                               ptr(inertia), ptr(changed), ptr(shift2), ptr(ws), need, stream_ptr()), "wm_kmeans_update")
    return new, counts, inertia, changed, shift2


def _kmeans_assign(x, centres):
    """One assignment pass for all restarts: (cols int32 [n, R] = r * k + label, dist float32 [n, R]).  wm_group_min_dist
    itself, what `group_min_distances` calls: the centres [R, k, d] are in runs of equal group ids already and every group
    has columns, so that function's sort, its gather, its fills and its index mapping would each be the identity."""
    import torch

    (n, d), (r, k, _) = x.shape, centres.shape
    group = torch.arange(r, dtype=torch.int32, device=x.device).repeat_interleave(k).contiguous()
    lib = _lib.load()
    need = lib.wm_group_min_dist_workspace_bytes(n, r * k, d, r)
    ws = workspace(need, f"kmeans assignment: unsupported sizes n={n} d={d} n_clusters={k} restarts={r}", x.device)
    dist = torch.empty((n, r), dtype=torch.float32, device=x.device)
    cols = torch.empty((n, r), dtype=torch.int32, device=x.device)
    check(lib.wm_group_min_dist(ptr(x), n, ptr(centres), ptr(group), r * k, d, 0, r, ptr(dist), ptr(cols), ptr(ws), need,
                                stream_ptr()), "wm_group_min_dist")
    return cols, dist


def _kmeans_centres(x, centres):
    """Prepared float32 centres [R, k, d_padded] on x's device and whether the restart axis was given."""
    import torch

    require_gpu(centres)
    if centres.dim() not in (2, 3):
        raise ValueError("centres [k, d] or [R, k, d] expected")
    many = centres.dim() == 3
    c = centres.float() if many else centres.float().unsqueeze(0)
    if c.shape[2] % 4:
        c = torch.nn.functional.pad(c, (0, 4 - c.shape[2] % 4))
    if c.shape[2] != x.shape[1]:
        raise ValueError(f"the centres have {centres.shape[-1]} features, the rows {x.shape[1]} (after padding)")
    if c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError("at least one restart and one centre expected")
    return c.contiguous(), many


def kmeans_step(x, centres, prev=None) -> KMeansStep:
    """One Lloyd iteration on device tensors: the assignment pass (`group_min_distances`, every restart a group of
    columns: one pass over x [n, d] serves all R restarts) and the update (wm_kmeans_update).  centres [k, d] or
    [R, k, d]; prev: the labels of an earlier step (int32, the shape of the labels returned here) or None, in which
    case n_changed = n.  A cluster without a member keeps its centre and has count 0 (`KMeans.fit` then applies
    `kmeans_relocation_plan`; this function does not).  Returns a `KMeansStep`."""
    import torch

    x = _prep(x)
    c, many = _kmeans_centres(x, centres)
    r, k, _ = c.shape
    offs = (torch.arange(r, dtype=torch.int32, device=x.device) * k).unsqueeze(0)
    prev_cols = None
    if prev is not None:
        require_gpu(prev)
        p = prev if many else prev.unsqueeze(1)
        if p.shape != (x.shape[0], r) or p.dtype != torch.int32:
            raise ValueError("prev: the int32 labels of an earlier step expected")
        prev_cols = (p + offs).contiguous()
    cols, dist = _kmeans_assign(x, c)
    new, counts, inertia, changed, shift2 = _kmeans_update(x, cols, dist, prev_cols, c)
    labels = cols - offs
    new = new[:, :, :centres.shape[-1]].contiguous()
    if many:
        return KMeansStep(labels, dist, new, counts, inertia, changed, shift2)
    return KMeansStep(labels[:, 0].contiguous(), dist[:, 0].contiguous(), new[0], counts[0], inertia[0], changed[0], shift2[0])


def kmeans_plusplus(x, n_clusters: int, *, random_state=None, uniforms=None, n_local_trials: Optional[int] = None,
                    return_details: bool = False):
    """Greedy k-means++ seeding on the device (wm_kmeans_seed): (centres float32 [k, d] on the device, indices int64
    [k], numpy), the chosen rows of x [n, d] and their row numbers.

    The rule is sklearn.cluster.kmeans_plusplus's: the first centre uniformly, every later one the best of
    `n_local_trials` (default 2 + int(ln k)) rows drawn with probability proportional to the squared distance to the
    nearest centre chosen so far, the best being the one that lowers the potential most.  This is sklearn's
    DISTRIBUTION and not sklearn's random stream: the draws come from a table of uniforms u float64 [k, T] in [0, 1),
    `numpy.random.default_rng(random_state).random((k, T))` unless `uniforms` gives it, and the same seed picks other
    rows than sklearn does.  Centre 0 is row min(floor(u[0, 0] * n), n - 1); trial t of centre c is the first row whose
    running sum of the squared distances exceeds u[c, t] * potential (strictly, so a row at distance 0 is never drawn);
    include/wafer_hip.h states the rest.  With `return_details` a dict follows: candidates int64 [k, T] (-1 unused) and
    potentials float64 [k, T] (inf unused) of every step, and the uniforms."""
    import torch

    x = _prep(x)
    n, d = x.shape
    k = int(n_clusters)
    if not 1 <= k <= n:
        raise ValueError(f"n_clusters ({k}) must be in [1, n_samples = {n}]")
    t = 2 + int(math.log(k)) if n_local_trials is None else int(n_local_trials)
    if uniforms is None:
        u = np.random.default_rng(random_state).random((k, t))
    else:
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.shape != (k, t) or not ((u >= 0) & (u < 1)).all():
            raise ValueError(f"uniforms: float64 [{k}, {t}] in [0, 1) expected")
    lib = _lib.load()
    need = lib.wm_kmeans_seed_workspace_bytes(n, d, k, t)
    ws = workspace(need, f"kmeans_plusplus: unsupported sizes n={n} d={d} n_clusters={k} n_local_trials={t} (1 .. 16 trials)",
                   x.device)
    u_d = torch.from_numpy(u).to(x.device)
    centres = torch.empty((k, d), dtype=torch.float32, device=x.device)
    idx = torch.empty(k, dtype=torch.int32, device=x.device)
    cand = torch.empty((k, t), dtype=torch.int32, device=x.device) if return_details else None
    pots = torch.empty((k, t), dtype=torch.float64, device=x.device) if return_details else None
    check(lib.wm_kmeans_seed(ptr(x), n, d, k, t, ptr(u_d), ptr(centres), ptr(idx), ptr(cand), ptr(pots), ptr(ws), need,
                             stream_ptr()), "wm_kmeans_seed")
    out = (centres, idx.cpu().numpy().astype(np.int64))
    if return_details:
        return out + ({"candidates": cand.cpu().numpy().astype(np.int64), "potentials": pots.cpu().numpy(), "uniforms": u},)
    return out


class KMeans:
    """sklearn.cluster.KMeans (Lloyd) on device tensors.  `fit(x)` sets `cluster_centers_` (float32 [k, d] on the
    device), `labels_` (numpy int64 [n]), `inertia_`, `n_iter_`, `n_features_in_`, and per restart `inertias_` and
    `n_iters_` (numpy [R]).

    `init`: "k-means++" (`kmeans_plusplus`, one table of uniforms per restart from one generator), "random" (k distinct
    rows from a host permutation per restart), an array or tensor [k, d], or (an extension) [R, k, d] for R explicit
    restarts.  `n_init="auto"` is 1 for k-means++ or an array and 10 for "random", as sklearn; with an array the number
    of restarts is the array's.  All restarts advance together, one assignment pass per iteration over all of them
    (`kmeans_step`); a restart that has stopped leaves the pass.  No sum depends on the number of restarts, so each
    restart's result is bit-equal to that restart run alone.  The kept restart is the one of the lowest inertia, the
    lowest index among equals.

    Stopping rule (sklearn's, `kmeans_stop`): `tol` is scaled by the mean per-feature variance of x.  After the update of
    iteration i a restart stops when no row changed its centre against iteration i - 1 (the centres of the update are
    then the ones the labels were assigned to), or when the squared centre shift is at most the scaled tolerance, or at
    max_iter.  After a stop on the tolerance or on max_iter one more assignment pass runs, so that `labels_` and
    `inertia_` belong to `cluster_centers_`.  `n_iter_` is the number of updates, as sklearn counts.

    Empty clusters follow this module's own rule (`kmeans_relocation_plan`, a host detour on the iteration that has a
    zero count; no parity with sklearn's relocation is claimed); a restart never stops on the iteration that relocated.
    `sample_weight` and algorithm="elkan" are not implemented."""

    def __init__(self, n_clusters: int = 8, *, init="k-means++", n_init="auto", max_iter: int = 300, tol: float = 1e-4,
                 random_state=None, algorithm: str = "lloyd"):
        if algorithm == "elkan":
            raise NotImplementedError("algorithm='elkan' is not implemented (available: lloyd)")
        if algorithm != "lloyd":
            raise ValueError(f"unknown algorithm {algorithm!r} (available: lloyd)")
        if int(n_clusters) < 1:
            raise ValueError("n_clusters must be at least 1")
        if isinstance(init, str) and init not in ("k-means++", "random"):
            raise ValueError(f"init must be 'k-means++', 'random' or an array of centres ({init!r} given)")
        if int(max_iter) < 1 or float(tol) < 0:
            raise ValueError("max_iter >= 1 and tol >= 0 required")
        self.n_clusters, self.init, self.n_init = int(n_clusters), init, n_init
        self._n_init = _kmeans_n_init(n_init, init)
        self.max_iter, self.tol, self.random_state, self.algorithm = int(max_iter), float(tol), random_state, algorithm
        self.cluster_centers_ = self.labels_ = self.inertia_ = self.n_iter_ = self.n_features_in_ = None
        self.inertias_ = self.n_iters_ = None

    @staticmethod
    def _refuse_weights(sample_weight):
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not implemented")

    def _initial(self, xp):
        """float32 [R, k, d_padded] on the device."""
        import torch

        n, k = xp.shape[0], self.n_clusters
        if not isinstance(self.init, str):
            init = self.init if hasattr(self.init, "is_cuda") else torch.as_tensor(np.asarray(self.init, dtype=np.float32)).to(xp.device)
            c, _ = _kmeans_centres(xp, init.contiguous())
            if c.shape[1] != k:
                raise ValueError(f"init holds {c.shape[1]} centres, n_clusters is {k}")
            return c
        rng = np.random.default_rng(self.random_state)
        out = []
        for _ in range(self._n_init):
            if self.init == "random":
                rows = np.sort(rng.permutation(n)[:k])
                out.append(xp[torch.from_numpy(rows).to(xp.device)])
            else:
                t = 2 + int(math.log(k))
                out.append(kmeans_plusplus(xp, k, uniforms=rng.random((k, t)))[0])
        return torch.stack(out).contiguous()

    def fit(self, x, y=None, sample_weight=None) -> "KMeans":
        import torch

        self._refuse_weights(sample_weight)
        xp = _prep(x)
        n, k = xp.shape[0], self.n_clusters
        if k > n:
            raise ValueError(f"n_clusters ({k}) must be at most the number of samples ({n})")
        cur = self._initial(xp)  # the centres of the restarts that still run, [len(active), k, d]; never written in place
        r = cur.shape[0]
        centres = torch.empty_like(cur)  # every restart's final centres
        tol_scaled = float(xp[:, :x.shape[1]].double().var(dim=0, unbiased=False).mean()) * self.tol  # (no padding columns)
        active = list(range(r))
        prev = None  # cols [n, len(active)] of the iteration before
        labels = np.zeros((r, n), dtype=np.int64)
        inertias, n_iters = np.zeros(r), np.zeros(r, dtype=np.int64)
        again = []  # restarts that need the closing assignment pass
        for it in range(1, self.max_iter + 1):
            cols, dist = _kmeans_assign(xp, cur)
            new, counts, inertia, changed, shift2 = _kmeans_update(xp, cols, dist, prev, cur)
            # one synchronisation per iteration: what the stopping rule reads, and whether a cluster is empty
            inertia_h, shift_h, changed_h, empty_h = torch.stack(
                [inertia, shift2, changed.double(), (counts == 0).any(dim=1).double()]).cpu().numpy()
            relocated = set()
            for a in np.flatnonzero(empty_h):
                lab, counts_a = (cols[:, a] - a * k).cpu().numpy(), counts[a].cpu().numpy()
                clusters, rows = kmeans_relocation_plan(counts_a, lab, dist[:, a].cpu().numpy())
                if rows.size:
                    c_new, _, shift_h[a] = kmeans_relocate(xp, lab, cur[a].cpu().numpy(), new[a].cpu().numpy(), counts_a, clusters,
                                                           rows)
                    new[a] = torch.from_numpy(c_new).to(xp.device)
                    relocated.add(int(a))
            keep = []
            for a, rr in enumerate(active):
                why = None if a in relocated else kmeans_stop(changed_h[a], shift_h[a], tol_scaled)
                if why is None and it < self.max_iter:
                    keep.append(a)
                    continue
                n_iters[rr] = it
                centres[rr] = new[a]
                if why == "labels":
                    labels[rr] = (cols[:, a] - a * k).cpu().numpy()
                    inertias[rr] = inertia_h[a]
                else:
                    again.append(rr)
            if not keep:
                break
            if len(keep) == len(active):
                cur, prev = new, cols
                continue
            k_idx = torch.tensor(keep, device=xp.device)
            offs = (torch.arange(len(keep), dtype=torch.int32, device=xp.device) - k_idx.to(torch.int32)) * k
            cur = new[k_idx].contiguous()
            prev = (cols[:, k_idx] + offs.unsqueeze(0)).contiguous()  # (the columns renumbered for the restarts that go on)
            active = [active[a] for a in keep]
        if again:
            sel = torch.tensor(again, device=xp.device)
            last = centres[sel].contiguous()
            cols, dist = _kmeans_assign(xp, last)
            _, _, inertia, _, _ = _kmeans_update(xp, cols, dist, None, last)
            offs = (torch.arange(len(again), dtype=torch.int32, device=xp.device) * k).unsqueeze(0)
            labels[again] = (cols - offs).cpu().numpy().T
            inertias[again] = inertia.cpu().numpy()
        best = int(np.argmin(inertias))
        d_in = int(x.shape[1])
        self._centres_padded = centres[best].contiguous()
        self.cluster_centers_ = centres[best, :, :d_in].contiguous()
        self.labels_, self.inertia_, self.n_iter_ = labels[best], float(inertias[best]), int(n_iters[best])
        self.inertias_, self.n_iters_, self.n_features_in_ = inertias, n_iters, d_in
        return self

    def _check_fitted(self, x):
        if self.cluster_centers_ is None:
            raise RuntimeError("KMeans used before fit")
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"rows have {x.shape[-1]} features, the model was fitted on {self.n_features_in_}")

    def fit_predict(self, x, y=None, sample_weight=None) -> np.ndarray:
        return self.fit(x, sample_weight=sample_weight).labels_

    def predict(self, x) -> np.ndarray:
        """The nearest centre of every row: numpy int64 [m]; `manifold.knn_query(x, cluster_centers_, 1)`'s choice."""
        self._check_fitted(x)
        cols, _ = _kmeans_assign(_prep(x), self._centres_padded.unsqueeze(0))
        return cols[:, 0].cpu().numpy().astype(np.int64)

    def transform(self, x):
        """The distance of every row to every centre: float32 [m, k] on the device (every centre a group of its own)."""
        import torch

        self._check_fitted(x)
        k = self.n_clusters
        return group_min_distances(_prep(x), self._centres_padded, torch.arange(k, dtype=torch.int32), k)[0]

    def fit_transform(self, x, y=None, sample_weight=None):
        return self.fit(x, sample_weight=sample_weight).transform(x)

    def score(self, x, y=None, sample_weight=None) -> float:
        """Minus the inertia of x under the fitted centres (the double sum of the squared float32 distances)."""
        self._refuse_weights(sample_weight)
        self._check_fitted(x)
        xp = _prep(x)
        c = self._centres_padded.unsqueeze(0)
        cols, dist = _kmeans_assign(xp, c)
        return -float(_kmeans_update(xp, cols, dist, None, c)[2][0])


class SpectralClustering:
    """sklearn.cluster.SpectralClustering on device tensors with a nearest-neighbour affinity and
    assign_labels="kmeans": the rows of the first `n_clusters` columns of the spectral embedding of the affinity graph
    (`manifold.spectral_embedding`, the first column kept) are clustered by `KMeans` (k-means++, `n_init` restarts).
    affinity: "connectivity" (sklearn's nearest_neighbors, 0.5 (A + A^T) of the 0/1 kNN graph, self included) or
    "fuzzy" (UMAP's fuzzy simplicial set); the kNN graph is exact.  `fit(x)` sets `labels_` (numpy int64 [n]),
    `affinity_matrix_` (manifold.CSR), `embedding_` (float32 [n, n_clusters] on the device) and `converged_`."""

    def __init__(self, n_clusters: int = 8, *, n_neighbors: int = 10, affinity: str = "connectivity", metric: str = "euclidean",
                 n_init: int = 10, random_state=0, tol: float = 1e-6):
        metric_code(metric)
        if affinity not in ("connectivity", "fuzzy"):
            raise ValueError(f"affinity must be 'connectivity' or 'fuzzy' ({affinity!r} given)")
        if int(n_clusters) < 1 or int(n_neighbors) < 1 or int(n_init) < 1:
            raise ValueError("n_clusters, n_neighbors and n_init must be at least 1")
        self.n_clusters, self.n_neighbors, self.affinity, self.metric = int(n_clusters), int(n_neighbors), affinity, metric
        self.n_init, self.random_state, self.tol = int(n_init), random_state, float(tol)
        self.labels_ = self.affinity_matrix_ = self.embedding_ = self.converged_ = None

    def fit(self, x, y=None) -> "SpectralClustering":
        from . import manifold

        graph = manifold.affinity_graph(x, min(self.n_neighbors, x.shape[0]), self.metric, self.affinity)
        emb, _, _, self.converged_ = manifold.spectral_embedding(graph, self.n_clusters, self.tol, drop_first=False)
        self.affinity_matrix_ = graph
        self.embedding_ = emb.float().contiguous()
        self.labels_ = KMeans(self.n_clusters, n_init=self.n_init, random_state=self.random_state).fit(self.embedding_).labels_
        return self

    def fit_predict(self, x, y=None) -> np.ndarray:
        return self.fit(x).labels_
