"""GPU checks of the sliced schedule of csrc/cluster.hip at the sizes where a column slice holds more than one tile: the
k-list and the register-resident best carried from tile to tile, the prefetch of the next tile behind an epilogue, a
short last slice, the merge kernels behind multi-tile slices, the block-diagonal cut with per > 1 and slices that
receive no tile.  Shapes, references, families and checkers are tests/cluster_cases.py's; tests/test_cluster_cases_cpu.py
proves there, without a GPU, that every shape has the schedule it is here for and that the checkers reject each seeded
error of a restatement of the schedule.

The one tolerance is eps(d) = (d + 3) 2^-24 (csrc/cluster.hip; test_gpu_cluster.py), plus test_gpu_dbcv.py's DOUBLE for
the all-points core distance; on the integer lattice results are equal.  d = 4 is one staged chunk with 28 zero-filled
features, d = 52 two chunks, the second partial, so that the prefetch across tiles runs with nchunks > 1; width itself is
covered at small n.  Both metrics run at d = 4; at d = 52 the float64 reference of a shape costs more than a second, so
Euclidean runs alone there.  The lattice is four-dimensional: d = 4 only."""
import math

import numpy as np
import pytest
import torch
from parity_log import parity

import cluster_cases as cc
from cluster_cases import KS, SHAPES, case, eps, plan
from guarded import Guarded, finish, stream
from test_cluster_cpu import prim_mst
from test_gpu_cluster import check_tree

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["singletons", "halves", "single", "blocks"]
# (family, d, metric): both metrics at d = 4, Euclidean alone at d = 52 (the module's note)
FAMILIES = [("rows", 4, "euclidean"), ("rows", 4, "manhattan"), ("rows", 52, "euclidean"), ("lattice", 4, "euclidean"),
            ("lattice", 4, "manhattan")]
SQUARES = [("sq3000",) + f for f in FAMILIES] + [("sq4200",) + f for f in FAMILIES if f[1] == 4]  # n = 4200: d = 4 only


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(*t):
    out = tuple(a.cpu().numpy() for a in t)
    return out if len(out) > 1 else out[0]


def alphas_of(family):
    return (1.0, 2.0) if family == "lattice" else (1.0,)  # (a power of two scales exactly)


def same_bits(a, b):
    return all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))


_DEVICE = {}


def on_device(c):
    """The operands of a case on the device, once per operand set."""
    key = id(c["x"])
    if key not in _DEVICE:
        _DEVICE.clear()
        _DEVICE[key] = (c["x"], dev(c["x"]), dev(c["xr"]) if c["xr"] is not c["x"] else None)
    return _DEVICE[key][1:]


# ------------------------------------------------------------------------------------------------ square: lists


@pytest.mark.parametrize("shape,family,d,metric", SQUARES)
def test_core_distance_and_knn_graph_over_multi_tile_slices(shape, family, d, metric):
    from ssl_wafermap_amd import cluster, manifold

    n = SHAPES[shape]["n"]
    for k in KS:
        c = case(shape, "core", family, d, metric, k=k)
        xd, _ = on_device(c)
        got = host(cluster.core_distances(xd, k, metric))
        c["check"](got, parity)
        assert same_bits([got], [host(cluster.core_distances(xd, k, metric))])
        c = case(shape, "knn", family, d, metric, k=k)
        dist, idx = host(*manifold.knn_graph(xd, k, metric))
        c["check"]((dist, idx.astype(np.int64)), parity)
        assert same_bits((dist, idx), host(*manifold.knn_graph(xd, k, metric)))
        assert np.array_equal(dist[:, k - 1], got), "the core distance is the kNN graph's last column"
        # the first column is the row itself, or an equal earlier row
        first = idx[:, 0]
        assert (first <= np.arange(n)).all() and (dist[:, 0] == 0).all() and np.array_equal(c["x"][first], c["x"])


@pytest.mark.parametrize("family,d,metric", FAMILIES)
def test_knn_query_of_the_fitted_rows_is_the_graph_at_3000(family, d, metric):
    from ssl_wafermap_amd import manifold

    x, _, _ = cc.operands("sq3000", family, d)
    xd = dev(x)
    for k in (1, 17, 64):
        assert same_bits(host(*manifold.knn_query(xd, xd, k, metric)), host(*manifold.knn_graph(xd, k, metric))), (metric, k)


# ------------------------------------------------------------------------------------------------ square: min edge


@pytest.mark.parametrize("shape,family,d,metric", SQUARES)
def test_min_edge_over_multi_tile_slices(shape, family, d, metric):
    from ssl_wafermap_amd import cluster

    for kind in KINDS:
        for alpha in alphas_of(family):
            c = case(shape, "minedge", family, d, metric, kind=kind, alpha=alpha)
            xd, _ = on_device(c)
            args = (xd, dev(c["kw"]["core"]), dev(c["kw"]["comp"]), metric)
            got = host(*cluster.min_outgoing_edges(*args, alpha=alpha))
            # (on the lattice: the weight's bits and the lowest j over the whole row, across tiles and slices)
            c["check"]((got[0], got[1].astype(np.int64)), parity)
            assert same_bits(got, host(*cluster.min_outgoing_edges(*args, alpha=alpha)))
            if kind == "single":
                assert (got[1] == -1).all()


@pytest.mark.parametrize("metric", cc.METRICS)
def test_spanning_tree_at_3000_against_float64_prim(metric):
    from ssl_wafermap_amd import cluster

    n, d, k = 3000, 52, 5
    x = cc.rows(n, d, 7 + n)
    xd = dev(x)
    u, v, w, rounds = cluster.mutual_reachability_mst(xd, k, metric, return_rounds=True)
    check_tree(u, v, w, n)
    assert 1 <= rounds <= math.ceil(math.log2(n))
    _, _, w_ref = prim_mst(x, k, metric)
    parity(f"mst total weight {metric} n={n} abs", abs(w.sum() - w_ref.sum()), n * eps(d) * w_ref.max())
    u2, v2, w2 = cluster.mutual_reachability_mst(xd, k, metric)
    assert np.array_equal(u, u2) and np.array_equal(v, v2) and np.array_equal(w.view(np.int64), w2.view(np.int64))


# ------------------------------------------------------------------------------------------------ queries


def run_query(c, metric, alpha):
    from ssl_wafermap_amd import cluster

    xd, xqd = on_device(c)
    args = (xqd, dev(c["kw"]["core_q"]), xd, dev(c["kw"]["core"]), metric)
    got = host(*cluster.mreach_query(*args, alpha=alpha))
    assert same_bits(got, host(*cluster.mreach_query(*args, alpha=alpha)))
    return got[0], got[1], got[2].astype(np.int64)


@pytest.mark.parametrize("family,d,metric", FAMILIES)
def test_queries_over_multi_tile_slices(family, d, metric):
    """4200 x 2600: 21 slices of two tiles, the last of one.  The fitted rows' core distances are the float64
    reference's, rounded to float32."""
    from ssl_wafermap_amd import manifold

    shape = "q4200x2600"
    for k in KS:
        c = case(shape, "knn", family, d, metric, k=k)
        xd, xqd = on_device(c)
        got = host(*manifold.knn_query(xqd, xd, k, metric))
        c["check"]((got[0], got[1].astype(np.int64)), parity)
        assert same_bits(got, host(*manifold.knn_query(xqd, xd, k, metric)))
    for alpha in alphas_of(family):
        c = case(shape, "mreachq", family, d, metric, alpha=alpha)
        c["check"](run_query(c, metric, alpha), parity)  # (on the lattice: the (w, dist, j) order exactly)


@pytest.mark.parametrize("family", ["rows", "lattice"])
def test_queries_of_1024_row_tiles_through_one_slice_of_four_tiles(family):
    """130 945 x 200 at d = 4: slices == 1 but not `direct`, so the one slice goes through the merge; the last row tile
    holds one row.  Euclidean alone and the two ends of the k list: the reference's sort and the index check of
    130 945 x 64 entries are what this case costs, not the kernels."""
    from ssl_wafermap_amd import manifold

    shape, metric = "q130945x200", "euclidean"
    for k in (2, 64):
        c = case(shape, "knn", family, 4, metric, k=k)
        xd, xqd = on_device(c)
        got = host(*manifold.knn_query(xqd, xd, k, metric))
        c["check"]((got[0], got[1].astype(np.int64)), parity)
        assert same_bits(got, host(*manifold.knn_query(xqd, xd, k, metric)))
    for alpha in alphas_of(family):
        c = case(shape, "mreachq", family, 4, metric, alpha=alpha)
        c["check"](run_query(c, metric, alpha), parity)


# ------------------------------------------------------------------------------------------------ block-diagonal


@pytest.mark.parametrize("family,d,metric", FAMILIES)
def test_allpoints_core_with_two_tiles_per_slice_and_empty_slices(family, d, metric):
    """n = 2600 sorted by group (2200, 300, 63, 36, 1 rows), 64-row tiles, 21 slices: per == 2 for the large group, slices
    without a tile for every row tile, a row tile that spans three groups."""
    from ssl_wafermap_amd import cluster

    c = case("ap2600", "apcore", family, d, metric)
    xd, _ = on_device(c)
    got = cluster.allpoints_core_distances(xd, c["group"], d=c["kw"]["p"], metric=metric)
    assert got.dtype == torch.float64
    got = host(got)
    c["check"](got, parity)
    assert got[-1] == 0  # the group of one row
    assert same_bits([got], [host(cluster.allpoints_core_distances(xd, c["group"], d=c["kw"]["p"], metric=metric))])


@pytest.mark.parametrize("family,d,metric", FAMILIES)
def test_grouped_min_edge_with_two_tiles_per_slice_and_empty_slices(family, d, metric):
    from ssl_wafermap_amd import cluster

    for kind in KINDS:
        c = case("g3000", "minedge_g", family, d, metric, kind=kind)
        xd, _ = on_device(c)
        args = (xd, dev(c["kw"]["core"]), dev(c["kw"]["comp"]), torch.from_numpy(c["group"]), 5, metric)
        got = host(*cluster.grouped_min_outgoing_edges(*args))
        c["check"]((got[0], got[1].astype(np.int64)), parity)
        assert same_bits(got, host(*cluster.grouped_min_outgoing_edges(*args)))
        assert got[1][-1] == -1  # the group of one row has no edge


@pytest.mark.parametrize("metric", cc.METRICS)
def test_grouped_boruvka_at_3000_against_per_group_prim(metric):
    """The forest of the groups of 2600, 300, 63 and 36 rows (the single row has no edge) against prim_mst on each group's
    rows alone; the core distances are each group's own float64 5th-smallest, rounded to float32 (half an ulp, inside
    eps)."""
    from ssl_wafermap_amd import cluster

    n, d, k = 3000, 52, 5
    x = cc.rows(n, d, 11 + n)
    group = cc.grouped_labels(n)
    spans = [(a, b) for a, b in cc.group_bounds(group, 5)]
    trees = [prim_mst(x[a:b], k, metric) if b - a >= k else None for a, b in spans]
    core = np.zeros(n, dtype=np.float32)
    for a, b in spans:
        if b - a >= k:
            core[a:b] = np.sort(cc.dist64(x[a:b], x[a:b], metric), axis=1)[:, k - 1].astype(np.float32)
    xd = dev(x)
    u, v, w, rounds = cluster._boruvka(xd, dev(core), metric, 1.0, dev(group), 5)
    assert u.shape == (n - 5,) and (group[u] == group[v]).all()
    assert rounds <= math.ceil(math.log2(n - 400))
    for (a, b), tree in zip(spans, trees):
        e = group[u] == group[a]
        if tree is None:
            assert not e.any()
            continue
        check_tree(u[e] - a, v[e] - a, w[e], b - a)
        parity(f"grouped mst weight {metric} n={n} group at {a} abs", abs(w[e].sum() - tree[2].sum()), (b - a) * eps(d) * tree[2].max())
    again = cluster._boruvka(xd, dev(core), metric, 1.0, dev(group), 5)
    assert np.array_equal(u, again[0]) and np.array_equal(v, again[1]) and np.array_equal(w.view(np.int64), again[2].view(np.int64))


# ------------------------------------------------------------------------------------------------ the production row count


@pytest.mark.parametrize("metric", cc.METRICS)
def test_core_distance_and_knn_graph_at_12449_rows(metric):
    """11 slices of 18 tiles, the last of 15.  The reference covers about 512 sampled rows: rows are independent, and
    each crosses every slice."""
    from ssl_wafermap_amd import cluster, manifold

    k = 16
    c = case("prod12449", "knn", "rows", 4, metric, k=k)
    sel = c["rows"]
    assert {0, 127, 128, 12416, 12448} <= set(sel.tolist()) and 500 <= sel.size <= 512
    xd = dev(c["x"])
    dist, idx = host(*manifold.knn_graph(xd, k, metric))
    c["check"]((dist[sel], idx[sel].astype(np.int64)), parity)
    core = host(cluster.core_distances(xd, k, metric))
    case("prod12449", "core", "rows", 4, metric, k=k)["check"](core[sel], parity)
    assert np.array_equal(core, dist[:, k - 1])
    assert (idx[:, 0] <= np.arange(idx.shape[0])).all() and (dist[:, 0] == 0).all()
    assert same_bits((dist, idx), host(*manifold.knn_graph(xd, k, metric)))


# ------------------------------------------------------------------------------------------------ workspace


def _bytes(t):
    return Guarded((t.numel() * t.element_size(),), torch.uint8)


def _calls(lib):
    """name -> (plan, the wrapper's outputs, call(ws_ptr, ws_bytes, *output ptrs)): every C entry point of the sliced modes
    at a multi-tile shape, d = 4, Euclidean."""
    from ssl_wafermap_amd import cluster, manifold

    st = stream()
    out = {}
    k, metric = 16, "euclidean"
    c = case("sq3000", "knn", "rows", 4, metric, k=k)
    n = 3000
    x = dev(c["x"])
    out["wm_core_distance"] = (plan("core", n, n, k), [cluster.core_distances(x, k, metric)],
                               lambda ws, wb, o: lib.wm_core_distance(x.data_ptr(), n, 4, 0, k, o, ws, wb, st))
    out["wm_knn_graph"] = (plan("knn", n, n, k), list(manifold.knn_graph(x, k, metric)),
                           lambda ws, wb, o, oj: lib.wm_knn_graph(x.data_ptr(), n, 4, 0, k, o, oj, ws, wb, st))
    c = case("sq3000", "minedge", "rows", 4, metric, kind="blocks")
    core, comp = dev(c["kw"]["core"]), dev(c["kw"]["comp"])
    out["wm_mreach_min_edge"] = (plan("minedge", n, n), list(cluster.min_outgoing_edges(x, core, comp, metric)),
                                 lambda ws, wb, o, oj: lib.wm_mreach_min_edge(x.data_ptr(), core.data_ptr(), comp.data_ptr(), n, 4, 0,
                                                                              1.0, o, oj, ws, wb, st))
    c = case("g3000", "minedge_g", "rows", 4, metric, kind="blocks")
    xg, cg, pg, gg = dev(c["x"]), dev(c["kw"]["core"]), dev(c["kw"]["comp"]), dev(c["group"])
    out["wm_mreach_min_edge_grouped"] = (
        plan("minedge_g", n, n, 1, 5), list(cluster.grouped_min_outgoing_edges(xg, cg, pg, gg, 5, metric)),
        lambda ws, wb, o, oj: lib.wm_mreach_min_edge_grouped(xg.data_ptr(), cg.data_ptr(), pg.data_ptr(), gg.data_ptr(), n, 4, 0, 5, o,
                                                             oj, ws, wb, st))
    c = case("ap2600", "apcore", "rows", 4, metric)
    xa, ga = dev(c["x"]), dev(c["group"])
    out["wm_allpoints_core"] = (plan("apcore", 2600, 2600, 1, 5), [cluster.allpoints_core_distances(xa, c["group"], d=4.0, metric=metric)],
                                lambda ws, wb, o: lib.wm_allpoints_core(xa.data_ptr(), ga.data_ptr(), 2600, 4, 0, 5, 4.0, o, ws, wb, st))
    c = case("q4200x2600", "mreachq", "rows", 4, metric)
    m, nq = 4200, 2600
    xf, xq, cf, cq = dev(c["x"]), dev(c["xr"]), dev(c["kw"]["core"]), dev(c["kw"]["core_q"])
    out["wm_knn_query"] = (plan("knn", m, nq, k), list(manifold.knn_query(xq, xf, k, metric)),
                           lambda ws, wb, o, oj: lib.wm_knn_query(xq.data_ptr(), m, xf.data_ptr(), nq, 4, 0, k, o, oj, ws, wb, st))
    out["wm_mreach_query"] = (plan("mreachq", m, nq), list(cluster.mreach_query(xq, cq, xf, cf, metric)),
                              lambda ws, wb, o, od, oj: lib.wm_mreach_query(xq.data_ptr(), cq.data_ptr(), m, xf.data_ptr(), cf.data_ptr(),
                                                                            nq, 4, 0, 1.0, o, od, oj, ws, wb, st))
    return out


def test_every_sliced_entry_point_stays_inside_exactly_its_planned_workspace():
    """Exactly plan.bytes of workspace (the size function's answer less its slack of 256) between sentinel margins: the
    call succeeds, gives the wrapper's bits and leaves the margins alone; one byte less is the workspace error, before any
    launch (the outputs keep their sentinel)."""
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    for name, (pl, want, call) in _calls(lib).items():
        ws = Guarded((pl.bytes,), torch.uint8)
        outs = [_bytes(t) for t in want]
        assert call(ws.ptr, pl.bytes - 1, *[o.ptr for o in outs]) == -3, name
        torch.cuda.synchronize()
        assert all(bool((o.whole == o.fill).all()) for o in outs) and bool((ws.whole == ws.fill).all()), f"{name}: a launch despite the error"
        _lib.check(call(ws.ptr, pl.bytes, *[o.ptr for o in outs]), name)
        live = list(Guarded.live)
        finish(name)
        assert len(live) == len(outs) + 1
        for o, t in zip(outs, want):
            assert torch.equal(o.t, t.contiguous().view(-1).view(torch.uint8)), f"{name}: the wrapper's bits"
