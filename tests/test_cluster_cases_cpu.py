"""CPU proof of tests/cluster_cases.py, the helper of tests/test_gpu_cluster_slices.py: the schedule mirror against the
library's own size functions (host code, no GPU), the property every GPU shape was chosen for, the honest restatement
against every checker, every seeded switch against the checkers on a (shape, mode, family) the GPU file runs, and the
chunked references against the small-n ones."""
import numpy as np
import pytest

import cluster_cases as cc
from cluster_cases import SHAPES, case, emulated, plan
from test_cluster_cpu import pairwise64, prim_mst
from test_dbcv_cpu import allpoints_core64


def _k(shape, family):
    """The list length a (shape, family) is emulated with: the lattice's run of equal rows needs the full 64; the
    production shape runs k = 16; the 130 945-row shape a short list on random rows (its sort is the cost here)."""
    if SHAPES[shape].get("sampled"):
        return 16
    if family == "lattice":
        return 64
    return 2 if shape == "q130945x200" else 17


def _families(shape):
    return ("rows",) if SHAPES[shape].get("sampled") else ("rows", "lattice")  # (big_lattice ends at 4200 rows)


# ------------------------------------------------------------------------------------------------ the mirror


def _library_bytes(lib, mode, m, n, d, k, g):
    if mode == "core":
        return lib.wm_core_distance_workspace_bytes(n, d, k)
    if mode == "knn":
        if m == n:
            assert lib.wm_knn_graph_workspace_bytes(n, d, k) == lib.wm_knn_query_workspace_bytes(n, n, d, k)
        return lib.wm_knn_query_workspace_bytes(m, n, d, k)
    if mode == "minedge":
        return lib.wm_mreach_min_edge_workspace_bytes(n, d)
    if mode == "minedge_g":
        return lib.wm_mreach_min_edge_grouped_workspace_bytes(n, d, g)
    if mode == "apcore":
        return lib.wm_allpoints_core_workspace_bytes(n, d, g)
    if mode == "mreachq":
        return lib.wm_mreach_query_workspace_bytes(m, n, d)
    if mode == "rank":
        return lib.wm_rank_query_workspace_bytes(m, n, d, k)
    return lib.wm_group_min_dist_workspace_bytes(m, n, d, g)


def _edges(mode):
    """The square sizes on either side of tiles_per_slice going 1 -> 2 for the mode's tile height, from the mirror."""
    out = []
    for n in range(64, 4000):
        if plan(mode, n, n).tiles_per_slice == 1 and plan(mode, n + 1, n + 1).tiles_per_slice == 2:
            out += [n, n + 1]
    assert out, mode
    return out


def test_plan_bytes_are_the_librarys_size_functions():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    square = ("core", "minedge", "minedge_g", "apcore")
    checked = 0
    for mode in cc._MODES:
        sizes = [(sp["m"], sp["n"]) for sp in SHAPES.values()]
        sizes += [(n, n) for n in _edges(mode)] + [(1, 1), (63, 64), (65, 65), (300, 300), (700, 700), (2100, 2600), (65500, 200)]
        for m, n in sizes:
            if mode in square and m != n:
                continue
            for k in cc.KS:
                for g in (1, 5, 37):
                    for d in (4, 52):
                        want = _library_bytes(lib, mode, m, n, d, k, g)
                        assert plan(mode, m, n, k, g).bytes + 256 == want, (mode, m, n, k, g, d)
                        checked += 1
    assert checked > 1000
    # the edges are where the issue's arithmetic puts them: n of about 2 900 for 128-row tiles, 2 050 for 64-row tiles
    assert 2800 <= _edges("knn")[0] <= 3000 and 2000 <= _edges("apcore")[0] <= 2100


def test_every_gpu_shape_has_the_property_it_was_chosen_for():
    p = plan("knn", 3000, 3000)
    assert (p.row_tiles, p.col_tiles, p.tiles_per_slice, p.slices, p.last_tiles) == (24, 47, 2, 24, 1)
    assert 3000 - 46 * cc.COLS == 56  # the last tile's columns; a short last slice
    for mode in ("core", "minedge"):
        assert plan(mode, 3000, 3000)[1:7] == p[1:7]
    p = plan("knn", 4200, 4200)
    assert p.tiles_per_slice == 3 and p.slices == 22 and p.last_tiles == 3 and 4200 - 65 * cc.COLS == 40
    for mode in ("knn", "mreachq"):
        p = plan(mode, 4200, 2600)
        assert (p.row_tiles, p.col_tiles, p.tiles_per_slice, p.slices, p.last_tiles) == (33, 41, 2, 21, 1)
        p = plan(mode, 130945, 200)
        assert p.row_tiles == 1024 and p.slices == 1 and p.col_tiles == p.tiles_per_slice == 4 and not p.direct
        assert 130945 - 1023 * p.row_tile == 1  # the last row tile holds one row
    p = plan("core", 12449, 12449, 16)
    assert (p.tiles_per_slice, p.slices, p.last_tiles) == (18, 11, 15)
    # the block-diagonal shapes: per == 2 for the row tiles of the large group, slices without a tile there and for every
    # other group, and (all-points core) a row tile that spans three groups
    for mode, n, slices in (("apcore", 2600, 21), ("minedge_g", 3000, 24)):
        p = plan(mode, n, n, 1, 5)
        assert p.slices == slices
        lab = cc.grouped_labels(n)
        assert np.bincount(lab).tolist() == [n - 400, 300, 63, 36, 1]
        cuts = cc.diagonal_cut(cc.group_bounds(lab, 5), lab, p.row_tile, p.slices)
        assert len(cuts) == p.row_tiles
        large = [c for r, c in enumerate(cuts) if lab[min((r + 1) * p.row_tile, n) - 1] == 0]
        assert len(large) >= 20 and all(c[2] == 2 for c in large)
        for t0, t1, per, ranges in cuts:
            assert sum(b - a for a, b in ranges) == t1 - t0 and ranges[0][0] == t0  # every tile once
            assert all(a2 == b1 or b2 == a2 for (_, b1), (a2, b2) in zip(ranges, ranges[1:]))
            assert sum(b == a for a, b in ranges) >= 1, "every row tile has at least one slice without a tile"
        spans = [np.unique(lab[r * p.row_tile:(r + 1) * p.row_tile]).size for r in range(p.row_tiles)]
        assert max(spans) >= 3 if mode == "apcore" else max(spans) >= 2
        floor = cc.diagonal_cut(cc.group_bounds(lab, 5), lab, p.row_tile, p.slices, floor=True)
        assert any(sum(b - a for a, b in c[3]) < c[1] - c[0] for c in floor)  # (the seeded error loses tiles here)


def test_the_lattice_run_crosses_a_tile_edge_inside_a_slice_and_a_slice_edge():
    for shape, sp in SHAPES.items():
        if sp.get("sampled"):
            continue
        x, _, _ = cc.operands(shape, "lattice", 4)
        # the run: the longest stretch of consecutive equal rows
        eq = (x[1:] == x[:-1]).all(axis=1)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], eq.astype(np.int8), [0]])))
        a, b = max(zip(edges[::2], edges[1::2]), key=lambda ab: ab[1] - ab[0])
        first, last = int(a), int(b)  # rows first .. last are equal
        assert last - first + 1 >= 120 > max(cc.KS)
        mode = sp["modes"][0]
        p = plan(mode, sp["m"], sp["n"], 1, sp.get("g", 1))
        per = 2 if mode in cc.BLOCK_DIAGONAL else p.tiles_per_slice
        tile_a, tile_b = first // cc.COLS, last // cc.COLS
        assert tile_b - tile_a >= 2, shape
        # two of its tiles share a slice, and (with several slices) it reaches into the next slice
        assert any(t // per == (t + 1) // per for t in range(tile_a, tile_b)), shape
        if p.slices > 1:
            assert tile_a // per != tile_b // per, shape
        assert (np.unique(x) == np.arange(8)).all() and x.shape[1] == 4


# ------------------------------------------------------------------------------------------------ the restatement

HONEST = [(shape, mode, family) for shape, sp in SHAPES.items() for mode in sp["modes"] for family in _families(shape)]


@pytest.mark.parametrize("shape,mode,family", HONEST)
def test_honest_restatement_passes_every_checker(shape, mode, family):
    for metric in (cc.METRICS if shape == "sq3000" else cc.METRICS[:1]):
        for alpha in ((1.0, 2.0) if family == "lattice" and mode in ("minedge", "mreachq") else (1.0,)):
            c = case(shape, mode, family, 4, metric, k=_k(shape, family), kind="blocks", alpha=alpha)
            c["check"](emulated(c, mode, metric))


# Every switch on pairs that the GPU file runs (all at d = 4, Euclidean).  Where a switch is left out for a mode it is
# equivalent there:
#   tie_keeps_later_tile, merge_tie_takes_later_slice on `core`: the k-th VALUE of a multiset does not depend on the
#     order of its equal members; on `apcore`: a sum has no ties.
#   last_slice_takes_full_length on `minedge`: the columns behind n would be zero rows in no component; one wins only
#     for a row nearer the origin than every row outside its component, which neither family has at these sizes (the
#     mask `j < n` is the same expression in every mode's epilogue, and `core`, `knn` and `mreachq` show it).
#   merge_skips_last_slice on the block-diagonal shapes: with per == 2 of 35 or 41 tiles the last slice has no tile for
#     any row tile, so leaving it out changes nothing; cl_minedge_merge is the square mode's (shown there), and
#     cl_apcore_merge's last slice holds a tile in test_gpu_dbcv's one-group case at n = 700 (11 slices of one tile).
#   query_tie_ignores_dist outside the lattice: random rows have no two equal weights with different distances.
REJECTED = [
    ("list_reset_per_tile", "sq3000", "core", "rows"),
    ("list_reset_per_tile", "sq4200", "knn", "lattice"),
    ("list_reset_per_tile", "sq3000", "minedge", "rows"),
    ("list_reset_per_tile", "q4200x2600", "mreachq", "rows"),
    ("list_reset_per_tile", "ap2600", "apcore", "rows"),
    ("list_reset_per_tile", "g3000", "minedge_g", "rows"),
    ("list_reset_per_tile", "prod12449", "knn", "rows"),
    ("drop_last_tile_of_slice", "sq4200", "knn", "rows"),
    ("drop_last_tile_of_slice", "sq3000", "minedge", "lattice"),
    ("drop_last_tile_of_slice", "q130945x200", "mreachq", "rows"),
    ("drop_last_tile_of_slice", "ap2600", "apcore", "lattice"),
    ("drop_last_tile_of_slice", "g3000", "minedge_g", "rows"),
    ("drop_last_tile_of_slice", "prod12449", "core", "rows"),
    ("last_slice_takes_full_length", "sq3000", "core", "rows"),
    ("last_slice_takes_full_length", "sq3000", "knn", "lattice"),
    ("last_slice_takes_full_length", "q4200x2600", "mreachq", "rows"),
    ("tie_keeps_later_tile", "sq3000", "knn", "lattice"),
    ("tie_keeps_later_tile", "sq4200", "minedge", "lattice"),
    ("tie_keeps_later_tile", "q4200x2600", "mreachq", "lattice"),
    ("tie_keeps_later_tile", "q130945x200", "knn", "lattice"),
    ("tie_keeps_later_tile", "g3000", "minedge_g", "lattice"),
    ("merge_skips_last_slice", "sq3000", "core", "rows"),
    ("merge_skips_last_slice", "sq4200", "knn", "lattice"),
    ("merge_skips_last_slice", "sq3000", "minedge", "rows"),
    ("merge_skips_last_slice", "q4200x2600", "mreachq", "rows"),
    ("merge_skips_last_slice", "prod12449", "knn", "rows"),
    ("merge_tie_takes_later_slice", "sq3000", "knn", "rows"),
    ("merge_tie_takes_later_slice", "sq4200", "minedge", "lattice"),
    ("merge_tie_takes_later_slice", "q4200x2600", "mreachq", "lattice"),
    ("merge_tie_takes_later_slice", "g3000", "minedge_g", "lattice"),
    ("diagonal_per_floor", "ap2600", "apcore", "rows"),
    ("diagonal_per_floor", "g3000", "minedge_g", "rows"),
    ("empty_slice_contributes_zero", "ap2600", "apcore", "rows"),
    ("empty_slice_contributes_zero", "g3000", "minedge_g", "rows"),
    ("query_tie_ignores_dist", "q4200x2600", "mreachq", "lattice"),
    ("query_tie_ignores_dist", "q130945x200", "mreachq", "lattice"),
]


def test_every_switch_is_in_the_table():
    assert {r[0] for r in REJECTED} == set(cc.SWITCHES)
    assert all(r[2] in SHAPES[r[1]]["modes"] and r[3] in _families(r[1]) for r in REJECTED)


@pytest.mark.parametrize("switch,shape,mode,family", REJECTED)
def test_seeded_switch_is_rejected(switch, shape, mode, family):
    c = case(shape, mode, family, 4, "euclidean", k=_k(shape, family), kind="blocks")
    got = emulated(c, mode, "euclidean", seed_error=switch)
    with pytest.raises(AssertionError):
        c["check"](got)


# ------------------------------------------------------------------------------------------------ the references


@pytest.mark.parametrize("metric", cc.METRICS)
def test_references_agree_with_the_small_ones_at_300_rows(metric):
    n, d, k = 300, 52, 5
    x = cc.rows(n, d, 11)
    small = pairwise64(x, metric)
    dist = cc.dist64(x, x, metric)
    assert cc.max_rel(dist, small) <= (d + 3) * cc.U64  # the same differences summed in another order, in float64: eps's count
    old, cc.CHUNK_BYTES = cc.CHUNK_BYTES, 7 * n * d * 8  # several chunks, the last one short
    try:
        assert np.array_equal(cc.dist64(x, x, metric), dist)
    finally:
        cc.CHUNK_BYTES = old
    vals, idx = cc.knn_ref(small, 64)
    assert np.array_equal(vals, np.sort(small, axis=1)[:, :64])
    assert np.array_equal(np.take_along_axis(small, idx, axis=1), vals)
    assert (idx[:, 0] == [0 if i in (3, 5, 7, n - 1) else i for i in range(n)]).all()  # an equal earlier row leads
    assert np.array_equal(cc.pair64(x, x, idx, metric), np.take_along_axis(dist, idx, axis=1))
    # one Boruvka round on singletons holds every row's lightest edge; the lightest of them all opens Prim's tree too
    core = np.sort(small, axis=1)[:, k - 1]
    w_all, w_min, j_min = cc.min_edge_ref(small, core, cc.components(n, "singletons"))
    u, v, w = prim_mst(x, k, metric)
    assert w_min.min() == w[0] and np.isinf(np.diag(w_all)).all()
    mr = np.maximum(np.maximum(core[:, None], core[None, :]), small)
    assert np.array_equal(mr[u, v], w)
    every = np.where(np.eye(n, dtype=bool), np.inf, mr)
    assert np.array_equal(w_min, every.min(axis=1)) and np.array_equal(j_min, every.argmin(axis=1))
    # the query form on x against itself with the (w, dist, j) order, by a sort of the triples
    qw, w_q, d_q, j_q = cc.query_ref(small, core, core)
    for i in range(0, n, 17):
        first = min(zip(qw[i].tolist(), small[i].tolist(), range(n)))
        assert (w_q[i], d_q[i], j_q[i]) == first
    # the all-points core distance, group by group, against test_dbcv_cpu's row loop
    group = np.repeat(np.arange(3), [200, 99, 1])
    got = cc.apcore_ref(small, group, float(d))
    for a, b in cc.group_bounds(group, 3):
        want = allpoints_core64(small[a:b, a:b], float(d)) if b - a > 1 else np.zeros(1)
        assert cc.max_rel(got[a:b], want) <= cc.DOUBLE  # (float64 log-add-exp in two orders: what DOUBLE was derived for)
    # the grouped lightest edge is the square one inside every group
    wg = cc.min_edge_ref(small, core, cc.components(n, "singletons"), group=group)
    assert wg[2][-1] == -1 and np.isposinf(wg[1][-1])
    sub = cc.min_edge_ref(small[:200, :200], core[:200], cc.components(n, "singletons")[:200])
    assert np.array_equal(wg[1][:200], sub[1]) and np.array_equal(wg[2][:200], sub[2])


def test_the_exact_family_is_exact_in_float32():
    x = cc.big_lattice(300, 3)
    for metric in cc.METRICS:
        d32 = cc.dist64(x, x, metric, exact32=True)
        d64 = cc.dist64(x, x, metric)
        assert d32.dtype == np.float32
        # float32 arithmetic in the kernel's order gives these bits: every partial sum is a small integer
        diff = x[:, None, :] - x[None, :, :]
        acc = np.zeros((300, 300), dtype=np.float32)
        for q in range(4):
            acc = acc + (diff[..., q] * diff[..., q] if metric == "euclidean" else np.abs(diff[..., q]))
        assert np.array_equal(np.sqrt(acc) if metric == "euclidean" else acc, d32)
        assert np.array_equal(d32, d64.astype(np.float32)) or metric == "euclidean"
        assert cc.max_rel(d32, d64) <= cc.U  # the root's one rounding
