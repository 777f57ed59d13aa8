"""What the slice-level tests of csrc/cluster.hip share, without a GPU: a mirror of the host schedule (cl_mode / cl_grid /
cl_plan and the block-diagonal cut of cl_pairs), float64 references computed by direct differences, an exact integer
family large enough for several tiles per slice, a numpy restatement of the sliced selection with switches that each seed
one wrong computation, and the checkers that tests/test_gpu_cluster_slices.py applies to the kernels and
tests/test_cluster_cases_cpu.py to the restatement.

The one tolerance is eps(d) = (d + 3) * 2^-24 relative, the bound csrc/cluster.hip states for one float32 distance against
the exact distance of the float32 rows (test_gpu_cluster.py repeats the count).  Order statistics, minima and maxima of
values within eps are within eps.  The all-points core distance adds DOUBLE = 2^-36 for its float64 arithmetic, as derived
in test_gpu_dbcv.py (p |log dist| < 2^13 holds here: p <= 52 and distances between 1e-3 and 1e3).  On big_lattice every
distance is exactly representable and results are equal, not close."""
from collections import namedtuple

import numpy as np

COLS = 64           # CL_COLS: rows j per column tile
WANT_GROUPS = 1024  # cl_grid: about this many workgroups
CHUNK_BYTES = 64 << 20  # the largest temporary of a reference (the issue allows about 256 MB; smaller stays in cache)
U, U64 = 2.0 ** -24, 2.0 ** -53  # the unit roundoffs of float32 and float64
DOUBLE = 2.0 ** -36          # the float64 arithmetic of the all-points core distance (test_gpu_dbcv.py derives it)

METRICS = ["euclidean", "manhattan"]


def eps(d):
    return (d + 3) * U


def rows(n, d, seed):
    """float32 rows with exact duplicates among them (rows 3, 5, 7 and the last equal row 0 when they exist)."""
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    for i in (3, 5, 7, n - 1):
        if 0 < i < n:
            x[i] = x[0]
    return x


def max_rel(got, want):
    """Largest relative error where the reference is positive; where it is exactly 0 so must the result be."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    zero = want == 0
    assert (got[zero] == 0).all(), "an exactly zero reference needs an exactly zero result"
    return float(np.max(np.abs(got - want)[~zero] / want[~zero])) if (~zero).any() else 0.0


def components(n, kind):
    """Component ids of a Boruvka round.  `blocks`: runs of 100 rows, so that a row's lightest outgoing edge often lies in
    a later tile or slice than the row itself."""
    if kind == "singletons":
        return np.arange(n, dtype=np.int32)[::-1].copy()  # ids are labels, not positions
    if kind == "halves":
        return (np.arange(n) % 2).astype(np.int32) * 7 + 2
    if kind == "blocks":
        return (np.arange(n) // 100).astype(np.int32) * 3 + 1
    return np.full(n, 5, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the schedule

# cl_mode's lines: (tm, what a slice keeps an entry for, bytes per entry over all planes, direct, bounds, max slices)
_ANY = 1 << 30
_MODES = {
    "core": (8, "k", 4, False, False, _ANY),
    "knn": (8, "k", 8, False, False, _ANY),
    "minedge": (8, "row", 8, False, False, _ANY),
    "minedge_g": (8, "row", 8, False, True, _ANY),
    "mreachq": (8, "row", 12, False, False, _ANY),
    "apcore": (4, "row", 16, False, True, _ANY),
    "rank": (4, "k", 4, True, False, _ANY),
    "groupmin": (4, "group", 8, True, False, 16),
}
BLOCK_DIAGONAL = ("apcore", "minedge_g")

Plan = namedtuple("Plan", "mode row_tile row_tiles col_tiles tiles_per_slice slices last_tiles direct bytes")


def cdiv(a, b):
    return -(-a // b)


def plan(mode, m, n, k=1, g=1):
    """cl_plan<mode>(m, n, k, g): the grid and the workspace the entry point asks for (its size function adds 256)."""
    tm, per, entry, direct, bounds, max_slices = _MODES[mode]
    row_tile = 16 * tm
    row_tiles, col_tiles = cdiv(m, row_tile), cdiv(n, COLS)
    want = min(cdiv(WANT_GROUPS, row_tiles), col_tiles, max_slices)
    tps = cdiv(col_tiles, want)
    slices = cdiv(col_tiles, tps)
    direct = direct and slices == 1
    width = {"k": k, "group": g, "row": 1}[per]
    entries = 0 if direct else slices * m * width
    return Plan(mode, row_tile, row_tiles, col_tiles, tps, slices, col_tiles - (slices - 1) * tps, direct,
                entries * entry + (8 * g if bounds else 0))


def group_bounds(labels, g):
    """cl_group_bounds: per group its columns [first, last + 1) of the non-decreasing ids."""
    labels = np.asarray(labels)
    starts = np.searchsorted(labels, np.arange(g + 1))
    return np.stack([starts[:-1], starts[1:]], axis=1)


def diagonal_cut(bounds, labels, row_tile, slices, floor=False):
    """The block-diagonal cut of cl_pairs: per row tile (t0, t1, per, [(tile0, tile1) of every slice]).  `floor`: per by
    floor division, the seeded error."""
    labels = np.asarray(labels)
    n = labels.size
    out = []
    for i0 in range(0, n, row_tile):
        ga, gb = labels[i0], labels[min(i0 + row_tile, n) - 1]
        c0, c1 = max(int(bounds[ga][0]), 0), min(int(bounds[gb][1]), n)
        t0 = c0 // COLS
        t1 = cdiv(c1, COLS) if c1 > c0 else t0
        per = (t1 - t0) // slices if floor else cdiv(t1 - t0, slices)
        cuts = [(t0 + s * per, max(t0 + s * per, min(t0 + s * per + per, t1))) for s in range(slices)]
        out.append((t0, t1, per, cuts))
    return out


# ------------------------------------------------------------------------------------------------ references


def dist64(xr, x, metric, exact32=False):
    """The distances of the float32 rows xr [m, d] to x [n, d] in float64 by direct differences, [m, n], chunked over the
    rows.  exact32 (integer rows only): the float32 value of every distance, the way float32 arithmetic gives it -- the sum
    is an exact integer, the root is taken in float32, which numpy rounds correctly as the kernel's sqrtf does."""
    a, b = np.asarray(xr, dtype=np.float64), np.asarray(x, dtype=np.float64)
    m, n, d = a.shape[0], b.shape[0], b.shape[1]
    out = np.empty((m, n), dtype=np.float32 if exact32 else np.float64)
    step = max(1, CHUNK_BYTES // (n * d * 8))
    for r in range(0, m, step):
        diff = a[r:r + step, None, :] - b[None, :, :]
        if metric == "euclidean":
            np.multiply(diff, diff, out=diff)
            s = diff.sum(axis=-1)
            out[r:r + step] = np.sqrt(s.astype(np.float32)) if exact32 else np.sqrt(s)
        else:
            np.abs(diff, out=diff)
            out[r:r + step] = diff.sum(axis=-1)
    return out


def pair64(xr, x, idx, metric):
    """dist(xr[i], x[idx[i, q]]) in float64, [m, k]."""
    a, b = np.asarray(xr, dtype=np.float64), np.asarray(x, dtype=np.float64)
    diff = a[:, None, :] - b[np.asarray(idx, dtype=np.int64)]
    return np.sqrt((diff * diff).sum(-1)) if metric == "euclidean" else np.abs(diff).sum(-1)


def knn_ref(dist, k):
    """The k smallest of every row under (distance, index): (values [m, k], indices [m, k])."""
    idx = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(dist, idx, axis=1), idx


def min_edge_ref(dist, core, comp, alpha=1.0, group=None):
    """(w_all, w_min, j_min): the mutual-reachability weights max(core_i, core_j, dist / alpha) with +inf where no edge is
    allowed (same component; another group), the lightest per row and its lowest column; -1 where there is none."""
    core = np.asarray(core, dtype=dist.dtype)
    w = np.maximum(np.maximum(core[:, None], core[None, :]), dist / dist.dtype.type(alpha))
    ok = comp[:, None] != comp[None, :]
    if group is not None:
        ok &= np.asarray(group)[:, None] == np.asarray(group)[None, :]
    w[~ok] = np.inf
    j = w.argmin(axis=1)
    w_min = w[np.arange(w.shape[0]), j]
    return w, w_min, np.where(np.isinf(w_min), -1, j)


def query_ref(dist, core_q, core, alpha=1.0):
    """(w_all, w, dist, j) of the column first under (w, dist, j) for every query row."""
    cq, cr = np.asarray(core_q, dtype=dist.dtype), np.asarray(core, dtype=dist.dtype)
    w = np.maximum(np.maximum(cq[:, None], cr[None, :]), dist / dist.dtype.type(alpha))
    w_min = w.min(axis=1)
    j = np.where(w == w_min[:, None], dist, np.inf).argmin(axis=1)
    return w, w_min, dist[np.arange(dist.shape[0]), j], j


def _power_mean(lse, nc, p):
    with np.errstate(over="ignore"):
        return np.where(np.isneginf(lse) | (nc < 2), 0.0, np.exp(-(lse - np.log(np.maximum(nc - 1, 1))) / p))


def apcore_ref(dist, group, p):
    """DBCV's all-points core distance of every row inside its own group, by log-add-exp over the positive distances."""
    group = np.asarray(group)
    g = int(group.max()) + 1
    out = np.zeros(dist.shape[0])
    for a, b in group_bounds(group, g):
        blk = dist[a:b, a:b].astype(np.float64)  # (the exact family's float32 distances: the logarithm is a double's)
        with np.errstate(divide="ignore"):
            t = np.where(blk > 0, -p * np.log(blk), -np.inf)
        out[a:b] = _power_mean(np.logaddexp.reduce(t, axis=1), np.full(b - a, b - a), p)
    return out


# ------------------------------------------------------------------------------------------------ the exact family


def big_lattice(n, seed, boundary=None):
    """n <= 4200 float32 rows drawn with repetition from the integer grid {0..7}^4 (4096 points: exact duplicates
    everywhere), with a run of 120 identical rows from 104 columns before `boundary` to 16 behind it.  boundary: a column
    that starts a slice of at least two tiles, so that the run crosses the tile edge 64 columns before it INSIDE a slice
    (more than 64 equal candidates meet one carried list) and the slice edge itself; by default the first slice edge of the
    square TM = 8 schedule, or column 128 when its slices hold one tile.  Squares stay below 4 * 49, Manhattan sums below
    29: every distance is exact."""
    assert 200 <= n <= 4200
    x = np.random.default_rng(seed).integers(0, 8, (n, 4)).astype(np.float32)
    if boundary is None:
        boundary = COLS * max(plan("knn", n, n).tiles_per_slice, 2)
    assert boundary % COLS == 0 and boundary >= 2 * COLS and boundary + 16 <= n
    x[boundary - 104:boundary + 16] = x[boundary]
    return x


# ------------------------------------------------------------------------------------------------ the restatement

SWITCHES = ("list_reset_per_tile", "drop_last_tile_of_slice", "last_slice_takes_full_length", "tie_keeps_later_tile",
            "merge_skips_last_slice", "merge_tie_takes_later_slice", "diagonal_per_floor", "empty_slice_contributes_zero",
            "query_tie_ignores_dist")


def _lex_better(new, old, keys):
    """new before old under the lexicographic order of `keys` (tuples of arrays), strictly."""
    better = np.zeros(new[0].shape, dtype=bool)
    equal = np.ones(new[0].shape, dtype=bool)
    for q in keys:
        better |= equal & (new[q] < old[q])
        equal &= new[q] == old[q]
    return better


def emulate(mode, x, metric, pl, *, xq=None, k=1, core=None, comp=None, core_q=None, group=None, alpha=1.0, p=1.0,
            exact32=False, seed_error=None):
    """What the sliced schedule `pl` selects, restated in numpy on distances from dist64 (so the honest restatement
    differs from the references only in HOW it selects): per slice its tiles in order with the carried k-list / best /
    log-sum, then the merge in slice order.  xq: the row operand (x itself when None; a subset of x for sampled rows).

    Returns what the entry point returns: core -> kth [m]; knn -> (dist [m, k], idx [m, k]); minedge, minedge_g ->
    (w, j); mreachq -> (w, dist, j); apcore -> core [m].

    seed_error, one of SWITCHES, seeds one wrong computation:
      list_reset_per_tile            the carried list / best / sum starts afresh at every tile of a slice
      drop_last_tile_of_slice        a slice of more than one tile stops one tile early
      last_slice_takes_full_length   the last slice is not cut at col_tiles and nothing masks the columns behind n: they
                                     are the zero rows the staging pads with, core 0, in no component (not applied to the
                                     block-diagonal modes, whose cut has no last-slice clamp of this kind)
      tie_keeps_later_tile           a candidate of a later tile goes before its equals (lists) / replaces an equal best
      merge_skips_last_slice         the merge leaves out the last slice
      merge_tie_takes_later_slice    the merge orders equal candidates by descending slice
      diagonal_per_floor             the block-diagonal `per` by floor division
      empty_slice_contributes_zero   a slice without a tile hands the merge a zero (weight 0 at column 0; a term exp(0))
      query_tie_ignores_dist         the query's order is (w, j), not (w, dist, j)
    A switch that does not concern the mode changes nothing."""
    assert mode in _MODES and (seed_error is None or seed_error in SWITCHES)
    err = seed_error
    x = np.asarray(x)
    xr = x if xq is None else np.asarray(xq)
    n, m = x.shape[0], xr.shape[0]
    assert xq is None or mode in ("core", "knn", "mreachq"), "the other modes are square"
    diagonal = mode in BLOCK_DIAGONAL
    phantom = err == "last_slice_takes_full_length" and not diagonal
    width = COLS * (pl.slices * pl.tiles_per_slice if phantom else pl.col_tiles)
    xp = np.concatenate([x, np.zeros((width - n, x.shape[1]), dtype=x.dtype)])
    D = dist64(xr, xp, metric, exact32)
    col_ok = np.arange(width) < (width if phantom else n)
    inf = D.dtype.type(np.inf)
    pad = lambda v, fill: np.concatenate([np.asarray(v), np.full(width - n, fill, dtype=np.asarray(v).dtype)])  # noqa: E731

    # what a tile hands the epilogue: V [m, width] the value compared (+inf: not a candidate)
    if mode in ("core", "knn"):
        V = np.where(col_ok[None, :], D, inf)
    elif mode in ("minedge", "minedge_g"):
        cr, cp = pad(core, 0).astype(D.dtype), pad(comp, -1)
        V = np.maximum(np.maximum(cr[:n, None], cr[None, :]), D / D.dtype.type(alpha))
        ok = (cp[:n, None] != cp[None, :]) & col_ok[None, :]
        if mode == "minedge_g":
            gp = pad(group, -2)
            ok &= gp[:n, None] == gp[None, :]
        V = np.where(ok, V, inf)
    elif mode == "mreachq":
        cr = pad(core, 0).astype(D.dtype)
        V = np.maximum(np.maximum(np.asarray(core_q, dtype=D.dtype)[:, None], cr[None, :]), D / D.dtype.type(alpha))
        V = np.where(col_ok[None, :], V, inf)
    else:  # apcore: t = -p log dist, -inf for another group, a zero distance or a padded column
        gp = pad(group, -2)
        with np.errstate(divide="ignore"):
            V = np.where((gp[:n, None] == gp[None, :]) & (D > 0), -p * np.log(D.astype(np.float64)), -np.inf)

    # the row blocks and every slice's tile range
    if diagonal:
        cuts = diagonal_cut(group_bounds(group, int(np.max(group)) + 1), group, pl.row_tile, pl.slices,
                            floor=err == "diagonal_per_floor")
        blocks = [(r * pl.row_tile, min((r + 1) * pl.row_tile, m), c[3]) for r, c in enumerate(cuts)]
    else:
        rng = []
        for s in range(pl.slices):
            a = s * pl.tiles_per_slice
            rng.append((a, a + pl.tiles_per_slice if phantom else min(a + pl.tiles_per_slice, pl.col_tiles)))
        blocks = [(0, m, rng)]

    keys = {"minedge": (0, 2), "minedge_g": (0, 2), "mreachq": (0, 2) if err == "query_tie_ignores_dist" else (0, 1, 2)}.get(mode)
    outs = []
    for r0, r1, ranges in blocks:
        mb, ar = r1 - r0, np.arange(r1 - r0)
        parts = []
        for a, b in ranges:
            if err == "drop_last_tile_of_slice" and b - a > 1:
                b -= 1
            empty = b <= a
            if mode in ("core", "knn"):
                L, J = np.full((mb, k), inf), np.full((mb, k), -1, dtype=np.int64)
            elif mode == "apcore":
                L = np.full(mb, -np.inf)
            else:
                L = (np.full(mb, inf), np.full(mb, inf), np.full(mb, -1, dtype=np.int64))
            for t in range(a, b):
                c0 = t * COLS
                v = V[r0:r1, c0:c0 + COLS]
                cj = np.where(col_ok[c0:c0 + COLS], np.arange(c0, c0 + COLS), -1)
                if err == "list_reset_per_tile":
                    if mode in ("core", "knn"):
                        L, J = np.full((mb, k), inf), np.full((mb, k), -1, dtype=np.int64)
                    elif mode == "apcore":
                        L = np.full(mb, -np.inf)
                    else:
                        L = (np.full(mb, inf), np.full(mb, inf), np.full(mb, -1, dtype=np.int64))
                if mode in ("core", "knn"):
                    # a candidate below the k-th goes behind its equals: a stable sort with the list first
                    both = [L, v] if err != "tie_keeps_later_tile" else [v, L]
                    bj = [J, np.broadcast_to(cj, v.shape)] if err != "tie_keeps_later_tile" else [np.broadcast_to(cj, v.shape), J]
                    vv, jj = np.concatenate(both, axis=1), np.concatenate(bj, axis=1)
                    jj = np.where(np.isinf(vv), -1, jj)
                    o = np.argsort(vv, axis=1, kind="stable")[:, :k]
                    L, J = np.take_along_axis(vv, o, axis=1), np.take_along_axis(jj, o, axis=1)
                elif mode == "apcore":
                    L = np.logaddexp(L, np.logaddexp.reduce(v, axis=1))
                else:
                    dd = D[r0:r1, c0:c0 + COLS]
                    if 1 in keys:
                        at = np.where(v == v.min(axis=1)[:, None], dd, inf).argmin(axis=1)
                    else:
                        at = v.argmin(axis=1)
                    new = (v[ar, at], dd[ar, at], c0 + at)
                    take = np.isfinite(new[0]) & ((L[2] < 0) | (new[0] <= L[0] if err == "tie_keeps_later_tile" else
                                                                 _lex_better(new, L, keys)))
                    L = tuple(np.where(take, nw, od) for nw, od in zip(new, L))
            if empty and err == "empty_slice_contributes_zero":
                if mode == "apcore":
                    L = np.zeros(mb)
                elif mode not in ("core", "knn"):
                    L = (np.zeros(mb, dtype=D.dtype), np.zeros(mb, dtype=D.dtype), np.zeros(mb, dtype=np.int64))
            parts.append((L, J) if mode in ("core", "knn") else L)
        if err == "merge_skips_last_slice" and len(parts) > 1:
            parts = parts[:-1]
        if mode in ("core", "knn"):
            vv = np.concatenate([q[0] for q in parts], axis=1)
            jj = np.concatenate([q[1] for q in parts], axis=1)
            second = np.where(jj < 0, np.iinfo(np.int64).max, jj)
            if err == "merge_tie_takes_later_slice":
                second = np.broadcast_to(-np.repeat(np.arange(len(parts)), k), vv.shape)
            o = np.lexsort((second, vv), axis=-1)[:, :k]
            outs.append((np.take_along_axis(vv, o, axis=1), np.take_along_axis(jj, o, axis=1)))
        elif mode == "apcore":
            lse = np.full(mb, -np.inf)
            for q in parts:
                lse = np.logaddexp(lse, q)
            outs.append(lse)
        else:
            best = (np.full(mb, inf), np.full(mb, inf), np.full(mb, -1, dtype=np.int64))
            for q in parts:
                take = (q[2] >= 0) & ((best[2] < 0) | (q[0] <= best[0] if err == "merge_tie_takes_later_slice" else
                                                       _lex_better(q, best, keys)))
                best = tuple(np.where(take, nw, od) for nw, od in zip(q, best))
            outs.append(best)

    if mode in ("core", "knn"):
        dist, idx = (np.concatenate([o[q] for o in outs]) for q in range(2))
        return dist[:, k - 1] if mode == "core" else (dist, idx)
    if mode == "apcore":
        sizes = np.bincount(np.asarray(group))[np.asarray(group)]
        return _power_mean(np.concatenate(outs), sizes, p)
    w, dd, j = (np.concatenate([o[q] for o in outs]) for q in range(3))
    return (w, dd, j) if mode == "mreachq" else (w, j)


# ------------------------------------------------------------------------------------------------ the checkers


def bounded(name, measured, bound):
    """The plain form of parity_log.parity (the CPU file has no log to write)."""
    assert measured <= bound, f"{name}: measured {measured:.6g} > bound {bound:.6g}"


def check_core(tag, got, want_kth, d, log=bounded, exact=False):
    assert got.shape == want_kth.shape, tag
    if exact:
        assert np.array_equal(np.asarray(got, dtype=np.float32), want_kth.astype(np.float32)), f"{tag}: bits"
    log(f"{tag} rel", max_rel(got, want_kth), eps(d))


def check_knn(tag, got_d, got_j, want_d, want_j, xr, x, metric, log=bounded, exact=False):
    """Values within eps of the rank statistics; the returned index's true distance within eps of them too; every list
    sorted by (distance, index); no index twice; all in [0, n).  exact: the reference's bits and indices."""
    d, n = x.shape[1], x.shape[0]
    assert got_d.shape == got_j.shape == want_d.shape, tag
    assert (got_j >= 0).all() and (got_j < n).all(), f"{tag}: an index outside [0, n)"
    ordered = (got_d[:, 1:] > got_d[:, :-1]) | ((got_d[:, 1:] == got_d[:, :-1]) & (got_j[:, 1:] > got_j[:, :-1]))
    assert ordered.all(), f"{tag}: a list is not ordered by (distance, index)"
    s = np.sort(got_j, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), f"{tag}: an index appears twice"
    if exact:
        assert np.array_equal(np.asarray(got_d, dtype=np.float32), want_d.astype(np.float32)), f"{tag}: distance bits"
        assert np.array_equal(got_j, want_j), f"{tag}: indices under (distance, index)"
    log(f"{tag} distance rel", max_rel(got_d, want_d), eps(d))
    log(f"{tag} index rel", max_rel(pair64(xr, x, got_j, metric), want_d), eps(d))


def check_min_edge(tag, got_w, got_j, ref, comp, d, group=None, log=bounded, exact=False):
    """ref: min_edge_ref's triple.  The argmin satisfies its filter, its true weight and the returned weight are within eps
    of the minimum, rows without an edge say -1 / +inf.  exact: the weight's bits and the lowest j of the whole row."""
    w_all, w_min, j_min = ref
    none = j_min < 0
    assert np.array_equal(got_j < 0, none), f"{tag}: the rows without an outgoing edge differ"
    assert np.isposinf(np.asarray(got_w)[none]).all(), tag
    has = np.flatnonzero(~none)
    gj = got_j[has]
    assert (gj < w_all.shape[1]).all() and (comp[gj] != comp[has]).all(), f"{tag}: an edge inside a component"
    if group is not None:
        assert (np.asarray(group)[gj] == np.asarray(group)[has]).all(), f"{tag}: an edge between two groups"
    if exact:
        assert np.array_equal(np.asarray(got_w, dtype=np.float32)[has], w_min[has].astype(np.float32)), f"{tag}: weight bits"
        assert np.array_equal(got_j, j_min), f"{tag}: equal weights must resolve to the lowest j of the whole row"
    if has.size:
        log(f"{tag} weight rel", max_rel(np.asarray(got_w)[has], w_min[has]), eps(d))
        log(f"{tag} argmin rel", max_rel(w_all[has, gj], w_min[has]), eps(d))


def check_query(tag, got_w, got_d, got_j, ref, d, log=bounded, exact=False):
    """ref: query_ref's (w_all, w, dist, j) with the distances it was made from as ref[4].  exact: the (w, dist, j) order."""
    w_all, w_min, d_min, j_min, dist = ref
    ar = np.arange(w_all.shape[0])
    assert (got_j >= 0).all() and (got_j < w_all.shape[1]).all(), f"{tag}: an index outside [0, n)"
    if exact:
        assert np.array_equal(np.asarray(got_w, dtype=np.float32), w_min.astype(np.float32)), f"{tag}: weight bits"
        assert np.array_equal(np.asarray(got_d, dtype=np.float32), d_min.astype(np.float32)), f"{tag}: equal weights go to the nearer"
        assert np.array_equal(got_j, j_min), f"{tag}: equal (w, dist) go to the lowest j"
    log(f"{tag} weight rel", max_rel(got_w, w_min), eps(d))
    log(f"{tag} argmin rel", max_rel(w_all[ar, got_j], w_min), eps(d))
    log(f"{tag} distance of the argmin rel", max_rel(got_d, dist[ar, got_j]), eps(d))


def check_apcore(tag, got, want, d, log=bounded):
    assert got.shape == want.shape and np.isfinite(got).all(), tag
    log(f"{tag} rel", max_rel(got, want), eps(d) + DOUBLE)


# ------------------------------------------------------------------------------------------------ the shapes

# The shapes of test_gpu_cluster_slices.py, each chosen for a property of the schedule that test_cluster_cases_cpu.py
# re-proves from plan(): m rows against n columns, the modes run on it, the widths d, g groups (rows sorted by group).
SHAPES = {
    "sq3000": dict(m=3000, n=3000, modes=("core", "knn", "minedge"), widths=(4, 52)),
    "sq4200": dict(m=4200, n=4200, modes=("core", "knn", "minedge"), widths=(4,)),
    "q4200x2600": dict(m=4200, n=2600, modes=("knn", "mreachq"), widths=(4, 52)),
    "q130945x200": dict(m=130945, n=200, modes=("knn", "mreachq"), widths=(4,)),
    "ap2600": dict(m=2600, n=2600, modes=("apcore",), widths=(4, 52), g=5),
    "g3000": dict(m=3000, n=3000, modes=("minedge_g",), widths=(4, 52), g=5),
    "prod12449": dict(m=12449, n=12449, modes=("core", "knn"), widths=(4,), sampled=True),
}
KS = (1, 2, 16, 17, 64)  # the list-length edges of the small tests
CORE_K = 5               # the k of the core distances that the min-edge and query cases use


def grouped_labels(n):
    """Five groups of n - 400, 300, 63, 36 and 1 rows, sorted."""
    return np.repeat(np.arange(5), [n - 400, 300, 63, 36, 1]).astype(np.int32)


def sample_rows(n, count=512):
    """About `count` rows of n: the first, both sides of the first row-tile edge, the first and the last row of the last
    128-row tile, the rest spread evenly."""
    fixed = [0, 127, 128, (n - 1) // 128 * 128, n - 1]
    return np.unique(np.concatenate([fixed, np.linspace(0, n - 1, count - 3).astype(np.int64)]))


def lattice_rows(m, seed):
    return np.random.default_rng(seed).integers(0, 8, (m, 4)).astype(np.float32)


def operands(shape, family, d):
    """(x [n, d], xq [m, d] or None for a square shape, group [n] or None) of a shape and a family (`rows`, `lattice`)."""
    sp = SHAPES[shape]
    m, n = sp["m"], sp["n"]
    seed = 1000 * n + d
    if family == "rows":
        x = rows(n, d, seed)
        xq = None if m == n else rows(m, d, seed + 1)
        if xq is not None:
            xq[[1, m // 2, m - 1]] = x[[0, n // 2, n - 1]]  # queries that are fitted rows: exact zeros
    else:
        assert d == 4, "the lattice is four-dimensional"
        mode = sp["modes"][0]
        pl = plan(mode, m, n, 1, sp.get("g", 1))
        per = 2 if mode in BLOCK_DIAGONAL else pl.tiles_per_slice  # (the large group's per, which the CPU file asserts)
        x = big_lattice(n, seed, COLS * (max(per, 2) if pl.slices > 1 else 2))
        xq = None if m == n else lattice_rows(m, seed + 1)
    return x, xq, (grouped_labels(n) if "g" in sp else None)


_DIST = {}


def distances(shape, family, d, metric):
    """(x, xq, group, rows, dist): the operands, the row indices the distances are for (all, or the sample), and dist64 of
    those rows against x (float32 and exact on the lattice).  One shape's matrix is kept at a time."""
    key = (shape, family, d, metric)
    if key not in _DIST:
        _DIST.clear()
        x, xq, group = operands(shape, family, d)
        sel = sample_rows(x.shape[0]) if SHAPES[shape].get("sampled") else None
        xr = xq if xq is not None else (x if sel is None else x[sel])
        _DIST[key] = (x, xq, group, sel, dist64(xr, x, metric, exact32=family == "lattice"))
    return _DIST[key]


_CASES, _KNN = {}, {}


def kth(dist, k):
    """The k-th smallest of every row (self included)."""
    return np.partition(dist, k - 1, axis=1)[:, k - 1]


def case(shape, mode, family, d, metric, k=1, kind="singletons", alpha=1.0):
    """Everything one comparison needs: dict(x, xr, pl, kw = emulate's operands, ref, check(got, log)).  `got` is what
    emulate returns for the mode, or the entry point's outputs as numpy arrays in the same order."""
    key = (shape, mode, family, d, metric, k, kind, alpha)
    if key in _CASES:
        return _CASES[key]
    if len(_CASES) > 8:
        _CASES.clear()
    x, xq, group, sel, dist = distances(shape, family, d, metric)
    sp = SHAPES[shape]
    exact = family == "lattice"
    f32 = lambda v: v.astype(np.float32)  # noqa: E731
    tag = f"{shape} {mode} {family} {metric} d={d}"
    pl = plan(mode, sp["m"], sp["n"], k, sp.get("g", 1))
    xr = xq if xq is not None else (x if sel is None else x[sel])
    kw = dict(xq=xq if sel is None else xr, exact32=exact)
    if mode in ("core", "knn"):
        if (shape, family, d, metric) not in _KNN:  # one sort per distance matrix, at the longest list
            _KNN.clear()
            _KNN[shape, family, d, metric] = knn_ref(dist, min(max(KS), sp["n"]))
        want_d, want_j = (a[:, :k] for a in _KNN[shape, family, d, metric])
        kw["k"] = k
        if mode == "core":
            check = lambda got, log=bounded: check_core(f"{tag} k={k}", got, want_d[:, k - 1], d, log, exact)  # noqa: E731
        else:
            check = lambda got, log=bounded: check_knn(f"{tag} k={k}", got[0], got[1], want_d, want_j, xr, x, metric, log, exact)  # noqa: E731
        ref = (want_d, want_j)
    elif mode in ("minedge", "minedge_g"):
        core = f32(kth(dist, CORE_K))
        comp = components(sp["n"], kind)
        ref = min_edge_ref(dist, core, comp, alpha, group)
        kw.update(core=core, comp=comp, alpha=alpha, group=group)
        check = lambda got, log=bounded: check_min_edge(f"{tag} {kind} alpha={alpha:g}", got[0], got[1], ref, comp, d, group, log, exact)  # noqa: E731
    elif mode == "mreachq":
        own = dist64(x, x, metric, exact32=exact)
        core = f32(kth(own, CORE_K))
        core_q = f32(kth(dist, CORE_K))
        ref = query_ref(dist, core_q, core, alpha) + (dist,)
        kw.update(core=core, core_q=core_q, alpha=alpha)
        check = lambda got, log=bounded: check_query(f"{tag} alpha={alpha:g}", got[0], got[1], got[2], ref, d, log, exact)  # noqa: E731
    else:
        p = float(d)
        ref = apcore_ref(dist, group, p)
        kw.update(group=group, p=p)
        check = lambda got, log=bounded: check_apcore(f"{tag} p={p:g}", got, ref, d, log)  # noqa: E731
    _CASES[key] = dict(x=x, xr=xr, rows=sel, group=group, pl=pl, kw=kw, ref=ref, check=check, exact=exact, tag=tag)
    return _CASES[key]


def emulated(c, mode, metric, seed_error=None):
    return emulate(mode, c["x"], metric, c["pl"], seed_error=seed_error, **c["kw"])
