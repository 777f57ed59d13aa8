"""The retrieval kernels of csrc/knn.hip and csrc/knn_general.hip restated for their tests: the exact reference and the
derived bound of a returned score, the checker `check_topk`, the input families, the launch arithmetic of knn.hip in
Python (`plan`, `route`, `workspace_bytes`), and `emulate_topk`, a numpy restatement of the two-stage selection with
switches that each seed ONE wrong computation.  tests/test_knn_cases_cpu.py proves that the honest emulation passes the
checker and that every switch is rejected; tests/test_gpu_knn.py runs the kernels through the same checker.

Reference: float64 `q @ bank.T` on the values the kernel reads, ordered by a stable sort (score descending, index
ascending).  Bound: a returned score is a float32 fmaf chain over d products (bf16 x bf16 products are exact in float32,
float32 products are rounded once inside the fma) and the four-lane xor-shuffle sum adds two additions, so
|score - exact| <= (d + 2) * 2^-24 * sum_i |q_i b_i|, taken per pair from |q| @ |bank|.T in float64.  (The general kernel
sums 16 fmaf per lane, six shuffle additions and the bias: fewer roundings, the same bound holds.)"""
import collections

import numpy as np
import torch

from parity_log import parity

U = 2.0 ** -24
ROWS = 128          # KNN_ROWS: bank rows per chunk
SLAB = 256          # KNN_SLAB: bytes per row per slab
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ launch arithmetic
def cdiv(a, b):
    return -(-a // b)


def pick_qt(rowbytes, nq, kt):
    qt = 2 if kt > 8 else 4
    while qt > 1 and qt * 32 * rowbytes > 65536:
        qt >>= 1
    while qt > 2 and (qt // 2) * 32 >= nq:
        qt >>= 1
    return qt


Plan = collections.namedtuple("Plan", "qt kt qtiles nslices iters ring")


def plan(nq, n, rowbytes, k, bf16=False):
    """make_plan of knn.hip: (32-query sub-tiles per block, list length, query tiles, slices, chunks of slice 0 -- the
    longest --, ring depth; `bf16` matters to the ring depth only).  Slice s owns chunks s, s + nslices, ...; a ring step is one 256-byte slab of one chunk."""
    kt = 8 if k <= 8 else 16
    qt = pick_qt(rowbytes, nq, kt)
    qtiles = cdiv(nq, qt * 32)
    total = cdiv(n, ROWS)
    want = min(max((256 if qt == 4 else 512) // qtiles, 1), 512)
    nslices = min(total, want)
    nslices = cdiv(total, cdiv(total, nslices))
    ring = (4 if qt == 4 else 2) if (bf16 and rowbytes == SLAB) else 3  # knn_stream_b128: bf16 rows of one slab
    return Plan(qt, kt, qtiles, nslices, cdiv(total, nslices), ring)


def route(dtype, d, k):
    """Where functional.knn_topk sends a call: 'b128' / 'stream' (knn.hip), 'general' (knn_general.hip), 'paged'."""
    if k > 16:
        return "paged"
    rowbytes = d * (2 if dtype == torch.bfloat16 else 4)
    ok = rowbytes % SLAB == 0 and rowbytes <= (2048 if dtype == torch.float32 else 1024) and (k <= 8 or rowbytes <= 1024)
    if not ok:
        return "general"
    return "b128" if dtype == torch.bfloat16 and rowbytes == SLAB else "stream"


def workspace_bytes(nq, n, d, k):
    """wm_knn_topk_workspace_bytes, from `plan`: a drift of the C plan shows as a different size."""
    cand = []
    for rowbytes in (2 * d, 4 * d):
        p = plan(nq, n, rowbytes, k)
        cand.append(p.qtiles * p.qt * 32 * p.nslices * p.kt)
    return max(cand) * 8 + nq * (8 if k <= 8 else 16) * 8 + 256


# ------------------------------------------------------------------------------------------------ reference and checker
def reference(q, bank):
    """(float64 scores [nq, n], per-pair bound [nq, n]) on the device the operands live on"""
    qd, bd = q.to(torch.float64), bank.to(torch.float64)
    d = q.shape[1]
    return qd @ bd.t(), (d + 2) * U * (qd.abs() @ bd.abs().t())


def stable_topk(ref, k):
    """the k first of every row in the order (score descending, index ascending)"""
    v, i = torch.sort(ref, dim=1, descending=True, stable=True)
    return v[:, :k], i[:, :k]


def _rank_in_class(bank):
    """for every bank row, how many bit-identical rows precede it"""
    _, inv = torch.unique(bank.to(torch.float32), dim=0, return_inverse=True)
    order = torch.argsort(inv, stable=True)
    sorted_cls = inv[order]
    n = inv.numel()
    pos = torch.arange(n, device=inv.device)
    first = torch.full((int(sorted_cls.max()) + 1,), n, device=inv.device, dtype=pos.dtype)
    first.scatter_reduce_(0, sorted_cls, pos, reduce="amin")
    rank = torch.empty(n, device=inv.device, dtype=pos.dtype)
    rank[order] = pos - first[sorted_cls]
    return inv, rank


def check_topk(sim, idx, q, bank, k, index_base=0, exact=False, name="knn", ref=None):
    """Every row of (sim, idx) against the float64 reference; no row is excused from any criterion.
    1. indices in [base, base + n), distinct per row; scores finite
    2. sim[r, j] within the pair's bound of the float64 score of the row it names
    3. sim descending; bit-equal scores in ascending index; of bit-identical bank rows the lowest come back first
    4. completeness: no bank row left out beats the k-th returned row by more than both bounds
    5. exact=True: sim is the reference in bits and idx the stable argsort, for every row
    Returns the worst fraction of the bound used (also written to the parity log)."""
    dev = q.device
    sim, idx = sim.to(dev), idx.to(dev).long()
    nq, n = q.shape[0], bank.shape[0]
    assert sim.shape == (nq, k) and idx.shape == (nq, k), f"{name}: shapes {tuple(sim.shape)} {tuple(idx.shape)}"
    assert sim.dtype == torch.float32
    sc, bound = reference(q, bank) if ref is None else ref
    loc = idx - index_base
    assert bool(((loc >= 0) & (loc < n)).all()), f"{name}: index outside [{index_base}, {index_base + n})"
    assert bool(torch.isfinite(sim).all()), f"{name}: non-finite score"
    srt = torch.sort(loc, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{name}: an index is returned twice"
    # 2
    sc_at, b_at = torch.gather(sc, 1, loc), torch.gather(bound, 1, loc)
    err = (sim.double() - sc_at).abs()
    frac = torch.where(b_at > 0, err / b_at.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    worst = parity(f"{name} |score - float64| / ((d + 2) 2^-24 sum|q b|)", float(frac.max()), 1.0)
    # 3
    assert bool((sim[:, :-1] >= sim[:, 1:]).all()), f"{name}: scores not descending"
    tie = sim[:, :-1] == sim[:, 1:]
    assert bool((loc[:, :-1] < loc[:, 1:])[tie].all()), f"{name}: bit-equal scores not in ascending index"
    cls, rank = _rank_in_class(bank)
    cr = cls[loc]
    same = (cr[:, :, None] == cr[:, None, :]).sum(-1)
    bad = rank[loc] >= same
    assert not bool(bad.any()), (f"{name}: a bit-identical bank row with a lower index was left out, e.g. query "
                                 f"{int(bad.any(1).nonzero()[0])}: {loc[bad.any(1)][0].tolist()}")
    # 4
    kth = sc_at[:, -1:] + b_at[:, -1:]
    out = torch.ones_like(sc, dtype=torch.bool)
    out.scatter_(1, loc, False)
    miss = out & (sc - bound > kth)
    assert not bool(miss.any()), (f"{name}: {int(miss.any(1).sum())} queries miss a neighbour that beats their k-th by more "
                                  f"than the bounds, e.g. query {int(miss.any(1).nonzero()[0])}")
    # 5
    if exact:
        assert bool((sc.float().double() == sc).all()), f"{name}: the exact family is not exact in float32 here"
        v, i = stable_topk(sc, k)
        assert torch.equal(sim, v.float()), f"{name}: scores differ from the exact reference in bits"
        neq = (loc != i).any(1)
        assert not bool(neq.any()), (f"{name}: {int(neq.sum())} rows differ from the stable argsort, e.g. query "
                                     f"{int(neq.nonzero()[0])}: got {loc[neq][0].tolist()} want {i[neq][0].tolist()}")
    return worst


# ------------------------------------------------------------------------------------------------ input families
def _bf16_exact(x):
    return x.bfloat16().float()


def _unit(x):
    return torch.nn.functional.normalize(x, dim=1)


def gauss(nq, n, d, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return _bf16_exact(_unit(torch.randn(nq, d, generator=g))), _bf16_exact(_unit(torch.randn(n, d, generator=g)))


def negative(nq, n, d, seed=0):
    """every query is minus the bank's mean direction plus noise: all similarities below zero, so a padded row (score 0)
    or a repeated row would win"""
    g = torch.Generator().manual_seed(2000 + seed)
    m = _unit(torch.randn(1, d, generator=g))
    bank = _bf16_exact(_unit(m + 0.5 * torch.randn(n, d, generator=g) / d ** 0.5))
    q = _bf16_exact(_unit(-m + 0.5 * torch.randn(nq, d, generator=g) / d ** 0.5))
    return q, bank


def scaled(nq, n, d, seed=0):
    """rows of norm 2^10 and 2^-10 mixed (powers of two keep the values bf16-exact): only a relative bound passes"""
    g = torch.Generator().manual_seed(3000 + seed)
    q, bank = gauss(nq, n, d, seed + 77)
    sq = torch.where(torch.rand(nq, 1, generator=g) < 0.5, 2.0 ** 10, 2.0 ** -10)
    sb = torch.where(torch.rand(n, 1, generator=g) < 0.5, 2.0 ** 10, 2.0 ** -10)
    return q * sq, bank * sb


def lattice(nq, n, d, seed=0):
    """entries in {-2 .. 2} / 8: for d <= 512 every partial sum is a multiple of 1/64 below 2^24 / 64, so any summation
    order gives the same bits; ties abound"""
    assert d <= 1024
    g = torch.Generator().manual_seed(4000 + seed)
    return (torch.randint(-2, 3, (nq, d), generator=g).float() / 8, torch.randint(-2, 3, (n, d), generator=g).float() / 8)


def planted_positions(n, p, copies):
    """Lists of `copies` bank positions whose bit-identical rows must come back lowest first -- each list more than kt
    long where it can be, so that a selection that ranks tied groups by anything but their lowest row drops one:
      half     : inside one 16-row accumulator half (rows 0 .. 15 of a wave's 32)
      straddle : around rows 127 / 128
      tail     : the rows before the last one of the ragged chunk;  last: row n - 1 (one copy)
      heads    : the first row of every slice, then of every later chunk
      cross    : later chunks of slice 0 (low first chunk) against the first chunks of slices 1, 2, ..."""
    total = cdiv(n, ROWS)
    out = {}
    half = list(range(16))[:copies]
    out["half"] = half
    out["straddle"] = [r for r in range(128 - copies // 2, 128 - copies // 2 + copies) if 0 <= r < n]
    out["tail"] = list(range(max(n - 1 - copies, 0), n - 1))
    out["last"] = [n - 1]   # alone: the query's other neighbours sit in other groups, which a repeated row n - 1 displaces
    out["heads"] = [c * ROWS for c in range(total)][:copies]
    # every chunk of the first slices, one row in each half of wave (chunk's place in its slice) % 4: every row its own
    # group, more tied groups than a list holds, and the later chunks of slice 0 (low first chunk) hold higher rows than
    # the first chunks of slices 1, 2, ...
    cross = []
    for c in range(total):
        if c % p.nslices < 6:
            for hf in (0, 1):
                r = c * ROWS + ((c // p.nslices) % 4) * 32 + hf * 16 + (c % 3)
                if r < n:
                    cross.append(r)
    out["cross"] = cross
    return {k_: sorted(set(v)) for k_, v in out.items() if len(v) > 0}


def planted(nq, n, d, k, rowbytes=None, seed=0):
    """gauss plus bit-identical copies of one row per pattern at the positions of planted_positions; query 37 * j + 1
    (wrapped into [0, nq)) is pattern j's row.  Returns (q, bank, {query: expected first k indices})."""
    q, bank = gauss(nq, n, d, seed + 5)
    g = torch.Generator().manual_seed(5000 + seed)
    p = plan(nq, n, rowbytes or 2 * d, k)
    kt = p.kt
    pos = planted_positions(n, p, kt + 3)
    used, taken, expect = set(), set(), {}
    for j, (name_, rows) in enumerate(sorted(pos.items())):
        rows = [r for r in rows if r not in used]
        if len(rows) < 1:
            continue
        used.update(rows)
        v = _bf16_exact(_unit(torch.randn(1, d, generator=g)))
        bank[rows] = v
        qi = (37 * j + 1) % nq
        while qi in taken:
            qi = (qi + 1) % nq
        taken.add(qi)
        q[qi] = v[0]
        if len(rows) >= k:
            expect[qi] = rows[:k]
    return q, bank, expect


FAMILIES = {"gauss": gauss, "negative": negative, "scaled": scaled, "lattice": lattice}


def make(family, nq, n, d, k, rowbytes=None, seed=0):
    """(q, bank, expect) of a family; expect is {} but for `planted`"""
    if family == "planted":
        return planted(nq, n, d, k, rowbytes, seed)
    q, bank = FAMILIES[family](nq, n, d, seed)
    return q, bank, {}


# ------------------------------------------------------------------------------------------------ emulation
def acc_row(reg, half):
    """bank row, inside a wave's 32, of accumulator register `reg` of lane half `half` (knn.hip feeds the MFMA its rows
    in the order tile_row, which makes a half's 16 rows consecutive)"""
    return reg + 16 * half


def _key(v, ident):
    """knn_key: unsigned order = (value descending, id ascending)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ident.astype(np.uint64))


def emulate_topk(q, bank, k, pl, b128=False, index_base=0, nq_total=None, unmasked_tail=False, unmasked_query_pad=False,
                 drop_last_chunk=False, doubled_chunk=False, tie_by_gid=False, tie_higher_index=False,
                 group_keeps_argmax_only=False, offer_skips_partial_group=False, index_base_dropped=False,
                 k16_as_k8=False, stale_ring_stage=False):
    """knn_stream / knn_stream_b128 + knn_select in numpy for the queries given (the schedule is `pl`'s, which may belong
    to a larger batch these queries are the head of).  Scores are the float32 rounding of the float64 product in both
    stages.  Stage 1: slice s takes chunks s, s + nslices, ...; a lane (wave, half) folds the 16 rows acc_row(e, half) of
    four consecutive chunks of its slice (64 rows) into one maximum and offers (maximum, group id); the K best groups by key
    survive the lane lists, the block merge and the selection (each keeps the K best under one total order).  Stage 2:
    the rows of those groups are rescored and the k best come back (value descending, index ascending).
    Switches (each ONE wrong computation):
      unmasked_tail            rows past n in the last chunk compete: score 0 (zero page) or row n - 1 again (b128)
      unmasked_query_pad       the queries of a ragged last query tile are staged as zeros
      drop_last_chunk          the last chunk of every slice is not multiplied
      doubled_chunk            the second chunk of a slice is its first one again
      tie_by_gid               groups keyed by (first chunk, wave, half), not by their best row
      tie_higher_index         the final order takes the higher index among equal scores
      group_keeps_argmax_only  only the best row of a selected group is rescored
      offer_skips_partial_group the offer of a slice's last, incomplete group is missing
      index_base_dropped       indices come back without the base
      k16_as_k8                lists of 8 where k > 8 needs 16
      stale_ring_stage         a chunk is multiplied one ring turn late (the stage still holds the chunk `ring` before)"""
    qn, bn = q.double().numpy(), bank.double().numpy()
    nq, n = qn.shape[0], bn.shape[0]
    S = (qn @ bn.T).astype(np.float32)
    total = cdiv(n, ROWS)
    ns = pl.nslices
    npad = total * ROWS
    rows = np.arange(npad)
    chunk = rows // ROWS
    sl, crel = chunk % ns, chunk // ns
    wave, within = (rows % ROWS) // 32, rows % 32
    half = within >> 4
    my_chunks = np.array([cdiv(total - s, ns) for s in range(ns)])
    # stage-1 scores: what the streaming kernel multiplies
    St = np.full((nq, npad), -np.inf, dtype=np.float32)
    St[:, :n] = S
    if unmasked_tail and npad > n:
        St[:, n:] = S[:, n - 1:n] if b128 else 0.0
    if unmasked_query_pad:
        qb = pl.qt * 32
        tot = nq_total or nq
        if tot % qb:
            St[(tot // qb) * qb:] = np.where(np.isfinite(St[(tot // qb) * qb:]), np.float32(0), -np.inf)
    src = rows.copy()   # the row whose data the stage holds when `rows` is multiplied
    if doubled_chunk:
        m = (crel == 1)
        src[m] = rows[m] - ns * ROWS
    if stale_ring_stage:
        m = crel >= pl.ring
        src[m] = rows[m] - pl.ring * ns * ROWS
    if doubled_chunk or stale_ring_stage:
        St = np.where((rows < n)[None, :], St[:, src], St)
    live = np.ones(npad, dtype=bool)
    if drop_last_chunk:
        live &= ~((crel == my_chunks[sl] - 1) & (my_chunks[sl] > 1))
    if offer_skips_partial_group:
        live &= ~((crel // 4 == (my_chunks[sl] - 1) // 4) & (my_chunks[sl] % 4 != 0))
    St = np.where(live[None, :], St, -np.inf)
    # groups
    gcode = ((sl * cdiv(int(my_chunks.max()), 4) + crel // 4) * 4 + wave) * 2 + half
    order = np.argsort(gcode, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(gcode[order]) != 0])
    ng = starts.size
    Sp = St[:, order]
    gmax = np.maximum.reduceat(Sp, starts, axis=1)                                  # [nq, ng]
    seg = np.repeat(np.arange(ng), np.diff(np.r_[starts, npad]))
    first = np.where(Sp == gmax[:, seg], order[None, :], INT_MAX)                   # the lowest row that attains it
    rep = np.minimum.reduceat(first, starts, axis=1)
    gid = ((sl + (crel & ~3) * ns) << 3 | wave << 1 | half)[order][starts]         # (first chunk, wave, half)
    ident = np.broadcast_to(gid[None, :], gmax.shape) if tie_by_gid else (rep & ~15)  # first row of the 16-row set
    K = 8 if (pl.kt == 8 or k16_as_k8) else 16
    gkey = np.where(np.isfinite(gmax), _key(gmax, np.minimum(ident, INT_MAX)), np.uint64(0))
    top = np.argsort(gkey, axis=1, kind="stable")[:, ::-1][:, :K]                   # keys are distinct (or 0)
    topkey = np.take_along_axis(gkey, top, 1)
    # stage 2: the rows of the selected groups, rescored
    grows = np.full((ng, 64), -1)
    cnt = np.diff(np.r_[starts, npad])
    for g_ in range(ng):
        grows[g_, :cnt[g_]] = order[starts[g_]:starts[g_] + cnt[g_]]
    cand = grows[top]                                                               # [nq, K, 64]
    if group_keeps_argmax_only:
        only = np.take_along_axis(rep, top, 1)
        cand = np.where(cand == only[:, :, None], cand, -1)
    cand = np.where(topkey[:, :, None] != 0, cand, -1).reshape(nq, -1)
    valid = (cand >= 0) & (cand < n)
    cs = np.where(valid, np.take_along_axis(S, np.clip(cand, 0, n - 1), 1), -np.inf).astype(np.float32)
    cid = np.where(valid, cand, 0)
    ckey = np.where(valid, _key(cs, (INT_MAX - cid) if tie_higher_index else cid), np.uint64(0))
    best = np.argsort(ckey, axis=1, kind="stable")[:, ::-1][:, :k]
    ok = np.take_along_axis(ckey, best, 1) != 0
    sim = np.where(ok, np.take_along_axis(cs, best, 1), -np.inf).astype(np.float32)
    idx = np.where(ok, np.take_along_axis(cid, best, 1) + (0 if index_base_dropped else index_base), -1).astype(np.int32)
    return torch.from_numpy(sim), torch.from_numpy(idx)


SWITCHES = ("unmasked_tail", "unmasked_query_pad", "drop_last_chunk", "doubled_chunk", "tie_by_gid", "tie_higher_index",
            "group_keeps_argmax_only", "offer_skips_partial_group", "index_base_dropped", "k16_as_k8", "stale_ring_stage")


# ------------------------------------------------------------------------------------------------ the cases
BF16, F32 = torch.bfloat16, torch.float32
Route = collections.namedtuple("Route", "dtype d k nq kernel qt kt ring")

# Small bank, many query tiles: n = 2597 is 21 chunks on 4 slices (slice 0: 6, the others 5): every ring depth wraps, every
# slice has a full and a partial group, the last chunk is ragged (37 rows).
SMALL_N, SMALL_N_CONTROL = 2597, 2560
STREAM_ROUTES = [
    Route(BF16, 128, 8, 8192, "b128", 4, 8, 4),
    Route(BF16, 128, 16, 8192, "b128", 2, 16, 2),
    Route(BF16, 256, 8, 8192, "stream", 4, 8, 3),
    Route(BF16, 256, 16, 8192, "stream", 2, 16, 3),
    Route(BF16, 384, 5, 8192, "stream", 2, 8, 3),
    Route(BF16, 512, 8, 8192, "stream", 2, 8, 3),
    Route(F32, 64, 8, 8192, "stream", 4, 8, 3),
    Route(F32, 64, 12, 8192, "stream", 2, 16, 3),
    Route(F32, 128, 8, 8192, "stream", 4, 8, 3),
    Route(F32, 192, 3, 8192, "stream", 2, 8, 3),
    Route(F32, 256, 16, 8192, "stream", 2, 16, 3),
    Route(F32, 320, 8, 4096, "stream", 1, 8, 3),
    Route(F32, 512, 8, 4096, "stream", 1, 8, 3),
]
# 64-query tiles with one query tile: 516 chunks on 258 slices of two chunks each
ONE_TILE = Route(BF16, 128, 8, 8, "b128", 2, 8, 2)
ONE_TILE_N = 66003


def route_id(r):
    return f"{'bf16' if r.dtype == BF16 else 'f32'}-d{r.d}-k{r.k}-{r.kernel}-QT{r.qt}-K{r.kt}-S{r.ring}"


def assert_route(r, n, nslices=None, iters=None):
    """the instantiation and schedule a case claims, against `plan` (called at collection time)"""
    rb = r.d * (2 if r.dtype == BF16 else 4)
    p = plan(r.nq, n, rb, r.k, r.dtype == BF16)
    assert route(r.dtype, r.d, r.k) == r.kernel, (route_id(r), route(r.dtype, r.d, r.k))
    assert (p.qt, p.kt, p.ring) == (r.qt, r.kt, r.ring), (route_id(r), p)
    if nslices is not None:
        assert (p.nslices, p.iters) == (nslices, iters), (route_id(r), n, p)
    return p


for _r in STREAM_ROUTES:
    assert_route(_r, SMALL_N, 4, 6)
    assert_route(_r, SMALL_N_CONTROL, 4, 5)
assert_route(ONE_TILE, ONE_TILE_N, 258, 2)
assert len({(r.dtype, r.kernel, r.qt, r.kt) for r in STREAM_ROUTES + [ONE_TILE]}) == 10  # every streaming instantiation

EDGE_NQ = (1, 31, 32, 33, 64, 65, 129)
EDGE_N = (1, 16, 17, 127, 128, 129, 512, 513)
