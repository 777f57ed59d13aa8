"""GPU tests of the retrieval kernels (csrc/knn.hip, csrc/knn_general.hip) and their Python layer against exact and
float64 references (tests/knn_cases.py): every streaming instantiation on schedules with ring wrap-around, partial
groups and a ragged tail chunk; both selection forms; the edges; the fall-back routes; the general kernel with a bias;
paging; merge; vote; cosine and Euclidean retrieval.  Every streaming case asserts the instantiation it reaches through
`knn_cases.plan` (at collection) and the library's workspace size (here)."""
import math

import numpy as np
import pytest
import torch

import knn_cases as kc
from parity_log import parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = kc.U
INT_MAX = kc.INT_MAX


def _F():
    from ssl_wafermap_amd import functional as F

    return F


def _lib():
    from ssl_wafermap_amd import _lib

    return _lib.load()


def _check_workspace(nq, n, d, k):
    got, want = _lib().wm_knn_topk_workspace_bytes(nq, n, d, k), kc.workspace_bytes(nq, n, d, k)
    assert got == want, f"the C plan and knn_cases.plan differ at nq={nq} n={n} d={d} k={k}: {got} != {want} bytes"


def _topk_checked(q, bank, dtype, k, base, exact, name, expect=None, monkeypatch=None, ref=None):
    """knn_topk on the device (both selection forms where k <= 8) through check_topk"""
    qd, bd = q.to(DEV), bank.to(DEV)
    ref = ref or kc.reference(qd, bd)
    qk, bk = qd.to(dtype).contiguous(), bd.to(dtype).contiguous()
    assert torch.equal(qk.float(), qd) and torch.equal(bk.float(), bd)  # the family is exact in the kernel's type
    forms = ("1024", "256") if (k <= 8 and monkeypatch is not None) else (None,)
    outs = []
    for th in forms:
        if th is not None:
            monkeypatch.setenv("WM_KNN_SELECT_THREADS", th)  # read per call
        sim, idx = _F().knn_topk(qk, bk, k, index_base=base)
        torch.cuda.synchronize()
        kc.check_topk(sim, idx, qd, bd, k, base, exact=exact, name=f"{name} select{th or ''}", ref=ref)
        for qi, rows in (expect or {}).items():
            assert idx[qi].tolist() == [r + base for r in rows], (name, qi, idx[qi].tolist(), rows)
        outs.append((sim, idx))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), f"{name}: the selection forms differ"
    return outs[0]


# ------------------------------------------------------------------------------------------------ streaming kernels
_EXTRA = {"bf16-d128-k8-b128-QT4-K8-S4", "bf16-d128-k16-b128-QT2-K16-S2", "f32-d128-k8-stream-QT4-K8-S3",
          "f32-d256-k16-stream-QT2-K16-S3"}
_STREAM = [(r, fam, n) for r in kc.STREAM_ROUTES for fam in ("lattice", "negative") for n in (kc.SMALL_N,)] + \
          [(r, "lattice", kc.SMALL_N_CONTROL) for r in kc.STREAM_ROUTES] + \
          [(r, fam, kc.SMALL_N) for r in kc.STREAM_ROUTES if kc.route_id(r) in _EXTRA for fam in ("gauss", "scaled", "planted")]


@pytest.mark.parametrize("r,family,n", _STREAM, ids=[f"{kc.route_id(r)}-{fam}-n{n}" for r, fam, n in _STREAM])
def test_stream_routes_small_bank_many_query_tiles(r, family, n, monkeypatch):
    """21 chunks on 4 slices (6 + 5 + 5 + 5): every ring depth wraps, every slice has a full and a partial group, the tail
    chunk has 37 rows (n = 2560: the control without a ragged tail); 64 or 128 query tiles."""
    p = kc.assert_route(r, n, 4, 6 if n == kc.SMALL_N else 5)
    assert p.qtiles in (64, 128)
    _check_workspace(r.nq, n, r.d, r.k)
    rb = r.d * (2 if r.dtype == kc.BF16 else 4)
    q, bank, expect = kc.make(family, r.nq, n, r.d, r.k, rb)
    _topk_checked(q, bank, r.dtype, r.k, 1000, family == "lattice", f"{kc.route_id(r)} {family} n{n}", expect, monkeypatch)


@pytest.mark.parametrize("family", ["planted", "negative", "lattice"])
def test_stream_one_query_tile_two_chunks_per_slice(family, monkeypatch):
    """64-query tiles, one query tile: 516 chunks on 258 slices, two chunks each; the planted ties cross slices (the
    second chunk of slice 0 against the first chunks of slices 1 .. 5)"""
    r, n = kc.ONE_TILE, kc.ONE_TILE_N
    kc.assert_route(r, n, 258, 2)
    _check_workspace(r.nq, n, r.d, r.k)
    q, bank, expect = kc.make(family, r.nq, n, r.d, r.k, 256)
    if family == "planted":
        assert max(kc.planted_positions(n, kc.plan(r.nq, n, 256, r.k, True), 11)["cross"]) >= 258 * kc.ROWS
    _topk_checked(q, bank, r.dtype, r.k, 7, family == "lattice", f"one-tile {family}", expect, monkeypatch)


@pytest.mark.parametrize("r", kc.STREAM_ROUTES, ids=kc.route_id)
def test_cross_slice_ties_come_back_lowest_first(r, monkeypatch):
    """the planted bit-identical rows, on every streaming instantiation and both selection forms: the k lowest in order"""
    rb = r.d * (2 if r.dtype == kc.BF16 else 4)
    q, bank, expect = kc.planted(r.nq, kc.SMALL_N, r.d, r.k, rb)
    keep = sorted(expect)
    assert len(keep) >= 4
    m = max(keep) + 1
    # the schedule is the full batch's: run all queries, check the head that holds the planted ones
    qd, bd = q.to(DEV).to(r.dtype), bank.to(DEV).to(r.dtype)
    for th in (("1024", "256") if r.k <= 8 else ("1024",)):
        monkeypatch.setenv("WM_KNN_SELECT_THREADS", th)
        sim, idx = _F().knn_topk(qd, bd, r.k)
        for qi in keep:
            assert idx[qi].tolist() == expect[qi], (kc.route_id(r), th, qi, idx[qi].tolist(), expect[qi])
            assert bool((sim[qi] == sim[qi, 0]).all())
    kc.check_topk(sim[:m], idx[:m], q[:m].to(DEV), bank.to(DEV), r.k, name=f"{kc.route_id(r)} planted head")


@pytest.mark.parametrize("n", kc.EDGE_N)
def test_stream_edges(n, monkeypatch):
    """nq in {1, 31, 32, 33, 64, 65, 129} x n x k in {1, 8, 9, 16, n}, a nonzero index base, lattice (bits) and negative"""
    for dtype, d in ((kc.BF16, 128), (kc.F32, 64)):
        for family in ("lattice", "negative"):
            qa, bank = kc.FAMILIES[family](max(kc.EDGE_NQ), n, d, seed=n)
            bd = bank.to(DEV)
            for nq in kc.EDGE_NQ:
                qd = qa[:nq].to(DEV)
                ref = kc.reference(qd, bd)
                for k in sorted({k for k in (1, 8, 9, 16, n) if k <= min(n, 16)}):
                    assert kc.route(dtype, d, k) in ("b128", "stream")
                    _check_workspace(nq, n, d, k)
                    _topk_checked(qd, bd, dtype, k, 12345, family == "lattice", f"edge nq{nq} n{n} k{k} {family}",
                                  monkeypatch=monkeypatch if nq in (1, 33, 129) else None, ref=ref)
    with pytest.raises(Exception):
        _F().knn_topk(qd.to(dtype), bd.to(dtype), n + 1)


@pytest.mark.parametrize("dtype,d,k", [(kc.F32, 512, 9), (kc.F32, 512, 16), (kc.BF16, 768, 5), (kc.F32, 768, 16),
                                       (kc.BF16, 768, 16)])
def test_fallback_routes_to_the_general_kernel(dtype, d, k):
    assert kc.route(dtype, d, k) == "general"
    nq, n = 70, 1500
    for family in ("lattice", "negative"):
        q, bank = kc.FAMILIES[family](nq, n, d)
        _topk_checked(q, bank, dtype, k, 77, family == "lattice", f"fallback d{d} k{k} {family}")


# ------------------------------------------------------------------------------------------------ general kernel, paging
@pytest.mark.parametrize("d", [4, 6, 100, 1024])
def test_general_kernel_with_bias(d):
    """wm_knn_topk_general: score = q.x + bias[row] on lattice rows with a bias of multiples of 1/64 (some rows -inf):
    exact in float32, so bits and indices against the stable argsort"""
    from ssl_wafermap_amd.retrieval import _topk_general

    g = torch.Generator().manual_seed(d)
    for n in (1, 3, 4, 255, 256, 257, 1025):
        qa, bank = kc.lattice(9, n, d, seed=n)
        bias = torch.randint(-64, 65, (n,), generator=g).float() / 64
        bias[torch.rand(n, generator=g) < 0.1] = -math.inf
        pad = (-d) % 4
        bp = torch.nn.functional.pad(bank, (0, pad)).to(DEV).contiguous()
        for nq in (1, 8, 9):
            qp = torch.nn.functional.pad(qa[:nq], (0, pad)).to(DEV).contiguous()
            sc = qp.double() @ bp.double().t() + bias.to(DEV).double()
            assert bool((sc.float().double() == sc).all())
            for k in sorted({k for k in (1, 16, n) if k <= min(n, 16)}):
                sim, idx = _topk_general(qp, bp, bias.to(DEV), k)
                v, i = kc.stable_topk(sc, k)
                assert torch.equal(sim, v.float()), (d, n, nq, k)
                assert torch.equal(idx.long(), i), (d, n, nq, k)


@pytest.mark.parametrize("dtype,d", [(kc.F32, 96), (kc.BF16, 128)])
def test_paged_topk_ties_across_pages(dtype, d):
    """k > 16: pages of 16 from the general kernel; lattice rows, so ties span the page boundaries"""
    q, bank = kc.lattice(9, 777, d)
    qd, bd = q.to(DEV), bank.to(DEV)
    sc = qd.double() @ bd.double().t()
    for k in (17, 32, 33, 200):
        assert kc.route(dtype, d, k) == "paged"
        sim, idx = _F().knn_topk(qd.to(dtype), bd.to(dtype), k, index_base=3)
        v, i = kc.stable_topk(sc, k)
        assert torch.equal(sim, v.float()) and torch.equal(idx.long() - 3, i), k


# ------------------------------------------------------------------------------------------------ merge, vote
@pytest.mark.parametrize("parts", [1, 2, 7, 64])
@pytest.mark.parametrize("k", [1, 8, 9, 16])
def test_merge_is_the_sorted_union(parts, k):
    nq = 37
    g = torch.Generator().manual_seed(parts * 100 + k)
    sims = torch.randint(-8, 9, (parts, nq, k), generator=g).float() / 8           # equal scores across parts abound
    idxs = torch.stack([torch.randperm(parts * k, generator=g) for _ in range(nq)]).reshape(nq, parts, k) \
        .permute(1, 0, 2).contiguous().int()                                        # distinct per query
    if parts > 1:
        short = torch.randint(k - k // 2, k + 1, (parts, nq, 1), generator=g)       # lists padded with (-inf, INT_MAX)
        padm = torch.arange(k).view(1, 1, k) >= short
        sims[padm], idxs[padm] = -math.inf, INT_MAX
    # every list in the list order
    key = np.lexsort((idxs.numpy(), -sims.numpy()), axis=-1)
    sims, idxs = torch.from_numpy(np.take_along_axis(sims.numpy(), key, -1)), torch.from_numpy(np.take_along_axis(idxs.numpy(), key, -1))
    msim, midx = _F().knn_merge(sims.to(DEV), idxs.to(DEV))
    alls, alli = sims.permute(1, 0, 2).reshape(nq, -1).numpy(), idxs.permute(1, 0, 2).reshape(nq, -1).numpy()
    o = np.lexsort((alli, -alls), axis=-1)[:, :k]
    assert np.array_equal(np.take_along_axis(alls, o, 1).view(np.uint32), msim.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.take_along_axis(alli, o, 1), midx.cpu().numpy())


@pytest.mark.parametrize("nc", [1, 9, 64])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_vote_scores_and_order(nc, k):
    """class scores against float64 sums of exp(sim / T) at (k + 4) 2^-24 relative; the predictions are the order of the
    kernel's own scores (descending, ties to the lower class id) and equal the float64 order wherever that is decided"""
    nq, n = 300, 5000
    g = torch.Generator().manual_seed(nc * 31 + k)
    labels = torch.randint(0, nc, (n,), generator=g)
    sim = torch.sort(torch.rand(nq, k, generator=g) * 2 - 1, dim=1, descending=True).values
    idx = torch.randint(0, n, (nq, k), generator=g).int()
    if k > 1:
        sim[::3, 1] = sim[::3, 0]            # two neighbours with one similarity: tied class scores where their classes differ
        sim[::7, -1], idx[::7, -1] = -math.inf, -1   # the padding entry of a short shard list
    for T in (0.07, 0.1, 1.0):
        pred, sc = _F().knn_vote(sim.to(DEV), idx.to(DEV), labels.to(DEV), nc, T, return_scores=True)
        pred, sc = pred.cpu(), sc.cpu()
        t32 = float(np.float32(T))           # the temperature the kernel reads
        w = torch.where(idx >= 0, torch.exp(sim.double() / t32), torch.zeros(nq, k, dtype=torch.float64))
        ref = torch.zeros(nq, nc, dtype=torch.float64)
        ref.scatter_add_(1, labels[idx.clamp_min(0).long()], w)
        tol = (k + 4) * U
        err = ((sc.double() - ref).abs() / ref.clamp_min(1e-300))[ref > 0]
        assert bool((sc[ref == 0] == 0).all())
        parity(f"knn_vote nc{nc} k{k} T{T} |score - float64| / ((k + 4) 2^-24 score)", float(err.max()) / tol, 1.0)
        # the kernel's order of its own scores
        own = torch.sort(sc, dim=1, descending=True, stable=True).indices
        assert torch.equal(pred, own), (nc, k, T)
        assert bool((torch.sort(pred, 1).values == torch.arange(nc)).all())
        rs, ro = torch.sort(ref, dim=1, descending=True, stable=True)
        # a rank whose float64 score is apart from both its neighbours' by more than the two errors is decided
        apart = torch.ones(nq, nc + 1, dtype=torch.bool)
        apart[:, 1:nc] = (rs[:, :-1] - rs[:, 1:]) > 2 * tol * rs[:, :-1]
        decided = apart[:, :-1] & apart[:, 1:]
        assert bool(decided[:, 0].float().mean() > 0.5) or k == 1 or nc == 1
        assert bool((pred == ro)[decided].all())
    if nc == 64:
        with pytest.raises(Exception):
            _F().knn_vote(sim.to(DEV), idx.to(DEV), labels.to(DEV), 65, 0.1)


# ------------------------------------------------------------------------------------------------ retrieval
def _check_distances(dist, idx, ref, rel, name):
    """nearest_neighbors against float64 distances `ref` [nq, n]: values within `rel` of the named pair's distance,
    ascending, distinct indices, and nothing left out that is nearer than the k-th by more than both errors"""
    idx = idx.long()
    at = torch.gather(ref, 1, idx)
    err = (dist.double() - at).abs()
    frac = torch.where(at > 0, err / (rel * at.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    parity(f"{name} |dist - float64| / bound", float(frac.max()), 1.0)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    srt = torch.sort(idx, 1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    out = torch.ones_like(ref, dtype=torch.bool)
    out.scatter_(1, idx, False)
    miss = out & (ref * (1 + rel) < at[:, -1:] * (1 - rel))
    assert not bool(miss.any()), f"{name}: a nearer row was left out"


def test_nearest_neighbors_against_float64():
    from ssl_wafermap_amd.retrieval import nearest_neighbors

    g = torch.Generator().manual_seed(9)
    for d, k in ((128, 8), (100, 5), (512, 16)):
        x = torch.randn(3000, d, generator=g).to(DEV)
        q = (x[:200] + 0.05 * torch.randn(200, d, generator=g).to(DEV)).contiguous()
        xd, qd = x.double(), q.double()
        l2 = torch.cdist(qd, xd, compute_mode="donot_use_mm_for_euclid_dist")  # the difference form
        dist, idx = nearest_neighbors(q, x, k, metric="l2")
        assert dist.dtype == torch.float32 and idx.dtype == torch.int64
        _check_distances(dist, idx, l2, (d + 3) * U, f"nearest_neighbors l2 d{d}")
        cos = 1 - torch.nn.functional.normalize(qd, dim=1) @ torch.nn.functional.normalize(xd, dim=1).t()
        dist, idx = nearest_neighbors(q, x, k, metric="cosine")
        assert dist.dtype == torch.float32 and idx.dtype == torch.int64
        # 1 - cos of rows normalised in float32: (d + 2) 2^-24 for the product of unit rows, and (d / 2 + 3) 2^-24
        # relative for each normalisation (d roundings under the square root, the root, the multiply)
        at = torch.gather(cos, 1, idx)
        parity(f"nearest_neighbors cosine d{d} |dist - float64| / (2 (d + 4) 2^-24)",
               float((dist.double() - at).abs().max()) / (2 * (d + 4) * U), 1.0)
        out = torch.ones_like(cos, dtype=torch.bool)
        out.scatter_(1, idx, False)
        assert not bool((out & (cos + 4 * (d + 4) * U < at[:, -1:])).any())


def test_nearest_neighbors_l2_with_a_large_common_offset():
    """mean 10, std 1, d = 512; the queries are bank rows and bank rows have bit-duplicates: the self-match and the
    duplicates come back at exactly 0 in index order, every distance within (d + 3) 2^-24 relative (the requirement
    manifold.knn_query documents).  |q|^2 - 2 (q.x - |x|^2 / 2) in float32 cancels at |x|^2 ~ 5e4 and does neither."""
    from ssl_wafermap_amd.retrieval import nearest_neighbors

    g = torch.Generator().manual_seed(10)
    d, n = 512, 2000
    x = 10 + torch.randn(n, d, generator=g)
    x[1000:1040] = x[:40]          # bit-duplicates
    x[1500:1520] = x[:20]
    x = x.to(DEV)
    q = x[:64].contiguous()
    dist, idx = nearest_neighbors(q, x, 5, metric="l2")
    ref = torch.cdist(q.double(), x.double(), compute_mode="donot_use_mm_for_euclid_dist")
    print("self-match distance, worst:", float(dist[:, 0].max()))
    for i in range(64):
        dup = [i] + ([i + 1000] if i < 40 else []) + ([i + 1500] if i < 20 else [])
        assert idx[i, :len(dup)].tolist() == dup, (i, idx[i].tolist())
        assert bool((dist[i, :len(dup)] == 0).all()), (i, dist[i].tolist())
    _check_distances(dist, idx, ref, (d + 3) * U, "nearest_neighbors l2 offset")
