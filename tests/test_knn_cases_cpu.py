"""CPU proof of the kNN checker (tests/knn_cases.py): the honest emulation of the two-stage selection passes check_topk
on every family and route of tests/test_gpu_knn.py, and every seeded wrong computation is rejected on a named case."""
import numpy as np
import pytest
import torch

import knn_cases as kc

NQ_CPU = 192  # the head of the GPU case's query batch, under the GPU case's plan


def _case(r, n, family, seed=0):
    rb = r.d * (2 if r.dtype == kc.BF16 else 4)
    q, bank, expect = kc.make(family, r.nq, n, r.d, r.k, rb, seed)
    m = min(NQ_CPU, r.nq)
    return q[:m].contiguous(), bank, {a: b for a, b in expect.items() if a < m}, kc.plan(r.nq, n, rb, r.k, r.dtype == kc.BF16)


def _run(r, n, family, index_base=0, **sw):
    q, bank, expect, pl = _case(r, n, family)
    sim, idx = kc.emulate_topk(q, bank, r.k, pl, b128=r.kernel == "b128", index_base=index_base, nq_total=r.nq, **sw)
    kc.check_topk(sim, idx, q, bank, r.k, index_base, exact=family == "lattice", name=f"emul {kc.route_id(r)} {family}")
    for qi, rows in expect.items():
        assert idx[qi].tolist() == [x + index_base for x in rows], (qi, idx[qi].tolist(), rows)


@pytest.mark.parametrize("family", ["gauss", "negative", "scaled", "lattice", "planted"])
@pytest.mark.parametrize("r", kc.STREAM_ROUTES, ids=kc.route_id)
def test_honest_emulation_passes(r, family):
    _run(r, kc.SMALL_N, family, index_base=1000)
    if family in ("lattice", "planted"):
        _run(r, kc.SMALL_N_CONTROL, family)


@pytest.mark.parametrize("family", ["planted", "negative", "lattice"])
def test_honest_emulation_passes_one_query_tile(family):
    _run(kc.ONE_TILE, kc.ONE_TILE_N, family, index_base=7)


@pytest.mark.parametrize("n", kc.EDGE_N)
@pytest.mark.parametrize("nq", (1, 33, 129))
def test_honest_emulation_passes_edges(nq, n):
    for k in sorted({1, min(8, n), min(9, n), min(16, n)}):
        r = kc.Route(kc.BF16, 128, k, nq, "b128", 0, 0, 0)
        for family in ("lattice", "negative"):
            _run(r, n, family, index_base=5)


def test_families_are_what_they_claim():
    for r in kc.STREAM_ROUTES + [kc.ONE_TILE]:
        n = kc.ONE_TILE_N if r is kc.ONE_TILE else kc.SMALL_N
        nq = min(r.nq, 48)
        for fam in ("gauss", "negative", "scaled", "lattice"):
            q, bank = kc.FAMILIES[fam](nq, n, r.d)
            assert torch.equal(q, q.bfloat16().float()) and torch.equal(bank, bank.bfloat16().float()), fam  # bf16-exact
        q, bank = kc.negative(nq, n, r.d)
        assert float((q.double() @ bank.double().t()).max()) < 0, "negative: a similarity is not below zero"
        q, bank = kc.lattice(nq, n, r.d)
        s64 = q.double() @ bank.double().t()
        acc = np.zeros(s64.shape, dtype=np.float32)  # a float32 chain in feature order
        for c in range(r.d):
            acc = (acc + q[:, c:c + 1].numpy() * bank[:, c].numpy()[None, :]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), s64.numpy()), "lattice: float32 and float64 products differ"
        q, bank = kc.scaled(nq, n, r.d)
        nb = bank.norm(dim=1)
        assert float(nb.max()) > 900 and float(nb.min()) < 1.1e-3


def test_plan_restates_the_documented_schedules():
    # banks above 32 768 rows (65 536 for 64-query tiles) give a slice more than one chunk
    assert kc.plan(128, 32768, 256, 8).iters == 1 and kc.plan(128, 32769, 256, 8).iters == 2
    assert kc.plan(64, 65536, 256, 8).iters == 1 and kc.plan(64, 65537, 256, 8).iters == 2
    p = kc.plan(64, 262235, 256, 8)   # tests/test_gpu_embed.py: 2 049 chunks on 410 slices
    assert (p.qt, p.nslices) == (2, 410)
    p = kc.plan(100, 100003, 512, 8)  # 782 chunks on 196 slices
    assert (p.qt, p.nslices) == (4, 196)
    assert kc.route(kc.F32, 512, 9) == "general" and kc.route(kc.BF16, 768, 5) == "general"
    assert kc.route(kc.F32, 768, 5) == "general" and kc.route(kc.F32, 512, 8) == "stream"


R = {kc.route_id(r): r for r in kc.STREAM_ROUTES}
B128_K8, B128_K16 = R["bf16-d128-k8-b128-QT4-K8-S4"], R["bf16-d128-k16-b128-QT2-K16-S2"]
F32_QT4, F32_K16 = R["f32-d128-k8-stream-QT4-K8-S3"], R["f32-d256-k16-stream-QT2-K16-S3"]
EDGE_RAGGED_Q = kc.Route(kc.BF16, 128, 8, 33, "b128", 0, 0, 0)

# switch -> the cases (route, n, family) that must reject it
CATCHES = {
    "unmasked_tail": [(F32_QT4, kc.SMALL_N, "negative"), (B128_K8, kc.SMALL_N, "planted")],
    "unmasked_query_pad": [(EDGE_RAGGED_Q, 513, "lattice"), (EDGE_RAGGED_Q, 513, "negative")],
    "drop_last_chunk": [(B128_K8, kc.SMALL_N, "planted"), (F32_QT4, kc.SMALL_N, "gauss")],
    "doubled_chunk": [(B128_K8, kc.SMALL_N, "gauss"), (F32_QT4, kc.SMALL_N, "lattice")],
    "tie_by_gid": [(B128_K8, kc.SMALL_N, "planted"), (B128_K16, kc.SMALL_N, "planted"), (kc.ONE_TILE, kc.ONE_TILE_N, "planted"),
                   (F32_QT4, kc.SMALL_N, "lattice")],
    "tie_higher_index": [(B128_K8, kc.SMALL_N, "lattice"), (B128_K8, kc.SMALL_N, "planted")],
    "group_keeps_argmax_only": [(B128_K8, kc.SMALL_N, "planted"), (F32_QT4, kc.SMALL_N, "lattice")],
    "offer_skips_partial_group": [(B128_K8, kc.SMALL_N, "gauss"), (F32_K16, kc.SMALL_N, "negative")],
    "index_base_dropped": [(B128_K8, kc.SMALL_N, "gauss")],
    "k16_as_k8": [(B128_K16, kc.SMALL_N, "planted"), (F32_K16, kc.SMALL_N, "gauss")],
    "stale_ring_stage": [(B128_K16, kc.SMALL_N, "gauss"), (F32_QT4, kc.SMALL_N, "negative"), (B128_K8, kc.SMALL_N, "lattice")],
}


def test_every_switch_has_a_case():
    assert set(CATCHES) == set(kc.SWITCHES)


@pytest.mark.parametrize("switch", kc.SWITCHES)
def test_seeded_error_is_rejected(switch):
    for r, n, family in CATCHES[switch]:
        with pytest.raises(AssertionError):
            _run(r, n, family, index_base=1000, **{switch: True})
        _run(r, n, family, index_base=1000)  # and the same case passes unseeded


def test_tie_at_the_cut_of_the_lists_shows_the_defect():
    """Rows 133 and 517 bit-identical, nslices = 4: row 517 lies in slice 0's second chunk (first chunk 0), row 133 in
    slice 1's first.  Two tied groups both fit the lists of 8, so k = 1 still comes back right; the tie has to sit at
    the cut of the lists: seven better rows in seven other groups, k = 8.  Keyed by (first chunk, wave, half) the eighth
    neighbour is then 517; keyed by the group's best row it is 133."""
    q, bank = kc.gauss(4, 640, 128)
    g = torch.Generator().manual_seed(1)
    w = torch.nn.functional.normalize(q[:1] + 0.09 * torch.randn(1, 128, generator=g), dim=1).bfloat16().float()
    bank[133] = bank[517] = w[0]
    better = [256 + 16 * j for j in range(7)]  # chunk 2: seven (wave, half) sets, seven groups
    bank[better] = q[0]
    assert 0.5 < float(q[0] @ w[0]) < float(q[0] @ q[0])
    pl = kc.Plan(4, 8, 1, 4, 2, 4)
    _, idx = kc.emulate_topk(q, bank, 8, pl, b128=True, tie_by_gid=True)
    assert idx[0].tolist() == better + [517]
    sim, idx = kc.emulate_topk(q, bank, 8, pl, b128=True)
    assert idx[0].tolist() == better + [133]
    kc.check_topk(sim, idx, q, bank, 8, name="tie at the cut")
