"""CPU proofs for tests/vit_cases.py (no GPU): every float64 reference agrees with torch autograd in double, written
independently, and with the project's oracles; every seeded error is rejected by the very criteria and at the very shapes
tests/test_gpu_vit_losses.py and tests/test_gpu_tokens.py use (each test states the family that shows the error); the honest
variants -- the float32 restatement with every sum in the reverse order (loss_cases.other_order), other bf16 rounding events
(kernel_check.jitter), every float32 element moved to a neighbour -- are accepted at every shape and family; and the launch
mirrors give hand-computed values."""
import kernel_check as kc
import loss_cases as lc
import pytest
import torch
import torch.nn.functional as F
import vit_cases as vc
from oracle import ntxent as on
from oracle import vit as ov

F64, F32 = torch.float64, torch.float32
ONE_ULP = 1.0 + 2.0 ** -24          # (a float64 scalar moved by one float32 rounding)


def _ulp(t, seed=0):
    """every element of a float32 tensor moved to its float32 neighbour, up or down at random; an exact 0 stays"""
    g = torch.Generator().manual_seed(seed)
    up = torch.rand(t.shape, generator=g) < 0.5
    out = torch.nextafter(t, torch.where(up, torch.full_like(t, float("inf")), torch.full_like(t, -float("inf"))))
    return torch.where(t == 0, t, out)


def _line(rows):
    return ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)


def _accept32(got, ref, emul, floor, what):
    rows, finite = lc.verdict_f32(got, ref, emul, floor)
    assert finite and all(m <= b for _, m, b in rows), f"honest result rejected -- {what}: {_line(rows)}"


def _reject32(got, ref, emul, floor, what):
    rows, finite = lc.verdict_f32(got, ref, emul, floor)
    print(f"{what}: {_line(rows)}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {_line(rows)}"


def _verdict_bf16(got, ref, emul, floor):
    """loss_cases.check_bf16 without the assertion"""
    return kc.verdict(got, ref, emul, abs_floor=floor, floor_all=floor > 0, floor_cosine=floor > 0)


def _accept16(got, ref, emul, floor, what):
    rows, finite = _verdict_bf16(got, ref, emul, floor)
    assert finite and all(m <= b for _, m, b in rows), f"honest result rejected -- {what}: {_line(rows)}"


def _reject16(got, ref, emul, floor, what):
    rows, finite = _verdict_bf16(got, ref, emul, floor)
    print(f"{what}: {_line(rows)}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {_line(rows)}"


def _scalar_rejected(bad, ref, emul, chain, what):
    got = float(bad["terms"].double().sum())
    print(f"{what}: loss {got:.9g} vs {float(ref['terms'].sum()):.9g}, bound {lc.scalar_bound(ref['terms'], emul['terms'], chain, ref.get('mags')):.3g}")
    assert not (got == got and abs(got) != float("inf")) or not lc.scalar_ok(got, ref["terms"], emul["terms"], chain, ref.get("mags")), \
        f"seeded error accepted -- {what}"


def _scalar_honest(fn_other, ref, emul, chain, what):
    """the yardstick's own sum moved by a rounding, and the reverse-order restatement's sum"""
    for got in (float(emul["terms"].double().sum()) * ONE_ULP, float(lc._sum(fn_other["terms"].reshape(-1), 0))):
        assert lc.scalar_ok(got, ref["terms"], emul["terms"], chain, ref.get("mags")), f"honest scalar rejected -- {what}: {got}"


# ------------------------------------------------------------------------------------------------ launch mirrors
def test_launch_mirrors_give_hand_computed_values():
    assert vc.EW_CAP == 2097152 and vc.DL_MAX_D == 8192
    assert [vc.mse_blocks(n) for n in vc.MSE_SHAPES] == [1, 1, 1024, 1024, 1024]
    assert [vc.mse_sweeps(n) for n in vc.MSE_SHAPES] == [1, 1, 1, 2, 4]      # 3 x 2 097 152 + 8: three full sweeps and one chunk
    assert [vc.mse_chain(n) for n in vc.MSE_SHAPES] == [18, 18, 1041, 1049, 1065]
    assert 2040 // 8 == 255 and vc.mse_blocks(2048) == 1 and vc.mse_blocks(2056) == 2
    assert [vc.row_passes(d) for d in vc.ROW_D] == [1, 1, 1, 2, 4] and vc.row_passes(8200) == 5
    assert vc.dino_chain(3, 5, 2) == 160 + 9 + 6 and vc.memax_chain(2056) == 19 and vc.memax_chain(8) == 11
    assert vc.ew_blocks(1) == 1 and vc.ew_blocks(vc.EW_CAP) == 8192 and vc.ew_sweeps(vc.EW_CAP) == 1
    n, np_, d = vc.TOKEN_SHAPES[-1]
    assert n * (np_ + 1) * (d // 8) == 2155968 and vc.ew_sweeps(2155968) == 2
    assert all(vc.ew_sweeps(a * (b + 1) * (c // 8)) == 1 for a, b, c in vc.TOKEN_SHAPES[:-1])
    n, s, p = vc.PATCHIFY_SHAPES[-1]
    assert n * s * s * 3 // 8 == 2107392 and vc.ew_sweeps(2107392) == 2
    b, s, k, c = vc.ROWS_SHAPES[-1]
    assert b * k * (c // 8) == 2113536 and vc.ew_sweeps(2113536) == 2
    geo = {(1, 8): (1, 1, 1, 64), (63, 384): (48, 1, 1, 64), (64, 384): (48, 1, 1, 64), (65, 384): (48, 1, 2, 64),
           (129, 512): (64, 1, 3, 64), (129, 520): (64, 2, 3, 64), (3, 37 * 384): (64, 28, 1, 64), (25216, 192): (24, 1, 394, 64)}
    assert {s: vc.colsum_geometry(*s) for s in vc.COLSUM_SHAPES} == geo
    assert vc.colsum_row_lanes(384) == (5, 16) and vc.colsum_row_lanes(8) == (256, 0) and vc.colsum_row_lanes(520) == (4, 0)
    assert (520 // 8) % 64 == 1 and (37 * 384 // 8) % 64 == 48          # the last slab: one chunk; 48 of 64 chunks


# ------------------------------------------------------------------------------------------------ MSE / L1
@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
def test_mse_reference_is_autograd(l1):
    pred, target = vc.mse_inputs("randn", 2040, seed=3)
    pr = pred.double().requires_grad_(True)
    loss = (F.l1_loss if l1 else F.mse_loss)(pr, target.double())
    loss.backward()
    ref = vc.mse(pred, target, l1, dt=F64)
    torch.testing.assert_close(ref["dpred"], pr.grad, rtol=1e-12, atol=0)
    torch.testing.assert_close(ref["loss"], loss.detach(), rtol=1e-12, atol=0)
    # at a tie torch's L1 gradient is 0 as well
    a = torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]])
    ar = a.double().requires_grad_(True)
    F.l1_loss(ar, torch.zeros(1, 8, dtype=F64) + a.double() * torch.tensor([1, 0, 1, 0, 1, 1, 1, 1.0])).backward()
    assert torch.equal(vc.mse(a, a * torch.tensor([1, 0, 1, 0, 1, 1, 1, 1.0]), True, dt=F64)["dpred"], ar.grad)


@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
@pytest.mark.parametrize("family", vc.MSE_FAMILIES)
@pytest.mark.parametrize("n", vc.MSE_SHAPES)
def test_mse_honest_accepted_and_seeded_errors_rejected(n, family, l1):
    """dpred is judged by bit equality with the float32 restatement, the scalar by scalar_bound with mse_chain(n).
    mean_over_rows, grad_factor_1: every family and shape (grad_factor_1 is the MSE's alone).  l1_sign_at_zero: the lattice
    family, whose differences tie at 0 (L1 alone).  sweep_tail_dropped: by dpred in every family from n = 2 097 160 on (nothing
    lies behind the first sweep below that), by the scalar at 3 x 2 097 152 + 8 (two thirds of the sum)."""
    (pred, target), ref, emul = vc.mse_case(family, n, l1)
    chain = vc.mse_chain(n)
    with lc.other_order():
        other = vc.mse(pred, target, l1, dt=F32)
    assert torch.equal(other["dpred"], emul["dpred"])                  # (no sum enters dpred: any order gives these bits)
    _scalar_honest(other, ref, emul, chain, f"{family} n={n}")
    errors = ["mean_over_rows"] + ([] if l1 else ["grad_factor_1"])
    if l1 and family == "lattice":
        assert bool((pred == target).any())
        errors.append("l1_sign_at_zero")
    if vc.mse_sweeps(n) > 1:
        errors.append("sweep_tail_dropped")
    for error in errors:
        bad = vc.mse(pred, target, l1, dt=F32, seed_error=error)
        assert not torch.equal(bad["dpred"], emul["dpred"]), f"{error} accepted by dpred ({family}, n={n})"
        if error not in ("grad_factor_1", "l1_sign_at_zero"):          # (these two leave the scalar alone)
            if error == "sweep_tail_dropped" and n == vc.EW_CAP + 8:
                continue       # (ONE chunk of 262 145 is 4e-6 of the sum, inside the bound of a chain of 1049: dpred shows it)
            _scalar_rejected(bad, ref, emul, chain, f"{error} {family} n={n}")


# ------------------------------------------------------------------------------------------------ DINO / soft CE
def _autograd_dino(student, probs, vs, vt, b, temp, skip):
    x = student.double().reshape(vs, b, -1).requires_grad_(True)
    p = probs.double().reshape(vt, b, -1)
    ls = F.log_softmax(x / float(torch.tensor(temp, dtype=F32)), -1)
    total, n_terms = 0.0, 0
    for s in range(vs):
        for t in range(vt):
            if skip and s == t:
                continue
            total = total - (p[t] * ls[s]).sum(-1).mean()
            n_terms += 1
    loss = total / n_terms
    loss.backward()
    return loss.detach(), x.grad.reshape(vs * b, -1)


@pytest.mark.parametrize("vs,vt,b", vc.DINO_VIEWS)
def test_dino_reference_is_autograd_and_oracle(vs, vt, b):
    d = 2040
    i, ref, _ = vc.dino_case("randn", vs, vt, b, d, 0.04)
    # (autograd differentiates sum_d p_d as it is; the formula takes it as 1, which the float32 probs are to 1e-8 only: the
    # comparison feeds both the float64 probabilities)
    p64 = vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F64)
    ref = vc.dino_loss(i["student"], p64, vs, vt, b, vc.STUDENT_TEMP, 1, dt=F64)
    loss, grad = _autograd_dino(i["student"], p64, vs, vt, b, vc.STUDENT_TEMP, True)
    torch.testing.assert_close(ref["terms"].sum(), loss, rtol=1e-12, atol=0)
    torch.testing.assert_close(ref["dstudent"], grad, rtol=1e-9, atol=1e-18)
    # the project's oracle (float32, from the teacher logits): teacher probabilities and loss together
    o_loss, _ = ov.dino_loss(list(i["teacher"].reshape(vt, b, d)), list(i["student"].reshape(vs, b, d)), i["center"].reshape(1, 1, d), 0.04, 0.1)
    torch.testing.assert_close(o_loss.double(), ref["terms"].sum(), rtol=2e-5, atol=0)      # (the oracle's float32)
    probs = vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F64)
    t = float(torch.tensor(0.04, dtype=F32))
    torch.testing.assert_close(probs, torch.softmax((i["teacher"].double() - i["center"].double()) / t, -1), rtol=1e-12, atol=1e-300)


def test_soft_ce_and_memax_references_are_autograd_and_the_msn_oracle():
    """soft cross-entropy (Vt = 1, no skip) + the mean-entropy regulariser = oracle.ntxent.msn_loss without Sinkhorn and
    sharpening; each piece against autograd in double, the KL-to-prior form as well"""
    views, b, k, dim = 3, 7, 1024, 32
    g = torch.Generator().manual_seed(11)
    anchors, targets, protos = (torch.randn(r, dim, generator=g, dtype=F64) for r in (views * b, b, k))
    logits = F.normalize(anchors, dim=1) @ F.normalize(protos, dim=1).t()
    tp = torch.softmax(F.normalize(targets, dim=1) @ F.normalize(protos, dim=1).t() / 0.1, 1)
    ce = vc.dino_loss(logits, tp, views, 1, b, 0.1, 0, dt=F64)
    me = vc.mean_entropy_reg(logits, None, 0.1, dt=F64)
    t32 = float(torch.tensor(0.1, dtype=F32))
    for power in (None, 0.25):
        lp = None
        if power is not None:
            prior = 1.0 / torch.arange(1, k + 1, dtype=F64) ** power
            lp = (prior / prior.sum()).log()
        me = vc.mean_entropy_reg(logits, lp, 0.1, dt=F64)
        want = on.msn_loss(anchors, targets, protos, temperature=t32, sinkhorn_iterations=0, target_sharpen_temperature=1.0,
                           power_law_exponent=power)
        torch.testing.assert_close(ce["terms"].sum() + me["terms"].sum(), want, rtol=1e-6, atol=0)   # (the prior is cast through m's dtype)
        x = logits.clone().requires_grad_(True)
        p = torch.softmax(x / t32, 1)
        m = p.mean(0)
        reg = (m * (m.log() - (0.0 if lp is None else lp))).sum()
        reg.backward()
        torch.testing.assert_close(me["terms"].sum(), reg.detach(), rtol=1e-12, atol=0)
        torch.testing.assert_close(me["dlogits"], x.grad, rtol=1e-9, atol=1e-18)
        torch.testing.assert_close(me["m"], m.detach(), rtol=1e-12, atol=0)
    x = logits.clone().requires_grad_(True)
    loss = -(tp.repeat(views, 1) * F.log_softmax(x / t32, 1)).sum(1).mean()
    loss.backward()
    torch.testing.assert_close(ce["terms"].sum(), loss.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(ce["dstudent"], x.grad, rtol=1e-9, atol=1e-18)


def _dino_floor(family, ref):
    return vc.softmax_floor(family, ref)


def _dino_honest(i, vs, vt, b, skip):
    args = (i["student"], i["probs"], vs, vt, b, vc.STUDENT_TEMP, skip)
    with lc.other_order(), kc.jitter(vs + vt + b):
        return vc.dino_loss(*args, dt=F32)


@pytest.mark.parametrize("d", vc.ROW_D)
@pytest.mark.parametrize("vs,vt,b", vc.DINO_VIEWS)
def test_dino_shapes_honest_accepted_and_seeded_errors_rejected(vs, vt, b, d):
    """randn at every row width and view geometry.  count_diag, no_skip, grad_without_temp: rejected here (count_diag and
    no_skip by dstudent and by the scalar).  nt_is_vt: wherever a student view meets fewer than Vt teachers (s < min(Vs, Vt)).
    tail_chunk_dropped: by the scalar from D = 2056 on (one pass holds 2048 elements)."""
    i, ref, emul = vc.dino_case("randn", vs, vt, b, d, 0.04)
    chain = vc.dino_chain(vs, vt, b)
    hon = _dino_honest(i, vs, vt, b, 1)
    _accept16(hon["dstudent"], ref["dstudent"], emul["dstudent"], 0.0, f"dino dstudent {vs, vt, b, d}")
    _scalar_honest(hon, ref, emul, chain, f"dino {vs, vt, b, d}")
    args = (i["student"], i["probs"], vs, vt, b, vc.STUDENT_TEMP, 1)
    for error in ("count_diag", "no_skip", "grad_without_temp", "nt_is_vt"):
        bad = vc.dino_loss(*args, dt=F32, seed_error=error)
        _reject16(bad["dstudent"], ref["dstudent"], emul["dstudent"], 0.0, f"{error} dstudent {vs, vt, b, d}")
        if error in ("count_diag", "no_skip"):
            _scalar_rejected(bad, ref, emul, chain, f"{error} {vs, vt, b, d}")
    probs_ref = vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F64)
    probs_emul = vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F32)
    with lc.other_order():
        _accept32(_ulp(vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F32)), probs_ref, probs_emul, lc.f32_floor(probs_ref),
                  f"probs {vs, vt, b, d}")
    if vc.row_passes(d) > 1:
        bad = vc.dino_loss(*args, dt=F32, seed_error="tail_chunk_dropped")
        _scalar_rejected(bad, ref, emul, chain, f"tail_chunk_dropped {vs, vt, b, d}")
        _reject32(vc.dino_teacher_probs(i["teacher"], i["center"], 0.04, dt=F32, seed_error="tail_chunk_dropped"), probs_ref, probs_emul,
                  lc.f32_floor(probs_ref), f"tail_chunk_dropped probs D={d}")


@pytest.mark.parametrize("family", vc.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("temp_t", vc.TEACHER_TEMPS)
@pytest.mark.parametrize("d,views", vc.DINO_FAMILY_SHAPES)
def test_dino_families_honest_accepted_and_seeded_errors_rejected(family, temp_t, d, views):
    """every family.  no_max: rejected in `offset` alone (x / T = 300 overflows expf; elsewhere |x / T| stays below 88).
    center_ignored, probs_unnormalised: the teacher probabilities of `randn` and `offset` (a constant centre shifts nothing, and a
    near one-hot row is 1 at its maximum with or without the centre and the division)."""
    vs, vt, b = views
    i, ref, emul = vc.dino_case(family, vs, vt, b, d, temp_t)
    chain = vc.dino_chain(vs, vt, b)
    floor = _dino_floor(family, ref)
    hon = _dino_honest(i, vs, vt, b, 1)
    _accept16(hon["dstudent"], ref["dstudent"], emul["dstudent"], floor, f"dino dstudent {family} T={temp_t} D={d}")
    _scalar_honest(hon, ref, emul, chain, f"dino {family} T={temp_t} D={d}")
    args = (i["student"], i["probs"], vs, vt, b, vc.STUDENT_TEMP, 1)
    if family == "offset":
        bad = vc.dino_loss(*args, dt=F32, seed_error="no_max")
        _reject16(bad["dstudent"], ref["dstudent"], emul["dstudent"], floor, f"no_max dstudent {family}")
        _scalar_rejected(bad, ref, emul, chain, f"no_max {family}")
    # the teacher probabilities of the same inputs
    pr, pe = (vc.dino_teacher_probs(i["teacher"], i["center"], temp_t, dt=dt) for dt in (F64, F32))
    pfloor = lc.f32_floor(pr)
    with lc.other_order():
        _accept32(_ulp(vc.dino_teacher_probs(i["teacher"], i["center"], temp_t, dt=F32)), pr, pe, pfloor, f"probs {family} T={temp_t} D={d}")
    if family in ("randn", "offset"):
        for error in ("center_ignored", "probs_unnormalised"):
            _reject32(vc.dino_teacher_probs(i["teacher"], i["center"], temp_t, dt=F32, seed_error=error), pr, pe, pfloor, f"{error} {family} D={d}")


@pytest.mark.parametrize("views,b", vc.SOFT_CE_VIEWS)
@pytest.mark.parametrize("d", vc.ROW_D)
def test_soft_ce_honest_accepted_and_seeded_errors_rejected(views, b, d):
    """Vt = 1, nothing skipped: grad_without_temp by dstudent, tail_chunk_dropped by the scalar from D = 2056 on; count_diag,
    no_skip and nt_is_vt compute the same thing here (asserted)."""
    i, ref, emul = vc.dino_case("randn", views, 1, b, d, 0.07, 0)
    chain = vc.dino_chain(views, 1, b)
    hon = _dino_honest(i, views, 1, b, 0)
    _accept16(hon["dstudent"], ref["dstudent"], emul["dstudent"], 0.0, f"soft CE dstudent {views, b, d}")
    _scalar_honest(hon, ref, emul, chain, f"soft CE {views, b, d}")
    args = (i["student"], i["probs"], views, 1, b, vc.STUDENT_TEMP, 0)
    for error in ("count_diag", "no_skip", "nt_is_vt"):
        assert torch.equal(vc.dino_loss(*args, dt=F32, seed_error=error)["dstudent"], emul["dstudent"])
    _reject16(vc.dino_loss(*args, dt=F32, seed_error="grad_without_temp")["dstudent"], ref["dstudent"], emul["dstudent"], 0.0, "grad_without_temp")
    if vc.row_passes(d) > 1:
        _scalar_rejected(vc.dino_loss(*args, dt=F32, seed_error="tail_chunk_dropped"), ref, emul, chain, f"tail_chunk_dropped D={d}")


def test_dino_without_terms_is_an_error():
    with pytest.raises(ValueError):
        vc.dino_loss(torch.zeros(3, 8), torch.zeros(3, 8), 1, 1, 3, 0.1, 1)


# ------------------------------------------------------------------------------------------------ me-max
@pytest.mark.parametrize("prior", [False, True], ids=["memax", "prior"])
@pytest.mark.parametrize("family", vc.MEMAX_FAMILIES)
@pytest.mark.parametrize("k", vc.MEMAX_K)
@pytest.mark.parametrize("n", vc.MEMAX_N)
def test_memax_honest_accepted_and_seeded_errors_rejected(n, k, family, prior):
    """prior_ignored: with a prior, by the scalar in every family and by dlogits in randn / offset / underflow at N > 1.  mean_is_sum: by m,
    N > 1.  grad_without_temp: by dlogits in randn / offset / underflow (constant rows have no gradient: u - <p, u> = 0).
    scalar_from_row_sum: by the scalar, N > 1 (at N = 1 all three are the same computation)."""
    (x, lp), ref, emul = vc.memax_case(family, n, k, prior)
    chain = vc.memax_chain(k)
    if family == "underflow":
        assert float(emul["m"][k // 2]) == 0.0 and float(ref["m"][k // 2]) < vc.MEMAX_CLAMP
    with lc.other_order():
        other = vc.mean_entropy_reg(x, lp, vc.MEMAX_TEMP, dt=F32)
    _accept32(_ulp(other["m"]), ref["m"], emul["m"], ref["m_floor"], f"m {family} {n}x{k}")
    _accept32(_ulp(other["dlogits"], 1), ref["dlogits"], emul["dlogits"], ref["floor"], f"dlogits {family} {n}x{k}")
    _scalar_honest(other, ref, emul, chain, f"memax {family} {n}x{k}")
    live = family != "constant"

    def bad(error):
        return vc.mean_entropy_reg(x, lp, vc.MEMAX_TEMP, dt=F32, seed_error=error)

    if prior:
        _scalar_rejected(bad("prior_ignored"), ref, emul, chain, f"prior_ignored {family} {n}x{k}")
        if live and n > 1:       # (one row at T = 0.1 is nearly one-hot: its whole gradient is a cancellation, prior or not)
            _reject32(bad("prior_ignored")["dlogits"], ref["dlogits"], emul["dlogits"], ref["floor"], f"prior_ignored dlogits {family}")
    if live:
        _reject32(bad("grad_without_temp")["dlogits"], ref["dlogits"], emul["dlogits"], ref["floor"], f"grad_without_temp {family} {n}x{k}")
    if n > 1:
        _reject32(bad("mean_is_sum")["m"], ref["m"], emul["m"], ref["m_floor"], f"mean_is_sum {family} {n}x{k}")
        _scalar_rejected(bad("scalar_from_row_sum"), ref, emul, chain, f"scalar_from_row_sum {family} {n}x{k}")
    else:
        for error in ("mean_is_sum", "scalar_from_row_sum"):
            assert torch.equal(bad(error)["terms"], emul["terms"])


# ------------------------------------------------------------------------------------------------ tokens and permutations
@pytest.mark.parametrize("n,np_,d", vc.TOKEN_SHAPES[:3])
def test_tokens_reference_and_seeded_errors(n, np_, d):
    """bit equality with float32-add-then-bf16.  pos_shift, cls_without_pos: every shape.  patch_rows_transposed: N > 1 and
    np > 1 (a transposition of one row or one column moves nothing: asserted)."""
    patches, cls, pos = vc.tokens_inputs(n, np_, d, seed=n + np_)
    emul = vc.tokens_assemble(patches, cls, pos, n, np_, dt=F32)
    want = torch.cat([(cls + pos[0]).expand(n, 1, d), patches.reshape(n, np_, d) + pos[1:]], 1).bfloat16().float().reshape(-1, d)
    assert torch.equal(emul, want)
    torch.testing.assert_close(vc.tokens_assemble(patches, cls, pos, n, np_, dt=F64), want.double(), rtol=2.0 ** -8, atol=0)
    for error in ("pos_shift", "cls_without_pos", "patch_rows_transposed"):
        bad = vc.tokens_assemble(patches, cls, pos, n, np_, dt=F32, seed_error=error)
        if error == "patch_rows_transposed" and (n == 1 or np_ == 1):
            assert torch.equal(bad, emul)
        else:
            assert not torch.equal(bad, emul), error


def test_patchify_reference_is_the_einsum():
    img = torch.arange(3 * 32 * 32 * 3, dtype=torch.float32).reshape(3, 32, 32, 3)
    for p in (8, 16, 32):
        g = 32 // p
        want = torch.einsum("nhpwqc->nhwpqc", img.reshape(3, g, p, g, p, 3)).reshape(3 * g * g, p, p, 3)
        assert torch.equal(vc.patchify(img, p), want)
    assert torch.equal(vc.patchify(img, 8)[1 * 16 + 2 * 4 + 3, 5, 6], img[1, 2 * 8 + 5, 3 * 8 + 6])


@pytest.mark.parametrize("b,s,k,c", vc.ROWS_SHAPES[:3])
@pytest.mark.parametrize("hostile", [False, True])
def test_rows_by_index_reference_and_seeded_errors(b, s, k, c, hostile):
    """gather_batch_stride_k: B > 1 and K != S.  scatter_as_gather: every shape with S > 1.  Skipped indices leave the prefilled
    pattern untouched."""
    idx = vc.index_inputs(b, s, k, seed=b + s, hostile=hostile)
    g = torch.Generator().manual_seed(1)
    big, small = torch.randn(b * s, c, generator=g), torch.randn(b * k, c, generator=g)
    pat_small, pat_big = torch.full((b * k, c), -3.0), torch.full((b * s, c), -3.0)
    got = vc.rows_by_index(big, idx, b, s, k, pat_small)
    sc = vc.rows_by_index(small, idx, b, s, k, pat_big, scatter=True)
    for bi in range(b):
        for j in range(k):
            t = int(idx[bi, j])
            if 0 <= t < s:
                assert torch.equal(got[bi * k + j], big[bi * s + t]) and torch.equal(sc[bi * s + t], small[bi * k + j])
            else:
                assert bool((got[bi * k + j] == -3.0).all())
    valid = ((idx >= 0) & (idx < s)).sum()
    assert int((sc != -3.0).all(1).sum()) == int(valid)
    if b > 1 and k != s:
        assert not torch.equal(vc.rows_by_index(big, idx, b, s, k, pat_small, seed_error="gather_batch_stride_k"), got)
    if s > 1 and int(valid) > 0:
        assert not torch.equal(vc.rows_by_index(small, idx, b, s, k, pat_big, scatter=True, seed_error="scatter_as_gather")[:b * k], sc[:b * k])


@pytest.mark.parametrize("s", vc.ARGSORT_S)
@pytest.mark.parametrize("kind", vc.ARGSORT_KEYS)
def test_argsort_reference_and_seeded_errors(s, kind):
    """argsort_ties_high: the families with ties (equal, two_values, signed_zero, inf), S > 1.  argsort_descending: the families
    with two different keys, S > 1 (all-equal and the signed zeros are one value)."""
    keys = vc.argsort_inputs(kind, 3, s, seed=s)
    want = vc.argsort_rows(keys)
    for r in range(3):
        pairs = sorted((float(keys[r, j]) + 0.0, j) for j in range(s))
        assert [j for _, j in pairs] == want[r].tolist()
    if s > 2:
        if kind != "uniform":
            assert not torch.equal(vc.argsort_rows(keys, "argsort_ties_high"), want)
        if kind in ("uniform", "two_values", "inf"):
            assert not torch.equal(vc.argsort_rows(keys, "argsort_descending"), want)
        else:
            assert torch.equal(vc.argsort_rows(keys, "argsort_descending"), want)


# ------------------------------------------------------------------------------------------------ column sums, matmul
@pytest.mark.parametrize("family", vc.COLSUM_FAMILIES)
@pytest.mark.parametrize("rows,c", vc.COLSUM_SHAPES)
def test_colsum_honest_accepted_and_seeded_errors_rejected(rows, c, family):
    """lattice: bit equality (integer sums are exact in any order).  rows-1: every shape (a single row leaves 0).
    last_block_dropped: every shape.  slab_tail_dropped: C = 520 and C = 37 x 384, the shapes with a partial slab."""
    x, ref, emul = vc.colsum_case(family, rows, c)
    torch.testing.assert_close(ref["out"], x.double().sum(0), rtol=1e-13, atol=1e-11)
    with lc.other_order():
        other = vc.colsum(x, dt=F32)
    errors = ["rows-1", "last_block_dropped"] + (["slab_tail_dropped"] if (c >> 3) % vc.colsum_geometry(rows, c)[0] else [])
    assert ("slab_tail_dropped" in errors) == (c in (520, 37 * 384))
    for key in ("part", "out"):
        floor = ref[key + "_floor"]
        if family == "lattice":
            assert torch.equal(other[key].double(), ref[key]) and torch.equal(emul[key].double(), ref[key])
        else:
            _accept32(_ulp(other[key]), ref[key], emul[key], floor, f"colsum {key} {family} {rows}x{c}")
        for error in errors:
            bad = vc.colsum(x, dt=F32, seed_error=error)[key]
            if family == "lattice":
                assert not torch.equal(bad.double(), ref[key]), error
            else:
                _reject32(bad, ref[key], emul[key], floor, f"{error} {key} {family} {rows}x{c}")


@pytest.mark.parametrize("m,k,n", vc.MATMUL_SHAPES)
def test_matmul_restatement_against_float64(m, k, n):
    a, b = vc.matmul_inputs(m, k, n, seed=m + k + n)
    got = lc.fma_matmul_f32(a, b)
    ref = a.double() @ b.double()
    _accept32(got, ref, got, lc.mag_floor(a.double().abs() @ b.double().abs()), f"matmul {m, k, n}")
    assert float((got.double() - ref).abs().max()) <= k * lc.U * float((a.double().abs() @ b.double().abs()).max())
