"""CPU proofs for tests/update_cases.py: (1) the float64 references are torch.optim.SGD / AdamW / Adam, oracle.resnet.lars_step and
sklearn's StandardScaler; (2) another honest float32 realisation of every kernel -- the emulation with its rounding events moved
(kernel_check.jitter) and without fma contraction (f32_cases.uncontracted) -- passes the bounds tests/test_gpu_update_kernels.py
asserts, on the families and sizes it runs; (3) every seeded error is rejected under those bounds on a named combination that file
runs, or shown equivalent."""
import f32_cases as fc
import kernel_check as kc
import numpy as np
import pytest
import torch
import update_cases as uc

SUM = kc.F32_SUM_FACTOR
BIG = {"sgd": uc.SGD_CAP + 77, "adamw": uc.EW_CAP + 77, "adam": uc.EW_CAP + 77}


def ok(got, ref, emul, factor=kc.FACTOR, **kw):
    return fc.verdict32(got, ref, emul, factor, **kw)


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------ (1) the references
@pytest.mark.parametrize("kind", ["sgd", "adamw", "adam"])
@pytest.mark.parametrize("hset", ["own", "visible"])
def test_step_reference_is_torch_optim_over_five_steps(kind, hset):
    """the per-step reference (state handed in, one step) chained five times against ONE torch.optim object stepping five times"""
    h = dict(uc.HYPER[kind][hset])
    gs = h.pop("grad_scale")
    cls = {"sgd": torch.optim.SGD, "adamw": torch.optim.AdamW, "adam": torch.optim.Adam}[kind]
    x = uc.step_inputs("randn", 257, 11)
    q = torch.nn.Parameter(x["p"].double().clone())
    opt = cls([q], **h)
    grads = [torch.randn(257, generator=torch.Generator().manual_seed(s)) for s in range(5)]
    ps, _, _ = uc.chain(kind, [x["p"]], [[g] for g in grads], [dict(h, grad_scale=gs)] * 5, emulate=False)
    for g in grads:
        q.grad = g.double() * gs
        opt.step()
    assert rel(ps[0], q.detach()) <= 1e-13


def test_lars_reference_is_the_oracle_in_float64():
    from oracle import resnet as orn

    for hset in ("barlow", "vicreg", "visible", "wd0"):
        h = uc.HYPER["lars"][hset]
        a = uc.lars_arena(5, "fresh")
        segs = uc.lars_segments(a["seg"])
        p, mom = a["p"].double(), a["mom"].double()
        ref = {str(i): p[b:e].clone() for i, (b, e) in enumerate(segs)}
        bufs = {}
        for step in range(5):
            g = torch.randn(p.numel(), generator=torch.Generator().manual_seed(step)).double()
            g[segs[2][0]:segs[2][1]] = 0.0
            p, mom, _ = uc.lars_ref(p, g, mom, a["seg"], **h)
            orn.lars_step(ref, {str(i): g[b:e] * h["grad_scale"] for i, (b, e) in enumerate(segs)}, bufs, h["lr"], h["momentum"],
                          h["weight_decay"], h["trust_coeff"], h["eps"])
        for i, (b, e) in enumerate(segs):
            assert rel(p[b:e], ref[str(i)]) <= 1e-13 and rel(mom[b:e], bufs[str(i)]) <= 1e-13, (hset, i)


def test_lars_without_weight_decay_is_plain_momentum_sgd():
    a = uc.lars_arena(2, "warm")
    h = uc.HYPER["lars"]["wd0"]
    p, mom, _ = uc.lars_ref(a["p"], a["g"], a["mom"], a["seg"], **h)
    for b, e in uc.lars_segments(a["seg"]):
        q, mo = uc.sgd_ref(a["p"][b:e], a["g"][b:e], a["mom"][b:e], h["lr"], h["momentum"], 0.0, h["grad_scale"])
        assert rel(p[b:e], q) <= 1e-13 and rel(mom[b:e], mo) <= 1e-13


@pytest.mark.parametrize("family", ["randn", "big_mean", "constant_column"])
def test_scaler_reference_is_sklearn(family):
    from sklearn.preprocessing import StandardScaler

    x = uc.col_inputs(family, 513, 33, 3)
    sk = StandardScaler().fit(x.double().numpy())
    r = uc.scaler_ref(x, x)
    np.testing.assert_allclose(r["mean"].numpy(), sk.mean_, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["var"].numpy(), sk.var_, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(r["scale"].numpy(), sk.scale_, rtol=1e-12)
    np.testing.assert_allclose(r["y"].numpy(), sk.transform(x.double().numpy()), rtol=1e-12, atol=1e-11)
    if family == "constant_column":
        assert (r["scale"][0::2] == 1).all() and (r["var"][0::2] == 0).all()


def test_bf16_rounding_is_torchs():
    x = uc.cast_specials()
    assert uc.same_bf16(uc.bf16_bits(x), uc.torch_bf16_bits(x))
    y = uc.bf16_specials(65536)
    for s in (1.0, 0.25, 1.0 / 3.0, 3.0e38):
        want = uc.torch_bf16_bits(y * torch.tensor(s, dtype=torch.float32))
        assert uc.same_bf16(uc.scale_bf16_bits(y, s), want)


def test_lattice_steps_are_exact_in_float32():
    """with the lattice inputs and hyper-parameters the emulation IS the reference: the GPU tests may ask equality there"""
    for kind in ("sgd", "adamw", "adam"):
        for state in ("fresh", "warm") if kind == "sgd" else ("fresh",):
            x = uc.step_inputs("lattice", 257, 4, state)
            h = uc.HYPER[kind]["lattice"]
            r, e = uc.step_outputs(kind, x, h), uc.step_outputs(kind, x, h, emulate=True)
            assert all(torch.equal(r[k], e[k]) for k in r), (kind, state)
            assert all(torch.equal(r[k], r[k].float().double()) for k in r)
    ema, p = uc.step_inputs("lattice", 257, 5)["p"], uc.step_inputs("lattice", 257, 6)["p"]
    assert torch.equal(uc.ema_emul(ema, p, 0.5), uc.ema_ref(ema, p, 0.5))
    x = uc.col_inputs("lattice", 64, 33, 1)
    (m, v), (me, ve) = uc.colstats_ref(x), uc.colstats_emul(x)
    assert torch.equal(m, me) and torch.equal(v, ve)
    c0 = uc.col_inputs("lattice", 1, 33, 2)[0]
    assert torch.equal(uc.center_emul(x, c0, 0.5), uc.center_ref(x, c0, 0.5))
    g = 2.0 ** torch.randint(-2, 3, (33,)).float()
    dy = uc.col_inputs("lattice", 64, 33, 3)
    assert all(torch.equal(a, b) for a, b in zip(uc.colscale_emul(x, g, dy, g), uc.colscale_ref(x, g, dy, g)))


# ------------------------------------------------------------------------------------------------ (2) honest realisations pass
def _honest(f):
    """the two other realisations: rounding events moved, and a * b + c rounded twice"""
    with kc.jitter(7):
        a = f()
    with fc.uncontracted():
        b = f()
    return a, b


STEP_CASES = [(kind, fam, hset, state, n, 1) for kind in ("sgd", "adamw", "adam") for fam, hset in (("randn", "own"), ("randn", "visible"))
              for state in ("fresh", "warm") for n in uc.ELEMENT_SIZES] + \
             [(kind, "randn", hset, "warm", BIG[kind], 1) for kind in ("sgd", "adamw", "adam") for hset in ("own", "visible")] + \
             [(kind, "tiny_grad", hset, state, 257, t) for kind in ("adamw", "adam") for hset in ("own", "visible")
              for state in ("fresh", "warm") for t in (1, 2, 1000)]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_honest_steps_pass(case):
    kind, fam, hset, state, n, t = case
    x, h = uc.step_inputs(fam, n, n + t, state), uc.HYPER[kind][hset]
    ref, em = uc.step_outputs(kind, x, h, t), uc.step_outputs(kind, x, h, t, emulate=True)
    for other in _honest(lambda: uc.step_outputs(kind, x, h, t, emulate=True)):
        for k in uc.STEP_TENSORS[kind]:
            assert ok(other[k], ref[k], em[k], **uc.step_floor(k, ref)), (case, k)


@pytest.mark.parametrize("m", [0.99, 0.996, 0.0, 1.0 - 0.1])
def test_honest_ema_passes(m):
    for n in uc.ELEMENT_SIZES + (uc.EW_CAP + 77,):
        x = uc.step_inputs("randn", n, n, "warm")
        ref, em = uc.ema_ref(x["p"], x["g"], m), uc.ema_emul(x["p"], x["g"], m)
        for other in _honest(lambda: uc.ema_emul(x["p"], x["g"], m)):
            assert ok(other, ref, em, abs_floor=fc.elem_floor(ref), floor_all=True), (m, n)
    x = uc.step_inputs("randn", 257, 1)
    assert torch.equal(uc.ema_emul(x["p"], x["g"], 0.0), x["g"].double())        # m = 0: a copy


def lars_ok(got, ref, em, a, h):
    """the comparison of the GPU test, per segment: p, the momentum buffer and the update with F32_SUM_FACTOR (they inherit the
    float32 norms' summation noise through the ratio), the squared norms of all segments relative to their float64 values with
    f32_sum_floor in that form (update_cases.lars_rel_norms).  -> the (segment, tensor) that fail; the norms as segment -1"""
    bad = []
    for s, (b, e) in enumerate(uc.lars_segments(a["seg"])):
        for k in ("p", "m", "update"):
            if not ok(got[k][b:e], ref[k][b:e], em[k][b:e], SUM, **uc.lars_step_floor(k, a, h, ref, b, e)):
                bad.append((s, k))
    (gn, nz), (en, _) = uc.lars_rel_norms(got, ref), uc.lars_rel_norms(em, ref)
    if not (bool((got["norms"][~nz] == 0).all()) and ok(gn, torch.ones_like(gn), en, SUM, abs_floor=uc.LARS_NORM_FLOOR, floor_all=True)):
        bad.append((-1, "norms"))
    return bad


@pytest.mark.parametrize("hset", list(uc.HYPER["lars"]))
@pytest.mark.parametrize("state,rot", [("fresh", 0), ("warm", 3)])
def test_honest_lars_passes(hset, state, rot):
    a, h = uc.lars_arena(9, state, rot), uc.HYPER["lars"][hset]
    ref, em = uc.lars_outputs(a, h), uc.lars_outputs(a, h, emulate=True)
    for other in _honest(lambda: uc.lars_outputs(a, h, emulate=True)):
        assert lars_ok(other, ref, em, a, h) == []


def test_honest_lars_passes_in_any_order_of_the_atomics():
    """the blocks' partial norms arrive in an order that changes from run to run: twenty random orders of the honest emulation pass
    the comparison of the GPU test"""
    for hset, state, rot in (("vicreg", "warm", 3), ("barlow", "fresh", 0)):
        a, h = uc.lars_arena(9, state, rot), uc.HYPER["lars"][hset]
        ref, em = uc.lars_outputs(a, h), uc.lars_outputs(a, h, emulate=True)
        for seed in range(20):
            with uc.atomics_shuffled(seed):
                other = uc.lars_outputs(a, h, emulate=True)
            assert lars_ok(other, ref, em, a, h) == [], (hset, seed)


COL_SMALL = [(rows, c) for rows in uc.COL_ROWS[:-1] for c in (1, 33)] + [(513, 512), (16385, 31), (16385, 32)]


@pytest.mark.parametrize("family", ["randn", "big_mean", "constant_column"])
def test_honest_column_statistics_pass(family):
    for rows, c in COL_SMALL:
        x = uc.col_inputs(family, rows, c, rows + c)
        (mr, vr), (me, ve) = uc.colstats_ref(x), uc.colstats_emul(x)
        sr, se = uc.scaler_ref(x, x), uc.scaler_emul(x, x)
        with kc.jitter(3):
            mo, vo = uc.colstats_emul(x)
            so = uc.scaler_emul(x, x)
        assert ok(mo, mr, me, SUM, abs_floor=uc.mean_floor(x), floor_all=True, floor_cosine=True), (rows, c)
        assert ok(vo, vr, ve, SUM, abs_floor=uc.var_floor(x), floor_all=True, floor_cosine=True), (rows, c)
        assert torch.equal(so["scale"] == 1, sr["scale"] == 1)
        assert ok(so["y"], sr["y"], se["y"], SUM, abs_floor=uc.scaled_floor(x, sr), floor_all=True, floor_cosine=True), (rows, c)


def test_honest_small_kernels_pass():
    for rows in uc.CENTER_ROWS:
        for d in (8, 33):
            t, c0 = uc.col_inputs("randn", rows, d, rows, bf16=True), uc.col_inputs("randn", 1, d, 5)[0]
            for m in (0.9, 0.0):
                ref, em = uc.center_ref(t, c0, m), uc.center_emul(t, c0, m)
                for other in _honest(lambda: uc.center_emul(t, c0, m)):
                    assert ok(other, ref, em, SUM, abs_floor=kc.f32_stat_floor(t, c0), floor_all=True)
    for rows in uc.COLSCALE_ROWS:
        x, dy = uc.col_inputs("randn", rows, 33, rows, bf16=True), uc.col_inputs("randn", rows, 33, rows + 1, bf16=True)
        g, dg0 = uc.col_inputs("randn", 1, 33, 7)[0], uc.col_inputs("randn", 1, 33, 8)[0]
        ref, em = uc.colscale_ref(x, g, dy, dg0), uc.colscale_emul(x, g, dy, dg0)
        with kc.jitter(5):
            other = uc.colscale_emul(x, g, dy, dg0)
        assert kc.passes(other[0], ref[0], em[0]) and kc.passes(other[1], ref[1], em[1])
        assert ok(other[2], ref[2], em[2], SUM, abs_floor=uc.colscale_dg_floor(x, dy, dg0))
    for n in uc.MEAN_N:
        x = torch.rand(n, generator=torch.Generator().manual_seed(n)) + 0.1
        for sq in (False, True):
            ref, em = uc.mean_ref(x, 0.7, sq), uc.mean_emul(x, 0.7, sq)
            with kc.jitter(5):
                other = uc.mean_emul(x, 0.7, sq)
            assert ok(other, ref, em, SUM, abs_floor=uc.mean_f32_floor(x, 0.7, sq), floor_all=True)


# ------------------------------------------------------------------------------------------------ (3) seeded errors
# (kernel, switch) -> the combination of tests/test_gpu_update_kernels.py that rejects it and the tensor that does.
# step combinations: (kind, family, hyper set, state, n, t); LARS: (hyper set, state, rot).
CATCHES = {
    ("sgd", "wd_dropped"): (("sgd", "randn", "own", "warm", 257, 1), "m"),
    # grad_scale = 1 in "own": the order of scaling and decay cannot matter there
    ("sgd", "grad_scale_after_wd"): (("sgd", "randn", "visible", "warm", 257, 1), "m"),
    ("sgd", "dampening"): (("sgd", "randn", "own", "warm", 257, 1), "m"),
    ("sgd", "nesterov"): (("sgd", "randn", "own", "warm", 257, 1), "update"),
    # the parameter cannot see it (the update uses the new buffer either way): only the stored buffer does
    ("sgd", "buf_not_stored"): (("sgd", "randn", "own", "warm", 257, 1), "m"),
    ("adamw", "l2_for_decoupled"): (("adamw", "randn", "own", "warm", 257, 1), "m"),
    # SwaV's weight_decay = 1e-6 moves exp_avg by 1e-7 |p|: float32 noise; proved where the decay carries weight
    ("adamw", "decoupled_for_l2"): (("adam", "randn", "visible", "warm", 257, 1), "m"),
    ("adamw", "bc1_missing"): (("adamw", "randn", "own", "fresh", 257, 1), "update"),
    ("adamw", "bc2_not_sqrt"): (("adamw", "randn", "own", "fresh", 257, 1), "update"),
    # eps = 1e-8 against sqrt(v) ~ 1 moves p by 1e-8 relative on randn gradients: proved on tiny_grad (and visible on randn
    # with eps = 1e-3, test_eps_placement_is_invisible_on_randn_at_1e_8 states both)
    ("adamw", "eps_inside_sqrt"): (("adamw", "tiny_grad", "own", "fresh", 257, 1), "update"),
    # (at t = 1000 sqrt(1 - b2^t) is 1 in float32 and the two placements are the same number: proved at t = 1)
    ("adamw", "eps_before_bc2"): (("adamw", "tiny_grad", "own", "warm", 257, 1), "update"),
    # at lr = 1.5e-4, wd = 0.05 the order of decay and update moves p by lr wd |update| = 1e-9: proved at "visible"
    ("adamw", "decay_after_update"): (("adamw", "randn", "visible", "warm", 257, 1), "update"),
    # grad_scale = 1 in "own"
    ("adamw", "grad_scale_dropped"): (("adamw", "randn", "visible", "warm", 257, 1), "m"),
    ("adamw", "v_from_unscaled_g"): (("adamw", "randn", "visible", "warm", 257, 1), "v"),
    # Barlow Twins' weight_decay = 1.5e-6 leaves the term at float32 noise on randn segments
    # (test_lars_decay_term_is_invisible_at_barlow_on_randn_segments)
    ("lars", "wd_not_added_to_g"): (("vicreg", "warm", 3), "m"),
    ("lars", "wd_missing_in_ratio"): (("visible", "warm", 3), "m"),
    ("lars", "ratio_before_wd"): (("vicreg", "warm", 3), "m"),
    # grad_scale = 1 at the models' own sets
    ("lars", "norm_of_unscaled_g"): (("visible", "warm", 3), "m"),
    ("lars", "ratio_when_norm_zero"): (("visible", "fresh", 0), "m"),
    ("lars", "ratio_without_wd_gate"): (("wd0", "warm", 3), "m"),
    # eps = 1e-8 against |g| + wd |w| ~ 1: seen only on the tiny_grad segment
    ("lars", "eps_dropped"): (("barlow", "fresh", 0), "m"),
}
EQUIVALENT = {("lars", "segment_takes_neighbour")}
DIRECT = {("ema", "m_swapped"), ("center", "momentum_swapped"), ("center", "sum_not_mean"), ("colstats", "unbiased_var"),
          ("colstats", "var_about_zero"), ("standardize", "scale_not_inverse"), ("colscale", "dg_from_y"), ("colscale", "dx_without_g"),
          ("scale_bf16", "truncate"), ("cast", "truncate")}


def test_every_switch_is_named():
    assert set(CATCHES) | EQUIVALENT | DIRECT == {(op, sw) for op, sws in uc.SWITCHES.items() for sw in sws}
    assert all(c[0] in STEP_CASES for (op, _), c in CATCHES.items() if op != "lars")


def _step_verdicts(combo, sw):
    kind, fam, hset, state, n, t = combo
    x, h = uc.step_inputs(fam, n, n + t, state), uc.HYPER[kind][hset]
    ref, em = uc.step_outputs(kind, x, h, t), uc.step_outputs(kind, x, h, t, emulate=True)
    bad = uc.step_outputs(kind, x, h, t, emulate=True, seed_error=sw)
    return {k: ok(bad[k], ref[k], em[k], **uc.step_floor(k, ref)) for k in uc.STEP_TENSORS[kind]}


def _lars_failures(combo, sw):
    hset, state, rot = combo
    a, h = uc.lars_arena(9, state, rot), uc.HYPER["lars"][hset]
    ref, em = uc.lars_outputs(a, h), uc.lars_outputs(a, h, emulate=True)
    return lars_ok(uc.lars_outputs(a, h, emulate=True, seed_error=sw), ref, em, a, h)


@pytest.mark.parametrize("op,sw", sorted(CATCHES), ids=lambda v: str(v))
def test_seeded_error_is_rejected(op, sw):
    combo, tensor = CATCHES[(op, sw)]
    if op == "lars":
        assert tensor in {k for _, k in _lars_failures(combo, sw)}, (op, sw)
    else:
        assert not _step_verdicts(combo, sw)[tensor], (op, sw)


def test_buf_not_stored_is_invisible_in_the_parameter():
    """why the GPU tests compare the buffers and not the parameters alone"""
    v = _step_verdicts(("sgd", "randn", "own", "warm", 257, 1), "buf_not_stored")
    assert v["p"] and v["update"] and not v["m"]


def test_eps_placement_is_invisible_on_randn_at_1e_8():
    """what the older tests could not see: with eps = 1e-8 and randn gradients both misplacements of eps pass every tensor; at
    eps = 1e-3 ("visible") and on tiny gradients they do not"""
    for sw in ("eps_inside_sqrt", "eps_before_bc2"):
        assert all(_step_verdicts(("adamw", "randn", "own", "warm", 257, 1), sw).values())
        assert not _step_verdicts(("adamw", "randn", "visible", "warm", 257, 1), sw)["update"]
        assert not _step_verdicts(("adam", "tiny_grad", "own", "fresh", 257, 2), sw)["update"]


def test_lars_decay_term_is_invisible_at_barlow_on_randn_segments():
    """weight_decay = 1.5e-6: leaving wd * w out of the gradient passes every tensor of every randn segment (what the older test
    fed) -- the term is at float32 noise there.  The zero_grad_param and tiny_grad segments do see it even at Barlow Twins' own
    hyper-parameters (wd * w is then all, or 1 %, of the gradient); VICReg's 1e-4 and "visible" reject it on randn segments too."""
    a = uc.lars_arena(9, "warm", 3)
    seen = {a["kinds"][s] for s, _ in _lars_failures(("barlow", "warm", 3), "wd_not_added_to_g") if s >= 0}
    assert seen == {"zero_grad_param", "tiny_grad"}
    for hset in ("vicreg", "visible"):
        assert "randn" in {a["kinds"][s] for s, _ in _lars_failures((hset, "warm", 3), "wd_not_added_to_g") if s >= 0}


def test_direct_seeded_errors_are_rejected():
    x = uc.step_inputs("randn", 257, 1)
    ref, em = uc.ema_ref(x["p"], x["g"], 0.99), uc.ema_emul(x["p"], x["g"], 0.99)
    assert not ok(uc.ema_emul(x["p"], x["g"], 0.99, "m_swapped"), ref, em, abs_floor=fc.elem_floor(ref), floor_all=True)
    t, c0 = uc.col_inputs("randn", 7, 33, 7, bf16=True), uc.col_inputs("randn", 1, 33, 5)[0]
    ref, em = uc.center_ref(t, c0, 0.9), uc.center_emul(t, c0, 0.9)
    for sw in uc.SWITCHES["center"]:
        assert not ok(uc.center_emul(t, c0, 0.9, sw), ref, em, SUM, abs_floor=kc.f32_stat_floor(t, c0), floor_all=True), sw
    for sw, family in (("unbiased_var", "randn"), ("var_about_zero", "big_mean")):
        x = uc.col_inputs(family, 63, 33, 96)
        (_, vr), (_, ve) = uc.colstats_ref(x), uc.colstats_emul(x)
        assert not ok(uc.colstats_emul(x, sw)[1], vr, ve, SUM, abs_floor=uc.var_floor(x), floor_all=True, floor_cosine=True), sw
    x = uc.col_inputs("randn", 63, 33, 96)
    sr, se = uc.scaler_ref(x, x), uc.scaler_emul(x, x)
    assert not ok(uc.scaler_emul(x, x, "scale_not_inverse")["y"], sr["y"], se["y"], SUM, abs_floor=uc.scaled_floor(x, sr), floor_all=True, floor_cosine=True)
    x, dy = uc.col_inputs("randn", 64, 33, 64, bf16=True), uc.col_inputs("randn", 64, 33, 65, bf16=True)
    g = uc.col_inputs("randn", 1, 33, 7)[0]
    ref, em = uc.colscale_ref(x, g, dy), uc.colscale_emul(x, g, dy)
    assert not ok(uc.colscale_emul(x, g, dy, seed_error="dg_from_y")[2], ref[2], em[2], SUM, abs_floor=uc.colscale_dg_floor(x, dy, None))
    assert not kc.passes(uc.colscale_emul(x, g, dy, seed_error="dx_without_g")[1], ref[1], em[1])
    v = uc.cast_specials()
    assert not uc.same_bf16(uc.bf16_bits(v, truncate=True), uc.torch_bf16_bits(v))
    y = uc.bf16_specials(65536)
    assert not uc.same_bf16(uc.scale_bf16_bits(y, 1.0 / 3.0, "truncate"), uc.torch_bf16_bits(y * torch.tensor(1.0 / 3.0)))


def test_seeded_errors_that_are_equivalent():
    """segment_takes_neighbour: a norm over [begin, next begin) adds the alignment gap behind the segment, and the gaps of an arena
    are exactly 0 in the parameters and the gradients (optim._Arena zero-fills them, every update kernel maps 0 to 0 there, and the
    GPU tests assert that they stay 0): the norms, hence every output, are bit-identical.  Nothing is hidden by leaving it out."""
    for hset, state, rot in (("visible", "warm", 3), ("vicreg", "fresh", 0)):
        a, h = uc.lars_arena(9, state, rot), uc.HYPER["lars"][hset]
        good, bad = uc.lars_outputs(a, h, emulate=True), uc.lars_outputs(a, h, emulate=True, seed_error="segment_takes_neighbour")
        assert all(torch.equal(good[k], bad[k]) for k in good)
