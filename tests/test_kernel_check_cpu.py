"""The criteria of tests/kernel_check.py have teeth: proved on the CPU, without a kernel.

For every input family the GPU tests use, `check` is fed
  (a) an honest result: the emulation with every value moved by a few float32 ulp before each bf16 rounding
      (kernel_check.jitter), so its rounding events are independent of the yardstick's -- it must pass;
  (b) deliberately wrong computations, each of which the single criterion max |err| <= rel * max |ref| of
      tests/test_gpu_vit.py::_close accepts on unit-scale randn inputs -- each must fail at least one criterion.
A seeded error that passed would mean the inputs are too tame; the remedy is other inputs, never a wider bound."""
import kernel_check as kc
import pytest
import torch


def _reject(got, ref, emul, what):
    rows, finite = kc.verdict(got, ref, emul)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {line}"


def _accept(got, ref, emul, what):
    rows, finite = kc.verdict(got, ref, emul)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert finite and all(m <= b for _, m, b in rows), f"honest result rejected -- {what}: {line}"


# ---------------------------------------------------------------------------------------------------- attention
ATT_SHAPES = [(2, 37, 2, 64), (1, 197, 2, 64), (1, 250, 2, 32)]


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("b,s,h,hd", ATT_SHAPES)
def test_attention_honest_result_passes(family, b, s, h, hd):
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale, do)
    emul = kc.attention_ref(qkv, scale, do, emulate=True)
    with kc.jitter(1):
        got = kc.attention_ref(qkv, scale, do, emulate=True)
    _accept(got[0], ref[0], emul[0], f"out {family} S={s}")
    _accept(got[2], ref[2], emul[2], f"dqkv {family} S={s}")
    _accept(kc.attention_lse_f32(qkv, scale) * (1 + 2.0 ** -24), ref[1], kc.attention_lse_f32(qkv, scale), f"lse {family} S={s}")


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("b,s,h,hd", ATT_SHAPES)
@pytest.mark.parametrize("error,tensor", [("noscale", 0), ("nodelta", 2), ("bwd_noscale", 2), ("lse_m", 1)])
def test_attention_seeded_errors_fail(family, b, s, h, hd, error, tensor):
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale, do)
    emul = kc.attention_ref(qkv, scale, do, emulate=True)
    bad = kc.attention_ref(qkv, scale, do, emulate=True, seed_error=error)
    yard = kc.attention_lse_f32(qkv, scale) if tensor == 1 else emul[tensor]
    _reject(bad[tensor], ref[tensor], yard, f"{error} {family} S={s}")


@pytest.mark.parametrize("family", ["randn", "zero_query", "v_offset", "offset-80"])
def test_attention_unmasked_padding_fails(family):
    """S = 250 in a 256-slot tile: the six padded key slots (logit 0, value 0) join the softmax.  On unit randn the old
    criterion scores 0.0121 against its bound 0.015.  (With logits near +80 or of spread 16 a logit-0 slot carries no
    weight a bf16 result could show: those families cannot see this error and are not asked to.)"""
    b, s, h, hd = 1, 250, 2, 64
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale)
    emul = kc.attention_ref(qkv, scale, emulate=True)
    bad = kc.attention_ref(qkv, scale, emulate=True, seed_error="pad6")
    if family == "randn":
        old = float((bad[0] - ref[0]).abs().max() / ref[0].abs().max())
        assert old <= 1.5e-2, old  # the criterion this pull request replaces accepted it
    _reject(bad[0], ref[0], emul[0], f"pad6 {family}")


# ---------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(130, 768), (37, 192)]


@pytest.mark.parametrize("family", kc.LN_FAMILIES)
@pytest.mark.parametrize("rows,c", LN_SHAPES)
@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_layer_norm_honest_result_passes(family, rows, c, eps):
    x, gamma, beta, dy, dres = kc.layer_norm_inputs(family, rows, c, seed=rows)
    for skip in (None, dres):
        ref = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip)
        emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
        with kc.jitter(2):
            got = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
        _accept(got[0], ref[0], emul[0], f"y {family}")
        _accept(got[1], ref[1], emul[1], f"dx {family}")
    dg, db = kc.layer_norm_param_grads_f32(x, dy, eps)
    _accept(dg * (1 + 2.0 ** -24), ref[2], dg, f"dgamma {family}")
    _accept(db * (1 + 2.0 ** -24), ref[3], db, f"dbeta {family}")
    if family == "constant":
        assert torch.equal(emul[0], kc.bf(beta.double()).expand(rows, c))


@pytest.mark.parametrize("family", ["randn", "tight", "mean300", "big_row"])
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layer_norm_statistics_without_the_last_piece_fail(family, rows, c):
    """The last 8 columns left out of mean and variance: 0.0065 on the old criterion at 130 x 768 (bound 0.01)."""
    x, gamma, beta, dy, _ = kc.layer_norm_inputs(family, rows, c, seed=rows)
    ref = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True, seed_error="last8")
    if family == "randn" and c == 768:
        assert float((bad[0] - ref[0]).abs().max() / ref[0].abs().max()) <= 1e-2
    _reject(bad[0], ref[0], emul[0], f"last8 y {family} {rows}x{c}")


@pytest.mark.parametrize("rows,c", LN_SHAPES)
@pytest.mark.parametrize("eps,error", [(1e-6, "eps0"), (1e-6, "eps1e-5"), (1e-6, "eps1e-3"), (1e-5, "eps0"), (1e-5, "eps1e-3")])
def test_layer_norm_wrong_eps_fails_on_tight_rows(rows, c, eps, error):
    """eps is invisible on unit-scale rows (1e-7 .. 1e-4 on the old criterion, bound 0.01); on rows of spread ~1e-3 it
    decides the result.  Both eps values the GPU tests pass are covered, so a hard-coded one shows."""
    x, gamma, beta, dy, _ = kc.layer_norm_inputs("tight", rows, c, seed=rows)
    ref = kc.layer_norm_ref(x, gamma, beta, eps, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, eps, dy, emulate=True, seed_error=error)
    _reject(bad[0], ref[0], emul[0], f"{error} (asked {eps:g}) y")
    _reject(bad[1], ref[1], emul[1], f"{error} (asked {eps:g}) dx")
    xr, gr, br, dyr, _ = kc.layer_norm_inputs("randn", rows, c, seed=rows)
    r2 = kc.layer_norm_ref(xr, gr, br, eps, dyr)
    b2 = kc.layer_norm_ref(xr, gr, br, eps, dyr, emulate=True, seed_error=error)
    assert float((b2[0] - r2[0]).abs().max() / r2[0].abs().max()) <= 1e-2  # the old inputs and criterion accepted it


@pytest.mark.parametrize("family", ["randn", "tight", "mean300", "big_row"])
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layer_norm_dx_without_mean_of_dy_fails(family, rows, c):
    x, gamma, beta, dy, dres = kc.layer_norm_inputs(family, rows, c, seed=rows)
    dy = kc.bf(dy + 3.0)   # (the GPU tests' gradient for the parameter sums: column mean not zero)
    ref = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True, seed_error="no_mean_dy")
    _reject(bad[1], ref[1], emul[1], f"no_mean_dy {family}")


# ---------------------------------------------------------------------------------------------------- bias / act
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("res", [False, True])
def test_bias_act_honest_result_passes_and_short_dbias_fails(act, res):
    rows, c = 264, 64
    g = torch.Generator().manual_seed(act)
    x = kc.act_grid(rows, c, seed=act)
    bias = torch.randn(c, generator=g) * 0.3
    r = kc.bf(torch.randn(rows, c, generator=g)) if res else None
    dy = kc.bf(torch.randn(rows, c, generator=g) + 3.0)
    ref = kc.bias_act_ref(x, bias, act, r, dy)
    emul = kc.bias_act_ref(x, bias, act, r, dy, emulate=True)
    with kc.jitter(3):
        got = kc.bias_act_ref(x, bias, act, r, dy, emulate=True)
    _accept(got[0], ref[0], emul[0], f"y act={act}")
    _accept(got[1], ref[1], emul[1], f"dx act={act}")
    yard = kc.colsum_f32(emul[1])
    _accept(yard * (1 + 2.0 ** -24), emul[2], yard, f"dbias act={act}")
    bad = kc.bias_act_ref(x, bias, act, r, dy, emulate=True, seed_error="rows-1")
    _reject(bad[2], emul[2], yard, f"dbias over rows-1 rows, act={act}")
    if act == 2:  # ReLU gradient at exactly 0 is 0, as torch
        z = torch.zeros(8, 8)
        assert torch.equal(kc.bias_act_ref(z, None, 2, None, torch.ones(8, 8))[1], torch.zeros(8, 8, dtype=torch.float64))


def test_gelu_and_mish_match_torch_float64():
    v = torch.linspace(-12, 12, 4001, dtype=torch.float64).requires_grad_(True)
    for act, fn in ((1, torch.nn.functional.gelu), (3, torch.nn.functional.mish)):
        y = fn(v)
        (gr,) = torch.autograd.grad(y.sum(), v)
        torch.testing.assert_close(kc._act64(v.detach(), act), y.detach(), rtol=1e-12, atol=1e-14)   # (torch's own 1 + erf cancels in the tail)
        torch.testing.assert_close(kc._act_grad64(v.detach(), act), gr, rtol=1e-10, atol=1e-14)


# ---------------------------------------------------------------------------------------------------- references
def test_float64_references_match_autograd():
    """The closed-form float64 gradients the GPU tests compare with are what autograd gives."""
    qkv, do = kc.attention_inputs("randn", 2, 19, 2, 32, seed=0)
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))
    out = (((q @ k.transpose(-2, -1)) * 0.3).softmax(-1) @ v).transpose(1, 2)
    out.backward(do.double())
    ref = kc.attention_ref(qkv, 0.3, do)
    torch.testing.assert_close(ref[0], out.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ref[2], x.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref[1], torch.logsumexp((q @ k.transpose(-2, -1)) * 0.3, -1).detach(), rtol=1e-12, atol=1e-14)
    xl, gamma, beta, dy, dres = kc.layer_norm_inputs("randn", 9, 24, seed=1)
    t = [u.double().requires_grad_(True) for u in (xl, gamma, beta)]
    y = torch.nn.functional.layer_norm(t[0], (24,), t[1], t[2], 1e-5)
    (y * dy.double()).sum().backward()
    r = kc.layer_norm_ref(xl, gamma, beta, 1e-5, dy, dres)
    torch.testing.assert_close(r[0], y.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r[1], t[0].grad + dres.double(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r[2], t[1].grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r[3], t[2].grad, rtol=1e-10, atol=1e-12)
    g = torch.Generator().manual_seed(2)
    xm, res, dym = (kc.bf(torch.randn(11, 16, generator=g)) for _ in range(3))
    w1, w2 = kc.bf(torch.randn(32, 16, generator=g) * 0.3), kc.bf(torch.randn(16, 32, generator=g) * 0.3)
    b1, b2 = torch.randn(32, generator=g) * 0.1, torch.randn(16, generator=g) * 0.1
    tt = [u.double().requires_grad_(True) for u in (xm, w1, b1, w2, b2)]
    F = torch.nn.functional
    ym = F.linear(F.gelu(F.linear(tt[0], tt[1], tt[2])), tt[3], tt[4]) + res.double()
    ym.backward(dym.double())
    rm = kc.mlp_ref(xm, w1, b1, w2, b2, res, dym)
    torch.testing.assert_close(rm["y"], ym.detach(), rtol=1e-12, atol=1e-14)
    for name, u in zip(("dx", "dw1", "db1", "dw2", "db2"), tt):
        torch.testing.assert_close(rm[name], u.grad, rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- convolution
# (N, C, H, W, K, R, stride, pad): a ragged 3 x 3 / 1 with one row tile and a ragged chunk, and a 3 x 3 / 2 of two
# images whose input gradient runs by parity class
CONV_SHAPES = [(1, 64, 9, 11, 64, 3, 1, 1), (2, 64, 16, 16, 128, 3, 2, 1)]


def _conv_case(family, shape, seed_error=None, emulate=False, res=True):
    n, c, h, w, k, r, stride, pad = shape
    p, q = kc.conv_out_hw(h, w, r, r, stride, pad)
    i = kc.conv_inputs(family, n, h, w, c, k, r, r, p, q, seed=h)
    tiles = kc.row_tiles(n * p * q) or [torch.arange(n * p * q)]   # (M = 99: one ragged tile stands in for the slot)
    return i, kc.conv_ref(i["x"], i["w"], stride, pad, i["dy"], dres=i["dres"] if res else None, emulate=emulate,
                          seed_error=seed_error, tiles=tiles)


def _conv_f32(i, out, tiles_of="y"):
    """the float32 restatements: dW by matmul_tn_f32 on the im2col, the statistics slot sums by colsum_f32"""
    m = out["cols"].shape[0]
    k = i["w"].shape[0]
    dw = kc.matmul_tn_f32(i["dy"].reshape(m, k), out["cols"]).reshape(out["dw"].shape)
    floor = float(2.0 ** -24 * (i["dy"].reshape(m, k).double().abs().t() @ out["cols"].abs()).max())
    return dw, floor


@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
def test_conv_honest_result_passes(family, shape):
    i, ref = _conv_case(family, shape)
    _, emul = _conv_case(family, shape, emulate=True)
    with kc.jitter(4):
        _, got = _conv_case(family, shape, emulate=True)
    for key in ("y", "dx"):
        _accept(got[key], ref[key], emul[key], f"conv {key} {family} {shape}")
    dw32, floor = _conv_f32(i, ref)
    rows, finite = kc.verdict(dw32 * (1 + 2.0 ** -24), ref["dw"], dw32, kc.F32_SUM_FACTOR, floor)
    assert finite and all(m <= b for _, m, b in rows), rows
    if family == "lattice":   # the exact tier: the emulation rounds nothing away, the float32 restatement is exact
        kc.lattice_exact(ref)
        for key in ("y", "dx", "dw", "stats"):
            assert torch.equal(emul[key], ref[key]), key
        assert torch.equal(dw32.double(), ref["dw"])


def test_conv_ref_is_torch_conv2d():
    F = torch.nn.functional
    for n, c, h, w, k, r, stride, pad in CONV_SHAPES + [(1, 128, 5, 7, 64, 1, 2, 0), (2, 64, 10, 10, 64, 3, 1, 0)]:
        i, ref = _conv_case("randn", (n, c, h, w, k, r, stride, pad), res=False)
        x = i["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
        wt = i["w"].double().permute(0, 3, 1, 2).requires_grad_(True)
        y = F.conv2d(x, wt, None, stride, pad)
        y.backward(i["dy"].double().permute(0, 3, 1, 2))
        torch.testing.assert_close(ref["y"].permute(0, 3, 1, 2), y.detach(), rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(ref["dx"].permute(0, 3, 1, 2), x.grad, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(ref["dw"].permute(0, 3, 1, 2), wt.grad, rtol=1e-12, atol=1e-12)
    # the cropped 4 x 4 / pad 2 form of the space-to-depth stem
    g = torch.Generator().manual_seed(0)
    x, wt = kc.bf(torch.randn(2, 8, 8, 16, generator=g)), kc.bf(torch.randn(64, 4, 4, 16, generator=g))
    y = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), None, 1, 2)[:, :, :8, :8]
    torch.testing.assert_close(kc.conv_ref(x, wt, 1, 2, out_hw=(8, 8))["y"].permute(0, 3, 1, 2), y, rtol=1e-12, atol=1e-13)


# which tensors show each seeded error (a forward-only error leaves dx alone, and so on)
CONV_ERRORS = [("wrap_border", ("y", "dx", "dw")), ("image_bleed", ("y", "dx", "dw")), ("tap_transpose", ("y", "dx", "dw")),
               ("drop_tail", ("y", "dx", "dw")), ("one_class_missing", ("dx",)), ("res_unrounded", ("dx",)),
               ("stats_unrounded", ("stats",))]


def _conv_error_applies(error, shape, key):
    n, c, h, w, k, r, stride, pad = shape
    p, q = kc.conv_out_hw(h, w, r, r, stride, pad)
    if error == "image_bleed":
        return n > 1
    if error == "one_class_missing":
        return stride == 2
    if error == "drop_tail":   # a tail exists: M mod 128 rows of y, N H W mod 128 rows of dx, M mod 64 pixels of the last chunk
        return {"y": (n * p * q) % 128, "dx": (n * h * w) % 128, "dw": (n * p * q) % 64}[key] != 0
    return True


# big_pixel is there for what a huge value does to its neighbourhood (an overflow, a poisoned tile): the rounding error of
# the outputs that pixel reaches IS the yardstick, and an error that lives at the image border or in the tail rows, away
# from it, is below that.  Those three are asked of lattice, randn and offset.
CONV_ERROR_CASES = [(f, e, k) for f in kc.CONV_FAMILIES for e, k in CONV_ERRORS
                    if not (f == "big_pixel" and e in ("wrap_border", "image_bleed", "drop_tail"))]


@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("family,error,keys", CONV_ERROR_CASES)
def test_conv_seeded_errors_fail(family, shape, error, keys):
    """Every seeded error is rejected by `check` on every family, and on `lattice` by plain equality with float64.
    Two are invisible to the exact tier BY CONSTRUCTION and are asked of the other families only: on the lattice every
    accumulator is bf16-exact, so rounding it before (res_unrounded) or after the residual add, or taking the
    statistics from it (stats_unrounded), gives the same numbers.  stats_unrounded is also below what `check` can
    promise on the tolerance tier (see test_conv_stats_from_accumulators_...)."""
    i, ref = _conv_case(family, shape)
    _, emul = _conv_case(family, shape, emulate=True)
    _, bad = _conv_case(family, shape, seed_error=error, emulate=True)
    dw32, floor = _conv_f32(i, ref)
    _, bad_plain = _conv_case(family, shape, seed_error=error)
    asked = 0
    for key in keys:
        if not _conv_error_applies(error, shape, key):
            continue
        if error in ("res_unrounded", "stats_unrounded"):
            if family == "lattice":
                assert torch.equal(bad[key], ref[key])   # provably invisible: see the docstring
            continue
        asked += 1
        if family == "lattice":
            assert not torch.equal(bad[key], ref[key]), f"{error} {key}: exact tier blind"
        if key == "dw":
            # the float32 restatement of the wrong computation (its own im2col)
            m, k = bad["cols"].shape[0], i["w"].shape[0]
            got = bad_plain["dw"].float()
            rows, finite = kc.verdict(got, ref["dw"], dw32, kc.F32_SUM_FACTOR, floor)
            assert any(mm > b for _, mm, b in rows), f"seeded error accepted -- {error} dw {family}: {rows}"
        else:
            _reject(bad[key], ref[key], emul[key], f"{error} {key} {family} {shape}")
    if error not in ("res_unrounded", "stats_unrounded"):
        assert asked or not any(_conv_error_applies(error, shape, k) for k in keys)


@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("family", ["randn", "offset", "big_pixel"])
def test_conv_rounding_place_errors(family, shape):
    """res_unrounded and stats_unrounded differ from the honest kernel by ONE bf16 rounding per element, the size of
    the yardstick's own error: a factor-2 bound on distribution criteria cannot tell them apart, and this test records
    that instead of pretending.  What does see them: the statistics slots are compared with the float64 column sums of
    the kernel's OWN stored tile under the float32 summation bound (tests/test_gpu_conv.py), which sums taken from
    the accumulators miss by orders of magnitude -- asserted here on the same numbers."""
    i, ref = _conv_case(family, shape)
    _, emul = _conv_case(family, shape, emulate=True)
    _, bad = _conv_case(family, shape, seed_error="stats_unrounded", emulate=True)
    own = emul["stats"]                                   # float64 sums of the rounded (= stored) outputs
    n, c, h, w, k, r, stride, pad = shape
    m = emul["y"].numel() // k
    tiles = kc.row_tiles(m) or [torch.arange(m)]
    y = emul["y"].reshape(m, k)
    bound = kc.f32_sum_bound(y, tiles)
    assert bool(((bad["stats"][:, 0] - own[:, 0]).abs() > bound[0]).any()), "sums of the accumulators within the float32 bound"
    _, bad = _conv_case(family, shape, seed_error="res_unrounded", emulate=True)
    print("res_unrounded dx:", kc.verdict(bad["dx"], ref["dx"], emul["dx"])[0])


# ---------------------------------------------------------------------------------------------------- BatchNorm-backward epilogue
def _bnb_case(family, form, groups=2, seed_error=None, emulate=False, res=True):
    shape = (4, 64, 8, 8, 64, 3, 1, 1)
    n, c, h, w, k, r, stride, pad = shape
    i = kc.conv_inputs(family, n, h, w, c, k, r, r, h, w, seed=7)
    b = kc.bn_inputs(family, n * h * w, c, groups, seed=8)
    conv = kc.conv_ref(i["x"], i["w"], stride, pad, i["dy"])
    tiles = kc.pair_tiles(n, h, w)
    out = kc.bn_dgrad_epilogue_ref(conv["dx_acc"], i["dres"] if res else None, b["bn_y"], b["mean"], b["invstd"], b["gamma"],
                                   b["beta"], form, b["relu_x"], b["mask"], tiles, emulate=emulate, seed_error=seed_error)
    return b, tiles, out


# (the recomputed mask of the mean-50 `offset` rows hangs on float32 cancellation: that form is asked of lattice and randn)
@pytest.mark.parametrize("family,form", [(f, m) for f in ("lattice", "randn", "offset") for m in ("x", "bits", "recompute")
                                         if (f, m) != ("offset", "recompute")])
def test_bn_dgrad_epilogue_honest_passes_and_errors_fail(family, form):
    b, tiles, ref = _bnb_case(family, form)
    _, _, emul = _bnb_case(family, form, emulate=True)
    with kc.jitter(5):
        _, _, got = _bnb_case(family, form, emulate=True)
    if form == "recompute" and family == "randn":
        assert kc.bn_preact_margin(b) > 8 * kc.BF16_ULP
    _accept(got["dx"], ref["dx"], emul["dx"], f"bnb dx {family} {form}")
    for j, key in enumerate(("g", "gy")):
        yard = kc.tile_sums_f32(emul[key], tiles)
        rows, finite = kc.verdict(yard * (1 + 2.0 ** -24), ref["stats"][:, j], yard, kc.F32_SUM_FACTOR,
                                  max(kc.f32_sum_floor(emul[key][t]) for t in tiles))
        assert finite and all(m <= bb for _, m, bb in rows), (key, rows)
    if family == "lattice":
        kc.lattice_exact({"dx": ref["dx"], "stats": ref["stats"]})
        assert torch.equal(emul["dx"], ref["dx"]) and torch.equal(emul["stats"], ref["stats"])
    errors = (["mask_off_by_channel"] if form == "bits" else []) + (["stat_uncentred"] if family != "randn" else [])
    for error in errors:
        _, _, bad = _bnb_case(family, form, seed_error=error, emulate=True)
        j = 1 if error == "stat_uncentred" else 0
        key = ("g", "gy")[j]
        if family == "lattice":
            assert not torch.equal(bad["stats"][:, j], ref["stats"][:, j]), error
        yard = kc.tile_sums_f32(emul[key], tiles)
        rows, finite = kc.verdict(kc.tile_sums_f32(bad[key], tiles), ref["stats"][:, j], yard, kc.F32_SUM_FACTOR,
                                  max(kc.f32_sum_floor(emul[key][t]) for t in tiles))
        assert any(m > bb for _, m, bb in rows), f"seeded error accepted -- {error} {family} {form}: {rows}"
        if error == "mask_off_by_channel":
            _reject(bad["dx"], ref["dx"], emul["dx"], f"{error} dx {family}")


# ---------------------------------------------------------------------------------------------------- BatchNorm
# The smallest narrow shapes tests/test_gpu_bn.py runs, one of several blocks, and the smallest wide ones: (rows / G, C, wide)
BN_SHAPES = [(3, 8, False), (2, 64, False), (530, 40, False), (2, 2056, True), (5, 2056, True)]
BN_EPS, BN_MOM = 1e-5, 0.1
# rows / G of every GPU case (narrow, grid caps, wide, the two-rank totals of the synchronised tests)
BN_ROW_COUNTS = [2, 3, 4, 5, 10, 33, 37, 38, 40, 74, 523, 524, 530, 1366, 1367, 8200, 16500]


def _bn_fwd(b, g, wide=False, emulate=False, seed_error=None, relu=1, res=True, eps=BN_EPS):
    return kc.bn_forward_ref(b["y"], b["residual"] if res else None, b["gamma"], b["beta"], g, eps, BN_MOM, relu,
                             (b["running_mean"], b["running_var"]), emulate=emulate, wide=wide and emulate, seed_error=seed_error)


def _stat_verdict(got, ref, emul, floor):
    return kc.verdict(got, ref, emul, kc.F32_SUM_FACTOR, floor, floor_all=True)


def _bn_floors(b, g):
    y, m = b["y"].double(), b["y"].shape[0] // g
    return {"mean": kc.f32_sum_floor(y) / m, "running_mean": kc.f32_sum_floor(y) / m + kc.f32_stat_floor(b["running_mean"]),
            "running_var": kc.f32_sum_floor(y * y) / max(m - 1, 1) + kc.f32_stat_floor(b["running_var"])}


def _stat_rejected(bad, ref, emul, floor, what):
    rows, finite = _stat_verdict(bad, ref, emul, floor)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {line}"


def test_bn_references_agree_with_torch_in_float64():
    """bn_forward_ref / bn_backward_ref against torch's own batch_norm and autograd per statistics group, in float64"""
    import torch.nn.functional as F

    rows, c, g = 24, 16, 3
    b = kc.bn_forward_inputs("randn", rows, c, g, seed=1)
    ref = _bn_fwd(b, g)
    y = b["y"].double().requires_grad_(True)
    ga, be = b["gamma"].double().requires_grad_(True), b["beta"].double().requires_grad_(True)
    rm, rv = b["running_mean"].double().clone(), b["running_var"].double().clone()
    pre = torch.cat([F.batch_norm(part, rm, rv, ga, be, True, float(torch.tensor(BN_MOM).float()), float(torch.tensor(BN_EPS).float()))
                     for part in y.chunk(g)])
    out = F.relu(pre + b["residual"].double())
    torch.testing.assert_close(out, ref["out"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rm, ref["running_mean"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv, ref["running_var"], rtol=1e-12, atol=1e-12)
    dout = torch.randn(rows, c, generator=torch.Generator().manual_seed(2)).double()
    out.backward(dout)
    back = kc.bn_backward_ref(b["y"], dout, b["gamma"], b["beta"], ref["mean"], ref["invstd"], g, out_relu=ref["out"])
    torch.testing.assert_close(back["dy"], y.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(back["dgamma"], ga.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(back["dbeta"], be.grad, rtol=1e-10, atol=1e-11)
    remask = kc.bn_backward_ref(b["y"], dout, b["gamma"], b["beta"], ref["mean"], ref["invstd"], g, remask=True)
    nores = _bn_fwd(b, g, res=False)
    assert torch.equal(remask["dz"], dout * (nores["out"] > 0))


@pytest.mark.parametrize("family", kc.BN_FORWARD_FAMILIES[1:])
@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("rpg,c,wide", BN_SHAPES)
def test_bn_forward_honest_result_passes(rpg, c, wide, g, family):
    b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=rpg + c)
    ref, emul = _bn_fwd(b, g), _bn_fwd(b, g, wide, emulate=True)
    with kc.jitter(6):
        got = _bn_fwd(b, g, wide, emulate=True)
    _accept(got["out"], ref["out"], emul["out"], f"out {family}")
    floors = _bn_floors(b, g)
    for name in ("mean", "invstd", "running_mean", "running_var"):
        rows, finite = _stat_verdict(emul[name] * (1 + 2.0 ** -24), ref[name], emul[name], floors.get(name, kc.f32_stat_floor(ref[name])))
        assert finite and all(m <= bd for _, m, bd in rows), (name, rows)


def test_bn_forward_lattice_is_exact_in_float32():
    """The emulation (float32 block sums in row order) and float64 agree bit for bit on the lattice: out, mean, invstd,
    running_mean always, running_var where rows / G - 1 is a power of two"""
    for rpg, c in [(2, 64), (4, 8), (530, 40), (38, 1032)]:
        for g in (1, 2, 3):
            b = kc.bn_forward_inputs("lattice", rpg * g, c, g, seed=rpg)
            assert g == 1 or not torch.equal(b["mean"][0], b["mean"][1])
            ref, emul = _bn_fwd(b, g, eps=0.0), _bn_fwd(b, g, emulate=True, eps=0.0)
            ref = dict(ref, **{k: v for k, v in kc.bn_forward_ref(b["y"], b["residual"], b["gamma"], b["beta"], g, 0.0, 0.125, 1,
                                                                  (b["running_mean"], b["running_var"])).items() if "running" in k})
            emul = dict(emul, **{k: v for k, v in kc.bn_forward_ref(b["y"], b["residual"], b["gamma"], b["beta"], g, 0.0, 0.125, 1,
                                                                    (b["running_mean"], b["running_var"]), emulate=True).items() if "running" in k})
            for name in ("out", "mean", "invstd", "scale", "shift", "running_mean") + (("running_var",) if rpg == 2 else ()):
                assert torch.equal(ref[name], emul[name]), (name, rpg, c, g)
            assert torch.equal(ref["relu_mask"], emul["relu_mask"]) and bool((ref["out"] == 0).any())
            bad = _bn_fwd(b, g, emulate=True, eps=0.0, seed_error="mask_ge_zero")
            assert not torch.equal(bad["relu_mask"], ref["relu_mask"])            # mask_ge_zero on the lattice: plain inequality


# (error, tensor that shows it, families that can see it, needs G >= 2).  Left out, with the reason:
#   eps_dropped on randn / offset / big_value -- eps is 2.5e-6 of the variance (or less), below the float32 noise of invstd;
#     "constant" decides it (variance exactly 0: invstd = eps^-1/2 against inf)
#   groups_pooled, running_from_last_group_only at G = 1 -- one group: nothing to pool or to leave out
BN_FWD_ERRORS = [
    # (offset is left out here: at 530 rows in one reduce block the float32 sum of y^2 is past 2^24 grid steps and the variance
    # of the narrow path carries 5e-4 .. 2e-3 of noise, the size of 1 / (M - 1); randn at every row count is the test below)
    ("biased_running_var", "running_var", ("randn", "constant", "big_value"), False),
    ("eps_dropped", "invstd", ("constant",), False),
    ("groups_pooled", "mean", ("randn", "offset", "constant", "big_value"), True),
    ("running_from_last_group_only", "running_mean", ("randn", "offset", "constant", "big_value"), True),
    ("residual_after_relu", "out", ("randn", "offset", "constant", "big_value"), False),
    ("var_over_m_minus_1", "invstd", ("randn", "constant", "big_value"), False),   # (offset: see the cancellation test -- its
    # float32 noise on invstd at |mean| / std = 50 is of the size of 1 / (2 M) from a few hundred rows on)
]


@pytest.mark.parametrize("error,tensor,families,multi", BN_FWD_ERRORS)
@pytest.mark.parametrize("rpg,c,wide", BN_SHAPES)
def test_bn_forward_seeded_errors_fail(rpg, c, wide, error, tensor, families, multi):
    for family in families:
        for g in ((2, 3) if multi else (1, 2, 3)):
            b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=rpg + c)
            ref, emul = _bn_fwd(b, g), _bn_fwd(b, g, wide, emulate=True)
            bad = _bn_fwd(b, g, wide, emulate=True, seed_error=error)
            what = f"{error} {family} {rpg}x{c} G={g}"
            if tensor == "out":
                _reject(bad[tensor], ref[tensor], emul[tensor], what)
            else:
                _stat_rejected(bad[tensor], ref[tensor], emul[tensor], _bn_floors(b, g).get(tensor, kc.f32_stat_floor(ref[tensor])), what)


@pytest.mark.parametrize("rpg", BN_ROW_COUNTS)
def test_bn_biased_running_variance_fails_at_every_row_count(rpg):
    """1 / (M - 1) relative: 6e-5 at the largest count, three orders above the float32 yardstick"""
    for wide, c in ((False, 8), (True, 2056)):
        if wide and rpg > 40:
            continue
        b = kc.bn_forward_inputs("randn", rpg, c, 1, seed=rpg)
        ref, emul = _bn_fwd(b, 1), _bn_fwd(b, 1, wide, emulate=True)
        bad = _bn_fwd(b, 1, wide, emulate=True, seed_error="biased_running_var")
        _stat_rejected(bad["running_var"], ref["running_var"], emul["running_var"], _bn_floors(b, 1)["running_var"], f"biased M={rpg}")


def test_bn_dropped_eps_fails_on_constant_channels():
    for rpg, c, wide in BN_SHAPES:
        b = kc.bn_forward_inputs("constant", rpg * 2, c, 2, seed=c)
        ref, emul = _bn_fwd(b, 2), _bn_fwd(b, 2, wide, emulate=True)
        eps32 = torch.tensor(BN_EPS).float().double()
        assert bool((ref["invstd"][:, ::3] == eps32.rsqrt()).all())                                # variance exactly 0: eps decides
        assert torch.equal(emul["invstd"][:, ::3], ref["invstd"][:, ::3].float().double())
        bad = _bn_fwd(b, 2, wide, emulate=True, seed_error="eps_dropped")
        assert not bool(torch.isfinite(bad["invstd"]).all())
        _stat_rejected(bad["invstd"], ref["invstd"], emul["invstd"], kc.f32_stat_floor(ref["invstd"]), f"eps_dropped {rpg}x{c}")


def _bn_bwd(b, g, emulate=False, wide=False, seed_error=None, form="out", **kw):
    return kc.bn_backward_ref(b["bn_y"], b["dout"], b["gamma"], b["beta"], b["mean"], b["invstd"], g,
                              out_relu=b["relu_x"] if form == "out" else None, remask=form == "y", emulate=emulate,
                              wide=wide and emulate, seed_error=seed_error, **kw)


# (error, tensor, families, form).  mask_ge_zero is a lattice matter: randn / offset draw relu_x from randn (no exact zero), and
# their recomputed pre-activations keep a margin from zero by construction, so > and >= select the same elements there.
BN_BWD_ERRORS = [
    ("dz_unmasked", "dz", ("lattice", "randn", "offset"), "out"),
    ("dz_unmasked", "dy", ("lattice", "randn"), "y"),
    ("xhat_uncentred", "dy", ("lattice", "randn", "offset"), "out"),
    ("xhat_uncentred", "dgamma", ("lattice", "randn", "offset"), None),
    ("s2_term_dropped", "dy", ("lattice", "randn", "offset"), None),
    ("mask_ge_zero", "dz", ("lattice",), "out"),
    ("mask_ge_zero", "dz", ("lattice",), "y"),
]


@pytest.mark.parametrize("error,tensor,families,form", BN_BWD_ERRORS)
@pytest.mark.parametrize("rpg,c,wide", [(4, 8, False), (2, 64, False), (512, 40, False), (2, 2056, True), (4, 2056, True)])
def test_bn_backward_seeded_errors_fail(rpg, c, wide, error, tensor, families, form):
    for family in families:
        for g in (1, 2, 3):
            b = kc.bn_backward_inputs(family, rpg * g, c, g, seed=rpg + c)
            ref, bad = _bn_bwd(b, g, form=form), _bn_bwd(b, g, True, wide, error, form)
            what = f"{error} {family} {rpg}x{c} G={g} {tensor}"
            if family == "lattice":
                kc.bn_lattice_exact(ref["pre"])
                want = kc.bf(ref[tensor]) if tensor == "dy" else ref[tensor]
                assert not torch.equal(bad[tensor], want), what
                assert torch.equal(_bn_bwd(b, g, True, wide, None, form)[tensor], want), what   # (and the honest emulation is exact)
                continue
            emul = _bn_bwd(b, g, True, wide, None, form)
            if tensor == "dgamma":
                dz, xh = ref["dz"], (b["bn_y"].double() - b["mean"].double()[torch.arange(rpg * g) // rpg]) * b["invstd"].double()[torch.arange(rpg * g) // rpg]
                _stat_rejected(bad[tensor], ref[tensor], emul[tensor], kc.f32_sum_floor(dz * xh), what)
            else:
                _reject(bad[tensor], ref[tensor], emul[tensor], what)
                with kc.jitter(7):
                    _accept(_bn_bwd(b, g, True, wide, None, form)[tensor], ref[tensor], emul[tensor], what + " honest")


@pytest.mark.parametrize("family", ["lattice", "randn", "offset"])
def test_bn_backward_form_errors_fail(family):
    """mean_over_local_rows (the synchronised form divides by the local rows), fx_unscaled (slots holding sum g (y - mean) not
    multiplied by invstd), accumulate_ignored"""
    rl, c, g = 32, 40, 2
    b = kc.bn_backward_inputs(family, 2 * rl * g, c, g, seed=9)
    whole = _bn_bwd(b, g, form=None)
    half = {k: (v.reshape(g, 2, rl, c)[:, 0].reshape(g * rl, c) if k in ("bn_y", "dout", "relu_x") else v) for k, v in b.items()}
    lat = family == "lattice"

    def differs(bad, ref, emul, what):
        if lat:
            assert not torch.equal(bad, ref) and torch.equal(emul, ref), what
        else:
            _reject(bad, ref, emul, what)

    ref = _bn_bwd(half, g, form=None, group_count=2 * rl, totals=whole["sums"])
    emul = _bn_bwd(half, g, True, form=None, group_count=2 * rl, totals=whole["sums"].float())
    bad = _bn_bwd(half, g, True, form=None, group_count=2 * rl, totals=whole["sums"].float(), seed_error="mean_over_local_rows")
    assert torch.equal(ref["dy"], whole["dy"].reshape(g, 2, rl, c)[:, 0].reshape(g * rl, c))     # a rank's rows of the whole batch
    differs(bad["dy"], kc.bf(ref["dy"]) if lat else ref["dy"], emul["dy"], f"mean_over_local_rows {family}")
    grp = torch.arange(2 * rl * g) // (2 * rl)
    gr = b["dout"].double()
    slots = kc.bn_row_slots(gr, gr * (b["bn_y"].double() - b["mean"].double()[grp]), g, 5, seed=3)
    ref, emul = _bn_bwd(b, g, form=None, fx_slots=slots), _bn_bwd(b, g, True, form=None, fx_slots=slots)
    bad = _bn_bwd(b, g, True, form=None, fx_slots=slots, seed_error="fx_unscaled")
    if not lat:
        assert float((ref["dgamma"] - whole["dgamma"]).abs().max()) <= 1e-5 * float(whole["dgamma"].abs().max())  # slots = the sums
    differs(bad["dy"], kc.bf(ref["dy"]) if lat else ref["dy"], emul["dy"], f"fx_unscaled dy {family}")
    assert not torch.equal(bad["dgamma"], ref["dgamma"])
    if not lat:
        _stat_rejected(bad["dgamma"], ref["dgamma"], emul["dgamma"], kc.f32_sum_floor(gr * 4.0), f"fx_unscaled dgamma {family}")
    ref = _bn_bwd(b, g, form=None, accumulate_into=b["acc"])
    emul = _bn_bwd(b, g, True, form=None, accumulate_into=b["acc"])
    bad = _bn_bwd(b, g, True, form=None, accumulate_into=b["acc"], seed_error="accumulate_ignored")
    for name in ("dgamma", "dbeta"):
        if lat:
            assert not torch.equal(bad[name], ref[name]) and torch.equal(emul[name], ref[name])
        else:
            _stat_rejected(bad[name], ref[name], emul[name], kc.f32_sum_floor(gr * 4.0), f"accumulate_ignored {name} {family}")


def test_bn_narrow_path_cancellation_is_measured():
    """The documented narrow-path arithmetic (float32 block sums of y and y^2, var = ss / M - mean^2 in double) against float64
    on save_invstd for the offset family, with bn_col_fwd's two-pass float32 form beside it.  A measurement of the FORMULA
    (profiles/bn_kernel_check.md holds the numbers).  Asserted: both stay inside what Higham's bound of a float32 sum of n
    terms allows them -- gamma_n (mean^2 / var + 1) on the one-pass variance (n = the rows of a reduce block), gamma_n on the
    two-pass one (n = the rows of the group) -- and invstd moves by half of the variance's relative error."""
    u = 2.0 ** -24
    for rows, c in ((1568, 64), (530, 40)):
        n_block = max(b - a for a, b in kc.bn_block_rows(rows, c))
        for ratio in (50.0, 300.0):
            b = kc.bn_forward_inputs("offset", rows, c, 1, seed=int(ratio), offset=ratio)
            ref = _bn_fwd(b, 1)["invstd"]
            narrow = _bn_fwd(b, 1, emulate=True)["invstd"]
            two_pass = _bn_fwd(b, 1, wide=True, emulate=True)["invstd"]
            en, ew = ((narrow - ref).abs() / ref), ((two_pass - ref).abs() / ref)
            print(f"{rows} x {c}, |mean| / std = {ratio:g}: one-pass max {float(en.max()):.3g} rms {float(en.pow(2).mean().sqrt()):.3g}; "
                  f"two-pass max {float(ew.max()):.3g} rms {float(ew.pow(2).mean().sqrt()):.3g}; bf16 ulp {kc.BF16_ULP:.3g}")
            var_min = float(ref.pow(-2).min())
            assert float(ew.max()) < 0.5 * rows * u * 1.1 + u
            assert float(en.max()) < 0.5 * n_block * u * (ratio * ratio / var_min + 1.0) * 1.1 + u


# ---------------------------------------------------------------------------------------------------- pooling
def test_pool_references_and_their_seeded_errors():
    """maxpool_ref / maxpool_bwd_ref / gap_ref against torch; a padding of 0 is rejected on all-negative inputs (and only
    there: on relu outputs, what tests/test_gpu_ops.py feeds, it is invisible); the last of equal maxima on constant patches."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(0)
    for n, h, w, c in [(1, 2, 2, 8), (2, 3, 5, 24), (3, 7, 6, 64), (2, 7, 5, 8)]:
        x = kc.bf(torch.randn(n, h, w, c, generator=g))
        best, code = kc.maxpool_ref(x)
        xt = x.permute(0, 3, 1, 2).double().requires_grad_(True)
        want = F.max_pool2d(xt, 3, 2, 1)
        assert torch.equal(best.double(), want.permute(0, 2, 3, 1))
        dy = torch.randn(best.shape, generator=g)
        want.backward(dy.permute(0, 3, 1, 2).double())
        assert torch.equal(kc.maxpool_bwd_ref(dy, code, h, w), xt.grad.permute(0, 2, 3, 1))
        neg = -x.abs() - 0.5
        assert not torch.equal(kc.maxpool_ref(neg, "zero_pad")[0], kc.maxpool_ref(neg)[0])
        pos = x.clamp_min(0.0)
        assert torch.equal(kc.maxpool_ref(pos, "zero_pad")[0], kc.maxpool_ref(pos)[0])            # relu outputs cannot see it
        if h % 2 == 1 and w % 2 == 1:
            flat = torch.ones(n, h, w, c)
            assert not torch.equal(kc.maxpool_ref(flat, "last_max")[1], kc.maxpool_ref(flat)[1])
            assert torch.equal(kc.maxpool_ref(flat, "last_max")[0], kc.maxpool_ref(flat)[0])
    x = kc.bf(torch.randn(5, 49, 24, generator=g) * 2 + 0.5)
    torch.testing.assert_close(kc.gap_ref(x), x.double().mean(1), rtol=1e-14, atol=1e-14)
    _accept(kc.gap_ref(x, emulate=True), kc.gap_ref(x), kc.gap_ref(x, emulate=True), "gap emulation")
    _reject(kc.bf(x.double()[:, :-1].mean(1)), kc.gap_ref(x), kc.gap_ref(x, emulate=True), "gap without the last pixel")


# ---------------------------------------------------------------------------------------------------- loss kernels
# csrc/embed.hip: tests/loss_cases.py holds the references (dt = float64), the float32 restatements (dt = float32) and the
# seeded errors; tests/test_gpu_losses.py feeds the kernels the same families at the same shapes.
import functools  # noqa: E402
import math  # noqa: E402

import loss_cases as lc  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from oracle import ntxent as on  # noqa: E402

F64, F32 = torch.float64, torch.float32
ONE_ULP = 1.0 + 2.0 ** -24          # (a float64 scalar moved by one float32 rounding)


def _ulp(t, seed=0):
    """every element of a float32 tensor moved to its float32 NEIGHBOUR, up or down at random (torch.nextafter): one more
    rounding somewhere in the chain.  An exact 0 stays (a masked entry, 0 x anything: no order of operations moves it)."""
    if not (torch.is_tensor(t) and t.dtype == F32):
        return t
    g = torch.Generator().manual_seed(seed)
    up = torch.rand(t.shape, generator=g) < 0.5
    out = torch.nextafter(t, torch.where(up, torch.full_like(t, float("inf")), torch.full_like(t, -float("inf"))))
    out = torch.where(t == 0, t, out)
    assert not bool((t != 0).any()) or not torch.equal(out, t)
    return out


def _honest(fn, *args, **kw):
    """An honest float32 result that is NOT the yardstick: the float32 restatement with every sum in the reverse order
    (loss_cases.other_order: another reduction tree), then every element moved to a float32 neighbour (_ulp)"""
    with lc.other_order():
        out = fn(*args, dt=F32, **kw)
    if torch.is_tensor(out):
        return _ulp(out)
    return {k: _ulp(v, seed=i) for i, (k, v) in enumerate(out.items())}


def _accept32(got, ref, emul, floor, what):
    rows, finite = lc.verdict_f32(got, ref, emul, floor)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    assert finite and all(m <= b for _, m, b in rows), f"honest result rejected -- {what}: {line}"


def _reject32(got, ref, emul, floor, what):
    rows, finite = lc.verdict_f32(got, ref, emul, floor)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {line}"


# Where a seeded error computes the SAME thing on a family, the test that leaves the pair out says so at that place and,
# where it is cheap, asserts the equality (test_seeded_errors_that_are_equivalent).  The NT-Xent pairs not run: pos_at_rank0 at
# rank_offset = 0 (that column is the right one); drop_last_tile where 2 b_global % 64 == 0 (no ragged tile); drop_last_split
# where nsplit == 1 (one slab); no_max where every exp(logit) stays below the float32 maximum e^88 (T >= 0.07, or randn rows
# at T = 0.01, whose cosines at d = 96 stay below 0.5).


def test_seeded_errors_that_are_equivalent():
    """the pairs the rejection tests leave out give bit-identical float32 results: nothing is hidden by leaving them out"""
    same = lambda x, y: all(torch.equal(x[k], y[k]) for k in x if torch.is_tensor(x[k]))  # noqa: E731
    args, _, emul = _nx_case("randn", 33, 1, 0, 96, 0.5)
    assert same(lc.ntxent(*args, dt=F32, seed_error="pos_at_rank0"), emul)                 # rank_offset = 0
    args, _, emul = _nx_case("randn", 256, 1, 0, 32, 0.07)
    assert same(lc.ntxent(*args, dt=F32, seed_error="drop_last_tile"), emul)               # 512 % 64 == 0
    args, _, emul = _nx_case("randn", 1, 1, 0, 32, 0.5)
    assert same(lc.ntxent(*args, dt=F32, seed_error="drop_last_split"), emul)              # nsplit == 1
    x, t = lc.logit_inputs("randn", 7, 5, seed=1), torch.rand(7, 5)
    assert same(lc.bce_logits(x, t, None, dt=F32, seed_error="pos_weight_by_row"), lc.bce_logits(x, t, None, dt=F32))
    y = torch.arange(7) % 5
    for error in ("mean_over_B", "ignored_counted"):                                       # no weights, nothing ignored
        assert same({"d": lc.cross_entropy(x, y, None, dt=F32, seed_error=error)["dlogits"]}, {"d": lc.cross_entropy(x, y, None, dt=F32)["dlogits"]})
    z0, z1 = lc.dcl_inputs(3, 32, seed=1)
    for error in ("weights_differentiated", "weight_one_direction"):                       # DCL: the weights are the constant 1
        bad, good = lc.dcl(z0, z1, 0.1, None, dt=F32, seed_error=error), lc.dcl(z0, z1, 0.1, None, dt=F32)
        assert torch.equal(bad["dz0"], good["dz0"]) and torch.equal(bad["terms"], good["terms"])
    raw = torch.randn(17, 17)
    assert same(lc.barlow(raw, 0.1, 5e-3, 0.0, dt=F32, seed_error="lambda_on_diagonal"), lc.barlow(raw, 0.1, 5e-3, 0.0, dt=F32))
    xs = lc.sinkhorn_inputs(1, 7, seed=1)                                                 # B = 1: Q is the row's softmax either way
    for error in ("samples_first", "one_round_short"):
        assert torch.equal(lc.sinkhorn(xs, 0.05, 0, dt=F32, seed_error=error), lc.sinkhorn(xs, 0.05, 0, dt=F32))   # iters = 0: no round
    x0 = torch.zeros(2, 8)
    assert torch.equal(lc.l2norm(x0, 1e-3, dt=F32, seed_error="eps_added")["y"], lc.l2norm(x0, 1e-3, dt=F32)["y"])   # a zero row: 0 either way


@functools.lru_cache(maxsize=None)
def _nx_case(family, b_local, world, rank, d, temp):
    z0, z1 = lc.ntxent_inputs(family, b_local * world, d, seed=b_local + d)
    bg = b_local * world
    zall = lc.normalized32(torch.cat([z0, z1]))
    zn = torch.cat([zall[rank * b_local:(rank + 1) * b_local], zall[bg + rank * b_local:bg + (rank + 1) * b_local]]).contiguous()
    args = (zn, zall, b_local, bg, rank * b_local, temp, 1.0 / (2 * b_local))
    return args, lc.ntxent(*args, dt=F64), lc.ntxent(*args, dt=F32)


def _nx_compare(fn, bad, ref, emul, temp, what):
    for key, floor in (("lse", lc.ntxent_lse_floor(temp, ref)), ("loss_rows", lc.ntxent_lse_floor(temp, ref)), ("dzn", ref["dzn_floor"])):
        fn(bad[key], ref[key], emul[key], floor, f"{what} {key}")


@pytest.mark.parametrize("family", lc.NTXENT_FAMILIES)
@pytest.mark.parametrize("b_local,world,rank,d,temp", [(1, 1, 0, 32, 0.5), (33, 1, 0, 96, 0.5), (33, 1, 0, 96, 0.01),
                                                        (256, 1, 0, 32, 0.07), (37, 3, 2, 32, 0.07)])
def test_ntxent_reference_is_autograd_and_honest_emulation_passes(family, b_local, world, rank, d, temp):
    args, ref, emul = _nx_case(family, b_local, world, rank, d, temp)
    zn, zall, _, bg, off, _, gs = args
    # the reference against torch: all global rows' cross-entropy on the masked logits, differentiated by autograd in double
    za = zall.double().requires_grad_(True)
    t = float(torch.tensor(temp, dtype=F32))
    s = (za @ za.t() / t).masked_fill(torch.eye(2 * bg, dtype=torch.bool), -float("inf"))
    pos = torch.cat([torch.arange(bg, 2 * bg), torch.arange(0, bg)])
    rows_all = F.cross_entropy(s, pos, reduction="none")
    (rows_all.sum() * float(torch.tensor(gs, dtype=F32))).backward()
    mine = torch.cat([torch.arange(off, off + b_local), torch.arange(bg + off, bg + off + b_local)])
    torch.testing.assert_close(ref["loss_rows"], rows_all.detach()[mine], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["dzn"], za.grad[mine], rtol=1e-10, atol=1e-12 * ref["dzn_floor"] / lc.U)   # (collapsed: the terms cancel to 0)
    if world == 1 and b_local > 1:
        # ... and the oracle fed doubles (it normalises once more: float32 unit rows have norm 1 within 2^-23, times 1 / T)
        want = float(on.ntxent_lightly(zn[:b_local].double(), zn[b_local:].double(), t))
        assert abs(float(ref["loss_rows"].mean()) - want) <= 4 * 2.0 ** -23 / t + 1e-12
    if family == "collapsed":
        assert abs(float(ref["loss_rows"].mean()) - math.log(2 * bg - 1)) < 1e-5
    _nx_compare(_accept32, _honest(lc.ntxent, *args), ref, emul, temp,
                f"ntxent {family} b={b_local} T={temp}")


NX_ERRORS = [  # (error, tensors it must show in, (family, b_local, world, rank, d, temp))
    ("self_included", ("lse", "dzn"), ("randn", 33, 1, 0, 96, 0.5)),
    ("self_included", ("lse", "dzn"), ("offset", 256, 1, 0, 32, 0.07)),
    ("no_max", ("lse",), ("collapsed", 33, 1, 0, 96, 0.01)),
    ("no_max", ("lse",), ("duplicates", 256, 1, 0, 32, 0.01)),
    ("pos_at_rank0", ("loss_rows", "dzn"), ("randn", 37, 3, 2, 32, 0.07)),
    ("drop_last_tile", ("lse", "dzn"), ("randn", 33, 1, 0, 96, 0.5)),
    ("drop_last_tile", ("lse", "dzn"), ("collapsed", 1100, 1, 0, 32, 0.5)),
    ("drop_last_split", ("dzn",), ("randn", 1100, 1, 0, 32, 0.5)),
    ("drop_last_split", ("dzn",), ("offset", 33, 1, 0, 96, 0.07)),
    ("lse_row_only", ("dzn",), ("randn", 33, 1, 0, 96, 0.5)),
    ("lse_row_only", ("dzn",), ("duplicates", 256, 1, 0, 32, 0.01)),
    ("temp_once", ("dzn",), ("randn", 33, 1, 0, 96, 0.5)),
    ("temp_once", ("dzn",), ("antipodal", 33, 1, 0, 96, 0.07)),
]


@pytest.mark.parametrize("error,tensors,case", NX_ERRORS)
def test_ntxent_seeded_errors_fail(error, tensors, case):
    family, b_local, world, rank, d, temp = case
    args, ref, emul = _nx_case(*case)
    bad = lc.ntxent(*args, dt=F32, seed_error=error)
    floors = {"lse": lc.ntxent_lse_floor(temp, ref), "loss_rows": lc.ntxent_lse_floor(temp, ref), "dzn": ref["dzn_floor"]}
    for key in tensors:
        _reject32(bad[key], ref[key], emul[key], floors[key], f"{error} {family} b={b_local} T={temp} {key}")


def test_ntxent_launch_arithmetic_mirrors():
    """the shapes tests/test_gpu_losses.py claims paths with (the issue's table)"""
    assert lc.nx_fwd_rpw(1024) == 2 and lc.nx_fwd_rpw(1025) == 8
    assert lc.nx_bwd_plan(1, 1) == (1, 1, 1)
    assert lc.nx_bwd_plan(256, 256) == (16, 8, 1)
    assert lc.nx_bwd_plan(1025, 1025) == (65, 3, 11)
    assert lc.nx_bwd_plan(1100, 1100) == (69, 3, 12) and lc.cdiv(2200, 64) - 2 * 12 == 11 and 2200 % 64 == 24
    assert lc.nx_bwd_plan(2049, 2049) == (129, 1, 65)
    assert lc.nx_bwd_lds_bytes(256) == 107648
    assert lc.grid_blocks(4100 * 65, lc.BCE_CAP) == lc.BCE_CAP and lc.grid_blocks(730 * 730, lc.BARLOW_CAP) == lc.BARLOW_CAP
    assert lc.grid_blocks(4200 * 250, lc.CENTER_CAP) == lc.CENTER_CAP and lc.grid_blocks(16400, 1 << 30) > lc.VICREG_CAP
    assert lc.grid_blocks(300 * 3000, lc.SK_WRITE_CAP) == lc.SK_WRITE_CAP


@pytest.mark.parametrize("rows,d", [(5, 8), (3, 65), (300, 100)])
@pytest.mark.parametrize("eps", [1e-12, 1e-3])
def test_l2norm_reference_and_seeded_error(rows, d, eps):
    x, dy = lc.l2norm_inputs(rows, d, eps, seed=rows + d)
    e32 = float(torch.tensor(eps, dtype=F32))
    xr = x.double().requires_grad_(True)
    y = F.normalize(xr, dim=1, eps=e32)
    (y * dy.double()).sum().backward()
    ref = lc.l2norm(x, eps, dy, scale=1.0, dt=F64)
    assert float((ref["norm"] / e32 - 1).abs().min()) > 0.4            # no row near the clamp's switch
    torch.testing.assert_close(ref["y"], y.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(ref["dx"], xr.grad, rtol=1e-10, atol=1e-13 * float(xr.grad.abs().max()))
    live = ref["norm"] > e32
    for bf16 in (False, True):
        emul = lc.l2norm(x, eps, dy, dt=F32, y_bf16=bf16, dx_bf16=bf16)
        bad = lc.l2norm(x, eps, dy, dt=F32, y_bf16=bf16, dx_bf16=bf16, seed_error="eps_added")
        if bf16:
            with kc.jitter(3):
                got = lc.l2norm(x, eps, dy, dt=F32, y_bf16=True, dx_bf16=True)
            _accept(got["y"], ref["y"], emul["y"], "l2norm y bf16")
            _accept(got["dx"][live], ref["dx"][live], emul["dx"][live], "l2norm dx bf16")
            if eps == 1e-3:
                _reject(bad["y"], ref["y"], emul["y"], "eps_added y bf16")
        else:
            got = _honest(lc.l2norm, x, eps, dy)
            _accept32(got["y"], ref["y"], emul["y"], lc.f32_floor(ref["y"]), "l2norm y")
            _accept32(got["dx"][live], ref["dx"][live], emul["dx"][live], lc.mag_floor(ref["dx_terms"][live]), "l2norm dx")
            if eps == 1e-3:   # (at 1e-12 the added eps is below a float32 rounding of any live norm: equivalent there)
                _reject32(bad["y"], ref["y"], emul["y"], lc.f32_floor(ref["y"]), "eps_added y")
                _reject32(bad["inv_norm"][live], ref["inv_norm"][live], emul["inv_norm"][live], lc.f32_floor(ref["inv_norm"][live]),
                          "eps_added inv_norm")


@pytest.mark.parametrize("b,d,k,temp,tie", [(1, 32, 1, 0.1, False), (48, 128, 200, 0.1, True), (5, 100, 63, 0.01, False)])
def test_bank_loss_reference_and_seeded_error(b, d, k, temp, tie):
    q, kp, bank = lc.bank_inputs(b, d, k, seed=b + k, key_in_bank=tie)
    t = float(torch.tensor(temp, dtype=F32))
    qr, kr = q.double().requires_grad_(True), kp.double().requires_grad_(True)
    logits = torch.cat([(qr * kr).sum(1, keepdim=True), qr @ bank.double()], 1) / t
    F.cross_entropy(logits, torch.zeros(b, dtype=torch.long)).backward()
    ref, emul = lc.bank_loss(q, kp, bank, temp, dt=F64), lc.bank_loss(q, kp, bank, temp, dt=F32)
    want = float(on.ntxent_memory_bank(q.double(), kp.double(), bank.double(), t))
    assert abs(float(ref["terms"].sum()) - want) <= 4 * 2.0 ** -23 / t + 1e-12
    torch.testing.assert_close(ref["dq"], qr.grad, rtol=1e-10, atol=1e-14)
    torch.testing.assert_close(ref["dk"], kr.grad, rtol=1e-10, atol=1e-14)
    chain = lc.row_chain(lc.cdiv(k, 256), b)
    assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain, ref["mags"])
    bad = lc.bank_loss(q, kp, bank, temp, dt=F32, seed_error="pos_not_in_lse")
    assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain, ref["mags"])
    got = _honest(lc.bank_loss, q, kp, bank, temp)
    for key in ("dq", "dk"):
        _accept32(got[key], ref[key], emul[key], ref[key + "_floor"], f"bank {key}")
        _reject32(bad[key], ref[key], emul[key], ref[key + "_floor"], f"pos_not_in_lse {key}")


@pytest.mark.parametrize("b,d,zero", [(b, d, z) for b, d in [(1, 1), (37, 63), (37, 2048)]
                                      for z in [(), ("x0",), ("x1",), ("both",), ("x0", "x1", "both")] if b > 1 or len(z) < 2])
def test_neg_cosine_reference_and_seeded_error(b, d, zero):
    """torch clamps each norm in place under no_grad, so for 0 < |x| < eps its gradient treats the norm as unclamped while the
    kernel differentiates the clamped function; on a ZERO row (the only clamped rows the reference's models can produce, and
    the ones tested) both give x1 / (eps |x1|).  Rows with a clamped norm hold gradients of size 1 / eps: they are
    compared apart from the live rows, so that their scale does not hide the others."""
    x0, x1 = lc.neg_cosine_inputs(b, d, seed=b + d, zero=zero)
    eps = 1e-8
    e32 = float(torch.tensor(eps, dtype=F32))
    ar, br = x0.double().requires_grad_(True), x1.double().requires_grad_(True)
    (-F.cosine_similarity(ar, br, dim=1, eps=e32).mean()).backward()
    ref, emul = lc.neg_cosine(x0, x1, eps, dt=F64), lc.neg_cosine(x0, x1, eps, dt=F32)
    assert lc.neg_cosine_margin(ref, e32) > 0.9
    torch.testing.assert_close(ref["d0"], ar.grad, rtol=1e-10, atol=1e-14)
    torch.testing.assert_close(ref["d1"], br.grad, rtol=1e-10, atol=1e-14)
    live = (ref["l0"] > e32) & (ref["l1"] > e32)
    bad = lc.neg_cosine(x0, x1, eps, dt=F32, seed_error="eps_on_product")
    got = _honest(lc.neg_cosine, x0, x1, eps)
    for rows in (live, ~live):
        if not bool(rows.any()):
            continue
        for key in ("d0", "d1"):
            _accept32(got[key][rows], ref[key][rows], emul[key][rows], ref["floor"](key, rows), f"-cos {key}")
    chain = lc.row_chain(lc.cdiv(d, 64), b)
    assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain)
    if ("x0" in zero or "x1" in zero) and b > 1:      # one norm clamped, the other not: the product form differs
        key = "d0" if "x0" in zero else "d1"
        _reject32(bad[key][~live], ref[key][~live], emul[key][~live], ref["floor"](key, ~live), f"eps_on_product {key}")


@pytest.mark.parametrize("b,c", [(1, 1), (70, 9), (5, 65), (33, 1000)])
@pytest.mark.parametrize("family", ["randn", "offset+1e4", "dominant"])
def test_cross_entropy_reference_and_seeded_errors(b, c, family):
    g = torch.Generator().manual_seed(b + c)
    x = lc.logit_inputs(family, b, c, seed=b * c)
    labels = torch.randint(0, c, (b,), generator=g)
    w = torch.rand(c, generator=g) + 0.2
    w[c // 2] = 0.0
    if b > 4:
        labels[1], labels[b - 1] = -100, -100
    for weight in (None, w):
        if b == 1 and weight is not None:
            continue                                        # (C = 1 with its only weight 0: 0 / 0, as torch)
        xr = x.double().requires_grad_(True)
        F.cross_entropy(xr, labels, weight=None if weight is None else weight.double()).backward()
        ref, emul = lc.cross_entropy(x, labels, weight, dt=F64), lc.cross_entropy(x, labels, weight, dt=F32)
        torch.testing.assert_close(ref["dlogits"], xr.grad, rtol=1e-9, atol=1e-15)
        _accept32(_honest(lc.cross_entropy, x, labels, weight)["dlogits"], ref["dlogits"], emul["dlogits"], ref["floor"], "CE dlogits")
        chain = lc.row_chain(0, b)
        assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain, ref["mags"])
        if b > 4:
            bad = lc.cross_entropy(x, labels, weight, dt=F32, seed_error="ignored_counted")
            _reject32(bad["dlogits"], ref["dlogits"], emul["dlogits"], ref["floor"], "ignored_counted")
            bad = lc.cross_entropy(x, labels, weight, dt=F32, seed_error="mean_over_B")
            _reject32(bad["dlogits"], ref["dlogits"], emul["dlogits"], ref["floor"], "mean_over_B")
            if family != "dominant":   # (a dominant logit on the label leaves a loss of ~0 whatever divides it)
                assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain, ref["mags"])


@pytest.mark.parametrize("b,c", [(70, 8), (7, 5), (4100, 65)])
@pytest.mark.parametrize("family", ["randn", "saturated"])
def test_bce_reference_and_seeded_error(b, c, family):
    g = torch.Generator().manual_seed(b + c)
    x = lc.logit_inputs(family, b, c, seed=b + c)
    target = torch.rand(b, c, generator=g)
    pw = torch.rand(c, generator=g) * 3 + 0.5
    for pos_weight in (None, pw):
        xr = x.double().requires_grad_(True)
        F.binary_cross_entropy_with_logits(xr, target.double(), pos_weight=None if pos_weight is None else pos_weight.double()).backward()
        ref, emul = lc.bce_logits(x, target, pos_weight, dt=F64), lc.bce_logits(x, target, pos_weight, dt=F32)
        torch.testing.assert_close(ref["dlogits"], xr.grad, rtol=1e-9, atol=1e-16)
        floor = ref["floor"]
        _accept32(_honest(lc.bce_logits, x, target, pos_weight)["dlogits"], ref["dlogits"], emul["dlogits"], floor, "BCE dlogits")
        chain = lc.grid_chain(b * c, lc.BCE_CAP)
        assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain, ref["mags"])
        if pos_weight is not None:
            bad = lc.bce_logits(x, target, pos_weight, dt=F32, seed_error="pos_weight_by_row")
            _reject32(bad["dlogits"], ref["dlogits"], emul["dlogits"], floor, f"pos_weight_by_row {b}x{c}")
            assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain, ref["mags"])


@pytest.mark.parametrize("b,d,temp,sigma,dup", [(2, 32, 0.1, 0.5, False), (3, 100, 0.07, 0.05, False), (96, 32, 0.1, 0.5, True),
                                                 (257, 32, 0.07, 0.5, False)])
def test_dcl_reference_and_seeded_errors(b, d, temp, sigma, dup):
    z0, z1 = lc.dcl_inputs(b, d, seed=b + d, duplicates=dup)
    t, sg = float(torch.tensor(temp, dtype=F32)), float(torch.tensor(sigma, dtype=F32))
    for s_, s32 in ((None, None), (sigma, sg)):
        ref, emul = lc.dcl(z0, z1, temp, s_, dt=F64), lc.dcl(z0, z1, temp, s_, dt=F32)
        got = _honest(lc.dcl, z0, z1, temp, s_)
        r0, r1 = z0.double().requires_grad_(True), z1.double().requires_grad_(True)
        want = on.dcl_loss(r0, r1, t, s32)
        want.backward()
        # (it normalises once more: float32 unit rows have norm 1 within 2^-23, times 1 / T, and times B in the weights 2 - B softmax)
        assert abs(float(ref["terms"].sum()) - float(want.detach())) <= 8 * 2.0 ** -23 / t * max(1.0, b * 1.0 if s_ else 1.0) + 1e-12
        for key, z, r in (("dz0", z0, r0), ("dz1", z1, r1)):
            # the oracle normalises once more: its gradient is the tangent-space part of ours
            proj = ref[key] - z.double() * (ref[key] * z.double()).sum(1, keepdim=True)
            torch.testing.assert_close(proj, r.grad, rtol=1e-5, atol=1e-6 * float(r.grad.abs().max()))
            _accept32(got[key], ref[key], emul[key], ref[key + "_floor"], f"DCL {key}")
        chain = lc.row_chain(0, 2 * b)
        assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain, ref["mags"])
        errors = ["self_in_negatives"] + (["weights_differentiated", "weight_one_direction"] if s_ else [])
        for error in errors:
            bad = lc.dcl(z0, z1, temp, s_, dt=F32, seed_error=error)
            _reject32(bad["dz0"], ref["dz0"], emul["dz0"], ref["dz0_floor"], f"{error} b={b} dz0")
            if error != "weights_differentiated":     # (the weights are detached in the VALUE: that error changes the gradient only)
                assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain, ref["mags"]), error


@pytest.mark.parametrize("d", [1, 17, 256])
@pytest.mark.parametrize("diag_weight", [1.0, 0.0])
def test_barlow_reference_and_seeded_error(d, diag_weight):
    g = torch.Generator().manual_seed(d)
    n = 64
    raw = (torch.randn(d, d, generator=g) * 8 + torch.eye(d) * n).float()
    scale, lam = (n - 1) / (n * n), 5e-3
    rr = raw.double().requires_grad_(True)
    c = rr * float(torch.tensor(scale, dtype=F32))
    on_ = (torch.diagonal(c) - 1).pow(2).sum() * diag_weight
    off = (c.pow(2).sum() - torch.diagonal(c).pow(2).sum()) * float(torch.tensor(lam, dtype=F32))
    (on_ + off).backward()
    ref, emul = lc.barlow(raw, scale, lam, diag_weight, dt=F64), lc.barlow(raw, scale, lam, diag_weight, dt=F32)
    torch.testing.assert_close(ref["draw"], rr.grad, rtol=1e-10, atol=1e-16)
    assert abs(float(ref["terms"].sum()) - float(on_ + off)) <= 1e-10 * abs(float(on_ + off)) + 1e-14
    floor = ref["floor"]
    _accept32(_honest(lc.barlow, raw, scale, lam, diag_weight)["draw"], ref["draw"], emul["draw"], floor, "barlow draw")
    chain = lc.grid_chain(d * d, lc.BARLOW_CAP)
    assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain)
    bad = lc.barlow(raw, scale, lam, diag_weight, dt=F32, seed_error="lambda_on_diagonal")
    if diag_weight:
        _reject32(bad["draw"], ref["draw"], emul["draw"], floor, "lambda_on_diagonal draw")
        assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain)


@pytest.mark.parametrize("n,d", [(2, 1), (64, 256), (64, 16400)])
def test_vicreg_variance_reference_and_seeded_errors(n, d):
    vb = lc.vicreg_inputs(n, d, seed=d)
    eps = 1e-4
    ref, emul = lc.vicreg_variance(vb, n, eps, dt=F64), lc.vicreg_variance(vb, n, eps, dt=F32)
    assert lc.vicreg_margin(ref) > 0.01
    # autograd: centred columns with exactly these biased variances
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, min(d, 300), generator=g, dtype=F64)
    x = x - x.mean(0)
    x = (x / x.pow(2).mean(0).sqrt() * vb[:x.shape[1]].double().sqrt()).requires_grad_(True)
    sd = torch.sqrt(x.var(dim=0) + float(torch.tensor(eps, dtype=F32)))
    (torch.relu(1.0 - sd).sum() / d).backward()
    torch.testing.assert_close(ref["coef"][:x.shape[1]] * x.detach(), x.grad, rtol=1e-9, atol=1e-15)
    floor = lc.f32_floor(ref["coef"])
    _accept32(_honest(lc.vicreg_variance, vb, n, eps)["coef"], ref["coef"], emul["coef"], floor, "vicreg coef")
    chain = lc.grid_chain(d, lc.VICREG_CAP)
    assert lc.scalar_ok(emul["terms"].double().sum() * ONE_ULP, ref["terms"], emul["terms"], chain)
    for error in ("biased_variance", "coef_without_hinge"):
        if n == 2 and d == 1 and error == "coef_without_hinge":
            continue                                     # the only column has sd 0.5: the hinge is active (EQUIVALENT)
        bad = lc.vicreg_variance(vb, n, eps, dt=F32, seed_error=error)
        _reject32(bad["coef"], ref["coef"], emul["coef"], floor, f"{error} coef")
    bad = lc.vicreg_variance(vb, n, eps, dt=F32, seed_error="biased_variance")
    assert not lc.scalar_ok(bad["terms"].double().sum(), ref["terms"], emul["terms"], chain)
    z = kc.bf(torch.randn(n, min(d, 256), generator=torch.Generator().manual_seed(1)) + 3)
    mean = z.double().mean(0).float()
    cref, cem = lc.center_columns(z, mean, dt=F64), lc.center_columns(z, mean, dt=F32)
    with kc.jitter(5):
        _accept(lc.center_columns(z, mean, dt=F32), cref, cem, "center_columns")
    _reject(kc.bf(z.double() - mean.double().roll(1)[None, :]) if d > 1 else cem + 1, cref, cem, "centred with the neighbour's mean")


@pytest.mark.parametrize("b,k", [(1, 1), (48, 255), (48, 257), (300, 3000)])
@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("eps", [0.05, 0.02])
def test_sinkhorn_reference_and_seeded_errors(b, k, iters, eps):
    x = lc.sinkhorn_inputs(b, k, seed=b + k)
    assert float(x.abs().max()) <= 1.0
    e32 = float(torch.tensor(eps, dtype=F32))
    ref, emul = lc.sinkhorn(x, eps, iters, dt=F64), lc.sinkhorn(x, eps, iters, dt=F32)
    assert bool(torch.isfinite(emul).all())
    torch.testing.assert_close(ref, on.sinkhorn(x.double(), iters, e32), rtol=1e-9, atol=1e-300)
    if iters > 0:
        torch.testing.assert_close(ref.sum(1), torch.ones(b, dtype=F64), rtol=1e-12, atol=0)
    floor = lc.f32_floor(ref)
    _accept32(_honest(lc.sinkhorn, x, eps, iters), ref, emul, floor, "sinkhorn Q")
    if iters > 0 and b > 1:     # (B = 1: every round leaves the row's softmax; iters = 0: no round -- equivalent, see above)
        for error in ("samples_first", "one_round_short"):
            _reject32(lc.sinkhorn(x, eps, iters, dt=F32, seed_error=error), ref, emul, floor, f"{error} {b}x{k} iters={iters}")


@pytest.mark.parametrize("n,d", [(64, 256), (96, 128)])
def test_barlow_twins_module_reference_and_wiring_error(n, d):
    a, b = lc.e2e_inputs(n, d, seed=n + d)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = on.barlow_twins_loss(ar, br)
    want.backward()
    ref, emul = lc.barlow_twins_e2e(a, b), lc.barlow_twins_e2e(a, b, emulate=True)
    # (the reference takes scale, lambda and eps as the float32 values the kernels receive: 2^-24 relative each, squared in places)
    assert abs(ref["loss"] - float(want.detach())) <= 16 * lc.U * abs(float(want.detach()))
    torch.testing.assert_close(ref["dz_a"], ar.grad, rtol=0, atol=16 * lc.U * float(ar.grad.abs().max()))
    torch.testing.assert_close(ref["dz_b"], br.grad, rtol=0, atol=16 * lc.U * float(br.grad.abs().max()))
    with kc.jitter(7):
        got = lc.barlow_twins_e2e(a, b, emulate=True)
    bad = lc.barlow_twins_e2e(a, b, emulate=True, seed_error="scale_1_over_n")
    assert abs(got["loss"] - ref["loss"]) <= ref["loss_bound"] < abs(bad["loss"] - ref["loss"])
    assert abs(emul["loss"] - ref["loss"]) <= ref["loss_bound"]
    for key in ("dz_a", "dz_b"):
        _accept(got[key], ref[key], emul[key], f"BarlowTwinsLoss {key}")
        _reject(bad[key], ref[key], emul[key], f"scale_1_over_n {key}")


@pytest.mark.parametrize("n,d", [(64, 256), (96, 128)])
def test_vicreg_module_reference_and_wiring_errors(n, d):
    a, b = lc.e2e_inputs(n, d, seed=n + d, small_std=True)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = on.vicreg_loss(ar, br, eps=float(torch.tensor(1e-4, dtype=F32)))
    want.backward()
    ref, emul = lc.vicreg_e2e(a, b), lc.vicreg_e2e(a, b, emulate=True)
    # (the reference takes scale, lambda and eps as the float32 values the kernels receive: 2^-24 relative each, squared in places)
    assert abs(ref["loss"] - float(want.detach())) <= 16 * lc.U * abs(float(want.detach()))
    torch.testing.assert_close(ref["dz_a"], ar.grad, rtol=0, atol=16 * lc.U * float(ar.grad.abs().max()))
    torch.testing.assert_close(ref["dz_b"], br.grad, rtol=0, atol=16 * lc.U * float(br.grad.abs().max()))
    with kc.jitter(9):
        got = lc.vicreg_e2e(a, b, emulate=True)
    assert abs(got["loss"] - ref["loss"]) <= ref["loss_bound"] and abs(emul["loss"] - ref["loss"]) <= ref["loss_bound"]
    for key in ("dz_a", "dz_b"):
        _accept(got[key], ref[key], emul[key], f"VICRegLoss {key}")
    for error in ("cov_scale_n", "mu_not_halved"):
        bad = lc.vicreg_e2e(a, b, emulate=True, seed_error=error)
        assert abs(bad["loss"] - ref["loss"]) > ref["loss_bound"], error
        _reject(bad["dz_a"], ref["dz_a"], emul["dz_a"], f"{error} dz_a")
