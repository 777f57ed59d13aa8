"""CPU proofs for tests/f32_cases.py: on every family and shape class tests/test_gpu_f32_kernels.py uses, (1) another honest
float32 realisation of the same operation -- the emulation without fma contraction, and torch's own float32 CPU kernels
where they exist -- passes kernel_check.check under the bounds the GPU tests assert, and (2) every seeded error is rejected
on at least one named case.  The references themselves are held against torch float64 autograd."""
import f32_cases as fc
import kernel_check as kc
import pytest
import torch
import torch.nn.functional as F

SUM = kc.F32_SUM_FACTOR


def ok(got, ref, emul, factor=kc.FACTOR, **kw):
    return fc.verdict32(got, ref, emul, factor, **kw)


def test_every_switch_is_named():
    assert set(CATCHES) == {(op, sw) for op, sws in fc.SWITCHES.items() for sw in sws}


def test_check_takes_the_ulp_of_the_output_format():
    """criterion 4 counts an error in ulps of the stated format: a relative error of 2^-20 on every element is 2^-12 bf16 ulp
    (the default, unchanged) and 8 float32 ulp"""
    key = "max |err| / (a + ulp |ref|)"
    ref = torch.randn(100, generator=torch.Generator().manual_seed(0)).double()
    got = ref * (1.0 + 2.0 ** -20)
    assert abs(kc.scores(got, ref, 0.0)[key] - 2.0 ** -12) < 1e-9
    assert abs(kc.scores(got, ref, 0.0, fc.F32_ULP)[key] - 8.0) < 1e-5
    emul = ref.float().double()
    assert fc.verdict32(emul, ref, emul) and not fc.verdict32(got, ref, emul) and kc.passes(emul, ref, emul)


# ------------------------------------------------------------------------------------------------ convolution
CONV_CASES = {  # name -> (n, h, w, c, k, r, s, stride, pad)
    "3x3 M65 K5 Kd27": (1, 5, 13, 3, 5, 3, 3, 1, 1),
    "3x3/2 H7 K65": (1, 7, 7, 2, 65, 3, 3, 2, 1),
    "3x3/2 H8": (2, 8, 8, 3, 4, 3, 3, 2, 1),
    "1x1/2 H7 Kd17": (1, 7, 7, 17, 3, 1, 1, 2, 0),
    "1x3 p1": (1, 5, 6, 2, 3, 1, 3, 1, 1),
    "7x7/2 C3": (1, 12, 10, 3, 4, 7, 7, 2, 3),
}


def _conv(name, family, seed=0):
    n, h, w, c, k, r, s, stride, pad = CONV_CASES[name]
    return fc.conv_inputs(family, n, h, w, c, k, r, s, stride, pad, seed), (r, s, stride, pad, h, w)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_emulations_follow_torch(name, family):
    t, (r, s, stride, pad, h, w) = _conv(name, family)
    ref, _ = fc.conv_fwd_ref(t["x"], t["w"], stride, pad, t["bias"], fc.ACT_GELU, t["res"])
    em = fc.conv_fwd_emul(t["x"], t["w"], stride, pad, t["bias"], fc.ACT_GELU, t["res"])
    x32, w32 = _nchw(t["x"]).clone().requires_grad_(True), _nchw(t["w"]).clone().requires_grad_(True)
    y32 = F.conv2d(x32, w32, t["bias"], stride, pad)
    got = F.gelu(y32) + _nchw(t["res"])
    want = F.gelu(F.conv2d(_nchw(t["x"]).double(), _nchw(t["w"]).double(), t["bias"].double(), stride, pad)) + _nchw(t["res"]).double()
    torch.testing.assert_close(_nchw(ref), want, rtol=1e-12, atol=1e-12)
    assert ok(got.detach().permute(0, 2, 3, 1), ref, em, SUM), "torch float32 conv does not pass the forward bound"
    # gradients of the plain convolution: float64 autograd, torch float32 as the other honest kernel
    o = kc.conv_ref(t["x"], t["w"], stride, pad, dy=t["dy"])
    y32.backward(_nchw(t["dy"]))
    dxe = fc.conv_dgrad_emul(t["dy"], t["w"], h, w, stride, pad)
    dwe = fc.conv_wgrad_emul(t["x"], t["dy"], r, s, stride, pad)
    assert ok(x32.grad.permute(0, 2, 3, 1), o["dx"], dxe, SUM)
    assert ok(w32.grad.permute(0, 2, 3, 1), o["dw"], dwe, SUM, abs_floor=fc.wgrad_floor(t["x"], t["dy"], r, s, stride, pad))
    if family == "lattice":
        exact, _ = fc.conv_fwd_ref(t["x"], t["w"], stride, pad, t["bias"], fc.ACT_RELU, t["res"])
        assert torch.equal(fc.conv_fwd_emul(t["x"], t["w"], stride, pad, t["bias"], fc.ACT_RELU, t["res"]), exact)
        assert torch.equal(dxe, o["dx"]) and torch.equal(dwe, o["dw"])


def _conv_seeded(op, name, family, sw):
    t, (r, s, stride, pad, h, w) = _conv(name, family)
    if op == "conv_fwd":
        ref, _ = fc.conv_fwd_ref(t["x"], t["w"], stride, pad, t["bias"])
        return (fc.conv_fwd_emul(t["x"], t["w"], stride, pad, t["bias"], seed_error=sw), ref,
                fc.conv_fwd_emul(t["x"], t["w"], stride, pad, t["bias"]), SUM, {})
    o = kc.conv_ref(t["x"], t["w"], stride, pad, dy=t["dy"])
    if op == "conv_dgrad":
        return (fc.conv_dgrad_emul(t["dy"], t["w"], h, w, stride, pad, sw), o["dx"],
                fc.conv_dgrad_emul(t["dy"], t["w"], h, w, stride, pad), SUM, {})
    return (fc.conv_wgrad_emul(t["x"], t["dy"], r, s, stride, pad, sw), o["dw"], fc.conv_wgrad_emul(t["x"], t["dy"], r, s, stride, pad),
            SUM, {"abs_floor": fc.wgrad_floor(t["x"], t["dy"], r, s, stride, pad)})


def _linear(rows, c, k, family, sw=None):
    """a Linear layer's weight gradient: the 1 x 1 convolution on `rows` 1 x 1 images"""
    t = fc.conv_inputs(family, rows, 1, 1, c, k, 1, 1, 1, 0, rows)
    o = kc.conv_ref(t["x"], t["w"], 1, 0, dy=t["dy"])
    return (fc.conv_wgrad_emul(t["x"], t["dy"], 1, 1, 1, 0, sw), o["dw"], fc.conv_wgrad_emul(t["x"], t["dy"], 1, 1, 1, 0), SUM,
            {"abs_floor": fc.wgrad_floor(t["x"], t["dy"], 1, 1, 1, 0)})


def test_wgrad_slab_arithmetic():
    assert fc.wgrad_slabs(4096, False) == (1, 4096) and fc.wgrad_slabs(4100, False) == (2, 2050)
    assert fc.wgrad_slabs(256, True) == (1, 256) and fc.wgrad_slabs(257, True) == (2, 129) and fc.wgrad_slabs(300, True) == (2, 150)
    assert fc.wgrad_slabs(65793, True) == (256, 258) and fc.wgrad_slabs(1025 * 1025, False) == (256, 4105)


@pytest.mark.parametrize("rows", [255, 257, 300])
@pytest.mark.parametrize("family", ["lattice", "randn", "offset"])
def test_linear_weight_gradient_slabs(rows, family):
    got, ref, em, f, kw = _linear(rows, 5, 3, family)
    assert ok(got, ref, em, f, **kw)
    t = fc.conv_inputs(family, rows, 1, 1, 5, 3, 1, 1, 1, 0, rows)
    assert ok(kc.matmul_tn_f32(t["dy"].reshape(rows, 3), t["x"].reshape(rows, 5)).reshape(3, 1, 1, 5), ref, em, f, **kw), \
        "the row-order float32 product does not pass the slab bound"


def test_conv_weight_gradient_two_slabs_with_a_ragged_step():
    t = fc.conv_inputs("randn", 1, 41, 100, 2, 3, 1, 1, 1, 0, 5)
    o = kc.conv_ref(t["x"], t["w"], 1, 0, dy=t["dy"])
    em = fc.conv_wgrad_emul(t["x"], t["dy"], 1, 1, 1, 0)
    kw = {"abs_floor": fc.wgrad_floor(t["x"], t["dy"], 1, 1, 1, 0)}
    assert ok(em, o["dw"], em, SUM, **kw)
    for sw in fc.WGRAD_SWITCHES:
        assert not ok(fc.conv_wgrad_emul(t["x"], t["dy"], 1, 1, 1, 0, sw), o["dw"], em, SUM, **kw), sw


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn(family, rows, c, groups, relu, res, eps=1e-5, sw=None, seed=0):
    t = fc.bn_inputs(family, rows, c, groups, seed)
    run = (t["running_mean"], t["running_var"])
    r = t["residual"] if res else None
    ref = kc.bn_forward_ref(t["y"], r, t["gamma"], t["beta"], groups, eps, 0.1, relu, running=run)
    em = fc.bn_fwd_emul(t["y"], r, t["gamma"], t["beta"], groups, eps, 0.1, relu, running=run)
    got = fc.bn_fwd_emul(t["y"], r, t["gamma"], t["beta"], groups, eps, 0.1, relu, running=run, seed_error=sw)
    return t, ref, em, got


def _bn_fwd_ok(t, ref, em, got):
    fl = fc.bn_fwd_floors(t, ref)
    return all(ok(got[k], ref[k], em[k], abs_floor=fl[k], floor_all=True, floor_cosine=k == "out") for k in fl)


BN_SHAPES = [(2, 5, 2), (2, 1, 1), (4, 5, 2), (14, 33, 2), (18, 31, 1), (1026, 3, 2), (1000, 7, 1)]


@pytest.mark.parametrize("family", fc.BN_FAMILIES)
@pytest.mark.parametrize("rows,c,groups", BN_SHAPES)
def test_bn_forward_without_contraction_passes(family, rows, c, groups):
    eps = fc.bn_eps(family, rows // groups)
    for relu, res in ((False, False), (True, True)):
        t, ref, em, _ = _bn(family, rows, c, groups, relu, res, eps)
        with fc.uncontracted():
            other = fc.bn_fwd_emul(t["y"], t["residual"] if res else None, t["gamma"], t["beta"], groups, eps, 0.1, relu,
                                   running=(t["running_mean"], t["running_var"]))
        assert _bn_fwd_ok(t, ref, em, other)
        if family == "randn" and rows // groups > 1:
            # and torch's float32 batch_norm, group by group
            rm, rv = t["running_mean"].clone(), t["running_var"].clone()
            outs = [F.batch_norm(p, rm, rv, t["gamma"], t["beta"], True, 0.1, eps) for p in t["y"].chunk(groups)]
            o = torch.cat(outs) + (t["residual"] if res else 0.0)
            tt = {"out": F.relu(o) if relu else o, "mean": ref["mean"], "invstd": ref["invstd"], "running_mean": rm, "running_var": rv}
            assert _bn_fwd_ok(t, ref, em, tt)


def _bn_bwd(family, rows, c, groups, relu, sw=None):
    t, _, em, _ = _bn(family, rows, c, groups, relu, True, fc.bn_eps(family, rows // groups))
    out = em["out"] if relu else None
    a = (t["y"], t["dout"], out, t["gamma"], em["mean"], em["invstd"], groups)
    ref = kc.bn_backward_ref(t["y"], t["dout"], t["gamma"], t["beta"], em["mean"], em["invstd"], groups, out_relu=out)
    return ref, fc.bn_bwd_emul(*a), fc.bn_bwd_emul(*a, seed_error=sw), a


def bn_bwd_ok(ref, em, got):
    fl = {"dgamma": kc.f32_sum_floor(em["terms"][1]), "dbeta": kc.f32_sum_floor(em["terms"][0])}
    fd = {"abs_floor": max(fc.elem_floor(ref["dy"]), em["dy_floor"]), "floor_all": True, "floor_cosine": True}
    return (ok(got["dy"], ref["dy"], em["dy"], **fd) and ok(got["dz"], ref["dz"], em["dz"]) and
            all(ok(got[k], ref[k], em[k], abs_floor=fl[k]) for k in fl))


@pytest.mark.parametrize("family", ["lattice", "randn", "offset", "big_value"])
@pytest.mark.parametrize("rows,c,groups", BN_SHAPES)
def test_bn_backward_without_contraction_passes(family, rows, c, groups):
    for relu in (False, True):
        ref, em, _, a = _bn_bwd(family, rows, c, groups, relu)
        with fc.uncontracted():
            other = fc.bn_bwd_emul(*a)
        assert bn_bwd_ok(ref, em, other)


def test_bn_references_follow_torch_autograd():
    t = fc.bn_inputs("randn", 64, 6, 2, 3)
    y = t["y"].double().requires_grad_(True)
    gamma, beta = t["gamma"].double().requires_grad_(True), t["beta"].double().requires_grad_(True)
    outs = [F.batch_norm(p, None, None, gamma, beta, True, 0.1, 1e-5) for p in y.chunk(2)]
    out = F.relu(torch.cat(outs) + t["residual"].double())
    out.backward(t["dout"].double())
    ref = kc.bn_forward_ref(t["y"], t["residual"], t["gamma"], t["beta"], 2, 1e-5, 0.1, True)
    torch.testing.assert_close(ref["out"], out.detach(), rtol=1e-9, atol=1e-9)
    b = kc.bn_backward_ref(t["y"], t["dout"], t["gamma"], t["beta"], ref["mean"], ref["invstd"], 2, out_relu=ref["out"])
    for k, want in (("dy", y.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        torch.testing.assert_close(b[k], want, rtol=1e-7, atol=1e-9)


def test_bn_eval_emulation():
    t = fc.bn_inputs("randn", 30, 9, 1, 1)
    ref = kc.bn_eval_ref(t["y"], t["residual"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], 1e-5, True)["out"]
    em = fc.bn_eval_emul(t["y"], t["residual"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], 1e-5, True)
    got = F.relu(F.batch_norm(t["y"], t["running_mean"], t["running_var"], t["gamma"], t["beta"], False, 0.1, 1e-5) + t["residual"])
    assert ok(got, ref, em)


# ------------------------------------------------------------------------------------------------ pooling, GAP, column sums
@pytest.mark.parametrize("family", fc.POOL_FAMILIES)
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 3), (7, 8), (8, 7), (14, 14)])
def test_pool_reference_is_torch_on_untied_positions(family, h, w):
    x, dy = fc.pool_inputs(family, 2, h, w, 3, h * 16 + w)
    y, dx = fc.maxpool_fwd_bwd(x, dy)
    assert torch.equal(y, F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.permute(0, 3, 1, 2).double())
    assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1))
    assert float(dx.sum()) == float(dy.sum())        # every window gives its gradient to exactly one element


def test_gap_and_colsum_emulations():
    x = fc.offset_rows(4 * 50, 7, 1).reshape(4, 50, 7)
    assert ok(fc.gap_emul(x), x.double().mean(1), fc.gap_emul(x))
    assert not ok(fc.gap_emul(x, "hw_minus_1"), x.double().mean(1), fc.gap_emul(x))
    dy = fc.offset_rows(4, 7, 2)
    assert ok((dy / 50).unsqueeze(1).expand(-1, 50, -1), (dy.double() / 50).unsqueeze(1).expand(-1, 50, -1), fc.gap_bwd_emul(dy, 50))
    r = fc.offset_rows(1000, 5, 3)
    kw = {"abs_floor": kc.f32_sum_floor(r)}
    assert ok(fc.colsum_emul(r), r.double().sum(0), fc.colsum_emul(r), **kw)    # (the kernel sums in double: no float32 sum is a stand-in)
    assert not ok(fc.colsum_emul(r, "last_row"), r.double().sum(0), fc.colsum_emul(r), **kw)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln(family, rows, c, eps, sw=None):
    x, gamma, beta, dy, _ = fc.ln_inputs(family, rows, c, c + rows)
    e = fc.f32c(eps)
    ref = kc.layer_norm_ref(x, gamma, beta, e, dy)
    return (x, gamma, beta, dy), ref, fc.ln_emul(x, gamma, beta, eps, dy), fc.ln_emul(x, gamma, beta, eps, dy, sw)


def ln_ok(a, ref, em, got):
    x, gamma, beta, dy = a
    xh = (ref[0] - beta.double()) / gamma.double()
    fl = (kc.f32_sum_floor(dy.double() * xh), kc.f32_sum_floor(dy))
    el = [{"abs_floor": fc.elem_floor(ref[i]), "floor_all": True} for i in (0, 1)]
    return (ok(got[0], ref[0], em[0], **el[0]) and ok(got[1], ref[1], em[1], **el[1]) and ok(got[2], ref[2], em[2], abs_floor=fl[0]) and
            ok(got[3], ref[3], em[3], abs_floor=fl[1]))


@pytest.mark.parametrize("family", kc.LN_FAMILIES)
@pytest.mark.parametrize("c", [1, 8, 63, 64, 65, 192])
@pytest.mark.parametrize("eps", [1e-6, 1e-12])
def test_layernorm_without_contraction_passes(family, c, eps):
    a, ref, em, _ = _ln(family, 3, c, eps)
    with fc.uncontracted():
        other = fc.ln_emul(*a[:3], eps, a[3])
    assert ln_ok(a, ref, em, other)
    if family == "randn" and c >= 63:     # (torch takes the statistics in float32; over 8 columns that, not the chain, is its error)
        x = a[0].clone().requires_grad_(True)
        F.layer_norm(x, (c,), a[1], a[2], eps).backward(a[3])
        assert ok(x.grad, ref[1], em[1], abs_floor=fc.elem_floor(ref[1]), floor_all=True), "torch float32 LayerNorm backward does not pass the dx bound"


# ------------------------------------------------------------------------------------------------ bias / activation
@pytest.mark.parametrize("act", [fc.ACT_NONE, fc.ACT_GELU, fc.ACT_RELU])
def test_bias_act_without_contraction_and_torch_pass(act):
    with kc.float32_inputs():
        x = kc.act_grid(40, 33, 1)
    g = torch.Generator().manual_seed(2)
    bias, res, dy = torch.randn(33, generator=g) * 0.1, torch.randn(40, 33, generator=g), torch.randn(40, 33, generator=g)
    for b, r in ((None, None), (bias, res)):
        ref = kc.bias_act_ref(x, b, act, r, dy)
        em = fc.bias_act_emul(x, b, act, r, dy)
        with fc.uncontracted():
            other = fc.bias_act_emul(x, b, act, r, dy)
        fl = kc.f32_sum_floor(ref[1])
        el = [{"abs_floor": fc.elem_floor(ref[i]), "floor_all": True} for i in (0, 1)]
        assert ok(other[0], ref[0], em[0], **el[0]) and ok(other[1], ref[1], em[1], **el[1]) and ok(other[2], ref[2], em[2], abs_floor=fl)
        if act == fc.ACT_RELU and b is None:
            assert torch.equal(em[0], ref[0]) and torch.equal(em[1], ref[1])
        # (torch's own float32 GELU is no stand-in here: its vectorised erf is several ulp of 1 off near |erf| = 1, where
        # 1 + erf cancels: 7.5e-7 at v = -2.99 against the 0.9e-7 of a correctly rounded erf)


# ------------------------------------------------------------------------------------------------ attention
def _attn(family, b, s, h, hd, scale=None, sw=None, bwd=True):
    qkv, dout = fc.attn_inputs(family, b, s, h, hd, s * hd, scale)
    sc = hd ** -0.5 if scale is None else scale
    ro, _, rg = kc.attention_ref(qkv, fc.f32c(sc), dout if bwd else None)
    eo, eg = fc.attention_emul(qkv, sc, dout if bwd else None)
    go, gg = fc.attention_emul(qkv, sc, dout if bwd else None, sw) if sw else (eo, eg)
    return (qkv, dout, sc), (ro, rg), (eo, eg), (go, gg)


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("s,hd", [(1, 32), (17, 32), (17, 64), (65, 64)])
def test_attention_torch_float32_passes(family, s, hd):
    (qkv, dout, sc), (ro, rg), (eo, eg), _ = _attn(family, 1, s, 2, hd)
    x = qkv.clone().requires_grad_(True)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))
    out = (torch.softmax((q @ k.transpose(-2, -1)) * sc, -1) @ v).transpose(1, 2)
    out.backward(dout)
    assert ok(out.detach(), ro, eo, SUM), "torch float32 attention does not pass the forward bound"
    assert ok(x.grad, rg, eg, SUM), "torch float32 attention does not pass the backward bound"


# ------------------------------------------------------------------------------------------------ softmax, pair CE, reduce, losses
@pytest.mark.parametrize("family", ["randn", "big", "constant"])
@pytest.mark.parametrize("d", [1, 255, 256, 257, 2048])
def test_softmax_emulation_and_what_the_contraction_buys(family, d):
    """The yardstick is the CONTRACTED form expf(fma(x - sub, 1 / T, -m)): every exponent is then the exact product minus one common
    m, whose own rounding cancels in the normalisation.  The form that rounds the product first (torch's float32 softmax does) is
    2 .. 200 times further from float64 on these rows (1 / T = 25 puts the logits at hundreds to thousands, half an ulp of which is
    1e-5 .. 1e-4 in the exponent) and does NOT pass these bounds: a build that loses the contraction is a finding here."""
    x, sub = fc.softmax_inputs(family, 3, d, d)
    key = "relative RMS error"
    for s in (None, sub):
        for it in (1 / 0.04, 1 / 0.1):
            for log in (False, True):
                ref, em = fc.softmax_ref(x, s, it, log), fc.softmax_emul(x, s, it, log)
                assert ok(em, ref, em, abs_floor=fc.elem_floor(ref), floor_all=True)
                with fc.uncontracted():
                    un = fc.softmax_emul(x, s, it, log)
                z = (x - (s if s is not None else 0.0)) * torch.tensor(it)
                tt = torch.log_softmax(z, -1) if log else torch.softmax(z, -1)
                if family == "big" and d >= 255 and s is None and not log:
                    assert kc.scores(un, ref)[key] > kc.scores(em, ref)[key]
                    assert kc.scores(tt, ref)[key] > kc.scores(em, ref)[key]


def _pair_ce(tv, sv, b, d, onehot, sw=None):
    g = torch.Generator().manual_seed(tv * 1000 + sv * 100 + b * 10 + d)
    logq = torch.log_softmax(torch.randn(sv * b, d, generator=g) * 3, -1)
    if onehot:
        probs = F.one_hot(torch.randint(0, d, (tv * b,), generator=g), d).float()
    else:
        probs = torch.softmax(torch.randn(tv * b, d, generator=g) * 3, -1)
    ref = fc.pair_ce_emul(probs, logq, tv, sv, b, rnd=lambda t: t)
    return (probs, logq), ref, fc.pair_ce_emul(probs, logq, tv, sv, b), fc.pair_ce_emul(probs, logq, tv, sv, b, sw)


def test_pair_ce_one_hot_is_exact():
    """one-hot probabilities: pair (t, s, b) is exactly -logq[s, b, d(t, b)], 0 on the diagonal"""
    (probs, logq), ref, em, _ = _pair_ce(2, 4, 3, 257, True)
    hot = probs.argmax(-1).reshape(2, 3)
    want = torch.stack([torch.stack([torch.stack([-logq.reshape(4, 3, 257)[s, b, hot[t, b]] * (t != s) for b in range(3)])
                                     for s in range(4)]) for t in range(2)]).reshape(-1)
    assert torch.equal(em.float(), want.float() + 0.0)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reduce_emulation_is_the_float64_sum(n, mode):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g) + 3, torch.randn(n, generator=g)
    d = a.double() - b.double()
    want = (a.double().sum(), (d * d).sum(), d.abs().sum())[mode] * (1.0 / n)
    ref = fc.reduce_emul(a, b, mode, 1.0 / n, rnd=lambda t: t)
    torch.testing.assert_close(ref, want, rtol=1e-13, atol=0)
    assert float(fc.reduce_emul(a, b, mode, 1.0 / n)) == float(ref.float())


def _loss_bwd(mode, n, sw=None):
    g = torch.Generator().manual_seed(n)
    p, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    t[::7] = p[::7]                                   # exact zeros in pred - target
    ref = fc.loss_bwd_ref(p, t, mode, 1.0 / n, 1.7)
    return ref, fc.loss_bwd_emul(p, t, mode, 1.0 / n, 1.7), fc.loss_bwd_emul(p, t, mode, 1.0 / n, 1.7, sw)


def test_loss_bwd_and_center_update_emulations():
    for mode in (1, 2):
        for n in (255, 257):
            ref, em, _ = _loss_bwd(mode, n)
            assert ok(em, ref, em)
            assert bool((em[::7] == 0).all())
    g = torch.Generator().manual_seed(0)
    c, t = torch.randn(257, generator=g), torch.randn(16, 257, generator=g)
    for m in (0.0, 0.9, 1.0):
        ref, em = fc.center_update_ref(c, t, m), fc.center_update_emul(c, t, m)
        with fc.uncontracted():
            assert ok(fc.center_update_emul(c, t, m), ref, em, abs_floor=kc.f32_stat_floor(c, t), floor_all=True)


def test_dino_loss_reference_is_lightly_formula():
    g = torch.Generator().manual_seed(0)
    sv, tv, b, d = 4, 2, 3, 257
    student, probs = torch.randn(sv * b, d, generator=g), torch.softmax(torch.randn(tv * b, d, generator=g) * 2, -1)
    logq = torch.log_softmax(student.double() * fc.f32c(1 / 0.1), -1)
    logq, p = logq.reshape(sv, b, d), probs.double().reshape(tv, b, d)
    terms = [-(p[t] * logq[s]).sum(-1).mean() for t in range(tv) for s in range(sv) if s != t]
    want = sum(terms) / len(terms)
    ref, em = fc.dino_loss_ref(student, probs, sv, tv, b, 0.1), fc.dino_loss_ref(student, probs, sv, tv, b, 0.1, emulate=True)
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=0)
    assert abs(float(em) - float(ref)) <= 4 * fc.F32_ULP * abs(float(ref))


# ------------------------------------------------------------------------------------------------ seeded errors
def _seeded_conv(op, name, family):
    return lambda sw: _conv_seeded(op, name, family, sw)


def _seeded_bn_fwd(family, rows, c, groups, eps, key):
    def run(sw):
        t, ref, em, got = _bn(family, rows, c, groups, True, True, eps, sw)
        fl = fc.bn_fwd_floors(t, ref)
        return got[key], ref[key], em[key], kc.FACTOR, {"abs_floor": fl[key], "floor_all": True, "floor_cosine": key == "out"}
    return run


def _seeded_bn_bwd(family, rows, c, groups, key):
    def run(sw):
        ref, em, got, _ = _bn_bwd(family, rows, c, groups, True, sw)
        kw = {"abs_floor": max(fc.elem_floor(ref["dy"]), em["dy_floor"]), "floor_all": True, "floor_cosine": True} if key == "dy" else {}
        return got[key], ref[key], em[key], kc.FACTOR, kw
    return run


def _seeded_pool(family, h, w, key):
    def run(sw):
        x, dy = fc.pool_inputs(family, 2, h, w, 3, 5)
        ref, got = fc.maxpool_fwd_bwd(x, dy), fc.maxpool_fwd_bwd(x, dy, sw)
        return got[key], ref[key], ref[key], kc.FACTOR, {"exact": True}
    return run


def _seeded_ln(family, c, eps, key):
    def run(sw):
        _, ref, em, got = _ln(family, 3, c, eps, sw)
        return got[key], ref[key], em[key], kc.FACTOR, ({"abs_floor": fc.elem_floor(ref[key]), "floor_all": True} if key < 2 else {})
    return run


def _seeded_attn(family, s, hd, key, bwd=True, scale=None):
    def run(sw):
        _, ref, em, got = _attn(family, 1, s, 1, hd, scale, sw, bwd)
        return got[key], ref[key], em[key], SUM, {}
    return run


def _seeded_softmax(sw):
    x, sub = fc.softmax_inputs("randn", 3, 257, 1)
    return fc.softmax_emul(x, sub, 10.0, True, sw), fc.softmax_ref(x, sub, 10.0, True), fc.softmax_emul(x, sub, 10.0, True), kc.FACTOR, {}


def _seeded_pair_ce(tv, sv, b, d, onehot):
    def run(sw):
        _, ref, em, got = _pair_ce(tv, sv, b, d, onehot, sw)
        return got, ref, em, kc.FACTOR, {}
    return run


def _seeded_reduce(mode):
    def run(sw):
        g = torch.Generator().manual_seed(mode)
        a, b = torch.randn(1025, generator=g) + 3, torch.randn(1025, generator=g)
        ref = fc.reduce_emul(a, b, mode, 1 / 1025, rnd=lambda t: t)
        return fc.reduce_emul(a, b, mode, 1 / 1025, sw).reshape(1), ref.reshape(1), fc.reduce_emul(a, b, mode, 1 / 1025).reshape(1), kc.FACTOR, {}
    return run


def _seeded_bias_act(act, key):
    def run(sw):
        with kc.float32_inputs():
            x = kc.act_grid(40, 33, 1)
        g = torch.Generator().manual_seed(2)
        bias, dy = torch.randn(33, generator=g) * 0.1, torch.randn(40, 33, generator=g)
        b = None if sw == "relu_ge_zero" else bias            # (exact zeros of x stay exact zeros without a bias)
        ref = kc.bias_act_ref(x, b, act, None, dy)[key]
        return (fc.bias_act_emul(x, b, act, None, dy, sw)[key], ref, fc.bias_act_emul(x, b, act, None, dy)[key], kc.FACTOR,
                {"abs_floor": fc.elem_floor(ref), "floor_all": True})
    return run


def _seeded_colsum(sw):
    r = fc.offset_rows(1000, 5, 3)
    return fc.colsum_emul(r, sw), r.double().sum(0), fc.colsum_emul(r), kc.FACTOR, {"abs_floor": kc.f32_sum_floor(r)}


def _seeded_gap(sw):
    x = fc.offset_rows(4 * 50, 7, 1).reshape(4, 50, 7)
    return fc.gap_emul(x, sw), x.double().mean(1), fc.gap_emul(x), kc.FACTOR, {}


def _seeded_center(sw):
    g = torch.Generator().manual_seed(0)
    c, t = torch.randn(257, generator=g), torch.randn(16, 257, generator=g)
    return (fc.center_update_emul(c, t, 0.9, sw), fc.center_update_ref(c, t, 0.9), fc.center_update_emul(c, t, 0.9), kc.FACTOR,
            {"abs_floor": kc.f32_stat_floor(c, t), "floor_all": True})


def _seeded_loss_bwd(sw):
    ref, em, got = _loss_bwd(2, 257, sw)
    return got, ref, em, kc.FACTOR, {}


# (entry point, switch) -> the named cases that must reject it
CATCHES = {
    ("conv_fwd", "drop_m_tail"): [_seeded_conv("conv_fwd", "3x3 M65 K5 Kd27", "randn"), _seeded_conv("conv_fwd", "3x3 M65 K5 Kd27", "lattice")],
    ("conv_fwd", "drop_k_tail"): [_seeded_conv("conv_fwd", "3x3/2 H7 K65", "randn")],
    ("conv_fwd", "drop_red_tail"): [_seeded_conv("conv_fwd", "3x3 M65 K5 Kd27", "offset"), _seeded_conv("conv_fwd", "1x1/2 H7 Kd17", "lattice")],
    ("conv_fwd", "rs_swapped"): [_seeded_conv("conv_fwd", "1x3 p1", "lattice"), _seeded_conv("conv_fwd", "1x3 p1", "randn")],
    ("conv_dgrad", "no_divisibility"): [_seeded_conv("conv_dgrad", "3x3/2 H7 K65", "lattice"), _seeded_conv("conv_dgrad", "3x3/2 H8", "randn"),
                                        _seeded_conv("conv_dgrad", "1x1/2 H7 Kd17", "lattice")],
    ("conv_dgrad", "drop_m_tail"): [_seeded_conv("conv_dgrad", "3x3 M65 K5 Kd27", "randn")],
    ("conv_wgrad", "slab_overrun"): [lambda sw: _linear(300, 5, 3, "randn", sw), lambda sw: _linear(257, 5, 3, "lattice", sw)],
    ("conv_wgrad", "last_slab_dropped"): [lambda sw: _linear(257, 5, 3, "randn", sw), lambda sw: _linear(300, 5, 3, "offset", sw)],
    ("bn_fwd", "var_unclamped"): [_seeded_bn_fwd("constant", 1000, 31, 1, 1e-12, "invstd")],
    ("bn_fwd", "running_var_biased"): [_seeded_bn_fwd("randn", 14, 33, 2, 1e-5, "running_var"), _seeded_bn_fwd("randn", 1026, 3, 2, 1e-5, "running_var")],
    ("bn_fwd", "groups_share_stats"): [_seeded_bn_fwd("offset", 14, 33, 2, 1e-5, "out"), _seeded_bn_fwd("lattice", 1000, 7, 2, 0.0, "out")],
    ("bn_bwd", "mask_ge_zero"): [_seeded_bn_bwd("randn", 14, 33, 2, "dz"), _seeded_bn_bwd("lattice", 18, 31, 1, "dy"),
                                 _seeded_bn_bwd("randn", 14, 33, 2, "dbeta")],
    ("bn_bwd", "dz_unmasked"): [_seeded_bn_bwd("randn", 1026, 3, 2, "dz"), _seeded_bn_bwd("offset", 14, 33, 2, "dgamma")],
    ("bn_bwd", "groups_share_stats"): [_seeded_bn_bwd("offset", 14, 33, 2, "dy"), _seeded_bn_bwd("randn", 1026, 3, 2, "dgamma")],
    ("maxpool", "last_max"): [_seeded_pool("three_level", 7, 7, 1), _seeded_pool("post_relu", 3, 3, 1), _seeded_pool("all_equal", 7, 7, 1)],
    ("maxpool", "zero_pad"): [_seeded_pool("all_negative", 7, 8, 0), _seeded_pool("all_negative", 2, 2, 1), _seeded_pool("neg_inf_plane", 8, 7, 0)],
    ("layernorm", "eps_dropped"): [_seeded_ln("constant", 64, 1e-6, 0), _seeded_ln("tight", 8, 1e-5, 0), _seeded_ln("tight", 8, 1e-5, 1)],
    ("layernorm", "tail_dropped"): [_seeded_ln("mean300", 65, 1e-6, 0), _seeded_ln("randn", 63, 1e-6, 1), _seeded_ln("randn", 192 + 8, 1e-6, 2)],
    ("attention", "no_max"): [_seeded_attn("offset+80", 17, 32, 0, False), _seeded_attn("offset+80", 17, 64, 1)],
    ("attention", "first_stride_only"): [_seeded_attn("randn", 257, 32, 0, False), _seeded_attn("randn", 65, 64, 1)],
    ("attention", "dk_noscale"): [_seeded_attn("randn", 17, 32, 1), _seeded_attn("v_offset", 17, 64, 1)],
    ("softmax", "subtract_ignored"): [_seeded_softmax],
    ("pair_ce", "diag_not_zeroed"): [_seeded_pair_ce(2, 2, 1, 257, False), _seeded_pair_ce(2, 4, 3, 257, True)],
    ("pair_ce", "decode_order"): [_seeded_pair_ce(2, 4, 3, 257, True), _seeded_pair_ce(2, 2, 3, 257, False)],
    ("reduce", "tail_dropped"): [_seeded_reduce(0), _seeded_reduce(1), _seeded_reduce(2)],
    ("loss_bwd", "l1_sign_at_zero"): [_seeded_loss_bwd],
    ("bias_act", "relu_ge_zero"): [_seeded_bias_act(fc.ACT_RELU, 1)],
    ("bias_act", "bias_row0"): [_seeded_bias_act(fc.ACT_GELU, 0), _seeded_bias_act(fc.ACT_NONE, 0)],
    ("colsum", "last_row"): [_seeded_colsum],
    ("gap", "hw_minus_1"): [_seeded_gap],
    ("center_update", "momentum_swapped"): [_seeded_center],
}


@pytest.mark.parametrize("op,switch", list(CATCHES), ids=[f"{o}-{s}" for o, s in CATCHES])
def test_seeded_error_is_rejected(op, switch):
    for case in CATCHES[(op, switch)]:
        got, ref, em, factor, kw = case(switch)
        if kw.pop("exact", False):
            assert not torch.equal(got.double(), ref.double()), f"{op} / {switch}: the seeded result equals the reference"
            continue
        assert ok(em, ref, em, factor, **kw)                                    # the same case passes unseeded
        assert not ok(got, ref, em, factor, **kw), f"{op} / {switch} passes the bound"
