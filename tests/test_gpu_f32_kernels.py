"""GPU: every wm_f32_* entry point of csrc/f32path.hip (the float32 "parity" preset, f32path.py) against a float64 reference on
the same float32 inputs, one section per entry point.

No bound here is a number taken from a run of the kernels: a comparison is either exact (torch.equal against float64 on inputs
whose every product and partial sum is a float32 number), or kernel_check.check with one float32 ulp, whose four bounds are a
factor times the score of the CPU emulation (tests/f32_cases.py) on the same input -- FACTOR for element-wise outputs and double
sums, F32_SUM_FACTOR for float32 chains over a reduction -- with the derived float32 rounding floors where the emulation can
land on the exact value.  tests/test_f32_cases_cpu.py proves on the CPU that these bounds admit the other honest float32
realisations and reject every seeded error.  Shapes are the smallest at which each kernel takes another path: ragged 64 x 64 x 16
tiles, slab edges of the weight gradient, empty row slices of the BatchNorm sums, the query strides and the LDS gate of the
attention kernels, ties in every pooling window, and the grid-stride loops beyond the 65535-block cap."""
import f32_cases as fc
import kernel_check as kc
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM = kc.F32_SUM_FACTOR
WM_EUNSUPPORTED = -2


def f32path():
    from ssl_wafermap_amd import f32path as m

    return m


def dev(t, grad=False):
    if t is None:
        return None
    d = t.detach().to(DEV)
    return d.requires_grad_(True) if grad else d


def nchw(t):
    """kernel_check's [N, H, W, C] (or [K, R, S, C]) -> the logical [N, C, H, W] view torch modules pass"""
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.detach().cpu().permute(0, 2, 3, 1)


def elem(ref):
    return {"abs_floor": fc.elem_floor(ref), "floor_all": True}


# ------------------------------------------------------------------------------------------------ convolution
def run_conv(t, stride, pad, bias=False, act=fc.ACT_NONE, res=False, grads=True):
    """f32path.conv2d on kernel_check's layouts -> dict(y, dx, dw, db, dres) on the CPU"""
    x, w = dev(nchw(t["x"]), grads), dev(nchw(t["w"]), grads)
    b, r = dev(t["bias"] if bias else None, grads), dev(nchw(t["res"]) if res else None, grads)
    y = f32path().conv2d(x, w, stride, pad, bias=b, act=act, residual=r)
    out = {"y": nhwc(y)}
    if grads:
        y.backward(dev(nchw(t["dy"])))
        out.update(dx=nhwc(x.grad), dw=nhwc(w.grad), db=b.grad.cpu() if bias else None, dres=nhwc(r.grad) if res else None)
    return out


EXACT_CONVS = {  # name -> (n, h, w, c, k, r, s, stride, pad): M = 63 / 64 / 65, K = 1 / 63 / 64 / 65, R S C = 15 / 16 / 17 / 27 / 147
    "M63 K1 RSC15": (1, 9, 7, 15, 1, 1, 1, 1, 0),
    "M64 K63 RSC16": (1, 8, 8, 16, 63, 1, 1, 1, 0),
    "M65 K64 RSC17": (1, 5, 13, 17, 64, 1, 1, 1, 0),
    "M65 K65 RSC27 3x3/1": (1, 5, 13, 3, 65, 3, 3, 1, 1),
    "3x3/2 H7": (2, 7, 7, 4, 6, 3, 3, 2, 1),
    "3x3/2 H8": (2, 8, 8, 4, 6, 3, 3, 2, 1),
    "1x1/2 H7": (2, 7, 7, 5, 3, 1, 1, 2, 0),
    "1x1/2 H8": (2, 8, 8, 5, 3, 1, 1, 2, 0),
    "7x7/2 C3 20x24": (2, 20, 24, 3, 8, 7, 7, 2, 3),
}


@pytest.mark.parametrize("name", list(EXACT_CONVS))
def test_conv_lattice_is_exact(name):
    """integers in -2 .. 2, weights in {-1, 0, 1}: every sum stays below 2^24, so y, dx and dw equal float64 bit for bit"""
    n, h, w, c, k, r, s, stride, pad = EXACT_CONVS[name]
    t = fc.conv_inputs("lattice", n, h, w, c, k, r, s, stride, pad, 1)
    ref = kc.conv_ref(t["x"], t["w"], stride, pad, dy=t["dy"])
    assert float(ref["cols"].abs().sum(1).max() * 2) < 2.0 ** 24
    got = run_conv(t, stride, pad)
    for key in ("y", "dx", "dw"):
        assert torch.equal(got[key].double(), ref[key]), f"{name}: {key} differs from float64"


def test_conv_1x3_tap_decode_at_the_c_api():
    """R != S (no module of the models has it): 1 x 3, pad 1 -- an (r, s) decode that mixes the two up reads other pixels"""
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd._lib import check, ptr, stream_ptr

    n, h, w, c, k, r, s, stride, pad = 2, 5, 6, 2, 3, 1, 3, 1, 1
    t = fc.conv_inputs("lattice", n, h, w, c, k, r, s, stride, pad, 2)
    p, q = kc.conv_out_hw(h, w, r, s, stride, pad)
    ref = kc.conv_ref(t["x"], t["w"], stride, pad, dy=t["dy"])
    lib = _lib.load()
    x, wt, dy = dev(t["x"].contiguous()), dev(nchw(t["w"]).contiguous()), dev(t["dy"].contiguous())
    y, dx, dw = torch.empty(n, p, q, k, device=DEV), torch.empty(n, h, w, c, device=DEV), torch.empty(k, c, r, s, device=DEV)
    ws = torch.empty(max(lib.wm_f32_conv2d_workspace_bytes(c, k, r, s), lib.wm_f32_conv2d_wgrad_workspace_bytes(n, p, q, c, k, r, s)),
                     dtype=torch.uint8, device=DEV)
    check(lib.wm_f32_conv2d_fwd(ptr(x), ptr(wt), 0, 0, ptr(y), n, h, w, c, k, r, s, p, q, stride, pad, 0, ptr(ws), ws.numel(),
                                stream_ptr()), "wm_f32_conv2d_fwd")
    check(lib.wm_f32_conv2d_dgrad(ptr(dy), ptr(wt), ptr(dx), n, h, w, c, k, r, s, p, q, stride, pad, ptr(ws), ws.numel(),
                                  stream_ptr()), "wm_f32_conv2d_dgrad")
    check(lib.wm_f32_conv2d_wgrad(ptr(dy), ptr(x), ptr(dw), n, h, w, c, k, r, s, p, q, stride, pad, ptr(ws), ws.numel(),
                                  stream_ptr()), "wm_f32_conv2d_wgrad")
    assert torch.equal(y.cpu().double(), ref["y"]) and torch.equal(dx.cpu().double(), ref["dx"])
    assert torch.equal(nhwc(dw).double(), ref["dw"])
    assert not torch.equal(fc.conv_fwd_emul(t["x"], t["w"], stride, pad, seed_error="rs_swapped"), ref["y"])


FLOAT_CONVS = {"3x3/1 M126 K70": (2, 7, 9, 5, 70, 3, 3, 1, 1), "3x3/2 H8 K5": (2, 8, 8, 6, 5, 3, 3, 2, 1)}
EPILOGUES = [(False, fc.ACT_NONE, False), (True, fc.ACT_GELU, True), (True, fc.ACT_RELU, False), (False, fc.ACT_GELU, True)]


def conv_chain(t, stride, pad, bias, act, res, h, w, r, s):
    """(ref64, emulation) of forward and backward: the backward recomputes the pre-activation with the forward kernel, takes dy
    through act', then input gradient, weight gradient, bias gradient = column sums"""
    b, rs = (t["bias"] if bias else None), (t["res"] if res else None)
    y64, pre64 = fc.conv_fwd_ref(t["x"], t["w"], stride, pad, b, act, rs)
    dpre64 = t["dy"].double() * kc._act_grad64(pre64, act)
    o = kc.conv_ref(t["x"], t["w"], stride, pad, dy=dpre64)
    ref = {"y": y64, "dx": o["dx"], "dw": o["dw"], "db": dpre64.reshape(-1, dpre64.shape[-1]).sum(0), "dres": t["dy"].double()}
    pre = fc.conv_fwd_emul(t["x"], t["w"], stride, pad, b)
    dpre = fc.act_bwd_emul(pre, None, t["dy"], act)
    em = {"y": fc.conv_fwd_emul(t["x"], t["w"], stride, pad, b, act, rs), "dx": fc.conv_dgrad_emul(dpre, t["w"], h, w, stride, pad),
          "dw": fc.conv_wgrad_emul(t["x"], dpre, r, s, stride, pad), "db": fc.colsum_emul(dpre.reshape(-1, dpre.shape[-1])),
          "dres": t["dy"].double()}
    floors = {"dw": fc.wgrad_floor(t["x"], dpre64, r, s, stride, pad), "db": kc.f32_sum_floor(dpre64.reshape(-1, dpre64.shape[-1]))}
    return ref, em, floors


@pytest.mark.parametrize("family", ["randn", "offset", "big_pixel"])
@pytest.mark.parametrize("name", list(FLOAT_CONVS))
def test_conv_forward_and_backward_through_every_epilogue(name, family):
    n, h, w, c, k, r, s, stride, pad = FLOAT_CONVS[name]
    t = fc.conv_inputs(family, n, h, w, c, k, r, s, stride, pad, 3)
    for bias, act, res in EPILOGUES:
        ref, em, floors = conv_chain(t, stride, pad, bias, act, res, h, w, r, s)
        got = run_conv(t, stride, pad, bias, act, res)
        what = f"f32 conv {name} {family} bias {bias} act {act} res {res}"
        fc.check32(got["y"], ref["y"], em["y"], f"{what}: y", SUM)
        fc.check32(got["dx"], ref["dx"], em["dx"], f"{what}: dx", SUM)
        fc.check32(got["dw"], ref["dw"], em["dw"], f"{what}: dw", SUM, abs_floor=floors["dw"])
        if bias:
            fc.check32(got["db"], ref["db"], em["db"], f"{what}: dbias", abs_floor=floors["db"])
        if res:
            assert torch.equal(got["dres"].double(), ref["dres"])


def test_conv_takes_contiguous_nchw_and_bf16_inputs():
    n, h, w, c, k, r, s, stride, pad = FLOAT_CONVS["3x3/2 H8 K5"]
    t = fc.conv_inputs("randn", n, h, w, c, k, r, s, stride, pad, 4)
    ref, _ = fc.conv_fwd_ref(t["x"], t["w"], stride, pad)
    em = fc.conv_fwd_emul(t["x"], t["w"], stride, pad)
    y = f32path().conv2d(dev(nchw(t["x"]).contiguous()), dev(nchw(t["w"]).contiguous()), stride, pad)
    fc.check32(nhwc(y), ref, em, "f32 conv, NCHW-contiguous input: y", SUM)
    xb = t["x"].bfloat16()
    ref, _ = fc.conv_fwd_ref(xb.float(), t["w"], stride, pad)
    y = f32path().conv2d(dev(nchw(xb)), dev(nchw(t["w"])), stride, pad)
    fc.check32(nhwc(y), ref, fc.conv_fwd_emul(xb.float(), t["w"], stride, pad), "f32 conv, bf16 input: y", SUM)


def wgrad_only(t, stride, pad, linear=False):
    if linear:
        rows, c = t["x"].shape[0], t["x"].shape[-1]
        k = t["w"].shape[0]
        w = dev(t["w"].reshape(k, c), True)
        f32path().linear(dev(t["x"].reshape(rows, c)), w).backward(dev(t["dy"].reshape(rows, k)))
        return w.grad.cpu().reshape(k, 1, 1, c)
    w = dev(nchw(t["w"]), True)
    f32path().conv2d(dev(nchw(t["x"])), w, stride, pad).backward(dev(nchw(t["dy"])))
    return nhwc(w.grad)


# (n, h, w, c, k, linear): one slab of 4096 pixels; two slabs of 2050 (a ragged 16-pixel step inside the slab); Linear rows around one
# slab of 256 and two of 150; the cap of 256 slabs: Linear 65793 rows -> 258 per slab, 1 x 1 conv on 1025 x 1025 -> 4105 per slab
SLAB_CASES = {"conv M4096": (1, 64, 64, 3, 2, False), "conv M4100": (1, 41, 100, 3, 2, False), "linear 255": (255, 1, 1, 5, 3, True),
              "linear 256": (256, 1, 1, 5, 3, True), "linear 257": (257, 1, 1, 5, 3, True), "linear 300": (300, 1, 1, 5, 3, True),
              "linear 65793 cap": (65793, 1, 1, 8, 8, True), "conv 1025x1025 cap": (1, 1025, 1025, 1, 1, False)}


@pytest.mark.parametrize("name", list(SLAB_CASES))
def test_wgrad_slabs(name):
    n, h, w, c, k, linear = SLAB_CASES[name]
    assert fc.wgrad_slabs(n * h * w, linear)[0] == {"conv M4096": 1, "conv M4100": 2, "linear 255": 1, "linear 256": 1, "linear 257": 2,
                                                    "linear 300": 2, "linear 65793 cap": 256, "conv 1025x1025 cap": 256}[name]
    t = fc.conv_inputs("lattice", n, h, w, c, k, 1, 1, 1, 0, 5)
    want = (t["dy"].double().reshape(-1, k).t() @ t["x"].double().reshape(-1, c)).reshape(k, 1, 1, c)
    assert float((t["dy"].double().reshape(-1, k).abs().t() @ t["x"].double().reshape(-1, c).abs()).max()) < 2.0 ** 24
    assert torch.equal(wgrad_only(t, 1, 0, linear).double(), want), f"{name}: lattice dw differs from float64"
    t = fc.conv_inputs("randn", n, h, w, c, k, 1, 1, 1, 0, 6)
    want = (t["dy"].double().reshape(-1, k).t() @ t["x"].double().reshape(-1, c)).reshape(k, 1, 1, c)
    fc.check32(wgrad_only(t, 1, 0, linear), want, fc.conv_wgrad_emul(t["x"], t["dy"], 1, 1, 1, 0), f"f32 wgrad {name}: dw", SUM,
               abs_floor=fc.wgrad_floor(t["x"], t["dy"], 1, 1, 1, 0))


# ------------------------------------------------------------------------------------------------ BatchNorm
BN_SHAPES = [(1, 70, 4), (2, 33, 2), (2, 1, 1), (7, 32, 1), (8, 31, 2), (9, 1, 4), (511, 33, 1), (512, 32, 2), (513, 31, 4), (1000, 70, 1),
             (1000, 1, 2)]                  # (rows per group, C, groups)


def bn_dy_floor(bref, bem):
    return {"abs_floor": max(fc.elem_floor(bref["dy"]), bem["dy_floor"]), "floor_all": True, "floor_cosine": True}


def bn_two_updates(t, groups, eps, relu, res, emulate):
    """the forward twice (the running statistics take two updates of G groups each) -> the second call's result"""
    run = (t["running_mean"], t["running_var"])
    for _ in range(2):
        if emulate:
            o = fc.bn_fwd_emul(t["y"], t["residual"] if res else None, t["gamma"], t["beta"], groups, eps, 0.1, relu, running=run)
        else:
            o = kc.bn_forward_ref(t["y"], t["residual"] if res else None, t["gamma"], t["beta"], groups, eps, 0.1, relu, running=run)
        run = (o["running_mean"], o["running_var"])
    return o


def bn_case(family, rpg, c, groups, relu, res, what, four_d=None):
    rows = rpg * groups
    t = fc.bn_inputs(family, rows, c, groups, rpg + c)
    eps = fc.bn_eps(family, rpg)
    ref, em = bn_two_updates(t, groups, eps, relu, res, False), bn_two_updates(t, groups, eps, relu, res, True)
    shape = (lambda v: v) if four_d is None else (lambda v: nchw(v.reshape(four_d[0], four_d[1], four_d[2], c)))
    y, r = dev(shape(t["y"]), True), dev(shape(t["residual"]) if res else None, True)
    gamma, beta = dev(t["gamma"], True), dev(t["beta"], True)
    rm, rv, nb = dev(t["running_mean"].clone()), dev(t["running_var"].clone()), torch.zeros((), dtype=torch.long, device=DEV)
    for i in range(2):
        out = f32path().batch_norm(y, gamma, beta, rm, rv, True, r, relu, eps, 0.1, groups, nb)
        assert int(nb) == groups * (i + 1)
    saved = out.grad_fn.saved_tensors
    mean, invstd = saved[2].cpu(), saved[3].cpu()
    rows_of = (lambda v: v.detach().cpu()) if four_d is None else (lambda v: nhwc(v).reshape(rows, c))
    got = {"out": rows_of(out), "mean": mean, "invstd": invstd, "running_mean": rm.cpu(), "running_var": rv.cpu()}
    fl = fc.bn_fwd_floors(t, ref)
    for key in fl:
        fc.check32(got[key], ref[key], em[key], f"{what}: {key}", abs_floor=fl[key], floor_all=True, floor_cosine=key == "out")
    if family == "lattice" and rpg % 2 == 0:
        assert torch.equal(got["out"].double(), ref["out"]) and torch.equal(mean.double(), ref["mean"]) and torch.equal(invstd.double(), ref["invstd"])
    if relu:
        assert bool((got["out"] >= 0).all())
    # backward on the kernel's own operands: y, dout, its output, its saved statistics
    out.backward(dev(shape(t["dout"])))
    o = got["out"] if relu else None
    bref = kc.bn_backward_ref(t["y"], t["dout"], t["gamma"], t["beta"], mean, invstd, groups, out_relu=o)
    bem = fc.bn_bwd_emul(t["y"], t["dout"], o, t["gamma"], mean, invstd, groups)
    fc.check32(rows_of(y.grad), bref["dy"], bem["dy"], f"{what}: dy", **bn_dy_floor(bref, bem))
    fc.check32(gamma.grad.cpu(), bref["dgamma"], bem["dgamma"], f"{what}: dgamma", abs_floor=kc.f32_sum_floor(bem["terms"][1]))
    fc.check32(beta.grad.cpu(), bref["dbeta"], bem["dbeta"], f"{what}: dbeta", abs_floor=kc.f32_sum_floor(bem["terms"][0]))
    if res:
        assert torch.equal(rows_of(r.grad).double(), bref["dz"]), "dz is dout where the output is positive, exactly 0 elsewhere"


@pytest.mark.parametrize("family", fc.BN_FAMILIES)
@pytest.mark.parametrize("rpg,c,groups", BN_SHAPES)
def test_batchnorm_training_forward_and_backward(rpg, c, groups, family):
    for relu, res in ((False, False), (True, True)):
        bn_case(family, rpg, c, groups, relu, res, f"f32 BN {rpg} x {c} G {groups} {family} relu {relu} res {res}")


def test_batchnorm_on_a_4d_tensor():
    bn_case("randn", 2 * 3 * 5, 33, 2, True, True, "f32 BN NCHW 4 x 33 x 3 x 5 G 2", four_d=(4, 3, 5))


@pytest.mark.parametrize("relu,res", [(False, False), (True, True)])
def test_batchnorm_eval_forward(relu, res):
    t = fc.bn_inputs("randn", 513, 33, 1, 9)
    r = t["residual"] if res else None
    ref = kc.bn_eval_ref(t["y"], r, t["gamma"], t["beta"], t["running_mean"], t["running_var"], 1e-5, relu)
    em = fc.bn_eval_emul(t["y"], r, t["gamma"], t["beta"], t["running_mean"], t["running_var"], 1e-5, relu)
    rm, rv = dev(t["running_mean"].clone()), dev(t["running_var"].clone())
    out = f32path().batch_norm(dev(t["y"]), dev(t["gamma"]), dev(t["beta"]), rm, rv, False, dev(r), relu, 1e-5, 0.1, 4, None)
    fl = 2.0 * kc.f32_stat_floor(t["running_mean"].double() * ref["scale"], ref["shift"])
    fc.check32(out.cpu(), ref["out"], em, f"f32 BN eval relu {relu} res {res}: out", abs_floor=fl, floor_all=True, floor_cosine=True)
    assert torch.equal(rm.cpu(), t["running_mean"]) and torch.equal(rv.cpu(), t["running_var"])


def test_batchnorm_refusals_and_parameter_gradients():
    t = fc.bn_inputs("randn", 14, 8, 2, 1)
    args = lambda y, g, b, training, groups: (y, g, b, dev(t["running_mean"].clone()), dev(t["running_var"].clone()), training, None, False,  # noqa: E731
                                               1e-5, 0.1, groups, torch.zeros((), dtype=torch.long, device=DEV))
    with pytest.raises(ValueError):
        f32path().batch_norm(*args(dev(t["y"]), dev(t["gamma"]), dev(t["beta"]), True, 4))
    y = dev(t["y"], True)
    with pytest.raises(NotImplementedError):
        f32path().batch_norm(*args(y, dev(t["gamma"]), dev(t["beta"]), False, 1)).sum().backward()
    # a frozen gamma keeps beta trainable, and the other way round
    both = [dev(t["gamma"], True), dev(t["beta"], True)]
    f32path().batch_norm(*args(dev(t["y"]), both[0], both[1], True, 2)).backward(dev(t["dout"]))
    for frozen in (0, 1):
        p = [dev(t["gamma"], frozen != 0), dev(t["beta"], frozen != 1)]
        f32path().batch_norm(*args(dev(t["y"]), p[0], p[1], True, 2)).backward(dev(t["dout"]))
        assert p[frozen].grad is None
        assert p[1 - frozen].grad is not None and torch.equal(p[1 - frozen].grad, both[1 - frozen].grad)


# ------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("family", fc.POOL_FAMILIES)
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 3), (7, 8), (8, 7), (14, 14)])
def test_maxpool_forward_and_backward_are_exact(h, w, family):
    for c in (1, 3, 65):
        x, dy = fc.pool_inputs(family, 2, h, w, c, h * 16 + w + c)
        y, dx = fc.maxpool_fwd_bwd(x, dy)
        xd = dev(nchw(x), True)
        out = f32path().max_pool3x3s2(xd)
        out.backward(dev(nchw(dy)))
        assert torch.equal(nhwc(out), y), f"max-pool {h} x {w} x {c} {family}: y"
        assert torch.equal(nhwc(xd.grad).double(), dx), f"max-pool {h} x {w} x {c} {family}: dx (first maximum in scan order)"


@pytest.mark.parametrize("hw", [1, 49, 50])
def test_gap_forward_and_backward(hw):
    for nc in ((5, 51), (4, 64), (1, 257)):          # N C = 255, 256, 257
        n, c = nc
        x = fc.offset_rows(n * hw, c, hw + c).reshape(n, hw, c)
        dy = fc.offset_rows(n, c, hw + c + 1, 1.0)
        xd = dev(nchw(x.reshape(n, hw, 1, c)), True)
        y = f32path().global_avg_pool(xd)
        y.backward(dev(dy))
        ref, rb = x.double().mean(1), (dy.double() / hw).unsqueeze(1).expand(-1, hw, -1)
        fc.check32(y.cpu(), ref, fc.gap_emul(x), f"f32 GAP {n} x {hw} x {c}: y", **elem(ref))
        fc.check32(nhwc(xd.grad).reshape(n, hw, c), rb, fc.gap_bwd_emul(dy, hw), f"f32 GAP {n} x {hw} x {c}: dx", **elem(rb))


@pytest.mark.parametrize("rows", [1, 1000])
def test_colsum_through_broadcast_and_a_bias_gradient(rows):
    for c in (1, 255, 256, 257):
        g = fc.offset_rows(rows, c, rows + c)
        t = torch.zeros(c, device=DEV, requires_grad=True)
        f32path().broadcast(t, rows).backward(dev(g))
        b = torch.zeros(c, device=DEV, requires_grad=True)
        f32path().bias_act(dev(g), b).backward(dev(g))
        for name, got in (("broadcast", t.grad), ("bias gradient", b.grad)):
            fc.check32(got.cpu(), g.double().sum(0), fc.colsum_emul(g), f"f32 colsum {rows} x {c} via {name}", abs_floor=kc.f32_sum_floor(g))


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_SHAPES = [(1, 1000, 1e-6), (2, 65, 1e-5), (150, 192, 1e-12), (513, 63, 1e-6), (1000, 8, 1e-5), (150, 1, 1e-6), (150, 64, 1e-12)]


@pytest.mark.parametrize("family", kc.LN_FAMILIES)
@pytest.mark.parametrize("rows,c,eps", LN_SHAPES)
def test_layernorm_forward_and_backward(rows, c, eps, family):
    x, gamma, beta, dy, _ = fc.ln_inputs(family, rows, c, rows + c)
    ref = kc.layer_norm_ref(x, gamma, beta, fc.f32c(eps), dy)
    em = fc.ln_emul(x, gamma, beta, eps, dy)
    xd, gd, bd = dev(x, True), dev(gamma, True), dev(beta, True)
    y = f32path().layer_norm(xd, gd, bd, eps)
    y.backward(dev(dy))
    what = f"f32 LayerNorm {rows} x {c} eps {eps:g} {family}"
    xh = (ref[0] - beta.double()) / gamma.double()
    fc.check32(y.detach().cpu(), ref[0], em[0], f"{what}: y", **elem(ref[0]))
    fc.check32(xd.grad.cpu(), ref[1], em[1], f"{what}: dx", **elem(ref[1]))
    fc.check32(gd.grad.cpu(), ref[2], em[2], f"{what}: dgamma", abs_floor=kc.f32_sum_floor(dy.double() * xh))
    fc.check32(bd.grad.cpu(), ref[3], em[3], f"{what}: dbeta", abs_floor=kc.f32_sum_floor(dy))
    # each parameter gradient requested alone is the same bits
    for only in (0, 1):
        p = [dev(gamma, only == 0), dev(beta, only == 1)]
        f32path().layer_norm(dev(x), p[0], p[1], eps).backward(dev(dy))
        assert p[1 - only].grad is None and torch.equal(p[only].grad, (gd, bd)[only].grad)


# ------------------------------------------------------------------------------------------------ bias / activation
@pytest.mark.parametrize("act", [fc.ACT_NONE, fc.ACT_GELU, fc.ACT_RELU])
def test_bias_act_forward_and_backward(act):
    with kc.float32_inputs():
        x = kc.act_grid(40, 33, 1)
    g = torch.Generator().manual_seed(2)
    bias, res, dy = torch.randn(33, generator=g) * 0.1, torch.randn(40, 33, generator=g), torch.randn(40, 33, generator=g)
    for b, r in ((None, None), (bias, None), (None, res), (bias, res)):
        ref, em = kc.bias_act_ref(x, b, act, r, dy), fc.bias_act_emul(x, b, act, r, dy)
        xd, bd, rd = dev(x, True), dev(b, True), dev(r, True)
        y = f32path().bias_act(xd, bd, act, rd)
        y.backward(dev(dy))
        what = f"f32 bias_act act {act} bias {b is not None} res {r is not None}"
        fc.check32(y.detach().cpu(), ref[0], em[0], f"{what}: y", **elem(ref[0]))
        fc.check32(xd.grad.cpu(), ref[1], em[1], f"{what}: dx", **elem(ref[1]))
        if b is not None:
            fc.check32(bd.grad.cpu(), ref[2], em[2], f"{what}: dbias", abs_floor=kc.f32_sum_floor(ref[1]))
        if r is not None:
            assert torch.equal(rd.grad.cpu(), dy)
        if act == fc.ACT_RELU and b is None:
            assert torch.equal(xd.grad.cpu().double(), ref[1]), "ReLU' is 0 at exactly 0"


# ------------------------------------------------------------------------------------------------ attention
def attn_case(family, b, s, h, hd, scale, what, backward=True):
    qkv, dout = fc.attn_inputs(family, b, s, h, hd, s * hd + b, scale)
    sc = hd ** -0.5 if scale is None else scale
    ro, _, rg = kc.attention_ref(qkv, fc.f32c(sc), dout if backward else None)
    eo, eg = fc.attention_emul(qkv, sc, dout if backward else None)
    qd = dev(qkv.reshape(b * s, 3 * h * hd), backward)
    out = f32path().attention(qd, b, s, h, scale, hd)
    fc.check32(out.detach().cpu().reshape(b, s, h, hd), ro, eo, f"{what}: out", SUM)
    if backward:
        out.backward(dev(dout.reshape(b * s, h * hd)))
        fc.check32(qd.grad.cpu().reshape(b, s, 3, h, hd), rg, eg, f"{what}: dqkv", SUM)


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("s", [1, 2, 17, 64, 65, 128, 129, 197, 256, 257])
def test_attention_forward_and_backward_across_the_query_strides(s, hd):
    """forward: queries strided by 256; backward: by 256 / (hd / 16) = 128 (hd 32) or 64 (hd 64) rows"""
    i = [1, 2, 17, 64, 65, 128, 129, 197, 256, 257].index(s) + (hd == 64)
    family = kc.ATTENTION_FAMILIES[i % len(kc.ATTENTION_FAMILIES)]
    b, h = (2, 3) if s <= 65 else (1, 1)
    scale = 1.0 if i % 2 and family not in ("offset+80", "offset-80") else None
    attn_case(family, b, s, h, hd, scale, f"f32 attention {b} x {h} x {hd}, {s} tokens, {family}, scale {scale}")


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_families(hd, family):
    attn_case(family, 2, 17, 3, hd, None, f"f32 attention 2 x 3 x {hd}, 17 tokens, {family}")
    attn_case(family, 1, 65, 1, hd, None if family.startswith("offset") else 1.0, f"f32 attention 1 x 1 x {hd}, 65 tokens, {family}")


def test_attention_at_the_lds_gate():
    """160 KiB of LDS: forward 2 S hd floats (S <= 320 at hd 64), backward 2 S hd + 3 S (S <= 312)"""
    attn_case("randn", 1, 312, 1, 64, None, "f32 attention 1 x 1 x 64, 312 tokens (backward gate)")
    attn_case("peaked", 1, 320, 1, 64, None, "f32 attention 1 x 1 x 64, 320 tokens (forward gate)", backward=False)


def test_attention_beyond_the_lds_gate_is_refused_and_launches_nothing():
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd._lib import ptr, stream_ptr

    lib = _lib.load()
    qkv = torch.randn(321, 3 * 64, device=DEV)
    out = torch.full((321, 64), 7.0, device=DEV)
    assert lib.wm_f32_attention(ptr(qkv), 1, 321, 1, 64, 0.125, ptr(out), stream_ptr()) == WM_EUNSUPPORTED
    dq = torch.full((313, 3 * 64), 7.0, device=DEV)
    assert lib.wm_f32_attention_bwd(ptr(qkv), ptr(out), ptr(out), 1, 313, 1, 64, 0.125, ptr(dq), stream_ptr()) == WM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dq == 7.0).all())
    with pytest.raises(_lib.WaferHipError):
        f32path().attention(qkv, 1, 321, 1, None, 64)


# ------------------------------------------------------------------------------------------------ softmax rows, pair CE, reduce, losses
@pytest.mark.parametrize("family", ["randn", "big", "constant"])
@pytest.mark.parametrize("d", [1, 255, 256, 257, 2048, 65536])
def test_softmax_rows(d, family):
    x, sub = fc.softmax_inputs(family, 3, d, d)
    for s in (None, sub):
        for it in (1 / 0.04, 1 / 0.1):
            for log in (False, True):
                ref, em = fc.softmax_ref(x, s, it, log), fc.softmax_emul(x, s, it, log)
                got = f32path().softmax_rows(dev(x), dev(s), it, log)
                fc.check32(got.cpu(), ref, em, f"f32 softmax_rows D {d} {family} subtract {s is not None} 1/T {it:g} log {log}",
                           **elem(ref))


def pair_ce(probs, logq, tv, sv, b):
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd._lib import check, ptr, stream_ptr

    out = torch.empty(tv * sv * b, device=DEV)
    p, q = dev(probs), dev(logq)
    check(_lib.load().wm_f32_pair_ce(ptr(p), ptr(q), tv, sv, b, probs.shape[1], ptr(out), stream_ptr()), "wm_f32_pair_ce")
    return out.cpu()


@pytest.mark.parametrize("d", [1, 257, 2048])
def test_pair_ce(d):
    for sv in (2, 4, 8):
        for b in (1, 3):
            g = torch.Generator().manual_seed(sv * 100 + b * 10 + d)
            logq = torch.log_softmax(torch.randn(sv * b, d, generator=g) * 3, -1)
            # one-hot teacher rows: pair (t, s, b) is exactly -logq[s, b, hot[t, b]] and 0 on the diagonal: settles the pair order
            hot = torch.randint(0, d, (2 * b,), generator=g)
            probs = torch.nn.functional.one_hot(hot, d).float()
            lq, hot = logq.reshape(sv, b, d), hot.reshape(2, b)
            want = torch.stack([-lq[s, i, hot[t, i]] * (t != s) for t in range(2) for s in range(sv) for i in range(b)])
            assert torch.equal(pair_ce(probs, logq, 2, sv, b), want + 0.0), f"pair CE one-hot T 2 SV {sv} B {b} D {d}"
            probs = torch.softmax(torch.randn(2 * b, d, generator=g) * 3, -1)
            ref = fc.pair_ce_emul(probs, logq, 2, sv, b, rnd=lambda v: v)
            fc.check32(pair_ce(probs, logq, 2, sv, b), ref, fc.pair_ce_emul(probs, logq, 2, sv, b), f"f32 pair CE T 2 SV {sv} B {b} D {d}",
                       **elem(ref))


def scalar_check(got, ref, em, what):
    """a float32 scalar from a double sum: within FACTOR roundings of the result (the emulation's own error where it is larger)"""
    err, yard = abs(float(got) - float(ref)), abs(float(em) - float(ref))
    from parity_log import parity

    parity(what, err, kc.FACTOR * max(yard, 2.0 ** -24 * abs(float(ref))), note="FACTOR x max(emulation's error, one float32 rounding)")


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 73728])
def test_reduce_and_the_loss_values(n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g) + 3, torch.randn(n, generator=g)
    for mode in (0, 1, 2):
        ref = fc.reduce_emul(a, b, mode, 0.37 / n, rnd=lambda v: v)
        got = f32path()._reduce(dev(a), dev(b) if mode else None, mode, 0.37 / n)
        scalar_check(got, ref, fc.reduce_emul(a, b, mode, 0.37 / n), f"f32 reduce mode {mode} n {n}")
    for mode, fn in ((1, f32path().mse_loss), (2, f32path().l1_loss)):
        ref = fc.reduce_emul(a, b, mode, 1.0 / n, rnd=lambda v: v)
        scalar_check(fn(dev(a), dev(b)), ref, fc.reduce_emul(a, b, mode, 1.0 / n), f"f32 {'mse' if mode == 1 else 'l1'}_loss n {n}")


@pytest.mark.parametrize("n", [255, 257])
def test_loss_bwd(n):
    g = torch.Generator().manual_seed(n)
    p, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    t[::7] = p[::7]                                       # exact zeros in pred - target
    for mode, fn in ((1, f32path().mse_loss), (2, f32path().l1_loss)):
        pd, td = dev(p, True), dev(t, True)
        (fn(pd, td) * 1.7).backward()                     # a non-unit incoming gradient
        ref, em = fc.loss_bwd_ref(p, t, mode, 1.0 / n, 1.7), fc.loss_bwd_emul(p, t, mode, 1.0 / n, 1.7)
        fc.check32(pd.grad.cpu(), ref, em, f"f32 loss_bwd mode {mode} n {n}: d pred", **elem(ref))
        assert torch.equal(td.grad, -pd.grad)
        assert bool((pd.grad[::7] == 0).all()), "the gradient is 0 where pred == target (L1: sign(0) = 0)"


def test_dino_loss_matches_float64_and_refuses_backward():
    g = torch.Generator().manual_seed(0)
    sv, tv, b, d = 4, 2, 3, 2048
    student, probs = torch.randn(sv * b, d, generator=g) * 2, torch.softmax(torch.randn(tv * b, d, generator=g) * 2, -1)
    ref, em = fc.dino_loss_ref(student, probs, sv, tv, b, 0.1), fc.dino_loss_ref(student, probs, sv, tv, b, 0.1, emulate=True)
    sd = dev(student, True)
    loss = f32path().dino_loss(sd, dev(probs), sv, tv, b, 0.1)
    scalar_check(loss.detach(), ref, em, "f32 dino_loss vs float64")
    with pytest.raises(NotImplementedError):
        loss.backward()


@pytest.mark.parametrize("rows", [1, 16])
def test_dino_center_update(rows):
    for d in (1, 255, 256, 257):
        g = torch.Generator().manual_seed(rows + d)
        c, t = torch.randn(d, generator=g), torch.randn(rows, d, generator=g)
        for m in (0.0, 0.9, 1.0):
            cd = dev(c.clone())
            f32path().dino_center_update(cd, dev(t), m)
            ref = fc.center_update_ref(c, t, m)
            fc.check32(cd.cpu(), ref, fc.center_update_emul(c, t, m), f"f32 center update {rows} x {d} momentum {m}",
                       abs_floor=kc.f32_stat_floor(c, t), floor_all=True)


# ------------------------------------------------------------------------------------------------ beyond the grid cap of 65535 blocks
BIG_ROWS, BIG_C = 65600, 256             # 16 793 600 elements > 65535 * 256: the grid-stride loops take a second trip


def test_bias_act_beyond_the_grid_cap():
    g = torch.Generator().manual_seed(0)
    x, bias = torch.randn(BIG_ROWS, BIG_C, generator=g), torch.randn(BIG_C, generator=g)
    xd, bd = dev(x, True), dev(bias)
    y = f32path().bias_act(xd, bd, fc.ACT_RELU)
    y.backward(xd.detach())
    v = x + bias                                          # one float32 addition, then the ReLU: exact on either side
    assert torch.equal(y.detach().cpu(), v.clamp_min(0.0)), "bias + ReLU beyond the grid cap"
    assert torch.equal(xd.grad.cpu(), x * (v > 0)), "ReLU backward beyond the grid cap"


_BIG_BN = {}


def big_bn():
    """the 65600 x 256 BatchNorm case, run once for the two tests below: inputs, the kernel's results, the forward reference"""
    if not _BIG_BN:
        t = fc.bn_inputs("randn", BIG_ROWS, BIG_C, 1, 0)
        y, gamma, beta = dev(t["y"], True), dev(t["gamma"], True), dev(t["beta"], True)
        out = f32path().batch_norm(y, gamma, beta, dev(t["running_mean"].clone()), dev(t["running_var"].clone()), True, None, True, 1e-5,
                                   0.1, 1, torch.zeros((), dtype=torch.long, device=DEV))
        mean, invstd = out.grad_fn.saved_tensors[2].cpu(), out.grad_fn.saved_tensors[3].cpu()
        out.backward(dev(t["dout"]))
        _BIG_BN.update(t=t, out=out.detach().cpu(), mean=mean, invstd=invstd, dy=y.grad.cpu(), dgamma=gamma.grad.cpu(), dbeta=beta.grad.cpu())
    return _BIG_BN


def test_batchnorm_forward_beyond_the_grid_cap():
    b = big_bn()
    t, run = b["t"], (b["t"]["running_mean"], b["t"]["running_var"])
    ref = kc.bn_forward_ref(t["y"], None, t["gamma"], t["beta"], 1, 1e-5, 0.1, True, running=run)
    em = fc.bn_fwd_emul(t["y"], None, t["gamma"], t["beta"], 1, 1e-5, 0.1, True, running=run)
    fl = fc.bn_fwd_floors(t, ref)
    fc.check32(b["out"], ref["out"], em["out"], "f32 BN 65600 x 256: out", abs_floor=fl["out"], floor_all=True, floor_cosine=True)


def test_batchnorm_backward_beyond_the_grid_cap():
    b = big_bn()
    t = b["t"]
    bref = kc.bn_backward_ref(t["y"], t["dout"], t["gamma"], t["beta"], b["mean"], b["invstd"], 1, out_relu=b["out"])
    bem = fc.bn_bwd_emul(t["y"], t["dout"], b["out"], t["gamma"], b["mean"], b["invstd"], 1)
    fc.check32(b["dy"], bref["dy"], bem["dy"], "f32 BN 65600 x 256: dy", **bn_dy_floor(bref, bem))
    fc.check32(b["dgamma"], bref["dgamma"], bem["dgamma"], "f32 BN 65600 x 256: dgamma", abs_floor=kc.f32_sum_floor(bem["terms"][1]))
    fc.check32(b["dbeta"], bref["dbeta"], bem["dbeta"], "f32 BN 65600 x 256: dbeta", abs_floor=kc.f32_sum_floor(bem["terms"][0]))
    _BIG_BN.clear()


def test_maxpool_backward_beyond_the_grid_cap():
    h = w = 4097                                          # 16 785 409 input elements > 16 776 960
    x, dy = fc.pool_inputs("three_level", 1, h, w, 1, 0)
    y, dx = fc.maxpool_fwd_bwd(x, dy)
    xd = dev(nchw(x), True)
    out = f32path().max_pool3x3s2(xd)
    out.backward(dev(nchw(dy)))
    assert torch.equal(nhwc(out), y) and torch.equal(nhwc(xd.grad).double(), dx)
