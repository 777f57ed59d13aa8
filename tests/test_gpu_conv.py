"""csrc/conv.hip against float64, on every route the host code can take.

Every case first asks wm_conv2d_route which kernel instantiation serves it (tests/conv_cases.py names the one it is
there for) and then runs two tiers:
  * `lattice` inputs (small integers, sparse +-1 weights): every product, partial sum and rounded output is exact, so the
    kernel must EQUAL the float64 reference -- y, dx, the weight-gradient slabs and the delivered gradient, the statistics
    slots, the masked gradient and its sums.  No tolerance.
  * `randn`, `offset`, `big_pixel` through kernel_check.check: bounds of 2 x what the bf16 emulation of the kernel's own
    rounding places scores itself (float32 sums: F32_SUM_FACTOR and f32_sum_floor, as the Linear dW tests).

Outputs are prefilled with NaN inside a larger buffer whose margins (more than one 128 x 128 tile on either side) hold
a sentinel that must survive; inputs sit between NaN margins, so a read outside a tensor poisons the result instead of
supplying a plausible zero.  The margins are ordinary allocated memory.  Shapes: (N, C, H, W, K, R, stride, pad)."""
import functools
import os

import conv_cases as cc
import kernel_check as kc
import parity_log
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 32768   # elements on either side: a 128 x 128 bf16 tile is 16384; a multiple of 8, so views stay 16-byte aligned
SENTINEL = {torch.bfloat16: 12352.0, torch.float32: 12345.0}
BF, F32 = torch.bfloat16, torch.float32
RATIOS = {}      # (kernel, tensor) -> worst measured / bound of the tolerance tier


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    out = os.path.dirname(parity_log._PATH)   # beside the parity log of the other GPU tests
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "conv_kernel_check_ratios.txt"), "w") as fh:
        for (kern, tensor), v in sorted(RATIOS.items()):
            fh.write(f"{v:.3f} {kern} {tensor}\n")


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    return _lib.load()


def _ok(rc, what):
    from ssl_wafermap_amd import _lib

    _lib.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _out(shape, dtype):
    """(view prefilled with NaN, whole buffer with sentinel margins)"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((2 * MARGIN + n,), SENTINEL[dtype], dtype=dtype, device=DEV)
    buf[MARGIN:MARGIN + n] = float("nan")
    return buf[MARGIN:MARGIN + n].view(shape), buf


def _inp(t, dtype=BF):
    """the tensor as a view between NaN margins (uint8 masks: between 0xff bytes)"""
    n = t.numel()
    fill = 0xFF if dtype == torch.uint8 else float("nan")
    buf = torch.full((2 * MARGIN + n,), fill, dtype=dtype, device=DEV)
    buf[MARGIN:MARGIN + n] = t.reshape(-1).to(DEV, dtype)
    return buf[MARGIN:MARGIN + n].view(t.shape)


def _host(view, buf, what):
    """the result on the host as float64, after the margin and NaN checks"""
    torch.cuda.synchronize()
    n = view.numel()
    s = SENTINEL[view.dtype]
    assert bool((buf[:MARGIN] == s).all()) and bool((buf[MARGIN + n:] == s).all()), f"{what}: wrote outside its output"
    got = view.double().cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: NaN left (an element nobody wrote, or a read outside an input)"
    return got


def _judge(family, kern, tensor, got, ref, emul, what, f32_floor=None):
    if family == "lattice":
        assert torch.equal(got, ref), f"{what}: differs from float64 in {int((got != ref).sum())} of {ref.numel()} elements, max {float((got - ref).abs().max())}"
        return
    if f32_floor is None:
        r = kc.check(got, ref, emul, what)
    else:
        r = kc.check(got, ref, emul, what, factor=kc.F32_SUM_FACTOR, abs_floor=f32_floor)
    RATIOS[(kern, tensor)] = max(RATIOS.get((kern, tensor), 0.0), r)


@functools.lru_cache(maxsize=12)
def _case(family, g):
    """inputs and float64 reference of geometry g, computed once and shared (callers do not modify them)"""
    n, h, w, c, k, r, s, p, q, stride, pad = g
    i = kc.conv_inputs(family, n, h, w, c, k, r, s, p, q, seed=sum(g))
    ref = kc.conv_ref(i["x"], i["w"], stride, pad, i["dy"], out_hw=(p, q))
    if family == "lattice":   # the preconditions of the exact tier, asserted on the float64 reference
        kc.lattice_exact(ref)
        kc.lattice_exact({"dx + shortcut": ref["dx"] + i["dres"].double()})
    return i, ref


def _kern(route):
    return f"route {route}"


# ------------------------------------------------------------------------------------------------ forward
def _fwd(lib, g, x, wk, stats_groups=0):
    n, p, q, k = g[0], g[7], g[8], g[4]
    y, ybuf = _out((n, p, q, k), BF)
    if not stats_groups:
        _ok(lib.wm_conv2d_fwd(x.data_ptr(), wk.data_ptr(), y.data_ptr(), *g, _st()), "wm_conv2d_fwd")
        return y, ybuf, None, None
    rpg = n * p * q // stats_groups
    tiles = lib.wm_conv2d_fwd_stats_tiles(*g, rpg)
    assert tiles > 0
    part, pbuf = _out((stats_groups, tiles, 2, k), F32)
    _ok(lib.wm_conv2d_fwd_stats(x.data_ptr(), wk.data_ptr(), y.data_ptr(), *g, part.data_ptr(), tiles, rpg, _st()),
        "wm_conv2d_fwd_stats")
    return y, ybuf, part, pbuf


@pytest.mark.parametrize("route,shape", [c for c in cc.FWD if c[1][1] != 3])
def test_forward(lib, route, shape):
    g = cc.geom(shape)
    assert lib.wm_conv2d_route(0, *g, 0, 0) == route
    for family in kc.CONV_FAMILIES:
        i, ref = _case(family, g)
        y, ybuf, _, _ = _fwd(lib, g, _inp(i["x"]), i["w"].to(DEV, BF))
        # emulation: the accumulator tile is staged as bf16 (stage_acc_frag) and stored
        _judge(family, _kern(route), "y", _host(y, ybuf, f"y {family}"), ref["y"], kc.bf(ref["y"]), f"fwd {shape} {family} y")


def _stat_tiles(route, g, groups, slots=None):
    n, p, q = g[0], g[7], g[8]
    if route == kc.ROUTE_STEM_PATCH:
        return kc.stem_tiles(n, p, q, groups, slots)
    return kc.pair_tiles(n, p, q) if route == kc.route_patch(0) else kc.row_tiles(n * p * q)


def _judge_stats(family, route, part, pbuf, y_own, y_ref_rows, tiles, what):
    """the slots against float64 (exact on the lattice; else the float32 row-order sums of the emulated bf16 outputs
    are the yardstick: store_tile_with_stats sums the ROUNDED tile), and against the float64 sums of the kernel's OWN
    stored outputs under the bound no order of float32 additions can exceed (kc.f32_sum_bound)"""
    k = y_own.shape[-1]
    got = _host(part, pbuf, what).reshape(-1, 2, k)
    assert got.shape[0] == len(tiles)
    own = y_own.reshape(-1, k)
    b1, b2 = kc.f32_sum_bound(own, tiles)
    e1, e2 = (got[:, 0] - kc.tile_sums(own, tiles)).abs(), (got[:, 1] - kc.tile_sums(own * own, tiles)).abs()
    assert bool((e1 <= b1).all()), f"{what}: slot sums vs the stored tile: worst {float((e1 / b1.clamp_min(1e-300)).max()):.3g} x the float32 bound"
    assert bool((e2 <= b2).all()), f"{what}: slot squares vs the stored tile: worst {float((e2 / b2.clamp_min(1e-300)).max()):.3g} x the float32 bound"
    emul = kc.bf(y_ref_rows)
    for j, (r64, e64) in enumerate(((y_ref_rows, emul), (y_ref_rows * y_ref_rows, emul * emul))):
        floor = 0.0 if family == "lattice" else max(kc.f32_sum_floor(e64[t]) for t in tiles)
        yard = None if family == "lattice" else kc.tile_sums_f32(e64, tiles)
        _judge(family, _kern(route), ("stat sum", "stat squares")[j], got[:, j], kc.tile_sums(r64, tiles), yard,
               f"{what} {('sums', 'squares')[j]}", f32_floor=floor)


@pytest.mark.parametrize("route,shape,groups", [c for c in cc.FWD_STATS if c[1][1] != 3])
def test_forward_with_statistics(lib, route, shape, groups):
    g = cc.geom(shape)
    n, p, q, k = g[0], g[7], g[8], g[4]
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, n * p * q // groups) == route
    tiles = _stat_tiles(route, g, groups)
    for family in kc.CONV_FAMILIES:
        i, ref = _case(family, g)
        y, ybuf, part, pbuf = _fwd(lib, g, _inp(i["x"]), i["w"].to(DEV, BF), groups)
        y_own = _host(y, ybuf, f"y {family}")
        _judge(family, _kern(route), "y", y_own, ref["y"], kc.bf(ref["y"]), f"fwd+stats {shape} {family} y")
        _judge_stats(family, route, part, pbuf, y_own, ref["y_acc"], tiles, f"fwd+stats {shape} {family}")


# ------------------------------------------------------------------------------------------------ the stem
def _stem_inputs(family, shape):
    n, _, h, w, k, _, _, _ = shape
    return kc.conv_inputs(family, n, h, w, 3, k, 7, 7, h // 2, w // 2, seed=n + h + w)


def _stem_operands(lib, i, fmt_nchw):
    """the space-to-depth image and weights the stem kernels read, made by the library's own layout kernels"""
    from ssl_wafermap_amd import _lib

    n, h, w, _ = i["x"].shape
    k = i["w"].shape[0]
    if fmt_nchw:
        img, fmt = i["x"].permute(0, 3, 1, 2).contiguous().to(DEV), _lib.WM_IMG_NCHW_F32
    else:
        img, fmt = i["x"].to(DEV, BF).contiguous(), _lib.WM_IMG_NHWC_BF16
    xs = _inp(torch.zeros(n, h // 2, w // 2, 16))
    _ok(lib.wm_image_to_s2d(img.data_ptr(), fmt, n, h, w, xs.data_ptr(), _st()), "wm_image_to_s2d")
    w32 = i["w"].permute(0, 3, 1, 2).contiguous().to(DEV)          # [K, 3, 7, 7] float32
    ws = torch.empty(k, 4, 4, 16, dtype=BF, device=DEV)
    _ok(lib.wm_stem_weights_prepare(w32.data_ptr(), k, ws.data_ptr(), _st()), "wm_stem_weights_prepare")
    return xs, ws


@pytest.mark.parametrize("route,shape", [c for c in cc.FWD if c[1][1] == 3])
def test_stem_forward_and_weight_gradient(lib, route, shape):
    """both entries (float32 NCHW and bf16 NHWC images) against the 7 x 7 / 2 / 3 convolution of the IMAGE in float64"""
    g = cc.geom(shape)
    assert lib.wm_conv2d_route(0, *g, 0, 0) == route
    wroute = dict((s, r) for r, s in cc.WGRAD_STEM)[shape]
    assert lib.wm_conv2d_route(2, *g, 0, 0) == wroute
    n, h2, w2, k = g[0], g[1], g[2], g[4]
    for family in kc.CONV_FAMILIES:
        i = _stem_inputs(family, shape)
        ref = kc.conv_ref(i["x"], i["w"], 2, 3, i["dy"])
        if family == "lattice":
            kc.lattice_exact(ref)
        m = n * h2 * w2
        dw32 = floor = None
        if family != "lattice":
            dw32 = kc.matmul_tn_f32(i["dy"].reshape(m, k), ref["cols"]).reshape(k, 7, 7, 3).permute(0, 3, 1, 2)
            floor = float(2.0 ** -24 * (i["dy"].reshape(m, k).double().abs().t() @ ref["cols"].abs()).max())
        for fmt_nchw in (True, False):
            xs, ws = _stem_operands(lib, i, fmt_nchw)
            y, ybuf, _, _ = _fwd(lib, g, xs, ws)
            _judge(family, _kern(route), "y", _host(y, ybuf, "stem y"), ref["y"], kc.bf(ref["y"]), f"stem {shape} {family} y")
        ns = lib.wm_conv2d_wgrad_splits(*g)
        slabs, sbuf = _out((ns, k, 4, 4, 16), F32)
        _ok(lib.wm_conv2d_wgrad(_inp(i["dy"]).data_ptr(), xs.data_ptr(), slabs.data_ptr(), *g, _st()), "wm_conv2d_wgrad")
        grad, gbuf = _out((k, 3, 7, 7), F32)
        _ok(lib.wm_stem_wgrad_finalize(slabs.data_ptr(), ns, k, grad.data_ptr(), 0, _st()), "wm_stem_wgrad_finalize")
        # the slabs, summed in float64, against the 4 x 4 convolution over the space-to-depth operands the kernel read
        s2d = kc.conv_ref(xs.float().cpu(), ws.float().cpu(), 1, 2, i["dy"], out_hw=(h2, w2))
        torch.testing.assert_close(s2d["y"], ref["y"], rtol=1e-12, atol=1e-12)   # (the same convolution in another layout)
        sw32 = None if family == "lattice" else kc.matmul_tn_f32(i["dy"].reshape(m, k), s2d["cols"]).reshape(k, 4, 4, 16)
        _judge(family, _kern(wroute), "dW slabs", _host(slabs, sbuf, "stem slabs").sum(0), s2d["dw"], sw32,
               f"stem {shape} {family} slabs", f32_floor=floor)
        _judge(family, _kern(wroute), "dW", _host(grad, gbuf, "stem dW"), ref["dw"].permute(0, 3, 1, 2), dw32,
               f"stem {shape} {family} dW", f32_floor=floor)


def _stem_stats(lib, shape, groups, families):
    g = cc.geom(shape)
    n, h2, w2, k = g[0], g[1], g[2], g[4]
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, n * h2 * w2 // groups) == kc.ROUTE_STEM_PATCH
    slots = lib.wm_conv2d_fwd_stats_tiles(*g, n * h2 * w2 // groups)
    tiles = kc.stem_tiles(n, h2, w2, groups, slots)
    assert len(tiles) == groups * slots
    for family in families:
        i = _stem_inputs(family, shape)
        ref = kc.conv_ref(i["x"], i["w"], 2, 3)
        xs, ws = _stem_operands(lib, i, False)
        y, ybuf, part, pbuf = _fwd(lib, g, xs, ws, groups)
        y_own = _host(y, ybuf, "stem y")
        _judge(family, _kern(kc.ROUTE_STEM_PATCH), "y", y_own, ref["y"], kc.bf(ref["y"]), f"stem+stats {shape} {family} y")
        _judge_stats(family, kc.ROUTE_STEM_PATCH, part, pbuf, y_own, ref["y_acc"], tiles, f"stem+stats {shape} {family}")
    return slots, len(kc.pair_tiles(n, h2, w2)) // groups


def test_stem_forward_with_statistics(lib):
    (route, shape, groups), = [c for c in cc.FWD_STATS if c[1][1] == 3]
    _stem_stats(lib, shape, groups, kc.CONV_FAMILIES)


def test_stem_blocks_loop_over_a_second_tile_pair(lib):
    """more tile pairs than resident blocks: a handful of blocks walk on to a second pair and flush the sums of both.
    The lattice tier alone (exact; no row-order yardstick at this size)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cc.stem_loop_images(cus)
    slots, pairs = _stem_stats(lib, (n, 3, 16, 16, 64, 7, 2, 3), 1, ("lattice",))
    assert slots < pairs <= slots + 16, (slots, pairs)


# ------------------------------------------------------------------------------------------------ input gradient
def _dgrad(lib, g, dy, wc, dres=None):
    n, h, w, c = g[0], g[1], g[2], g[3]
    dx, dbuf = _out((n, h, w, c), BF)
    if dres is None:
        _ok(lib.wm_conv2d_dgrad(dy.data_ptr(), wc.data_ptr(), dx.data_ptr(), *g, _st()), "wm_conv2d_dgrad")
    else:
        _ok(lib.wm_conv2d_dgrad_add(dy.data_ptr(), wc.data_ptr(), dres.data_ptr(), dx.data_ptr(), *g, _st()), "wm_conv2d_dgrad_add")
    return dx, dbuf


@pytest.mark.parametrize("route,shape", cc.DGRAD)
def test_input_gradient(lib, route, shape):
    g = cc.geom(shape)
    assert lib.wm_conv2d_route(1, *g, 0, 0) == route and lib.wm_conv2d_route(1, *g, kc.ROUTE_F_RESIDUAL, 0) == route
    for family in kc.CONV_FAMILIES:
        i, ref = _case(family, g)
        dy, wc = _inp(i["dy"]), i["w"].permute(3, 1, 2, 0).contiguous().to(DEV, BF)
        acc = ref["dx_acc"].reshape(ref["dx"].shape)
        dx, dbuf = _dgrad(lib, g, dy, wc)
        _judge(family, _kern(route), "dx", _host(dx, dbuf, "dx"), acc, kc.bf(acc), f"dgrad {shape} {family} dx")
        # the shortcut gradient is added to the ROUNDED tile and the sum rounded again (bf16x8_add in the store loops)
        dx, dbuf = _dgrad(lib, g, dy, wc, _inp(i["dres"]))
        _judge(family, _kern(route), "dx + shortcut", _host(dx, dbuf, "dx"), acc + i["dres"].double(),
               kc.bf(kc.bf(acc) + i["dres"].double()), f"dgrad {shape} {family} dx + shortcut gradient")


def _bnb_tiles(route, g, groups):
    n, h, w = g[0], g[1], g[2]
    if route == kc.route_patch(1, True):
        return kc.pair_tiles(n, h, w)
    return kc.class_tiles(n, h, w, groups) if g[9] == 2 else kc.row_tiles(n * h * w)


@pytest.mark.parametrize("route,shape,groups", cc.DGRAD_BNB)
def test_input_gradient_with_batchnorm_backward_epilogue(lib, route, shape, groups):
    """g = (dgrad (+ shortcut gradient)) * mask and the per-tile (sum g, sum g (bn_y - mean)), all three mask forms, with
    and without the shortcut gradient, against float64.  The `offset` BatchNorm operands (channel mean 50, spread 1) are
    the case an uncentred sum g bn_y would lose to cancellation."""
    g = cc.geom(shape)
    n, h, w, c = g[0], g[1], g[2], g[3]
    rows = n * h * w
    assert lib.wm_conv2d_dgrad_bnstat_ok(*g, groups) == 1 and lib.wm_conv2d_dgrad_bnstat_ok(*cc.geom(cc.BNB_REFUSED), 1) == 0
    tiles = _bnb_tiles(route, g, groups)
    nt = rows // groups // 128
    assert len(tiles) == groups * nt
    first = (route, shape, groups) == cc.DGRAD_BNB[0]
    for family, bn_family in (("lattice", "lattice"), ("randn", "randn")) + ((("randn", "offset"),) if first else ()):
        i, ref = _case(family, g)
        b = kc.bn_inputs(bn_family, rows, c, groups, seed=rows + groups)
        if bn_family == "randn":
            assert kc.bn_preact_margin(b) > 8 * kc.BF16_ULP   # no pre-activation near zero: the recomputed mask is decided
        dy, wc = _inp(i["dy"]), i["w"].permute(3, 1, 2, 0).contiguous().to(DEV, BF)
        bn_y, relu_x, mask = _inp(b["bn_y"]), _inp(b["relu_x"]), _inp(b["mask"], torch.uint8)
        dres = _inp(i["dres"])
        dev = {key: b[key].to(DEV).contiguous() for key in ("mean", "invstd", "gamma", "beta")}
        for form in ("x", "bits") + (("recompute",) if bn_family != "offset" else ()):
            for with_res in (False, True):
                flags = kc.ROUTE_F_BNB | (kc.ROUTE_F_RESIDUAL if with_res else 0)
                assert lib.wm_conv2d_route(1, *g, flags, groups) == route
                res = i["dres"] if with_res else None
                args = (ref["dx_acc"], res, b["bn_y"], b["mean"], b["invstd"], b["gamma"], b["beta"], form, b["relu_x"], b["mask"], tiles)
                r64 = kc.bn_dgrad_epilogue_ref(*args)
                if family == "lattice":
                    kc.lattice_exact({"dx": r64["dx"], "stats": r64["stats"]})
                em = r64 if family == "lattice" else kc.bn_dgrad_epilogue_ref(*args, emulate=True)
                dx, dbuf = _out((n, h, w, c), BF)
                part, pbuf = _out((groups, nt, 2, c), F32)
                _ok(lib.wm_conv2d_dgrad_bnstat(
                    dy.data_ptr(), wc.data_ptr(), dres.data_ptr() if with_res else None, dx.data_ptr(), *g, bn_y.data_ptr(),
                    relu_x.data_ptr() if form == "x" else None, mask.data_ptr() if form == "bits" else None,
                    dev["gamma"].data_ptr() if form == "recompute" else None, dev["beta"].data_ptr() if form == "recompute" else None,
                    dev["mean"].data_ptr(), dev["invstd"].data_ptr(), groups, part.data_ptr(), nt, _st()), "wm_conv2d_dgrad_bnstat")
                what = f"dgrad+bnb {shape} G={groups} {family}/{bn_family} mask {form} shortcut {with_res}"
                _judge(family, _kern(route), "masked dx", _host(dx, dbuf, what).reshape(rows, c), r64["dx"], em["dx"], what + " dx")
                got = _host(part, pbuf, what).reshape(-1, 2, c)
                for j, key in enumerate(("g", "gy")):
                    lat = family == "lattice"
                    _judge(family, _kern(route), ("sum g", "sum g (y - mean)")[j], got[:, j], r64["stats"][:, j],
                           None if lat else kc.tile_sums_f32(em[key], tiles), what + f" slot {j}",
                           f32_floor=0.0 if lat else max(kc.f32_sum_floor(em[key][t]) for t in tiles))


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad(lib, g, dy, x):
    n, h, w, c, k, r, s = g[:7]
    ns = lib.wm_conv2d_wgrad_splits(*g)
    assert ns > 0
    slabs, sbuf = _out((ns, k, r, s, c), F32)
    _ok(lib.wm_conv2d_wgrad(dy.data_ptr(), x.data_ptr(), slabs.data_ptr(), *g, _st()), "wm_conv2d_wgrad")
    grad, gbuf = _out((k, c, r, s), F32)
    _ok(lib.wm_wgrad_finalize(slabs.data_ptr(), ns, k, c, r, s, grad.data_ptr(), 0, _st()), "wm_wgrad_finalize")
    return _host(slabs, sbuf, "slabs").sum(0), _host(grad, gbuf, "dW")


def _wgrad_yardstick(i, ref):
    m, k = ref["cols"].shape[0], i["w"].shape[0]
    dyr = i["dy"].reshape(m, k)
    return (kc.matmul_tn_f32(dyr, ref["cols"]).reshape(ref["dw"].shape),
            float(2.0 ** -24 * (dyr.double().abs().t() @ ref["cols"].abs()).max()))


@pytest.mark.parametrize("route,g,splits", cc.WGRAD)
def test_weight_gradient(lib, route, g, splits):
    """the slabs summed in float64 and the gradient wm_wgrad_finalize delivers, against float64 (the float32 yardstick:
    matmul_tn_f32 on the im2col, in pixel order)"""
    assert lib.wm_conv2d_route(2, *g, 0, 0) == route
    assert splits is None or lib.wm_conv2d_wgrad_splits(*g) == splits
    for family in kc.CONV_FAMILIES:
        i, ref = _case(family, g)
        slab_sum, grad = _wgrad(lib, g, _inp(i["dy"]), _inp(i["x"]))
        dw32, floor = (None, 0.0) if family == "lattice" else _wgrad_yardstick(i, ref)
        _judge(family, _kern(route), "dW slabs", slab_sum, ref["dw"], dw32, f"wgrad {g} {family} slabs", f32_floor=floor)
        _judge(family, _kern(route), "dW", grad, ref["dw"].permute(0, 3, 1, 2), None if dw32 is None else dw32.permute(0, 3, 1, 2),
               f"wgrad {g} {family} delivered", f32_floor=floor)


@pytest.mark.parametrize("route,g", cc.WGRAD_PATCH_OFF)
def test_weight_gradient_without_the_patch_kernel(lib, route, g, monkeypatch):
    """WM_WGRAD_PATCH=0 (read per call) sends the patch shapes to conv_wgrad<64, 8, 3>: same numbers on the lattice"""
    i, ref = _case("lattice", g)
    dy, x = _inp(i["dy"]), _inp(i["x"])
    assert lib.wm_conv2d_route(2, *g, 0, 0) == kc.ROUTE_WGRAD_PATCH64
    on = _wgrad(lib, g, dy, x)
    monkeypatch.setenv("WM_WGRAD_PATCH", "0")
    assert lib.wm_conv2d_route(2, *g, 0, 0) == route
    off = _wgrad(lib, g, dy, x)
    assert torch.equal(on[1], off[1]) and torch.equal(off[1], ref["dw"].permute(0, 3, 1, 2)) and torch.equal(off[0], ref["dw"])
    i, ref = _case("randn", g)
    dw32, floor = _wgrad_yardstick(i, ref)
    slab_sum, grad = _wgrad(lib, g, _inp(i["dy"]), _inp(i["x"]))
    _judge("randn", _kern(route), "dW slabs", slab_sum, ref["dw"], dw32, f"wgrad {g} patch kernel off", f32_floor=floor)


# ------------------------------------------------------------------------------------------------ block order
def _order_runs(monkeypatch, run):
    outs = []
    for v in ("0", "1", "2", "3"):
        monkeypatch.setenv("WM_XCD_SWIZZLE", v)
        outs.append([t.clone() for t in run()])
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])  # noqa: E731
    for v, o in enumerate(outs[1:], 1):
        for a, b in zip(outs[0], o):
            assert torch.equal(bits(a), bits(b)), f"WM_XCD_SWIZZLE={v} changes the result"


@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
def test_block_order_does_not_change_a_bit(lib, family, monkeypatch):
    """WM_XCD_SWIZZLE (read on every call) = 0 .. 3 on grids of fewer than 8 blocks or a count no multiple of 8: the
    per-tile and per-split partial sums do not depend on which block computes them"""
    # conv_igemm forward, 2 x 3 tiles (with statistics: M = 256)
    g = cc.geom((1, 64, 16, 16, 192, 1, 1, 0))
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, 256) == kc.route_igemm(64, 8, 0)
    i, _ = _case(family, g)
    x, wk = _inp(i["x"]), i["w"].to(DEV, BF)
    _order_runs(monkeypatch, lambda: [t for t in _fwd(lib, g, x, wk, 1) if t is not None][::2])
    # conv3x3_patch forward, 9 pairs, with statistics; and conv_wgrad_patch64 on the same shape
    g = cc.geom((2, 64, 24, 24, 64, 3, 1, 1))
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, 1152) == kc.route_patch(0)
    i, _ = _case(family, g)
    x, wk, dy = _inp(i["x"]), i["w"].to(DEV, BF), _inp(i["dy"])
    _order_runs(monkeypatch, lambda: [t for t in _fwd(lib, g, x, wk, 1) if t is not None][::2])
    _order_runs(monkeypatch, lambda: list(_wgrad(lib, g, dy, x)))
    # MODE 2 input gradient, four tiles
    g = cc.geom((2, 64, 16, 16, 128, 3, 2, 1))
    assert lib.wm_conv2d_route(1, *g, 0, 0) == kc.route_igemm(64, 8, 2)
    i, _ = _case(family, g)
    dy, wc = _inp(i["dy"]), i["w"].permute(3, 1, 2, 0).contiguous().to(DEV, BF)
    _order_runs(monkeypatch, lambda: [_dgrad(lib, g, dy, wc)[0]])
    # conv_wgrad<64, 8, 3>: 3 column groups x 1 x 2 splits
    g = cc.geom((1, 64, 9, 11, 64, 3, 1, 1))
    assert lib.wm_conv2d_route(2, *g, 0, 0) == kc.route_wgrad(64, 8, 3) and lib.wm_conv2d_wgrad_splits(*g) == 2
    i, _ = _case(family, g)
    dy, x = _inp(i["dy"]), _inp(i["x"])
    _order_runs(monkeypatch, lambda: list(_wgrad(lib, g, dy, x)))
    # conv_stem_patch, 9 pairs
    shape = (2, 3, 48, 48, 64, 7, 2, 3)
    g = cc.geom(shape)
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, 1152) == kc.ROUTE_STEM_PATCH
    xs, ws = _stem_operands(lib, _stem_inputs(family, shape), False)
    _order_runs(monkeypatch, lambda: [t for t in _fwd(lib, g, xs, ws, 1) if t is not None][::2])
