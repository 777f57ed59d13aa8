"""bias / activation (bias_act_fwd, colsum_kernel), Linear (tiled GEMM and the C = 192 / k = 192 panel kernel) and the
GELU MLP epilogues (wm_linear_bias_gelu_fwd, wm_linear_dgrad_gelu) against float64, judged by tests/kernel_check.py.
Activation inputs cover [-12, 12] on a grid with exact 0 and its bf16 neighbours, in addition to randn."""
import kernel_check as kc
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("rows,c", [(264, 64), (197, 384), (33, 8)])
def test_bias_act_on_the_grid(rows, c, act, res):
    from ssl_wafermap_amd import vit_ops

    g = torch.Generator().manual_seed(rows + act)
    x = kc.act_grid(rows, c, seed=rows)
    bias = torch.randn(c, generator=g) * 0.3
    bias[:8] = 0.0                                    # row 0, columns 0..7 hold the exact 0 and the neighbours of 0
    r = kc.bf(torch.randn(rows, c, generator=g)) if res else None
    dy = kc.bf(torch.randn(rows, c, generator=g) + 3.0)
    ref = kc.bias_act_ref(x, bias, act, r, dy)
    emul = kc.bias_act_ref(x, bias, act, r, dy, emulate=True)
    xd, bd = x.to(DEV).bfloat16().requires_grad_(True), bias.to(DEV).requires_grad_(True)
    rd = r.to(DEV).bfloat16().requires_grad_(True) if res else None
    y = vit_ops.bias_act(xd, bd, act, rd)
    y.backward(dy.to(DEV).bfloat16())
    tag = f"bias_act act={act} res={res} {rows}x{c}"
    kc.check(y, ref[0], emul[0], f"{tag} y")
    kc.check(xd.grad, ref[1], emul[1], f"{tag} dx")
    # the sums see the rounded dx: reference = float64 sum of the kernel's own dx, yardstick = float32 sum in row order
    dx_own = xd.grad.float().cpu()
    kc.check(bd.grad, dx_own.double().sum(0), kc.colsum_f32(dx_own), f"{tag} dbias", factor=kc.F32_SUM_FACTOR,
             abs_floor=kc.f32_sum_floor(dx_own))
    if res:
        assert torch.equal(rd.grad.float().cpu(), dy)
    if act == 2:  # ReLU gradient at exactly 0 (x + bias == 0) is 0, as torch
        zero = (x[0, :8] == 0)
        assert zero.sum() == 2 and torch.equal(xd.grad[0, :8].float().cpu()[zero], torch.zeros(2))


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_dbias_at_25216_rows_with_nonzero_mean(act):
    from ssl_wafermap_amd import vit_ops

    rows, c = 25216, 192
    g = torch.Generator().manual_seed(act)
    x = kc.bf(torch.randn(rows, c, generator=g) * 1.5)
    bias = torch.randn(c, generator=g) * 0.3
    dy = kc.bf(torch.randn(rows, c, generator=g) + 3.0)
    xd, bd = x.to(DEV).bfloat16().requires_grad_(True), bias.to(DEV).requires_grad_(True)
    vit_ops.bias_act(xd, bd, act).backward(dy.to(DEV).bfloat16())
    ref = kc.bias_act_ref(x, bias, act, None, dy)
    emul = kc.bias_act_ref(x, bias, act, None, dy, emulate=True)
    kc.check(xd.grad, ref[1], emul[1], f"bias_act act={act} 25216x192 dx")
    dx_own = xd.grad.float().cpu()
    kc.check(bd.grad, dx_own.double().sum(0), kc.colsum_f32(dx_own), f"bias_act act={act} 25216x192 dbias", factor=kc.F32_SUM_FACTOR,
             abs_floor=kc.f32_sum_floor(dx_own))


# the shapes of test_gpu_vit.py::test_linear_bias_gradient_rides_in_wgrad (tiled kernel; c = 192 forward and k = 192 input
# gradient: the panel kernel) plus rows 1, 127, 129
LINEAR = [(591, 384, 1152, False), (100, 768, 3072, False), (1000, 1536, 384, True), (37, 512, 512, True),
          (5000, 384, 384, False), (64, 256, 2048, False), (300, 192, 576, False), (5000, 192, 192, True),
          (131, 192, 768, False), (1000, 768, 192, True), (25216, 192, 576, False),
          (1, 384, 384, True), (127, 384, 1152, False), (129, 768, 384, True),
          (1, 192, 576, False), (127, 192, 384, True), (129, 192, 768, False), (1, 768, 192, True), (129, 384, 192, False)]


@pytest.mark.parametrize("rows,c,k,res", LINEAR)
def test_linear(rows, c, k, res):
    from ssl_wafermap_amd import vit_ops

    g = torch.Generator().manual_seed(rows + k)
    x = kc.bf(torch.randn(rows, c, generator=g))
    w = kc.bf(torch.randn(k, c, generator=g) * 0.05)
    b = torch.randn(k, generator=g) * 0.2
    r = kc.bf(torch.randn(rows, k, generator=g)) if res else None
    dy = kc.bf(torch.randn(rows, k, generator=g) + 0.5)
    ref = kc.linear_ref(x, w, b, r, dy)
    emul = kc.linear_ref(x, w, b, r, dy, emulate=True)
    dw32, db32 = kc.linear_param_grads_f32(x, dy)
    xd, wd, bd = x.to(DEV).bfloat16().requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    rd = r.to(DEV).bfloat16().requires_grad_(True) if res else None
    y = vit_ops.linear(xd, wd, bd, residual=rd)
    y.backward(dy.to(DEV).bfloat16())
    tag = f"linear {rows}x{c}->{k} res={res}"
    kc.check(y, ref[0], emul[0], f"{tag} y")
    kc.check(xd.grad, ref[1], emul[1], f"{tag} dx")
    kc.check(wd.grad, ref[2], dw32, f"{tag} dW", factor=kc.F32_SUM_FACTOR,
             abs_floor=float(2.0 ** -24 * (dy.double().abs().t() @ x.double().abs()).max()))
    kc.check(bd.grad, ref[3], db32, f"{tag} dbias", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy))
    if res:
        assert torch.equal(rd.grad.float().cpu(), dy)


@pytest.mark.parametrize("rows,c,hid", [(264, 64, 64), (264, 192, 384), (129, 192, 768), (127, 384, 1536)])
def test_mlp_gelu_epilogues_on_the_grid(rows, c, hid):
    """wm_linear_bias_gelu_fwd / wm_linear_dgrad_gelu through vit_ops.mlp_gelu.  With fc1 = [I; -I; ...] and a zero bias
    the pre-activations ARE the activation grid (and its negative), so the GELU epilogues see [-12, 12], exact 0 and
    the neighbours of 0; the last case has random weights."""
    from ssl_wafermap_amd import vit_ops

    g = torch.Generator().manual_seed(rows + hid)
    if hid <= 2 * c:
        x = kc.act_grid(rows, c, seed=hid)
        w1 = torch.cat([torch.eye(c) * (-1.0) ** i for i in range(hid // c)])
        b1 = torch.zeros(hid)
    else:
        x = kc.bf(torch.randn(rows, c, generator=g))
        w1 = kc.bf(torch.randn(hid, c, generator=g) * c ** -0.5)
        b1 = torch.randn(hid, generator=g) * 0.1
    w2 = kc.bf(torch.randn(c, hid, generator=g) * hid ** -0.5)
    b2 = torch.randn(c, generator=g) * 0.1
    res, dy = kc.bf(torch.randn(rows, c, generator=g)), kc.bf(torch.randn(rows, c, generator=g))
    ref = kc.mlp_ref(x, w1, b1, w2, b2, res, dy)
    emul = kc.mlp_ref(x, w1, b1, w2, b2, res, dy, emulate=True)
    dev = [t.to(DEV).requires_grad_(True) for t in (x.bfloat16(), w1, b1, w2, b2, res.bfloat16())]
    y = vit_ops.mlp_gelu(*dev)
    y.backward(dy.to(DEV).bfloat16())
    tag = f"mlp {rows}x{c} hid={hid}"
    kc.check(y, ref["y"], emul["y"], f"{tag} y")
    kc.check(dev[0].grad, ref["dx"], emul["dx"], f"{tag} dx")
    # float32 parameter gradients: float32 products of the emulation's own bf16 operands
    kc.check(dev[1].grad, ref["dw1"], emul["dpre"].float().t() @ x.float(), f"{tag} dW1")
    kc.check(dev[2].grad, ref["db1"], kc.colsum_f32(emul["dpre"]), f"{tag} db1")
    kc.check(dev[3].grad, ref["dw2"], dy.float().t() @ emul["hid"].float(), f"{tag} dW2")
    kc.check(dev[4].grad, ref["db2"], kc.colsum_f32(dy), f"{tag} db2", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy))
    with torch.no_grad():  # the one-launch form where it is served (C = 192): the same bound
        y2 = vit_ops.mlp_gelu(*[t.detach() for t in dev])
    kc.check(y2, ref["y"], emul["y"], f"{tag} y (no-grad path)")
