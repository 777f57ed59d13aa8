"""LayerNorm kernels (ln_fwd / ln_bwd in csrc/transformer.hip, wm_ln_fragments in csrc/ln_regs.h behind wm_ln_linear_fwd
and wm_ln_mlp_fused_fwd) against float64, judged by tests/kernel_check.py.  Input families where eps, a one-pass
variance, a skipped column piece or a hard-coded eps decide the result; both sides of every instantiation edge of the
width dispatch; row counts around the rows-per-wave / rows-per-block edges and beyond the grid caps."""
import kernel_check as kc
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _separate(family, rows, c, eps, seed=None, dy_shift=0.0, forms=("plain", "skip")):
    from ssl_wafermap_amd import vit_ops

    x, gamma, beta, dy, dres = kc.layer_norm_inputs(family, rows, c, seed=rows * 7 + c if seed is None else seed)
    if dy_shift:
        dy = kc.bf(dy + dy_shift)
    tag = f"LayerNorm {family} {rows}x{c} eps={eps:g}"
    dg32, db32 = kc.layer_norm_param_grads_f32(x, dy, eps)
    for form in forms:
        skip = dres if form == "skip" else None
        ref = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip)
        emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
        xd = x.to(DEV).bfloat16().requires_grad_(True)
        gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        if form == "skip":
            y, sk = vit_ops.layer_norm_skip(xd, gd, bd, eps)
            assert torch.equal(sk.detach(), xd.detach())
            torch.autograd.backward([y, sk], [dy.to(DEV).bfloat16(), dres.to(DEV).bfloat16()])
        else:
            y = vit_ops.layer_norm(xd, gd, bd, eps)
            y.backward(dy.to(DEV).bfloat16())
        kc.check(y, ref[0], emul[0], f"{tag} {form} y")
        kc.check(xd.grad, ref[1], emul[1], f"{tag} {form} dx")
        xh = kc.layer_norm_ref(x, gamma * 0 + 1, beta * 0, eps)[0]
        kc.check(gd.grad, ref[2], dg32, f"{tag} {form} dgamma", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy * xh))
        kc.check(bd.grad, ref[3], db32, f"{tag} {form} dbeta", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy))
        if family == "constant":  # exactly constant rows: y = bf16(beta), whatever eps
            assert torch.equal(y.detach().float().cpu(), beta.bfloat16().float().expand(rows, c))
            assert torch.isfinite(xd.grad).all() and torch.isfinite(gd.grad).all()


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("family", kc.LN_FAMILIES)
@pytest.mark.parametrize("rows,c", [(130, 768), (37, 192), (1000, 384)])
def test_families_and_eps(family, rows, c, eps):
    _separate(family, rows, c, eps)


# 256 / 264, 512 / 520, 1024 / 1032: both sides of the ln_fwd / ln_bwd instantiations; 2048: the widest accepted;
# 1000: a multiple of 8 and of nothing larger
@pytest.mark.parametrize("c", [8, 192, 256, 264, 384, 512, 520, 768, 1000, 1024, 1032, 2048])
def test_widths(c):
    _separate("randn", 67, c, 1e-6)
    _separate("tight", 67, c, 1e-6, forms=("plain",))


@pytest.mark.parametrize("c", [192, 768, 2048])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65])
def test_row_counts(rows, c):
    _separate("mean300", rows, c, 1e-5)


@pytest.mark.parametrize("rows,c", [(49300, 192), (24700, 512), (6200, 2048)])
def test_rows_beyond_the_grid_cap(rows, c):
    """More rows than 1536 forward blocks (768 backward blocks) cover in one trip: blocks stride over rows."""
    _separate("randn", rows, c, 1e-6, forms=("skip",))


@pytest.mark.parametrize("c", [192, 384])
def test_parameter_gradients_with_nonzero_column_mean(c):
    """dgamma / dbeta at 25216 rows (a DINO ViT-Tiny step's row count) with dy = randn + 3: a dropped block of rows or a
    float32 ordering problem shows against the float64 sums."""
    _separate("randn", 25216, c, 1e-6, dy_shift=3.0)


@pytest.mark.parametrize("rows,c,with_res", [(25216, 192, True), (1000, 384, False), (67, 1000, True)])
def test_slot_form(rows, c, with_res):
    """wm_layernorm_bwd_parts: per-block channel sums stored as slots [2][blocks][C]; added in order they are dgamma and
    dbeta, and dx is the atomic form's to the bit."""
    from ssl_wafermap_amd import _lib

    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    eps = 1e-6
    x, gamma, beta, dy, dres = kc.layer_norm_inputs("randn", rows, c, seed=rows + c)
    dy = kc.bf(dy + 3.0)
    skip = dres if with_res else None
    xd, dyd = x.to(DEV).bfloat16(), dy.to(DEV).bfloat16()
    rd = dres.to(DEV).bfloat16() if with_res else None
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y, dx, dx2 = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    _lib.check(lib.wm_layernorm_fwd(ptr(xd), ptr(gd), ptr(bd), eps, rows, c, ptr(y), ptr(mean), ptr(rstd), st()), "fwd")
    nb = int(lib.wm_layernorm_bwd_blocks(rows, c))
    assert nb > 0
    part = torch.full((2, nb, c), float("nan"), device=DEV)   # every slot must be overwritten
    _lib.check(lib.wm_layernorm_bwd_parts(ptr(xd), ptr(dyd), ptr(gd), ptr(mean), ptr(rstd), rows, c, ptr(rd), ptr(dx),
                                          ptr(part), st()), "bwd_parts")
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    if with_res:
        _lib.check(lib.wm_layernorm_bwd_add(ptr(xd), ptr(dyd), ptr(gd), ptr(mean), ptr(rstd), rows, c, ptr(rd), ptr(dx2),
                                            ptr(dg), ptr(db), st()), "bwd_add")
    else:
        _lib.check(lib.wm_layernorm_bwd(ptr(xd), ptr(dyd), ptr(gd), ptr(mean), ptr(rstd), rows, c, ptr(dx2), ptr(dg),
                                        ptr(db), st()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    ref = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip)
    emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
    dg32, db32 = kc.layer_norm_param_grads_f32(x, dy, eps)
    tag = f"LayerNorm slots {rows}x{c}"
    kc.check(dx, ref[1], emul[1], f"{tag} dx")
    xh = kc.layer_norm_ref(x, gamma * 0 + 1, beta * 0, eps)[0]
    kc.check(kc.colsum_f32(part[0].cpu()), ref[2], dg32, f"{tag} dgamma", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy * xh))
    kc.check(kc.colsum_f32(part[1].cpu()), ref[3], db32, f"{tag} dbeta", factor=kc.F32_SUM_FACTOR, abs_floor=kc.f32_sum_floor(dy))
    # the statistics the backward reads: float32 mean and 1 / sqrt(var + eps)
    xs = x.double()
    m32 = kc.colsum_f32(x.t()) / c                                                  # float32 sums in column order
    v32 = kc.colsum_f32((x.float() - m32[:, None]).pow(2).t()) / c
    kc.check(mean, xs.mean(1), m32, f"{tag} mean")
    kc.check(rstd, (xs.var(1, unbiased=False) + eps).rsqrt(), (v32 + eps).rsqrt(), f"{tag} rstd")


# ------------------------------------------------------------------------------------- LayerNorm inside the GEMMs
def _fused_inputs(family, rows, n, hid, seed):
    c = 192
    x, gamma, beta, _, _ = kc.layer_norm_inputs(family, rows, c, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    w = kc.bf(torch.randn(n, c, generator=g) * c ** -0.5)
    b = torch.randn(n, generator=g) * 0.2
    w1 = kc.bf(torch.randn(hid, c, generator=g) * c ** -0.5)
    w2 = kc.bf(torch.randn(c, hid, generator=g) * hid ** -0.5)
    b1, b2 = torch.randn(hid, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
    return x, gamma, beta, w, b, w1, b1, w2, b2


def _fused(family, rows, n, eps, hid=768):
    from ssl_wafermap_amd import vit_ops

    x, gamma, beta, w, b, w1, b1, w2, b2 = _fused_inputs(family, rows, n, hid, seed=rows + n)
    dev = [t.to(DEV) for t in (gamma, beta, w, b, w1, b1, w2, b2)]
    xd = x.to(DEV).bfloat16()
    tag = f"{family} rows={rows} eps={eps:g}"
    with torch.no_grad():
        y = vit_ops.ln_linear(xd, dev[0], dev[1], eps, dev[2], dev[3])
        assert y is not None, "wm_ln_linear_fwd must serve C = 192"
        z = vit_ops.ln_mlp_gelu(xd, dev[0], dev[1], eps, dev[4], dev[5], dev[6], dev[7])
        assert z is not None, "wm_ln_mlp_fused_fwd must serve C = 192"
    ln64 = kc.layer_norm_ref(x, gamma, beta, eps)[0]
    lnem = kc.layer_norm_ref(x, gamma, beta, eps, emulate=True)[0]
    kc.check(y, kc.linear_ref(ln64, w, b)[0], kc.linear_ref(lnem, w, b, emulate=True)[0], f"ln_linear N={n} {tag}")
    kc.check(z, kc.mlp_ref(x, w1, b1, w2, b2, res=x, ln=(gamma, beta, eps))["y"],
             kc.mlp_ref(x, w1, b1, w2, b2, res=x, ln=(gamma, beta, eps), emulate=True)["y"], f"ln_mlp hid={hid} {tag}")


@pytest.mark.parametrize("n", [384, 576, 768])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 32768])
def test_fused_forms_rows_and_widths(rows, n):
    """32768 rows: the largest count wm_mlp_fused_fwd_ok accepts."""
    _fused("randn", rows, n, 1e-6, hid={384: 768, 576: 384, 768: 1536}[n])


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("family", kc.LN_FAMILIES)
def test_fused_forms_families_and_eps(family, eps):
    _fused(family, 129, 576, eps)
