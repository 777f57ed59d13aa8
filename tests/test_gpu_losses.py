"""The loss kernels of csrc/embed.hip against float64, through the lowest Python entry point that reaches each.

Every output tensor goes through tests/kernel_check.py::check with the float32 restatement of tests/loss_cases.py as the
yardstick (loss_cases.check_f32: F32_SUM_FACTOR and one float32 rounding at the operands' scale as the floor; bf16 outputs
with the default factor against the emulation that rounds where the kernel does); every scalar loss gets the derived
summation bound loss_cases.scalar_bound.  No tolerance here is a literal.  A test that claims a launch path asserts it
through the Python mirror of embed.hip's launch arithmetic.  tests/test_kernel_check_cpu.py proves on the CPU that these
criteria reject every seeded error of loss_cases at these shapes."""
import functools

import kernel_check as kc
import loss_cases as lc
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def lib():
    from ssl_wafermap_amd import _lib

    return _lib.load()


def HipError():
    """the exception type the ctypes wrapper raises for a non-zero return code of the library"""
    from ssl_wafermap_amd import _lib

    return _lib.WaferHipError


def call(fn_name, *args):
    from ssl_wafermap_amd import _lib

    _lib.check(getattr(lib(), fn_name)(*args, _lib.stream_ptr()), fn_name)


def ptr(t):
    return 0 if t is None else int(t.data_ptr())


def f32c(got, ref, emul, what, floor, kernel):
    """(the kernel's name goes into the record of the comparison: profiles/loss_kernel_check.md groups by it)"""
    lc.check_f32(got, ref, emul, f"[{kernel}] {what}", floor)


def bf16c(got, ref, emul, what, kernel, floor=0.0):
    lc.check_bf16(got, ref, emul, f"[{kernel}] {what}", floor)


def scalar(got, r64, r32, chain, what, kernel):
    lc.check_scalar(got, r64["terms"], r32["terms"], chain, f"[{kernel}] {what}", r64.get("mags"))


# ---------------------------------------------------------------------------------------------------- NT-Xent
@functools.lru_cache(maxsize=4)
def nx_case(family, b_local, world, rank, d, temp):
    z0, z1 = lc.ntxent_inputs(family, b_local * world, d, seed=b_local + d)
    bg = b_local * world
    zall = lc.normalized32(torch.cat([z0, z1]))
    zn = torch.cat([zall[rank * b_local:(rank + 1) * b_local], zall[bg + rank * b_local:bg + (rank + 1) * b_local]]).contiguous()
    args = (zn, zall, b_local, bg, rank * b_local, temp, 1.0 / (2 * b_local))
    return args, lc.ntxent(*args, dt=F64), lc.ntxent(*args, dt=F32)


def run_ntxent(family, b_local, world, rank, d, temp, tag):
    from ssl_wafermap_amd import functional as Fh

    args, ref, emul = nx_case(family, b_local, world, rank, d, temp)
    zn, zall, _, bg, off, _, gs = args
    zn_d, zall_d = zn.to(DEV), zall.to(DEV)
    lse, rows = Fh.ntxent_forward(zn_d, zall_d, b_local, bg, off, temp)
    floor = lc.ntxent_lse_floor(temp, ref)
    kern = f"ntxent_fwd_kernel<{lc.nx_fwd_rpw(b_local)}>"
    f32c(lse, ref["lse"], emul["lse"], f"{tag} lse", floor, kern)
    f32c(rows, ref["loss_rows"], emul["loss_rows"], f"{tag} loss_rows", floor, kern)
    if world == 1:
        lse_all = lse
    else:   # the ranks' all-gather of the kernel's own lse: every rank's forward, reassembled view-major
        parts = []
        for r in range(world):
            loc = torch.cat([zall_d[r * b_local:(r + 1) * b_local], zall_d[bg + r * b_local:bg + (r + 1) * b_local]]).contiguous()
            parts.append(Fh.ntxent_forward(loc, zall_d, b_local, bg, r * b_local, temp)[0])
        lse_all = torch.cat([torch.cat([p[:b_local] for p in parts]), torch.cat([p[b_local:] for p in parts])])
    dzn = Fh.ntxent_backward(zn_d, zall_d, lse_all, b_local, bg, off, temp, gs)
    nsplit = lc.nx_bwd_plan(b_local, bg)[1]
    f32c(dzn, ref["dzn"], emul["dzn"], f"{tag} dzn", ref["dzn_floor"], "ntxent_bwd_kernel" + (" + reduce" if nsplit > 1 else ""))
    return dzn.cpu(), ref, emul


NX_SHAPES = [  # b, d, RPW, (rowtiles, nsplit, tiles_per_split), what it reaches
    (1, 32, 2, (1, 1, 1), "two rows: one positive and no other negative, one ragged tile, no reduce"),
    (31, 96, 2, (2, 1, 1), "one column tile, nu = 3, ragged row block"),
    (32, 96, 2, (2, 1, 1), "exactly one column tile"),
    (33, 96, 2, (3, 2, 1), "two column tiles, the second with 2 columns"),
    (256, 256, 2, (16, 8, 1), "tiles_per_split = 1, 8 slabs, maximum LDS"),
    (1024, 32, 2, (64, 4, 8), "the last RPW = 2 shape"),
    (1025, 32, 8, (65, 3, 11), "the first RPW = 8 shape, last row block of 2 rows, tiles_per_split = 11, nsplit = 3"),
    (1100, 32, 8, (69, 3, 12), "tiles_per_split = 12, last split 11 tiles, last tile 24 columns"),
    (2049, 32, 8, (129, 1, 65), "nsplit = 1 over 65 column tiles: direct store, no reduce"),
]


@pytest.mark.parametrize("b,d,rpw,plan,why", NX_SHAPES, ids=[f"b{s[0]}-d{s[1]}" for s in NX_SHAPES])
def test_ntxent_launch_paths(b, d, rpw, plan, why):
    assert lc.nx_fwd_rpw(b) == rpw and lc.nx_bwd_plan(b, b) == plan, why
    if (b, d) == (256, 256):
        assert lc.nx_bwd_lds_bytes(d) == 107648
    if b == 1100:
        assert lc.cdiv(2 * b, 64) - 2 * plan[2] == 11 and (2 * b) % 64 == 24
    run_ntxent("randn", b, 1, 0, d, 0.5, f"ntxent b={b} d={d}")


@pytest.mark.parametrize("family", lc.NTXENT_FAMILIES)
@pytest.mark.parametrize("temp", [0.5, 0.07, 0.01])
@pytest.mark.parametrize("b,d", [(33, 96), (256, 32)])
def test_ntxent_families_and_temperatures(family, temp, b, d):
    _, ref, _ = run_ntxent(family, b, 1, 0, d, temp, f"ntxent {family} b={b} T={temp}")
    if family == "collapsed":
        assert abs(float(ref["loss_rows"].mean()) - torch.log(torch.tensor(2.0 * b - 1)).item()) < 1e-5   # (the reference itself)


@pytest.mark.parametrize("world,b_local,rank,d", [(3, 37, 0, 32), (3, 37, 1, 32), (3, 37, 2, 32), (2, 1025, 1, 32)])
def test_ntxent_gathered(world, b_local, rank, d):
    """b_global > b_local: self and positive columns sit rank_offset columns off the diagonal -- at world = 2, b_local = 1025
    in other column tiles and other splits than the row's own."""
    bg = world * b_local
    if b_local == 1025:
        rowtiles, nsplit, tps = lc.nx_bwd_plan(b_local, bg)
        assert lc.nx_fwd_rpw(b_local) == 8 and nsplit > 1 and tps > 1
        assert (rank * b_local) // (tps * 64) != (bg + rank * b_local) // (tps * 64)      # self and positive: different splits
    dzn, ref, emul = run_ntxent("randn", b_local, world, rank, d, 0.5, f"ntxent gathered world={world} rank={rank}")
    # ... and in the tangent space of the unit rows, which is what reaches the projections
    zl = nx_case("randn", b_local, world, rank, d, 0.5)[0][0].double()
    proj = lambda t: t.double() - zl * (t.double() * zl).sum(1, keepdim=True)  # noqa: E731
    f32c(proj(dzn), proj(ref["dzn"]), proj(emul["dzn"]), "ntxent gathered tangent dzn", ref["dzn_floor"], "ntxent_bwd_kernel + reduce")


def test_ntxent_rejections():
    from ssl_wafermap_amd import functional as Fh

    for d in (100, 288):
        zn = torch.zeros(16, d, device=DEV)
        with pytest.raises(HipError(), match="wm_ntxent_fwd"):
            Fh.ntxent_forward(zn, zn, 8, 8, 0, 0.5)
        with pytest.raises(HipError(), match="wm_ntxent_bwd"):
            Fh.ntxent_backward(zn, zn, torch.zeros(16, device=DEV), 8, 8, 0, 0.5, 1.0)
    zn, zall = torch.zeros(16, 32, device=DEV), torch.zeros(32, 32, device=DEV)
    with pytest.raises(HipError(), match="wm_ntxent_fwd"):
        Fh.ntxent_forward(zn, zall, 8, 16, 9, 0.5)
    with pytest.raises(HipError(), match="wm_ntxent_bwd"):
        Fh.ntxent_backward(zn, zall, torch.zeros(32, device=DEV), 8, 16, 9, 0.5, 1.0)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ntxent_stacked_projection_node(dtype):
    """_NTXentProjections on raw projections: wm_l2_normalize -> NT-Xent -> l2norm_bwd with the DEVICE scale (3 loss)."""
    from ssl_wafermap_amd.loss import NTXentLoss, stacked_views

    b, d, temp, up = 33, 96, 0.5, 3.0
    z0, z1 = lc.ntxent_inputs("randn", b, d, seed=5)
    z = torch.cat([z0, z1]) * 2
    z = kc.bf(z) if dtype == BF16 else z
    out = {}
    for dt in (F64, F32):
        n = lc.l2norm(z, 1e-12, dt=dt)
        nx = lc.ntxent(n["y"], n["y"], b, b, 0, temp, 1.0 / (2 * b), dt=dt)
        back = lc.l2norm(z, 1e-12, dy=nx["dzn"], scale=up, dt=dt, dx_bf16=dtype == BF16)
        out[dt] = {"terms": nx["loss_rows"] / (2 * b), "dz": back["dx"], "floor": lc.mag_floor(back["dx_terms"])}
    zd = z.to(DEV).to(dtype).requires_grad_(True)
    loss = NTXentLoss(temperature=temp)(*stacked_views(zd, b))
    assert type(loss.grad_fn).__name__ == "_NTXentProjectionsBackward"
    (up * loss).backward()
    scalar(loss.detach(), out[F64], out[F32], 2 * b, f"projection node loss {dtype}", "wm_mean_f32(ntxent rows)")
    if dtype == BF16:
        bf16c(zd.grad, out[F64]["dz"], out[F32]["dz"], "projection node dz bf16", "l2norm_bwd<float, bf16>", out[F64]["floor"])
    else:
        f32c(zd.grad, out[F64]["dz"], out[F32]["dz"], "projection node dz", out[F64]["floor"], "l2norm_bwd<float, float>")


# ---------------------------------------------------------------------------------------------------- L2 normalise
@pytest.mark.parametrize("rows", [1, 3, 5, 300])
@pytest.mark.parametrize("d", [1, 8, 63, 64, 65, 100, 513])
def test_l2_normalize_all_dtypes(rows, d):
    """forward and backward kernels called as loss.py calls them, the four dtype combinations each, eps 1e-12 and 1e-3, with
    (from 3 rows on) a zero row and a row of norm eps / 2; the backward with and without the device scale"""
    from ssl_wafermap_amd import _lib

    for eps in (1e-12, 1e-3):
        for bf_in in (False, True):
            x, dy32 = lc.l2norm_inputs(rows, d, eps, seed=rows * 7 + d, bf16_in=bf_in)
            ref = lc.l2norm(x, eps, dt=F64)
            assert float((ref["norm"] / float(torch.tensor(eps, dtype=F32)) - 1).abs().min()) > 0.4     # nothing near the switch
            live = ref["norm"] > eps
            xd = x.to(DEV).to(BF16 if bf_in else F32)
            for bf_out in (False, True):
                emul = lc.l2norm(x, eps, dt=F32, y_bf16=bf_out)
                y = torch.empty(rows, d, dtype=BF16 if bf_out else F32, device=DEV)
                inv = torch.empty(rows, dtype=F32, device=DEV)
                call("wm_l2_normalize", ptr(xd), _lib.dtype_code(xd), rows, d, eps, ptr(y), _lib.dtype_code(y), ptr(inv))
                tag = f"l2norm {rows}x{d} eps={eps:g} in={'bf16' if bf_in else 'f32'} out={'bf16' if bf_out else 'f32'}"
                kern = f"l2norm_fwd<{'bf16' if bf_in else 'float'}, {'bf16' if bf_out else 'float'}>"
                if bf_out:
                    bf16c(y, ref["y"], emul["y"], f"{tag} y", kern)
                else:
                    f32c(y, ref["y"], emul["y"], f"{tag} y", lc.f32_floor(ref["y"]), kern)
                # clamped rows hold 1 / eps (1e12): compared apart, so that their scale does not hide the live rows
                for sel in (live, ~live):
                    if bool(sel.any()):
                        f32c(inv.cpu()[sel], ref["inv_norm"][sel], emul["inv_norm"][sel], f"{tag} inv_norm", lc.f32_floor(ref["inv_norm"][sel]), kern)
            # backward: reads the float32 y and inv_norm of the forward
            yd = torch.empty(rows, d, dtype=F32, device=DEV)
            invd = torch.empty(rows, dtype=F32, device=DEV)
            call("wm_l2_normalize", ptr(xd), _lib.dtype_code(xd), rows, d, eps, ptr(yd), _lib.WM_F32, ptr(invd))
            for bf_dy in (False, True):
                dy = kc.bf(dy32) if bf_dy else dy32
                dyd = dy.to(DEV).to(BF16 if bf_dy else F32)
                for bf_dx in (False, True):
                    scale = 3.0 if bf_dy == bf_dx else None
                    r64 = lc.l2norm(x, eps, dy, scale or 1.0, dt=F64)
                    r32 = lc.l2norm(x, eps, dy, scale or 1.0, dt=F32, dx_bf16=bf_dx)
                    dx = torch.empty(rows, d, dtype=BF16 if bf_dx else F32, device=DEV)
                    sc = torch.tensor([scale], dtype=F32, device=DEV) if scale else None
                    call("wm_l2_normalize_bwd", ptr(dyd), _lib.dtype_code(dyd), ptr(yd), ptr(invd), rows, d, ptr(dx), _lib.dtype_code(dx), ptr(sc))
                    kern = f"l2norm_bwd<{'bf16' if bf_dy else 'float'}, {'bf16' if bf_dx else 'float'}>"
                    tag = f"l2norm bwd {rows}x{d} eps={eps:g} x={'bf16' if bf_in else 'f32'} dy={'bf16' if bf_dy else 'f32'} dx={'bf16' if bf_dx else 'f32'}"
                    for sel in (live, ~live):
                        if not bool(sel.any()):
                            continue
                        floor = lc.mag_floor(r64["dx_terms"][sel])       # dy - y <y, dy>: the two can cancel
                        if bf_dx:
                            bf16c(dx.cpu()[sel], r64["dx"][sel], r32["dx"][sel], f"{tag} dx", kern, floor)
                        else:
                            f32c(dx.cpu()[sel], r64["dx"][sel], r32["dx"][sel], f"{tag} dx", floor, kern)


@pytest.mark.parametrize("rows,d", [(3, 8), (5, 100), (300, 513)])
@pytest.mark.parametrize("mode", ["f32", "bf16_in", "bf16_rows"])
def test_l2_normalize_autograd_node(rows, d, mode):
    """functional.l2_normalize and its backward node: float32 rows from a float32 or a bf16 input (the gradient leaves in the
    input's dtype), and differentiable_bf16 (bf16 rows out, bf16 gradients in and out)"""
    from ssl_wafermap_amd import functional as Fh

    eps = 1e-3
    x, w = lc.l2norm_inputs(rows, d, eps, seed=rows + d, bf16_in=mode != "f32")
    bf_rows = mode == "bf16_rows"
    dy = kc.bf(w) if bf_rows else w                    # (y * w).sum(): autograd hands the node w in y's dtype
    r64 = lc.l2norm(x, eps, dy, dt=F64)
    r32 = lc.l2norm(x, eps, dy, dt=F32, y_bf16=bf_rows, dx_bf16=mode != "f32")
    assert float((r64["norm"] / eps - 1).abs().min()) > 0.4
    xd = x.to(DEV).to(F32 if mode == "f32" else BF16).requires_grad_(True)
    y = Fh.l2_normalize(xd, eps=eps, differentiable_bf16=bf_rows)
    assert y.dtype == (BF16 if bf_rows else F32)
    (y.float() * w.to(DEV)).sum().backward()
    assert xd.grad.dtype == xd.dtype
    tag = f"l2_normalize node {rows}x{d} {mode}"
    floor = lc.mag_floor(r64["dx_terms"])
    if bf_rows:
        bf16c(y, r64["y"], r32["y"], f"{tag} y", "l2norm_fwd + cast")
    else:
        f32c(y, r64["y"], r32["y"], f"{tag} y", lc.f32_floor(r64["y"]), "l2norm_fwd")
    live = r64["norm"] > eps
    for sel in (live, ~live):
        if mode == "f32":
            f32c(xd.grad.cpu()[sel], r64["dx"][sel], r32["dx"][sel], f"{tag} dx", lc.mag_floor(r64["dx_terms"][sel]), "l2norm_bwd node")
        else:
            bf16c(xd.grad.cpu()[sel], r64["dx"][sel], r32["dx"][sel], f"{tag} dx", "l2norm_bwd node", lc.mag_floor(r64["dx_terms"][sel]))


# ---------------------------------------------------------------------------------------------------- MoCo bank
BANK_SHAPES = [(1, 32, 1), (48, 128, 200), (5, 100, 63), (300, 128, 4097), (3, 512, 15360)]


@pytest.mark.parametrize("b,d,k", BANK_SHAPES)
@pytest.mark.parametrize("temp", [0.1, 0.01])
@pytest.mark.parametrize("tie", [False, True])
def test_bank_loss(b, d, k, temp, tie):
    from ssl_wafermap_amd.loss import _NTXentBank

    if (b, d, k) == BANK_SHAPES[-1]:
        assert 2 * d + k == lc.BANK_LDS_FLOATS          # at the LDS limit
    q, kp, bank = lc.bank_inputs(b, d, k, seed=b + k, key_in_bank=tie)
    r64, r32 = lc.bank_loss(q, kp, bank, temp, dt=F64), lc.bank_loss(q, kp, bank, temp, dt=F32)
    qd, kd = q.to(DEV).requires_grad_(True), kp.to(DEV).requires_grad_(True)
    loss = _NTXentBank.apply(qd, kd, bank.to(DEV), temp)
    loss.backward()
    tag = f"bank {b}x{d}x{k} T={temp}{' tie' if tie else ''}"
    scalar(loss.detach(), r64, r32, lc.row_chain(lc.cdiv(k, 256), b), f"{tag} loss", "ntxent_bank_kernel loss")
    f32c(qd.grad, r64["dq"], r32["dq"], f"{tag} dq", r64["dq_floor"], "ntxent_bank_kernel dq / dk")
    f32c(kd.grad, r64["dk"], r32["dk"], f"{tag} dk", r64["dk_floor"], "ntxent_bank_kernel dq / dk")


def test_bank_loss_beyond_the_lds_limit_is_rejected():
    from ssl_wafermap_amd.loss import _NTXentBank

    b, d, k = 3, 512, 15361
    assert 2 * d + k == lc.BANK_LDS_FLOATS + 1
    q = torch.zeros(b, d, device=DEV)
    with pytest.raises(HipError(), match="wm_ntxent_bank_fwd_bwd"):
        _NTXentBank.apply(q, q, torch.zeros(d, k, device=DEV), 0.1)


# ---------------------------------------------------------------------------------------------------- -cos
@pytest.mark.parametrize("b", [1, 37])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 2048])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_negative_cosine(b, d, dtype):
    """every row compared; rows with a clamped (zero) norm hold gradients of size 1 / eps and are compared apart from the live
    rows, so that their scale does not hide the others"""
    from ssl_wafermap_amd.loss import NegativeCosineSimilarity

    eps = 1e-8
    patterns = [(), ("x0",), ("x1",), ("both",)] + ([("x0", "x1", "both")] if b > 1 else [])
    for zero in patterns:
        for need in ((True, True), (True, False), (False, True)):
            x0, x1 = lc.neg_cosine_inputs(b, d, seed=b + d, zero=zero, bf16=dtype == BF16)
            r64, r32 = lc.neg_cosine(x0, x1, eps, dt=F64), lc.neg_cosine(x0, x1, eps, dt=F32)
            assert lc.neg_cosine_margin(r64, eps) > 0.9                      # no norm near the l > eps switch
            live = (r64["l0"] > eps) & (r64["l1"] > eps)
            a = x0.to(DEV).to(dtype).requires_grad_(need[0])
            c = x1.to(DEV).to(dtype).requires_grad_(need[1])
            loss = NegativeCosineSimilarity(eps=eps)(a, c)
            loss.backward()
            tag = f"-cos {b}x{d} {dtype} zero={zero} grads={need}"
            scalar(loss.detach(), r64, r32, lc.row_chain(lc.cdiv(d, 64), b), f"{tag} loss", "neg_cosine_kernel loss")
            for t, key, wanted in ((a, "d0", need[0]), (c, "d1", need[1])):
                if not wanted:
                    assert t.grad is None
                    continue
                for sel in (live, ~live):
                    if not bool(sel.any()):
                        continue
                    if dtype == BF16:      # the module hands the float32 gradient back in the input's dtype
                        bf16c(t.grad.cpu()[sel], r64[key][sel], kc.bf(r32[key][sel]), f"{tag} {key}", "neg_cosine_kernel<bf16> d0 / d1", r64["floor"](key, sel))
                    else:
                        f32c(t.grad.cpu()[sel], r64[key][sel], r32[key][sel], f"{tag} {key}", r64["floor"](key, sel), "neg_cosine_kernel<float> d0 / d1")


# ---------------------------------------------------------------------------------------------------- cross-entropy / BCE
@pytest.mark.parametrize("b,c", [(1, 1), (70, 9), (5, 64), (5, 65), (33, 1000)])
@pytest.mark.parametrize("family", ["randn", "offset+1e4", "dominant"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_cross_entropy(b, c, family, dtype):
    from ssl_wafermap_amd.loss import CrossEntropyLoss

    g = torch.Generator().manual_seed(b + c)
    x = lc.logit_inputs(family, b, c, seed=b * c, bf16=dtype == BF16)
    labels = torch.randint(0, c, (b,), generator=g)
    w = torch.rand(c, generator=g) + 0.2
    w[c // 2] = 0.0                                          # a class of weight zero
    if b > 4:
        labels[1], labels[b - 1] = -100, -100                # ignored rows
    for weight in (None, w):
        if c == 1 and weight is not None:
            continue                                         # (its only weight is the zero one: 0 / 0, as torch)
        r64, r32 = lc.cross_entropy(x, labels, weight, dt=F64), lc.cross_entropy(x, labels, weight, dt=F32)
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        loss = CrossEntropyLoss(weight=weight).to(DEV)(xd, labels.to(DEV))
        loss.backward()
        tag = f"CE {b}x{c} {family} {dtype} weight={weight is not None}"
        # acc[0] and acc[1] are each a sum of B atomics; their quotient adds one rounding (inside the bound's four per term)
        scalar(loss.detach(), r64, r32, lc.row_chain(0, b) + b, f"{tag} loss", "cross_entropy_kernel loss")
        if dtype == BF16:
            bf16c(xd.grad, r64["dlogits"], kc.bf(r32["dlogits"]), f"{tag} dlogits", "cross_entropy_kernel<bf16> dlogits", r64["floor"])
        else:
            f32c(xd.grad, r64["dlogits"], r32["dlogits"], f"{tag} dlogits", r64["floor"], "cross_entropy_kernel<float> dlogits")


@pytest.mark.parametrize("b,c", [(70, 8), (7, 5), (4100, 65)])
@pytest.mark.parametrize("family", ["randn", "saturated"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bce_with_logits(b, c, family, dtype):
    from ssl_wafermap_amd.loss import BCEWithLogitsLoss

    if b == 4100:
        assert lc.cdiv(b * c, 256) > lc.BCE_CAP and c & (c - 1) != 0      # beyond the grid cap, C no power of two
    g = torch.Generator().manual_seed(b + c)
    x = lc.logit_inputs(family, b, c, seed=b + c, bf16=dtype == BF16)
    target = torch.rand(b, c, generator=g)                                # soft targets
    pw = torch.rand(c, generator=g) * 3 + 0.5
    for pos_weight in (None, pw):
        r64, r32 = lc.bce_logits(x, target, pos_weight, dt=F64), lc.bce_logits(x, target, pos_weight, dt=F32)
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        loss = BCEWithLogitsLoss(pos_weight=pos_weight).to(DEV)(xd, target.to(DEV))
        loss.backward()
        tag = f"BCE {b}x{c} {family} {dtype} pos_weight={pos_weight is not None}"
        scalar(loss.detach(), r64, r32, lc.grid_chain(b * c, lc.BCE_CAP), f"{tag} loss", "bce_logits_kernel loss")
        if dtype == BF16:
            bf16c(xd.grad, r64["dlogits"], kc.bf(r32["dlogits"]), f"{tag} dlogits", "bce_logits_kernel<bf16> dlogits", r64["floor"])
        else:
            f32c(xd.grad, r64["dlogits"], r32["dlogits"], f"{tag} dlogits", r64["floor"], "bce_logits_kernel<float> dlogits")


# ---------------------------------------------------------------------------------------------------- DCL / DCLW
@pytest.mark.parametrize("b,d,temp,sigma,dup", [(2, 32, 0.1, 0.5, False), (3, 100, 0.07, 0.05, False), (96, 300, 0.1, 0.5, False),
                                                 (96, 32, 0.07, 0.05, True), (257, 32, 0.07, 0.5, False), (300, 100, 0.1, 0.05, False)])
@pytest.mark.parametrize("weighted", [False, True])
def test_dcl(b, d, temp, sigma, dup, weighted):
    from ssl_wafermap_amd.loss import _DCL

    z0, z1 = lc.dcl_inputs(b, d, seed=b + d, duplicates=dup)
    s_ = sigma if weighted else None
    r64, r32 = lc.dcl(z0, z1, temp, s_, dt=F64), lc.dcl(z0, z1, temp, s_, dt=F32)
    a, c = z0.to(DEV).requires_grad_(True), z1.to(DEV).requires_grad_(True)
    loss = _DCL.apply(a, c, temp, sigma, weighted)
    loss.backward()
    tag = f"DCL{'W' if weighted else ''} {b}x{d} T={temp} sigma={sigma}{' duplicates' if dup else ''}"
    scalar(loss.detach(), r64, r32, lc.row_chain(0, 2 * b), f"{tag} loss", "dcl_rows_kernel loss")
    f32c(a.grad, r64["dz0"], r32["dz0"], f"{tag} dz0", r64["dz0_floor"], "dcl_grad_kernel")
    f32c(c.grad, r64["dz1"], r32["dz1"], f"{tag} dz1", r64["dz1_floor"], "dcl_grad_kernel")


def test_dcl_beyond_the_lds_limit_is_rejected():
    from ssl_wafermap_amd.loss import _DCL

    b, d = 2, 16381
    assert d + 2 * b > lc.DCL_LDS_FLOATS
    z = torch.zeros(b, d, device=DEV)
    with pytest.raises(HipError(), match="wm_dcl_fwd_bwd"):
        _DCL.apply(z, z, 0.1, 0.5, False)


# ---------------------------------------------------------------------------------------------------- Barlow / VICReg pieces
@pytest.mark.parametrize("d", [1, 17, 256, 730])
@pytest.mark.parametrize("diag_weight", [1.0, 0.0])
def test_barlow_kernel(d, diag_weight):
    if d == 730:
        assert lc.cdiv(d * d, 256) > lc.BARLOW_CAP
    g = torch.Generator().manual_seed(d)
    n = 64
    raw = (torch.randn(d, d, generator=g) * 8 + torch.eye(d) * n).float()    # a float32 matrix: the reference sees the same operand
    scale, lam = (n - 1) / (n * n), 5e-3
    r64, r32 = lc.barlow(raw, scale, lam, diag_weight, dt=F64), lc.barlow(raw, scale, lam, diag_weight, dt=F32)
    rd = raw.to(DEV)
    loss = torch.zeros(1, dtype=F32, device=DEV)
    draw = torch.empty_like(rd)
    call("wm_barlow_twins_fwd_bwd", ptr(rd), d, scale, lam, diag_weight, ptr(loss), ptr(draw))
    tag = f"barlow D={d} diag_weight={diag_weight:g}"
    scalar(loss[0], r64, r32, lc.grid_chain(d * d, lc.BARLOW_CAP), f"{tag} loss", "barlow_kernel loss")
    f32c(draw, r64["draw"], r32["draw"], f"{tag} draw", r64["floor"], "barlow_kernel draw")


@pytest.mark.parametrize("rows,c", [(3, 5), (64, 256), (4200, 250)])
def test_center_columns(rows, c):
    if rows == 4200:
        assert lc.cdiv(rows * c, 256) > lc.CENTER_CAP and c & (c - 1) != 0
    g = torch.Generator().manual_seed(rows)
    z = kc.bf(torch.randn(rows, c, generator=g) + 3)
    mean = z.double().mean(0).float()
    ref, emul = lc.center_columns(z, mean, dt=F64), lc.center_columns(z, mean, dt=F32)
    zd, out = z.to(DEV).to(BF16), torch.empty(rows, c, dtype=BF16, device=DEV)
    call("wm_center_columns", ptr(zd), ptr(mean.to(DEV)), rows, c, ptr(out))
    bf16c(out, ref, emul, f"center_columns {rows}x{c}", "center_columns_kernel")


@pytest.mark.parametrize("n,d", [(2, 1), (64, 256), (64, 16400)])
def test_vicreg_variance(n, d):
    if d == 16400:
        assert lc.cdiv(d, 256) > lc.VICREG_CAP
    eps = 1e-4
    vb = lc.vicreg_inputs(n, d, seed=d)
    r64, r32 = lc.vicreg_variance(vb, n, eps, dt=F64), lc.vicreg_variance(vb, n, eps, dt=F32)
    assert lc.vicreg_margin(r64) > 0.01                                      # no sd near the hinge
    assert d == 1 or (bool((r64["sd"] < 1).any()) and bool((r64["sd"] > 1).any()))
    loss = torch.zeros(1, dtype=F32, device=DEV)
    coef = torch.empty(d, dtype=F32, device=DEV)
    call("wm_vicreg_variance", ptr(vb.to(DEV)), n, d, eps, ptr(loss), ptr(coef))
    scalar(loss[0], r64, r32, lc.grid_chain(d, lc.VICREG_CAP), f"vicreg_variance {n}x{d} loss", "vicreg_variance_kernel loss")
    f32c(coef, r64["coef"], r32["coef"], f"vicreg_variance {n}x{d} coef", lc.f32_floor(r64["coef"]), "vicreg_variance_kernel coef")


# ---------------------------------------------------------------------------------------------------- the two modules, end to end
E2E_SHAPES = [(64, 256), (96, 128)]


def loss_within(got, ref, what):
    from parity_log import parity

    parity(f"{what}: |loss - float64|", abs(float(got) - ref["loss"]), ref["loss_bound"],
           note="any pattern of bf16 roundings of the stored projections (first order) + float32 summation bounds")


@pytest.mark.parametrize("n,d", E2E_SHAPES)
def test_barlow_twins_loss_module(n, d):
    """BarlowTwinsLoss as it composes its kernels (standardise -> bf16 -> GEMM -> barlow kernel -> two GEMMs -> BatchNorm
    backward) against float64, the gradients bounded by the emulation that rounds to bf16 where the module stores bf16"""
    from ssl_wafermap_amd.loss import BarlowTwinsLoss

    a, b = lc.e2e_inputs(n, d, seed=n + d)
    ref, emul = lc.barlow_twins_e2e(a, b), lc.barlow_twins_e2e(a, b, emulate=True)
    ad, bd = a.to(DEV).to(BF16).requires_grad_(True), b.to(DEV).to(BF16).requires_grad_(True)
    loss = BarlowTwinsLoss().to(DEV)(ad, bd)
    loss.backward()
    loss_within(loss.detach(), ref, f"BarlowTwinsLoss {n}x{d}")
    bf16c(ad.grad, ref["dz_a"], emul["dz_a"], f"BarlowTwinsLoss {n}x{d} dz_a", "BarlowTwinsLoss")
    bf16c(bd.grad, ref["dz_b"], emul["dz_b"], f"BarlowTwinsLoss {n}x{d} dz_b", "BarlowTwinsLoss")


@pytest.mark.parametrize("n,d", E2E_SHAPES)
def test_vicreg_loss_module(n, d):
    """VICRegLoss (MSE + per branch: column statistics, bf16 centring, variance hinge, covariance GEMM and barlow kernel, the
    backward through draw and coef) against float64, in the same way"""
    from ssl_wafermap_amd.loss import VICRegLoss

    a, b = lc.e2e_inputs(n, d, seed=n + d, small_std=True)
    ref, emul = lc.vicreg_e2e(a, b), lc.vicreg_e2e(a, b, emulate=True)
    ad, bd = a.to(DEV).to(BF16).requires_grad_(True), b.to(DEV).to(BF16).requires_grad_(True)
    loss = VICRegLoss().to(DEV)(ad, bd)
    loss.backward()
    loss_within(loss.detach(), ref, f"VICRegLoss {n}x{d}")
    bf16c(ad.grad, ref["dz_a"], emul["dz_a"], f"VICRegLoss {n}x{d} dz_a", "VICRegLoss")
    bf16c(bd.grad, ref["dz_b"], emul["dz_b"], f"VICRegLoss {n}x{d} dz_b", "VICRegLoss")


# ---------------------------------------------------------------------------------------------------- Sinkhorn
@pytest.mark.parametrize("b,k", [(1, 1), (48, 255), (48, 257), (300, 3000)])
@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_sinkhorn(b, k, iters, dtype):
    from ssl_wafermap_amd.loss import sinkhorn

    if b == 300:
        assert lc.cdiv(b * k, 256) > lc.SK_WRITE_CAP
    for eps in (0.05, 0.02):
        x = lc.sinkhorn_inputs(b, k, seed=b + k, bf16=dtype == BF16)
        assert float(x.abs().max()) <= 1.0
        ref, emul = lc.sinkhorn(x, eps, iters, dt=F64), lc.sinkhorn(x, eps, iters, dt=F32)
        assert bool(torch.isfinite(emul).all())                               # the float32 restatement stays finite
        q = sinkhorn(x.to(DEV).to(dtype), iters, eps)
        tag = f"sinkhorn {b}x{k} iters={iters} eps={eps} {dtype}"
        f32c(q, ref, emul, f"{tag} Q", lc.f32_floor(ref), f"sinkhorn<{'bf16' if dtype == BF16 else 'float'}>")
        if iters > 0:   # rows of Q sum to 1: K float32 terms summed in double here, each within the bound above of a set that does
            rs = q.double().sum(1).cpu()
            f32c(rs, torch.ones(b, dtype=F64), emul.double().sum(1), f"{tag} row sums", lc.f32_floor(1.0), "sinkhorn row sums")


def test_sinkhorn_rejects_more_than_100_iterations():
    from ssl_wafermap_amd.loss import sinkhorn

    with pytest.raises(HipError(), match="wm_sinkhorn"):
        sinkhorn(torch.zeros(4, 8, device=DEV), 101, 0.05)
