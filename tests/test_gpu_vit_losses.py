"""The loss kernels of the second half of csrc/transformer.hip (MSE / L1, the DINO teacher probabilities and loss, soft
cross-entropy, the mean-entropy regulariser) against float64, through the C ABI, every output between sentinel margins
(tests/guarded.py) that are asserted untouched after each call.

dpred of MSE / L1 is compared bit for bit with the float32 restatement of tests/vit_cases.py; float32 outputs go through
loss_cases.check_f32, bf16 outputs through loss_cases.check_bf16 against the emulation that rounds where the kernel packs, and
every scalar through loss_cases.check_scalar with the chain length of the kernel's own reduction.  No tolerance here is a
literal.  A test that claims a launch path asserts it through the Python mirror of the launch arithmetic.
tests/test_vit_cases_cpu.py proves on the CPU that these criteria reject every seeded error of vit_cases at these shapes and
accept the honest variants."""
import guarded as G
import kernel_check as kc
import loss_cases as lc
import pytest
import torch
import vit_cases as vc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
WM_EINVAL, WM_EUNSUPPORTED = -1, -2


def lib():
    from ssl_wafermap_amd import _lib

    return _lib.load()


def call(fn_name, *args):
    from ssl_wafermap_amd import _lib

    _lib.check(getattr(lib(), fn_name)(*args, _lib.stream_ptr()), fn_name)


def rc_of(fn_name, *args):
    from ssl_wafermap_amd import _lib

    return int(getattr(lib(), fn_name)(*args, _lib.stream_ptr()))


def ptr(t):
    return 0 if t is None else int(t.data_ptr())


def dev_bf16(t):
    """a bf16-exact float32 CPU tensor on the device as bf16"""
    return t.to(DEV).to(BF16).contiguous()


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


def zero_loss():
    """the loss buffer, zeroed before the call as the Python layer does"""
    return G.Guarded((1,), F32, init=torch.zeros(1))


# ---------------------------------------------------------------------------------------------------- MSE / L1
MSE_PATHS = {8: (1, 1, "one chunk"), 2040: (1, 1, "255 chunks: one ragged block"), vc.EW_CAP: (1024, 1, "the last one-sweep size"),
             vc.EW_CAP + 8: (1024, 2, "one chunk in the second sweep"), 3 * vc.EW_CAP + 8: (1024, 4, "three full sweeps and a chunk")}


@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
@pytest.mark.parametrize("family", vc.MSE_FAMILIES)
@pytest.mark.parametrize("n", vc.MSE_SHAPES)
def test_mse_l1(n, family, l1):
    assert (vc.mse_blocks(n), vc.mse_sweeps(n)) == MSE_PATHS[n][:2], MSE_PATHS[n][2]
    (pred, target), ref, emul = vc.mse_case(family, n, l1)
    fn = "wm_l1_fwd_bwd" if l1 else "wm_mse_fwd_bwd"
    what = f"{fn} {family} n={n}"
    pd, td = dev_bf16(pred), dev_bf16(target)
    got = []
    for _ in range(2):
        loss, dp = zero_loss(), G.Guarded(tuple(pred.shape), BF16)
        call(fn, ptr(pd), ptr(td), n, loss.ptr, dp.ptr)
        G.finish(what)
        got.append((dp.t.clone(), float(loss.t[0])))
    assert same_bits(got[0][0].cpu(), emul["dpred"].bfloat16()), f"{what}: dpred differs from the float32 restatement"
    assert same_bits(got[0][0], got[1][0]), f"{what}: dpred differs between two calls"
    lc.check_scalar(got[0][1], ref["terms"], emul["terms"], vc.mse_chain(n), f"[mse_kernel<{'L1' if l1 else 'MSE'}>] {what}")


def test_mse_rejections():
    z = torch.zeros(16, dtype=BF16, device=DEV)
    loss = torch.zeros(1, device=DEV)
    for fn in ("wm_mse_fwd_bwd", "wm_l1_fwd_bwd"):
        assert rc_of(fn, ptr(z), ptr(z), 12, ptr(loss), ptr(z)) == WM_EINVAL
        assert rc_of(fn, ptr(z), ptr(z), 0, ptr(loss), ptr(z)) == WM_EINVAL


# ---------------------------------------------------------------------------------------------------- DINO / soft CE
def run_teacher_probs(i, temp_t, what):
    rows, d = i["teacher"].shape
    pr, pe = (vc.dino_teacher_probs(i["teacher"], i["center"], temp_t, dt=dt) for dt in (F64, F32))
    td, cd = dev_bf16(i["teacher"]), i["center"].to(DEV)
    got = []
    for _ in range(2):
        out = G.Guarded((rows, d), F32)
        call("wm_dino_teacher_probs", ptr(td), ptr(cd), temp_t, rows, d, out.ptr)
        G.finish(what)
        got.append(out.t.clone())
    assert same_bits(got[0], got[1]), f"{what}: probs differ between two calls"
    lc.check_f32(got[0], pr, pe, f"[dino_teacher_probs] {what}", lc.f32_floor(pr))


def run_dino(family, vs, vt, b, d, temp_t, skip):
    i, ref, emul = vc.dino_case(family, vs, vt, b, d, temp_t, skip)
    kern = "dino_loss_kernel" if skip else "dino_loss_kernel (soft CE)"
    what = f"{family} Vs={vs} Vt={vt} B={b} D={d} Tt={temp_t}"
    sd, pd = dev_bf16(i["student"]), i["probs"].to(DEV).contiguous()
    got = []
    for _ in range(2):
        loss, ds = zero_loss(), G.Guarded((vs * b, d), BF16)
        if skip:
            call("wm_dino_loss_fwd_bwd", ptr(sd), ptr(pd), vs, vt, b, d, vc.STUDENT_TEMP, loss.ptr, ds.ptr)
        else:
            call("wm_soft_cross_entropy_fwd_bwd", ptr(sd), ptr(pd), vs, b, d, vc.STUDENT_TEMP, loss.ptr, ds.ptr)
        G.finish(what)
        got.append((ds.t.clone(), float(loss.t[0])))
    assert same_bits(got[0][0], got[1][0]), f"{what}: dstudent differs between two calls"
    lc.check_bf16(got[0][0], ref["dstudent"], emul["dstudent"], f"[{kern}] {what} dstudent", vc.softmax_floor(family, ref))
    lc.check_scalar(got[0][1], ref["terms"], emul["terms"], vc.dino_chain(vs, vt, b), f"[{kern}] {what} loss", ref["mags"])
    return i


ROW_PATHS = {8: 1, 2040: 1, 2048: 1, 2056: 2, 8192: 4}      # register passes: a row is D / 8 chunks over 256 threads


@pytest.mark.parametrize("d", vc.ROW_D)
@pytest.mark.parametrize("vs,vt,b", vc.DINO_VIEWS)
def test_dino_loss_shapes(vs, vt, b, d):
    """every edge of the register tiling (255, 256, 257 chunks; all DL_MAXV passes) at every view geometry: Vs = Vt, Vs > Vt,
    Vs < Vt (one student view that meets one teacher only), more teachers than students"""
    assert vc.row_passes(d) == ROW_PATHS[d] and d <= vc.DL_MAX_D
    i = run_dino("randn", vs, vt, b, d, 0.04, 1)
    run_teacher_probs(i, 0.04, f"randn rows={vt * b} D={d} Tt=0.04")


@pytest.mark.parametrize("family", vc.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("temp_t", vc.TEACHER_TEMPS)
@pytest.mark.parametrize("d,views", vc.DINO_FAMILY_SHAPES)
def test_dino_loss_families(family, temp_t, d, views):
    vs, vt, b = views
    i = run_dino(family, vs, vt, b, d, temp_t, 1)
    run_teacher_probs(i, temp_t, f"{family} rows={vt * b} D={d} Tt={temp_t}")


@pytest.mark.parametrize("views,b", vc.SOFT_CE_VIEWS)
@pytest.mark.parametrize("d", vc.ROW_D)
def test_soft_cross_entropy(views, b, d):
    assert vc.row_passes(d) == ROW_PATHS[d]
    run_dino("randn", views, 1, b, d, 0.07, 0)


@pytest.mark.parametrize("family", ["offset", "onehot", "constant", "matched"])
def test_soft_cross_entropy_families(family):
    run_dino(family, 3, 1, 7, 2056, 0.07, 0)


def test_row_softmax_rejections():
    """D = 8200 (a fifth register pass) is unsupported, D = 12 (no whole chunks) and a loss without terms are invalid; nothing
    is launched (the outputs keep their sentinels)"""
    for d, want in ((8200, WM_EUNSUPPORTED), (12, WM_EINVAL)):
        s, p, c = torch.zeros(2, d, dtype=BF16, device=DEV), torch.zeros(2, d, device=DEV), torch.zeros(d, device=DEV)
        loss, ds, pr, dl, ws = zero_loss(), G.Guarded((2, d), BF16), G.Guarded((2, d), F32), G.Guarded((2, d), F32), G.Guarded((d,), F32)
        assert rc_of("wm_dino_loss_fwd_bwd", ptr(s), ptr(p), 2, 1, 1, d, 0.1, loss.ptr, ds.ptr) == want
        assert rc_of("wm_soft_cross_entropy_fwd_bwd", ptr(s), ptr(p), 2, 1, d, 0.1, loss.ptr, ds.ptr) == want
        assert rc_of("wm_dino_teacher_probs", ptr(s), ptr(c), 0.04, 2, d, pr.ptr) == want
        assert rc_of("wm_mean_entropy_reg_fwd_bwd", ptr(s), 0, 2, d, 0.1, loss.ptr, dl.ptr, ws.ptr) == want
        torch.cuda.synchronize()
        for g in (ds, pr, dl, ws):
            assert bool((g.t == g.fill).all())
        assert float(loss.t[0]) == 0.0
        G.finish(f"rejections D={d}")
    s, p = torch.zeros(3, 8, dtype=BF16, device=DEV), torch.zeros(3, 8, device=DEV)
    loss, ds = zero_loss(), G.Guarded((3, 8), BF16)
    assert rc_of("wm_dino_loss_fwd_bwd", ptr(s), ptr(p), 1, 1, 3, 8, 0.1, loss.ptr, ds.ptr) == WM_EINVAL      # (1, 1, B): no terms
    G.finish("no terms")


# ---------------------------------------------------------------------------------------------------- me-max
@pytest.mark.parametrize("prior", [False, True], ids=["memax", "prior"])
@pytest.mark.parametrize("family", vc.MEMAX_FAMILIES)
@pytest.mark.parametrize("k", vc.MEMAX_K)
@pytest.mark.parametrize("n", vc.MEMAX_N)
def test_mean_entropy_reg(n, k, family, prior):
    (x, lp), ref, emul = vc.memax_case(family, n, k, prior)
    assert vc.row_passes(k) == {8: 1, 1024: 1, 2056: 2}[k]
    if family == "underflow":
        assert float(emul["m"][k // 2]) == 0.0                       # the clamp at 1e-30 decides log m there
    what = f"{family} N={n} K={k} prior={int(prior)}"
    xd, lpd = dev_bf16(x), (None if lp is None else lp.to(DEV))
    got = []
    for _ in range(2):
        loss, dl, ws = zero_loss(), G.Guarded((n, k), F32), G.Guarded((k,), F32)
        call("wm_mean_entropy_reg_fwd_bwd", ptr(xd), ptr(lpd), n, k, vc.MEMAX_TEMP, loss.ptr, dl.ptr, ws.ptr)
        G.finish(what)
        got.append((dl.t.clone(), ws.t.clone(), float(loss.t[0])))
    if n == 1:          # (one row: one atomicAdd per element of m, no order to differ in)
        assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
    lc.check_f32(got[0][1], ref["m"], emul["m"], f"[memax_mean_kernel] {what} m", ref["m_floor"])
    lc.check_f32(got[0][0], ref["dlogits"], emul["dlogits"], f"[memax_grad_kernel] {what} dlogits", ref["floor"])
    lc.check_scalar(got[0][2], ref["terms"], emul["terms"], vc.memax_chain(k), f"[memax_grad_kernel] {what} scalar", ref["mags"])


# ---------------------------------------------------------------------------------------------------- autograd nodes
UP = 3.0        # the upstream gradient of the scalar losses


def _scaled(d_emul):
    """what a node hands back: the stored gradient times the upstream gradient in float32, rounded to bf16"""
    return kc.bf(d_emul.float() * UP)


@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
def test_mse_node_against_autograd(l1):
    from ssl_wafermap_amd import vit_ops

    pred, target = vc.mse_inputs("randn", 2040, seed=5)
    pr = pred.double().requires_grad_(True)
    ((torch.nn.functional.l1_loss if l1 else torch.nn.functional.mse_loss)(pr, target.double()) * UP).backward()
    emul = vc.mse(pred, target, l1, dt=F32)
    ref = vc.mse(pred, target, l1, dt=F64)
    pd = dev_bf16(pred).requires_grad_(True)
    loss = (vit_ops.l1_loss if l1 else vit_ops.mse_loss)(pd, dev_bf16(target))
    assert type(loss.grad_fn).__name__ == "_MSEBackward"
    (loss * UP).backward()
    lc.check_bf16(pd.grad, pr.grad, _scaled(emul["dpred"]), f"[_MSE node] {'l1' if l1 else 'mse'} dpred")
    lc.check_scalar(loss.detach(), ref["terms"], emul["terms"], vc.mse_chain(2040), f"[_MSE node] {'l1' if l1 else 'mse'} loss")


def _autograd_softmax_loss(student, probs, vs, vt, b, skip):
    x = student.double().reshape(vs, b, -1).requires_grad_(True)
    p = probs.double().reshape(vt, b, -1)
    ls = torch.log_softmax(x / float(torch.tensor(vc.STUDENT_TEMP, dtype=F32)), -1)
    pairs = [(s, t) for s in range(vs) for t in range(vt) if not (skip and s == t)]
    loss = sum(-(p[t] * ls[s]).sum(-1).mean() for s, t in pairs) / len(pairs)
    (loss * UP).backward()
    return x.grad.reshape(vs * b, -1)


@pytest.mark.parametrize("skip", [1, 0], ids=["dino", "soft_ce"])
def test_dino_and_soft_ce_nodes_against_autograd(skip):
    from ssl_wafermap_amd import vit_ops

    vs, vt, b, d = (3, 2, 5, 264) if skip else (3, 1, 5, 264)
    i, ref, emul = vc.dino_case("randn", vs, vt, b, d, 0.04, skip)
    want = _autograd_softmax_loss(i["student"], i["probs"], vs, vt, b, skip)
    sd = dev_bf16(i["student"]).requires_grad_(True)
    pd = i["probs"].to(DEV)
    loss = vit_ops.dino_loss(sd, pd, vs, vt, b, vc.STUDENT_TEMP) if skip else vit_ops.soft_cross_entropy(sd, pd, vs, b, vc.STUDENT_TEMP)
    node = "_DinoLoss" if skip else "_SoftCE"
    assert type(loss.grad_fn).__name__ == node + "Backward"
    (loss * UP).backward()
    lc.check_bf16(sd.grad, want, _scaled(emul["dstudent"]), f"[{node} node] dstudent")
    lc.check_scalar(loss.detach(), ref["terms"], emul["terms"], vc.dino_chain(vs, vt, b), f"[{node} node] loss", ref["mags"])


def test_mean_entropy_reg_node_against_autograd():
    from ssl_wafermap_amd import vit_ops

    n, k = 7, 1024
    (x, lp), ref, emul = vc.memax_case("randn", n, k, True)
    xr = x.double().requires_grad_(True)
    m = torch.softmax(xr / float(torch.tensor(vc.MEMAX_TEMP, dtype=F32)), 1).mean(0)
    ((m * (m.log() - lp.double())).sum() * UP).backward()
    xd = dev_bf16(x).requires_grad_(True)
    loss = vit_ops.mean_entropy_reg(xd, vc.MEMAX_TEMP, lp.to(DEV))
    assert type(loss.grad_fn).__name__ == "_MeanEntropyRegBackward"
    (loss * UP).backward()
    # the float32 gradient is rounded to bf16 once: its terms cancel, so the float32 floor of the kernel's output carries over
    lc.check_bf16(xd.grad, xr.grad, _scaled(emul["dlogits"]), "[_MeanEntropyReg node] dlogits", UP * ref["floor"])
    lc.check_scalar(loss.detach(), ref["terms"], emul["terms"], vc.memax_chain(k), "[_MeanEntropyReg node] loss", ref["mags"])
