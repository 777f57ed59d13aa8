"""The token plumbing of the ViT step (csrc/transformer.hip: tokens_assemble, patchify, row gather / scatter, the per-row
argsort), the column sums behind the dpos / dcls gradients and the small float32 matmul, through the C ABI, every output
between sentinel margins (tests/guarded.py).

Data movement is compared bit for bit with the permutations of tests/vit_cases.py, tokens_assemble with float32-add-then-bf16,
the matmul with loss_cases.fma_matmul_f32, the integer (`lattice`) column sums with the exact sums; the other column sums go
through loss_cases.check_f32 with one float32 rounding of the summed magnitudes as the floor.  No tolerance here is a literal.
A test that claims a launch path (the 8192-block cap of ew_blocks, a partial column slab, idle row lanes) asserts it through
the Python mirror of the launch arithmetic."""
import guarded as G
import kernel_check as kc
import loss_cases as lc
import pytest
import torch
import vit_cases as vc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int64
WM_EINVAL, WM_EUNSUPPORTED = -1, -2
ACT_NONE = 0


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
    return t.to(DEV).to(BF16).contiguous()


_INT = {BF16: torch.int16, F32: torch.int32, I64: I64}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype]))


def twice(fn, what):
    """run fn (which allocates its guarded outputs and returns them) two times: margins intact, the same bits"""
    first = [g.t.clone() for g in fn()]
    G.finish(what)
    second = [g.t.clone() for g in fn()]
    G.finish(what)
    assert all(same_bits(a, b) for a, b in zip(first, second)), f"{what}: two calls differ"
    return first


# ---------------------------------------------------------------------------------------------------- tokens_assemble
@pytest.mark.parametrize("n,np_,d", vc.TOKEN_SHAPES)
def test_tokens_assemble(n, np_, d):
    work = n * (np_ + 1) * (d // 8)
    assert vc.ew_sweeps(work) == (2 if (n, np_, d) == vc.TOKEN_SHAPES[-1] else 1)
    patches, cls, pos = vc.tokens_inputs(n, np_, d, seed=n + np_)
    want = vc.tokens_assemble(patches, cls, pos, n, np_, dt=F32).bfloat16()
    pd, cd, sd = dev_bf16(patches), cls.to(DEV), pos.to(DEV)

    def run():
        out = G.Guarded((n * (np_ + 1), d), BF16)
        call("wm_tokens_assemble", ptr(pd), ptr(cd), ptr(sd), n, np_, d, out.ptr)
        return [out]

    (got,) = twice(run, f"tokens_assemble {n, np_, d}")
    assert same_bits(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------- patchify
@pytest.mark.parametrize("n,s,p", vc.PATCHIFY_SHAPES)
def test_patchify(n, s, p):
    chunks = n * s * s * 3 // 8
    assert vc.ew_sweeps(chunks) == (2 if (n, s, p) == vc.PATCHIFY_SHAPES[-1] else 1)
    g = torch.Generator().manual_seed(s + p)
    img = torch.randint(-32768, 32767, (n, s, s, 3), generator=g, dtype=torch.int32).to(torch.int16)     # every bit pattern
    imd = img.to(DEV).view(BF16)
    gg = s // p

    def run():
        out = G.Guarded((n * gg * gg, p, p, 3), BF16)
        call("wm_patchify", ptr(imd), n, s, p, out.ptr)
        return [out]

    (got,) = twice(run, f"patchify {n, s, p}")
    assert torch.equal(got.view(torch.int16).cpu(), vc.patchify(img, p))


def test_patchify_rejections():
    z = torch.zeros(3 * 32 * 32, dtype=BF16, device=DEV)
    assert rc_of("wm_patchify", ptr(z), 1, 32, 12, ptr(z)) == WM_EINVAL        # S % p
    assert rc_of("wm_patchify", ptr(z), 1, 30, 5, ptr(z)) == WM_EINVAL         # a patch row of 15 elements: no 16-byte chunks


# ---------------------------------------------------------------------------------------------------- gather / scatter
@pytest.mark.parametrize("hostile", [False, True], ids=["distinct", "with_out_of_range"])
@pytest.mark.parametrize("b,s,k,c", vc.ROWS_SHAPES)
def test_gather_and_scatter_rows(b, s, k, c, hostile):
    work = b * k * (c // 8)
    assert vc.ew_sweeps(work) == (2 if (b, s, k, c) == vc.ROWS_SHAPES[-1] else 1)
    idx = vc.index_inputs(b, s, k, seed=b + s, hostile=hostile)
    if hostile:
        assert int(idx.min()) == -1 and (k == 1 or int(idx.max()) == s)
    g = torch.Generator().manual_seed(c)
    big = torch.randint(-32768, 32767, (b * s, c), generator=g, dtype=torch.int32).to(torch.int16)
    small = torch.randint(-32768, 32767, (b * k, c), generator=g, dtype=torch.int32).to(torch.int16)
    pattern = torch.tensor(0x1234, dtype=torch.int16)           # the prefill: a skipped row must keep it
    idd, bigd, smalld = idx.to(DEV), big.to(DEV).view(BF16), small.to(DEV).view(BF16)

    def gather():
        out = G.Guarded((b * k, c), BF16)
        out.t.view(torch.int16).fill_(pattern)
        call("wm_gather_rows", ptr(bigd), ptr(idd), b, s, k, c, out.ptr)
        return [out]

    def scatter():
        out = G.Guarded((b * s, c), BF16)
        out.t.view(torch.int16).fill_(pattern)
        call("wm_scatter_rows", ptr(smalld), ptr(idd), b, s, k, c, out.ptr)
        return [out]

    (got,) = twice(gather, f"gather_rows {b, s, k, c}")
    assert torch.equal(got.view(torch.int16).cpu(), vc.rows_by_index(big, idx, b, s, k, pattern.expand(b * k, c)))
    (got,) = twice(scatter, f"scatter_rows {b, s, k, c}")
    want = vc.rows_by_index(small, idx, b, s, k, pattern.expand(b * s, c), scatter=True)
    assert torch.equal(got.view(torch.int16).cpu(), want)
    valid = int(((idx >= 0) & (idx < s)).sum())
    assert int((want == pattern).all(1).sum()) >= b * s - valid       # the rows nothing was scattered to keep the prefill


# ---------------------------------------------------------------------------------------------------- argsort
@pytest.mark.parametrize("kind", vc.ARGSORT_KEYS)
@pytest.mark.parametrize("s", vc.ARGSORT_S)
def test_argsort_rows(s, kind):
    rows = 5
    keys = vc.argsort_inputs(kind, rows, s, seed=s)
    kd = keys.to(DEV)

    def run():
        out = G.Guarded((rows, s), I64)
        call("wm_argsort_rows", ptr(kd), rows, s, out.ptr)
        return [out]

    (got,) = twice(run, f"argsort_rows S={s} {kind}")
    assert torch.equal(got.cpu(), vc.argsort_rows(keys))


def test_argsort_rows_rejects_more_than_256_keys():
    kd = torch.zeros(2, vc.ARGSORT_MAX + 1, device=DEV)
    out = G.Guarded((2, vc.ARGSORT_MAX + 1), I64)
    assert rc_of("wm_argsort_rows", ptr(kd), 2, vc.ARGSORT_MAX + 1, out.ptr) == WM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out.t == out.fill).all())
    G.finish("argsort rejection")


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("family", vc.COLSUM_FAMILIES)
@pytest.mark.parametrize("rows,c", vc.COLSUM_SHAPES)
def test_colsum_forms(rows, c, family):
    """colsum_kernel<1> in its three forms: wm_colsum_bf16 overwriting and accumulating (float32 atomics: no determinism is
    asserted), and the slot form of wm_bias_act_bwd_parts(WM_ACT_NONE), whose `part` is compared block by block"""
    cb, slabs, rb, rpb = vc.colsum_geometry(rows, c)
    if (rows, c) == (65, 384):
        assert (cb, rb) == (48, 2) and vc.colsum_row_lanes(c) == (5, 16)
    if c == 520:
        assert slabs == 2 and (c // 8) % cb == 1
    if (rows, c) == (3, 37 * 384):
        assert slabs == 28 and rb == 1
    x, ref, emul = vc.colsum_case(family, rows, c)
    xd = dev_bf16(x)
    what = f"{family} {rows}x{c}"
    assert int(lib().wm_colsum_blocks(rows, c)) == rb

    def slots():
        part = G.Guarded((rb, c), F32)
        call("wm_bias_act_bwd_parts", 0, 0, ptr(xd), ACT_NONE, rows, c, 0, part.ptr)
        return [part]

    (part,) = twice(slots, f"colsum slots {what}")
    out = G.Guarded((c,), F32)
    call("wm_colsum_bf16", ptr(xd), rows, c, out.ptr, 0)
    G.finish(f"colsum_bf16 {what}")
    g = torch.Generator().manual_seed(rows)
    base = torch.randint(-5, 6, (c,), generator=g).float() if family == "lattice" else torch.randn(c, generator=g)
    acc = G.Guarded((c,), F32, init=base)
    call("wm_colsum_bf16", ptr(xd), rows, c, acc.ptr, 1)
    G.finish(f"colsum_bf16 accumulate {what}")
    acc_ref, acc_emul = base.double() + ref["out"], base + emul["out"]
    if family == "lattice":
        assert torch.equal(part.cpu().double(), ref["part"]) and torch.equal(out.t.cpu().double(), ref["out"])
        assert torch.equal(acc.t.cpu().double(), acc_ref)
        return
    lc.check_f32(part, ref["part"], emul["part"], f"[colsum_kernel<1> slots] {what}", ref["part_floor"])
    lc.check_f32(out.t, ref["out"], emul["out"], f"[colsum_kernel<1> atomics] {what}", ref["out_floor"])
    lc.check_f32(acc.t, acc_ref, acc_emul, f"[colsum_kernel<1> atomics] accumulate {what}",
                 kc.f32_sum_floor(torch.cat([x, base[None, :]])))


# ---------------------------------------------------------------------------------------------------- small matmul
@pytest.mark.parametrize("trans_a", [0, 1])
@pytest.mark.parametrize("m,k,n", vc.MATMUL_SHAPES)
def test_matmul_f32_is_one_fma_chain_in_k_order(m, k, n, trans_a):
    a, b = vc.matmul_inputs(m, k, n, seed=m + k + n)
    want = lc.fma_matmul_f32(a, b)
    ad, bd = (a.t().contiguous() if trans_a else a).to(DEV), b.to(DEV)

    def run():
        out = G.Guarded((m, n), F32)
        call("wm_matmul_f32", ptr(ad), ptr(bd), out.ptr, m, n, k, trans_a)
        return [out]

    (got,) = twice(run, f"matmul_f32 {m, k, n} trans_a={trans_a}")
    assert same_bits(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------- autograd nodes
def _bits_of(t):
    return t.detach().float().cpu()


def _token_reference(groups, cls, dy):
    """torch autograd in double of [cls + pos[0]; patches + pos[1:]] per image and group, upstream gradient dy"""
    cl = cls.double().requires_grad_(True)
    leaves, outs = [], []
    for patches, pos, n, np_ in groups:
        p, q = patches.double().requires_grad_(True), pos.double().requires_grad_(True)
        d = p.shape[1]
        tok = torch.cat([cl.reshape(1, 1, d).expand(n, 1, d), p.reshape(n, np_, d)], 1) + q.reshape(1, np_ + 1, d)
        outs.append(tok.reshape(-1, d))
        leaves.append((p, q))
    torch.cat(outs).backward(dy.double())
    return cl.grad, [(p.grad, q.grad) for p, q in leaves]


@pytest.mark.parametrize("multi", [False, True], ids=["_TokensAssemble", "_TokensAssembleMulti"])
def test_tokens_assemble_nodes_against_autograd(multi):
    from ssl_wafermap_amd import vit_ops

    d = 64
    geoms = [(3, 9), (5, 4)] if multi else [(3, 9)]
    g = torch.Generator().manual_seed(9)
    cls = torch.randn(1, 1, d, generator=g)
    groups = [(kc.bf(torch.randn(n * np_, d, generator=g)), torch.randn(1, np_ + 1, d, generator=g), n, np_) for n, np_ in geoms]
    rows = sum(n * (np_ + 1) for n, np_ in geoms)
    dy = kc.bf(torch.randn(rows, d, generator=g))
    dcls_ref, grads_ref = _token_reference(groups, cls, dy)
    cd = cls.to(DEV).requires_grad_(True)
    dev = [(dev_bf16(p).requires_grad_(True), q.to(DEV).requires_grad_(True), n, np_) for p, q, n, np_ in groups]
    out = vit_ops.tokens_assemble_multi(dev, cd) if multi else vit_ops.tokens_assemble(dev[0][0], cd, dev[0][1], *geoms[0])
    assert type(out.grad_fn).__name__ == ("_TokensAssembleMultiBackward" if multi else "_TokensAssembleBackward")
    want = torch.cat([vc.tokens_assemble(p, cls, q, n, np_, dt=F32) for p, q, n, np_ in groups])
    assert same_bits(out.detach().cpu(), want.bfloat16())
    out.backward(dev_bf16(dy))
    off, dcls_terms = 0, []
    for (p, q, n, np_), (pd, qd, _, _), (dp_ref, dq_ref) in zip(groups, dev, grads_ref):
        dyg = dy[off:off + n * (np_ + 1)].reshape(n, (np_ + 1) * d)
        off += n * (np_ + 1)
        assert torch.equal(_bits_of(pd.grad), dp_ref.float())               # the patch gradient is a row gather: exact
        lc.check_f32(qd.grad.reshape(-1), dq_ref.reshape(-1), kc.colsum_f32(dyg), f"[_TokensAssemble node] dpos N={n}", kc.f32_sum_floor(dyg))
        dcls_terms.append(dyg[:, :d])
    terms = torch.cat(dcls_terms)
    # dcls: every group's column sum, the groups then added in float32
    emul = sum(kc.colsum_f32(t) for t in dcls_terms)
    lc.check_f32(cd.grad.reshape(-1), dcls_ref.reshape(-1), emul, "[_TokensAssemble node] dcls", kc.f32_sum_floor(terms))


def test_gather_and_scatter_nodes_against_autograd():
    from ssl_wafermap_amd import vit_ops

    b, s, k, c = 4, 50, 12, 64
    idx = vc.index_inputs(b, s, k, seed=3)
    flat = (torch.arange(b)[:, None] * s + idx).reshape(-1)
    g = torch.Generator().manual_seed(4)
    x, src = kc.bf(torch.randn(b * s, c, generator=g)), kc.bf(torch.randn(b * k, c, generator=g))
    dy_g, dy_s = kc.bf(torch.randn(b * k, c, generator=g)), kc.bf(torch.randn(b * s, c, generator=g))
    # gather
    xr = x.double().requires_grad_(True)
    xr[flat].backward(dy_g.double())
    xd = dev_bf16(x).requires_grad_(True)
    out = vit_ops.gather_rows(xd, idx.to(DEV), b, s)
    assert type(out.grad_fn).__name__ == "_GatherRowsBackward" and torch.equal(_bits_of(out), x[flat])
    out.backward(dev_bf16(dy_g))
    assert torch.equal(_bits_of(xd.grad), xr.grad.float())
    # scatter
    br, sr = x.double().requires_grad_(True), src.double().requires_grad_(True)
    br.index_copy(0, flat, sr).backward(dy_s.double())
    bd, sd = dev_bf16(x).requires_grad_(True), dev_bf16(src).requires_grad_(True)
    out = vit_ops.scatter_rows(bd, sd, idx.to(DEV), b, s)
    assert type(out.grad_fn).__name__ == "_ScatterRowsBackward" and torch.equal(_bits_of(out), x.index_copy(0, flat, src))
    out.backward(dev_bf16(dy_s))
    assert torch.equal(_bits_of(bd.grad), br.grad.float()) and torch.equal(_bits_of(sd.grad), sr.grad.float())
