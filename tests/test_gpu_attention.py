"""wm_attention_fwd / wm_attention_bwd (csrc/attention.hip) against float64 on the same bf16 inputs, judged by
tests/kernel_check.py: four criteria per tensor, each bounded by twice what a CPU emulation with the kernel's documented
bf16 roundings scores itself.  Covers both sides of every key-length dispatch edge for both head dims, the one-block
long-sequence forward (B * H > 512), the one-block backward behind WM_ATTN_BWD_ROLES=0, non-default scales, input
families that break a softmax without max subtraction or with unmasked padding, the float32 `lse` output, isolation
from neighbouring rows of the buffer, and several segments in one call."""
import kernel_check as kc
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# lse is a float32 output, so the device's float32 transcendentals are not "orders below" its rounding as they are for a
# bf16 output.  The yardstick (torch's float32 logsumexp on the CPU) is within one float32 ulp of the exact value; the
# kernel's m + logf(sum expf(s - m)) chains expf and logf, each specified to 1 ulp on the device, and a lane-order sum.
# Measured at factor 2: 90 of 91 cases pass, scale = 0.03 at S = 37 (near-uniform rows, lse ~ log 37) scores 1.6e-7
# relative against a bound of 1.5e-7 (2.1 ulp of the result against the yardstick's 1.0).  Twice the usual factor for
# this one tensor; every consumer of lse rounds exp(s - lse) to bf16 (2^-9).
LSE_FACTOR = 4.0


def _run(qkv, dout, scale=None, segments=None, qkv_dev=None, dout_dev=None):
    """(out, lse, dqkv) of the kernels as CPU tensors shaped like the references'.  lse comes from a direct call of
    wm_attention_fwd (vit_ops keeps it inside the autograd node); its `out` must be the autograd path's to the bit."""
    from ssl_wafermap_amd import _lib, vit_ops

    b, s, _, h, hd = qkv.shape
    sc = hd ** -0.5 if scale is None else scale
    qd = (qkv_dev if qkv_dev is not None else qkv.to(DEV).bfloat16().reshape(b * s, 3 * h * hd)).requires_grad_(True)
    dd = dout_dev if dout_dev is not None else dout.to(DEV).bfloat16().reshape(b * s, h * hd)
    if segments is None:
        out = vit_ops.attention(qd, b, s, h, scale=scale, head_dim=hd)
    else:
        out = vit_ops.attention_segments(qd, segments, h, scale=scale, head_dim=hd)
    out.backward(dd)
    lse = None
    if segments is None:
        o2 = torch.empty_like(out)
        lse = torch.empty((b, h, s), dtype=torch.float32, device=DEV)
        _lib.check(_lib.load().wm_attention_fwd(_lib.ptr(qd.detach()), b, s, h, hd, sc, _lib.ptr(o2), _lib.ptr(lse),
                                                _lib.stream_ptr()), "wm_attention_fwd")
        assert torch.equal(o2, out.detach())
        lse = lse.cpu()
    torch.cuda.synchronize()
    return out.detach().float().cpu().reshape(b, s, h, hd), lse, qd.grad.float().cpu().reshape(b, s, 3, h, hd)


def _compare(qkv, dout, scale=None, what="", images=None):
    b, s, _, h, hd = qkv.shape
    sc = hd ** -0.5 if scale is None else scale
    out, lse, dqkv = _run(qkv, dout, scale)
    ref = kc.attention_ref(qkv, sc, dout, chunk=16)
    emul = kc.attention_ref(qkv, sc, dout, emulate=True, chunk=16)
    sel = slice(None) if images is None else images
    worst = kc.check(out[sel], ref[0][sel], emul[0][sel], f"attention {what} out")
    worst = max(worst, kc.check(lse[sel], ref[1][sel], kc.attention_lse_f32(qkv, sc)[sel], f"attention {what} lse",
                                factor=LSE_FACTOR))
    # q / k / v gradients one by one: they differ in scale by orders of magnitude in the peaked / offset families
    if s == 1:
        # one key: p = 1, so dv = dO and, in exact arithmetic, dq = dk = 0.  The kernel forms dS = (dP - delta) scale from
        # two float32 evaluations of the same hd-term dot product dO . v (an MFMA and an fma chain): they differ by at most
        # hd 2^-24 sum |dO_d v_d| (the textbook bound of a float32 dot product), and that residue times k (or q) is all
        # dq (dk) may hold.  A float64 emulation has no such residue, so the bound is written out instead.
        kc.check(dqkv[sel, :, 2], ref[2][sel, :, 2], emul[2][sel, :, 2], f"attention {what} dv")
        q, k, v = (qkv[:, :, j].double() for j in range(3))
        res = hd * 2.0 ** -24 * (dout.double().abs() * v.abs()).sum(-1, keepdim=True) * sc * (1 + kc.BF16_ULP)
        assert (dqkv[:, :, 0].double().abs() <= res * k.abs()).all() and (dqkv[:, :, 1].double().abs() <= res * q.abs()).all()
        return out, lse, dqkv
    for j, name in enumerate(("dq", "dk", "dv")):
        worst = max(worst, kc.check(dqkv[sel, :, j], ref[2][sel, :, j], emul[2][sel, :, j], f"attention {what} {name}"))
    return out, lse, dqkv


LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197, 223, 224, 225, 255, 256]


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("s", LENGTHS)
def test_every_dispatch_edge(s, hd):
    """Both sides of the key-length edges 32 / 64 / 128 / 224 / 256 (and the 16-row strip edges), forward and backward."""
    b, h = 2, 3
    qkv, dout = kc.attention_inputs("randn", b, s, h, hd, seed=s * 2 + hd)
    _compare(qkv, dout, what=f"S={s} hd={hd}")


@pytest.mark.parametrize("s,hd", [(197, 64), (256, 32)])
def test_one_block_forward_for_many_heads(s, hd):
    """B * H = 522 > 512: the forward runs ONE block per (image, head) at > 8 key tiles (what a batch of 128 ViT-S images
    takes); every (image, head) is compared."""
    b, h = 87, 6
    qkv, dout = kc.attention_inputs("randn", b, s, h, hd, seed=s)
    _compare(qkv, dout, what=f"B*H=522 S={s} hd={hd}")


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("s", [129, 197, 223, 224, 225, 255, 256])
def test_one_block_backward_behind_the_switch(s, hd, monkeypatch):
    """WM_ATTN_BWD_ROLES=0 (read per call): attn_bwd<14> / attn_bwd<16> instead of the role-split kernel."""
    monkeypatch.setenv("WM_ATTN_BWD_ROLES", "0")
    qkv, dout = kc.attention_inputs("randn", 2, s, 3, hd, seed=s * 2 + hd + 1)
    _compare(qkv, dout, what=f"roles=0 S={s} hd={hd}")


@pytest.mark.parametrize("scale", [1.0, 0.03])
@pytest.mark.parametrize("s,hd", [(37, 64), (197, 64), (250, 32)])
def test_scale_argument(s, hd, scale):
    qkv, dout = kc.attention_inputs("randn", 2, s, 3, hd, seed=s, scale=scale)
    if scale == 1.0:
        qkv[:, :, :2] = kc.bf(qkv[:, :, :2] * 0.5)   # logits of spread ~2-4 rather than 8: still a softmax, not an argmax
    _compare(qkv, dout, scale=scale, what=f"scale={scale:g} S={s} hd={hd}")


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("s,hd", [(37, 64), (197, 64), (250, 64), (250, 32)])
def test_input_families(family, s, hd):
    qkv, dout = kc.attention_inputs(family, 2, s, 3, hd, seed=s + hd)
    _compare(qkv, dout, what=f"{family} S={s} hd={hd}")


@pytest.mark.parametrize("s,hd", [(37, 64), (197, 64), (250, 32)])
def test_next_image_1e4_times_larger_does_not_leak(s, hd):
    """The rows after the last token of image b are real rows of image b + 1 (the padded slots of the key tile): image 1
    holds values 1e4 times image 0's; image 0 must stay within bound, image 1 finite."""
    qkv, dout = kc.attention_inputs("randn", 2, s, 3, hd, seed=s)
    qkv[1] = kc.bf(qkv[1] * 1e4)
    dout[1] = kc.bf(dout[1] * 1e4)
    out, lse, dqkv = _compare(qkv, dout, what=f"1e4 neighbour S={s} hd={hd}", images=slice(0, 1))
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()


@pytest.mark.parametrize("s,hd", [(37, 64), (197, 64), (250, 32), (256, 64)])
def test_nan_rows_after_the_buffer_slice_are_not_read(s, hd):
    """qkv and dout are slices of larger allocations whose following rows hold NaN (all accesses stay inside allocated
    memory): outputs and gradients of the in-range rows stay finite and within bound."""
    b, h = 2, 3
    qkv, dout = kc.attention_inputs("randn", b, s, h, hd, seed=s + 7)
    big_q = torch.full((b * s + 64, 3 * h * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    big_d = torch.full((b * s + 64, h * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    big_q[:b * s] = qkv.to(DEV).bfloat16().reshape(b * s, -1)
    big_d[:b * s] = dout.to(DEV).bfloat16().reshape(b * s, -1)
    out, lse, dqkv = _run(qkv, dout, qkv_dev=big_q[:b * s].detach(), dout_dev=big_d[:b * s])
    sc = hd ** -0.5
    ref = kc.attention_ref(qkv, sc, dout)
    emul = kc.attention_ref(qkv, sc, dout, emulate=True)
    kc.check(out, ref[0], emul[0], f"attention NaN neighbour S={s} out")
    kc.check(lse, ref[1], kc.attention_lse_f32(qkv, sc), f"attention NaN neighbour S={s} lse", factor=LSE_FACTOR)
    kc.check(dqkv, ref[2], emul[2], f"attention NaN neighbour S={s} dqkv")


@pytest.mark.parametrize("segments,hd", [([(2, 197), (5, 37)], 64), ([(3, 37), (1, 250), (4, 16)], 32),
                                         ([(2, 129), (3, 64), (2, 33)], 64)])
def test_segments_against_per_segment_float64(segments, hd):
    from ssl_wafermap_amd import vit_ops

    h = 3
    parts = [kc.attention_inputs("randn", b, s, h, hd, seed=b * 1000 + s) for b, s in segments]
    qd = torch.cat([q.reshape(-1, 3 * h * hd) for q, _ in parts]).to(DEV).bfloat16().requires_grad_(True)
    dd = torch.cat([d.reshape(-1, h * hd) for _, d in parts]).to(DEV).bfloat16()
    out = vit_ops.attention_segments(qd, segments, h, head_dim=hd)
    out.backward(dd)
    out, dqkv, off = out.detach().float().cpu(), qd.grad.float().cpu(), 0
    for (b, s), (qkv, dout) in zip(segments, parts):
        ref = kc.attention_ref(qkv, hd ** -0.5, dout)
        emul = kc.attention_ref(qkv, hd ** -0.5, dout, emulate=True)
        kc.check(out[off:off + b * s].reshape(b, s, h, hd), ref[0], emul[0], f"segments {segments} ({b}, {s}) out")
        kc.check(dqkv[off:off + b * s].reshape(b, s, 3, h, hd), ref[2], emul[2], f"segments {segments} ({b}, {s}) dqkv")
        off += b * s


def test_rejects_bad_shapes():
    from ssl_wafermap_amd import _lib, vit_ops

    x = torch.zeros(2 * 300, 3 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.WaferHipError):
        vit_ops.attention(x, 2, 300, 1)  # S > 256
    with pytest.raises(ValueError):
        vit_ops.attention(x, 2, 100, 1)
    with pytest.raises(_lib.WaferHipError):
        vit_ops.attention(torch.zeros(2 * 100, 3 * 48, dtype=torch.bfloat16, device=DEV), 2, 100, 1, head_dim=48)
