"""The two stem passes that own a PAIR of vertically adjacent windows / quads per thread and walk XCD-contiguous block
ranges: bn_relu_maxpool_fwd (csrc/pool.hip) and bn_pool_bwd_apply (csrc/bn.hip), through their C entry points.

Forward: all three outputs exactly equal a window scan written here (first maximum in (kh, kw) order over the library's own
unfused bf16(relu(bn(y))); the selected raw inputs gathered at the scan's positions).  Backward: dy, dgamma, dbeta bit-equal
to arrays recorded from the one-quad-per-thread kernel (tests/golden/stem_pool, written by tools/probes/stem_pool_golden.py
on the parent revision), and a float64 reference on a shape of several blocks.  The shapes are the smallest at which the
mapping can go wrong: a single clipped window, odd P, odd H and W, a channel-chunk count that is no power of two, and a
block count that is neither one nor a multiple of eight with a ragged last block."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from kernel_check import pooled_side, scan_reference

GOLDEN = Path(__file__).resolve().parent / "golden" / "stem_pool"

DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 4096   # never dereferenced: the calls that take it fail validation first
THREADS = 256

# (N, C, H, W, G)
FWD_SHAPES = [(2, 8, 2, 2, 1), (4, 64, 18, 22, 2), (4, 64, 17, 21, 2), (3, 24, 6, 10, 1), (6, 64, 36, 36, 2)]
MULTI_BLOCK = (6, 64, 36, 36, 2)
GOLDEN_SHAPES = [(2, 16, 12, 12, 1), (4, 64, 20, 24, 2)]


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def fwd_blocks(n, c, h, w):
    """(items, blocks) of the forward launch: one item per pair of pooled rows x pooled column x 8 channels."""
    items = n * ((pooled_side(h) + 1) // 2) * pooled_side(w) * (c // 8)
    return items, -(-items // THREADS)


def bwd_blocks(n, c, h, w):
    """(items, blocks) of the backward launch: one item per pair of 2 x 2 quad rows x quad column x 8 channels."""
    items = n * ((h // 2 + 1) // 2) * (w // 2) * (c // 8)
    return items, -(-items // THREADS)


def test_multi_block_shape_runs_the_remainder_paths():
    """The launch arithmetic of MULTI_BLOCK: more than eight blocks, a count that is no multiple of eight (the remainder
    path of the XCD remap) and a last block that is not full."""
    n, c, h, w, _ = MULTI_BLOCK
    for items, blocks in (fwd_blocks(n, c, h, w), bwd_blocks(n, c, h, w)):
        assert (items, blocks) == (7776, 31)
        assert blocks > 8 and blocks % 8 != 0 and items % THREADS != 0


def stem_inputs(n, c, h, w, seed):
    """y [N][H][W][C] bf16 on both sides of the ReLU threshold, with constant patches (every window inside ties), gamma with
    negative channels (there the low patch is the one that survives the ReLU), beta."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(n, h, w, c, generator=gen) * 2 + 0.3
    y[0, : max((h + 1) // 2, 2), : max((w + 1) // 2, 2)] = -6.0   # gamma > 0: every transformed value of these windows is 0
    y[-1, h // 2:, :] = 5.0                          # gamma < 0: likewise here; gamma > 0: a positive constant
    gamma = torch.rand(c, generator=gen) + 0.5
    gamma[::3] *= -1
    beta = torch.randn(c, generator=gen) * 0.2
    return y.bfloat16().to(DEV), gamma.to(DEV), beta.to(DEV)


def train_stats(lib, y, gamma, beta, g):
    """wm_bn_train_stats -> (mean, invstd, scale, shift) [G][C], as the fused stem's forward calls it."""
    from ssl_wafermap_amd import _lib

    n, h, w, c = y.shape
    rows = n * h * w
    ws = torch.empty(lib.wm_bn_workspace_bytes(rows, c, g), dtype=torch.uint8, device=DEV)
    mean, invstd, scale, shift = (torch.empty((g, c), dtype=torch.float32, device=DEV) for _ in range(4))
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    _lib.check(lib.wm_bn_train_stats(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0, rows, c, g,
                                     1e-5, 0.1, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), 0, 0,
                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wm_bn_train_stats")
    return mean, invstd, scale, shift


def fused_forward(lib, y, scale, shift, g, want_xsel=True):
    from ssl_wafermap_amd import _lib

    n, h, w, c = y.shape
    p, q = pooled_side(h), pooled_side(w)
    out = torch.zeros((n, p, q, c), dtype=torch.bfloat16, device=DEV)
    idx = torch.full((n, p, q, c), 255, dtype=torch.uint8, device=DEV)
    xsel = torch.zeros_like(out) if want_xsel else None
    _lib.check(lib.wm_bn_relu_maxpool3x3s2_fwd(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), n, h, w, c, g, out.data_ptr(),
                                               idx.data_ptr(), _lib.ptr(xsel), _lib.stream_ptr()), "wm_bn_relu_maxpool3x3s2_fwd")
    torch.cuda.synchronize()
    return out, idx, xsel


@pytest.fixture(scope="module")
def forward_cases(lib):
    """Per shape, computed once: inputs, the unfused bf16(relu(bn(y))), the scan reference over it, the fused outputs."""
    from ssl_wafermap_amd import ops

    cases = {}
    for i, (n, c, h, w, g) in enumerate(FWD_SHAPES):
        y, gamma, beta = stem_inputs(n, c, h, w, seed=10 + i)
        y_nchw = y.permute(0, 3, 1, 2)                       # the library's NHWC tensors are channels_last [N, C, H, W]
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        t = ops.batch_norm(y_nchw, gamma, beta, rm, rv, True, relu=True, groups=g)
        _, _, scale, shift = train_stats(lib, y, gamma, beta, g)
        out, idx, xsel = fused_forward(lib, y, scale, shift, g)
        t_nhwc = t.permute(0, 2, 3, 1).float().cpu()
        cases[(n, c, h, w, g)] = dict(y=y, t=t, t_nhwc=t_nhwc, ref=scan_reference(t_nhwc, y.float().cpu()), out=out, idx=idx,
                                      xsel=xsel, scale=scale, shift=shift)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_equals_the_window_scan(forward_cases, shape):
    from ssl_wafermap_amd import ops

    k = forward_cases[shape]
    best, code, sel = k["ref"]
    # the data does force the tie rule: windows whose candidates all tie at 0, and ones that tie at a positive constant
    t = k["t_nhwc"]
    assert (best == 0).any() and (t > 0).any() and (t == 0).any()
    out, idx, xsel = k["out"].float().cpu(), k["idx"].cpu(), k["xsel"].float().cpu()
    assert torch.equal(out, best), f"out: {(out != best).sum().item()} of {out.numel()} differ"
    assert torch.equal(idx, code), f"idx: {(idx != code).sum().item()} of {idx.numel()} differ"
    assert torch.equal(xsel, sel), f"xsel: {(xsel != sel).sum().item()} of {xsel.numel()} differ"
    pooled = ops.max_pool3x3s2(k["t"])                                   # [N, C, P, Q]
    assert torch.equal(k["out"].permute(0, 3, 1, 2), pooled)


@pytest.mark.gpu
def test_forward_without_the_selected_inputs(lib, forward_cases):
    """xsel = NULL (no gradient wanted) is a separate instantiation of the kernel: same out and idx."""
    shape = (4, 64, 17, 21, 2)
    k = forward_cases[shape]
    out, idx, _ = fused_forward(lib, k["y"], k["scale"], k["shift"], shape[4], want_xsel=False)
    assert torch.equal(out, k["out"]) and torch.equal(idx, k["idx"])


def fused_backward(lib, y, ysel, pdy, idx, gamma, beta, mean, invstd, g):
    from ssl_wafermap_amd import _lib

    n, h, w, c = y.shape
    ws = torch.empty(lib.wm_bn_workspace_bytes(n * h * w, c, g), dtype=torch.uint8, device=DEV)
    dy = torch.zeros_like(y)
    dgamma, dbeta = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.wm_bn_relu_maxpool_bwd(y.data_ptr(), ysel.data_ptr(), pdy.data_ptr(), idx.data_ptr(), n, h, w, c, gamma.data_ptr(),
                                          beta.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g, dgamma.data_ptr(), dbeta.data_ptr(),
                                          0, dy.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wm_bn_relu_maxpool_bwd")
    torch.cuda.synchronize()
    return dy, dgamma, dbeta


def from_bits(a):
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GOLDEN_SHAPES)
def test_backward_is_bit_equal_to_the_recorded_one_quad_kernel(lib, shape):
    n, c, h, w, g = shape
    tag = f"n{n}c{c}h{h}w{w}g{g}"
    a = {name: np.load(GOLDEN / f"{tag}_{name}.npy")
         for name in ("y", "pooled_dy", "ysel", "dy", "idx", "gamma", "beta", "mean", "invstd", "dgamma", "dbeta")}
    y, pdy, ysel = (from_bits(a[k]).to(DEV) for k in ("y", "pooled_dy", "ysel"))
    assert y.shape == (n, h, w, c) and pdy.shape == (n, pooled_side(h), pooled_side(w), c)
    idx = torch.from_numpy(a["idx"]).to(DEV)
    gamma, beta, mean, invstd = (torch.from_numpy(a[k]).to(DEV) for k in ("gamma", "beta", "mean", "invstd"))
    dy, dgamma, dbeta = fused_backward(lib, y, ysel, pdy, idx, gamma, beta, mean, invstd, g)
    want = from_bits(a["dy"])
    got_bits, want_bits = dy.cpu().view(torch.int16), want.view(torch.int16)
    assert torch.equal(got_bits, want_bits), f"dy: {(got_bits != want_bits).sum().item()} of {want.numel()} patterns differ"
    assert np.array_equal(dgamma.cpu().numpy(), a["dgamma"]) and np.array_equal(dbeta.cpu().numpy(), a["dbeta"])


def rel_max(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def rel_rms(got, ref):
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.gpu
def test_backward_matches_float64_on_several_blocks(lib, forward_cases):
    """MULTI_BLOCK against float64 autograd: BatchNorm per statistics group, ReLU, and a pooling that takes each window's
    value at the position the forward recorded (checked exactly above; float64 would break ties between values that are
    equal only after their bf16 rounding differently).  Bounds of test_bn_relu_maxpool_fused_matches_unfused: max |err| <=
    5e-3 max |ref| for dy and 3e-3 for dgamma / dbeta, relative RMS <= 4e-3 (bf16 rounding of dy: 2^-9 / sqrt 3 = 1.1e-3)."""
    n, c, h, w, g = MULTI_BLOCK
    k = forward_cases[MULTI_BLOCK]
    p, q = pooled_side(h), pooled_side(w)
    y, idx, ysel = k["y"], k["idx"], k["xsel"]
    gen = torch.Generator().manual_seed(77)
    pdy = torch.randn(n, p, q, c, generator=gen).bfloat16().to(DEV)
    gamma, beta = stem_inputs(n, c, h, w, seed=10 + FWD_SHAPES.index(MULTI_BLOCK))[1:]
    mean, invstd, _, _ = train_stats(lib, y, gamma, beta, g)
    dy, dgamma, dbeta = fused_backward(lib, y, ysel, pdy, idx, gamma, beta, mean, invstd, g)

    y64 = y.double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)          # [N, C, H, W]
    g64, b64 = gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    act = F.relu(torch.cat([F.batch_norm(part, None, None, g64, b64, True, 0.1, 1e-5) for part in y64.chunk(g)]))
    ap = F.pad(act, (1, 1, 1, 1))
    cands = torch.stack([ap[:, :, kh:kh + 2 * p - 1:2, kw:kw + 2 * q - 1:2] for kh in range(3) for kw in range(3)])
    pooled = cands.gather(0, idx.cpu().permute(0, 3, 1, 2).long()[None])[0]                # [N, C, P, Q]
    pooled.backward(pdy.double().cpu().permute(0, 3, 1, 2))
    ref_dy = y64.grad.permute(0, 2, 3, 1)
    figures = dict(dy_max=rel_max(dy.double().cpu(), ref_dy), dy_rms=rel_rms(dy.double().cpu(), ref_dy),
                   dgamma_max=rel_max(dgamma.double().cpu(), g64.grad), dbeta_max=rel_max(dbeta.double().cpu(), b64.grad))
    print("stem backward vs float64:", figures)
    assert figures["dy_max"] <= 5e-3 and figures["dy_rms"] <= 4e-3, figures
    assert figures["dgamma_max"] <= 3e-3 and figures["dbeta_max"] <= 3e-3, figures


def test_forward_entry_point_still_refuses_unsupported_shapes(lib):
    def call(**over):
        a = dict(x=FAKE, scale=FAKE, shift=FAKE, N=2, H=8, W=8, C=64, G=2, y=FAKE, idx=FAKE, xsel=None, stream=None)
        assert not set(over) - set(a)
        a.update(over)
        rc = lib.wm_bn_relu_maxpool3x3s2_fwd(*a.values())
        assert rc < 0, f"{over} passed validation (returned {rc}): it would launch on fake pointers"
        return rc

    for p in ("x", "scale", "shift", "y", "idx"):
        assert call(**{p: None}) == EINVAL, p
    for o in (dict(N=0), dict(H=1), dict(W=1), dict(C=0), dict(G=0)):
        assert call(**o) == EINVAL, o
    assert call(C=60) == EUNSUPPORTED                       # C % 8
    assert call(N=3) == EUNSUPPORTED                        # N % G
    assert call(N=64, H=2048, W=2048) == EUNSUPPORTED       # 2^31 16-byte items: past the 32-bit indices


def test_backward_entry_point_still_refuses_unsupported_shapes(lib):
    def call(**over):
        a = dict(y=FAKE, ysel=FAKE, pooled_dy=FAKE, pool_idx=FAKE, N=2, H=8, W=8, C=64, gamma=FAKE, beta=FAKE, save_mean=FAKE,
                 save_invstd=FAKE, G=2, dgamma=FAKE, dbeta=FAKE, accumulate=0, dy=FAKE, workspace=FAKE, workspace_bytes=1 << 30,
                 stream=None)
        assert not set(over) - set(a)
        a.update(over)
        rc = lib.wm_bn_relu_maxpool_bwd(*a.values())
        assert rc < 0, f"{over} passed validation (returned {rc}): it would launch on fake pointers"
        return rc

    assert call(pooled_dy=None) == EINVAL
    assert call(H=1) == EINVAL
    assert call(C=60) == EUNSUPPORTED                       # C % 8
    assert call(N=3, H=11, W=31) == EUNSUPPORTED            # rows % G
    assert call(N=1, H=2, W=2) == EUNSUPPORTED              # the single pooled row does not split into two groups
