"""csrc/pool.hip through its C entry points: wm_maxpool3x3s2_fwd / _bwd against the window scan of tests/kernel_check.py
(exactly: the first maximum in (kh, kw) order), wm_gap_fwd against float64 with the row-order float32 restatement as the
yardstick, wm_gap_bwd exactly.  Every output lies between sentinel margins that are asserted untouched."""
import kernel_check as kc
import numpy as np
import pytest
import torch
from guarded import DEV, Guarded, finish, ok, stream


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


POOL_SHAPES = [(1, 2, 2, 8), (2, 3, 5, 24), (3, 7, 6, 64), (2, 20, 22, 64)]      # (N, H, W, C)
POOL_FAMILIES = ("negative", "patches", "randn")


def pool_inputs(family, n, h, w, c, seed):
    """negative: every value below -0.5, so the padding can never win and a pad of 0 instead of -inf is wrong in every window
    on the border.  patches: constant patches, so that every window inside one ties at all nine positions.  randn."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=gen)
    if family == "negative":
        x = -x.abs() - 0.5
    elif family == "patches":
        x = x * 2 + 0.3
        x[0, : max((h + 1) // 2, 2), : max((w + 1) // 2, 2)] = -6.0
        x[-1, h // 2:, :] = 5.0
    return kc.bf(x)


def maxpool_fwd(lib, x):
    n, h, w, c = x.shape
    p, q = kc.pooled_side(h), kc.pooled_side(w)
    y, idx = Guarded((n, p, q, c), torch.bfloat16), Guarded((n, p, q, c), torch.uint8)
    xd = x.bfloat16().to(DEV)
    ok(lib, lib.wm_maxpool3x3s2_fwd(xd.data_ptr(), n, h, w, c, y.ptr, idx.ptr, stream()), "wm_maxpool3x3s2_fwd")
    finish("wm_maxpool3x3s2_fwd")
    return y.t.float().cpu(), idx.t.cpu()


def maxpool_bwd(lib, dy, idx, h, w):
    n, p, q, c = dy.shape
    dx = Guarded((n, h, w, c), torch.bfloat16)
    dyd, idd = dy.bfloat16().to(DEV), idx.to(DEV)
    ok(lib, lib.wm_maxpool3x3s2_bwd(dyd.data_ptr(), idd.data_ptr(), n, h, w, c, dx.ptr, stream()), "wm_maxpool3x3s2_bwd")
    finish("wm_maxpool3x3s2_bwd")
    return dx.t.float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("family", POOL_FAMILIES)
@pytest.mark.parametrize("n,h,w,c", POOL_SHAPES)
def test_maxpool_fwd_equals_the_window_scan(lib, n, h, w, c, family):
    x = pool_inputs(family, n, h, w, c, seed=h * w)
    best, code = kc.maxpool_ref(x)
    if family == "negative":
        assert float(x.max()) < 0 and not torch.equal(kc.maxpool_ref(x, "zero_pad")[0], best)
    if family == "patches" and h > 3:
        assert bool((code == 0).any()) and bool((x == 5.0).any())      # windows that tie from their first position on
    y, idx = maxpool_fwd(lib, x)
    assert torch.equal(y, best), f"y: {(y != best).sum().item()} of {y.numel()} differ"
    assert torch.equal(idx, code), f"idx: {(idx != code).sum().item()} of {idx.numel()} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,c", POOL_SHAPES)
def test_maxpool_bwd(lib, n, h, w, c):
    """Integer gradients: at most four of them meet in a pixel, the sum is exact.  randn gradients: check() with one bf16
    rounding of the float64 sum as the emulation."""
    x = pool_inputs("patches", n, h, w, c, seed=h * w)
    _, code = kc.maxpool_ref(x)
    gen = torch.Generator().manual_seed(n + h)
    dyi = torch.randint(-2, 3, code.shape, generator=gen).float()
    ref = kc.maxpool_bwd_ref(dyi, code, h, w)
    dx = maxpool_bwd(lib, dyi, code, h, w)
    assert torch.equal(dx.double(), ref), f"{(dx.double() != ref).sum().item()} of {ref.numel()} differ"
    dyr = kc.bf(torch.randn(code.shape, generator=gen))
    ref = kc.maxpool_bwd_ref(dyr, code, h, w)
    kc.check(maxpool_bwd(lib, dyr, code, h, w), ref, kc.bf(ref), f"maxpool_bwd randn {n}x{h}x{w}x{c}")


@pytest.mark.gpu
def test_maxpool_bwd_with_four_windows_on_one_pixel(lib):
    """A hand-made idx: pixel (1, 1) is selected by all four windows that cover it -- (0, 0) at code 8, (0, 1) at 6, (1, 0) at 2,
    (1, 1) at 0 -- every other window selects its centre."""
    n, h, w, c = 2, 3, 5, 24
    p, q = kc.pooled_side(h), kc.pooled_side(w)
    idx = torch.full((n, p, q, c), 4, dtype=torch.uint8)
    idx[:, 0, 0], idx[:, 0, 1], idx[:, 1, 0], idx[:, 1, 1] = 8, 6, 2, 0
    dy = torch.randint(1, 4, (n, p, q, c), generator=torch.Generator().manual_seed(4)).float()
    dx = maxpool_bwd(lib, dy, idx, h, w)
    ref = kc.maxpool_bwd_ref(dy, idx, h, w)
    assert torch.equal(ref[:, 1, 1], (dy[:, 0, 0] + dy[:, 0, 1] + dy[:, 1, 0] + dy[:, 1, 1]).double())
    assert torch.equal(dx.double(), ref)


# N so that N C / 8 threads are more than one block of 256 and no multiple of it
GAP_CASES = [(hw, c, n) for hw in (1, 49, 3136) for c, n in ((8, 259), (24, 87), (512, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,c,n", GAP_CASES)
def test_gap(lib, hw, c, n):
    assert n * c // 8 > 256 and (n * c // 8) % 256 != 0
    gen = torch.Generator().manual_seed(hw + c)
    x = kc.bf(torch.randn(n, hw, c, generator=gen) * 2 + 0.5)
    y = Guarded((n, c), torch.bfloat16)
    xd = x.bfloat16().to(DEV)
    ok(lib, lib.wm_gap_fwd(xd.data_ptr(), n, hw, c, y.ptr, stream()), "wm_gap_fwd")
    finish("wm_gap_fwd")
    kc.check(y.t.cpu(), kc.gap_ref(x), kc.gap_ref(x, emulate=True), f"gap_fwd {n}x{hw}x{c}")
    dy = torch.randn(n, c, generator=gen).bfloat16()
    dx = Guarded((n, hw, c), torch.bfloat16)
    dyd = dy.to(DEV)
    ok(lib, lib.wm_gap_bwd(dyd.data_ptr(), n, hw, c, dx.ptr, stream()), "wm_gap_bwd")
    finish("wm_gap_bwd")
    want = (dy.float() * torch.tensor(np.float32(1.0) / np.float32(hw))).bfloat16()
    assert torch.equal(dx.t.cpu(), want.unsqueeze(1).expand(n, hw, c))
