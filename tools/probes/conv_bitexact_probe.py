"""Run a fixed set of conv / Linear launches through the C ABI and save the outputs: run once per library build
(WM_HIP_LIB selects it) and compare the files (kernel-restructuring changes that must be bit-identical).

    WM_HIP_LIB=<build A> python tools/probes/conv_bitexact_probe.py a.pt
    WM_HIP_LIB=<build B> python tools/probes/conv_bitexact_probe.py b.pt
    python tools/probes/conv_bitexact_probe.py --compare a.pt b.pt      # exit status 1 if any entry differs

The table reaches every instantiation of csrc/conv.hip and the hand-off to the panel kernel (which call reaches which
kernel: profiles/conv_refactor.md).  Geometry: (N, H, W, C, K, R, S, stride, pad); P x Q follows, except for the
space-to-depth stem (C = 16), whose output has the size of its input."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = [k for k in sorted(set(a) | set(b))
           if k not in a or k not in b or not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    print(f"{len(a)} / {len(b)} entries, {sum(torch.is_tensor(v) for v in a.values())} tensors, {len(bad)} differ")
    for k in bad:
        print("DIFFERS:", k)
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from ssl_wafermap_amd import _lib  # noqa: E402
from ssl_wafermap_amd._lib import check, ptr  # noqa: E402

lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda").manual_seed(0)
out = {}


def randn(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g, device="cuda") * scale).bfloat16()


def geometry(N, H, W, C, K, R, S, stride, pad):
    P, Q = (H, W) if C == 16 else ((H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1)
    return (N, H, W, C, K, R, S, P, Q, stride, pad)


def queries(tag, geom, groups=(1, 2)):
    """the three geometry questions the callers put to the library"""
    out[f"q_splits_{tag}"] = lib.wm_conv2d_wgrad_splits(*geom)
    for G in groups:
        out[f"q_bnstat_ok_{tag}_G{G}"] = lib.wm_conv2d_dgrad_bnstat_ok(*geom, G)
        rows = geom[0] * geom[7] * geom[8]
        if rows % G == 0:
            out[f"q_stats_tiles_{tag}_G{G}"] = lib.wm_conv2d_fwd_stats_tiles(*geom, rows // G)


def fwd(tag, geom, stats_groups=()):
    N, H, W, C, K, R, S, P, Q, stride, pad = geom
    x, wk = randn(N, H, W, C), randn(K, R, S, C, scale=0.05)
    y = torch.empty(N, P, Q, K, device="cuda", dtype=torch.bfloat16)
    check(lib.wm_conv2d_fwd(ptr(x), ptr(wk), ptr(y), *geom, st), "f")
    out["y" + tag] = y.cpu()
    for G in stats_groups:
        rpg = N * P * Q // G
        tiles = lib.wm_conv2d_fwd_stats_tiles(*geom, rpg)
        assert tiles > 0, (tag, tiles)
        part = torch.zeros(G, tiles, 2, K, device="cuda")
        y.zero_()
        check(lib.wm_conv2d_fwd_stats(ptr(x), ptr(wk), ptr(y), *geom, ptr(part), tiles, rpg, st), "fs")
        out[f"ys{tag}_G{G}"], out[f"stat{tag}_G{G}"] = y.cpu(), part.cpu()


def dgrad(tag, geom):
    N, H, W, C, K, R, S, P, Q, stride, pad = geom
    dy, wc, res = randn(N, P, Q, K), randn(C, R, S, K, scale=0.05), randn(N, H, W, C)
    dx = torch.empty(N, H, W, C, device="cuda", dtype=torch.bfloat16)
    check(lib.wm_conv2d_dgrad(ptr(dy), ptr(wc), ptr(dx), *geom, st), "d")
    out["dx" + tag] = dx.cpu()
    check(lib.wm_conv2d_dgrad_add(ptr(dy), ptr(wc), ptr(res), ptr(dx), *geom, st), "da")
    out["dxa" + tag] = dx.cpu()


def dgrad_bnstat(tag, geom, G):
    """the three mask forms: relu_x; relu_mask with a residual; recomputed from gamma / beta"""
    N, H, W, C, K, R, S, P, Q, stride, pad = geom
    assert lib.wm_conv2d_dgrad_bnstat_ok(*geom, G) == 1, tag
    rows = N * H * W
    dy, wc, res = randn(N, P, Q, K), randn(C, R, S, K, scale=0.05), randn(N, H, W, C)
    bn_y, relu_x = randn(N, H, W, C), randn(N, H, W, C)
    mask = torch.randint(0, 256, (rows, C // 8), generator=g, device="cuda", dtype=torch.uint8)
    gamma, beta = torch.randn(C, generator=g, device="cuda"), torch.randn(C, generator=g, device="cuda")
    mean = torch.randn(G, C, generator=g, device="cuda") * 0.1
    invstd = torch.rand(G, C, generator=g, device="cuda") + 0.5
    tiles = rows // G // 128
    for form, (r, rx, rm, ga, be) in {"x": (None, relu_x, None, None, None), "m": (res, None, mask, None, None),
                                      "g": (None, None, None, gamma, beta)}.items():
        dx = torch.zeros(N, H, W, C, device="cuda", dtype=torch.bfloat16)
        part = torch.zeros(G, tiles, 2, C, device="cuda")
        p = lambda t: ptr(t) if t is not None else None  # noqa: E731
        check(lib.wm_conv2d_dgrad_bnstat(ptr(dy), ptr(wc), p(r), ptr(dx), *geom, ptr(bn_y), p(rx), p(rm), p(ga), p(be),
                                         ptr(mean), ptr(invstd), G, ptr(part), tiles, st), "db")
        out[f"dxb{form}{tag}"], out[f"statb{form}{tag}"] = dx.cpu(), part.cpu()


def wgrad(tag, geom, bias=False):
    """raw slabs and, where wm_wgrad_finalize takes the shape, the folded gradient"""
    N, H, W, C, K, R, S, P, Q, stride, pad = geom
    x, dy = randn(N, H, W, C), randn(N, P, Q, K)
    nsplit = lib.wm_conv2d_wgrad_splits(*geom)
    assert nsplit > 0, (tag, nsplit)
    slabs = torch.zeros(nsplit, K, R, S, C, device="cuda")
    if bias:
        db = torch.zeros(nsplit, K, device="cuda")
        check(lib.wm_conv2d_wgrad_bias(ptr(dy), ptr(x), ptr(slabs), ptr(db), *geom, st), "wb")
        out["dbias" + tag] = db.cpu()
    else:
        check(lib.wm_conv2d_wgrad(ptr(dy), ptr(x), ptr(slabs), *geom, st), "w")
    out["slabs" + tag] = slabs.cpu()
    if C % 64 == 0:
        grad = torch.zeros(K, C, R, S, device="cuda")
        check(lib.wm_wgrad_finalize(ptr(slabs), nsplit, K, C, R, S, ptr(grad), 0, st), "wf")
        out["dw" + tag] = grad.cpu()


def linear(rows, C, K):
    x, dy = randn(rows, C), randn(rows, K)
    wk, wc = randn(K, C, scale=0.05), randn(C, K, scale=0.05)
    bias = torch.randn(K, generator=g, device="cuda")
    res, prex = randn(rows, K), randn(rows, C)
    y = torch.empty(rows, K, device="cuda", dtype=torch.bfloat16)
    pre, dx = torch.empty_like(y), torch.empty_like(x)
    geom = (rows, 1, 1, C, K, 1, 1, 1, 1, 1, 0)
    tag = f"{rows}_{C}_{K}"
    for form, (b, r) in {"": (bias, res), "b": (bias, None), "r": (None, res)}.items():  # bias and residual, either alone
        check(lib.wm_conv2d_fwd_bias_res(ptr(x), ptr(wk), ptr(b) if b is not None else None,
                                         ptr(r) if r is not None else None, ptr(y), *geom, st), "l")
        out[f"ly{form}{tag}"] = y.cpu()
    check(lib.wm_linear_bias_gelu_fwd(ptr(x), ptr(wk), ptr(bias), ptr(pre), ptr(y), rows, C, K, st), "g")
    out["lg" + tag], out["lp" + tag] = y.cpu(), pre.cpu()
    check(lib.wm_conv2d_dgrad(ptr(dy), ptr(wc), ptr(dx), *geom, st), "ld")
    out["ldx" + tag] = dx.cpu()
    check(lib.wm_linear_dgrad_gelu(ptr(dy), ptr(wc), ptr(prex), ptr(dx), rows, C, K, st), "ldg")
    out["ldg" + tag] = dx.cpu()
    queries("l" + tag, geom)


def tag_of(s):
    return "_".join(str(v) for v in s)


# ---- the layers of the models (forward, input gradient with and without a residual)
for s in ((8, 14, 14, 256, 256, 3, 3, 1, 1), (6, 28, 28, 128, 128, 3, 3, 1, 1), (4, 7, 7, 512, 512, 3, 3, 1, 1),
          (5, 56, 56, 64, 128, 3, 3, 2, 1), (5, 56, 56, 64, 128, 1, 1, 2, 0), (3, 13, 13, 64, 64, 3, 3, 1, 1),
          (2, 9, 9, 128, 192, 5, 5, 1, 2), (7, 10, 10, 64, 64, 1, 1, 1, 0)):
    fwd(tag_of(s), geometry(*s))
    dgrad(tag_of(s), geometry(*s))
for (rows, C, K) in ((1000, 384, 1152), (777, 192, 192), (300, 1536, 384), (129, 64, 64), (64, 2048, 128)):
    linear(rows, C, K)

# ---- every dispatch branch at small shapes
# forward: stem patch kernel (two groups of one image); stem conv_igemm (CPT 2) 64- and 128-wide; conv3x3_patch<0> (two
# groups); conv_igemm 64- and 128-wide with and without statistics; a ragged last tile
for s, groups in (((2, 16, 16, 16, 64, 4, 4, 1, 2), (2,)), ((8, 12, 12, 16, 64, 4, 4, 1, 2), (1,)),
                  ((8, 12, 12, 16, 128, 4, 4, 1, 2), (1,)), ((4, 8, 8, 64, 64, 3, 3, 1, 1), (2,)),
                  ((8, 4, 4, 64, 64, 3, 3, 1, 1), (1,)), ((8, 8, 8, 64, 128, 3, 3, 2, 1), (1,)),
                  ((2, 9, 11, 64, 64, 3, 3, 1, 1), ())):
    fwd("f" + tag_of(s), geometry(*s), groups)
    queries("f" + tag_of(s), geometry(*s))
# EPI (bias, residual, both, GELU; dgrad times gelu') at 129 rows, 64- and 128-wide both ways; the panel hand-off
# (192 -> 384 forward, K = 192 -> C = 384 input gradient)
for (rows, C, K) in ((129, 64, 128), (129, 128, 64), (129, 192, 384), (129, 384, 192)):
    linear(rows, C, K)
# input gradient: MODE 3 (9 x 11), conv3x3_patch<1>, MODE 2 (3x3 and 1x1, stride 2, whole tiles per parity class),
# MODE 1 (stride 2 with odd sides, or classes that are no multiple of 128)
for s in ((2, 9, 11, 64, 128, 3, 3, 1, 1), (2, 9, 11, 128, 128, 3, 3, 1, 1), (2, 8, 8, 64, 64, 3, 3, 1, 1),
          (8, 8, 8, 64, 128, 3, 3, 2, 1), (8, 8, 8, 128, 128, 3, 3, 2, 1), (8, 8, 8, 64, 128, 1, 1, 2, 0),
          (8, 8, 8, 128, 128, 1, 1, 2, 0), (1, 5, 7, 64, 64, 3, 3, 2, 1), (1, 5, 7, 128, 64, 3, 3, 2, 1),
          (1, 8, 8, 64, 64, 3, 3, 2, 1), (1, 8, 8, 128, 64, 3, 3, 2, 1)):
    dgrad("d" + tag_of(s), geometry(*s))
    queries("d" + tag_of(s), geometry(*s))
# BatchNorm-backward epilogue, two groups: MODE 3 64- and 128-wide, the patch kernel, MODE 2 64- and 128-wide
for s in ((4, 8, 8, 64, 128, 3, 3, 1, 1), (4, 8, 8, 128, 128, 3, 3, 1, 1), (4, 8, 8, 64, 64, 3, 3, 1, 1),
          (16, 8, 8, 64, 128, 3, 3, 2, 1), (16, 8, 8, 128, 128, 3, 3, 2, 1)):
    dgrad_bnstat("b" + tag_of(s), geometry(*s), 2)
    queries("b" + tag_of(s), geometry(*s))
# weight gradient: conv_wgrad_patch64; <64, 8, 3>; <64, 8, 1>; <128, 8, 3>; <128, 8, 2>; <128, 8, 1>; the stem forms
# <64, 2, 4>, <128, 2, 2> (4 x 4) and <64, 2, 1>, <128, 2, 1> (3 x 4)
for s in ((2, 8, 8, 64, 64, 3, 3, 1, 1), (2, 9, 11, 64, 64, 3, 3, 1, 1), (2, 9, 11, 64, 64, 1, 1, 1, 0),
          (2, 9, 11, 64, 128, 3, 3, 1, 1), (2, 9, 11, 256, 128, 1, 1, 1, 0), (2, 9, 11, 64, 128, 1, 1, 1, 0),
          (2, 16, 16, 16, 64, 4, 4, 1, 2), (2, 16, 16, 16, 128, 4, 4, 1, 2), (2, 16, 16, 16, 64, 3, 4, 1, 1),
          (2, 16, 16, 16, 128, 3, 4, 1, 1)):
    wgrad("w" + tag_of(s), geometry(*s))
    queries("w" + tag_of(s), geometry(*s))
# ... with a bias gradient: <64, 8, 1, true>, <128, 8, 1, true>, <128, 8, 2, true> (Linear, 129 rows), <64, 8, 3, true>
# (192 -> 64), <128, 8, 3, true> (a 3x3 call with dbias)
for s in ((129, 1, 1, 64, 64, 1, 1, 1, 0), (129, 1, 1, 64, 128, 1, 1, 1, 0), (129, 1, 1, 256, 128, 1, 1, 1, 0),
          (129, 1, 1, 192, 64, 1, 1, 1, 0), (2, 9, 11, 64, 128, 3, 3, 1, 1)):
    wgrad("wb" + tag_of(s), geometry(*s), bias=True)
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print(f"saved {len(out)} entries to {sys.argv[1]}")
