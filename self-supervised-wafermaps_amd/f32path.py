"""Float32 ("parity") preset: tensor-level wrappers over the wm_f32_* entry points (csrc/f32path.hip).

The convolution / BatchNorm / pooling / Linear ops (the ResNet-18 + projection-head path) and the transformer ops of the MAE /
SimMIM steps (LayerNorm, fused bias + GELU, GELU Linear, attention, patch embedding, token assembly, row gather / scatter,
MSE / L1) have backward passes, so whole SimCLR, MAE and SimMIM optimiser steps run under the preset.  The DINO loss has no
backward yet and says so when differentiated (_NoBackward); nothing here detaches a gradient silently.  Activations are
float32: images / feature maps [N, C, H, W] in channels_last memory (NHWC), token and feature matrices [rows, C]; parameters
are used in their float32 master layout.  torch moves data here (cat, index gather / scatter, reshape); every FLOP runs in
the HIP kernels, sums over the batch of a broadcast parameter (class token, positional embedding, mask token) included
(wm_f32_colsum).  See precision.py for why the preset exists."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


class _NoBackward(torch.autograd.Function):
    """Marks a float32-preset result without a backward pass (the DINO loss): differentiating through it raises."""

    @staticmethod
    def forward(ctx, y, *deps):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, *g):
        raise NotImplementedError("float32 (parity) preset: this op has no backward pass (the DINO loss): run the backward "
                                  "pass under the bf16 preset")


def _mark(y: torch.Tensor, *deps) -> torch.Tensor:
    if torch.is_grad_enabled() and any(torch.is_tensor(d) and d.requires_grad for d in deps):
        return _NoBackward.apply(y, *[d for d in deps if torch.is_tensor(d)])
    return y


def _cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.WaferHipError(f"{what}: the HIP path needs a device tensor (no CPU fallback)")


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.detach().to(torch.float32).contiguous()


def as_nhwc(x: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] of any float dtype / layout -> float32 channels_last."""
    if x.dim() != 4:
        raise ValueError("expected a 4-D [N,C,H,W] tensor")
    return x.detach().to(torch.float32).contiguous(memory_format=torch.channels_last)


_WS = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    # per (device, stream): two passes may be in flight on different streams (the DINO teacher beside the student)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return ws


def _colsum(x: torch.Tensor, rows: int, c: int) -> torch.Tensor:
    """[c] = sum over the rows of x [rows, c] (ordered, double accumulation)."""
    out = torch.empty((c,), dtype=torch.float32, device=x.device)
    check(_lib.load().wm_f32_colsum(ptr(x), rows, c, ptr(out), stream_ptr()), "wm_f32_colsum")
    return out


class _Conv2d(torch.autograd.Function):
    """y = act(conv(x, w) + bias) + residual on NHWC float32; backward: the pre-activation recomputed by the forward kernel
    (act none) and taken through act' (act != none), then input gradient, weight gradient (pixel ranges summed in a fixed
    order), bias gradient = column sums, residual gradient = dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, padding, act):
        xs = as_nhwc(x)
        n, c, h, w = xs.shape
        k, c2, r, s = weight.shape
        if c2 != c:
            raise ValueError(f"conv2d: input channels {c} vs weight {tuple(weight.shape)}")
        p, q = (h + 2 * padding - r) // stride + 1, (w + 2 * padding - s) // stride + 1
        y = torch.empty((n, p, q, k), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
        lib = _lib.load()
        ws = _workspace(lib.wm_f32_conv2d_workspace_bytes(c, k, r, s), x.device)
        res = as_nhwc(residual) if residual is not None else None
        wf, bf = _f32(weight), _f32(bias)
        check(lib.wm_f32_conv2d_fwd(ptr(xs), ptr(wf), ptr(bf), ptr(res), ptr(y), n, h, w, c, k, r, s, p, q, stride,
                                    padding, int(act), ptr(ws), ws.numel(), stream_ptr()), "wm_f32_conv2d_fwd")
        ctx.save_for_backward(xs, wf, bf if int(act) != ACT_NONE else None)
        ctx.geom = (n, h, w, c, k, r, s, p, q, stride, padding)
        ctx.act, ctx.has_bias, ctx.has_res = int(act), bias is not None, residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, wf, bf = ctx.saved_tensors
        n, h, w, c, k, r, s, p, q, stride, padding = ctx.geom
        dy = as_nhwc(dy)
        lib = _lib.load()
        dres = dy if ctx.has_res else None
        if ctx.act != ACT_NONE:
            # dy of the pre-activation: the forward's GEMM (+ bias) run again without the activation, then act'
            pre = torch.empty((n, p, q, k), dtype=torch.float32, device=dy.device).permute(0, 3, 1, 2)
            ws = _workspace(lib.wm_f32_conv2d_workspace_bytes(c, k, r, s), dy.device)
            check(lib.wm_f32_conv2d_fwd(ptr(xs), ptr(wf), ptr(bf), 0, ptr(pre), n, h, w, c, k, r, s, p, q, stride, padding,
                                        ACT_NONE, ptr(ws), ws.numel(), stream_ptr()), "wm_f32_conv2d_fwd(recompute)")
            dpre = torch.empty_like(pre)
            check(lib.wm_f32_bias_act_bwd(ptr(pre), 0, ptr(dy), ctx.act, n * p * q, k, ptr(dpre), stream_ptr()),
                  "wm_f32_bias_act_bwd")
            dy = dpre
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device).permute(0, 3, 1, 2)
            ws = _workspace(lib.wm_f32_conv2d_workspace_bytes(c, k, r, s), dy.device)
            check(lib.wm_f32_conv2d_dgrad(ptr(dy), ptr(wf), ptr(dx), n, h, w, c, k, r, s, p, q, stride, padding, ptr(ws),
                                          ws.numel(), stream_ptr()), "wm_f32_conv2d_dgrad")
        if ctx.needs_input_grad[1]:
            dw = torch.empty((k, c, r, s), dtype=torch.float32, device=dy.device)
            ws = _workspace(lib.wm_f32_conv2d_wgrad_workspace_bytes(n, p, q, c, k, r, s), dy.device)
            check(lib.wm_f32_conv2d_wgrad(ptr(dy), ptr(xs), ptr(dw), n, h, w, c, k, r, s, p, q, stride, padding, ptr(ws),
                                          ws.numel(), stream_ptr()), "wm_f32_conv2d_wgrad")
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy, n * p * q, k)
        return dx, dw, db, dres, None, None, None


def conv2d(x, weight, stride=1, padding=0, bias=None, act=ACT_NONE, residual=None):
    _cuda(x, "conv2d(float32)")
    return _Conv2d.apply(x, weight, bias, residual, int(stride), int(padding), int(act))


def linear(x, weight, bias=None, act=ACT_NONE, residual=None):
    """act(x @ W^T + bias) + residual on [rows, C]: the 1 x 1 convolution on a 1 x 1 image (same kernels, same backward)."""
    _cuda(x, "linear(float32)")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"linear: x {tuple(x.shape)} vs weight {tuple(weight.shape)}")
    rows, c = x.shape
    k = weight.shape[0]
    res4 = residual.reshape(rows, k, 1, 1) if residual is not None else None
    y = _Conv2d.apply(x.reshape(rows, c, 1, 1), weight.reshape(k, c, 1, 1), bias, res4, 1, 0, int(act))
    return y.reshape(rows, k)


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, residual, gamma, beta, running_mean, running_var, training, relu, eps, momentum, groups, counter):
        four = y.dim() == 4
        ys = as_nhwc(y) if four else _f32(y)
        if four:
            n, c, h, w = ys.shape
            rows = n * h * w
        else:
            rows, c = ys.shape
        g = groups if training else 1
        if rows % g:
            raise ValueError("batch_norm: rows not divisible by groups")
        res = None
        if residual is not None:
            res = as_nhwc(residual) if four else _f32(residual)
        out = torch.empty_like(ys)
        mean = torch.empty((g, c), dtype=torch.float32, device=y.device)
        invstd = torch.empty_like(mean)
        lib = _lib.load()
        ws = _workspace(lib.wm_f32_bn_workspace_bytes(rows, c, g), y.device)
        check(lib.wm_f32_bn_fwd(ptr(ys), ptr(res), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                ptr(counter) if training else 0, rows, c, g, int(bool(training)), float(eps),
                                float(momentum), int(bool(relu)), ptr(mean), ptr(invstd), ptr(out), ptr(ws), ws.numel(),
                                stream_ptr()), "wm_f32_bn_fwd")
        ctx.save_for_backward(ys, out if relu else None, mean, invstd, _f32(gamma))
        ctx.meta = (rows, c, g, bool(training), residual is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        ys, out, mean, invstd, gamma = ctx.saved_tensors
        rows, c, g, training, has_res = ctx.meta
        if not training:
            raise NotImplementedError("batch_norm (float32 preset): backward through eval-mode statistics is not implemented")
        dout = as_nhwc(dout) if dout.dim() == 4 else _f32(dout)
        lib = _lib.load()
        dy = torch.empty_like(ys)
        dz = torch.empty_like(ys) if has_res else None
        dgamma = torch.empty((c,), dtype=torch.float32, device=ys.device)
        dbeta = torch.empty_like(dgamma)
        ws = _workspace(lib.wm_f32_bn_workspace_bytes(rows, c, g), ys.device)
        check(lib.wm_f32_bn_bwd(ptr(ys), ptr(dout), ptr(out), ptr(gamma), ptr(mean), ptr(invstd), rows, c, g, ptr(dgamma),
                                ptr(dbeta), ptr(dy), ptr(dz), ptr(ws), ws.numel(), stream_ptr()), "wm_f32_bn_bwd")
        # each parameter's gradient follows its own requires_grad (a frozen gamma keeps beta trainable)
        return (dy, dz, (dgamma if ctx.needs_input_grad[2] else None), (dbeta if ctx.needs_input_grad[3] else None), None, None,
                None, None, None, None, None, None)


def batch_norm(y, gamma, beta, running_mean, running_var, training, residual=None, relu=False, eps=1e-5, momentum=0.1,
               groups=1, num_batches_tracked=None):
    _cuda(y, "batch_norm(float32)")
    return _BatchNorm.apply(y, residual, gamma, beta, running_mean, running_var, bool(training), bool(relu), float(eps),
                            float(momentum), int(groups), num_batches_tracked)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xs = as_nhwc(x)
        n, c, h, w = xs.shape
        p, q = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty((n, p, q, c), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
        check(_lib.load().wm_f32_maxpool3x3s2(ptr(xs), n, h, w, c, ptr(y), stream_ptr()), "wm_f32_maxpool3x3s2")
        ctx.save_for_backward(xs)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xs,) = ctx.saved_tensors
        n, c, h, w = xs.shape
        dy = as_nhwc(dy)
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device).permute(0, 3, 1, 2)
        check(_lib.load().wm_f32_maxpool3x3s2_bwd(ptr(xs), ptr(dy), n, h, w, c, ptr(dx), stream_ptr()), "wm_f32_maxpool3x3s2_bwd")
        return dx


def max_pool3x3s2(x):
    return _MaxPool.apply(x)


class _Gap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xs = as_nhwc(x)
        n, c, h, w = xs.shape
        y = torch.empty((n, c), dtype=torch.float32, device=x.device)
        check(_lib.load().wm_f32_gap(ptr(xs), n, h * w, c, ptr(y), stream_ptr()), "wm_f32_gap")
        ctx.geom = (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w = ctx.geom
        dy = _f32(dy)
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device).permute(0, 3, 1, 2)
        check(_lib.load().wm_f32_gap_bwd(ptr(dy), n, h * w, c, ptr(dx), stream_ptr()), "wm_f32_gap_bwd")
        return dx


def global_avg_pool(x):
    return _Gap.apply(x)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        xs = _f32(x)
        rows, c = xs.shape
        y = torch.empty_like(xs)
        gf = _f32(gamma)
        check(_lib.load().wm_f32_layernorm(ptr(xs), ptr(gf), ptr(_f32(beta)), float(eps), rows, c, ptr(y), stream_ptr()),
              "wm_f32_layernorm")
        ctx.save_for_backward(xs, gf)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, gf = ctx.saved_tensors
        rows, c = xs.shape
        dy = _f32(dy)
        lib = _lib.load()
        dx = torch.empty_like(xs)
        dg = torch.empty((c,), dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[1] else None
        db = torch.empty((c,), dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[2] else None
        ws = _workspace(lib.wm_f32_layernorm_bwd_workspace_bytes(rows, c), dy.device)
        check(lib.wm_f32_layernorm_bwd(ptr(xs), ptr(gf), ptr(dy), ctx.eps, rows, c, ptr(dx), ptr(dg), ptr(db), ptr(ws),
                                       ws.numel(), stream_ptr()), "wm_f32_layernorm_bwd")
        return dx, dg, db, None


def layer_norm(x, gamma, beta, eps=1e-6):
    _cuda(x, "layer_norm(float32)")
    return _LayerNorm.apply(x, gamma, beta, float(eps))


class _BiasAct(torch.autograd.Function):
    """y = act(x + bias) + residual; backward dx = dy * act'(x + bias), dbias = its column sums, dresidual = dy."""

    @staticmethod
    def forward(ctx, x, bias, residual, act):
        xs = _f32(x)
        shape = xs.shape
        xs = xs.reshape(-1, shape[-1])
        rows, c = xs.shape
        y = torch.empty_like(xs)
        res = _f32(residual).reshape(rows, c) if residual is not None else None
        bf = _f32(bias)
        check(_lib.load().wm_f32_bias_act(ptr(xs), ptr(bf), ptr(res), int(act), rows, c, ptr(y), stream_ptr()),
              "wm_f32_bias_act")
        if int(act) != ACT_NONE:
            ctx.save_for_backward(xs, bf)
        ctx.act, ctx.shape = int(act), shape
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.res_shape = residual.shape if residual is not None else None
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        c = ctx.shape[-1]
        g = _f32(dy).reshape(-1, c)
        rows = g.shape[0]
        if ctx.act == ACT_NONE:
            dx = g
        else:
            xs, bf = ctx.saved_tensors
            dx = torch.empty_like(g)
            check(_lib.load().wm_f32_bias_act_bwd(ptr(xs), ptr(bf), ptr(g), ctx.act, rows, c, ptr(dx), stream_ptr()),
                  "wm_f32_bias_act_bwd")
        db = _colsum(dx, rows, c).reshape(ctx.bias_shape) if ctx.bias_shape is not None and ctx.needs_input_grad[1] else None
        dres = g.reshape(ctx.res_shape) if ctx.res_shape is not None and ctx.needs_input_grad[2] else None
        return dx.reshape(ctx.shape), db, dres, None


def bias_act(x, bias=None, act=ACT_NONE, residual=None):
    _cuda(x, "bias_act(float32)")
    return _BiasAct.apply(x, bias, residual, int(act))


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, batch, seq, heads, scale, head_dim):
        q = _f32(qkv)
        if q.shape != (batch * seq, 3 * heads * head_dim):
            raise ValueError(f"attention: qkv {tuple(q.shape)} vs batch {batch} seq {seq} heads {heads} x {head_dim}")
        out = torch.empty((batch * seq, heads * head_dim), dtype=torch.float32, device=qkv.device)
        check(_lib.load().wm_f32_attention(ptr(q), batch, seq, heads, head_dim, scale, ptr(out), stream_ptr()), "wm_f32_attention")
        ctx.save_for_backward(q, out)
        ctx.geom = (batch, seq, heads, head_dim, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, out = ctx.saved_tensors
        batch, seq, heads, head_dim, scale = ctx.geom
        g = _f32(dout)
        dq = torch.empty_like(q)
        check(_lib.load().wm_f32_attention_bwd(ptr(q), ptr(out), ptr(g), batch, seq, heads, head_dim, scale, ptr(dq),
                                               stream_ptr()), "wm_f32_attention_bwd")
        return dq, None, None, None, None, None


def attention(qkv, batch, seq, heads, scale=None, head_dim=64):
    _cuda(qkv, "attention(float32)")
    sc = float(scale) if scale is not None else head_dim ** -0.5
    return _Attention.apply(qkv, int(batch), int(seq), int(heads), sc, int(head_dim))


def attention_segments(qkv, segments, heads, scale=None, head_dim=64):
    outs, off = [], 0
    for n, seq in segments:
        outs.append(attention(qkv[off:off + n * seq], n, seq, heads, scale, head_dim))
        off += n * seq
    return torch.cat(outs, dim=0)


def patch_embed(images, weight):
    """[N,3,S,S] images, conv weight [D,3,p,p] -> patch rows [N * (S/p)^2, D] (no bias; bias_act adds it)."""
    p = weight.shape[-1]
    y = conv2d(images, weight, stride=p, padding=0)          # logical [N, D, g, g], memory [N][g][g][D]
    n, d, g, _ = y.shape
    return y.permute(0, 2, 3, 1).reshape(n * g * g, d)


class _Broadcast(torch.autograd.Function):
    """t (any shape, m elements) -> [n, m], n copies of it; backward: the ordered column sum over the n copies."""

    @staticmethod
    def forward(ctx, t, n):
        ctx.shape, ctx.n = t.shape, n
        return _f32(t).reshape(1, -1).expand(n, -1).contiguous()

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        return _colsum(g, ctx.n, g.shape[1]).reshape(ctx.shape), None


def broadcast(t, n):
    """[n, t.numel()] rows, each a copy of t (a class / mask token, a positional embedding shared by n images)."""
    _cuda(t, "broadcast(float32)")
    return _Broadcast.apply(t, int(n))


class _TokensAssemble(torch.autograd.Function):
    """[cls + pos[0]; patches + pos[1:]] per image; backward: patch rows of dy, class-token / positional-embedding gradients
    as ordered column sums over the images."""

    @staticmethod
    def forward(ctx, patches, cls, pos, n, np_):
        d = patches.shape[1]
        tok = torch.cat([_f32(cls).reshape(1, 1, d).expand(n, 1, d), _f32(patches).reshape(n, np_, d)], dim=1)
        posx = _f32(pos).reshape(1, np_ + 1, d).expand(n, np_ + 1, d).contiguous()
        rows = n * (np_ + 1)
        y = torch.empty((rows, d), dtype=torch.float32, device=tok.device)
        check(_lib.load().wm_f32_bias_act(ptr(tok), 0, ptr(posx), ACT_NONE, rows, d, ptr(y), stream_ptr()), "wm_f32_bias_act")
        ctx.geom, ctx.shapes = (n, np_, d), (cls.shape, pos.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, np_, d = ctx.geom
        g = _f32(dy).reshape(n, np_ + 1, d)
        dpatch = dcls = dpos = None
        if ctx.needs_input_grad[0]:
            dpatch = g[:, 1:].reshape(n * np_, d)
        if ctx.needs_input_grad[1]:
            dcls = _colsum(g[:, 0].contiguous(), n, d).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[2]:
            dpos = _colsum(g, n, (np_ + 1) * d).reshape(ctx.shapes[1])
        return dpatch, dcls, dpos, None, None


def tokens_assemble(patches, cls, pos, n, np_):
    """[N * np, D] patch rows -> [N * (np + 1), D] token rows: class token first, positional embedding added."""
    _cuda(patches, "tokens_assemble(float32)")
    return _TokensAssemble.apply(patches, cls, pos, int(n), int(np_))


def _rows_index(idx, batch, k, c):
    return idx.long().reshape(batch, k, 1).expand(batch, k, c)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, batch, seq):
        xs = _f32(x)
        c = xs.shape[1]
        k = idx.shape[1]
        ctx.save_for_backward(idx)
        ctx.geom = (batch, seq, k, c)
        return torch.gather(xs.reshape(batch, seq, c), 1, _rows_index(idx, batch, k, c)).reshape(batch * k, c)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        batch, seq, k, c = ctx.geom
        dx = torch.zeros((batch, seq, c), dtype=torch.float32, device=dy.device)
        dx.scatter_(1, _rows_index(idx, batch, k, c), _f32(dy).reshape(batch, k, c))
        return dx.reshape(batch * seq, c), None, None, None


def gather_rows(x, idx, batch, seq):
    """out[b * K + j] = x[b * seq + idx[b, j]] (indices distinct per row); backward scatters the rows back."""
    return _GatherRows.apply(x, idx, int(batch), int(seq))


class _ScatterRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base, src, idx, batch, seq):
        b, s = _f32(base), _f32(src)
        c = b.shape[-1]
        k = idx.shape[1]
        out = b.reshape(batch, seq, c).clone()
        out.scatter_(1, _rows_index(idx, batch, k, c), s.reshape(batch, k, c))
        ctx.save_for_backward(idx)
        ctx.geom = (batch, seq, k, c)
        ctx.shapes = (base.shape, src.shape)
        return out.reshape(batch * seq, c)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        batch, seq, k, c = ctx.geom
        g = _f32(dout).reshape(batch, seq, c)
        ix = _rows_index(idx, batch, k, c)
        dbase = dsrc = None
        if ctx.needs_input_grad[0]:
            dbase = g.clone().scatter_(1, ix, 0.0).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[1]:
            dsrc = torch.gather(g, 1, ix).reshape(ctx.shapes[1])
        return dbase, dsrc, None, None, None


def scatter_rows(base, src, idx, batch, seq):
    """Copy of base [B*S, C] with rows idx [B, K] (distinct per row) replaced by src [B*K, C]."""
    return _ScatterRows.apply(base, src, idx, int(batch), int(seq))


def softmax_rows(x, subtract=None, inv_temp=1.0, log=False):
    xs = _f32(x)
    rows, d = xs.shape
    y = torch.empty_like(xs)
    check(_lib.load().wm_f32_softmax_rows(ptr(xs), ptr(_f32(subtract).reshape(-1)) if subtract is not None else 0, float(inv_temp),
                                          int(bool(log)), rows, d, ptr(y), stream_ptr()), "wm_f32_softmax_rows")
    return y


def _reduce(a, b, mode, scale):
    a = _f32(a).reshape(-1)
    b = _f32(b).reshape(-1) if b is not None else None
    out = torch.empty((), dtype=torch.float32, device=a.device)
    check(_lib.load().wm_f32_reduce(ptr(a), ptr(b), a.numel(), mode, float(scale), ptr(out), stream_ptr()), "wm_f32_reduce")
    return out


class _Loss(torch.autograd.Function):
    """mean over the elements of (pred - target)^2 (mode 1) or |pred - target| (mode 2); backward wm_f32_loss_bwd (the target's
    gradient is the same kernel with the operands swapped: f'(target - pred) = -f'(pred - target) for both modes)."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        p, t = _f32(pred).reshape(-1), _f32(target).reshape(-1)
        if p.numel() != t.numel():
            raise ValueError(f"loss: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
        ctx.save_for_backward(p, t)
        ctx.mode, ctx.shapes = mode, (pred.shape, target.shape)
        return _reduce(p, t, mode, 1.0 / p.numel())

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        gs = _f32(g).reshape(1)
        lib = _lib.load()
        grads = []
        for i, (a, b) in enumerate(((p, t), (t, p))):
            d = None
            if ctx.needs_input_grad[i]:
                d = torch.empty_like(a)
                check(lib.wm_f32_loss_bwd(ptr(a), ptr(b), a.numel(), ctx.mode, 1.0 / a.numel(), ptr(gs), ptr(d), stream_ptr()),
                      "wm_f32_loss_bwd")
                d = d.reshape(ctx.shapes[i])
            grads.append(d)
        return grads[0], grads[1], None


def mse_loss(pred, target):
    _cuda(pred, "mse_loss(float32)")
    return _Loss.apply(pred, target, 1)


def l1_loss(pred, target):
    _cuda(pred, "l1_loss(float32)")
    return _Loss.apply(pred, target, 2)


def dino_loss(student, probs, n_student_views, n_teacher_views, batch, student_temp):
    """lightly DINOLoss: mean over the (teacher view, student view != teacher view, sample) pairs of the cross entropy."""
    logq = softmax_rows(student, None, 1.0 / student_temp, log=True)
    d = logq.shape[1]
    pair = torch.empty(n_teacher_views * n_student_views * batch, dtype=torch.float32, device=logq.device)
    check(_lib.load().wm_f32_pair_ce(ptr(_f32(probs)), ptr(logq), n_teacher_views, n_student_views, batch, d, ptr(pair),
                                     stream_ptr()), "wm_f32_pair_ce")
    n_terms = n_teacher_views * n_student_views - min(n_teacher_views, n_student_views)
    return _mark(_reduce(pair, None, 0, 1.0 / (n_terms * batch)), student)


def dino_center_update(center, teacher, momentum):
    t = _f32(teacher)
    check(_lib.load().wm_f32_center_update(ptr(center), ptr(t), t.shape[0], t.shape[1], float(momentum), stream_ptr()),
          "wm_f32_center_update")
