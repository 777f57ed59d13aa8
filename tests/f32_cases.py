"""References, emulations and input families of the float32 ("parity") kernels of csrc/f32path.hip, one per wm_f32_*
entry point; the sibling of loss_cases.py and knn_cases.py (no GPU import).

The comparison is kernel_check.check with ulp = one float32 ulp (F32_ULP).  `ref64` is the float64 result on the same float32
inputs; where tests/kernel_check.py already has that reference (conv_ref, bn_forward_ref, bn_backward_ref, layer_norm_ref,
bias_act_ref, attention_ref, maxpool_ref, ...) it is used, not restated.  The emulation (`*_emul`) is float64 everywhere
except where the kernel rounds: every float32 operation of its code is one f32_round here, an fmaf is one rounding of
a * b + c, and the double sums follow the kernel's stated order (slabs for the weight gradient, row slices for the BatchNorm
sums, the tree of f32_reduce).  Two things the source does not pin down are modelled as the compiler does by default and can be
switched: `a * b + c` written as two float32 operations is contracted into one fma (uncontracted() rounds both -- the other
honest realisation, which tests/test_f32_cases_cpu.py holds against the same bounds); erff / expf / logf are taken as
correctly rounded (the device functions are within a few ulp: what FACTOR is for).

Factors are kernel_check's: FACTOR for element-wise outputs and outputs whose sums are double, F32_SUM_FACTOR for outputs
that are a float32 chain over a reduction (convolution forward, input gradient, weight-gradient slabs, attention), f32_sum_floor /
f32_stat_floor where the emulation can land on the exact value.

Every emulation has switches (`seed_error`) that seed ONE wrong computation, values only; SWITCHES lists them per entry point
and tests/test_f32_cases_cpu.py proves each rejected on a named case."""
import contextlib

import kernel_check as kc
import numpy as np
import torch
from kernel_check import f32_round as r32

F32_ULP = 2.0 ** -23
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2

_CONTRACT = True


@contextlib.contextmanager
def uncontracted():
    """Inside the block a * b + c of two float32 operations is rounded twice (no fma contraction)"""
    global _CONTRACT
    _CONTRACT = False
    try:
        yield
    finally:
        _CONTRACT = True


def f32c(v) -> float:
    """a float constant / scalar argument as the kernel holds it"""
    return float(np.float32(v))


def fma32(a, b, c):
    """fmaf(a, b, c): one rounding (a, b float32-valued: the product is exact in float64)"""
    return r32(a * b + c)


def cfma32(a, b, c):
    """a * b + c as written in the source: contracted into an fma by default, two roundings under uncontracted()"""
    return r32(a * b + c) if _CONTRACT else r32(r32(a * b) + c)


def cmsub32(a, b, m):
    """a * b - m as written in the source (expf(s * scale - mx)): contracted, it is ONE rounding of the exact product minus m --
    for the row's maximum, whose m is the ROUNDED product, not 0 but the product's rounding error.  Measured on the MI355X: the
    compiler contracts it (wm_f32_softmax_rows on a single column answers log-probabilities of 1e-12 .. 3e-8 instead of 0)."""
    return r32(a * b - m) if _CONTRACT else r32(r32(a * b) - m)


def d64(t):
    return None if t is None else t.detach().double()


def fma_chain(a, b, steps=None):
    """[M, N]: acc = fmaf(a[:, j], b[j, :], acc) for j = 0, 1, ... (the first `steps` of them) in float32"""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
    for j in range(a.shape[1] if steps is None else steps):
        acc = r32(acc + a[:, j:j + 1] * b[j:j + 1, :])
    return acc


def tree_sum(v, f32=False):
    """sum over the last dim (a power of two) as `red[t] += red[t + o]`, o = n / 2 .. 1; f32: every addition rounded"""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
        if f32:
            v = r32(v)
    return v[..., 0]


def strided_sums(v, lanes, f32=False):
    """[..., lanes]: lane t adds v[..., t], v[..., t + lanes], ... in that order"""
    n = v.shape[-1]
    k = -(-n // lanes)
    p = torch.zeros(*v.shape[:-1], k * lanes, dtype=torch.float64)
    p[..., :n] = v
    p = p.reshape(*v.shape[:-1], k, lanes)
    acc = torch.zeros(*v.shape[:-1], lanes, dtype=torch.float64)
    for i in range(k):
        acc = acc + p[..., i, :]
        if f32:
            acc = r32(acc)
    return acc


# ------------------------------------------------------------------------------------------------ activations
def gelu32(v):
    """f32_gelu: 0.5f * v * (1.f + erff(v * 0.70710678f)), every operation rounded"""
    e = r32(torch.erf(r32(v * f32c(0.70710678118654752440))))
    return r32(r32(0.5 * v) * r32(1.0 + e))


def act32(v, act):
    if act == ACT_GELU:
        return gelu32(v)
    if act == ACT_RELU:
        return v.clamp_min(0.0) + 0.0
    return v


def act_bwd_emul(x, bias, dy, act, seed_error=None):
    """f32_act_bwd: dy * act'(x + bias).  seed_error "relu_ge_zero": the ReLU passes the gradient at exactly 0"""
    g = d64(dy)
    if act == ACT_NONE:
        return g
    v = d64(x)
    if bias is not None:
        v = r32(v + d64(bias))
    if act == ACT_GELU:
        cdf = r32(0.5 * r32(1.0 + r32(torch.erf(r32(v * f32c(0.70710678118654752440))))))
        pdf = r32(f32c(0.39894228040143267794) * r32(torch.exp(r32(r32(-0.5 * v) * v))))
        return r32(g * cfma32(v, pdf, cdf))
    keep = (v >= 0) if seed_error == "relu_ge_zero" else (v > 0)
    return g * keep


def bias_act_emul(x, bias, act, res=None, dy=None, seed_error=None):
    """wm_f32_bias_act (+ wm_f32_bias_act_bwd and the bias gradient's wm_f32_colsum) -> (y, dx, dbias).
    seed_error: "relu_ge_zero" (backward), "bias_row0" (the bias indexed by the row instead of the column)."""
    v = d64(x)
    if bias is not None:
        b = d64(bias)
        if seed_error == "bias_row0":
            b = b[torch.arange(v.shape[0]) % b.numel()].unsqueeze(1)
        v = r32(v + b)
    y = act32(v, act)
    if res is not None:
        y = r32(y + d64(res))
    if dy is None:
        return y, None, None
    dx = act_bwd_emul(x, bias, dy, act, seed_error)
    return y, dx, colsum_emul(dx)


def colsum_emul(x, seed_error=None):
    """wm_f32_colsum: one double sum per column in row order, rounded once.  seed_error "last_row": the last row left out"""
    v = d64(x)
    return r32((v[:-1] if seed_error == "last_row" else v).sum(0))


def offset_rows(rows, c, seed, offset=50.0):
    """family `offset`: [rows, c] float32, offset + randn (a float32 sum over the rows would carry the common term)"""
    return (offset + torch.randn(rows, c, generator=torch.Generator().manual_seed(seed))).float()


# ------------------------------------------------------------------------------------------------ convolution
# kernel_check's layouts: x [N, H, W, C], w [K, R, S, C], y / dy [N, P, Q, K], dw [K, R, S, C]
CONV_SWITCHES = ("drop_m_tail", "drop_k_tail", "drop_red_tail", "rs_swapped")
DGRAD_SWITCHES = ("no_divisibility", "drop_m_tail")
WGRAD_SWITCHES = ("slab_overrun", "last_slab_dropped")


def conv_inputs(family, n, h, w, c, k, r, s, stride, pad, seed):
    """kernel_check.conv_inputs with full float32 values, plus bias [K] and res [N, P, Q, K]"""
    p, q = kc.conv_out_hw(h, w, r, s, stride, pad)
    with kc.float32_inputs():
        t = kc.conv_inputs(family, n, h, w, c, k, r, s, p, q, seed)
    g = torch.Generator().manual_seed(seed + 104729)
    if family == "lattice":
        t["bias"], t["res"] = torch.randint(-2, 3, (k,), generator=g).float(), torch.randint(-2, 3, (n, p, q, k), generator=g).float()
    else:
        t["bias"], t["res"] = torch.randn(k, generator=g), torch.randn(n, p, q, k, generator=g)
    return t


def _fwd_gather(n, h, w, r, s, p, q, stride, pad, swapped):
    if not swapped:
        return kc.conv_gather(n, h, w, r, s, p, q, stride, pad)
    # column (r, s) reads the pixel of tap (s, r): what a decode that mixes r and s up fetches
    g = kc.conv_gather(n, h, w, s, r, p, q, stride, pad)
    return g.reshape(-1, s, r).transpose(1, 2).reshape(-1, r * s)


def conv_fwd_ref(x, w, stride, pad, bias=None, act=ACT_NONE, res=None):
    """act(conv(x, w) + bias) + res in float64 [N, P, Q, K]; also the pre-activation"""
    o = kc.conv_ref(x, w, stride, pad)
    pre = o["y_acc"] + (d64(bias) if bias is not None else 0.0)
    y = kc._act64(pre, act)
    if res is not None:
        y = y + d64(res).reshape(y.shape)
    return y.reshape(o["y"].shape), pre.reshape(o["y"].shape)


def conv_fwd_emul(x, w, stride, pad, bias=None, act=ACT_NONE, res=None, seed_error=None):
    """f32_conv_kernel<false>: one fmaf chain per output over the flattened (r, s, c) index in increasing order, then bias,
    activation, residual, each one float32 operation.
    seed_error: "drop_m_tail" / "drop_k_tail" (the ragged last 64-row / 64-channel tile not computed: zeros), "drop_red_tail"
    (the ragged last 16-deep reduction step left out), "rs_swapped" (tap decode with r and s exchanged)."""
    n, h, wd, c = x.shape
    k, r, s, _ = w.shape
    p, q = kc.conv_out_hw(h, wd, r, s, stride, pad)
    cols = kc.conv_im2col(x.reshape(-1, c), _fwd_gather(n, h, wd, r, s, p, q, stride, pad, seed_error == "rs_swapped"))
    kd = r * s * c
    v = fma_chain(cols, w.double().reshape(k, kd).t(), kd - kd % 16 if seed_error == "drop_red_tail" else None)
    if bias is not None:
        v = r32(v + d64(bias))
    v = act32(v, act)
    if res is not None:
        v = r32(v + d64(res).reshape(v.shape))
    m = v.shape[0]
    if seed_error == "drop_m_tail":
        v[m - m % 64:] = 0.0
    if seed_error == "drop_k_tail":
        v[:, k - k % 64:] = 0.0
    return v.reshape(n, p, q, k)


def dgrad_gather(n, h, w, r, s, p, q, stride, pad, no_divisibility=False):
    """[N H W, R S] long: the row of dy (output pixel in (n, p, q) order) that tap (r, s) of an INPUT pixel reads, -1 = none:
    ((h + pad - r) / stride, (w + pad - s) / stride) where both divide exactly.  no_divisibility: the quotient is taken
    without that test."""
    th = (torch.arange(h) + pad).view(h, 1, 1, 1) - torch.arange(r).view(1, 1, r, 1)
    tw = (torch.arange(w) + pad).view(1, w, 1, 1) - torch.arange(s).view(1, 1, 1, s)
    th, tw = th.expand(h, w, r, s), tw.expand(h, w, r, s)
    ok = (th >= 0) & (tw >= 0)
    if not no_divisibility:
        ok = ok & (th % stride == 0) & (tw % stride == 0)
    ph, pw = torch.div(th, stride, rounding_mode="floor"), torch.div(tw, stride, rounding_mode="floor")
    ok = ok & (ph < p) & (pw < q)
    g = (torch.arange(n) * (p * q)).view(n, 1, 1, 1, 1) + (ph * q + pw).unsqueeze(0)
    return torch.where(ok.unsqueeze(0).expand_as(g), g, torch.full_like(g, -1)).reshape(n * h * w, r * s)


def conv_dgrad_emul(dy, w, h, wd, stride, pad, seed_error=None):
    """f32_conv_kernel<true>: rows = input pixels, one fmaf chain over the flattened (r, s, k) index -> dx [N, H, W, C].
    seed_error: "no_divisibility", "drop_m_tail"."""
    n, p, q, k = dy.shape
    _, r, s, c = w.shape
    cols = kc.conv_im2col(dy.reshape(-1, k), dgrad_gather(n, h, wd, r, s, p, q, stride, pad, seed_error == "no_divisibility"))
    v = fma_chain(cols, w.double().permute(1, 2, 0, 3).reshape(r * s * k, c))
    if seed_error == "drop_m_tail":
        v[v.shape[0] - v.shape[0] % 64:] = 0.0
    return v.reshape(n, h, wd, c)


def wgrad_slabs(m, linear):
    """f32_wgrad_slabs: (Z, pixels per slab)"""
    chunk = 256 if linear else 4096
    z = max(1, min(256, -(-m // chunk)))
    return z, -(-m // z)


def conv_wgrad_emul(x, dy, r, s, stride, pad, seed_error=None):
    """f32_conv_wgrad + f32_wgrad_finalize: per slab of pixels one fmaf chain per weight in pixel order, the slabs added in
    slab order in double, one rounding -> dw [K, R, S, C].
    seed_error: "slab_overrun" (the last 16-pixel step of a slab is guarded by m < M instead of m < me: it adds the first
    pixels of the next slab), "last_slab_dropped"."""
    n, h, wd, c = x.shape
    _, p, q, k = dy.shape
    m = n * p * q
    z, chunk = wgrad_slabs(m, p == 1 and q == 1 and r == 1 and s == 1)
    cols = kc.conv_im2col(x.reshape(-1, c), kc.conv_gather(n, h, wd, r, s, p, q, stride, pad))
    span = -(-chunk // 16) * 16 if seed_error == "slab_overrun" else chunk
    px = (torch.arange(z) * chunk).view(z, 1) + torch.arange(span).view(1, span)
    end = torch.full((z, 1), m) if seed_error == "slab_overrun" else ((torch.arange(z) + 1) * chunk).clamp_max(m).view(z, 1)
    px = torch.where(px < end, px, torch.full_like(px, m))                     # row m = zeros
    a = torch.cat([dy.double().reshape(m, k), torch.zeros(1, k, dtype=torch.float64)])[px]       # [Z, span, K]
    b = torch.cat([cols, torch.zeros(1, cols.shape[1], dtype=torch.float64)])[px]                # [Z, span, RSC]
    acc = torch.zeros(z, k, cols.shape[1], dtype=torch.float64)
    for t in range(span):
        acc = r32(acc + a[:, t, :, None] * b[:, t, None, :])
    if seed_error == "last_slab_dropped":
        acc = acc[:-1]
    tot = torch.zeros_like(acc[0])
    for slab in acc:
        tot = tot + slab
    return r32(tot).reshape(k, r, s, c)


def wgrad_floor(x, dy, r, s, stride, pad):
    """f32_sum_floor of the weight gradient: one float32 rounding of the largest weight's sum of |dy| |x| over the pixels"""
    n, h, wd, c = x.shape
    _, p, q, k = dy.shape
    cols = kc.conv_im2col(x.reshape(-1, c), kc.conv_gather(n, h, wd, r, s, p, q, stride, pad))
    return float(2.0 ** -24 * (dy.double().reshape(-1, k).abs().t() @ cols.abs()).max())


# ------------------------------------------------------------------------------------------------ BatchNorm
BN_RB = 64
BN_FWD_SWITCHES = ("var_unclamped", "running_var_biased", "groups_share_stats")
BN_BWD_SWITCHES = ("mask_ge_zero", "dz_unmasked", "groups_share_stats")
BN_FAMILIES = kc.BN_FORWARD_FAMILIES


def bn_inputs(family, rows, c, groups, seed):
    """kernel_check.bn_forward_inputs with float32 values plus dout [rows, C].  `constant` differs: EVERY channel is constant
    within a group, at a value of 24 significant bits near 1000 (ss / n - mean^2 then cancels to rounding noise of either sign:
    the clamp at 0 decides), to be run with eps = 1e-12; `lattice` needs an even number of rows per group and is replaced by
    integer rows in -2 .. 2 where it is odd."""
    g = torch.Generator().manual_seed(seed + 15485863)
    rpg = rows // groups
    if family == "constant":
        const = (1000.0 + torch.rand(groups, c, generator=g) * 10).float()
        t = {"y": const[torch.arange(rows) // rpg].clone(), "residual": torch.randn(rows, c, generator=g),
             "gamma": torch.rand(c, generator=g) + 0.5, "beta": torch.randn(c, generator=g) * 0.3,
             "running_mean": torch.randn(c, generator=g) * 0.1, "running_var": torch.rand(c, generator=g) + 0.5}
    elif family == "lattice" and rpg % 2:
        t = {"y": torch.randint(-2, 3, (rows, c), generator=g).float(), "residual": torch.randint(-2, 3, (rows, c), generator=g).float(),
             "gamma": 2.0 ** torch.randint(-1, 2, (c,), generator=g).float(), "beta": torch.randint(-2, 3, (c,), generator=g).float(),
             "running_mean": torch.randint(-2, 3, (c,), generator=g).float() * 0.5,
             "running_var": torch.randint(1, 4, (c,), generator=g).float() * 0.5}
    else:
        with kc.float32_inputs():
            t = kc.bn_forward_inputs(family, rows, c, groups, seed)
    t["dout"] = torch.randint(-2, 3, (rows, c), generator=g).float() if family == "lattice" else torch.randn(rows, c, generator=g)
    return t


def bn_eps(family, rpg):
    """lattice (even rows per group) is exact with eps = 0; constant needs an eps below its rounding noise; else torch's default"""
    if family == "lattice" and rpg % 2 == 0:
        return 0.0
    return 1e-12 if family == "constant" else 1e-5


def slice_sums(v):
    """f32_colsums + the finalize loop on the rows v [rpg, C] of one group: slice rb of 64, lane ty of 8 adds rows rb * 8 + ty +
    512 i in order; the 8 lanes are added in order, then the 64 slices (all in double)"""
    rpg, c = v.shape
    k = -(-rpg // (BN_RB * 8))
    p = torch.zeros(k * BN_RB * 8, c, dtype=torch.float64)
    p[:rpg] = v
    p = p.reshape(k, BN_RB, 8, c)
    lane = torch.zeros(BN_RB, 8, c, dtype=torch.float64)
    for i in range(k):
        lane = lane + p[i]
    part = torch.zeros(BN_RB, c, dtype=torch.float64)
    for ty in range(8):
        part = part + lane[:, ty]
    tot = torch.zeros(c, dtype=torch.float64)
    for rb in range(BN_RB):
        tot = tot + part[rb]
    return tot


def bn_fwd_emul(y, residual, gamma, beta, groups, eps, momentum, relu, running=None, seed_error=None):
    """wm_f32_bn_fwd, training: double sums (slice_sums), mean = s / n, var = max(ss / n - mean^2, 0), float32 mean, invstd = 1 /
    sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale, out = fmaf(y, scale, shift) (+ residual) (ReLU); the running
    statistics updated in float32 group after group with var n / (n - 1) (n > 1).
    -> dict(out, mean, invstd [G, C], running_mean, running_var).
    seed_error: "var_unclamped", "running_var_biased", "groups_share_stats" (every group normalised with group 0's statistics)."""
    rows, c = y.shape
    rpg = rows // groups
    y64 = d64(y)
    ga = d64(gamma) if gamma is not None else torch.ones(c, dtype=torch.float64)
    be = d64(beta) if beta is not None else torch.zeros(c, dtype=torch.float64)
    e, mom = f32c(eps), f32c(momentum)
    keep = float(np.float32(1.0) - np.float32(momentum))
    rm, rv = (d64(running[0]).clone(), d64(running[1]).clone()) if running is not None else (None, None)
    means, invs, scs, shs = [], [], [], []
    for g in range(groups):
        yg = y64[g * rpg:(g + 1) * rpg]
        m = slice_sums(yg) / rpg
        var = slice_sums(yg * yg) / rpg - m * m
        if seed_error != "var_unclamped":
            var = var.clamp_min(0.0)
        fm, inv = r32(m), r32(1.0 / torch.sqrt(var + e))
        sc = r32(ga * inv)
        means.append(fm), invs.append(inv), scs.append(sc), shs.append(cfma32(-fm, sc, be))
        unb = var if seed_error == "running_var_biased" or rpg == 1 else var * rpg / (rpg - 1)
        if running is not None:
            rm, rv = cfma32(torch.tensor(mom, dtype=torch.float64), fm, r32(keep * rm)), cfma32(torch.tensor(mom, dtype=torch.float64), r32(unb), r32(keep * rv))
    mean, invstd, scale, shift = (torch.stack(t) for t in (means, invs, scs, shs))
    grp = torch.arange(rows) // rpg
    if seed_error == "groups_share_stats":
        grp = torch.zeros_like(grp)
    v = fma32(y64, scale[grp], shift[grp])
    if residual is not None:
        v = r32(v + d64(residual))
    if relu:
        v = v.clamp_min(0.0) + 0.0
    return {"out": v, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv}


def bn_fwd_floors(t, ref):
    """the absolute floors of the forward's tensors : one float32 rounding at the
    magnitude that enters each statistic; `out` carries the roundings of shift = beta - mean scale, a product and a subtraction
    where the compiler does not contract them: two roundings at |mean scale|"""
    return {"out": 2.0 * kc.f32_stat_floor(ref["mean"] * ref["scale"], ref["shift"]), "mean": kc.f32_stat_floor(t["y"]),
            "invstd": kc.f32_stat_floor(ref["invstd"]), "running_mean": kc.f32_stat_floor(ref["mean"], t["running_mean"]),
            "running_var": kc.f32_stat_floor(ref["running_var"], t["running_var"])}


def bn_eval_emul(y, residual, gamma, beta, running_mean, running_var, eps, relu):
    """wm_f32_bn_fwd, eval: invstd = (float)(1 / sqrt((double)var + eps)), scale, shift, out as above"""
    c = y.shape[1]
    ga = d64(gamma) if gamma is not None else torch.ones(c, dtype=torch.float64)
    be = d64(beta) if beta is not None else torch.zeros(c, dtype=torch.float64)
    sc = r32(ga * r32(1.0 / torch.sqrt(d64(running_var) + f32c(eps))))
    v = fma32(d64(y), sc, cfma32(-d64(running_mean), sc, be))
    if residual is not None:
        v = r32(v + d64(residual))
    return v.clamp_min(0.0) + 0.0 if relu else v


def bn_bwd_emul(y, dout, out_relu, gamma, mean, invstd, groups, seed_error=None):
    """wm_f32_bn_bwd on the kernel's own operands (y, dout, the forward's output where it had a ReLU, the saved float32 mean /
    invstd): gm = dout where out > 0; double sums s1 = sum gm, s2 = sum gm xhat with the float32 xhat = (y - mean) invstd; float32
    c1 = s1 / n, c2 = s2 / n; dy = (gamma invstd) (gm - c1 - xhat c2); dgamma / dbeta = the sums over the groups, one rounding.
    -> dict(dy, dz, dgamma, dbeta, terms: the summed terms, dy_floor).  dy_floor: one float32 rounding at the largest of the three
    terms of dy -- on two rows per group they cancel to (almost) nothing, and what is left is the roundings of the terms, of which
    the emulation is one draw and a kernel that contracts another product another.  seed_error: "mask_ge_zero", "dz_unmasked", "groups_share_stats"."""
    rows, c = y.shape
    rpg = rows // groups
    grp = torch.arange(rows) // rpg
    if seed_error == "groups_share_stats":
        grp = torch.zeros_like(grp)
    ga = d64(gamma) if gamma is not None else torch.ones(c, dtype=torch.float64)
    gm = d64(dout)
    if out_relu is not None and seed_error != "dz_unmasked":
        o = d64(out_relu)
        gm = gm * ((o >= 0) if seed_error == "mask_ge_zero" else (o > 0))
    mu, inv = d64(mean)[grp], d64(invstd)[grp]
    xh = r32(r32(d64(y) - mu) * inv)
    s1 = torch.stack([slice_sums(gm[g * rpg:(g + 1) * rpg]) for g in range(groups)])
    s2 = torch.stack([slice_sums((gm * xh)[g * rpg:(g + 1) * rpg]) for g in range(groups)])
    c1, c2 = r32(s1 / rpg)[grp], r32(s2 / rpg)[grp]
    dy = r32(r32(ga * inv) * cfma32(-xh, c2, r32(gm - c1)))
    sc = (ga * inv).abs()
    return {"dy": dy, "dz": gm, "dgamma": r32(s2.sum(0)), "dbeta": r32(s1.sum(0)), "terms": (gm, gm * xh),
            "dy_floor": kc.f32_stat_floor(sc * gm, sc * c1, sc * xh * c2)}


# ------------------------------------------------------------------------------------------------ pooling
POOL_FAMILIES = ("three_level", "all_equal", "post_relu", "all_negative", "neg_inf_plane")
POOL_SWITCHES = ("last_max", "zero_pad")


def pool_inputs(family, n, h, w, c, seed):
    """(x [N, H, W, C], dy [N, P, Q, C]), dy integers in 1 .. 5 (sums of up to four of them are exact).
    three_level: values in {0, 1, 2} (a wafer map: every window holds ties); all_equal; post_relu: relu(randn - 0.8) (mostly
    zeros); all_negative: -1 - |randn| rounded to eighths (ties, and a padding that counted as 0 would win every border window);
    neg_inf_plane: three_level with image 0, channel 0 all -inf."""
    g = torch.Generator().manual_seed(seed)
    if family in ("three_level", "neg_inf_plane"):
        x = torch.randint(0, 3, (n, h, w, c), generator=g).float()
        if family == "neg_inf_plane":
            x[0, :, :, 0] = float("-inf")
    elif family == "all_equal":
        x = torch.full((n, h, w, c), 0.5)
    elif family == "post_relu":
        x = (torch.randn(n, h, w, c, generator=g) - 0.8).clamp_min(0.0)
    elif family == "all_negative":
        x = -1.0 - (torch.randn(n, h, w, c, generator=g).abs() * 8).round() / 8
    else:
        raise ValueError(family)
    p, q = kc.pooled_side(h), kc.pooled_side(w)
    return x, torch.randint(1, 6, (n, p, q, c), generator=g).float()


def maxpool_fwd_bwd(x, dy, seed_error=None):
    """(y [N, P, Q, C] float32, dx [N, H, W, C] float64) of max-pool 3x3 / 2 / 1: kernel_check's scan reference (exact: the tests
    compare with torch.equal).  seed_error "last_max" (odd H and W); "zero_pad": the padding counts as 0 -- a border window whose
    values are all negative answers 0 and gives its gradient to nobody."""
    n, h, w, c = x.shape
    # a window that holds nothing above -inf records its first position INSIDE the image (torch's forward starts its index there,
    # the kernel's `bh < 0` does the same); the scan reference would name the padding: the position is taken with -inf lifted to
    # the lowest finite float32, which still loses to nothing but the padding
    xs = torch.nan_to_num(x, neginf=torch.finfo(torch.float32).min)
    if seed_error == "zero_pad":
        y0, code = kc.maxpool_ref(x)[0], kc.maxpool_ref(xs)[1]
        y, _ = kc.maxpool_ref(x, "zero_pad")
        return y, kc.maxpool_bwd_ref(dy * (y == y0), code, h, w)
    return kc.maxpool_ref(x, seed_error)[0], kc.maxpool_bwd_ref(dy, kc.maxpool_ref(xs, seed_error)[1], h, w)


def gap_emul(x, seed_error=None):
    """wm_f32_gap on x [N, HW, C]: (float)(double sum / HW).  seed_error "hw_minus_1": the last pixel left out of the sum"""
    v = d64(x)
    return r32((v[:, :-1] if seed_error == "hw_minus_1" else v).sum(1) / x.shape[1])


def gap_bwd_emul(dy, hw):
    """wm_f32_gap_bwd: dy * (1.f / HW) on every pixel -> [N, HW, C]"""
    return r32(d64(dy) * float(np.float32(1.0) / np.float32(hw))).unsqueeze(1).expand(-1, hw, -1)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_SWITCHES = ("eps_dropped", "tail_dropped")


def ln_inputs(family, rows, c, seed):
    with kc.float32_inputs():
        return kc.layer_norm_inputs(family, rows, c, seed)


def _wave_sum(v, tail_dropped=False):
    """sum over the last dim as one wave does: lane c % 64 adds its elements in order, then the xor butterfly (double)"""
    if tail_dropped:
        v = v[..., :v.shape[-1] - v.shape[-1] % 64]
        if v.shape[-1] == 0:
            return torch.zeros(v.shape[:-1], dtype=torch.float64)
    return tree_sum(strided_sums(v, 64))


def _ln_stats(x, eps, seed_error):
    c = x.shape[1]
    mean = _wave_sum(x, seed_error == "tail_dropped") / c
    q = _wave_sum((x - mean.unsqueeze(1)).pow(2)) / c
    e = 0.0 if seed_error == "eps_dropped" else f32c(eps)
    return r32(mean).unsqueeze(1), r32(1.0 / torch.sqrt(q + e)).unsqueeze(1)


def ln_emul(x, gamma, beta, eps, dy=None, seed_error=None):
    """wm_f32_layernorm / wm_f32_layernorm_bwd -> (y, dx, dgamma, dbeta): double sums per wave, float32 mean and rstd,
    y = (x - mean) rstd gamma + beta; gg = dy gamma, double means of gg and gg xhat, rounded, dx = rstd (gg - ma - xhat mb);
    dgamma / dbeta double sums over the rows of dy xhat / dy, one rounding.
    seed_error: "eps_dropped", "tail_dropped" (the columns past the last full 64 left out of the mean)."""
    x64, ga = d64(x), d64(gamma)
    c = x64.shape[1]
    fm, rstd = _ln_stats(x64, eps, seed_error)
    xh = r32(r32(x64 - fm) * rstd)
    y = cfma32(xh, ga, d64(beta))
    if dy is None:
        return y, None, None, None
    g = d64(dy)
    gg = r32(g * ga)
    ma, mb = r32(_wave_sum(gg) / c).unsqueeze(1), r32(_wave_sum(gg * xh) / c).unsqueeze(1)
    dx = r32(rstd * cfma32(-xh, mb, r32(gg - ma)))
    return y, dx, r32((g * xh).sum(0)), r32(g.sum(0))


# ------------------------------------------------------------------------------------------------ attention
ATTN_SWITCHES = ("no_max", "first_stride_only", "dk_noscale")


def attn_inputs(family, b, s, h, hd, seed, scale=None):
    with kc.float32_inputs():
        return kc.attention_inputs(family, b, s, h, hd, seed, scale)


def _chain_dot(a, b, chunk=None):
    """sum over the last dim of a * b as fmaf chains: one chain (chunk None), or chains of `chunk` terms joined pairwise
    (f32_dot16 + f32_group_sum's xor butterfly)"""
    hd = a.shape[-1]
    chunk = hd if chunk is None else chunk
    parts = []
    for c0 in range(0, hd, chunk):
        acc = torch.zeros(torch.broadcast_shapes(a.shape[:-1], b.shape[:-1]), dtype=torch.float64)
        for d in range(c0, c0 + chunk):
            acc = r32(acc + a[..., d] * b[..., d])
        parts.append(acc)
    while len(parts) > 1:
        parts = [r32(parts[i] + parts[i + 1]) for i in range(0, len(parts), 2)]
    return parts[0]


def attention_emul(qkv, scale, dout=None, seed_error=None):
    """wm_f32_attention (-> out [B, S, H, hd]) and wm_f32_attention_bwd (-> dqkv [B, S, 3, H, hd]) on qkv [B, S, 3, H, hd].
    Forward: logit = one fmaf chain over hd, times scale; the row maximum; p = expf(logit - max); l and o = sum p v added key
    after key in float32; out = o * (1 / l).  Backward: the logits as 16-term chains joined pairwise, the statistics as the
    forward takes them, p = expf(.) * (1 / l), ds = p (dO . v - dO . O), dq / dk / dv fmaf chains over keys / queries, dq and dk
    times scale.
    seed_error: "no_max" (the maximum not subtracted), "first_stride_only" (forward: queries past the first 256 not computed;
    backward: rows past the first 256 / (hd / 16)), "dk_noscale"."""
    b, s, _, h, hd = qkv.shape
    x = d64(qkv)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))                  # [B, H, S, hd]
    sc = f32c(scale)

    def shifted(logit):
        mx = torch.zeros_like(logit[..., :1]) if seed_error == "no_max" else r32(logit * sc).max(-1, keepdim=True).values
        return cmsub32(logit, sc, mx)

    e = r32(torch.exp(shifted(_chain_dot(q.unsqueeze(-2), k.unsqueeze(-3)))))
    l, o = torch.zeros(b, h, s, dtype=torch.float64), torch.zeros(b, h, s, hd, dtype=torch.float64)
    for j in range(s):
        l = r32(l + e[..., j])
        o = r32(o + e[..., j, None] * v[..., None, j, :])
    out = r32(o * r32(1.0 / l).unsqueeze(-1))
    if seed_error == "first_stride_only":
        out[:, :, 256:] = 0.0
    out = out.transpose(1, 2)                                                  # [B, S, H, hd]
    if dout is None:
        return out, None
    g, of = d64(dout).transpose(1, 2), out.transpose(1, 2)
    e = r32(torch.exp(shifted(_chain_dot(q.unsqueeze(-2), k.unsqueeze(-3), 16))))
    l = torch.zeros(b, h, s, dtype=torch.float64)
    for j in range(s):
        l = r32(l + e[..., j])
    p = r32(e * r32(1.0 / l).unsqueeze(-1))                                    # [B, H, S(query), S(key)]
    dd = _chain_dot(g, of, 16).unsqueeze(-1)
    ds = r32(p * r32(_chain_dot(g.unsqueeze(-2), v.unsqueeze(-3), 16) - dd))
    dq, dk, dv = (torch.zeros(b, h, s, hd, dtype=torch.float64) for _ in range(3))
    for j in range(s):
        dq = r32(dq + ds[..., :, j, None] * k[..., None, j, :])
    for i in range(s):
        dv = r32(dv + p[..., i, :, None] * g[..., None, i, :])
        dk = r32(dk + ds[..., i, :, None] * q[..., None, i, :])
    dq = r32(dq * sc)
    if seed_error != "dk_noscale":
        dk = r32(dk * sc)
    grads = torch.stack([dq, dk, dv], 0)                                       # [3, B, H, S, hd]
    if seed_error == "first_stride_only":
        grads[:, :, :, 256 // (hd // 16):] = 0.0
    return out, grads.permute(1, 3, 0, 2, 4)


# ------------------------------------------------------------------------------------------------ softmax rows, pair CE, reduce
SOFTMAX_SWITCHES = ("subtract_ignored",)
PAIR_CE_SWITCHES = ("diag_not_zeroed", "decode_order")
REDUCE_SWITCHES = ("tail_dropped",)
LOSS_BWD_SWITCHES = ("l1_sign_at_zero",)


def softmax_inputs(family, rows, d, seed):
    """(x [rows, D], subtract [D]): randn 3 randn; big: logits of magnitude 80 (x = +-80 + randn: without the maximum expf
    overflows at inverse temperature 10); constant: every row constant (uniform probabilities)"""
    g = torch.Generator().manual_seed(seed)
    sub = torch.randn(d, generator=g)
    if family == "randn":
        x = torch.randn(rows, d, generator=g) * 3
    elif family == "big":
        x = 80.0 * (torch.randint(0, 2, (rows, 1), generator=g).float() * 2 - 1) + torch.randn(rows, d, generator=g)
    elif family == "constant":
        x = (torch.randn(rows, 1, generator=g) * 5).expand(rows, d).clone()
    else:
        raise ValueError(family)
    return x, sub


def softmax_ref(x, subtract, inv_temp, log):
    z = (d64(x) - (d64(subtract) if subtract is not None else 0.0)) * f32c(inv_temp)
    return torch.log_softmax(z, -1) if log else torch.softmax(z, -1)


def softmax_emul(x, subtract, inv_temp, log, seed_error=None):
    """wm_f32_softmax_rows: z = (x - sub) * inv_temp, maximum, s = sum expf(z - m) by 256 lanes (each adds its elements in order)
    and the float32 tree, y = expf(z - m) / s or (z - m) - logf(s).  seed_error "subtract_ignored"."""
    v = d64(x)
    if subtract is not None and seed_error != "subtract_ignored":
        v = r32(v - d64(subtract))
    zm = cmsub32(v, f32c(inv_temp), r32(v * f32c(inv_temp)).max(-1, keepdim=True).values)
    e = r32(torch.exp(zm))
    s = tree_sum(strided_sums(e, 256, f32=True), f32=True).unsqueeze(-1)
    return r32(zm - r32(torch.log(s))) if log else r32(e / s)


def pair_ce_emul(probs, logq, t_views, s_views, batch, seed_error=None, rnd=r32):
    """wm_f32_pair_ce: pair i = (t, s, b), b fastest: -sum_d p[t, b, d] logq[s, b, d] in double, one rounding; 0 where t == s.
    rnd = identity gives the float64 reference.  seed_error: "diag_not_zeroed", "decode_order" (i decoded as (b, s, t), t fastest)."""
    d = probs.shape[-1]
    p, lq = d64(probs).reshape(t_views, batch, d), d64(logq).reshape(s_views, batch, d)
    out = torch.zeros(t_views * s_views * batch, dtype=torch.float64)
    for i in range(out.numel()):
        if seed_error == "decode_order":
            t, s, b = i % t_views, (i // t_views) % s_views, i // (t_views * s_views)
        else:
            b, s, t = i % batch, (i // batch) % s_views, i // (batch * s_views)
        if t != s or seed_error == "diag_not_zeroed":
            out[i] = -(p[t, b] * lq[s, b]).sum()
    return rnd(out)


def reduce_emul(a, b, mode, scale, seed_error=None, rnd=r32):
    """wm_f32_reduce: scale * sum f(a, b), f = a | (a - b)^2 | |a - b|, 1024 lanes in double (each adds its elements in order), the
    tree, one rounding.  seed_error "tail_dropped": only the first 1024 elements."""
    x = d64(a).reshape(-1)
    if mode:
        dlt = x - d64(b).reshape(-1)
        x = dlt * dlt if mode == 1 else dlt.abs()
    if seed_error == "tail_dropped":
        x = x[:1024]
    return rnd(tree_sum(strided_sums(x, 1024)) * float(scale))


def loss_bwd_emul(pred, target, mode, scale, grad_out, seed_error=None):
    """wm_f32_loss_bwd: f'(pred - target) * (g * scale), f' = 2 d (MSE) | sign d, 0 at 0 (L1).  seed_error "l1_sign_at_zero"."""
    gs = r32(torch.tensor(f32c(grad_out) * f32c(scale), dtype=torch.float64))
    dlt = r32(d64(pred) - d64(target))
    if mode == 1:
        f = 2.0 * dlt
    else:
        f = torch.sign(dlt)
        if seed_error == "l1_sign_at_zero":
            f = torch.where(dlt == 0, torch.ones_like(f), f)
    return r32(f * gs)


def loss_bwd_ref(pred, target, mode, scale, grad_out):
    dlt = d64(pred) - d64(target)
    return (2.0 * dlt if mode == 1 else torch.sign(dlt)) * (float(scale) * f32c(grad_out))


def center_update_emul(center, teacher, momentum, seed_error=None):
    """wm_f32_center_update: center * m + (1.f - m) * (float)(double column sum / rows).  seed_error "momentum_swapped"."""
    m = f32c(momentum)
    keep = float(np.float32(1.0) - np.float32(momentum))
    if seed_error == "momentum_swapped":
        m, keep = keep, m
    t = d64(teacher)
    return cfma32(torch.tensor(keep, dtype=torch.float64), r32(t.sum(0) / t.shape[0]), r32(d64(center) * m))


def center_update_ref(center, teacher, momentum):
    m = f32c(momentum)
    return d64(center) * m + (1.0 - m) * d64(teacher).mean(0)


def dino_loss_ref(student, probs, sv, tv, batch, temp, emulate=False):
    """lightly's DINOLoss on float32 inputs: mean over (t, s != t, b) of -sum p log softmax(student / temp); emulate: the three
    kernels in a row"""
    if emulate:
        logq = softmax_emul(student, None, 1.0 / temp, True)
        pair = pair_ce_emul(probs, logq, tv, sv, batch)
    else:
        logq = softmax_ref(student, None, 1.0 / temp, True)
        pair = pair_ce_emul(probs, logq, tv, sv, batch, rnd=lambda t: t)
    n_terms = tv * sv - min(tv, sv)
    return reduce_emul(pair, None, 0, 1.0 / (n_terms * batch), rnd=r32 if emulate else (lambda t: t))


SWITCHES = {"conv_fwd": CONV_SWITCHES, "conv_dgrad": DGRAD_SWITCHES, "conv_wgrad": WGRAD_SWITCHES, "bn_fwd": BN_FWD_SWITCHES,
            "bn_bwd": BN_BWD_SWITCHES, "maxpool": POOL_SWITCHES, "layernorm": LN_SWITCHES, "attention": ATTN_SWITCHES,
            "softmax": SOFTMAX_SWITCHES, "pair_ce": PAIR_CE_SWITCHES, "reduce": REDUCE_SWITCHES, "loss_bwd": LOSS_BWD_SWITCHES,
            "bias_act": ("relu_ge_zero", "bias_row0"), "colsum": ("last_row",), "gap": ("hw_minus_1",),
            "center_update": ("momentum_swapped",)}


def check32(got, ref64, emul, what, factor=kc.FACTOR, **kw):
    """kernel_check.check with one float32 ulp as the relative term of criterion 4"""
    return kc.check(got, ref64, emul, what, factor=factor, ulp=F32_ULP, **kw)


def elem_floor(ref64):
    """abs_floor (with floor_all) of an element-wise float32 output, a chain of two to five float32 operations per element: one
    float32 rounding at the largest magnitude.  On a few dozen elements the emulation's own worst element can sit well below
    half an ulp of the largest, and an honest kernel that rounds a * b + c twice cannot be asked to stay within twice that."""
    return kc.f32_stat_floor(ref64)


def verdict32(got, ref64, emul, factor=kc.FACTOR, **kw):
    rows, finite = kc.verdict(got, ref64, emul, factor, ulp=F32_ULP, **kw)
    return finite and all(m <= b for _, m, b in rows)
