"""References, emulations and input families of the optimiser and update kernels: wm_sgd_step, wm_lars_step, wm_cast_f32_bf16
(csrc/layout.hip), wm_adamw_step in both decay modes, wm_ema_update, wm_dino_center_update, wm_colstats, wm_standardize,
wm_colscale_fwd / _bwd (csrc/transformer.hip), wm_scale_bf16 and wm_mean_f32 (csrc/core.hip); the sibling of f32_cases.py (no GPU
import).

`*_ref` is float64 on the same float32 / bf16 inputs: torch.optim.SGD / AdamW / Adam themselves on float64 copies (with the
hyper-parameters as Python holds them), a float64 restatement of oracle/resnet.py::lars_step, a numpy restatement of
sklearn.preprocessing.StandardScaler, closed forms for the rest.  `*_emul` is float64 with one float32 rounding per operation
of the kernel's source, in its order: an fmaf is one rounding, `a * b + c` written as two operations is contracted unless
inside f32_cases.uncontracted(), the hyper-parameters are held as float32 (what the kernel reads from `hyper`), the reductions
follow the launch arithmetic (row lanes, block slabs, then the atomics in block order -- ONE order of many).  The emulation is
the yardstick of f32_cases.check32, not an oracle: bit equality with the device is asked only on the `lattice` family, where
every float32 operation is exact.

Inside kernel_check.jitter(seed) every rounding of an emulation is preceded by a move of up to an eighth of a float32 ulp: other
rounding events, what another honest realisation of the same source looks like (tests/test_update_cases_cpu.py holds it against
the bounds of the GPU tests).

Every emulation takes `seed_error=`: ONE wrong computation, values only.  SWITCHES lists them per kernel and
tests/test_update_cases_cpu.py proves each rejected on a combination tests/test_gpu_update_kernels.py runs."""
import contextlib
import math

import f32_cases as fc
import kernel_check as kc
import numpy as np
import torch
from f32_cases import d64, f32c

ALIGN = 64                      # optim._ALIGN: every parameter starts on a 64-element boundary of its arena
SGD_CAP = 2048 * 256            # grid_for of csrc/layout.hip (wm_sgd_step, wm_cast_f32_bf16): one element per thread up to here
EW_CAP = 8192 * 256             # ew_blocks of csrc/transformer.hip (wm_adamw_step, wm_ema_update)
SCALE_CAP = 8 * 4096 * 256      # wm_scale_bf16: 4096 blocks of 256 threads, eight values each
LARS_BLOCKS, LARS_THREADS = 32, 256

SWITCHES = {
    "sgd": ("wd_dropped", "grad_scale_after_wd", "dampening", "nesterov", "buf_not_stored"),
    "adamw": ("l2_for_decoupled", "decoupled_for_l2", "bc1_missing", "bc2_not_sqrt", "eps_inside_sqrt", "eps_before_bc2",
              "decay_after_update", "grad_scale_dropped", "v_from_unscaled_g"),
    "lars": ("wd_not_added_to_g", "wd_missing_in_ratio", "ratio_before_wd", "norm_of_unscaled_g", "ratio_when_norm_zero",
             "ratio_without_wd_gate", "segment_takes_neighbour", "eps_dropped"),
    "ema": ("m_swapped",),
    "center": ("momentum_swapped", "sum_not_mean"),
    "colstats": ("unbiased_var", "var_about_zero"),
    "standardize": ("scale_not_inverse",),
    "colscale": ("dg_from_y", "dx_without_g"),
    "scale_bf16": ("truncate",),
    "cast": ("truncate",),
}

# hyper-parameter sets.  "own": what the models train with (SimCLR SGD, MAE AdamW, SwaV Adam, Barlow Twins and VICReg LARS).
# "visible": every term carries weight.  "lattice": powers of two, for the exact tier.
HYPER = {
    "sgd": {"own": dict(lr=0.06, momentum=0.9, weight_decay=5e-4, grad_scale=1.0),
            "visible": dict(lr=0.1, momentum=0.9, weight_decay=0.3, grad_scale=0.25),
            "lattice": dict(lr=0.5, momentum=0.5, weight_decay=0.25, grad_scale=0.25)},
    "adamw": {"own": dict(lr=1.5e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, grad_scale=1.0),
              "visible": dict(lr=0.1, betas=(0.9, 0.95), eps=1e-3, weight_decay=0.3, grad_scale=0.25),
              "lattice": dict(lr=0.25, betas=(0.5, 0.75), eps=1.0, weight_decay=0.5, grad_scale=1.0)},
    "adam": {"own": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6, grad_scale=1.0),
             "visible": dict(lr=0.1, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.3, grad_scale=0.25),
             "lattice": dict(lr=0.25, betas=(0.5, 0.75), eps=1.0, weight_decay=0.0, grad_scale=1.0)},
    "lars": {"barlow": dict(lr=0.2, momentum=0.9, weight_decay=1.5e-6, trust_coeff=0.001, eps=1e-8, grad_scale=1.0),
             "vicreg": dict(lr=0.3, momentum=0.9, weight_decay=1e-4, trust_coeff=0.001, eps=1e-8, grad_scale=1.0),
             "visible": dict(lr=0.2, momentum=0.9, weight_decay=0.1, trust_coeff=0.02, eps=1e-8, grad_scale=0.25),
             "wd0": dict(lr=0.2, momentum=0.9, weight_decay=0.0, trust_coeff=0.02, eps=1e-8, grad_scale=0.25)},
}


def r32(t):
    """one float32 operation of an emulation (kernel_check.f32_round); inside kernel_check.jitter() moved by up to an eighth
    of an ulp first"""
    if kc._JITTER is not None:
        t = t * (1.0 + 2.0 ** -27 * (2.0 * torch.rand(t.shape, generator=kc._JITTER, dtype=torch.float64) - 1.0))
    return kc.f32_round(t)


def fma32(a, b, c):
    return r32(a * b + c)


def cfma32(a, b, c):
    """a * b + c written as two float32 operations: see f32_cases.cfma32"""
    return r32(a * b + c) if fc._CONTRACT else r32(r32(a * b) + c)


def _h32(h):
    """the hyper-parameters as the kernel reads them: float32"""
    return {k: (tuple(f32c(x) for x in v) if isinstance(v, tuple) else f32c(v)) for k, v in h.items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ element-wise inputs
STEP_FAMILIES = ("randn", "tiny_grad", "lattice")


def step_inputs(family, n, seed, state="fresh"):
    """p, g, m (momentum buffer / exp_avg), v (exp_avg_sq) [n] float32.  state "warm": buffers as after many steps (random m,
    positive v).  tiny_grad: |g| in 1e-9 .. 1e-6 with exact zeros.  lattice: p in quarters, g in {0, +-1, +-3} (|g| + 1 a power
    of two: Adam's quotient is exact), m in halves; with HYPER[...]["lattice"] every float32 operation of a step is exact."""
    g_ = _gen(seed)
    if family == "lattice":
        p = torch.randint(-8, 9, (n,), generator=g_).float() / 4
        g = torch.tensor([-3.0, -1.0, 0.0, 1.0, 3.0])[torch.randint(0, 5, (n,), generator=g_)]
        m = torch.randint(-4, 5, (n,), generator=g_).float() / 2 if state == "warm" else torch.zeros(n)
        return {"p": p, "g": g, "m": m, "v": torch.zeros(n)}
    p = torch.randn(n, generator=g_)
    if family == "tiny_grad":
        mag = 10.0 ** (-9.0 + 3.0 * torch.rand(n, generator=g_, dtype=torch.float64))
        sign = torch.randint(0, 2, (n,), generator=g_).double() * 2 - 1
        g = (mag * sign * (torch.rand(n, generator=g_) > 0.125)).float()
        scale = 1e-7
    else:
        g = torch.randn(n, generator=g_)
        scale = 1.0
    if state == "warm":
        m = (0.3 * scale * torch.randn(n, generator=g_, dtype=torch.float64)).float()
        v = (scale * scale * (0.1 * torch.randn(n, generator=g_, dtype=torch.float64).pow(2) + 1e-3)).float()
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return {"p": p, "g": g, "m": m, "v": v}


# ------------------------------------------------------------------------------------------------ SGD
def _torch_step(cls, p, g, state, grad_scale, **kw):
    """one step of torch.optim.<cls> on float64 copies, from the given state entries"""
    q = torch.nn.Parameter(d64(p).clone())
    q.grad = d64(g) * grad_scale
    opt = cls([q], **kw)
    opt.state[q] = {k: (v if isinstance(v, torch.Tensor) and v.dim() == 0 else d64(v).clone()) for k, v in state.items()}
    opt.step()
    return q.detach(), opt.state[q]


def sgd_ref(p, g, mom, lr, momentum, weight_decay, grad_scale=1.0):
    """torch.optim.SGD in float64 -> (p, momentum buffer)"""
    q, st = _torch_step(torch.optim.SGD, p, g, {"momentum_buffer": mom}, grad_scale, lr=lr, momentum=momentum,
                        weight_decay=weight_decay)
    return q, st["momentum_buffer"]


def sgd_emul(p, g, mom, lr, momentum, weight_decay, grad_scale=1.0, seed_error=None):
    """sgd_step: gv = g * gs; gv = fmaf(wd, p, gv); b = fmaf(mu, mom, gv); p - lr * b (contractible)"""
    h = _h32(dict(lr=lr, mu=momentum, wd=weight_decay, gs=grad_scale))
    lr, mu, wd, gs = h["lr"], h["mu"], h["wd"], h["gs"]
    pv, gv, mo = d64(p), d64(g), d64(mom)
    if seed_error == "grad_scale_after_wd":
        gv = r32(fma32(wd, pv, gv) * gs)
    else:
        gv = r32(gv * gs)
        if seed_error != "wd_dropped":
            gv = fma32(wd, pv, gv)
    b = fma32(mu, mo, r32((1.0 - mu) * gv) if seed_error == "dampening" else gv)
    upd = fma32(mu, b, gv) if seed_error == "nesterov" else b
    return cfma32(-lr, upd, pv), (mo if seed_error == "buf_not_stored" else b)


# ------------------------------------------------------------------------------------------------ AdamW / Adam
def adam_ref(p, g, m, v, t, lr, betas, eps, weight_decay, grad_scale=1.0, l2=False):
    """step t (1-based) of torch.optim.AdamW (l2 False) / torch.optim.Adam (l2 True) in float64 -> (p, exp_avg, exp_avg_sq)"""
    cls = torch.optim.Adam if l2 else torch.optim.AdamW
    st = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
    q, st = _torch_step(cls, p, g, st, grad_scale, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    return q, st["exp_avg"], st["exp_avg_sq"]


def adam_emul(p, g, m, v, t, lr, betas, eps, weight_decay, grad_scale=1.0, l2=False, seed_error=None):
    """adamw_kernel with the host's hyper row (optim.AdamW._update: bc1 = 1 - b1^t and bc2 = 1 - b2^t in Python floats, stored
    as float32): bc2s = sqrtf(bc2); step = lr / bc1; gi = g * gs; L2: gi = fmaf(wd, p, gi), decoupled: p *= 1 - lr * wd;
    m = b1 m + (1 - b1) gi; v = b2 v + (1 - b2) gi gi; p -= step * m / (sqrtf(v) / bc2s + eps)."""
    bc1, bc2 = f32c(1.0 - betas[0] ** t), f32c(1.0 - betas[1] ** t)
    h = _h32(dict(lr=lr, betas=betas, eps=eps, wd=weight_decay, gs=grad_scale))
    lr, (b1, b2), eps, wd, gs = h["lr"], h["betas"], h["eps"], h["wd"], h["gs"]
    one = torch.ones((), dtype=torch.float64)
    bc2s = bc2 * one if seed_error == "bc2_not_sqrt" else r32(torch.sqrt(bc2 * one))
    step = lr * one if seed_error == "bc1_missing" else r32(lr / (bc1 * one))
    omb1, omb2 = r32((1.0 - b1) * one), r32((1.0 - b2) * one)
    pi, g0, mi, vi = d64(p), d64(g), d64(m), d64(v)
    gi = g0 if seed_error == "grad_scale_dropped" else r32(g0 * gs)
    gv = g0 if seed_error == "v_from_unscaled_g" else gi
    if seed_error == "l2_for_decoupled":
        l2 = True
    if seed_error == "decoupled_for_l2":
        l2 = False
    decay = cfma32(-lr * one, wd * one, one)
    if l2:
        gi = fma32(wd, pi, gi)
        if seed_error != "v_from_unscaled_g":
            gv = gi
    elif seed_error != "decay_after_update":
        pi = r32(pi * decay)
    mi = cfma32(b1, mi, r32(omb1 * gi))
    vi = cfma32(b2, vi, r32(r32(omb2 * gv) * gv))
    if seed_error == "eps_inside_sqrt":      # sqrt(v / bc2 + eps^2): the dimensionally consistent way to put eps under the root
        den = r32(torch.sqrt(r32(r32(vi / bc2) + r32(eps * eps * one))))
    elif seed_error == "eps_before_bc2":
        den = r32(r32(r32(torch.sqrt(vi)) + eps) / bc2s)
    else:
        den = r32(r32(r32(torch.sqrt(vi)) / bc2s) + eps)
    pi = r32(pi - r32(r32(step * mi) / den))
    if not l2 and seed_error == "decay_after_update":
        pi = r32(pi * decay)
    return pi, mi, vi


# ------------------------------------------------------------------------------------------------ EMA
def ema_ref(ema, p, m):
    return d64(ema) * m + d64(p) * (1.0 - m)


def ema_emul(ema, p, m, seed_error=None):
    """ema_kernel: ema * m + p * (1.f - m).  seed_error "m_swapped": the weights exchanged"""
    m = f32c(m)
    om = float(r32(torch.tensor(1.0 - m, dtype=torch.float64)))
    if seed_error == "m_swapped":
        m, om = om, m
    return cfma32(d64(ema), m, r32(d64(p) * om))


# ------------------------------------------------------------------------------------------------ LARS
LARS_LENGTHS = (7, 1, 64, 8191, 8192, 8193, 40000)
LARS_KINDS = ("randn", "randn", "zero_grad_param", "randn", "zero_weight_param", "tiny_grad", "randn")


def lars_arena(seed, state="fresh", rot=0, lengths=LARS_LENGTHS):
    """One flat arena as optim.LARS builds it: parameters of `lengths` on 64-element boundaries, zero gaps.  Segment kinds
    (rotated by `rot` over the lengths): randn; zero_grad_param (the whole gradient 0); zero_weight_param (the whole parameter 0);
    tiny_grad (|g| in 1e-9 .. 1e-6 with zeros, parameter of size 1e-3: a bias late in training -- the one place where `eps`
    carries weight).  -> p, g, mom [total] float32, seg [2 n] int64 (begin, end pairs), kinds."""
    g_ = _gen(seed)
    offs, total = [], 0
    for n in lengths:
        offs.append(total)
        total += (n + ALIGN - 1) // ALIGN * ALIGN
    p, g, mom = torch.zeros(total), torch.zeros(total), torch.zeros(total)
    kinds = [LARS_KINDS[(i + rot) % len(LARS_KINDS)] for i in range(len(lengths))]
    for o, n, kind in zip(offs, lengths, kinds):
        t = step_inputs("tiny_grad" if kind == "tiny_grad" else "randn", n, int(torch.randint(0, 2 ** 31, (1,), generator=g_)), state)
        # warm buffers at the size they have after many steps: ratio |g| / (1 - mu), ratio = trust_coeff |w| / |g| ~ 1e-4
        pv, gv, mv = t["p"] * 0.1, t["g"], t["m"] * (1.0 if kind == "tiny_grad" else 1e-3)
        if kind == "tiny_grad":
            pv = t["p"] * 1e-3
        if kind == "zero_grad_param":
            gv = torch.zeros(n)
        if kind == "zero_weight_param":
            pv = torch.zeros(n)
        p[o:o + n], g[o:o + n], mom[o:o + n] = pv, gv, mv
    seg = torch.tensor([x for o, n in zip(offs, lengths) for x in (o, o + n)], dtype=torch.int64)
    return {"p": p, "g": g, "mom": mom, "seg": seg, "kinds": kinds, "n": len(lengths)}


def lars_segments(seg):
    s = seg.tolist()
    return list(zip(s[0::2], s[1::2]))


def lars_ref(p, g, mom, seg, lr, momentum, weight_decay, trust_coeff, eps, grad_scale=1.0):
    """float64 restatement of oracle/resnet.py::lars_step (timm's Lars: dampening 0, no nesterov, no trust clip, always_adapt
    False) over the segments of a flat arena, on the scaled gradient -> (p, mom, squared norms [n, 2])"""
    p, g, mom = d64(p).clone(), d64(g) * grad_scale, d64(mom).clone()
    norms = []
    for b, e in lars_segments(seg):
        w, gr = p[b:e], g[b:e]
        norms.append([float(w.pow(2).sum()), float(gr.pow(2).sum())])
        if weight_decay != 0:
            wn, gn = w.norm(), gr.norm()
            ratio = trust_coeff * wn / (gn + wn * weight_decay + eps) if wn > 0 and gn > 0 else 1.0
            gr = (gr + weight_decay * w) * ratio
        mom[b:e] = mom[b:e] * momentum + gr
        p[b:e] = w - lr * mom[b:e]
    return p, mom, torch.tensor(norms, dtype=torch.float64)


_ATOMIC_ORDER = None


@contextlib.contextmanager
def atomics_shuffled(seed):
    """Inside the block the 32 block partials of a LARS squared norm are added in a random order: what the atomics do"""
    global _ATOMIC_ORDER
    _ATOMIC_ORDER = _gen(seed)
    try:
        yield
    finally:
        _ATOMIC_ORDER = None


def _lars_sqnorm32(v):
    """segment_sqnorms over one segment: 32 blocks x 256 threads, every thread an fmaf chain over its strided elements, the wave
    sums (a butterfly: a tree here), the four waves in order, the blocks' atomics in block order"""
    waves = _strided_fma(v, LARS_BLOCKS * LARS_THREADS).reshape(LARS_BLOCKS, LARS_THREADS // 64, 64)
    n = 64
    while n > 1:
        n //= 2
        waves = r32(waves[..., :n] + waves[..., n:2 * n])
    waves = waves[..., 0]
    blocks = r32(r32(r32(waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3])
    if _ATOMIC_ORDER is not None:
        blocks = blocks[torch.randperm(blocks.numel(), generator=_ATOMIC_ORDER)]
    tot = torch.zeros((), dtype=torch.float64)
    for b in blocks:
        tot = r32(tot + b)
    return tot


def _strided_fma(v, lanes):
    n = v.numel()
    k = -(-n // lanes)
    pad = torch.zeros(k * lanes, dtype=torch.float64)
    pad[:n] = v
    acc = torch.zeros(lanes, dtype=torch.float64)
    for row in pad.reshape(k, lanes):
        acc = r32(acc + row * row)
    return acc


def lars_emul(p, g, mom, seg, lr, momentum, weight_decay, trust_coeff, eps, grad_scale=1.0, seed_error=None):
    """segment_sqnorms + lars_step.  -> (p, mom, squared norms [n, 2])"""
    h = _h32(dict(lr=lr, mu=momentum, wd=weight_decay, tc=trust_coeff, eps=eps, gs=grad_scale))
    lr, mu, wd, tc, eps, gs = h["lr"], h["mu"], h["wd"], h["tc"], h["eps"], h["gs"]
    p, g0, mom = d64(p).clone(), d64(g), d64(mom).clone()
    segs = lars_segments(seg)
    total = p.numel()
    norms = []
    for i, (b, e) in enumerate(segs):
        pv, gv = p[b:e], r32(g0[b:e] * gs)
        # the norm's range: [begin, next begin) under the seeded error (the zero gap after the segment comes with it)
        ne = (segs[i + 1][0] if i + 1 < len(segs) else total) if seed_error == "segment_takes_neighbour" else e
        a = _lars_sqnorm32(p[b:ne])
        c = _lars_sqnorm32(g0[b:ne] if seed_error == "norm_of_unscaled_g" else r32(g0[b:ne] * gs))
        norms.append([float(a), float(c)])
        ratio = torch.ones((), dtype=torch.float64)
        gated = wd != 0.0 or seed_error == "ratio_without_wd_gate"
        if gated:
            wn, gn = r32(torch.sqrt(a)), r32(torch.sqrt(c))
            if (wn > 0 and gn > 0) or seed_error == "ratio_when_norm_zero":
                den = gn if seed_error == "wd_missing_in_ratio" else cfma32(wn, wd, gn)
                if seed_error != "eps_dropped":
                    den = r32(den + eps)
                ratio = r32(r32(tc * wn) / den)
        if gated:
            if seed_error == "wd_not_added_to_g":
                gv = r32(gv * ratio)
            elif seed_error == "ratio_before_wd":
                gv = fma32(wd, pv, r32(gv * ratio))
            else:
                gv = r32(fma32(wd, pv, gv) * ratio)
        bu = fma32(mu, mom[b:e], gv)
        mom[b:e] = bu
        p[b:e] = cfma32(-lr, bu, pv)
    return p, mom, torch.tensor(norms, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ column kernels
COL_FAMILIES = ("randn", "big_mean", "constant_column", "lattice")


def col_inputs(family, rows, c, seed, bf16=False):
    """x [rows, c] float32 (bf16-representable when asked).  randn: column j has spread 0.5 + j % 4 and mean j % 3 - 1;
    big_mean: columns of mean 300 and spread 1; constant_column: every
    second column constant (3, -0.7, 300 in turn), the others randn; lattice: small integers (exact in bf16; with rows a power
    of two the mean and the biased variance are exact in float32)."""
    g_ = _gen(seed)
    if family == "lattice":
        x = torch.randint(-4, 5, (rows, c), generator=g_).float()
    else:
        j = torch.arange(c)
        x = torch.randn(rows, c, generator=g_) * (0.5 + j % 4) + (j % 3 - 1.0)
    if family == "big_mean":
        x = torch.randn(rows, c, generator=g_) + 300.0
    if family == "constant_column":
        consts = torch.tensor([3.0, -0.7, 300.0])
        for j in range(0, c, 2):
            x[:, j] = consts[(j // 2) % 3]
    return x.bfloat16().float() if bf16 else x


def colstats_rpb(rows):
    """launch_colstats: rows per block"""
    return max(64, (rows + 255) // 256)


def colstats_ref(x, seed_error=None):
    """mean and biased variance per column in float64"""
    v = d64(x)
    mean = v.mean(0)
    return mean, (v - mean).pow(2).mean(0)


def _lane_colsum32(v, rows_total, rpb, sq_of=None):
    """one pass of colstats_kernel: per block of rpb rows, eight row lanes add (x - mu [squared]) in row order, the lanes are
    added in order, divided by the row count, and the blocks' atomics arrive in block order"""
    acc = torch.zeros(v.shape[1], dtype=torch.float64)
    for r0 in range(0, v.shape[0], rpb):
        blk = v[r0:r0 + rpb]
        lanes = torch.zeros(8, v.shape[1], dtype=torch.float64)
        for r in range(0, blk.shape[0], 8):
            part = blk[r:r + 8]
            if sq_of is not None:
                d = r32(part - sq_of)
                lanes[:part.shape[0]] = cfma32(d, d, lanes[:part.shape[0]])
            else:
                lanes[:part.shape[0]] = r32(lanes[:part.shape[0]] + part)
        tot = torch.zeros(v.shape[1], dtype=torch.float64)
        for j in range(8):
            tot = r32(tot + lanes[j])
        acc = r32(acc + r32(tot / rows_total))
    return acc


def colstats_emul(x, seed_error=None):
    """wm_colstats -> (mean, var).  seed_error: "unbiased_var" (rows - 1), "var_about_zero" (the second pass without the mean)"""
    v = d64(x)
    rows = v.shape[0]
    rpb = colstats_rpb(rows)
    mean = _lane_colsum32(v, rows, rpb)
    about = torch.zeros_like(mean) if seed_error == "var_about_zero" else mean
    var = _lane_colsum32(v, max(rows - 1, 1) if seed_error == "unbiased_var" else rows, rpb, sq_of=about)
    return mean, var


def colstats_depth(rows):
    """additions on the longest path of a column's float32 mean: row-lane trips, the eight lanes, the blocks' atomics, the
    division"""
    rpb = colstats_rpb(rows)
    return -(-min(rpb, rows) // 8) + 8 + -(-rows // rpb) + 1


def colstats_blocks(rows):
    return -(-rows // colstats_rpb(rows))


def mean_floor(x):
    """Absolute term of the float32 column mean: one rounding at the largest |x|, times sqrt(blocks) -- the blocks' partial means
    arrive through `blocks` atomic additions at the size of the mean, in an order the test cannot know; their roundings add like
    a random walk, and the emulation's one order (which on a constant column adds exactly for many steps) is no bound for another"""
    return kc.f32_stat_floor(x) * math.sqrt(colstats_blocks(x.shape[0]))


def var_floor(x):
    """Absolute term of the float32 variance: one rounding at the largest squared deviation (times sqrt(blocks) as for the
    mean), plus delta^2 for the float32 mean's own error delta (mean((x - mu)^2) = var + (mu - mean)^2 exactly), delta <= depth
    roundings at the largest |x| -- what keeps a constant column, whose reference variance is exactly 0, judgeable."""
    v = d64(x)
    d2 = (v - v.mean(0)).pow(2)
    delta = colstats_depth(v.shape[0]) * 2.0 ** -24 * float(v.abs().max())
    return kc.f32_stat_floor(d2) * math.sqrt(colstats_blocks(v.shape[0])) + delta * delta


def scaled_floor(x, ref):
    """Absolute term of StandardScaler.transform's output: the mean's floor carried through the division by the smallest scale,
    plus one rounding at the largest output"""
    return mean_floor(x) / float(ref["scale"].min()) + kc.f32_stat_floor(ref["y"])


def colscale_dg_floor(x, dy, dg0):
    terms = d64(dy) * d64(x)
    if dg0 is not None:
        terms = torch.cat([terms, d64(dg0).unsqueeze(0)])
    return kc.f32_sum_floor(terms)


def mean_f32_floor(x, scale=1.0, sqrt_of=False):
    v = d64(x)
    v = torch.sqrt(f32c(scale) * v) if sqrt_of else v
    return kc.f32_sum_floor(v.reshape(-1, 1)) / v.numel()


def scaler_ref(x_fit, x=None):
    """numpy float64 restatement of sklearn.preprocessing.StandardScaler.fit (-> mean_, var_, scale_) and transform: biased
    variance; a feature whose variance is within the rounding error of the sums (var <= n eps var + (n mean eps)^2, eps of
    float64) keeps scale 1"""
    a = x_fit.detach().double().numpy()
    n = a.shape[0]
    mean, var = a.mean(0), a.var(0)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    var = np.where(constant, 0.0, var)
    out = {"mean": torch.from_numpy(mean), "var": torch.from_numpy(var), "scale": torch.from_numpy(scale)}
    if x is not None:
        out["y"] = torch.from_numpy((x.detach().double().numpy() - mean) / scale)
    return out


def standardize_emul(x, mean, inv_scale):
    """standardize_kernel: (x - mean[c]) * inv_scale[c]"""
    return r32(r32(d64(x) - d64(mean)) * d64(inv_scale))


def scaler_emul(x_fit, x, seed_error=None):
    """retrieval.StandardScaler.fit + transform: wm_colstats, the constant-feature rule with float32's eps, 1 / scale by torch
    in float32, wm_standardize.  seed_error "scale_not_inverse": the kernel is handed the scale, not its inverse"""
    mean, var = colstats_emul(x_fit)
    n = x_fit.shape[0]
    eps = float(torch.finfo(torch.float32).eps)
    bound = n * eps * var + (n * mean * eps) ** 2
    scale = torch.where(var <= bound, torch.ones_like(var), r32(torch.sqrt(var)))
    inv = scale if seed_error == "scale_not_inverse" else r32(1.0 / scale)
    return {"mean": mean, "var": var, "scale": scale, "y": standardize_emul(x, mean, inv)}


def center_ref(t, center, momentum):
    return momentum * d64(center) + (1.0 - momentum) * d64(t).mean(0)


def center_emul(t, center, momentum, seed_error=None):
    """dino_center_kernel: eight row lanes add the bf16 rows in order, the lanes in order, then
    momentum * center + (1.f - momentum) * tot / rows.  seed_error: "momentum_swapped", "sum_not_mean" (no division)"""
    v, c = d64(t), d64(center)
    rows = v.shape[0]
    lanes = torch.zeros(8, v.shape[1], dtype=torch.float64)
    for r in range(0, rows, 8):
        part = v[r:r + 8]
        lanes[:part.shape[0]] = r32(lanes[:part.shape[0]] + part)
    tot = torch.zeros(v.shape[1], dtype=torch.float64)
    for j in range(8):
        tot = r32(tot + lanes[j])
    m = f32c(momentum)
    om = float(r32(torch.tensor(1.0 - m, dtype=torch.float64)))
    if seed_error == "momentum_swapped":
        m, om = om, m
    new = r32(om * tot)
    if seed_error != "sum_not_mean":
        new = r32(new / rows)
    return cfma32(m, c, new)


def colscale_ref(x, g, dy=None, dg0=None):
    """y = x g[c]; dx = dy g[c]; dg[c] = sum_r dy x (+ dg0) in float64"""
    y = d64(x) * d64(g)
    if dy is None:
        return y, None, None
    dg = (d64(dy) * d64(x)).sum(0)
    return y, d64(dy) * d64(g), dg if dg0 is None else dg + d64(dg0)


def colscale_emul(x, g, dy=None, dg0=None, seed_error=None):
    """colscale_fwd_kernel / colscale_bwd_kernel: y and dx one float32 product rounded to bf16; dg one fmaf chain down the rows.
    seed_error: "dg_from_y" (the gain's gradient formed with the output instead of the input), "dx_without_g"."""
    xv, gv = d64(x), d64(g)
    y = kc.bf(r32(xv * gv))
    if dy is None:
        return y, None, None
    d = d64(dy)
    dx = d.clone() if seed_error == "dx_without_g" else kc.bf(r32(d * gv))
    other = y if seed_error == "dg_from_y" else xv
    acc = torch.zeros(xv.shape[1], dtype=torch.float64)
    for r in range(xv.shape[0]):
        acc = fma32(d[r], other[r], acc)
    return y, dx, acc if dg0 is None else r32(d64(dg0) + acc)


def mean_ref(x, scale=1.0, sqrt_of=False):
    v = d64(x)
    return (torch.sqrt(f32c(scale) * v) if sqrt_of else v).mean()


def mean_emul(x, scale=1.0, sqrt_of=False):
    """mean_kernel: 1024 threads add their strided elements in order, the fixed tree red[t] += red[t + o], / n"""
    v = d64(x)
    if sqrt_of:
        v = r32(torch.sqrt(r32(f32c(scale) * v)))
    n = v.numel()
    k = -(-n // 1024)
    pad = torch.zeros(k * 1024, dtype=torch.float64)
    pad[:n] = v
    acc = torch.zeros(1024, dtype=torch.float64)
    for row in pad.reshape(k, 1024):
        acc = r32(acc + row)
    w = 1024
    while w > 1:
        w //= 2
        acc = r32(acc[:w] + acc[w:2 * w])
    return r32(acc[0] / n)


# ------------------------------------------------------------------------------------------------ bf16 rounding, bit for bit
def bf16_bits(x, truncate=False):
    """[n] int64 in 0 .. 65535: the bf16 pattern of float32 x, round to nearest even (NaN kept NaN); truncate: the upper half"""
    u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    out = (u >> 16) if truncate else ((u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    out = torch.where(torch.isnan(x.float()), (u >> 16) | 0x40, out)
    return out & 0xFFFF


def torch_bf16_bits(x):
    return x.float().bfloat16().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def cast_specials(n=None):
    """float32 values around every bf16 rounding decision: each of the 65536 upper halves with the lower half 0x0000, 0x7FFF,
    0x8000 (the tie, above an even and above an odd pattern), 0x8001 and 0xFFFF -- +-0, +-inf, subnormals, NaNs, and the values that
    round up to inf among them.  Tiled / cut to n."""
    hi = torch.arange(65536, dtype=torch.int64).repeat_interleave(5) << 16
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64).repeat(65536)
    u = hi | lo
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
    x = u.view(torch.float32)
    if n is not None:
        x = x.repeat(-(-n // x.numel()))[:n]
    return x.clone()


def bf16_specials(n):
    """every bf16 pattern, tiled to n, as float32"""
    u = (torch.arange(65536, dtype=torch.int64) << 16)
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
    return u.view(torch.float32).repeat(-(-n // 65536))[:n].clone()


def same_bf16(bits, want):
    """bit equality, except that a NaN need only be a NaN"""
    nan_a = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)
    nan_b = ((want & 0x7F80) == 0x7F80) & ((want & 0x7F) != 0)
    return bool((nan_a == nan_b).all()) and bool((bits == want)[~nan_b].all())


def scale_bf16_bits(x, s, seed_error=None):
    """scale_bf16_kernel: the float32 product, rounded to bf16"""
    return bf16_bits((x.float() * torch.tensor(s, dtype=torch.float32)), truncate=seed_error == "truncate")


# ------------------------------------------------------------------------------------------------ chained steps (Python layer)
def chain(kind, params, grads_per_step, hypers_per_step, emulate, states=None, t0=0):
    """`len(grads_per_step)` steps of one optimiser over a list of parameters, in float64 (torch.optim / lars_ref) or with the
    emulation; hypers_per_step: one dict of keyword arguments per step.  -> (params, states) after the last step, and the
    parameters after every step."""
    ps = [d64(p).clone() for p in params]
    if states is None:
        states = [{"m": torch.zeros_like(p), "v": torch.zeros_like(p)} for p in ps]
    trail = []
    for s, (grads, h) in enumerate(zip(grads_per_step, hypers_per_step)):
        for i, g in enumerate(grads):
            st = states[i]
            if kind == "sgd":
                f = sgd_emul if emulate else sgd_ref
                ps[i], st["m"] = f(ps[i], g, st["m"], **h)
            elif kind in ("adamw", "adam"):
                f = adam_emul if emulate else adam_ref
                ps[i], st["m"], st["v"] = f(ps[i], g, st["m"], st["v"], t0 + s + 1, l2=kind == "adam", **h)
            else:
                f = lars_emul if emulate else lars_ref
                seg = torch.tensor([0, ps[i].numel()])
                q, mo, _ = f(ps[i].reshape(-1), g.reshape(-1), st["m"].reshape(-1), seg, **h)
                ps[i], st["m"] = q.reshape(ps[i].shape), mo.reshape(ps[i].shape)
        trail.append([p.clone() for p in ps])
    return ps, states, trail


def cosine_lrs(base_lr, warmup, total):
    """the learning rates utils.scheduler.CosineWarmupScheduler sets, one per step"""
    out = []
    for e in range(total):
        f = (e + 1) / warmup if e < warmup else 0.5 * (1.0 + math.cos(math.pi * (e - warmup) / (total - warmup)))
        out.append(base_lr * f)
    return out


# ------------------------------------------------------------------------------------------------ cases shared by both test files
ELEMENT_SIZES = (1, 63, 255, 256, 257)
STEP_TENSORS = {"sgd": ("p", "m", "update"), "adamw": ("p", "m", "v", "update"), "adam": ("p", "m", "v", "update")}
COL_ROWS, COL_C = (1, 2, 63, 64, 65, 513, 16385), (1, 31, 32, 33, 512)
CENTER_ROWS, CENTER_D = (1, 7, 8, 9, 1000), (8, 31, 32, 33, 2048)
COLSCALE_ROWS, COLSCALE_C = (1, 64, 300), (1, 255, 256, 257, 2048)
MEAN_N = (1, 1023, 1024, 1025, 100000)


def step_outputs(kind, x, h, t=1, emulate=False, seed_error=None):
    """one step of `kind` ("sgd", "adamw", "adam") on step_inputs x -> every tensor the kernel writes, and the update
    p_after - p_before in float64"""
    if kind == "sgd":
        f = sgd_emul if emulate else sgd_ref
        kw = {"seed_error": seed_error} if emulate else {}
        p, m = f(x["p"], x["g"], x["m"], **h, **kw)
        out = {"p": p, "m": m}
    else:
        f = adam_emul if emulate else adam_ref
        kw = {"seed_error": seed_error} if emulate else {}
        p, m, v = f(x["p"], x["g"], x["m"], x["v"], t, l2=kind == "adam", **h, **kw)
        out = {"p": p, "m": m, "v": v}
    out["update"] = out["p"] - d64(x["p"])
    return out


def step_floor(name, ref):
    """check32's absolute term for tensor `name` of a step: one float32 rounding at the tensor's largest magnitude
    (f32_cases.elem_floor); the update is a difference of stored parameters and is only good to one rounding of |p|"""
    return {"abs_floor": fc.elem_floor(ref["p" if name == "update" else name]), "floor_all": True}


def lars_outputs(a, h, emulate=False, seed_error=None):
    """wm_lars_step on a lars_arena -> p, mom (whole arenas), norms [n, 2], update"""
    f = lars_emul if emulate else lars_ref
    kw = {"seed_error": seed_error} if emulate else {}
    p, mom, norms = f(a["p"], a["g"], a["mom"], a["seg"], **h, **kw)
    return {"p": p, "m": mom, "norms": norms, "update": p - d64(a["p"])}


def lars_rel_norms(out, ref):
    """The squared norms as fractions of their float64 values, over the segments and both norms where that value is not 0
    -> ([k] float64, mask [n, 2]).  Every term of a squared norm is positive, so kernel_check.f32_sum_floor of a segment (one
    float32 rounding of the sum of magnitudes) is exactly 2^-24 of the norm itself: in this form one floor, LARS_NORM_FLOOR, serves
    all segments, and the yardstick is the emulation's worst over all of them, not ONE realisation of one sum -- the blocks'
    partial norms arrive through atomics in an order that changes from run to run (measured on one segment of 8193 elements:
    0.59 and 0.93 roundings of the sum in two runs of one process, against an emulation that happened to score 0.02), and no order
    can promise to stay within the one rounding a lucky yardstick leaves."""
    nz = ref["norms"] > 0
    return out["norms"][nz] / ref["norms"][nz], nz


LARS_NORM_FLOOR = 2.0 ** -24


def lars_step_floor(name, a, h, ref, b, e):
    """step_floor of tensor `name` on segment [b, e), plus one float32 rounding of the trust ratio at the largest scaled
    gradient: each squared norm is good to one rounding of its sum at best (LARS_NORM_FLOOR), the square roots halve that and
    the quotient |w| / (|g| + wd |w| + eps) adds the two halves, so the ratio -- hence every element of (g + wd w) ratio, the
    whole new term of the momentum buffer, and lr times it in p -- carries up to 2^-24 relative whatever the summation order."""
    kw = step_floor(name, {"p": ref["p"][b:e], "m": ref["m"][b:e]})
    if h["weight_decay"] != 0:
        gv = ref["m"][b:e] - h["momentum"] * d64(a["mom"][b:e])
        kw["abs_floor"] += 2.0 ** -24 * float(gv.abs().max()) * (1.0 if name == "m" else h["lr"])
    return kw
