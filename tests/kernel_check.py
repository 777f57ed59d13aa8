"""Comparison of a bf16 / float32 kernel result with a float64 reference, with a yardstick that is DERIVED, not copied
from a run: `check(got, ref64, emul, what)`.

`ref64` is the float64 result on the same bf16-rounded inputs.  `emul` is a CPU restatement of the same operation that
rounds to bf16 exactly where the kernel's own comments say it rounds (its output; the probabilities before the PV
product; the LayerNorm output before a fused GEMM; the un-fused gradient before a residual add; the staged GEMM
accumulator before the bias) and is float64 everywhere else -- or, for float32 outputs (dW, dbias, dgamma, dbeta,
lse), the plain float32 restatement.  Four criteria per tensor, and the bound of each is FACTOR x the value the
emulation itself scores against `ref64` on that very input:

  1. max |err| / max |ref|                         (outliers)
  2. RMS(err) / RMS(ref)                            (the bulk)
  3. 1 - cosine                                     (direction)
  4. max |err| / (a + r |ref|)                      (small elements count: r = one bf16 ulp = 2^-8, a = the 99.9th
                                                     percentile of |emul - ref64|)

FACTOR = 2 covers what the emulation does not model: float32 summation order, __expf / __frcp_rn / rsqrtf (a few float32
ulp, three orders below a bf16 rounding) and the fluctuation of a maximum over a different set of rounding events.  A
tensor that needs more is a finding; a call that passes a wider factor says next to it what was measured and why.

The module also holds the emulations (attention, LayerNorm, bias / activation, Linear, the GELU MLP, the convolutions
of csrc/conv.hip with their fused statistics and BatchNorm-backward epilogue, the BatchNorm entry points of csrc/bn.hip with
the launch arithmetic their block sums follow, the pooling of csrc/pool.hip), each with
switches that seed one wrong computation, and the input families.  tests/test_kernel_check_cpu.py proves on the CPU
that every seeded error is rejected by `check` on these families; the GPU tests feed the kernels the same families.
The loss kernels of csrc/embed.hip have theirs in the sibling tests/loss_cases.py, the float32 kernels of csrc/f32path.hip in
tests/f32_cases.py (check(..., ulp=2^-23), inputs drawn inside float32_inputs()), the ViT losses and the token plumbing of
the second half of csrc/transformer.hip (MSE / L1, DINO, soft cross-entropy, the mean-entropy regulariser, tokens_assemble,
patchify, row gather / scatter, argsort, the plain column sums, the small float32 matmul) in tests/vit_cases.py.
"""
import contextlib
import math

import numpy as np
import torch
from parity_log import parity

FACTOR = 2.0
# float32 SUMS over rows (dgamma, dbeta, dbias, dW): the whole error of such an output is summation-order noise, and the
# yardstick (float32 accumulation in row order) is ONE realisation of that noise, the kernel's blocked / atomic order
# another.  Criteria 1 and 4 compare the MAXIMUM of one realisation over C columns with the maximum of the other, and
# 1 - cosine is quadratic in the error (a factor 2 on it is 1.41 on the amplitude; verdict() squares a stated factor).  Measured against the factor-2
# bound: dgamma 1 - cosine up to 1.4x (mean-300 rows, 2 .. 1000 rows), dbeta criterion 4 up to 1.33x (1000 x 384), dW
# criterion 4 up to 1.14x (131 x 192 -> 768), all at relative errors of 1e-7 .. 1e-5.  Twice the usual factor for these
# tensors; a dropped block of 32 rows in 25216 moves dbeta by 1.3e-3 relative, three orders above this bound.
F32_SUM_FACTOR = 4.0
BF16_ULP = 2.0 ** -8


_JITTER = None


def bf(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even, through float32 as the kernels do), keep the dtype."""
    if _FLOAT32_INPUTS:  # see float32_inputs()
        return x.float().to(x.dtype)
    if _JITTER is not None:  # see jitter()
        x = x * (1.0 + 2.0 ** -20 * (2.0 * torch.rand(x.shape, generator=_JITTER, dtype=torch.float64) - 1.0)).to(x.dtype)
    return x.float().bfloat16().to(x.dtype)


@contextlib.contextmanager
def jitter(seed: int):
    """Inside the block every value is moved by up to 2^-20 relative (a few float32 ulp: another summation order, another
    exp) before bf() rounds it, so the rounding events differ from the emulation's: what an honest kernel looks like."""
    global _JITTER
    _JITTER = torch.Generator().manual_seed(seed)
    try:
        yield
    finally:
        _JITTER = None


_FLOAT32_INPUTS = False


@contextlib.contextmanager
def float32_inputs():
    """Inside the block bf() rounds to float32 instead: the input families (conv_inputs, attention_inputs, layer_norm_inputs,
    bn_forward_inputs, act_grid, ...) then hold full float32 values, what the float32 kernels of csrc/f32path.hip are fed
    (tests/f32_cases.py)."""
    global _FLOAT32_INPUTS
    _FLOAT32_INPUTS = True
    try:
        yield
    finally:
        _FLOAT32_INPUTS = False


def f32_round(t: torch.Tensor) -> torch.Tensor:
    """Round to float32 (nearest even), back in float64: one float32 operation of an emulation"""
    return t.float().double()


def _flat64(t) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64).reshape(-1)


def scores(x, ref64, a=None, ulp: float = BF16_ULP) -> dict:
    """The four criteria of x against ref64.  `a`: absolute term of criterion 4, `ulp`: its relative term (one ulp of the
    output's format: bf16 unless stated)."""
    x, r = _flat64(x), _flat64(ref64)
    assert x.shape == r.shape, (x.shape, r.shape)
    err = (x - r).abs()
    out = {}
    out["max |err| / max |ref|"] = float(err.max() / (r.abs().max() + 1e-300))
    out["relative RMS error"] = float(err.pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-300))
    out["1 - cosine"] = max(0.0, float(1.0 - (x @ r) / (x.norm() * r.norm() + 1e-300))) if float(r.norm()) > 0 else float(err.max() > 0)
    if ulp < BF16_ULP and float(r.norm()) > 0 and float(x.norm()) > 0:
        # a float32 output lies 1e-15 from its reference in 1 - cosine, below what the float64 dot product above resolves over
        # 1e5 elements: half the squared distance of the two unit vectors is the same quantity without the cancellation
        out["1 - cosine"] = float(0.5 * (x / x.norm() - r / r.norm()).pow(2).sum())
    if a is not None:
        den = a + ulp * r.abs()
        frac = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                             torch.zeros_like(err)))
        out["max |err| / (a + ulp |ref|)"] = float(frac.max())
    return out


def _abs_term(emul, ref64) -> float:
    d = (_flat64(emul) - _flat64(ref64)).abs()
    k = max(1, min(d.numel(), int(math.ceil(0.999 * d.numel()))))
    return float(torch.kthvalue(d, k).values)


def verdict(got, ref64, emul, factor: float = FACTOR, abs_floor: float = 0.0, floor_all: bool = False,
            floor_cosine: bool = False, ulp: float = BF16_ULP):
    """[(criterion, measured, bound)] and whether `got` is finite; no assertion (the CPU proofs use this).
    abs_floor: a lower limit of criterion 4's absolute term (see f32_sum_floor).
    floor_all (the float32 statistics of BatchNorm): criteria 1 and 2 are not asked to go below `factor` roundings of
    abs_floor either -- see f32_stat_floor.
    floor_cosine (the loss gradients, whose terms can cancel to zero as a whole: a collapsed batch, D = 1, a negative equal to
    the positive): neither is the direction.  `factor` roundings of abs_floor on each of n elements are an error of norm
    rho |ref| at the most, rho = factor abs_floor sqrt(n) / |ref|, and the angle it can turn the tensor by has sin <= rho:
    1 - cosine <= rho^2 for rho < 1, and nothing can be asked of the direction (2) where the floor exceeds the tensor."""
    g = _flat64(got)
    finite = bool(torch.isfinite(g).all())
    a = max(_abs_term(emul, ref64), float(abs_floor))
    yard = scores(emul, ref64, a, ulp)

    def bound(k):
        if k == "1 - cosine":
            # 1 - cosine = (relative error)^2 / 2: a stated factor f > 2 on the amplitude (F32_SUM_FACTOR) is f^2 here;
            # 2^-48 is the resolution of the float64 dot product and norms the criterion itself is computed with
            b = (factor if factor <= FACTOR else factor * factor) * yard[k] + 2.0 ** -48
            if floor_cosine and abs_floor > 0:
                r = _flat64(ref64)
                rho = factor * abs_floor * math.sqrt(r.numel()) / (float(r.norm()) + 1e-300)
                b = max(b, rho * rho if rho < 1.0 else 2.0)
            return b
        if k.startswith("max |err| / (a") and abs_floor > 0:
            # a >= one float32 rounding at the scale of the summed magnitudes: a score <= 1 is within that one rounding,
            # which no summation order can promise to beat (the row-order yardstick often adds few bf16 terms exactly)
            return max(factor * yard[k], 1.0)
        if floor_all and abs_floor > 0 and k != "1 - cosine":
            r = _flat64(ref64)
            scale = r.abs().max() if k.startswith("max |err| / max") else r.pow(2).mean().sqrt()
            return max(factor * yard[k], factor * abs_floor / (float(scale) + 1e-300))
        return factor * yard[k]

    if not finite:
        return [(k, math.inf, bound(k)) for k in yard], False
    mine = scores(g, ref64, a, ulp)
    return [(k, mine[k], bound(k)) for k in yard], True


def f32_sum_floor(terms) -> float:
    """Absolute term for criterion 4 of a float32 SUM over rows of `terms` [rows, ...]: one float32 rounding (2^-24) of
    the largest column's sum of magnitudes -- what a single addition of any summation order may commit.  Without it a
    column whose terms cancel to ~0 is judged against |ref| ~ 0, and a yardstick whose few bf16 terms happen to add
    exactly in row order (error 0) would demand exactness of every other order."""
    return float(2.0 ** -24 * terms.detach().double().abs().sum(0).max())


def f32_stat_floor(*magnitudes) -> float:
    """Absolute term for a float32 STATISTIC that is a short chain of float32 operations on sums (a mean, a running
    statistic after a few updates, a coefficient): one float32 rounding (2^-24) at the largest magnitude that enters it.
    With verdict(floor_all=True) criteria 1 and 2 accept `factor` such roundings: on two or three rows, or on one update
    rm' = (1 - momentum) rm + momentum mean, the float32 restatement often lands on the exact value (its score is 0, or a
    twentieth of an ulp), while a kernel that contracts the same expression into an fma, or adds its row lanes in another
    order, is one rounding away -- measured on the MI355X: running_mean at 5.3x the factor-4 bound of such a lucky
    yardstick (37 x 2048, G = 2), all of it one float32 ulp of the largest channel."""
    return float(2.0 ** -24 * max(float(torch.as_tensor(m).detach().double().abs().max()) for m in magnitudes))


def passes(got, ref64, emul, factor: float = FACTOR) -> bool:
    rows, finite = verdict(got, ref64, emul, factor)
    return finite and all(m <= b for _, m, b in rows)


def check(got, ref64, emul, what: str, factor: float = FACTOR, abs_floor: float = 0.0, floor_all: bool = False,
          floor_cosine: bool = False, ulp: float = BF16_ULP) -> float:
    """Assert the four criteria (each logged through parity()); returns the worst measured / bound ratio."""
    rows, finite = verdict(got, ref64, emul, factor, abs_floor, floor_all, floor_cosine, ulp)
    assert finite, f"{what}: result holds inf / nan"
    worst = 0.0
    failed = []
    for crit, m, b in rows:
        worst = max(worst, m / b if b > 0 else (0.0 if m == 0 else math.inf))
        try:
            parity(f"{what}: {crit}", m, b, note=f"bound = {factor:g} x the bf16 / float32 emulation's own score")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)
    return worst


# ------------------------------------------------------------------------------------------------ attention
def attention_ref(qkv, scale, dout=None, emulate=False, seed_error=None, chunk=64):
    """softmax(scale q k^T) v per (image, head) in float64.  qkv [B, S, 3, H, hd] (bf16-exact values), dout [B, S, H, hd].
    Returns (out [B, S, H, hd], lse [B, H, S], dqkv or None).

    emulate: round where csrc/attention.hip rounds -- the un-normalised probabilities exp(s - m) to bf16 before the PV
    product (the row sum l is taken from the unrounded ones), the output to bf16; backward: delta from the ROUNDED
    output, P to bf16 before dV = P^T dO, dS = P (dP - delta) scale to bf16 before dQ = dS K and dK = dS^T Q, the
    three gradients to bf16.
    seed_error: one deliberately wrong computation (tests/test_kernel_check_cpu.py): "pad6" (six padded key slots with
    logit 0 and value 0 join the softmax), "noscale" (softmax without the scale), "nodelta" (dS without delta),
    "lse_m" (lse = m without log l), "bwd_noscale" (the backward ignores the scale)."""
    b, s, _, h, hd = qkv.shape
    rnd = bf if emulate else (lambda t: t)
    outs, lses, grads = [], [], []
    for i in range(0, b, chunk):
        x = qkv[i:i + chunk].double()
        q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))            # [b, h, s, hd]
        sc = scale if seed_error != "noscale" else 1.0
        logits = (q @ k.transpose(-2, -1)) * sc
        m = logits.max(-1, keepdim=True).values
        if seed_error == "pad6":
            m = m.clamp_min(0.0)
        p = (logits - m).exp()
        l = p.sum(-1, keepdim=True)
        if seed_error == "pad6":
            l = l + 6.0 * (-m).exp()
        o = rnd((rnd(p) @ v) / l)
        lse = (m + (0.0 if seed_error == "lse_m" else l.log())).squeeze(-1)
        outs.append(o.transpose(1, 2))
        lses.append(lse)
        if dout is None:
            continue
        do = dout[i:i + chunk].double().transpose(1, 2)                      # [b, h, s, hd]
        bs = 1.0 if seed_error == "bwd_noscale" else sc
        pn = ((q @ k.transpose(-2, -1)) * bs - (lse.unsqueeze(-1) if not emulate else lse.float().double().unsqueeze(-1))).exp()
        delta = (do * o).sum(-1, keepdim=True)
        if seed_error == "nodelta":
            delta = torch.zeros_like(delta)
        ds = pn * (do @ v.transpose(-2, -1) - delta) * bs
        dv = rnd(rnd(pn).transpose(-2, -1) @ do)
        dq = rnd(rnd(ds) @ k)
        dk = rnd(rnd(ds).transpose(-2, -1) @ q)
        grads.append(torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4))     # [b, s, 3, h, hd]
    return torch.cat(outs), torch.cat(lses), (torch.cat(grads) if grads else None)


def attention_lse_f32(qkv, scale):
    """The float32 restatement of lse (float32 products and logsumexp): the yardstick of the float32 output."""
    x = qkv.float()
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)
    return torch.logsumexp((q @ k.transpose(-2, -1)) * torch.tensor(scale, dtype=torch.float32), -1)


ATTENTION_FAMILIES = ("randn", "peaked", "offset+80", "offset-80", "zero_query", "v_offset")


def attention_inputs(family, b, s, h, hd, seed, scale=None):
    """(qkv [B, S, 3, H, hd], dout [B, S, H, hd]) of bf16-exact float32 values.
    randn: unit normal.  peaked: q, k scaled so the logits have standard deviation ~16 (most probabilities lie below
    the bf16 resolution of the row maximum).  offset+80 / offset-80: a common vector c added to every key, with q = a
    multiple of c plus noise, so every logit of a row sits near +-80 (a missing max subtraction overflows or zeroes the
    row).  zero_query: query row 1 (or 0 when S = 1) of every head is zero (uniform probabilities).  v_offset: v = 50 +
    randn."""
    g = torch.Generator().manual_seed(seed)
    scale = hd ** -0.5 if scale is None else scale
    qkv = torch.randn(b, s, 3, h, hd, generator=g)
    dout = torch.randn(b, s, h, hd, generator=g)
    if family == "peaked":
        f = (16.0 / (scale * math.sqrt(hd))) ** 0.5
        qkv[:, :, 0] *= f
        qkv[:, :, 1] *= f
    elif family in ("offset+80", "offset-80"):
        # logit = scale (q . k) with q = u + n_q, k = +-t u + n_k, |u|^2 = hd: the common part is +-scale t hd = +-80
        u = torch.ones(hd)
        t = 80.0 / (scale * hd)
        sign = 1.0 if family == "offset+80" else -1.0
        qkv[:, :, 0] = qkv[:, :, 0] * 0.5 + u
        qkv[:, :, 1] = qkv[:, :, 1] * 0.5 + sign * t * u
    elif family == "zero_query":
        qkv[:, min(1, s - 1), 0] = 0.0
    elif family == "v_offset":
        qkv[:, :, 2] += 50.0
    elif family != "randn":
        raise ValueError(family)
    return bf(qkv), bf(dout)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layer_norm_ref(x, gamma, beta, eps, dy=None, dres=None, emulate=False, seed_error=None):
    """LayerNorm over the last dim in float64 -> (y, dx, dgamma, dbeta).  emulate: y rounded to bf16; dx rounded to bf16,
    and with a residual gradient `dres` rounded BEFORE the add and again after it (ln_bwd: "the un-fused chain rounds
    the LayerNorm gradient to bf16 before the add").  The parameter gradients stay float64 (layer_norm_param_grads_f32
    is their float32 yardstick).
    seed_error: "last8" (the last 8 columns left out of mean and variance), "eps0", "eps1e-5", "eps1e-3", "no_mean_dy"
    (dx without the mean-of-dy term)."""
    rnd = bf if emulate else (lambda t: t)
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    eps = {"eps0": 0.0, "eps1e-5": 1e-5, "eps1e-3": 1e-3}.get(seed_error, eps)
    xs = x[:, :-8] if seed_error == "last8" else x
    mu = xs.mean(-1, keepdim=True)
    var = (xs - mu).pow(2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = (x - mu) * rstd
    y = rnd(xh * gamma + beta)
    if dy is None:
        return y, None, None, None
    dy = dy.double()
    g = dy * gamma
    c1 = g.mean(-1, keepdim=True) if seed_error != "no_mean_dy" else 0.0
    c2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - c1 - xh * c2)
    dx = rnd(rnd(dx) + dres.double()) if dres is not None else rnd(dx)
    return y, dx, (dy * xh).sum(0), dy.sum(0)


def colsum_f32(t):
    """Column sums by plain float32 accumulation, one row after the other: the float32 restatement of a sum over rows
    (a Python loop: torch's own float32 sum / cumsum accumulate in double on the CPU, which would be a float64 yardstick
    in disguise).  A kernel that adds block partials is at least as accurate as this order."""
    a = t.detach().float().cpu().numpy()
    acc = np.zeros(a.shape[1:], dtype=np.float32)
    for row in a:
        acc += row
    return torch.from_numpy(acc)


def matmul_tn_f32(a, b):
    """a^T b for a [n, k], b [n, c] by float32 accumulation of the n outer products in row order (see colsum_f32)."""
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    tmp = np.empty_like(acc)
    for r in range(a.shape[0]):
        np.multiply(a[r][:, None], b[r][None, :], out=tmp)
        acc += tmp
    return torch.from_numpy(acc)


def layer_norm_param_grads_f32(x, dy, eps):
    """(dgamma, dbeta) in float32: float32 statistics, float32 products, rows added in order."""
    x, dy = x.float(), dy.float()
    c = x.shape[1]
    mu = (colsum_f32(x.t()) / c)[:, None]                      # (torch's own float32 mean accumulates in double)
    rstd = (colsum_f32((x - mu).pow(2).t()) / c + torch.tensor(eps, dtype=torch.float32)).rsqrt()[:, None]
    return colsum_f32(dy * ((x - mu) * rstd)), colsum_f32(dy)


LN_FAMILIES = ("randn", "tight", "mean300", "constant", "big_row")


def layer_norm_inputs(family, rows, c, seed):
    """(x, gamma, beta, dy, dres) of float32 values, x / dy / dres bf16-exact.
    randn: the inputs tests/test_gpu_vit.py::test_layer_norm uses (2 randn + 0.5).  tight: rows with spread 1e-3 around
    0.5 (eps decides the result).  mean300: mean 300, spread 1 (a one-pass variance cancels).  constant: every row
    constant (y = bf16(beta)).  big_row: randn with one row (the middle one) of magnitude 1e4."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(rows, c, generator=g)
    if family == "randn":
        x = n * 2 + 0.5
    elif family == "tight":
        # the bf16 grid is 2^-8 at 0.5: draw the spread on the grid 2^-9 below 0.5 (bf16-exact), a few steps wide
        x = 0.5 - torch.randint(0, 4, (rows, c), generator=g).float() * 2.0 ** -9
    elif family == "mean300":
        x = 300.0 + n
    elif family == "constant":
        x = (torch.randint(-3, 4, (rows, 1), generator=g).float() * 0.75 + 0.5).expand(rows, c).clone()
    elif family == "big_row":
        x = n * 2 + 0.5
        x[rows // 2] *= 1e4
    else:
        raise ValueError(family)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    dy, dres = torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)
    return bf(x), gamma, beta, bf(dy), bf(dres)


# ------------------------------------------------------------------------------------------------ bias / activation
def _act64(v, act):
    if act == 1:
        return v * 0.5 * torch.erfc(-v / math.sqrt(2.0))      # (erfc: no cancellation in the negative tail)
    if act == 2:
        return v.clamp_min(0.0)
    if act == 3:
        return v * torch.tanh(torch.nn.functional.softplus(v, threshold=1e9))
    return v


def _act_grad64(v, act):
    if act == 1:
        return 0.5 * torch.erfc(-v / math.sqrt(2.0)) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    if act == 2:
        return (v > 0).double()                                  # 0 at exactly 0, as torch
    if act == 3:
        t = torch.tanh(torch.nn.functional.softplus(v, threshold=1e9))
        return t + v * torch.sigmoid(v) * (1.0 - t * t)
    return torch.ones_like(v)


def bias_act_ref(x, bias, act, res=None, dy=None, emulate=False, seed_error=None):
    """act(x + bias) (+ res) in float64 -> (y, dx, dbias).  emulate: y and dx rounded to bf16, dbias summed from the
    ROUNDED dx (colsum_kernel: "the sums see the rounded gradient").  seed_error "rows-1": dbias over all rows but the last."""
    rnd = bf if emulate else (lambda t: t)
    v = x.double() + (bias.double() if bias is not None else 0.0)
    y = _act64(v, act)
    if res is not None:
        y = y + res.double()
    y = rnd(y)
    if dy is None:
        return y, None, None
    dx = rnd(dy.double() * _act_grad64(v, act))
    src = dx[:-1] if seed_error == "rows-1" else dx
    return y, dx, src.sum(0)


def act_grid(rows, c, seed):
    """[rows, c] bf16-exact inputs: a grid over [-12, 12] with exact 0 and the bf16 neighbours of 0 (the smallest
    normal bf16 values of either sign), followed by 1.5 randn rows."""
    g = torch.Generator().manual_seed(seed)
    n = rows * c
    grid = torch.linspace(-12.0, 12.0, n // 2)
    tiny = 2.0 ** -126
    special = torch.tensor([0.0, -0.0, tiny, -tiny, 2.0 ** -100, -2.0 ** -100, 12.0, -12.0])
    rest = torch.randn(n - grid.numel() - special.numel(), generator=g) * 1.5
    return bf(torch.cat([special, grid, rest]).reshape(rows, c))


# ------------------------------------------------------------------------------------------------ Linear / MLP
def linear_ref(x, w, bias=None, res=None, dy=None, emulate=False):
    """x W^T + bias (+ res) in float64 -> (y, dx, dW, dbias).  emulate: the GEMM stages its accumulator as bf16, adds the
    bias and rounds, adds the residual and rounds (conv.hip epilogue); dx = bf16(dy W).  dW / dbias stay float64."""
    rnd = bf if emulate else (lambda t: t)
    x, w = x.double(), w.double()
    y = rnd(x @ w.t())
    if bias is not None:
        y = rnd(y + bias.double())
    if res is not None:
        y = rnd(y + res.double())
    if dy is None:
        return y, None, None, None
    dy = dy.double()
    return y, rnd(dy @ w), dy.t() @ x, dy.sum(0)


def linear_param_grads_f32(x, dy):
    """(dW, dbias) by float32 accumulation in row order: the yardstick of the float32 weight / bias gradients."""
    return matmul_tn_f32(dy, x), colsum_f32(dy)


def mlp_ref(x, w1, b1, w2, b2, res=None, dy=None, emulate=False, ln=None):
    """fc2(gelu(fc1(x))) (+ res), optionally behind a LayerNorm (ln = (gamma, beta, eps)), float64 ->
    dict(y, pre, dx, dw1, db1, dw2, db2).  emulate: LN output, staged accumulators, pre-activation, hidden activation,
    dpre and every bf16 output rounded where mlp.hip / conv.hip round them."""
    rnd = bf if emulate else (lambda t: t)
    xin = x.double()
    if ln is not None:
        xin = layer_norm_ref(x, ln[0], ln[1], ln[2], emulate=emulate)[0]
    w1, w2 = w1.double(), w2.double()
    pre = rnd(rnd(xin @ w1.t()) + b1.double())
    hid = rnd(_act64(pre, 1))
    y = rnd(rnd(hid @ w2.t()) + b2.double())
    if res is not None:
        y = rnd(y + res.double())
    out = {"y": y, "pre": pre}
    if dy is not None:
        dy = dy.double()
        dpre = rnd(rnd(dy @ w2) * _act_grad64(pre, 1))
        out.update(dx=rnd(dpre @ w1), dw1=dpre.t() @ xin, db1=dpre.sum(0), dw2=dy.t() @ hid, db2=dy.sum(0), dpre=dpre,
                   hid=hid)
    return out


# ------------------------------------------------------------------------------------------------ convolution
# Layouts are the kernels' own: x [N, H, W, C], w [K, R, S, C], y / dy [N, P, Q, K], dW [K, R, S, C]; "rows" are pixels
# in (n, h, w) order.  Everything is an im2col product in float64; tests/test_kernel_check_cpu.py holds it against
# torch's own conv2d and autograd.
def route_igemm(bn, cpt, mode, epi=False, bnb=False):
    """WM_ROUTE_IGEMM of include/wafer_hip.h (and the other codes below): what wm_conv2d_route answers"""
    return 10000 + (bn // 64) * 1000 + cpt * 100 + mode * 10 + (2 if epi else 0) + (1 if bnb else 0)


def route_wgrad(bmo, cpt, nt, bias=False):
    return 20000 + (bmo // 64) * 1000 + cpt * 100 + nt * 10 + (1 if bias else 0)


def route_patch(mode, bnb=False):
    return 10 + 2 * mode + (1 if bnb else 0)


ROUTE_PANEL, ROUTE_STEM_PATCH, ROUTE_WGRAD_PATCH64 = 1, 2, 3
ROUTE_F_STATS, ROUTE_F_RESIDUAL, ROUTE_F_BIAS, ROUTE_F_BNB, ROUTE_F_ACT = 1, 2, 4, 8, 16


def conv_out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def conv_gather(n, h, w, r, s, p, q, stride, pad, seed_error=None):
    """[N P Q, R S] long: the row of x (pixel index in (n, h, w) order) that tap (r, s) of an output pixel reads; -1 = the
    zero padding.  seed_error "wrap_border": a tap left or right of the image reads the flattened neighbour pixel (the
    end of the previous / start of the next image row) instead of zero; "image_bleed": a tap above row 0 of image n > 0
    reads the last rows of image n - 1."""
    ih = (torch.arange(p) * stride - pad).view(p, 1, 1, 1) + torch.arange(r).view(1, 1, r, 1)
    iw = (torch.arange(q) * stride - pad).view(1, q, 1, 1) + torch.arange(s).view(1, 1, 1, s)
    ih, iw = ih.expand(p, q, r, s), iw.expand(p, q, r, s)
    okh, okw = (ih >= 0) & (ih < h), (iw >= 0) & (iw < w)
    flat = ih * w + iw
    g = (torch.arange(n) * (h * w)).view(n, 1, 1, 1, 1) + flat.unsqueeze(0)
    ok = (okh & okw).unsqueeze(0).expand_as(g)
    if seed_error == "wrap_border":
        ok = (okh & (okw | ((flat >= 0) & (flat < h * w)))).unsqueeze(0).expand_as(g)
    elif seed_error == "image_bleed":
        ok = ok | (((ih < 0) & okw).unsqueeze(0) & (g >= 0))
    return torch.where(ok, g, torch.full_like(g, -1)).reshape(n * p * q, r * s)


def conv_im2col(x_rows, idx):
    """[M, R S C] float64: the gathered operand of the implicit GEMM (zero where idx is -1)"""
    z = torch.cat([x_rows.double(), torch.zeros(1, x_rows.shape[1], dtype=torch.float64)])
    return z[idx].reshape(idx.shape[0], -1)


def row_tiles(rows, size=128):
    """Statistics tiles of conv_igemm: runs of 128 rows (a ragged last run is no tile: statistics need whole tiles)"""
    return [torch.arange(t * size, (t + 1) * size) for t in range(rows // size)]


def pair_tiles(n, h, w):
    """... of the tile-pair kernels: pair b = the 8 x 8 tiles 2 b and 2 b + 1 in (image, tile row, tile column) order,
    rows tile * 64 + ty * 8 + tx (conv3x3_patch: pair_pixel)"""
    th, tw = h // 8, w // 8
    org = [(i * h + a * 8) * w + b * 8 for i in range(n) for a in range(th) for b in range(tw)]
    inner = (torch.arange(8).view(8, 1) * w + torch.arange(8).view(1, 8)).reshape(-1)
    return [torch.cat([org[2 * b] + inner, org[2 * b + 1] + inner]) for b in range(len(org) // 2)]


def stem_tiles(n, h, w, groups, slots):
    """... of conv_stem_patch: one launch per group, block b of min(pairs, slots) blocks sums over the pairs b, b + blocks, ...
    of its group and owns slot b"""
    pairs = pair_tiles(n, h, w)
    per = len(pairs) // groups
    out = []
    for g in range(groups):
        blocks = min(per, slots)
        out += [torch.cat(pairs[g * per + b:(g + 1) * per:blocks]) for b in range(blocks)]
    return out


def class_tiles(n, h, w, groups):
    """... of the MODE 2 input gradient: dx pixels ordered by parity class pc = 2 (h & 1) + (w & 1), inside a class in (n, h / 2,
    w / 2) order; a group's slots run class by class (conv_igemm: stat_slot(a, m0 - pc * cls, pc * (stat_rpg / BM)))"""
    nn, hh, ww = torch.meshgrid(torch.arange(n), torch.arange(h // 2), torch.arange(w // 2), indexing="ij")
    cls = [((nn * h + 2 * hh + ph) * w + 2 * ww + pw).reshape(-1) for ph in (0, 1) for pw in (0, 1)]
    rpg = cls[0].numel() // groups
    return [c[g * rpg + t * 128:g * rpg + (t + 1) * 128] for g in range(groups) for c in cls for t in range(rpg // 128)]


def tile_sums(vals, tiles):
    """[T, C] float64 column sums of vals [rows, C] over each tile's rows"""
    v = vals.double()
    return torch.stack([v[t].sum(0) for t in tiles]) if tiles else v.new_zeros(0, v.shape[1])


def tile_sums_f32(vals, tiles):
    """the float32 row-order restatement of tile_sums (colsum_f32 per tile): yardstick of the float32 slots"""
    v = vals.float()
    return torch.stack([colsum_f32(v[t]) for t in tiles])


def _mm(a, b, chunk=16384):
    return torch.cat([a[i:i + chunk] @ b for i in range(0, a.shape[0], chunk)])


def conv_ref(x, w, stride, pad, dy=None, res=None, dres=None, emulate=False, seed_error=None, out_hw=None, tiles=None):
    """Convolution in float64 -> dict(y, dx, dw, stats [T, 2, K], and the pieces the float32 yardsticks need: cols [M, R S C],
    y_acc / dx_acc, the unrounded accumulators as rows).  res: added to y, dres: a shortcut gradient added to dx.
    out_hw: (P, Q) where the caller crops the output (the space-to-depth stem: P = H with pad 2, R 4).
    tiles: the rows of every statistics slot (row_tiles / pair_tiles / stem_tiles); default row_tiles.

    emulate: rounds where csrc/conv.hip does --
      * the accumulator tile is staged as bf16 (stage_acc_frag: pack_bf2 of every accumulator), y / dx are that;
      * a residual / shortcut gradient is added to the ROUNDED tile and the sum rounded again (bf16x8_add in the store
        loops of conv_igemm and conv3x3_patch);
      * the statistics are the sums of the ROUNDED outputs (store_tile_with_stats reads the staged bf16 tile).
    dw and stats stay float64 (the float32 restatements: matmul_tn_f32(dy rows, cols), tile_sums_f32).

    seed_error (tests/test_kernel_check_cpu.py): "wrap_border", "image_bleed" (conv_gather; the input gradient is the
    adjoint of the same wrong gather, the weight gradient uses it); "tap_transpose" (r and s of the weights swapped);
    "drop_tail" (the last M mod 128 rows of y and of dx keep their previous content, 0; the weight gradient leaves out
    the last partial 64-pixel chunk); "one_class_missing" (stride-2 dx without the parity class (1, 1));
    "res_unrounded" (residual added before the rounding); "stats_unrounded" (statistics of the accumulators)."""
    n, h, wd, c = x.shape
    k, r, s, _ = w.shape
    p, q = out_hw if out_hw is not None else conv_out_hw(h, wd, r, s, stride, pad)
    rnd = bf if emulate else (lambda t: t)
    ws = w.transpose(1, 2) if seed_error == "tap_transpose" else w
    wm = ws.double().reshape(k, r * s * c)
    idx = conv_gather(n, h, wd, r, s, p, q, stride, pad, seed_error)
    cols = conv_im2col(x.reshape(-1, c), idx)
    m = n * p * q
    acc = _mm(cols, wm.t())
    if seed_error == "drop_tail":
        acc[m - m % 128:] = 0.0
    y = rnd(acc)
    src = acc if seed_error == "stats_unrounded" else y
    if res is not None:
        rr = res.double().reshape(m, k)
        y = rnd(acc + rr) if seed_error == "res_unrounded" else rnd(y + rr)
    tiles = row_tiles(m) if tiles is None else tiles
    out = {"y": y.reshape(n, p, q, k), "y_acc": acc, "cols": cols,
           "stats": torch.stack([tile_sums(src, tiles), tile_sums(src * src, tiles)], 1)}
    if dy is None:
        return out
    dyr = dy.double().reshape(m, k)
    mx = n * h * wd
    d = _mm(dyr, wm).reshape(m * r * s, c)
    fi = idx.reshape(-1)
    dacc = torch.zeros(mx + 1, c, dtype=torch.float64).index_add_(0, torch.where(fi >= 0, fi, torch.full_like(fi, mx)), d)[:mx]
    if seed_error == "one_class_missing":
        dacc.view(n, h, wd, c)[:, 1::2, 1::2] = 0.0
    if seed_error == "drop_tail":
        dacc[mx - mx % 128:] = 0.0
    dx = rnd(dacc)
    if dres is not None:
        dr = dres.double().reshape(mx, c)
        dx = rnd(dacc + dr) if seed_error == "res_unrounded" else rnd(dx + dr)
    keep = m - m % 64 if seed_error == "drop_tail" else m
    dw = (dyr[:keep].t() @ cols[:keep]).reshape(k, r, s, c)
    if seed_error == "tap_transpose":
        dw = dw.transpose(1, 2)
    out.update(dx=dx.reshape(n, h, wd, c), dx_acc=dacc, dw=dw)
    return out


def bn_dgrad_epilogue_ref(dx_acc, res, bn_y, mean, invstd, gamma, beta, form, relu_x=None, mask=None, tiles=None,
                          emulate=False, seed_error=None):
    """The BatchNorm-backward epilogue of wm_conv2d_dgrad_bnstat in float64 on rows [rows, C]:
        g = (dgrad (+ residual)) * mask -> dx;  per tile (sum g, sum g (bn_y - mean)) per channel -> stats [T, 2, C]
    dx_acc: the unrounded input gradient (conv_ref "dx_acc"); mean / invstd [G, C] over G equal runs of images (= of rows).
    form "x": mask = relu_x > 0; "bits": bit c & 7 of mask[row, c >> 3]; "recompute": bn_y gamma invstd + beta - mean gamma
    invstd > 0.  tiles: rows of every slot (row_tiles, pair_tiles, class_tiles).
    emulate (bnb_epilogue): the staged bf16 gradient tile plus the residual in float32 WITHOUT a second rounding, masked;
    the sums are taken from that float32 value, dx is its bf16 rounding; the recomputed mask is fmaf(bn_y, scale, shift) > 0
    with the float32 scale = gamma invstd and shift = beta - mean scale of the BatchNorm forward.
    Returns dict(dx, stats, g [rows, C], gy [rows, C]: the summed terms).
    seed_error: "mask_off_by_channel" (the bit mask read one bit over), "stat_uncentred" (sum g bn_y)."""
    rows, c = dx_acc.shape
    groups = mean.shape[0]
    grp = torch.arange(rows) // (rows // groups)
    y = bn_y.double().reshape(rows, c)
    mu = mean.double()[grp]
    v = bf(dx_acc) if emulate else dx_acc.clone()
    if res is not None:
        v = (v.float() + res.reshape(rows, c).float()).double() if emulate else v + res.double().reshape(rows, c)
    if form == "x":
        keep = relu_x.reshape(rows, c) > 0
    elif form == "bits":
        e = torch.arange(c) & 7
        if seed_error == "mask_off_by_channel":
            e = (e + 1) & 7
        keep = ((mask.reshape(rows, c // 8).long()[:, torch.arange(c) >> 3] >> e) & 1) != 0
    elif emulate:
        sc = gamma.float() * invstd.float()
        sh = beta.float() - mean.float() * sc
        keep = (y * sc.double()[grp] + sh.double()[grp]).float() > 0    # (one rounding: fmaf)
    else:
        sc = gamma.double() * invstd.double()
        keep = y * sc[grp] + (beta.double() - mean.double() * sc)[grp] > 0
    g = v * keep
    gy = g * (y if seed_error == "stat_uncentred" else y - mu)
    tiles = row_tiles(rows) if tiles is None else tiles
    return {"dx": rnd_or(g, emulate), "stats": torch.stack([tile_sums(g, tiles), tile_sums(gy, tiles)], 1), "g": g, "gy": gy}


def rnd_or(t, emulate):
    return bf(t) if emulate else t


CONV_FAMILIES = ("lattice", "randn", "offset", "big_pixel")


def conv_inputs(family, n, h, w, c, k, r, s, p, q, seed):
    """dict(x [N, H, W, C], w [K, R, S, C], dy [N, P, Q, K], dres [N, H, W, C]) of bf16-exact float32 values.
    randn: unit normal activations, He-scaled weights.  offset: x = 8 + randn and dy = 8 + randn (every accumulator carries
    a large common term).  big_pixel: one pixel of x and of dy times 1e4.  lattice: x, dy, dres integers in -2 .. 2, weights
    in {-1, 0, 1} with about 96 non-zeros per output channel (and per input channel), every (tap, input channel) and every
    (tap, output channel) used: every product, every partial sum in any order and every rounded output is exact
    (lattice_exact asserts it), so kernel and float64 agree bit for bit."""
    g = torch.Generator().manual_seed(seed)
    if family == "lattice":
        x = torch.randint(-2, 3, (n, h, w, c), generator=g).float()
        dy = torch.randint(-2, 3, (n, p, q, k), generator=g).float()
        dres = torch.randint(-2, 3, (n, h, w, c), generator=g).float()
        dens = 1.0 if c == 3 else min(1.0, 96.0 / max(c * r * s, k * r * s))   # (the 3-channel stem: dense +-1)
        sign = torch.randint(0, 2, (k, r, s, c), generator=g).float() * 2 - 1
        wt = sign * (torch.rand(k, r, s, c, generator=g) < dens)
        # a (tap, channel) position no output (input) channel uses would hide that tap's address from the test
        for dim in (0, 3):
            dead = (wt != 0).sum(dim) == 0
            pick = torch.randint(0, wt.shape[dim], dead.shape, generator=g)
            fix = torch.zeros_like(wt).scatter_(dim, pick.unsqueeze(dim), 1.0) * dead.unsqueeze(dim)
            wt = torch.where(fix != 0, sign, wt)
        assert bool(((wt != 0).sum(0) > 0).all()) and bool(((wt != 0).sum(3) > 0).all())
        return {"x": x, "w": wt, "dy": dy, "dres": dres}
    x = torch.randn(n, h, w, c, generator=g)
    dy = torch.randn(n, p, q, k, generator=g)
    dres = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(k, r, s, c, generator=g) * (2.0 / (c * r * s)) ** 0.5
    if family == "offset":
        x, dy = x + 8.0, dy + 8.0
    elif family == "big_pixel":
        x[n // 2, h // 2, w // 2] *= 1e4
        dy[n // 2, p // 2, q // 2] *= 1e4
    elif family != "randn":
        raise ValueError(family)
    return {"x": bf(x), "w": bf(wt), "dy": bf(dy), "dres": bf(dres)}


def bn_inputs(family, rows, c, groups, seed):
    """Operands of the BatchNorm-backward epilogue: dict(bn_y, relu_x [rows, C] bf16-exact, mask [rows, C / 8] uint8,
    mean, invstd [G, C], gamma, beta [C]).
    lattice: bn_y integers in -2 .. 2, mean and beta integers, gamma and invstd powers of two.  offset: channel mean 50
    with spread 1 (|mean| >> std: an uncentred sum g bn_y cancels).  randn: bn_y is built FROM its pre-activation z,
    |z| >= 0.5, so that no pre-activation lies near zero and the recomputed mask does not hang on a rounding
    (bn_preact_margin asserts it on the float64 reference; nothing is excluded)."""
    g = torch.Generator().manual_seed(seed)
    relu_x = torch.randn(rows, c, generator=g)
    mask = torch.randint(0, 256, (rows, c // 8), generator=g, dtype=torch.uint8)
    grp = torch.arange(rows) // (rows // groups)
    if family == "lattice":
        mean = torch.randint(-2, 3, (groups, c), generator=g).float()
        beta = torch.randint(-2, 3, (c,), generator=g).float()
        gamma = 2.0 ** torch.randint(-1, 2, (c,), generator=g).float()
        invstd = 2.0 ** torch.randint(-1, 2, (groups, c), generator=g).float()
        bn_y = torch.randint(-2, 3, (rows, c), generator=g).float()
        # an integer pre-activation of exactly 0 is masked by both sides (0 > 0 is false): nothing hangs on a rounding
        relu_x = torch.randint(-2, 3, (rows, c), generator=g).float()
    elif family == "offset":
        mean = 50.0 + torch.randn(groups, c, generator=g)
        invstd, gamma, beta = torch.rand(groups, c, generator=g) + 0.5, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
        bn_y = bf(mean[grp] + torch.randn(rows, c, generator=g))
    else:
        mean, beta = torch.rand(groups, c, generator=g) * 0.6 - 0.3, torch.rand(c, generator=g) * 0.6 - 0.3
        invstd, gamma = torch.rand(groups, c, generator=g) * 0.5 + 0.75, torch.rand(c, generator=g) * 0.5 + 0.75
        z = torch.randn(rows, c, generator=g)
        z = torch.sign(z) * (0.5 + z.abs()).clamp_max(4.0)
        bn_y = bf(mean[grp] + (z - beta) / (gamma * invstd[grp]))
    return {"bn_y": bn_y, "relu_x": bf(relu_x), "mask": mask, "mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta}


def bn_preact_margin(b):
    """min over elements of |pre-activation| / (|bn_y scale| + |shift|) in float64: the recomputed mask is safe while this
    stays far above a bf16 ulp (2^-8)"""
    rows = b["bn_y"].shape[0]
    grp = torch.arange(rows) // (rows // b["mean"].shape[0])
    sc = (b["gamma"].double() * b["invstd"].double())[grp]
    sh = b["beta"].double() - b["mean"].double()[grp] * sc
    t = b["bn_y"].double() * sc
    return float(((t + sh).abs() / (t.abs() + sh.abs()).clamp_min(1e-300)).min())


def lattice_exact(out, f32_keys=("dw", "stats")):
    """Preconditions of the exact tier on a float64 result dict: every bf16 output equals its own bf16 rounding, every
    float32 output is an integer (or dyadic) sum below 2^24 in magnitude"""
    for key, t in out.items():
        if key in ("cols", "y_acc", "dx_acc", "g", "gy") or t is None or t.numel() == 0:
            continue
        if key in f32_keys:
            assert float(t.abs().max()) < 2.0 ** 24 and torch.equal(t, t.float().double()), key
        else:
            assert torch.equal(t, t.float().bfloat16().double()), f"{key}: not bf16-exact (max {float(t.abs().max())})"


def f32_sum_bound(vals, tiles):
    """(bound of sum, bound of sum of squares) [T, C]: what ANY order of float32 additions of a tile's n values (fmaf for the
    squares: one rounding per term) can miss the exact sums by -- gamma_(n-1) sum |v| and gamma_n sum v^2, gamma_j = j u /
    (1 - j u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Derived, not measured."""
    u = 2.0 ** -24
    v = vals.double()
    gam = lambda j: j * u / (1.0 - j * u)  # noqa: E731
    return (torch.stack([gam(len(t) - 1) * v[t].abs().sum(0) for t in tiles]),
            torch.stack([gam(len(t)) * (v[t] * v[t]).sum(0) for t in tiles]))


# ------------------------------------------------------------------------------------------------ BatchNorm (csrc/bn.hip)
# A tensor is rows [rows, C]; G equal runs of rows are the statistics groups.  The launch arithmetic of bn.hip, mirrored so
# that the emulation sums over the kernel's own blocks and the tests can assert which path a shape reaches:
BN_THREADS = 256
BN_STREAM_BLOCKS = 256 * 16          # stream_grid: blocks of the apply passes at the most
BN_SLOTS_DIRECT, BN_SLOTS_REDUCED = 512, 128


def bn_rpp(c):
    """row lanes of a bn_reduce block: BN_THREADS / (C / 8) threads-per-row, at least one"""
    return max(BN_THREADS // (c >> 3), 1)


def bn_reduce_blocks(rpg, c):
    return max(1, min(256, -(-rpg // (bn_rpp(c) * 16))))


def bn_block_rows(rpg, c):
    """[(first, last + 1)] rows of every bn_reduce block of a group (launch_reduce: ceil(rpg / nblk) rows each, clipped)"""
    nblk = bn_reduce_blocks(rpg, c)
    per = -(-rpg // nblk)
    return [(min(b * per, rpg), min((b + 1) * per, rpg)) for b in range(nblk)]


def bn_chunk_pow2(c):
    cpr = c >> 3
    return cpr > 0 and cpr & (cpr - 1) == 0 and BN_THREADS % cpr == 0


def bn_stream_grid(items):
    return max(1, min(BN_STREAM_BLOCKS, -(-items // BN_THREADS)))


def bn_prereduce_plan(t):
    """(R, output slots) of stats_prereduce for T > BN_SLOTS_DIRECT slots per group, else (1, T)"""
    if t <= BN_SLOTS_DIRECT:
        return 1, t
    r = 1
    while -(-t // r) > BN_SLOTS_REDUCED:
        r *= 2
    return r, -(-t // r)


def bn_wide(rows, c, groups):
    return 2048 < c <= 16384 and rows // groups <= 65536


def fma_colsum_f32(a, b):
    """sum over rows of a * b by acc = fmaf(a, b, acc) in float32, one row after the other (a bf16-exact, so the product is
    exact in float64 and the only rounding is the accumulator's)"""
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    acc = np.zeros(a.shape[1:], dtype=np.float32)
    for r in range(a.shape[0]):
        acc = (acc.astype(np.float64) + a[r] * b[r]).astype(np.float32)
    return torch.from_numpy(acc)


def _f32(t):
    return t.float().double()


def _slot_totals(slots, emulate):
    """[G, T, 2, C] float32-valued slots -> [G, 2, C] float64 totals; emulate: stats_prereduce's float32 sums of R consecutive
    slots first, then the finalize kernels' double accumulation"""
    s = slots.double()
    r, to = bn_prereduce_plan(s.shape[1])
    if emulate and r > 1:
        s = torch.stack([torch.stack([colsum_f32(s[g, o * r:(o + 1) * r].float()) for o in range(to)]) for g in range(s.shape[0])]).double()
    return s.sum(1)


def bn_forward_ref(y, residual, gamma, beta, groups, eps, momentum, relu, running=None, slots=None, group_count=None,
                   emulate=False, wide=False, seed_error=None):
    """Training BatchNorm forward on rows y [rows, C] (bf16-exact) in float64 -> dict(out, mean, invstd, scale, shift [G, C],
    running_mean, running_var [C] after the G updates, relu_mask = out > 0, sums [G, 2, C]).  gamma / beta may be None (1 / 0).
    slots [G, T, 2, C]: the partial sums (sum y, sum y^2) come from there instead of y (the from_stats and synchronised
    forms); group_count: the M the sums are divided by (default rows / G: y is the whole group).

    emulate restates the narrow path of bn.hip: per block of bn_block_rows float32 (sum y, fmaf sum y^2) in row order ->
    double totals -> mean = s / M, var = max(ss / M - mean^2, 0), float32 mean, invstd = 1 / sqrt(var + eps), scale = gamma
    invstd, shift = beta - mean scale -> out = bf16(relu(y scale + shift (+ residual))) with the float32 coefficients -> the
    mask from the STORED value -> the running statistics updated in float32 group after group with var M / (M - 1).
    wide: bn_col_fwd instead -- float32 row-order sum, mean = s / M, two-pass float32 variance sum fmaf(d, d), rsqrtf.
    seed_error: "biased_running_var", "eps_dropped", "groups_pooled" (one statistic for all groups), "running_from_last_group_only",
    "residual_after_relu", "var_over_m_minus_1" (the normalisation itself uses the unbiased variance), "mask_ge_zero"."""
    rows, c = y.shape
    rpg = rows // groups
    m_cnt = float(group_count if group_count is not None else rpg)
    y64 = y.double()
    ga = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64)
    be = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64)
    eps_used = 0.0 if seed_error == "eps_dropped" else float(np.float32(eps))
    yg = y64.reshape(groups, rpg, c)
    if seed_error == "groups_pooled" and slots is None:
        yg = y64.reshape(1, rows, c).expand(groups, rows, c)
        m_cnt = float(rows) if group_count is None else m_cnt * groups
    if slots is not None:
        tot = _slot_totals(slots, emulate)
        if seed_error == "groups_pooled":
            tot, m_cnt = tot.sum(0, keepdim=True).expand_as(tot), m_cnt * groups
        s, ss = tot[:, 0], tot[:, 1]
    elif emulate and not wide:
        blocks = bn_block_rows(yg.shape[1], c)
        s = torch.stack([sum(colsum_f32(g[a:b]).double() for a, b in blocks) for g in yg])
        ss = torch.stack([sum(colsum_f32(g[a:b] * g[a:b]).double() for a, b in blocks) for g in yg])
    else:
        s, ss = yg.sum(1), (yg * yg).sum(1)
    if emulate and wide:
        mean = torch.stack([colsum_f32(g) for g in yg]) / torch.tensor(m_cnt, dtype=torch.float32)
        var = torch.stack([_fma_sq_f32(g.float() - mu) for g, mu in zip(yg, mean)]) / torch.tensor(m_cnt, dtype=torch.float32)
        unb = var * torch.tensor(m_cnt, dtype=torch.float32) / torch.tensor(m_cnt - 1.0, dtype=torch.float32) if m_cnt > 1 else var
        if seed_error == "var_over_m_minus_1":
            var = unb
        invstd = _f32((var + torch.tensor(eps_used, dtype=torch.float32)).double().rsqrt())
        mean, var, unb = mean.double(), var.double(), unb.double()
    else:
        mean = s / m_cnt
        if slots is None and not emulate:
            var = (yg - mean.unsqueeze(1)).pow(2).sum(1) / m_cnt          # (two passes in float64)
        else:
            var = (ss / m_cnt - mean * mean).clamp_min(0.0)
        unb = var * m_cnt / (m_cnt - 1.0) if m_cnt > 1 else var
        if seed_error == "var_over_m_minus_1":
            var = unb
        invstd = (var + eps_used).rsqrt()
        if emulate:
            mean, invstd, unb = _f32(mean), _f32(invstd), _f32(unb)
    if seed_error == "biased_running_var":
        unb = _f32(var) if emulate else var
    scale = ga * invstd
    shift = be - mean * (_f32(scale) if emulate else scale)
    if emulate:
        scale, shift = _f32(scale), _f32(shift)
    grp = torch.arange(rows) // rpg
    v = y64 * scale[grp] + shift[grp]
    res = residual.double() if residual is not None else None
    if res is not None and seed_error != "residual_after_relu":
        v = v + res
    if relu:
        v = v.clamp_min(0.0)
    if res is not None and seed_error == "residual_after_relu":
        v = v + res
    out = bf(v) if emulate else v
    out = out + 0.0                                                          # (-0 -> +0 plays no role in > 0)
    mask = out >= 0 if seed_error == "mask_ge_zero" else out > 0
    result = {"out": out, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "relu_mask": mask,
              "sums": torch.stack([s, ss], 1)}
    if running is not None:
        rm, rv = running[0].double().clone(), running[1].double().clone()
        mom = float(np.float32(momentum))
        keep = float(np.float32(1.0) - np.float32(momentum)) if emulate else 1.0 - mom       # (the kernel's 1.f - momentum)
        for g in range(groups):
            if seed_error == "running_from_last_group_only" and g < groups - 1:
                continue
            rm, rv = keep * rm + mom * mean[g], keep * rv + mom * unb[g]
            if emulate:
                rm, rv = _f32(rm), _f32(rv)
        result.update(running_mean=rm, running_var=rv)
    return result


def _fma_sq_f32(d):
    """sum over rows of d^2 by q = fmaf(d, d, q) in float32 (d float32: the product is exact in float64)"""
    return fma_colsum_f32(d, d)


def bn_pack_mask(mask):
    """[rows, C] bool -> [rows, C / 8] uint8, bit e of byte (row, chunk) = channel 8 chunk + e (bn_apply's relu_mask)"""
    rows, c = mask.shape
    w = (2 ** torch.arange(8)).to(torch.int64)
    return (mask.reshape(rows, c // 8, 8).to(torch.int64) * w).sum(-1).to(torch.uint8)


def bn_eval_ref(y, residual, gamma, beta, running_mean, running_var, eps, relu, emulate=False):
    """Eval-mode BatchNorm in float64 -> dict(out, scale, shift); emulate: float32 invstd = 1 / sqrt(var + eps), scale and
    shift as bn_eval_params, one bf16 rounding of the output"""
    c = y.shape[1]
    ga = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64)
    be = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64)
    e = float(np.float32(eps))
    if emulate:
        invstd = _f32((running_var.float() + torch.tensor(e, dtype=torch.float32)).double().rsqrt())
        scale = _f32(ga * invstd)
        shift = _f32(be - _f32(running_mean.double() * scale))
    else:
        scale = ga * (running_var.double() + e).rsqrt()
        shift = be - running_mean.double() * scale
    v = y.double() * scale + shift
    if residual is not None:
        v = v + residual.double()
    if relu:
        v = v.clamp_min(0.0)
    return {"out": bf(v) if emulate else v, "scale": scale, "shift": shift}


def bn_backward_ref(y, dout, gamma, beta, mean, invstd, groups, out_relu=None, remask=False, group_count=None, want_dz=True,
                    fx_slots=None, totals=None, accumulate_into=None, emulate=False, wide=False, seed_error=None):
    """Training BatchNorm backward on rows [rows, C] in float64 -> dict(dy, dz, dgamma, dbeta, sums [G, 2, C], and pre: the
    values the exact tier needs to be float32-exact).
        dz = dout * mask;  s1 = sum dz, s2 = sum dz xhat per group, xhat = (y - mean) invstd
        dy = gamma invstd (dz - s1 / M - xhat s2 / M);  dgamma = sum over groups of s2, dbeta = ... of s1 (+ accumulate_into)
    mask: out_relu > 0, or (remask) the forward's own y scale + shift > 0, or none.  mean / invstd [G, C] are inputs (float32
    values).  fx_slots [G, T, 2, C]: the sums come from slots holding (sum g, sum g (y - mean)), dout is g (no mask).  totals
    [G, 2, C]: the all-reduced sums of the synchronised form, divided by group_count; dgamma / dbeta stay local.

    emulate: narrow path -- float32 block sums (bn_block_rows; s2 by fmaf with the float32 xhat) -> double totals, float32
    coefficients s1 / M, s2 / M, gamma invstd; the mask recomputed as bf16(fmaf(y, scale, shift)) > 0; dy one bf16 rounding.
    wide: bn_col_bwd -- float32 row-order sums, float32 c1 = s1 / M, c2 = s2 / M, dgamma summed over groups in float32.
    seed_error: "dz_unmasked", "xhat_uncentred", "s2_term_dropped", "mean_over_local_rows", "fx_unscaled", "accumulate_ignored",
    "mask_ge_zero"."""
    rows, c = y.shape
    rpg = rows // groups
    m_cnt = float(rpg if group_count is None or seed_error == "mean_over_local_rows" else group_count)
    grp = torch.arange(rows) // rpg
    y64, d = y.double(), dout.double()
    ga = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64)
    be = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64)
    mu, inv = mean.double(), invstd.double()
    sc = _f32(ga * inv) if emulate else ga * inv
    sh = _f32(be - _f32(mu * sc)) if emulate else be - mu * sc
    ge = seed_error == "mask_ge_zero"
    if seed_error == "dz_unmasked" or (out_relu is None and not remask):
        dz = d
    elif out_relu is not None:
        dz = d * ((out_relu.double() >= 0) if ge else (out_relu.double() > 0))
    else:
        pre = y64 * sc[grp] + sh[grp]
        pre = bf(pre.float().double()) if emulate else pre
        dz = d * ((pre >= 0) if ge else (pre > 0))
    cen = y64 if seed_error == "xhat_uncentred" else y64 - mu[grp]
    xh = cen * inv[grp]
    if emulate:
        xh = _f32(_f32(cen) * inv[grp])
    if fx_slots is not None:
        tot = _slot_totals(fx_slots, emulate)
        s1 = tot[:, 0]
        s2 = tot[:, 1] if seed_error == "fx_unscaled" else inv * tot[:, 1]
    elif emulate:
        dzg, xg = dz.reshape(groups, rpg, c), xh.reshape(groups, rpg, c)
        if wide:
            s1 = torch.stack([colsum_f32(g) for g in dzg]).double()
            s2 = torch.stack([fma_colsum_f32(g, x) for g, x in zip(dzg, xg)]).double()
        else:
            blocks = bn_block_rows(rpg, c)
            s1 = torch.stack([sum(colsum_f32(g[a:b]).double() for a, b in blocks) for g in dzg])
            s2 = torch.stack([sum(fma_colsum_f32(g[a:b], x[a:b]).double() for a, b in blocks) for g, x in zip(dzg, xg)])
    else:
        s1, s2 = dz.reshape(groups, rpg, c).sum(1), (dz * xh).reshape(groups, rpg, c).sum(1)
    sums = torch.stack([s1, s2], 1)
    if emulate and wide:
        dgamma, dbeta = colsum_f32(s2), colsum_f32(s1)
    else:
        dgamma, dbeta = s2.sum(0), s1.sum(0)
    if emulate:
        dgamma, dbeta, sums = _f32(dgamma), _f32(dbeta), _f32(sums)
    if accumulate_into is not None and seed_error != "accumulate_ignored":
        dgamma, dbeta = accumulate_into[0].double() + dgamma, accumulate_into[1].double() + dbeta
        if emulate:
            dgamma, dbeta = _f32(dgamma), _f32(dbeta)
    t1, t2 = (totals[:, 0].double(), totals[:, 1].double()) if totals is not None else (s1, s2)
    c1, c2 = t1 / m_cnt, t2 / m_cnt
    if emulate:
        c1, c2 = _f32(c1), _f32(c2)
    prod = xh * c2[grp]
    pre_dy = sc[grp] * (dz - c1[grp] - (0.0 if seed_error == "s2_term_dropped" else prod))
    return {"dy": bf(pre_dy) if emulate else pre_dy, "dz": dz if want_dz else None, "dgamma": dgamma, "dbeta": dbeta,
            "sums": sums, "pre": {"c1": c1, "c2": c2, "xhat c2": prod, "dy before rounding": pre_dy, "s1": s1, "s2": s2}}


def bn_lattice_exact(pre):
    """Precondition of the exact backward tier: every intermediate of the float64 result is a float32 value (24 bits), so a
    float32 kernel in any summation order, contracted or not, holds the same numbers"""
    for key, t in pre.items():
        assert torch.equal(t, t.float().double()), f"{key}: needs more than 24 bits"
        assert float(t.abs().max()) < 2.0 ** 24, key


BN_FORWARD_FAMILIES = ("lattice", "randn", "offset", "constant", "big_value")


def bn_forward_inputs(family, rows, c, groups, seed, offset=50.0):
    """dict(y, residual [rows, C] bf16-exact, gamma, beta [C], running_mean, running_var [C]) for the BatchNorm forward.
    lattice: every (group, channel) holds mean +- s on a shuffled half of its rows each (rows / G even), mean an integer
    that differs per group, s in {0.5, 1, 2}; gamma a power of two, beta and residual integers, the running statistics
    small dyadic numbers: with eps = 0 mean, invstd = 1 / s, scale, shift and out are exact in float32 in any order.
    randn: 2 randn + 0.5.  offset: channel mean `offset` with spread 1, the groups' means one apart.  constant: every third
    channel constant within a group (variance exactly 0: invstd = eps^-1/2, eps decides), the others randn.  big_value: randn
    with one element (first row of the middle group) times 1e4."""
    g = torch.Generator().manual_seed(seed)
    rpg = rows // groups
    grp = torch.arange(rows) // rpg
    if family == "lattice":
        assert rpg % 2 == 0, "the lattice needs an even number of rows per group"
        mean = torch.randint(-3, 4, (1, c), generator=g).float() + torch.arange(groups).float().view(groups, 1)
        s = 2.0 ** torch.randint(-1, 2, (groups, c), generator=g).float()
        sign = torch.stack([torch.stack([(torch.randperm(rpg, generator=g) % 2).float() * 2 - 1 for _ in range(min(c, 16))], 1)
                            for _ in range(groups)])                         # [G, rpg, 16]: 16 shuffles, cycled over the channels
        sign = sign.repeat(1, 1, -(-c // 16))[:, :, :c]
        y = (mean.view(groups, 1, c) + sign * s.view(groups, 1, c)).reshape(rows, c)
        return {"y": y, "residual": torch.randint(-2, 3, (rows, c), generator=g).float(),
                "gamma": 2.0 ** torch.randint(-1, 2, (c,), generator=g).float() * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1),
                "beta": torch.randint(-2, 3, (c,), generator=g).float(),
                "running_mean": torch.randint(-2, 3, (c,), generator=g).float() * 0.5,
                "running_var": torch.randint(1, 4, (c,), generator=g).float() * 0.5, "mean": mean, "s": s}
    n = torch.randn(rows, c, generator=g)
    if family == "randn":
        y = n * 2 + 0.5
    elif family == "offset":
        y = offset + grp.float().view(rows, 1) + n
    elif family == "constant":
        y = n * 2 + 0.5
        const = torch.randint(-3, 4, (groups, c), generator=g).float() * 0.75
        y[:, ::3] = const[grp][:, ::3]
    elif family == "big_value":
        # in the FIRST row of the middle group: a sequential float32 sum carries its rounding through every later addition.  (At
        # the end of a reduce block the row-order yardstick would commit none of it and ask the same of every other order.)
        y = n * 2 + 0.5
        y[(rows // 2) // rpg * rpg, c // 2] *= 1e4
    else:
        raise ValueError(family)
    return {"y": bf(y), "residual": bf(torch.randn(rows, c, generator=g)), "gamma": torch.rand(c, generator=g) + 0.5,
            "beta": torch.randn(c, generator=g) * 0.3, "running_mean": torch.randn(c, generator=g) * 0.1,
            "running_var": torch.rand(c, generator=g) + 0.5}


def bn_backward_inputs(family, rows, c, groups, seed):
    """bn_inputs plus the gradient dout [rows, C] (lattice: integers in -2 .. 2; else bf16 randn) and non-zero dgamma / dbeta
    to accumulate onto (lattice: integers)"""
    b = bn_inputs(family, rows, c, groups, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    if family == "lattice":
        b["dout"] = torch.randint(-2, 3, (rows, c), generator=g).float()
        b["acc"] = (torch.randint(-4, 5, (c,), generator=g).float(), torch.randint(-4, 5, (c,), generator=g).float())
    else:
        b["dout"] = bf(torch.randn(rows, c, generator=g))
        b["acc"] = (torch.randn(c, generator=g), torch.randn(c, generator=g))
    return b


def bn_row_slots(vals_a, vals_b, groups, t, seed):
    """Slots [G, T, 2, C] as a convolution epilogue leaves them: the float64 sums of (vals_a, vals_b) [rows, C] over a random
    partition of every group's rows into T runs, some of them empty (zeros), rounded to float32"""
    rows, c = vals_a.shape
    rpg = rows // groups
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(groups, t, 2, c, dtype=torch.float64)
    for gi in range(groups):
        cuts = torch.sort(torch.randint(0, rpg + 1, (t - 1,), generator=g)).values.tolist() if t > 1 else []
        edges = [0] + cuts + [rpg]
        for k in range(t):
            a, b = gi * rpg + edges[k], gi * rpg + edges[k + 1]
            out[gi, k, 0], out[gi, k, 1] = vals_a[a:b].double().sum(0), vals_b[a:b].double().sum(0)
    return out.float()


# ------------------------------------------------------------------------------------------------ pooling (csrc/pool.hip)
def pooled_side(s):
    return (s - 1) // 2 + 1


def scan_reference(t, y):
    """t, y [N][H][W][C] float (CPU): per window the maximum of t over its positions inside the image, the code kh * 3 + kw
    of the FIRST position in scan order that attains it, and y at that position."""
    n, h, w, c = t.shape
    p, q = pooled_side(h), pooled_side(w)
    tp = torch.full((n, h + 2, w + 2, c), float("-inf"))
    tp[:, 1:h + 1, 1:w + 1] = t
    yp = torch.zeros((n, h + 2, w + 2, c))
    yp[:, 1:h + 1, 1:w + 1] = y
    best = torch.full((n, p, q, c), float("-inf"))
    code = torch.zeros((n, p, q, c), dtype=torch.uint8)
    sel = torch.zeros((n, p, q, c))
    for kh in range(3):
        for kw in range(3):
            cand = tp[:, kh:kh + 2 * p - 1:2, kw:kw + 2 * q - 1:2]
            m = cand > best            # strict: the first maximum stays
            best = torch.where(m, cand, best)
            code = torch.where(m, torch.tensor(kh * 3 + kw, dtype=torch.uint8), code)
            sel = torch.where(m, yp[:, kh:kh + 2 * p - 1:2, kw:kw + 2 * q - 1:2], sel)
    return best, code, sel


def maxpool_ref(x, seed_error=None):
    """max_pool 3x3 / stride 2 / pad 1 of x [N, H, W, C] -> (y, idx): scan_reference.  seed_error "zero_pad": the padding
    counts as 0 (a window on the border never goes below 0); "last_max": the LAST of equal maxima is recorded."""
    if seed_error == "last_max":
        best, code, _ = scan_reference(x.flip(1, 2), x.flip(1, 2))
        h, w = x.shape[1:3]
        assert h % 2 == 1 and w % 2 == 1, "the flipped scan is the same set of windows only for odd H and W"
        return best.flip(1, 2), (8 - code.flip(1, 2).long()).to(torch.uint8)
    best, code, _ = scan_reference(x, x)
    if seed_error == "zero_pad":
        n, h, w, c = x.shape
        edge = torch.zeros(best.shape[1], best.shape[2], dtype=torch.bool)
        edge[0, :], edge[:, 0] = True, True
        if h % 2 == 0:
            pass                                                      # (the last window row ends inside the image)
        else:
            edge[-1, :] = True
        if w % 2 == 1:
            edge[:, -1] = True
        best = torch.where(edge.view(1, *edge.shape, 1), best.clamp_min(0.0), best)
    return best, code


def maxpool_bwd_ref(dy, idx, h, w):
    """The gradient of the pooling in float64: every window's dy [N, P, Q, C] goes to the position its code names"""
    n, p, q, c = dy.shape
    dx = torch.zeros(n, h + 2, w + 2, c, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dx[:, kh:kh + 2 * p - 1:2, kw:kw + 2 * q - 1:2] += dy.double() * (idx == kh * 3 + kw)
    return dx[:, 1:h + 1, 1:w + 1]


def gap_ref(x, emulate=False):
    """mean over HW of x [N, HW, C] in float64; emulate: gap_fwd's float32 row-order sum times float32(1 / HW), one bf16
    rounding"""
    n, hw, c = x.shape
    if not emulate:
        return x.double().mean(1)
    inv = np.float32(1.0) / np.float32(hw)
    s = torch.stack([colsum_f32(img) for img in x])
    return bf((s * torch.tensor(inv)).double())
