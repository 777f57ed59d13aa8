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

The module also holds the emulations (attention, LayerNorm, bias / activation, Linear and the GELU MLP), each with
switches that seed one wrong computation, and the input families.  tests/test_kernel_check_cpu.py proves on the CPU
that every seeded error is rejected by `check` on these families; the GPU tests feed the kernels the same families.
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


def _flat64(t) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64).reshape(-1)


def scores(x, ref64, a=None) -> dict:
    """The four criteria of x against ref64.  `a`: absolute term of criterion 4."""
    x, r = _flat64(x), _flat64(ref64)
    assert x.shape == r.shape, (x.shape, r.shape)
    err = (x - r).abs()
    out = {}
    out["max |err| / max |ref|"] = float(err.max() / (r.abs().max() + 1e-300))
    out["relative RMS error"] = float(err.pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-300))
    out["1 - cosine"] = max(0.0, float(1.0 - (x @ r) / (x.norm() * r.norm() + 1e-300))) if float(r.norm()) > 0 else float(err.max() > 0)
    if a is not None:
        den = a + BF16_ULP * r.abs()
        frac = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                             torch.zeros_like(err)))
        out["max |err| / (a + ulp |ref|)"] = float(frac.max())
    return out


def _abs_term(emul, ref64) -> float:
    d = (_flat64(emul) - _flat64(ref64)).abs()
    k = max(1, min(d.numel(), int(math.ceil(0.999 * d.numel()))))
    return float(torch.kthvalue(d, k).values)


def verdict(got, ref64, emul, factor: float = FACTOR, abs_floor: float = 0.0):
    """[(criterion, measured, bound)] and whether `got` is finite; no assertion (the CPU proofs use this).
    abs_floor: a lower limit of criterion 4's absolute term (see f32_sum_floor)."""
    g = _flat64(got)
    finite = bool(torch.isfinite(g).all())
    a = max(_abs_term(emul, ref64), float(abs_floor))
    yard = scores(emul, ref64, a)

    def bound(k):
        if k == "1 - cosine":
            # 1 - cosine = (relative error)^2 / 2: a stated factor f > 2 on the amplitude (F32_SUM_FACTOR) is f^2 here;
            # 2^-48 is the resolution of the float64 dot product and norms the criterion itself is computed with
            return (factor if factor <= FACTOR else factor * factor) * yard[k] + 2.0 ** -48
        if k.startswith("max |err| / (a") and abs_floor > 0:
            # a >= one float32 rounding at the scale of the summed magnitudes: a score <= 1 is within that one rounding,
            # which no summation order can promise to beat (the row-order yardstick often adds few bf16 terms exactly)
            return max(factor * yard[k], 1.0)
        return factor * yard[k]

    if not finite:
        return [(k, math.inf, bound(k)) for k in yard], False
    mine = scores(g, ref64, a)
    return [(k, mine[k], bound(k)) for k in yard], True


def f32_sum_floor(terms) -> float:
    """Absolute term for criterion 4 of a float32 SUM over rows of `terms` [rows, ...]: one float32 rounding (2^-24) of
    the largest column's sum of magnitudes -- what a single addition of any summation order may commit.  Without it a
    column whose terms cancel to ~0 is judged against |ref| ~ 0, and a yardstick whose few bf16 terms happen to add
    exactly in row order (error 0) would demand exactness of every other order."""
    return float(2.0 ** -24 * terms.detach().double().abs().sum(0).max())


def passes(got, ref64, emul, factor: float = FACTOR) -> bool:
    rows, finite = verdict(got, ref64, emul, factor)
    return finite and all(m <= b for _, m, b in rows)


def check(got, ref64, emul, what: str, factor: float = FACTOR, abs_floor: float = 0.0) -> float:
    """Assert the four criteria (each logged through parity()); returns the worst measured / bound ratio."""
    rows, finite = verdict(got, ref64, emul, factor, abs_floor)
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
