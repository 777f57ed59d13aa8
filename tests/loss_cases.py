"""The loss kernels of csrc/embed.hip restated on the CPU: one function per operation, written once and run in two
precisions.  `dt=torch.float64` is the reference; `dt=torch.float32` is the yardstick `emul` of tests/kernel_check.py:
the plain float32 restatement of the same formulae (these kernels are float32 throughout), rounded to bf16 exactly where
a kernel stores bf16 (l2norm_*<.., uint16_t>, center_columns).  Float32 sums go through numpy's float32 accumulation
(`_sum`), never through torch's float32 sum / mean / cumsum; `__expf` is modelled as the hardware computes it
(`_fast_exp`).  Every function carries switches that seed ONE wrong computation; tests/test_kernel_check_cpu.py proves that
each is rejected, and that every float64 reference agrees with torch autograd in double.

Also here: the launch arithmetic of embed.hip mirrored in Python (nx_fwd_rpw, nx_bwd_plan, the grid caps), so that a test
that claims a code path asserts that its shape reaches it; the input families; and the bound of a scalar loss that a
kernel accumulates with atomicAdd (scalar_bound)."""
import contextlib
import math

import kernel_check as kc
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                      # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ precision helpers
_REVERSED = False


@contextlib.contextmanager
def other_order():
    """Inside the block every float32 sum of the restatements (_sum, dots, fma_matmul_f32) runs over its terms in the
    REVERSE order: another realisation of the summation-order noise the bounds claim to admit -- what an honest kernel with
    another reduction tree looks like (tests/test_kernel_check_cpu.py).  float64 is not touched."""
    global _REVERSED
    _REVERSED = True
    try:
        yield
    finally:
        _REVERSED = False


def _sum(t, dim, keepdim=False):
    """sum over `dim` in t's own precision (float32: numpy accumulates float32 in float32)"""
    if t.dtype == F64:
        return t.sum(dim, keepdim=keepdim)
    if _REVERSED:
        t = t.flip(dim)
    return torch.from_numpy(np.asarray(np.add.reduce(t.contiguous().numpy(), axis=dim, dtype=np.float32, keepdims=keepdim)))


def dots(a, b):
    """a [n, d] . b [m, d] -> [n, m].  float32: one accumulator per dot, s = fmaf(a[i][c], b[j][c], s) for c in order, as
    dcl_rows_kernel computes its similarities -- at 1 / T = 10 .. 14 the rounding of a logit is that much relative error in
    exp(logit), so the chain of D roundings is what the softmax rows carry (a BLAS product blocks the sum)"""
    if a.dtype == F64:
        return a @ b.t()
    an, bn = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    acc = np.zeros((an.shape[0], bn.shape[0]), dtype=np.float32)
    cols = range(an.shape[1])
    for c in (reversed(cols) if _REVERSED else cols):
        acc = (acc + an[:, c:c + 1] * bn[:, c][None, :]).astype(np.float32)
    return torch.from_numpy(acc)


def _c(v, dt):
    """a host float as the kernel receives it: rounded to float32 (both precisions use THAT value)"""
    return torch.tensor(float(np.float32(v)), dtype=dt)


def _fast_exp(x):
    """__expf: v_exp_f32 of the float32 product x * log2(e) -- the rounding of that product is the whole modelled error
    (relative |x| 2^-24 in the result); float64 takes the exact exponential"""
    if x.dtype == F64:
        return x.exp()
    arg = x * torch.tensor(float(np.float32(1.4426950408889634)), dtype=F32)
    return torch.exp2(arg.double()).float()


def _store(t, dt, bf16):
    """what a kernel leaves in memory: bf16 rounding in the emulation when the kernel stores bf16"""
    return kc.bf(t) if (bf16 and dt == F32) else t


# ------------------------------------------------------------------------------------------------ launch arithmetic
NX_RT, NX_CT = 32, 64
BCE_CAP, BARLOW_CAP, CENTER_CAP, VICREG_CAP, SK_WRITE_CAP = 1024, 2048, 4096, 64, 2048
BANK_LDS_FLOATS = DCL_LDS_FLOATS = 16384


def cdiv(a, b):
    return -(-a // b)


def nx_fwd_rpw(b_local):
    """rows per wave of ntxent_fwd_kernel (wm_ntxent_fwd): 2 while 2 b_local <= 2048, else 8"""
    return 2 if 2 * b_local <= 2048 else 8


def nx_bwd_plan(b_local, b_global):
    """(rowtiles, nsplit, tiles_per_split) of wm_ntxent_bwd"""
    rowtiles = cdiv(2 * b_local, NX_RT)
    coltiles = cdiv(2 * b_global, NX_CT)
    nsplit = max(1, min(256 // rowtiles, coltiles))
    tps = cdiv(coltiles, nsplit)
    return rowtiles, cdiv(coltiles, tps), tps


def nx_bwd_lds_bytes(d):
    return (NX_RT * d + NX_CT * (d + 4) + NX_RT * (NX_CT + 1)) * 4


def grid_blocks(n, cap):
    """blocks of a 256-thread grid-stride kernel over n items with a cap"""
    return min(cap, cdiv(n, 256))


def grid_chain(n, cap):
    """the longest chain of float32 additions a term of such a kernel's scalar goes through: the thread's own
    grid-stride sum, 6 wave_sum steps, 3 additions of the wave partials, the block's atomicAdd among `blocks` of them"""
    blocks = grid_blocks(n, cap)
    return cdiv(n, blocks * 256) + 6 + 3 + blocks


def row_chain(per_lane, rows):
    """... of a one-wave-per-row (or one-block-per-row) kernel: the lane's sum, wave and block reduction, `rows` atomics"""
    return per_lane + 6 + 3 + rows


def scalar_bound(terms64, terms32, chain, mags=None):
    """Bound of |kernel scalar - float64 scalar| for a loss a kernel accumulates in float32 from `terms`:
        gamma_chain sum |t_i|                      any summation tree of height `chain` (Higham, Accuracy and Stability of
                                                   Numerical Algorithms, section 4.2: |E| <= gamma_h sum |x_i|)
      + sum_i max(F |t32_i - t64_i|, 4 u m_i)     the float32 error of the terms themselves: kernel_check.F32_SUM_FACTOR x
                                                   what the float32 restatement commits on that very term, and never less
                                                   than four roundings at the magnitude m_i that enters the term (default |t_i|)
      + u |sum|                                    the final rounding.
    Derived; nothing in it comes from a run of the kernel."""
    t64, t32 = terms64.double().reshape(-1), terms32.double().reshape(-1)
    m = t64.abs() if mags is None else mags.double().reshape(-1)
    gam = chain * U / (1.0 - chain * U)
    per_term = torch.maximum(kc.F32_SUM_FACTOR * (t32 - t64).abs(), 4.0 * U * m)
    return float(gam * t64.abs().sum() + per_term.sum() + U * t64.sum().abs())


def check_scalar(got, terms64, terms32, chain, what, mags=None):
    """assert the scalar bound (logged through parity()); returns measured / bound"""
    from parity_log import parity

    ref = float(terms64.double().sum())
    bound = scalar_bound(terms64, terms32, chain, mags)
    got = float(got)
    assert math.isfinite(got), f"{what}: {got}"
    parity(f"{what}: |loss - float64|", abs(got - ref), bound, note=f"Higham bound of a float32 sum of height {chain} + per-term float32 error")
    return abs(got - ref) / bound if bound > 0 else (0.0 if got == ref else math.inf)


def scalar_ok(got, terms64, terms32, chain, mags=None):
    return abs(float(got) - float(terms64.double().sum())) <= scalar_bound(terms64, terms32, chain, mags)


def f32_floor(*magnitudes):
    """absolute term of a float32 output: one float32 rounding at the largest magnitude that enters it (kernel_check.
    f32_stat_floor) -- the float32 restatement often lands on the exact value where another order of the same float32
    operations is one rounding away"""
    return kc.f32_stat_floor(*magnitudes)


def verdict_f32(got, ref64, emul, floor):
    """kernel_check.verdict for a float32 output: the yardstick is one realisation of float32 rounding noise, the kernel's
    order another (F32_SUM_FACTOR), and no criterion asks for less than a rounding at the operands' scale (floor_all)"""
    return kc.verdict(got, ref64, emul, kc.F32_SUM_FACTOR, floor, floor_all=True, floor_cosine=True)


def check_f32(got, ref64, emul, what, floor):
    return kc.check(got, ref64, emul, what, factor=kc.F32_SUM_FACTOR, abs_floor=floor, floor_all=True, floor_cosine=True)


def check_bf16(got, ref64, emul, what, floor=0.0):
    """a bf16 output: the emulation's bf16 roundings are the yardstick (factor 2); `floor`, where the float32 value that is
    rounded comes out of a cancellation"""
    return kc.check(got, ref64, emul, what, abs_floor=floor, floor_all=floor > 0, floor_cosine=floor > 0)


def mag_floor(*terms):
    """one float32 rounding at the largest sum of the magnitudes `terms` that make up an element: the floor of a gradient
    whose terms can cancel"""
    return float(U * sum(t.detach().double().abs() for t in terms).max())


def fma_matmul_f32(w, z, splits=None):
    """w [n, m] @ z [m, d] as the gradient kernels accumulate it: per output element ONE float32 accumulator,
    acc = fmaf(w[i][j], z[j][c], acc) for j in order (ntxent_bwd_kernel's `out`, dcl_grad_kernel's `g`) -- a chain of m
    roundings, where a BLAS product blocks the sum and is the more accurate for it.  splits [(first, last + 1)]: one
    accumulator per column split, the slabs then added in order (ntxent_bwd_reduce)."""
    wn, zn = w.detach().numpy().astype(np.float64), z.detach().numpy().astype(np.float64)
    total = None
    for a, b in (splits or [(0, wn.shape[1])]):
        acc = np.zeros((wn.shape[0], zn.shape[1]), dtype=np.float32)
        for j in (reversed(range(a, b)) if _REVERSED else range(a, b)):
            acc = (acc + wn[:, j:j + 1] * zn[j][None, :]).astype(np.float32)     # float32 x float32 is exact in float64: fmaf
        total = acc if total is None else (total + acc).astype(np.float32)
    return torch.from_numpy(total)


# ------------------------------------------------------------------------------------------------ L2 normalise
def l2norm(x, eps, dy=None, scale=1.0, dt=F64, y_bf16=False, dx_bf16=False, seed_error=None):
    """F.normalize(x, dim=1, eps) -> dict(y, inv_norm, dx).  x, dy: float32 or bf16-exact values.
    backward as torch's: dx = (dy - y <y, dy>) / |x| scale for |x| > eps, dy / eps scale for a clamped row (the clamp passes
    no gradient to the norm).  The backward reads the float32 y the forward saved (never the bf16 copy).
    seed_error "eps_added": x / (|x| + eps)."""
    v = x.to(dt)
    n = _sum(v * v, 1, True).sqrt()
    e = _c(eps, dt)
    denom = n + e if seed_error == "eps_added" else torch.maximum(n, e)
    yf = v / denom
    out = {"y": _store(yf, dt, y_bf16), "inv_norm": (1.0 / denom).reshape(-1), "norm": n.reshape(-1)}
    if dy is not None:
        g = dy.to(dt)
        dot = _sum(g * yf, 1, True)
        proj = torch.where(n > e, yf * dot, torch.zeros_like(yf))
        out["dx"] = _store((g - proj) * ((1.0 / denom) * _c(scale, dt)), dt, dx_bf16)
        out["dx_terms"] = (g.abs() + proj.abs()) * ((1.0 / denom) * _c(scale, dt))
    return out


def l2norm_inputs(rows, d, eps, seed, bf16_in=False, bf16_dy=False):
    """x = 3 randn with (rows permitting) row 0 zero and row 1 of norm 0.5 eps (well inside the clamp: the margin
    |norm / eps - 1| of every row is asserted by the tests); dy = randn"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * 3
    dy = torch.randn(rows, d, generator=g)
    if rows >= 3:
        x[0] = 0
        x[1] = x[1] / x[1].double().norm().float() * (0.5 * eps)
    return (kc.bf(x) if bf16_in else x), (kc.bf(dy) if bf16_dy else dy)


# ------------------------------------------------------------------------------------------------ NT-Xent
NTXENT_FAMILIES = ("randn", "duplicates", "collapsed", "antipodal", "offset")


def ntxent_inputs(family, b, d, seed):
    """(z0, z1) [b, d] raw projections (float32).  duplicates: rows 0 .. min(b, 5) - 1 of both views identical (the
    largest logit 1 / T sits among the negatives, with ties).  collapsed: every row equal (loss = log(2 b - 1)).
    antipodal: z1 = -z0.  offset: 5 + 0.1 randn (all cosines near 1)."""
    g = torch.Generator().manual_seed(seed)
    z0, z1 = torch.randn(b, d, generator=g), torch.randn(b, d, generator=g)
    if family == "duplicates":
        k = min(b, 5)
        z0[:k] = z0[0]
        z1[:k] = z0[0]
    elif family == "collapsed":
        z0 = z0[:1].expand(b, d).clone()
        z1 = z0.clone()
    elif family == "antipodal":
        z1 = -z0
    elif family == "offset":
        z0, z1 = 5 + 0.1 * z0, 5 + 0.1 * z1
    elif family != "randn":
        raise ValueError(family)
    return z0, z1


def normalized32(z):
    """float32 unit rows as wm_l2_normalize hands them to the NT-Xent kernels (the emulation's float32 values: both the
    reference and the kernel then see the SAME operand)"""
    return l2norm(z, 1e-12, dt=F32)["y"]


def _nx_ids(b_local, b_global, off):
    r = torch.arange(2 * b_local)
    v, i = r // b_local, r % b_local
    return v * b_global + off + i, (1 - v) * b_global + off + i


def _nx_lse(s, keep, dt, no_max=False):
    neg = torch.where(keep, s, torch.full_like(s, -math.inf))
    m = torch.zeros(s.shape[0], 1, dtype=dt) if no_max else neg.max(1, keepdim=True).values
    e = _fast_exp(neg - m)
    return (m + _sum(e, 1, True).log()).reshape(-1)


def ntxent(zn, zall, b_local, b_global, off, temp, grad_scale=None, dt=F64, seed_error=None):
    """NT-Xent on float32 unit rows zn [2 b_local, d] (view-major) against zall [2 b_global, d] -> dict(lse, loss_rows, dzn).
    Local row (v, i) is global row v b_global + off + i; its positive is the same index of the other view; itself is no
    negative.  dzn = grad_scale d(sum over ALL global rows of loss_row) / d zn -- row i enters as an anchor (weight
    exp(s_ij - lse_i)) and as a column of every other row j (weight exp(s_ij - lse_j)), and twice as a positive:
        dzn_i = grad_scale / T  sum_{j != i} (exp(s_ij - lse_i) + exp(s_ij - lse_j) - 2 [j = pos(i)]) zall_j
    The lse of the global rows is computed the same way from zall (the ranks' all-gather).
    seed_error: self_included, no_max, pos_at_rank0, drop_last_tile, drop_last_split, lse_row_only, temp_once."""
    z, za = zn.to(dt), zall.to(dt)
    nl, ng = 2 * b_local, 2 * b_global
    t = _c(temp, dt)
    s = (z @ za.t()) / t
    self_g, pos_g = _nx_ids(b_local, b_global, off)
    if seed_error == "pos_at_rank0":
        pos_g = _nx_ids(b_local, b_global, 0)[1]
    rows = torch.arange(nl)
    keep = torch.ones(nl, ng, dtype=torch.bool)
    if seed_error != "self_included":
        keep[rows, self_g] = False
    if seed_error == "drop_last_tile" and ng % NX_CT:
        keep[:, ng - ng % NX_CT:] = False
    lse = _nx_lse(s, keep, dt, no_max=seed_error == "no_max")
    out = {"lse": lse, "loss_rows": lse - s[rows, pos_g]}
    if grad_scale is None:
        return out
    if b_local == b_global:
        lse_all = lse
    else:
        sa = (za @ za.t()) / t
        ka = ~torch.eye(ng, dtype=torch.bool) if seed_error != "self_included" else torch.ones(ng, ng, dtype=torch.bool)
        lse_all = _nx_lse(sa, ka, dt)
        del sa, ka
    mv = _fast_exp(s - lse.unsqueeze(1))
    if seed_error != "lse_row_only":
        mv = mv + _fast_exp(s - lse_all.unsqueeze(0))
    mv = torch.where(keep, mv, torch.zeros_like(mv))
    mag = mv.abs().double()                  # the magnitudes that enter an element, before the positive's 2 cancels any
    mag[rows, pos_g] += 2.0
    mv[rows, pos_g] -= 2.0
    if seed_error == "drop_last_split":
        _, nsplit, tps = nx_bwd_plan(b_local, b_global)
        if nsplit > 1:
            mv[:, (nsplit - 1) * tps * NX_CT:] = 0.0
    sc = _c(grad_scale, dt) if seed_error == "temp_once" else _c(grad_scale, dt) / t
    if dt == F32:
        _, nsplit, tps = nx_bwd_plan(b_local, b_global)
        out["dzn"] = fma_matmul_f32(mv, za, [(sp * tps * NX_CT, min(ng, (sp + 1) * tps * NX_CT)) for sp in range(nsplit)]) * sc
    else:
        out["dzn"] = (mv @ za) * sc
    out["dzn_floor"] = float(U * ((mag @ za.abs().double()) * float(sc)).max())
    return out


def ntxent_lse_floor(temp, ref):
    """absolute term of lse / loss_rows: one float32 rounding at the magnitude of what both are made of, the logits (up to
    1 / T) and the lse itself"""
    return f32_floor(ref["lse"], 1.0 / temp)


# ------------------------------------------------------------------------------------------------ MoCo bank
def bank_loss(q, k, bank, temp, dt=F64, seed_error=None):
    """NT-Xent against a bank [D, K]: logits [<q_i, k_i>, q_i . bank] / T, label 0 -> dict(terms [B] (their sum is the
    loss), dq, dk, mags).  seed_error "pos_not_in_lse": the log-sum-exp runs over the bank columns only."""
    qq, kk, bk = q.to(dt), k.to(dt), bank.to(dt)
    b = q.shape[0]
    it = _c(1.0, dt) / _c(temp, dt)
    s0 = _sum(qq * kk, 1, True) * it
    s = (qq @ bk) * it
    m = torch.maximum(s0, s.max(1, keepdim=True).values)
    tot = _sum((s - m).exp(), 1, True)
    if seed_error != "pos_not_in_lse":
        tot = tot + (s0 - m).exp()
    lse = m + tot.log()
    w = it / b
    p0 = (s0 - lse).exp()
    p = (s - lse).exp()
    return {"terms": ((lse - s0) / b).reshape(-1), "mags": ((lse.abs() + s0.abs()) / b).reshape(-1),
            "dq": w * ((p0 - 1.0) * kk + p @ bk.t()), "dk": w * (p0 - 1.0) * qq,
            # p0 - 1 is itself a difference of numbers of size 1: that is the magnitude that enters
            "dq_floor": mag_floor(w * kk, w * (p @ bk.abs().t())), "dk_floor": mag_floor(w * qq)}


def bank_inputs(b, d, k, seed, key_in_bank=False):
    """unit rows q, k = q + 0.3 noise (float32, as wm_l2_normalize leaves them) and a bank of unit columns [d, k];
    key_in_bank: bank column 0 .. equals the key of row 0 (a negative that ties with the positive)"""
    g = torch.Generator().manual_seed(seed)
    o0 = torch.randn(b, d, generator=g)
    q, kp = normalized32(o0), normalized32(o0 + 0.3 * torch.randn(b, d, generator=g))
    bank = normalized32(torch.randn(k, d, generator=g)).t().contiguous()
    if key_in_bank:
        bank[:, k // 2] = kp[0]
    return q, kp, bank


# ------------------------------------------------------------------------------------------------ -cos
def neg_cosine(x0, x1, eps, dt=F64, seed_error=None):
    """-mean_i cos(x0_i, x1_i), each norm clamped at eps (torch.cosine_similarity) -> dict(terms [B], d0, d1, l0, l1).
    seed_error "eps_on_product": max(|a| |b|, eps)."""
    a, b = x0.to(dt), x1.to(dt)
    n = a.shape[0]
    e = _c(eps, dt)
    dot, l0, l1 = _sum(a * b, 1, True), _sum(a * a, 1, True).sqrt(), _sum(b * b, 1, True).sqrt()
    if seed_error == "eps_on_product":
        den = torch.maximum(l0 * l1, e)
        c0 = c1 = den.sqrt()
        live0 = live1 = l0 * l1 > e
    else:
        c0, c1 = torch.maximum(l0, e), torch.maximum(l1, e)
        den = c0 * c1
        live0, live1 = l0 > e, l1 > e
    cosv = dot / den
    k0 = torch.where(live0, cosv / (c0 * c0), torch.zeros_like(cosv))
    k1 = torch.where(live1, cosv / (c1 * c1), torch.zeros_like(cosv))
    w = -1.0 / n
    return {"terms": (-cosv / n).reshape(-1), "d0": w * (b / den - k0 * a), "d1": w * (a / den - k1 * b),
            "l0": l0.reshape(-1), "l1": l1.reshape(-1),
            "floor": lambda key, rows: mag_floor((w * (b / den))[rows], (w * k0 * a)[rows]) if key == "d0"
            else mag_floor((w * (a / den))[rows], (w * k1 * b)[rows])}


def neg_cosine_margin(r, eps):
    """min over rows and sides of |norm / eps - 1| on the float64 reference: the l > eps switch is safe far from 0"""
    return float(torch.cat([r["l0"], r["l1"]]).double().div(eps).sub(1.0).abs().min())


def neg_cosine_inputs(b, d, seed, zero=(), bf16=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(b, d, generator=g)
    c = a + torch.randn(b, d, generator=g)
    if "x0" in zero:
        a[0] = 0
    if "x1" in zero:
        c[b - 1] = 0
    if "both" in zero:
        a[b // 2] = 0
        c[b // 2] = 0
    return (kc.bf(a), kc.bf(c)) if bf16 else (a, c)


# ------------------------------------------------------------------------------------------------ cross-entropy / BCE
def cross_entropy(logits, labels, weight=None, dt=F64, seed_error=None):
    """torch's cross_entropy(weight, reduction="mean", ignore_index=-100) -> dict(terms [B] (sum = loss), dlogits, mags).
    seed_error: "mean_over_B" (divided by B, not by the weights' sum), "ignored_counted" (an ignored row counts with weight 1
    in the denominator)."""
    x = logits.to(dt)
    b, c = x.shape
    valid = (labels >= 0) & (labels < c)
    y = labels.clamp(0, c - 1)
    m = x.max(1, keepdim=True).values
    lse = m + _sum((x - m).exp(), 1, True).log()
    wy = (weight.to(dt)[y] if weight is not None else torch.ones(b, dtype=dt)) * valid
    nll = (lse - x.gather(1, y[:, None])).reshape(-1)
    den = _sum(wy, 0)
    if seed_error == "mean_over_B":
        den = torch.tensor(float(b), dtype=dt)
    elif seed_error == "ignored_counted":
        den = den + (~valid).sum().to(dt)
    onehot = torch.zeros(b, c, dtype=dt).scatter_(1, y[:, None], 1.0)
    dl = wy[:, None] * ((x - lse).exp() - onehot) / den
    # floor of dlogits: p - onehot is a difference of numbers of size 1, and the divisor is acc[1], B weights added by atomicAdd in
    # ANY order -- (B - 1) u relative at the most (Higham), asked for once, not F32_SUM_FACTOR times
    # (check_f32 asks for F32_SUM_FACTOR x the floor: the divisor's term is divided by that factor HERE so that it enters the
    # bound exactly once, as (B - 1) u max |dlogits|)
    floor = mag_floor(wy / den) + (b - 1) * U * float(dl.double().abs().max()) / kc.F32_SUM_FACTOR
    return {"terms": wy * nll / den, "dlogits": dl, "floor": floor,
             "mags": wy * (lse.reshape(-1).abs() + x.gather(1, y[:, None]).reshape(-1).abs()) / den}


def bce_logits(logits, target, pos_weight=None, dt=F64, seed_error=None):
    """BCEWithLogitsLoss(pos_weight), mean -> dict(terms [B, C], dlogits, mags).  seed_error "pos_weight_by_row": pos_weight[i / C]
    (mod C, so that it stays an index)."""
    x, t = logits.to(dt), target.to(dt)
    b, c = x.shape
    n = b * c
    if pos_weight is None:
        pw = torch.ones(b, c, dtype=dt)
    elif seed_error == "pos_weight_by_row":
        pw = pos_weight.to(dt)[(torch.arange(n) // c) % c].reshape(b, c)
    else:
        pw = pos_weight.to(dt)[None, :].expand(b, c)
    lw = 1.0 + (pw - 1.0) * t
    sp = (-x).clamp_min(0.0) + torch.log1p((-x.abs()).exp())
    term = (1.0 - t) * x + lw * sp
    sig = 1.0 / (1.0 + (-x).exp())
    inv = _c(1.0, dt) / _c(float(n), dt)
    return {"terms": term * inv, "dlogits": ((1.0 - t) - lw * (1.0 - sig)) * inv, "mags": (x.abs() + lw * sp) * inv,
            "floor": mag_floor((1.0 + lw) * inv)}


LOGIT_FAMILIES = ("randn", "offset+1e4", "dominant", "saturated")


def logit_inputs(family, b, c, seed, bf16=False):
    """[b, c] logits.  randn: 3 randn.  offset+1e4: 1e4 + randn.  dominant: one logit per row 100 above the rest.
    saturated: +-100 (BCE, with soft targets)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, generator=g) * 3
    if family == "offset+1e4":
        x = 1e4 + x / 3
    elif family == "dominant":
        x[torch.arange(b), torch.randint(0, c, (b,), generator=g)] += 100.0
    elif family == "saturated":
        x = torch.where(torch.rand(b, c, generator=g) < 0.5, torch.full_like(x, 100.0), torch.full_like(x, -100.0)) + x * 0.01
    elif family != "randn":
        raise ValueError(family)
    return kc.bf(x) if bf16 else x


# ------------------------------------------------------------------------------------------------ DCL / DCLW
def dcl(z0, z1, temp, sigma=None, dt=F64, seed_error=None):
    """lightly's DCLLoss (sigma None) / DCLWLoss on unit rows z0, z1 [B, D] -> dict(terms [2, B], dz0, dz1, mags).  Per direction
    (a, b) and row i:  l_i = -w_i <a_i, b_i> / T + lse_{k != i} <a_i, a_k> / T + lse_{k != i} <a_i, b_k> / T,  w detached.
    seed_error: self_in_negatives, weights_differentiated (the gradient flows through w), weight_one_direction (w = 1 in
    the second direction)."""
    zs = (z0.to(dt), z1.to(dt))
    b = z0.shape[0]
    it = _c(1.0, dt) / _c(temp, dt)
    eye = torch.eye(b, dtype=torch.bool)
    ones = torch.ones(b, dtype=dt)
    if sigma is None:
        w = [ones, ones]
    else:
        sp = dots(zs[0], zs[1]).diagonal() * (_c(1.0, dt) / _c(sigma, dt))
        e = (sp - sp.max()).exp()
        ww = 2.0 - b * e / _sum(e, 0)
        w = [ww, ones if seed_error == "weight_one_direction" else ww]
    pa, pb, terms, mags = [], [], [], []
    for dr in (0, 1):
        a, o = zs[dr], zs[1 - dr]
        saa, sab = dots(a, a) * it, dots(a, o) * it
        drop = torch.zeros_like(eye) if seed_error == "self_in_negatives" else eye
        ninf = torch.full_like(saa, -math.inf)

        def lse_p(s):
            sm = torch.where(drop, ninf, s)
            m = sm.max(1, keepdim=True).values
            l = m + _sum((sm - m).exp(), 1, True).log()
            return l.reshape(-1), torch.where(drop, torch.zeros_like(s), (s - l).exp())

        laa, p_aa = lse_p(saa)
        lab, p_ab = lse_p(sab)
        pos = sab.diagonal()
        terms.append((-w[dr] * pos + laa + lab) * 0.5 / b)
        mags.append((w[dr].abs() * pos.abs() + laa.abs() + lab.abs()) * 0.5 / b)
        pa.append(p_aa)
        pb.append(p_ab)
    cc = 0.5 * it / b
    grads, floors = [], []
    for which in (0, 1):
        a, o = zs[which], zs[1 - which]
        da, db = which, 1 - which
        wa, wo = pa[da] + pa[da].t(), pb[da] + pb[db].t()
        if dt == F32:    # dcl_grad_kernel: one accumulator, the two products of column k one after the other
            g = fma_matmul_f32(torch.stack([wa, wo], 2).reshape(b, 2 * b), torch.stack([a, o], 1).reshape(2 * b, -1))
        else:
            g = wa @ a + wo @ o
        grads.append(cc * (g - (w[da] + w[db])[:, None] * o))
        floors.append(mag_floor(cc * (wa.abs() @ a.abs() + wo.abs() @ o.abs()), cc * (w[da] + w[db]).abs()[:, None] * o))
    out = {"terms": torch.stack(terms), "mags": torch.stack(mags), "dz0": grads[0], "dz1": grads[1],
           "dz0_floor": floors[0], "dz1_floor": floors[1]}
    if seed_error == "weights_differentiated" and sigma is not None:
        r0, r1 = z0.double().clone().requires_grad_(True), z1.double().clone().requires_grad_(True)
        sp = (r0 * r1).sum(1) / float(np.float32(sigma))
        wd = 2.0 - b * torch.softmax(sp, 0)
        extra = (-(wd * (r0.detach() * r1.detach()).sum(1)) / float(np.float32(temp))).sum() / b   # both directions: 2 x 0.5
        g0, g1 = torch.autograd.grad(extra, (r0, r1))
        out["dz0"], out["dz1"] = out["dz0"] + g0.to(dt), out["dz1"] + g1.to(dt)
    return out


def dcl_inputs(b, d, seed, duplicates=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(b, d, generator=g)
    c = a + 0.5 * torch.randn(b, d, generator=g)
    if duplicates:
        k = min(b, 3)
        a[:k] = a[0]
        c[:k] = c[0]
    return normalized32(a), normalized32(c)


# ------------------------------------------------------------------------------------------------ Barlow / VICReg pieces
def barlow(raw, scale, lam, diag_weight, dt=F64, seed_error=None):
    """c = scale raw [D, D];  loss = diag_weight sum_i (c_ii - 1)^2 + lambda sum_{i != j} c_ij^2 -> dict(terms [D, D], draw).
    seed_error "lambda_on_diagonal": the diagonal terms carry lambda as well."""
    r = raw.to(dt)
    d = r.shape[0]
    sc, la, dw = _c(scale, dt), _c(lam, dt), _c(diag_weight, dt)
    c = r * sc
    eye = torch.eye(d, dtype=torch.bool)
    wd = dw * la if seed_error == "lambda_on_diagonal" else dw
    terms = torch.where(eye, wd * (c - 1.0) * (c - 1.0), la * c * c)
    g = torch.where(eye, 2.0 * wd * (c - 1.0), 2.0 * la * c)
    return {"terms": terms, "draw": g * sc, "floor": mag_floor(2.0 * torch.where(eye, wd * (c.abs() + 1.0), la * c.abs()) * sc)}


def center_columns(z, mean, dt=F64):
    """bf16(z - mean) of bf16 rows z [rows, C] and a float32 mean [C] (the emulation rounds, the reference does not)"""
    return _store(z.to(dt) - mean.to(dt)[None, :], dt, True)


def vicreg_variance(var_biased, n, eps, dt=F64, seed_error=None):
    """mean_d relu(1 - sqrt(var N / (N - 1) + eps)) and coef_d = d / d centred[n][d] / centred[n][d] = -[sd < 1] / (D (N - 1) sd)
    -> dict(terms [D], coef, sd).  seed_error: "biased_variance", "coef_without_hinge" (coef also where sd >= 1)."""
    v = var_biased.to(dt)
    d = v.shape[0]
    nn = _c(float(n), dt)
    var = v if seed_error == "biased_variance" else v * nn / _c(float(n - 1), dt)
    sd = (var + _c(eps, dt)).sqrt()
    hinge = (1.0 - sd).clamp_min(0.0)
    coef = -1.0 / (d * _c(float(n - 1), dt) * sd)
    if seed_error != "coef_without_hinge":
        coef = torch.where(hinge > 0, coef, torch.zeros_like(coef))
    return {"terms": hinge / d, "coef": coef, "sd": sd}


def vicreg_inputs(n, d, seed):
    """biased variances on both sides of the hinge, none with |sd - 1| below 0.01 (vicreg_margin asserts it on the reference)"""
    g = torch.Generator().manual_seed(seed)
    sd = torch.rand(d, generator=g) * 1.5 + 0.2
    sd = torch.where((sd - 1.0).abs() < 0.02, sd + 0.05, sd)
    if d >= 2:
        sd[0], sd[1] = 0.5, 1.5
    return (sd * sd * (n - 1) / n).float()


def vicreg_margin(r):
    return float((r["sd"].double() - 1.0).abs().min())


# ------------------------------------------------------------------------------------------------ Sinkhorn
def sinkhorn(out, eps, iters, dt=F64, seed_error=None):
    """lightly's sinkhorn on scores [B, K]: Q = E r c B with E = exp(out / eps), r = c = 1, and per round c_k = 1 / (K sum_b
    E r), then r_b = 1 / (B sum_k E c).  seed_error: "samples_first" (the two normalisations in the other order),
    "one_round_short"."""
    x = out.to(dt)
    b, k = x.shape
    e = (x * (_c(1.0, dt) / _c(eps, dt))).exp()
    r, c = torch.ones(b, 1, dtype=dt), torch.ones(1, k, dtype=dt)
    if iters == 0:      # nothing absorbs lightly's initial Q /= sum(Q) then
        return e / _sum(_sum(e, 1, True), 0, True) * float(b)
    for _ in range(iters - 1 if seed_error == "one_round_short" else iters):
        if seed_error == "samples_first":
            r = 1.0 / (_sum(e * c, 1, True) * b)
            c = 1.0 / (_sum(e * r, 0, True) * k)
        else:
            c = 1.0 / (_sum(e * r, 0, True) * k)
            r = 1.0 / (_sum(e * c, 1, True) * b)
    return e * r * c * float(b)


def sinkhorn_inputs(b, k, seed, bf16=False):
    """prototype scores are cosines: 0.9 clamp(randn, -1, 1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, k, generator=g).clamp(-1, 1) * 0.9
    return kc.bf(x) if bf16 else x


# ------------------------------------------------------------------------------------------------ end-to-end modules
# loss.BarlowTwinsLoss and loss.VICRegLoss as they compose their kernels, in float64.  emulate: a bf16 rounding wherever the
# module STORES bf16 -- the standardised / centred projections, the bf16 copy of `draw` the GEMM reads, the GEMM's output,
# the MSE gradient, every gradient handed back to autograd.  The float32 steps in between are three orders below that and
# stay float64 (kernel_check's rule).  Each returns dict(loss, dz_a, dz_b, loss_bound).
BF16_HALF_ULP = 2.0 ** -9          # the largest relative error of one bf16 rounding


def _stored_bound(*pairs):
    """what ANY pattern of bf16 roundings of stored tensors t can move a loss by, to first order: sum |dL/dt . t| 2^-9 over
    the (gradient, tensor) pairs"""
    return BF16_HALF_ULP * float(sum((g.double() * t.double()).abs().sum() for g, t in pairs))


def _gemm_bound(draw, a, b, n):
    """... and the float32 accumulation of raw = a^T b over n rows in any order: gamma_n |draw| . (|a|^T |b|)"""
    return float(n * U / (1.0 - n * U) * (draw.abs() * (a.abs().t() @ b.abs())).sum())


def barlow_twins_e2e(z_a, z_b, lam=5e-3, emulate=False, seed_error=None):
    """BarlowTwinsLoss: standardise over the batch (BatchNorm without affine, eps 0, biased variance) -> bf16 -> raw = za^T zb
    -> barlow kernel with scale (N - 1) / N^2 -> back through two GEMMs against the bf16 copy of draw and the BatchNorm
    backward.  seed_error "scale_1_over_n": c = raw / N (the unbiased-std factor forgotten)."""
    rnd = kc.bf if emulate else (lambda t: t)
    n, d = z_a.shape
    x, stat = [], []
    for z in (z_a.double(), z_b.double()):
        mean = z.mean(0)
        invstd = (z - mean).pow(2).mean(0).rsqrt()
        stat.append((z, mean, invstd))
        x.append(rnd((z - mean) * invstd))
    raw = x[0].t() @ x[1]
    scale = 1.0 / n if seed_error == "scale_1_over_n" else (n - 1) / (n * n)
    bl = barlow(raw, scale, lam, 1.0, dt=F64)
    w = rnd(bl["draw"])
    g = [rnd(x[1] @ w.t()), rnd(x[0] @ w)]
    out = {"loss": float(bl["terms"].sum())}
    for key, (z, mean, invstd), gz in zip(("dz_a", "dz_b"), stat, g):
        xh = (z - mean) * invstd
        out[key] = rnd(invstd * (gz - gz.mean(0) - xh * (gz * xh).mean(0)))
    t32 = barlow(raw.float(), scale, lam, 1.0, dt=F32)["terms"]
    out["loss_bound"] = (_stored_bound((x[1] @ bl["draw"].t(), x[0]), (x[0] @ bl["draw"], x[1])) + _gemm_bound(bl["draw"], x[0], x[1], n)
                         + scalar_bound(bl["terms"], t32, grid_chain(d * d, BARLOW_CAP)))
    return out


def vicreg_e2e(z_a, z_b, lam=25.0, mu=25.0, nu=1.0, eps=1e-4, emulate=False, seed_error=None):
    """VICRegLoss: lambda MSE(z_a, z_b) + per branch mu / 2 variance hinge (from the float32 column variance of z) + nu
    covariance term (centred projections stored in bf16 -> raw = zc^T zc -> barlow kernel with scale 1 / (N - 1), lambda 1 / D,
    no diagonal).  Gradients: the MSE's in bf16, times lambda in bf16; the branch's 2 nu GEMM(zc, bf16 draw) + mu / 2 coef zc,
    centred, in bf16; their sum in bf16.  seed_error: "cov_scale_n" (raw / N), "mu_not_halved"."""
    rnd = kc.bf if emulate else (lambda t: t)
    n, d = z_a.shape
    a, b = z_a.double(), z_b.double()
    diff = a - b
    loss = lam * float((diff * diff).mean())
    dm = rnd(rnd(2.0 * diff / (n * d)) * lam)
    bound = lam * (n * d) * U / (1.0 - n * d * U) * float((diff * diff).mean())      # any order of the N D float32 additions
    mu_b = mu if seed_error == "mu_not_halved" else 0.5 * mu
    grads = []
    for z, sign in ((a, 1.0), (b, -1.0)):
        mean = z.mean(0)
        zc = rnd(z - mean)
        vv = vicreg_variance((z - mean).pow(2).mean(0), n, eps, dt=F64)
        raw = zc.t() @ zc
        cs = 1.0 / n if seed_error == "cov_scale_n" else 1.0 / (n - 1)
        bl = barlow(raw, cs, 1.0 / d, 0.0, dt=F64)
        loss += mu_b * float(vv["terms"].sum()) + nu * float(bl["terms"].sum())
        dzc = 2.0 * nu * rnd(zc @ rnd(bl["draw"]).t()) + mu_b * vv["coef"] * zc
        grads.append(rnd(sign * dm + rnd(dzc - dzc.mean(0))))
        v32 = vicreg_variance((z - mean).pow(2).mean(0).float(), n, eps, dt=F32)
        t32 = barlow(raw.float(), cs, 1.0 / d, 0.0, dt=F32)["terms"]
        bound += (nu * (_stored_bound((2.0 * zc @ bl["draw"], zc)) + _gemm_bound(bl["draw"], zc, zc, n)
                        + scalar_bound(bl["terms"], t32, grid_chain(d * d, BARLOW_CAP)))
                  + mu_b * scalar_bound(vv["terms"], v32["terms"], grid_chain(d, VICREG_CAP) + n, vv["sd"] / d))
    return {"loss": loss, "dz_a": grads[0], "dz_b": grads[1], "loss_bound": bound + 8 * U * abs(loss)}


def e2e_inputs(n, d, seed, small_std=False):
    """bf16-exact projections of two views (the inputs tests/test_gpu_embed.py uses): small_std scales the columns by rand *
    1.5, so that some standard deviations lie below the VICReg hinge and some above"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, d, generator=g) * (torch.rand(d, generator=g) * 1.5 if small_std else 1.5) + (0.0 if small_std else 0.3)
    b = a + (0.4 if small_std else 0.7) * torch.randn(n, d, generator=g)
    return kc.bf(a), kc.bf(b)
