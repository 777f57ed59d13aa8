"""The loss and token kernels of the second half of csrc/transformer.hip restated on the CPU (sibling of tests/loss_cases.py,
whose tools it reuses): one function per operation, written once and run in two precisions.  `dt=torch.float64` is the
reference; `dt=torch.float32` is the yardstick `emul` of tests/kernel_check.py: the plain float32 restatement of the same
formulae, float32 sums through numpy's float32 accumulation (loss_cases._sum), bf16 roundings exactly where a kernel packs
bf16 (dpred, dstudent, the tokens).  expf / logf are plain float32 functions (these kernels do not use __expf).  Every
function carries switches that seed ONE wrong computation; tests/test_vit_cases_cpu.py proves that each is rejected by the
criteria and at the shapes of tests/test_gpu_vit_losses.py and tests/test_gpu_tokens.py, that the honest variants (another
summation order, other rounding events) are accepted, and that every float64 reference agrees with torch autograd in double.

Also here: the launch arithmetic of these kernels mirrored in Python (ew_blocks and its 8192-block cap, the 1024-block cap of
the MSE / L1 sweep, the DL_MAXV register passes of the row kernels, colsum_geometry), so that a test that claims a code path
asserts that its shape reaches it; the input families; and the cases (inputs, reference, yardstick) the CPU and the GPU tests
share, built once per shape."""
import functools
import math

import kernel_check as kc
import loss_cases as lc
import numpy as np
import torch
from loss_cases import F32, F64, _c, _store, _sum, cdiv

# ------------------------------------------------------------------------------------------------ launch arithmetic
TF_THREADS = 256
EW_BLOCK_CAP = 8192
EW_CAP = EW_BLOCK_CAP * TF_THREADS        # work items of one sweep of an ew_blocks grid: 2 097 152
MSE_BLOCK_CAP = 1024
DL_MAXV = 4
DL_MAX_D = TF_THREADS * 8 * DL_MAXV       # 8192: the widest row of the register-tiled row kernels
ARGSORT_MAX = 256


def ew_blocks(work):
    """blocks of a 256-thread grid-stride kernel over `work` items (transformer.hip: ew_blocks)"""
    return max(1, min(EW_BLOCK_CAP, cdiv(work, TF_THREADS)))


def ew_sweeps(work):
    """trips of the grid-stride loop the busiest thread makes"""
    return cdiv(work, ew_blocks(work) * TF_THREADS)


def mse_blocks(n):
    """wm_mse_fwd_bwd / wm_l1_fwd_bwd: one work item is a chunk of 8 elements, the grid is capped at 1024 blocks"""
    return min(MSE_BLOCK_CAP, cdiv(n // 8, TF_THREADS))


def mse_sweeps(n):
    return cdiv(n // 8, mse_blocks(n) * TF_THREADS)


def mse_chain(n):
    """the longest chain of float32 additions a term of the scalar goes through: 8 per chunk the thread sweeps, 6 wave_sum
    steps, 3 additions of the wave partials, the block's atomicAdd among `blocks`"""
    return 8 * mse_sweeps(n) + 6 + 3 + mse_blocks(n)


def row_passes(d):
    """register passes of a row kernel: a row is d / 8 chunks over 256 threads"""
    return cdiv(d // 8, TF_THREADS)


def dino_chain(vs, vt, b):
    return lc.row_chain(8 * DL_MAXV * vt, vs * b)


def memax_chain(k):
    """the scalar of the mean-entropy regulariser: block 0 sweeps K in steps of 256, block reduction, one atomicAdd"""
    return cdiv(k, TF_THREADS) + 6 + 3 + 1


def colsum_geometry(rows, c):
    """(CB, slabs, rb, rpb) of transformer.hip's colsum_geometry: CB chunks per column slab, rb row blocks of rpb rows"""
    nch = c >> 3
    cb = nch if nch <= 64 else 64
    slabs = cdiv(nch, cb)
    rb = cdiv(768, slabs)
    rpb = max(cdiv(rows, rb), 64)
    return cb, slabs, cdiv(rows, rpb), rpb


def colsum_row_lanes(c):
    """(RL, idle threads): row lanes of a colsum block, and the threads beyond RL * CB that do nothing"""
    cb = colsum_geometry(1, c)[0]
    rl = TF_THREADS // cb
    return rl, TF_THREADS - rl * cb


def _inv_temp(temp, dt):
    """1.f / temp as the host computes it from the float32 argument (both precisions start from THAT float32 temperature)"""
    return _c(1.0, dt) / _c(temp, dt)


# ------------------------------------------------------------------------------------------------ MSE / L1
MSE_SHAPES = (8, 2040, EW_CAP, EW_CAP + 8, 3 * EW_CAP + 8)
MSE_FAMILIES = ("randn", "lattice", "offset")


def mse_inputs(family, n, seed):
    """(pred, target) [n / 8, 8] bf16-exact.  lattice: integers in -2 .. 2 (exact differences, L1 ties at 0).  offset: both
    300 + randn (bf16 grid 2 there: the differences are small integers on a large common term)."""
    g = torch.Generator().manual_seed(seed)
    if family == "lattice":
        a, b = (torch.randint(-2, 3, (n // 8, 8), generator=g).float() for _ in range(2))
        return a, b
    a, b = torch.randn(n // 8, 8, generator=g), torch.randn(n // 8, 8, generator=g)
    if family == "offset":
        a, b = a + 300.0, b + 300.0
    elif family != "randn":
        raise ValueError(family)
    return kc.bf(a), kc.bf(b)


def mse(pred, target, l1=False, dt=F64, seed_error=None):
    """mean (pred - target)^2, or mean |pred - target| -> dict(terms (their sum is the loss), dpred (bf16 in the emulation), loss).
    float32 as the kernel: inv = 1.f / (float)n, d = 2 df inv (one rounding: 2 df is exact), L1 +-inv and 0 at df == 0.
    seed_error: mean_over_rows (inv = 1 / rows of the [rows, 8] view), grad_factor_1 (d = df inv), l1_sign_at_zero (+inv at a
    tie), sweep_tail_dropped (the elements behind the first grid sweep contribute nothing and their dpred stays 0)."""
    a, b = pred.to(dt), target.to(dt)
    n = a.numel()
    inv = _c(1.0, dt) / _c(float(a.shape[0] if seed_error == "mean_over_rows" else n), dt)
    df = a - b
    if l1:
        terms = df.abs() * inv
        pos = inv.expand_as(df) if seed_error == "l1_sign_at_zero" else torch.where(df > 0, inv, torch.zeros_like(df))
        d = torch.where(df < 0, -inv, pos)
    else:
        terms = df * df * inv
        d = (df * inv) if seed_error == "grad_factor_1" else (2.0 * df) * inv
    if seed_error == "sweep_tail_dropped":
        first = mse_blocks(n) * TF_THREADS * 8
        terms, d = terms.clone(), d.clone()
        terms.reshape(-1)[first:] = 0
        d.reshape(-1)[first:] = 0
    return {"terms": terms.reshape(-1), "dpred": _store(d, dt, True), "loss": _sum(terms.reshape(-1), 0)}


@functools.lru_cache(maxsize=2)
def mse_case(family, n, l1):
    pred, target = mse_inputs(family, n, seed=n % 1000 + 17)
    return (pred, target), mse(pred, target, l1, dt=F64), mse(pred, target, l1, dt=F32)


# ------------------------------------------------------------------------------------------------ row softmax losses
ROW_D = (8, 2040, 2048, 2056, 8192)
DINO_VIEWS = ((2, 2, 1), (8, 2, 5), (1, 2, 3), (3, 5, 2))
SOFT_CE_VIEWS = ((1, 1), (1, 7), (3, 1), (3, 7))
TEACHER_TEMPS = (0.04, 0.07)
STUDENT_TEMP = 0.1
SOFTMAX_FAMILIES = ("randn", "offset", "sharp", "onehot", "constant", "matched")


def _row_exp(x, seed_error):
    """(m, exp(x - m), their row sum) over the last dim.  no_max: m = 0.  tail_chunk_dropped: the sum stops after the first
    register pass (256 chunks = 2048 elements)."""
    m = torch.zeros_like(x[..., :1]) if seed_error == "no_max" else x.max(-1, keepdim=True).values
    e = (x - m).exp()
    src = e[..., :TF_THREADS * 8] if seed_error == "tail_chunk_dropped" else e
    return m, e, _sum(src, x.dim() - 1, True)


def dino_teacher_probs(teacher, center, temp, dt=F64, seed_error=None):
    """softmax((t - center) / T) per row -> [rows, D].  seed_error: center_ignored, probs_unnormalised, no_max,
    tail_chunk_dropped."""
    v = teacher.to(dt)
    if seed_error != "center_ignored":
        v = v - center.to(dt)[None, :]
    v = v * _inv_temp(temp, dt)
    _, e, s = _row_exp(v, seed_error)
    return e if seed_error == "probs_unnormalised" else e * (1.0 / s)


def dino_loss(student, probs, vs, vt, b, temp, skip_same=1, dt=F64, seed_error=None):
    """mean over (student view s, teacher view t != s when skip_same, sample) of -<p_t, log_softmax(x_s / T)> -> dict(terms [Vs, B]
    (their sum is the loss), dstudent [Vs B, D] (bf16 in the emulation), lse [Vs, B], mags, floor).
    w = 1 / (n_terms B), n_terms = Vs Vt - min(Vs, Vt) with the diagonal skipped; dstudent = w / T (nt softmax - sum_t p_t), nt
    the teacher views student view s meets.  Soft cross-entropy is Vt = 1, skip_same = 0.
    seed_error: count_diag (w from Vs Vt), no_skip (the diagonal terms join), nt_is_vt (nt = Vt for every view), no_max,
    grad_without_temp (w instead of w / T), tail_chunk_dropped (lse from the first 256 chunks of the row)."""
    d = student.shape[-1]
    it = _inv_temp(temp, dt)
    x = student.to(dt).reshape(vs, b, d) * it
    p = probs.to(dt).reshape(vt, b, d)
    m, _, s = _row_exp(x, seed_error)
    lse = m + s.log()
    ndiag = min(vs, vt) if skip_same else 0
    n_terms = vs * vt - (0 if seed_error == "count_diag" else ndiag)
    if vs * vt - ndiag <= 0:
        raise ValueError("no terms")
    mask = torch.ones(vs, vt, dtype=dt)
    if skip_same and seed_error != "no_skip":
        for i in range(min(vs, vt)):
            mask[i, i] = 0.0
    w = _c(1.0, dt) / (_c(float(n_terms), dt) * _c(float(b), dt))
    nt = torch.full((vs,), float(vt), dtype=dt) if seed_error == "nt_is_vt" else mask.sum(1)
    g = torch.einsum("st,tbd->sbd", mask, p)
    lsm = x - lse
    k = w if seed_error == "grad_without_temp" else w * it
    part_sm, part_p = k * nt[:, None, None] * lsm.exp(), k * g
    return {"terms": -_sum(g * lsm, 2) * w, "dstudent": _store((part_sm - part_p).reshape(vs * b, d), dt, True),
            "lse": lse.reshape(vs, b),
            # the magnitudes that enter a term: x / T and lse are subtracted before the product with p
            "mags": (g.double() * (x.double().abs() + lse.double().abs())).sum(2) * float(w),
            # ... and an element of the gradient: nt softmax and sum_t p_t cancel where the student matches its teachers
            "floor": lc.mag_floor(part_sm, part_p)}


def _max_to_tail(x):
    """every row's largest element swapped into the row's last chunk of 8 (at position D - 1 - row % 8): the same values, with
    the weight of the softmax where a register pass that is left out would lose it"""
    x = x.clone()
    r = torch.arange(x.shape[0])
    j, t = x.argmax(1), x.shape[1] - 1 - r % 8
    x[r, j], x[r, t] = x[r, t].clone(), x[r, j].clone()
    return x


def softmax_inputs(family, vs, vt, b, d, temp_t, seed):
    """dict(student [Vs B, D], teacher [Vt B, D] bf16-exact, center [D] float32, probs [Vt B, D] float32 = the float64
    reference's teacher probabilities stored as float32).
    offset: +30 on every student logit (x / T = 300).  sharp: one teacher logit per row 3 above the rest (75 at T = 0.04).
    onehot: exactly one-hot probs fed directly.  constant: every logit of a row equal.  matched: all student views equal
    and probs = their own softmax: the gradient cancels to nothing.  In every family the largest logit of a row lies in the row's
    last chunk (_max_to_tail)."""
    g = torch.Generator().manual_seed(seed)
    student, teacher = torch.randn(vs * b, d, generator=g), torch.randn(vt * b, d, generator=g)
    center = 0.1 * torch.randn(d, generator=g)
    if family == "offset":
        student = student + 30.0
    elif family == "sharp":
        teacher[torch.arange(vt * b), torch.randint(0, d, (vt * b,), generator=g)] += 3.0
    elif family == "constant":
        student = (torch.randint(-3, 4, (vs * b, 1), generator=g).float() * 0.75).expand(vs * b, d).clone()
        teacher = (torch.randint(-3, 4, (vt * b, 1), generator=g).float() * 0.75).expand(vt * b, d).clone()
        center = torch.full((d,), 0.25)
    elif family == "matched":
        student = student[:b].repeat(vs, 1)
    elif family not in ("randn", "onehot"):
        raise ValueError(family)
    student, teacher = kc.bf(_max_to_tail(student)), kc.bf(_max_to_tail(teacher))
    probs = dino_teacher_probs(teacher, center, temp_t, dt=F64).float()
    if family == "onehot":
        probs = torch.zeros(vt * b, d)
        probs[torch.arange(vt * b), torch.randint(0, d, (vt * b,), generator=g)] = 1.0
    elif family == "matched":
        probs = torch.softmax(student[:b].double() * float(_inv_temp(STUDENT_TEMP, F64)), 1).float().repeat(vt, 1)
    return {"student": student, "teacher": teacher, "center": center, "probs": probs}


@functools.lru_cache(maxsize=None)
def dino_case(family, vs, vt, b, d, temp_t, skip_same=1):
    i = softmax_inputs(family, vs, vt, b, d, temp_t, seed=vs * 100 + vt * 10 + b + d)
    args = (i["student"], i["probs"], vs, vt, b, STUDENT_TEMP, skip_same)
    return i, dino_loss(*args, dt=F64), dino_loss(*args, dt=F32)


def softmax_floor(family, ref):
    """absolute term of dstudent: 0 (the bf16 emulation alone is the yardstick) but in the families that make nt softmax and
    sum_t p_t cancel, where it is one float32 rounding at the magnitude of those two"""
    return ref["floor"] if family in ("matched", "constant") else 0.0


DINO_FAMILY_SHAPES =tuple((8, v) for v in ((2, 2, 1), (3, 5, 2))) + ((2056, (3, 5, 2)),)


# ------------------------------------------------------------------------------------------------ mean-entropy regulariser
MEMAX_N = (1, 7, 300)
MEMAX_K = (8, 1024, 2056)
MEMAX_FAMILIES = ("randn", "offset", "constant", "underflow")
MEMAX_TEMP = 0.1
MEMAX_CLAMP = 1e-30


def memax_inputs(family, n, k, seed):
    """(logits [N, K] bf16-exact, log_prior [K] float32: the power-law prior of PMSN).  underflow: prototype column K / 2 lies
    400 below the others, so that at T = 0.1 its probabilities and m_k are 0 in float32 (and in float64)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, k, generator=g)
    if family == "offset":
        x = x + 30.0
    elif family == "constant":
        x = (torch.randint(-3, 4, (n, 1), generator=g).float() * 0.75).expand(n, k).clone()
    elif family == "underflow":
        x[:, k // 2] -= 400.0
    elif family != "randn":
        raise ValueError(family)
    prior = 1.0 / torch.arange(1, k + 1, dtype=F64) ** 0.25
    return kc.bf(x), (prior / prior.sum()).log().float()


def mean_entropy_reg(logits, log_prior, temp, dt=F64, seed_error=None):
    """p = softmax(x / T), m = mean over the rows (float32: accumulated in row order), reg = sum_k m_k (log max(m_k, 1e-30) -
    log prior_k), dlogits = p (u - <p, u>) / (N T) with u = log max(m, 1e-30) - log prior + 1 -> dict(m, terms [K] (their sum
    is the scalar), dlogits (float32), floor, m_floor).  The clamp is applied in both precisions.
    seed_error: prior_ignored, mean_is_sum (m without 1 / N), grad_without_temp (1 / N instead of 1 / (N T)),
    scalar_from_row_sum (every row's block adds the scalar: N times the value)."""
    n, k = logits.shape
    it = _inv_temp(temp, dt)
    inv_n = _c(1.0, dt) / _c(float(n), dt)
    x = logits.to(dt) * it
    _, e, s = _row_exp(x, None)
    contrib = e * ((_c(1.0, dt) if seed_error == "mean_is_sum" else inv_n) / s)
    m = _sum(contrib, 0)
    lp = torch.zeros(k, dtype=dt) if (log_prior is None or seed_error == "prior_ignored") else log_prior.to(dt)
    logm = torch.maximum(m, _c(MEMAX_CLAMP, dt)).log()
    u = logm - lp + 1.0
    p = e * (1.0 / s)
    pu = _sum(p * u, 1, True)
    c = inv_n if seed_error == "grad_without_temp" else inv_n * it
    terms = m * (logm - lp)
    if seed_error == "scalar_from_row_sum":
        terms = terms * float(n)
    return {"m": m, "terms": terms, "dlogits": c * p * (u - pu), "mags": m.double() * (logm.double().abs() + lp.double().abs()),
            "floor": lc.mag_floor(c * p * u, c * p * pu), "m_floor": kc.f32_sum_floor(contrib)}


@functools.lru_cache(maxsize=None)
def memax_case(family, n, k, prior):
    x, lp = memax_inputs(family, n, k, seed=n + k)
    lp = lp if prior else None
    return (x, lp), mean_entropy_reg(x, lp, MEMAX_TEMP, dt=F64), mean_entropy_reg(x, lp, MEMAX_TEMP, dt=F32)


# ------------------------------------------------------------------------------------------------ tokens
TOKEN_SHAPES = ((1, 1, 8), (3, 36, 384), (2, 196, 192), (57, 196, 1536))        # (N, np, D); the last is over EW_CAP


def tokens_inputs(n, np_, d, seed):
    g = torch.Generator().manual_seed(seed)
    return kc.bf(torch.randn(n * np_, d, generator=g)), torch.randn(d, generator=g), torch.randn(np_ + 1, d, generator=g)


def tokens_assemble(patches, cls, pos, n, np_, dt=F64, seed_error=None):
    """[cls + pos[0]; patches + pos[1:]] per image -> [N (np + 1), D]: the float32 add, then bf16 (the emulation).
    seed_error: pos_shift (token s gets pos[s + 1], cyclically), cls_without_pos, patch_rows_transposed (token (n, s) takes patch
    row (s - 1) N + n)."""
    d = patches.shape[1]
    pt = patches.to(dt)
    pt = pt.reshape(np_, n, d).transpose(0, 1) if seed_error == "patch_rows_transposed" else pt.reshape(n, np_, d)
    tok = torch.cat([cls.to(dt).reshape(1, 1, d).expand(n, 1, d), pt], 1)
    pp = pos.to(dt).reshape(np_ + 1, d)
    if seed_error == "pos_shift":
        pp = pp.roll(-1, 0)
    add = pp[None].expand(n, np_ + 1, d).clone()
    if seed_error == "cls_without_pos":
        add[:, 0] = 0.0
    return _store((tok + add).reshape(n * (np_ + 1), d), dt, True)


PATCHIFY_SHAPES = ((1, 32, 8), (3, 32, 16), (1, 32, 32), (3, 96, 8), (1, 96, 16), (3, 96, 32), (1, 224, 8), (3, 224, 16),
                   (1, 224, 32), (112, 224, 16))      # (N, S, p); the last: 112 x 224 x 224 x 3 / 8 = 2 107 392 chunks


def patchify(img, p):
    """[N, S, S, 3] -> [N (S / p)^2, p, p, 3]: patch (gy, gx) of image n is row (n g + gy) g + gx"""
    n, s = img.shape[0], img.shape[1]
    g = s // p
    return img.reshape(n, g, p, g, p, 3).permute(0, 1, 3, 2, 4, 5).reshape(n * g * g, p, p, 3).contiguous()


ROWS_SHAPES = ((1, 1, 1, 8), (4, 50, 12, 64), (3, 197, 49, 384), (43, 256, 256, 1536))   # (B, S, K, C); the last: 2 113 536 chunks


def index_inputs(b, s, k, seed, hostile=False):
    """idx [B, K] int64: K distinct positions of 0 .. S - 1 per row; hostile: the first of every row is -1 and (K > 1) the
    last is S, both of which the kernel skips"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(s, generator=g)[:k] for _ in range(b)]).to(torch.int64)
    if hostile:
        idx[:, 0] = -1
        if k > 1:
            idx[:, -1] = s
    return idx


def rows_by_index(src, idx, b, s, k, out, scatter=False, seed_error=None):
    """gather: out[b K + j] = src[b S + idx[b][j]];  scatter: out[b S + idx[b][j]] = src[b K + j];  an index outside 0 .. S - 1
    moves nothing (the row of `out` keeps its content).  Works on any dtype: a pure permutation.
    seed_error: gather_batch_stride_k (the big row is b K + idx), scatter_as_gather."""
    out = out.clone()
    bi = torch.arange(b)[:, None].expand(b, k)
    ok = (idx >= 0) & (idx < s)
    big = (bi * (k if seed_error == "gather_batch_stride_k" else s) + idx)[ok]
    small = (bi * k + torch.arange(k)[None, :])[ok]
    if seed_error == "scatter_as_gather":
        scatter = False
    if scatter:
        out[big] = src[small]
    else:
        out[small] = src[big % src.shape[0]] if seed_error else src[big]
    return out


ARGSORT_S = (1, 2, 50, 255, 256)
ARGSORT_KEYS = ("uniform", "equal", "two_values", "signed_zero", "inf")


def argsort_inputs(kind, rows, s, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.rand(rows, s, generator=g)
    if kind == "equal":
        k = torch.full((rows, s), 0.5)
    elif kind == "two_values":
        k = (k < 0.5).float()
    elif kind == "signed_zero":
        k = torch.where(k < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    elif kind == "inf":
        k = torch.where(k < 0.3, torch.tensor(math.inf), k)
    elif kind != "uniform":
        raise ValueError(kind)
    return k


def argsort_rows(keys, seed_error=None):
    """ascending, ties to the lower index (numpy's stable argsort; -0.0 == 0.0).  seed_error: argsort_ties_high,
    argsort_descending (ties still to the lower index)."""
    a = keys.numpy()
    s = a.shape[1]
    if seed_error == "argsort_ties_high":
        return torch.from_numpy(s - 1 - np.argsort(a[:, ::-1], axis=1, kind="stable"))
    if seed_error == "argsort_descending":
        return torch.from_numpy(np.argsort(-a, axis=1, kind="stable"))
    return torch.from_numpy(np.argsort(a, axis=1, kind="stable"))


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_SHAPES = ((1, 8), (63, 384), (64, 384), (65, 384), (129, 512), (129, 520), (3, 37 * 384), (25216, 192))
COLSUM_FAMILIES = ("lattice", "randn", "offset")


def colsum_inputs(family, rows, c, seed):
    """[rows, C] bf16-exact.  lattice: integers in -2 .. 2 (every sum exact in any order).  offset: 8 + randn."""
    g = torch.Generator().manual_seed(seed)
    if family == "lattice":
        return torch.randint(-2, 3, (rows, c), generator=g).float()
    x = torch.randn(rows, c, generator=g)
    if family == "offset":
        x = x + 8.0
    elif family != "randn":
        raise ValueError(family)
    return kc.bf(x)


def colsum(x, dt=F64, seed_error=None):
    """colsum_kernel<1> -> dict(part [rb, C]: the block sums of the slot form, out [C]: their sum).  A block's sum is its RL row
    lanes (lane l walks rows r0 + l, r0 + l + RL, ...) added in lane order; float32 throughout in the emulation.
    seed_error: rows-1, last_block_dropped, slab_tail_dropped (the chunks of the last, partial column slab stay 0)."""
    rows, c = x.shape
    cb, slabs, rb, rpb = colsum_geometry(rows, c)
    rl = TF_THREADS // cb
    v = x.to(dt)
    use = rows - 1 if seed_error == "rows-1" else rows
    parts, part_floor = [], 0.0
    for blk in range(rb):
        xb = v[blk * rpb:min((blk + 1) * rpb, use)]
        if xb.shape[0] == 0 or (seed_error == "last_block_dropped" and blk == rb - 1):
            parts.append(torch.zeros(c, dtype=dt))
            continue
        part_floor = max(part_floor, kc.f32_sum_floor(xb))
        pad = (-xb.shape[0]) % rl
        xb = torch.cat([xb, torch.zeros(pad, c, dtype=dt)]).reshape(-1, rl, c)
        parts.append(_sum(_sum(xb, 0), 0))
    part = torch.stack(parts)
    if seed_error == "slab_tail_dropped" and (c >> 3) % cb:
        part[:, (slabs - 1) * cb * 8:] = 0.0
    # floors: one float32 rounding at the largest column's sum of magnitudes, of one block and of all rows
    return {"part": part, "out": _sum(part, 0), "part_floor": part_floor, "out_floor": kc.f32_sum_floor(v)}


@functools.lru_cache(maxsize=None)
def colsum_case(family, rows, c):
    x = colsum_inputs(family, rows, c, seed=rows + c)
    return x, colsum(x, dt=F64), colsum(x, dt=F32)


MATMUL_SHAPES = ((1, 1, 1), (16, 16, 16), (17, 33, 5), (36, 196, 384), (9, 49, 768))       # (M, K, N)


def matmul_inputs(m, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, k, generator=g), torch.randn(k, n, generator=g)
