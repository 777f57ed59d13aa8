"""GPU checks of the Gaussian log-sum kernel (csrc/kde.hip: wm_kde_logsum) and of density.py built on it, against the numpy
float64 restatement (density.ref_gaussian_log_sums; tests/test_kde_cpu.py checks it against sklearn) on the EXACT float64
squared distances of the same float32 rows and, end to end, against sklearn.

Bounds are derived, not tuned.  Notation: a = 1 / (2 h^2); s_ij the exact squared distance of the float32 rows i, j; L_i =
log sum_j exp(-a s_ij) the exact log-sum; w_ij = exp(-a s_ij - L_i) the softmax weights of row i; u = 2^-53.
  (a) Distances.  The kernel's s is the float32 chain of cl_dist.h: within eps = (d + 2) 2^-24 relative of s_ij (first
      order: one rounding per difference, twice in the square, one per fused multiply-add).  So each kernel term is the
      exact term times exp(delta_j), |delta_j| <= eps a s_ij, and the log-sum moves by at most
          log sum_j w_ij exp(eps a s_ij)                    (upwards; downwards by -log sum_j w_ij exp(-eps a s_ij), which
      is no larger: (sum w e^x)(sum w e^-x) >= 1).  It is computed per row and bandwidth from the reference in float64
      (`log_sum_reference`).  Rows of small integers make the chain exact: eps = 0 there (`exact=True`).
  (b) float64, kernel and restatement together (`float64_slack`), absolute in the log-sum.
      - A term exp(-a (s_j - s_min)).  The gap of two widened floats is rounded once, its product with a once: the
        argument moves by 2 u |a (s_j - s_min)|, the term by that relative amount; over the terms that carry weight,
        2 u sum_j w_ij a (s_j - s_min) per side, 4 u in all.
      - The exponential itself: at most 4 ulp = 8 u assumed for either library (both document less): 16 u.
      - The kernel reaches the row's minimum in steps: a thread rescales its sums when its minimum drops, once more to the
        row's minimum and once more to the minimum over the slices.  The arguments of these factors add up to the same
        a (s_j - s_min) (counted above); each factor adds an exponential and a product, 9 u, and there are at most
        ceil(n / 64) + 2 of them (one per column tile, the lanes, the slices).
      - A sum of n non-negative terms in any order: (n - 1) u relative per side.
      - log S with S in [1, n]: 4 ulp = 8 u log n per side; -a s_min rounded once, u |a s_min| per side; the final sum once,
        u |L| per side.
      Total: (2 (n - 1) + 16 + 9 (ceil(n / 64) + 2)) u + 4 u sum_j w_ij a (s_j - s_min) + 16 u log n + 2 u |a s_min| + 2 u |L|.
  (c) A log-sum-exp of values that move by at most b_c each moves by at most log sum_c v_c exp(b_c), v the softmax of the
      values (`propagate`): the classes' sums into the ungrouped one, the rows' sums into the uniformity, the classes'
      joint log-probabilities into the posterior's normaliser.
  (d) Bits.  The order of every sum is a function of (m, n, d); the shared minimum depends on s alone: two calls, a
      bandwidth alone and inside a list, and a list cut into launches give equal bits.
  (e) End to end, 512 golden rows, standardised, all 512 features, h in {0.5, 0.985, 2, 5, 10, 20}: sklearn in float64 on
      the same float32 values (one leaf: test_kde_cpu.sk_kde), whose own distance to the restatement is covered by the
      1e-10 of the CPU tests, added to every bound.  Asserted on the reference alone: the largest score_samples bound is
      below 1e-3 (1.0e-4 on these rows; 1.1e-4 .. 1.3e-4 on 2 000).  The leave-one-out bounds are NOT that small and cannot
      be: without the self the sum of an outlying row is led by a far neighbour, and (a) is eps a s_min there -- 0.12 at
      h = 0.5 (a = 2, s_min about 2 000), 1.1e-4 at h = 20 -- which is what float32 distances give; every row is still
      held to ITS bound.  sklearn has no leave-one-out: its value for row i is a refit without the row, 1.2 s for 64 rows
      here, so every row is judged against the restatement (which tests/test_kde_cpu.py holds to n refits at 1e-10) and
      the 16 rows of LOO_REFITS against sklearn's refits, for each of the six bandwidths.
"""
import math

import numpy as np
import pytest
import torch
from parity_log import parity

from test_kde_cpu import exact_sq, log_sum_reference, propagate, sk_kde, uniformity_formula
from test_spectral_cpu import golden_labels, golden_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
GOLDEN_H = [0.5, 0.985, 2.0, 5.0, 10.0, 20.0]
SKLEARN_SLACK = 1e-10
LOO_REFITS = range(0, 512, 32)  # the rows whose leave-one-out value sklearn refits


def D():
    from ssl_wafermap_amd import density

    return density


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def normal_rows(n, d, seed):
    return np.random.default_rng(1000 * n + d + seed).standard_normal((n, d)).astype(np.float32)


def neighbour_scale(sq):
    """The median over the rows of the distance to the nearest OTHER column (1 when there is none)."""
    if sq.shape[1] < 2:
        return 1.0
    off = np.where(np.eye(*sq.shape, dtype=bool), np.inf, sq) if sq.shape[0] == sq.shape[1] else sq
    return float(np.sqrt(np.median(off.min(axis=1)))) or 1.0


def worst(got, ref, bound):
    """max |got - ref| / bound over the finite reference entries; the others must be -inf on both sides; no NaN."""
    assert got.shape == ref.shape and got.dtype == np.float64 and not np.isnan(got).any()
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])  # -inf exactly where nothing is included
    if not fin.any():
        return 0.0
    assert np.isfinite(got[fin]).all()
    return float((np.abs(got[fin] - ref[fin]) / bound[fin]).max())


def check(name, xq, x, hs, self_offset, exact=False):
    """The kernel against the restatement on exact distances, inside the bound of (a) + (b); returns the device values."""
    dens = D()
    got = host(dens.gaussian_log_sums(dev(xq), dev(x), hs, self_offset=self_offset))
    ref, bound = log_sum_reference(exact_sq(xq, x), dens.scales_of(np.asarray(hs, dtype=np.float64)), x.shape[1], self_offset, exact)
    parity(f"kde log-sum {name} / bound", worst(got, ref, bound), 1.0)
    return got, ref, bound


# ------------------------------------------------------------------------------------------------ (a), (b) shapes


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_square_sizes(n):
    """n = 1 with the self excluded: -inf.  63 / 64 / 65: one column tile with and without padding, then two; 129: three
    column tiles in three slices, merged."""
    x = normal_rows(n, 6, 0)
    hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(exact_sq(x, x))
    loo, _, _ = check(f"n={n} d=6 leave-one-out", x, x, hs, 0)
    full, _, _ = check(f"n={n} d=6 all columns", x, x, hs, None)
    if n == 1:
        assert np.all(loo == -np.inf) and np.all(full == 0.0)
    else:
        assert np.all(full > loo)


@pytest.mark.parametrize("d", [1, 31, 32, 33, 70])
def test_feature_chunks(d):
    """The 32-feature staging chunk: below it, exactly one, one feature into the second, and a third with padding."""
    x = normal_rows(65, d, 1)
    hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(exact_sq(x, x))
    check(f"n=65 d={d} leave-one-out", x, x, hs, 0)
    check(f"n=65 d={d} all columns", x, x, hs, None)


@pytest.mark.parametrize("m, n", [(5, 200), (130, 3)])
def test_rectangular(m, n):
    xq, x = normal_rows(m, 6, 2), normal_rows(n, 6, 3)
    hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(exact_sq(xq, x))
    check(f"m={m} n={n} all columns", xq, x, hs, None)
    check(f"m={m} n={n} offset 0", xq, x, hs, 0)  # row i without column i, where there is one
    check(f"m={m} n={n} offset 2", xq, x, hs, 2)


def test_minimum_drops_tile_after_tile():
    """Five column tiles in five slices of one tile each: every thread's minimum is set once, from +inf, and what is
    rescaled is the lanes' and the slices' sums, to the row's minimum (the end of a slice and kde_merge).  The columns are
    sorted by falling and by rising distance from the queries' region, so the slices' minima fall and rise.  The thread's
    own rescale needs slices of several tiles: the two tests below."""
    x = normal_rows(300, 6, 4)
    x = x[np.argsort(-np.linalg.norm(x.astype(np.float64), axis=1))]
    xq = (0.05 * normal_rows(70, 6, 5)).astype(np.float32)
    sq = exact_sq(xq, x)
    assert np.all(sq[:, :64].min(axis=1) > sq[:, 64:128].min(axis=1)) and np.all(sq[:, 128:192].min(axis=1) > sq[:, 236:].min(axis=1))
    hs = np.array([0.1, 0.3, 1.0]) * neighbour_scale(sq)
    check("falling minima", xq, x, hs, None)
    check("rising minima", xq, x[::-1].copy(), hs, None)


def slices_of(m, n, d, b):
    """The number of column slices of a call, from the bytes the size function asks for ([slices][m] minima and
    [slices][b][m] sums of doubles, and 256)."""
    need = D()._lib.load().wm_kde_logsum_workspace_bytes(m, n, d + (-d) % 4, b)
    assert need > 256 and (need - 256) % (m * (1 + b) * 8) == 0
    return (need - 256) // (m * (1 + b) * 8)


def test_thread_rescale_when_a_slice_holds_several_tiles():
    """More than 1024 tiles, so a slice holds two column tiles and a thread carries sums from one tile into the next: the
    in-thread rescale `sum *= exp(-a (smin_old - smin_new))` with sums that are not zero, the reuse of the staging buffers
    by the second tile, and a short last slice (1025 column tiles: 512 slices of two and one of one).  40 query rows near
    the origin against 65 600 columns; the tiles alternate between the far half and the near half of the columns by
    distance from the origin, so in `far first` every thread's minimum drops at the second tile of its slice -- by far
    more than the bound resolves: a factor left out or inverted moves the far tile's terms by exp(a drop) -- and in `near
    first` it never does (sums carried on without a rescale)."""
    n = 65600
    x = normal_rows(n, 6, 9)
    x = x[np.argsort(-np.linalg.norm(x.astype(np.float64), axis=1))]
    tiles = np.arange(n).reshape(-1, 64)                       # 1025 tiles by falling norm
    far, near = tiles[:512], tiles[513:]
    order = np.concatenate([np.stack([far, near], axis=1).reshape(-1), tiles[512]])
    xq = (0.05 * normal_rows(40, 6, 10)).astype(np.float32)
    assert slices_of(40, n, 6, 3) == 513 < 1025
    for name, cols in (("far first", order), ("near first", np.concatenate([np.stack([near, far], axis=1).reshape(-1), tiles[512]]))):
        xs = np.ascontiguousarray(x[cols])
        sq = exact_sq(xq, xs)
        first, second = sq[:, :65536].reshape(40, 512, 2, 64)[:, :, 0].min(axis=2), sq[:, :65536].reshape(40, 512, 2, 64)[:, :, 1].min(axis=2)
        assert np.all(first > second) if name == "far first" else np.all(first < second)
        hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(sq)
        check(f"two tiles per slice, {name}", xq, xs, hs, None)


def test_square_matrix_beyond_1024_tiles():
    """m = n = 2112: 33 x 33 tiles, 17 slices (16 of two column tiles, the last of one), leave-one-out with the excluded
    column in either tile of a slice; the threads' minima drop or stay from the first tile to the second as the rows fall."""
    x = normal_rows(2112, 6, 11)
    assert slices_of(2112, 2112, 6, 3) == 17 < 33
    sq = exact_sq(x, x)
    hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(sq)
    check("n=2112 d=6 leave-one-out", x, x, hs, 0)


# ------------------------------------------------------------------------------------------------ exact rows and limits


def integer_rows():
    """70 rows of small integers (the float32 chain is exact) with duplicates in the same and in another column tile."""
    x = np.random.default_rng(7).integers(-6, 7, size=(70, 6)).astype(np.float32)
    x[5] = x[0]
    x[66] = x[1]
    x[67] = x[1]
    return x


def test_duplicates_count_and_the_self_does_not():
    x = integer_rows()
    sq = exact_sq(x, x)
    positive = sq[sq > 0].min()
    h = 1e-3 * math.sqrt(positive)
    a = float(D().scales_of(np.array([h]))[0])
    got, ref, bound = check("integer rows, tiny bandwidth", x, x, [h], 0, exact=True)
    off = np.where(np.eye(70, dtype=bool), np.inf, sq)
    smin = off.min(axis=1)
    mult = (off == smin[:, None]).sum(axis=1)
    assert list(mult[[0, 5, 1, 66, 67]]) == [1, 1, 2, 2, 2] and np.all(smin[[0, 5, 1, 66, 67]] == 0)
    want = -a * smin + np.log(mult)
    assert not np.isnan(got).any()
    parity("kde tiny bandwidth: -a s_min + log(multiplicity) / bound", float((np.abs(got[0] - want) / bound[0]).max()), 1.0)
    # with the self included a row of a duplicate pair counts two zeros, of the triple three
    full, _, _ = check("integer rows, tiny bandwidth, self included", x, x, [h], None, exact=True)
    assert np.allclose(full[0][[0, 5, 1, 66, 67]], np.log([2, 2, 3, 3, 3]), rtol=0, atol=1e-14)


def test_wide_bandwidth_counts_the_columns():
    x = integer_rows()
    sq = exact_sq(x, x)
    h = 1e3 * math.sqrt(sq.max())
    a = float(D().scales_of(np.array([h]))[0])
    got, ref, bound = check("integer rows, wide bandwidth", x, x, [h], 0, exact=True)
    # every term lies in [exp(-a s_max), 1]: log(n - 1) - a s_max <= L <= log(n - 1)
    assert np.all(got[0] <= math.log(69) + bound[0]) and np.all(got[0] >= math.log(69) - a * sq.max() - bound[0])
    assert a * sq.max() <= 5.1e-7


# ------------------------------------------------------------------------------------------------ (c) classes by offset


def test_offsets_on_a_label_sorted_matrix():
    """Per-class calls on the column ranges of a label-sorted matrix, each row left out of its own class: against the
    restatement, and their log-sum-exp over the classes against the ungrouped leave-one-out call."""
    dens = D()
    x = normal_rows(150, 6, 6)
    sizes = [70, 1, 79]  # the ranges cut column tiles; a class of one row
    sq = exact_sq(x, x)
    hs = np.array([0.3, 1.0, 4.0]) * neighbour_scale(sq)
    xd = dev(x)
    per_class, per_bound = [], []
    lo = 0
    for size in sizes:
        got = host(dens.gaussian_log_sums(xd, xd[lo:lo + size], hs, self_offset=lo))
        ref, bound = log_sum_reference(sq[:, lo:lo + size], dens.scales_of(hs), 6, lo)
        parity(f"kde class columns [{lo}, {lo + size}) / bound", worst(got, ref, bound), 1.0)
        per_class.append(got)
        per_bound.append(bound)
        lo += size
    assert per_class[1][0, 70] == -np.inf and np.isfinite(np.delete(per_class[1], 70, axis=1)).all()
    whole, _, whole_bound = check("ungrouped leave-one-out", x, x, hs, 0)
    stacked, stacked_bound = np.stack(per_class, axis=2), np.stack(per_bound, axis=2)
    joined = dens.host_logsumexp(stacked, axis=2)
    allowed = propagate(stacked, stacked_bound, axis=2) + whole_bound + 4 * U * np.abs(whole)
    parity("kde classes joined vs ungrouped / bound", float((np.abs(joined - whole) / allowed).max()), 1.0)


# ------------------------------------------------------------------------------------------------ (d) bits, buffers


def test_bits_and_buffers():
    dens = D()
    x = normal_rows(129, 6, 8)
    hs = np.array([0.2, 0.5, 1.0, 2.0, 4.0, 8.0]) * neighbour_scale(exact_sq(x, x))
    assert len(hs) > dens.MAX_BANDWIDTHS
    xd = dev(x)
    first = host(dens.gaussian_log_sums(xd, xd, hs, self_offset=0))
    assert np.array_equal(bits(first), bits(host(dens.gaussian_log_sums(xd, xd, hs, self_offset=0))))
    for q, h in enumerate(hs):
        alone = host(dens.gaussian_log_sums(xd, xd, [h], self_offset=0))
        assert np.array_equal(bits(alone[0]), bits(first[q])), q
    for part in ([0, 1], [1, 2, 3], [5, 0, 3, 2], [4, 4]):
        got = host(dens.gaussian_log_sums(xd, xd, hs[part], self_offset=0))
        assert np.array_equal(bits(got), bits(first[part])), part
    # sentinels behind out and behind the bytes the size function asked for
    lib = dens._lib.load()
    m, b = 129, 3
    need = lib.wm_kde_logsum_workspace_bytes(m, m, 8, b)
    assert need > 0
    ws = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    flat = torch.full((b * m + 64,), -7.25, dtype=torch.float64, device=DEV)
    out = flat[:b * m].view(b, m)
    back = dens.gaussian_log_sums(xd, xd, hs[:b], self_offset=0, out=out, ws=ws)
    assert back.data_ptr() == flat.data_ptr()
    assert np.array_equal(bits(host(out)), bits(first[:b]))
    assert bool((flat[b * m:] == -7.25).all()) and bool((ws[need:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ (e) end to end


_GOLDEN = {}


def golden():
    """512 golden rows with labels, their exact squared distances and, per bandwidth, the references and bounds of the
    full and the leave-one-out sums: computed once, read by the tests below and never changed."""
    if not _GOLDEN:
        dens = D()
        x, y = golden_rows(512), np.asarray(golden_labels(512)).astype(np.int64)
        sq = exact_sq(x, x)
        a = dens.scales_of(np.array(GOLDEN_H))
        _GOLDEN.update(x=x, y=y, sq=sq, full=log_sum_reference(sq, a, 512, None), loo=log_sum_reference(sq, a, 512, 0))
    return _GOLDEN


def test_golden_rows_against_sklearn():
    dens = D()
    g = golden()
    x, n = g["x"], 512
    (full_ref, full_bound), (loo_ref, loo_bound) = g["full"], g["loo"]
    parity("kde golden rows: largest score_samples bound (reference alone)", full_bound.max(), 1e-3)
    model = dens.KernelDensity(GOLDEN_H).fit(dev(x))
    scores, loo = model.score_samples(dev(x)), model.loo_score_samples()
    assert scores.shape == loo.shape == (6, n) and np.isfinite(loo).all()
    x64 = x.astype(np.float64)
    norm = dens.log_normaliser(GOLDEN_H, 512)
    # every row of the leave-one-out values against the restatement, inside its own bound
    want_loo = loo_ref - math.log(n - 1) - norm[:, None]
    parity("kde golden loo_score_samples, all rows vs restatement / bound",
           float((np.abs(loo - want_loo) / (loo_bound + 4 * U * np.abs(want_loo))).max()), 1.0)
    for q, h in enumerate(GOLDEN_H):
        want = sk_kde(h, x64).score_samples(x64)
        parity(f"kde golden score_samples h={h} / bound", float((np.abs(scores[q] - want) / (full_bound[q] + SKLEARN_SLACK)).max()), 1.0)
        refits = [abs(loo[q, i] - sk_kde(h, np.delete(x64, i, axis=0)).score_samples(x64[i:i + 1])[0]) / (loo_bound[q, i] + SKLEARN_SLACK)
                  for i in LOO_REFITS]
        parity(f"kde golden loo_score_samples h={h}, {len(refits)} rows vs sklearn refits / bound", max(refits), 1.0)
    ll = model.loo_log_likelihood()
    assert model.best().bandwidth_ == GOLDEN_H[int(np.argmax(ll))]
    one = dens.KernelDensity(GOLDEN_H[2]).fit(dev(x))
    assert np.array_equal(bits(one.score_samples(dev(x))), bits(scores[2])) and np.array_equal(bits(model[2].loo_score_samples()[0]), bits(loo[2]))


def test_golden_uniformity_and_alignment():
    dens = D()
    x = golden()["x"]
    z = host(dens.normalize_rows(dev(x)))  # float32, rounded once: what the kernel reads
    assert z.dtype == np.float32 and np.abs(np.linalg.norm(z.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    n = z.shape[0]
    ref, bound = log_sum_reference(exact_sq(z, z), [2.0], 512, 0)
    allowed = propagate(ref[0], bound[0]) + (2 * n + 16) * U + 4 * U * abs(math.log(n * (n - 1.0)))
    got = dens.uniformity(dev(x), t=2.0)
    want = uniformity_formula(z, 2.0)
    parity("kde uniformity(t=2) golden rows / bound", abs(got - want) / allowed, 1.0)
    assert np.array_equal(dens.uniformity(dev(x), t=[1.0, 2.0])[1], got)
    # alignment: the all-pairs kernels' distance, relative error (d + 3) 2^-24 per pair, to the power alpha = 2
    other = host(dens.normalize_rows(dev(np.roll(x, 1, axis=0))))
    want = float(np.mean(np.sum((z.astype(np.float64) - other.astype(np.float64)) ** 2, axis=1)))
    got = dens.alignment(dev(x), dev(np.roll(x, 1, axis=0)))
    parity("kde alignment golden rows / bound", abs(got - want) / (want * (2 * 515 * 2.0 ** -24 + 2.0 ** -23)), 1.0)


def test_golden_classifier_leave_one_out():
    """loo_predict_proba against Bayes' rule, written out in log space on the exact distances.  Every class's log-sum moves by at most its
    bound b_c (a) + (b); the joint log-probabilities move by the same, their normaliser by (c), so log p_c moves by at
    most b_c + propagate(b) and p_c by p_c (exp(that) - 1); labels must agree where the reference margin between the
    two best classes exceeds the two's bounds."""
    dens = D()
    g = golden()
    x, y, sq = g["x"], g["y"], g["sq"]
    hs = GOLDEN_H[1:4]
    clf = dens.KDEClassifier(hs).fit(dev(x), y)
    proba = clf.loo_predict_proba()
    assert proba.shape == (3, 512, clf.classes_.size) and not np.isnan(proba).any()
    a = dens.scales_of(np.array(hs))
    compared = 0
    classes, counts = np.unique(y, return_counts=True)
    assert np.array_equal(classes, clf.classes_)
    for q, h in enumerate(hs):
        # Bayes' rule in log space (the plain exponentials of bayes_log_posterior underflow in 512 dimensions)
        joint, b = np.empty((512, classes.size)), np.empty((512, classes.size))
        for k, c in enumerate(classes):
            cols = np.flatnonzero(y == c)
            own = cols[None, :] == np.arange(512)[:, None]
            # the class's columns, the row's own column masked by an infinite distance
            ref, bound = log_sum_reference(np.where(own, np.inf, sq[:, cols]), a[q:q + 1], 512)
            joint[:, k] = ref[0] - np.log(counts[k] - own.sum(axis=1)) + math.log(counts[k] / 512.0)
            b[:, k] = bound[0]
        want = joint - dens.host_logsumexp(joint, axis=1)[:, None]
        move = b + propagate(want, b, axis=1)[:, None] + 8 * U * (1.0 + np.abs(want))
        with np.errstate(invalid="ignore"):
            allowed = np.exp(want) * np.expm1(move) + 4 * U
        parity(f"kde loo_predict_proba h={h} / bound", float((np.abs(proba[q] - np.exp(want)) / allowed).max()), 1.0)
        top2 = np.sort(want, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > 2 * move.max(axis=1)
        assert np.array_equal(clf.loo_predict()[q][sure], classes[np.argmax(want, axis=1)][sure])
        compared += int(sure.sum())
    assert compared >= 3 * 500  # the margins are far above the bounds on nearly every row


# ------------------------------------------------------------------------------------------------ the script


def test_script_on_a_few_hundred_golden_rows(tmp_path):
    """scripts/embedding_density_amd.py end to end, in process: a list of bandwidths with --pca, --holdout and --by-class
    (files, shapes and what they must agree on), then a rule-of-thumb bandwidth without scaling, whose leave-one-out and
    held-out log densities are held to the restatement and to sklearn at their bounds."""
    import csv
    import json
    from pathlib import Path

    from scripts.embedding_density_amd import main

    golden_file = str(Path(__file__).resolve().parent / "golden" / "simsiam_preds_subset.npz")
    out = tmp_path / "listed"
    summary = main(["--embeddings", golden_file, "--rows", "300", "--holdout", "40", "--pca", "20", "--by-class",
                    "--bandwidths", "0.5:8:5", "--contamination", "0.1", "--out", str(out)])
    trials = list(csv.DictReader(open(out / "trials.csv")))
    assert len(trials) == 5 and set(trials[0]) == {"bandwidth", "loo_log_likelihood", "loo_mean_log_density", "loo_accuracy", "loo_macro_f1"}
    ll = np.array([float(t["loo_log_likelihood"]) for t in trials])
    assert np.isfinite(ll).all() and summary["chosen_bandwidth"] == float(trials[int(np.argmax(ll))]["bandwidth"])
    assert all(0.0 <= float(t["loo_macro_f1"]) <= float(t["loo_accuracy"]) <= 1.0 for t in trials)
    dens, flagged, hold = np.load(out / "log_density.npy"), np.load(out / "flagged.npy"), np.load(out / "holdout_log_density.npy")
    assert dens.shape == (260,) and hold.shape == (40,) and np.isfinite(dens).all() and np.isfinite(hold).all()
    assert np.array_equal(flagged, np.argsort(dens, kind="stable")[:26]) and summary["threshold"] == dens[flagged[-1]]
    assert summary["holdout_below_threshold"] == int((hold < summary["threshold"]).sum()) and summary["d"] == 20
    assert summary["uniformity"] < 0.0 and json.loads((out / "summary.json").read_text()) == summary
    assert set(summary["mean_log_density_per_class"]) == set(summary["flagged_per_class"])

    out = tmp_path / "rule"
    summary = main(["--embeddings", golden_file, "--rows", "200", "--holdout", "30", "--no-scale", "--bandwidths", "scott", "--out", str(out)])
    emb = np.load(golden_file)["embeddings"].astype(np.float32)[:200]
    fit, new = emb[:170], emb[170:]
    h = D().rule_of_thumb("scott", 170, 512)
    assert summary["bandwidths"] == [h] == [summary["chosen_bandwidth"]] and not summary["chosen_at_an_end"]
    a, norm = D().scales_of(np.array([h])), float(D().log_normaliser([h], 512)[0])
    ref, bound = log_sum_reference(exact_sq(fit, fit), a, 512, 0)
    got = np.load(out / "log_density.npy")
    parity("kde script: leave-one-out log density vs restatement / bound",
           float((np.abs(got - (ref[0] - math.log(169) - norm)) / (bound[0] + 4 * U * np.abs(ref[0] - norm))).max()), 1.0)
    _, bound = log_sum_reference(exact_sq(new, fit), a, 512)
    want = sk_kde(h, fit).score_samples(new.astype(np.float64))
    parity("kde script: held-out log density vs sklearn / bound",
           float((np.abs(np.load(out / "holdout_log_density.npy") - want) / (bound[0] + SKLEARN_SLACK)).max()), 1.0)
