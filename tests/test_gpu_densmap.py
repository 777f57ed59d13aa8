"""GPU checks of the DensMAP kernels (csrc/umap.hip: wm_densmap_graph_radii, wm_densmap_embedding_radii,
wm_densmap_layout) and their Python layer (manifold.DensMAP, scripts/embedding_umap_amd.py --densmap) against the
float64 reference of tests/test_densmap_cpu.py.

Bounds are derived, not tuned; u = 2^-24, t = 2^-40.
  double work     the radii and statistics kernels work in double on float32 inputs.  A row's sums have positive terms
                  only; a term takes at most dim + 12 double operations and a library pow (a few ulp), a row at most a
                  few hundred terms, a sum over the vertices at most 2^24 of them: every relative error (absolute, for
                  a logarithm or a mean of mixed signs, in units of the largest |element|) stays below 2^24 * 2^-53 *
                  2^8 < t.  numpy's own pairwise sums are inside the same figure.
  graph radii     ro: the argument of the logarithm within 2 t relative, so the logarithm within 2 t absolute; ONE
                  rounding to float32: u |ro| + 4 t.
  embedding radii D: one rounding of a positive sum: (u + t) D, and exactly 0 for a row without live entries;
                  re: one rounding: u |re| + 4 t.
  per-vertex      1 / D and 1 / (eps + N / D): one rounding each: (u + 4 t) of the value.  W = R - cov (re - mean) /
  values          std^2: re, mean and cov carry absolute errors of a few t (times the largest |re|, |re R|), so the
                  second part is off by at most 64 t (1 + |cov| (|re| + |mean|) / std^2); ONE rounding: u |W|.
                  mean, var and cov themselves (double): 64 t (1 + max |re|)^2 (1 + max |R|).
                  s = dens_lambda mu_tot / (std n): one rounding, (u + 64 t) s.
  density layout  see `densmap_bound`.
"""
import importlib.util
import json

import numpy as np
import pytest
import torch
from parity_log import parity

from test_densmap_cpu import (pearson, ref_densmap_fit, ref_density_epoch, ref_density_terms, ref_embedding_radii, ref_graph_dists,
                              ref_graph_radii, ref_live, ref_phase)
from test_gpu_umap import AB, GOLDEN, LAYOUT_SHAPES, ROOT, U, bits, dev, layout_case, rows
from test_gpu_umap import wafer_rows  # noqa: F401  (the fixture: 1 500 standardised golden rows)
from test_umap_cpu import ref_alpha, ref_layout_epoch

pytestmark = pytest.mark.gpu

T = 2.0 ** -40
LOG_EPS = float(np.log(1e-8))


def frac_of(got, want, bound):
    """Largest |got - want| / bound; where the bound is 0 the two must be equal."""
    got, want, bound = (np.asarray(v, dtype=np.float64) for v in (got, want, bound))
    assert np.isfinite(got).all()
    zero = bound == 0
    assert (got[zero] == want[zero]).all()
    return float((np.abs(got - want)[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def case_weights(q):
    """Weights in keeping with the rates (q = rint(65536 w / max w)), symmetric like q and positive: float32."""
    return (np.maximum(q, 1) / 65536.0).astype(np.float32)


def case_radii(n, seed):
    """Radii for the kernel tests: float32 normal about 1, both signs among them.  (Not standardised: to the kernels R
    is an input like any other, and a standardised pair of two vertices sums to 0, which would switch the term off.)"""
    return (1.0 + np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ graph radii


@pytest.mark.parametrize("k", [2, 15])
@pytest.mark.parametrize("n", [2, 65, 300])
def test_graph_radii_against_float64(n, k):
    """dists bit-equal to scipy's dmat.maximum(dmat.T) at the graph's entries (a float32 maximum is exact); ro within
    u |ro| + 4 t of the float64 formula: double inside, 1 rounding to float32."""
    from ssl_wafermap_amd import manifold

    k = min(k, n)
    xd = dev(rows(n, 8, 31 * n + k))
    graph, dists = manifold.fuzzy_simplicial_set(xd, k, return_dists=True)
    plain = manifold.fuzzy_simplicial_set(xd, k)
    assert all(np.array_equal(bits(p), bits(g)) for p, g in zip(plain, graph)), "return_dists must not change the graph"
    assert dists.dtype == torch.float32 and dists.shape == graph.data.shape and dists.is_cuda
    dist_t, idx_t = manifold.knn_graph(xd, k)
    want_d = ref_graph_dists(dist_t.cpu().numpy(), idx_t.cpu().numpy(), graph.to_scipy())
    assert np.array_equal(dists.cpu().numpy().astype(np.float64), want_d)
    q = manifold.sample_rates(graph.data)
    for n_epochs in (20, 500):
        ro = manifold.graph_radii(graph.indptr, graph.data, dists, q, n_epochs)
        assert ro.dtype == torch.float32 and ro.shape == (n,)
        want = ref_graph_radii(graph.indptr.cpu().numpy(), graph.data.cpu().numpy(), want_d, q.cpu().numpy(), n_epochs)
        parity(f"densmap graph radii n={n} k={k} epochs={n_epochs} (fraction of the bound)",
               frac_of(ro.cpu().numpy(), want, U * np.abs(want) + 4 * T), 1.0)
        assert np.array_equal(bits(ro), bits(manifold.graph_radii(graph.indptr, graph.data, dists, q, n_epochs)))


def test_graph_radii_skip_entries_that_are_not_live():
    """A hand-made graph at n_epochs = 20: rates 0 and 1 are never sampled (1 * 20 < 65536), row 2 has only such entries
    and row 3 none at all: both get log 1e-8, and row 0's dead entry takes no part in its mean."""
    from ssl_wafermap_amd import manifold

    indptr = np.array([0, 3, 5, 7, 7, 8], dtype=np.int32)
    q = np.array([65536, 1, 40000, 65536, 3277, 0, 1, 3276], dtype=np.int32)
    data = np.array([1.0, 0.5, 0.6, 1.0, 0.05, 0.3, 0.2, 0.05], dtype=np.float32)
    dists = np.array([2.0, 100.0, 3.0, 2.0, 0.0, 5.0, 7.0, 9.0], dtype=np.float32)
    assert ref_live(q, 20).tolist() == [True, False, True, True, True, False, False, False]
    ro = manifold.graph_radii(dev(indptr), dev(data), dev(dists), dev(q), 20).cpu().numpy()
    want = ref_graph_radii(indptr, data, dists, q, 20)
    assert want[2] == want[3] == want[4] == LOG_EPS and abs(want[0] - np.log((4.0 + 0.6 * 9.0) / 1.6)) < 1e-6
    parity("densmap graph radii, hand-made graph (fraction of the bound)", frac_of(ro, want, U * np.abs(want) + 4 * T), 1.0)
    assert ro[2] == ro[3] == ro[4] == np.float32(LOG_EPS)
    with pytest.raises(ValueError):
        manifold.graph_radii(dev(indptr), dev(data), dev(dists[:-1]), dev(q), 20)


# ------------------------------------------------------------------------------------------------ embedding radii, statistics


def check_terms(name, terms, y, indptr, indices, q, data, rad, a, b, n_epochs, lam, shift):
    """The per-vertex values and scalars of one phase epoch against float64 at the positions y."""
    re, big_d, ratio = ref_embedding_radii(y, indptr, indices, q, a, b, n_epochs)
    mu_tot = float(np.asarray(data, dtype=np.float64)[ref_live(q, n_epochs)].sum())
    want = ref_density_terms(re, big_d, ratio, rad, mu_tot, lam, shift)
    worst = max(
        frac_of(terms.inv_d.cpu().numpy(), want["inv_d"], (U + 4 * T) * want["inv_d"]),
        frac_of(terms.inv_den.cpu().numpy(), want["inv_den"], (U + 4 * T) * want["inv_den"]),
        frac_of(terms.re.cpu().numpy(), re, U * np.abs(re) + 4 * T),
        frac_of(terms.w.cpu().numpy(), want["w"], U * np.abs(want["w"]) + 64 * T * (
            1 + np.abs(want["cov"]) * (np.abs(re) + abs(want["mean"])) / want["std"] ** 2)),
        frac_of([terms.scale], [want["scale"]], [(U + 64 * T) * want["scale"]]),
        frac_of([terms.mu_tot, terms.std], [mu_tot, want["std"]], [64 * T * mu_tot, 64 * T * want["std"]]),
        frac_of([terms.mean, terms.var, terms.cov], [want["mean"], want["var"], want["cov"]],
                [64 * T * (1 + np.abs(re).max()) ** 2 * (1 + np.abs(rad).max())] * 3))
    parity(f"densmap per-vertex values {name} (fraction of the bound)", worst, 1.0)


@pytest.mark.parametrize("n,dim", LAYOUT_SHAPES)
def test_embedding_radii_against_float64(n, dim):
    """D and re: double inside, 1 rounding to float32 each; the four per-vertex values and s of a phase epoch: formed
    in double from the double-precision radii, 1 rounding each.  The graph has an isolated vertex (D = 0 exactly,
    re = log 1e-8), a coincident pair (r = 0 adds 1 to D and nothing to N) and rates 1 and 0 (not live at 20 epochs)."""
    from ssl_wafermap_amd import manifold

    a, b = AB[(n + dim) % 2]
    n_epochs, lam, shift = 20, 1.0, 0.1
    indptr, indices, q, y0 = layout_case(n, dim, 17 * n + dim)
    ip, ix, qd, yd = dev(indptr), dev(indices), dev(q), dev(y0)
    re_t, d_t = manifold.embedding_radii(yd, ip, ix, qd, a, b, n_epochs)
    assert re_t.dtype == d_t.dtype == torch.float32 and re_t.shape == d_t.shape == (n,)
    re, big_d, _ = ref_embedding_radii(y0, indptr, indices, q, a, b, n_epochs)
    if n > 2:
        assert big_d[n - 1] == 0 and re[n - 1] == LOG_EPS and not ref_live(q, n_epochs).all()
    parity(f"densmap embedding radii D n={n} dim={dim} (fraction of the bound)", frac_of(d_t.cpu().numpy(), big_d, (U + T) * big_d), 1.0)
    parity(f"densmap embedding radii re n={n} dim={dim} (fraction of the bound)",
           frac_of(re_t.cpu().numpy(), re, U * np.abs(re) + 4 * T), 1.0)
    again = manifold.embedding_radii(yd, ip, ix, qd, a, b, n_epochs)
    assert np.array_equal(bits(re_t), bits(again[0])) and np.array_equal(bits(d_t), bits(again[1]))
    data, rad = case_weights(q), case_radii(n, n + dim)
    _, terms = manifold.optimize_layout_densmap(yd, ip, ix, qd, dev(data), dev(rad), a, b, n_epochs, 0, 1, dens_lambda=lam,
                                                dens_frac=1.0, dens_var_shift=shift, return_terms=True)
    assert np.array_equal(bits(terms.re), bits(re_t)), "the layout's radii are embedding_radii's"
    check_terms(f"n={n} dim={dim}", terms, y0, indptr, indices, q, data, rad, a, b, n_epochs, lam, shift)
    # dens_var_shift = 0 on coincident radii: std = 0, no density force and W = R
    if n == 2:
        _, flat = manifold.optimize_layout_densmap(yd, ip, ix, qd, dev(data), dev(rad), a, b, n_epochs, 0, 1, dens_lambda=lam,
                                                   dens_frac=1.0, dens_var_shift=0.0, return_terms=True)
        assert flat.std == 0 and flat.scale == 0 and np.array_equal(bits(flat.w), rad.view(np.int32))


def test_statistics_beyond_one_stride():
    """40 000 vertices on a ring with chords: more than 128 blocks of 256, so every thread of the statistics kernels
    adds more than one element and every slot is used (the smaller cases use one or two slots)."""
    from ssl_wafermap_amd import manifold

    n, dim, n_epochs, lam, shift = 40000, 2, 20, 2.0, 0.1
    a, b = AB[0]
    rng = np.random.default_rng(5)
    i = np.arange(n)
    pairs = np.unique(np.sort(np.concatenate([np.stack([i, (i + 1) % n], 1), np.stack([i, (7 * i + 3) % n], 1)]), axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    rate = rng.integers(0, 65537, pairs.shape[0])
    head = np.concatenate([pairs[:, 0], pairs[:, 1]])
    tail = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((tail, head))
    indices, q = tail[order].astype(np.int32), np.concatenate([rate, rate])[order].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(head, minlength=n))]).astype(np.int32)
    assert indices.size > 128 * 256
    y0 = (3.0 * rng.standard_normal((n, dim))).astype(np.float32)
    data, rad = case_weights(q), case_radii(n, 6)
    _, terms = manifold.optimize_layout_densmap(dev(y0), dev(indptr), dev(indices), dev(q), dev(data), dev(rad), a, b, n_epochs, 0, 1,
                                                dens_lambda=lam, dens_frac=1.0, dens_var_shift=shift, return_terms=True)
    check_terms(f"n={n} dim={dim}", terms, y0, indptr, indices, q, data, rad, a, b, n_epochs, lam, shift)


# ------------------------------------------------------------------------------------------------ layout


def densmap_bound(y_ref, mag, dens_mag, pieces, alpha, deg, dim, b, rate):
    """`layout_bound` of tests/test_gpu_umap.py extended by the density term of a phase epoch, whose float32
    arithmetic the header of csrc/umap.hip states.  Roundings of one density term in units of u, with e_r = 3 + L and
    e_p = b e_r + P (P = 4) as there:
      a p + 1: e_p + 2;   phi = 1 / (a p + 1): e_phi = e_p + 3;
      t1 = fma(b, phi, float32(1 - b)): two positive parts, e_phi + 2;   t1 * invden_v: e_phi + 3;
      t2 = (float32(ab) p) / (r (a p + 1)): ab 1, product 1, p; r (a p + 1): e_r, e_p + 2, product 1; quotient 1:
        2 e_p + e_r + 7;   the sum of the two positive parts: 2 e_p + e_r + 8;
      phi * invD_v: e_phi + 1;   dr_v, their product: 3 e_p + e_r + 13;
      W_i dr_i + W_j dr_j: a product each and the sum, relative to |W_i dr_i| + |W_j dr_j| because the two can cancel: 2;
      times s: 1; over w_e: 1; the doubling is exact; d_c: 1; times d_c: 1 -- E_d = (3 b + 1) e_r + 3 P + 19.
    (The per-vertex values, s and w_e are the kernel's own float32 inputs: the reference epoch takes them as given.)
    clip is 1-Lipschitz, so a density term is off by at most E_d u times `pieces`, the unclipped term with the two pieces
    taken absolutely.  A lane now adds 2 + R terms per pass: N = ceil(deg / EPP)(2 + R) + EPP additions, each off by at
    most u times the sum of all |terms|, the density terms among them.
      |error| <= 1.01 u [alpha (E sum|plain terms| + E_d pieces + (N + 1) sum|all terms|) + |y'|]"""
    dp = 1 << int(np.ceil(np.log2(dim)))
    e_r = 3 + np.log2(dp)
    big_e = (2 * b + 1) * e_r + 2 * 4 + 10
    e_d = (3 * b + 1) * e_r + 3 * 4 + 19
    epp = 64 // dp
    adds = np.ceil(deg / epp) * (2 + rate) + epp
    return 1.01 * U * (alpha * (big_e * mag + e_d * pieces + (adds[:, None] + 1) * (mag + dens_mag)) + np.abs(y_ref))


@pytest.mark.parametrize("n,dim", LAYOUT_SHAPES)
def test_density_layout_teacher_forced_against_float64(n, dim):
    """20 epochs, one call each, with dens_frac 1.0 and 0.3; after every epoch the kernel's positions against one
    float64 reference epoch (plain terms + density terms) started from the kernel's own previous positions and, for
    the density terms, the kernel's own float32 per-vertex values and s (checked on their own above).  Then, in bits:
    [0, 20) = [0, 7) + [7, 20) = a second run; dens_lambda = 0 is optimize_layout; the epochs before the phase are
    optimize_layout's.  dens_lambda = 100 so that density terms clip at every shape and in both phases (in 50 and 64
    dimensions a component of y_i - y_j is small; a float64 run of these cases clips 12 .. 5 000 of them per phase)."""
    from ssl_wafermap_amd import manifold

    a, b = AB[(n + dim) % 2]
    gamma, lr, seed, rate, epochs, lam, shift = 1.0, 1.0, 1234 + n, 5, 20, 100.0, 0.1
    indptr, indices, q, y0 = layout_case(n, dim, 17 * n + dim)
    data, rad = case_weights(q), case_radii(n, n + dim)
    ip, ix, qd, wd, rd = dev(indptr), dev(indices), dev(q), dev(data), dev(rad)
    deg = np.diff(indptr).astype(np.float64)
    kw = dict(gamma=gamma, learning_rate=lr, seed=seed, negative_sample_rate=rate)
    plain = manifold.optimize_layout(dev(y0), ip, ix, qd, a, b, epochs, **kw)
    for frac in (1.0, 0.3):
        dkw = dict(kw, dens_lambda=lam, dens_frac=frac, dens_var_shift=shift)
        y = dev(y0)
        worst, clipped, hits, phase_epochs = 0.0, 0, 0, 0
        for ep in range(epochs):
            nxt, terms = manifold.optimize_layout_densmap(y, ip, ix, qd, wd, rd, a, b, epochs, ep, ep + 1, return_terms=True, **dkw)
            prev = y.cpu().numpy()
            alpha = ref_alpha(lr, ep, epochs)
            ref, mag, hit, _ = ref_layout_epoch(prev, indptr, indices, q, a, b, gamma, alpha, seed, ep, rate)
            dens_mag = pieces = np.zeros_like(mag)
            assert (terms is not None) == ref_phase(ep, epochs, lam, frac)
            if terms is not None:
                mine = dict(inv_d=terms.inv_d.cpu().numpy(), inv_den=terms.inv_den.cpu().numpy(), w=terms.w.cpu().numpy(),
                            scale=terms.scale)
                delta, dens_mag, pieces, clip = ref_density_epoch(prev, indptr, indices, q, data, a, b, alpha, ep, mine)
                ref = ref + delta
                clipped += clip
                hits += int(hit.sum())
                phase_epochs += 1
            got = nxt.cpu().numpy()
            assert np.isfinite(got).all()
            bound = densmap_bound(ref, mag, dens_mag, pieces, alpha, deg, dim, b, rate)
            worst = max(worst, float((np.abs(got - ref) / bound).max()))
            y = nxt
        assert phase_epochs == (20 if frac == 1.0 else 6)
        assert hits > 0 and clipped > 0, "the case must sample entries in the phase and clip density terms"
        parity(f"densmap layout n={n} dim={dim} dens_frac={frac} (fraction of the bound)", worst, 1.0)
        whole = manifold.optimize_layout_densmap(dev(y0), ip, ix, qd, wd, rd, a, b, epochs, 0, epochs, **dkw)
        part = manifold.optimize_layout_densmap(dev(y0), ip, ix, qd, wd, rd, a, b, epochs, 0, 7, **dkw)
        part = manifold.optimize_layout_densmap(part, ip, ix, qd, wd, rd, a, b, epochs, 7, epochs, **dkw)
        assert np.array_equal(bits(whole), bits(part)) and np.array_equal(bits(whole), bits(y))
        assert np.array_equal(bits(whole), bits(manifold.optimize_layout_densmap(dev(y0), ip, ix, qd, wd, rd, a, b, epochs, **dkw)))
        assert not np.array_equal(bits(whole), bits(plain)), "the density term must move something"
        if n > 2:
            assert np.array_equal(bits(whole)[n - 1], y0.view(np.int32)[n - 1])  # (the isolated vertex)
    off = manifold.optimize_layout_densmap(dev(y0), ip, ix, qd, wd, rd, a, b, epochs, **dict(kw, dens_lambda=0.0, dens_frac=1.0))
    assert np.array_equal(bits(off), bits(plain)), "dens_lambda = 0 is the plain layout"
    before = manifold.optimize_layout_densmap(dev(y0), ip, ix, qd, wd, rd, a, b, epochs, 0, 14,
                                              **dict(kw, dens_lambda=lam, dens_frac=0.3, dens_var_shift=shift))
    assert np.array_equal(bits(before), bits(manifold.optimize_layout(dev(y0), ip, ix, qd, a, b, epochs, 0, 14, **kw)))


def test_densmap_layout_validates_its_arguments():
    from ssl_wafermap_amd import manifold

    indptr, indices, q, y0 = layout_case(65, 2, 1)
    args = [dev(y0), dev(indptr), dev(indices), dev(q), dev(case_weights(q)), dev(case_radii(65, 0)), 1.5, 0.9, 10]
    for bad in ({"dens_lambda": -1.0}, {"dens_frac": -0.1}, {"dens_frac": 1.5}, {"dens_var_shift": -0.1}, {"epoch_end": 11},
                {"negative_sample_rate": 65}):
        with pytest.raises(ValueError):
            manifold.optimize_layout_densmap(*args, **bad)
    zero = case_weights(q)
    zero[0] = 0.0
    with pytest.raises(ValueError):
        manifold.optimize_layout_densmap(*(args[:4] + [dev(zero)] + args[5:]))
    with pytest.raises(ValueError):
        manifold.optimize_layout_densmap(*(args[:5] + [dev(case_radii(64, 0))] + args[6:]))


# ------------------------------------------------------------------------------------------------ end to end


def test_fit_preserves_density_like_the_float64_reference(wafer_rows):  # noqa: F811
    """k = 15, 2-D, init="random", 200 epochs, dens_lambda = 1 on 1 500 standardised golden rows.  The Pearson
    correlation of rad_orig_ and rad_emb_ must reach the float64 reference's at seed 0 minus 0.05, and sklearn's
    trustworthiness(15) the reference's minus 0.02: each margin is three times the spread the issue's prototype measured
    over seeds 0 - 2 (0.016 and 0.006).  The committed reference (tests/test_densmap_cpu.py: ref_densmap_fit) gives, for
    seeds 0, 1, 2: correlation 0.9365, 0.9474, 0.9467 and trustworthiness 0.9651, 0.9712, 0.9741 (0.8 % of the density
    term components clip); with dens_lambda = 0 at seed 0: 0.0584 and 0.9880.  (The prototype's table: 0.929 - 0.945 and
    0.9635 - 0.9697; plain 0.06 - 0.09.)  Plain manifold.UMAP on the same rows, scored with embedding_radii, must stay
    below the correlation bound: the bound discriminates.  Two fits give the same bits.  Measured on the MI355X:
    correlation 0.9256 and trustworthiness 0.9605 against the reference's 0.9374 and 0.9651 computed beside it (the layout
    is chaotic: the reference itself moves in the third digit between two hosts); plain UMAP: 0.1015."""
    from sklearn.manifold import trustworthiness

    from ssl_wafermap_amd import manifold

    x, _ = wafer_rows
    kw = dict(n_neighbors=15, n_components=2, init="random", n_epochs=200, random_state=0)
    model = manifold.DensMAP(dens_lambda=1.0, **kw)
    got = model.fit_transform(dev(x))
    assert got.shape == (1500, 2) and got.dtype == torch.float32 and got.is_cuda and model.embedding_ is got
    for rad in (model.rad_orig_, model.rad_emb_):
        assert rad.shape == (1500,) and rad.dtype == torch.float32 and rad.is_cuda and bool(torch.isfinite(rad).all())
    ref_y, ref_ro, ref_re, _ = ref_densmap_fit(x, 15, 2, model.a_, model.b_, 200, 0, 1.0)
    c_ref, t_ref = pearson(ref_ro, ref_re), trustworthiness(x, ref_y, n_neighbors=15)
    c_got = pearson(model.rad_orig_.cpu().numpy(), model.rad_emb_.cpu().numpy())
    t_got = trustworthiness(x, got.cpu().numpy(), n_neighbors=15)
    print(f"densmap 1500 rows: correlation {c_got:.4f} (reference {c_ref:.4f}), trustworthiness {t_got:.4f} (reference {t_ref:.4f})")
    g = model.graph_
    q = manifold.sample_rates(g.data)
    flat = manifold.UMAP(**kw).fit_transform(dev(x))
    c_flat = pearson(model.rad_orig_.cpu().numpy(),
                     manifold.embedding_radii(flat, g.indptr, g.indices, q, model.a_, model.b_, 200)[0].cpu().numpy())
    print(f"plain UMAP on the same rows: correlation {c_flat:.4f}")
    parity("densmap radii correlation, 1500 golden rows (bound: float64 reference - 0.05)", c_got, c_ref - 0.05, higher=True,
           note=f"float64 reference {c_ref:.4f}")
    parity("densmap trustworthiness(15), 1500 golden rows (bound: float64 reference - 0.02)", t_got, t_ref - 0.02, higher=True,
           note=f"float64 reference {t_ref:.4f}")
    parity("plain UMAP radii correlation stays below the densmap bound", c_flat, c_ref - 0.05)
    again = manifold.DensMAP(dens_lambda=1.0, **kw).fit(dev(x))
    assert np.array_equal(bits(got), bits(again.embedding_)) and np.array_equal(bits(model.rad_emb_), bits(again.rad_emb_))
    assert np.array_equal(bits(model.rad_orig_), bits(again.rad_orig_))


def test_densmap_reduction_hands_over_to_hdbscan(wafer_rows):  # noqa: F811
    """Notebook 3.2's flow: DensMAP(n_neighbors=30, n_components=50, min_dist=0, dens_lambda=0.1) -> HDBSCAN.  The
    radii correlation exceeds plain UMAP's on the same rows by at least 0.5 (float64 prototype, one seed: 0.79 against
    -0.23)."""
    from ssl_wafermap_amd import cluster, manifold

    x = wafer_rows[0][:600]
    kw = dict(n_neighbors=30, n_components=50, min_dist=0.0)
    model = manifold.DensMAP(dens_lambda=0.1, **kw)
    reduced = model.fit_transform(dev(x))
    assert reduced.shape == (600, 50) and bool(torch.isfinite(reduced).all())
    c_dens = pearson(model.rad_orig_.cpu().numpy(), model.rad_emb_.cpu().numpy())
    g = model.graph_
    flat = manifold.UMAP(**kw).fit_transform(dev(x))
    re_flat = manifold.embedding_radii(flat, g.indptr, g.indices, manifold.sample_rates(g.data), model.a_, model.b_, 700)[0]
    c_flat = pearson(model.rad_orig_.cpu().numpy(), re_flat.cpu().numpy())
    parity("densmap 3.2 flow: radii correlation over plain UMAP's (bound: + 0.5)", c_dens - c_flat, 0.5, higher=True,
           note=f"densmap {c_dens:.4f}, plain {c_flat:.4f}")
    labels = cluster.HDBSCAN(min_cluster_size=15).fit_predict(reduced)
    assert labels.shape == (600,) and labels.max() + 1 >= 2


def test_umap_script_with_densmap(tmp_path):
    spec = importlib.util.spec_from_file_location("embedding_umap_amd", ROOT / "scripts" / "embedding_umap_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    summary = mod.main(["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "600", "--epochs", "100", "--densmap",
                        "--out", str(tmp_path)])
    z = np.load(tmp_path / "reduced.npz")
    assert set(z.files) == {"embeddings", "labels", "rad_orig", "rad_emb"}
    assert z["embeddings"].shape == (600, 2) and z["embeddings"].dtype == np.float32 and z["labels"].shape == (600,)
    assert z["rad_orig"].shape == z["rad_emb"].shape == (600,) and z["rad_orig"].dtype == z["rad_emb"].dtype == np.float32
    assert all(np.isfinite(z[k]).all() for k in ("embeddings", "rad_orig", "rad_emb")) and (tmp_path / "umap.png").stat().st_size > 0
    on_disk = json.loads((tmp_path / "summary.json").read_text())
    assert on_disk["densmap"] is True and on_disk["dens_lambda"] == 2.0 and on_disk["n_epochs"] == 100
    assert on_disk["radii_correlation"] == summary["radii_correlation"]
    assert abs(on_disk["radii_correlation"] - pearson(z["rad_orig"], z["rad_emb"])) < 1e-12
    assert 0.5 <= on_disk["radii_correlation"] <= 1.0  # (plain UMAP sits near 0.06; the float64 reference at 600 rows, 100 epochs, lambda 2: 0.947 - 0.963)
    assert {"knn_graph", "fuzzy_set", "init", "graph_radii", "layout"} <= set(on_disk["seconds"])
    # without --densmap the outputs are what they were
    mod.main(["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "600", "--epochs", "100", "--out", str(tmp_path / "p")])
    assert set(np.load(tmp_path / "p" / "reduced.npz").files) == {"embeddings", "labels"}
    assert "radii_correlation" not in json.loads((tmp_path / "p" / "summary.json").read_text())
