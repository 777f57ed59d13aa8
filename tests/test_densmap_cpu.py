"""CPU checks of the DensMAP host code (ssl_wafermap_amd.manifold.DensMAP and its steps): the density phase, the epoch
default, argument validation and the refusals.  No GPU: nothing here launches a kernel.  The float64 reference of the
density term that the GPU tests compare against (tests/test_gpu_densmap.py) lives here, built on the UMAP reference of
tests/test_umap_cpu.py, so that its own pieces -- above all that the term is the gradient it claims to be -- are checked
without a GPU.  The formulas are those of the header of csrc/umap.hip."""
import numpy as np
import pytest

from test_umap_cpu import (ref_alpha, ref_knn, ref_layout_epoch, ref_random_init, ref_rates, ref_sampled, ref_smooth_knn,
                           ref_union)

EPS = 1e-8


# ------------------------------------------------------------------------------------------------ float64 reference


def ref_live(q, n_epochs):
    return np.asarray(q, dtype=np.int64) * int(n_epochs) >= 65536


def ref_graph_dists(dist, idx, graph):
    """umap-learn's dmat.maximum(dmat.T) of the kNN distances, read at the entries of the (scipy CSR) graph."""
    from scipy.sparse import csr_matrix

    n, k = np.asarray(idx).shape
    dmat = csr_matrix((np.asarray(dist, dtype=np.float64).ravel(), (np.repeat(np.arange(n), k), np.asarray(idx).ravel())),
                      shape=(n, n))
    dmat = csr_matrix(dmat.maximum(dmat.T))
    head = np.repeat(np.arange(n), np.diff(graph.indptr))
    return np.asarray(dmat[head, graph.indices]).ravel()


def ref_graph_radii(indptr, data, dists, q, n_epochs):
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    head = np.repeat(np.arange(n), np.diff(indptr))
    live = ref_live(q, n_epochs)
    w, d = np.asarray(data, dtype=np.float64)[live], np.asarray(dists, dtype=np.float64)[live]
    num = np.bincount(head[live], weights=w * d * d, minlength=n)
    den = np.bincount(head[live], weights=w, minlength=n)
    return np.log(EPS + np.divide(num, den, out=np.zeros(n), where=den > 0))


def ref_standardize(ro):
    ro = np.asarray(ro, dtype=np.float64)
    std = ro.std()
    return (ro - ro.mean()) / std if std > 0 else np.zeros_like(ro)


def ref_embedding_radii(y, indptr, indices, q, a, b, n_epochs):
    """(re, D, N / D) of the positions y over the live entries."""
    y = np.asarray(y, dtype=np.float64)
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = y.shape[0]
    head = np.repeat(np.arange(n), np.diff(indptr))
    live = ref_live(q, n_epochs)
    i, j = head[live], indices[live]
    r = ((y[i] - y[j]) ** 2).sum(axis=1)
    phi = 1.0 / (1.0 + a * r ** b)
    big_d = 2.0 * np.bincount(i, weights=phi, minlength=n)
    big_n = 2.0 * np.bincount(i, weights=phi * r, minlength=n)
    ratio = np.divide(big_n, big_d, out=np.zeros(n), where=big_d > 0)
    return np.log(EPS + ratio), big_d, ratio


def ref_density_terms(re, big_d, ratio, rad, mu_tot, dens_lambda, var_shift):
    """The per-vertex values and the scalar of a phase epoch: dict(inv_d, inv_den, w, scale, mean, var, cov, std)."""
    re, rad = np.asarray(re, dtype=np.float64), np.asarray(rad, dtype=np.float64)
    n = re.size
    mean = re.sum() / n
    var = ((re - mean) ** 2).sum() / n
    std = np.sqrt(var + var_shift)
    cov = (re * rad).sum() / (n - 1)
    return dict(inv_d=np.divide(1.0, big_d, out=np.zeros(n), where=big_d > 0), inv_den=1.0 / (EPS + ratio),
                w=rad - cov * (re - mean) / std ** 2 if std > 0 else rad.copy(),
                scale=dens_lambda * mu_tot / (std * n) if std > 0 else 0.0, mean=mean, var=var, cov=cov, std=std)


def ref_density_g(y, i, j, data, a, b, inv_d, inv_den, w, scale):
    """For the entries (i -> j) with weights `data`: (d = y_i - y_j, r, g_e, |W_i dr_i| + |W_j dr_j| times scale / w_e);
    g_e = 0 where r = 0."""
    y = np.asarray(y, dtype=np.float64)
    d = y[i] - y[j]
    r = (d * d).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = r ** b
        phi = 1.0 / (1.0 + a * p)
        t2 = a * b * p / (r * (1.0 + a * p))
        dri = phi * inv_d[i] * ((1.0 - b * (1.0 - phi)) * inv_den[i] + t2)
        drj = phi * inv_d[j] * ((1.0 - b * (1.0 - phi)) * inv_den[j] + t2)
        g = scale * (w[i] * dri + w[j] * drj) / data
        pieces = scale * (np.abs(w[i] * dri) + np.abs(w[j] * drj)) / data
    return d, r, np.where(r > 0, g, 0.0), np.where(r > 0, pieces, 0.0)


def ref_density_epoch(y, indptr, indices, q, data, a, b, alpha, ep, terms):
    """The density part of phase epoch `ep` from the positions y: (alpha * sum of the terms [n, dim], sum of |term|,
    sum of 4 |d_c| (|W_i dr_i| + |W_j dr_j|) scale / w_e -- the unclipped term with its two pieces taken absolutely --,
    number of term components that clip).  `terms`: inv_d, inv_den, w, scale as `ref_density_terms` returns them (the
    teacher-forced test passes the kernel's own float32 values)."""
    y = np.asarray(y, dtype=np.float64)
    n, dim = y.shape
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    head = np.repeat(np.arange(n), np.diff(indptr))
    e = np.flatnonzero(ref_sampled(q, ep))
    total, mag, pieces = np.zeros((n, dim)), np.zeros((n, dim)), np.zeros((n, dim))
    clipped = 0
    if e.size:
        i, j = head[e], indices[e]
        d, _, g, pc = ref_density_g(y, i, j, np.asarray(data, dtype=np.float64)[e], a, b, np.asarray(terms["inv_d"], dtype=np.float64),
                                    np.asarray(terms["inv_den"], dtype=np.float64), np.asarray(terms["w"], dtype=np.float64),
                                    float(terms["scale"]))
        raw = 2.0 * g[:, None] * d
        clipped = int((np.abs(raw) > 4.0).sum())
        term = 2.0 * np.clip(raw, -4.0, 4.0)
        np.add.at(total, i, term)
        np.add.at(mag, i, np.abs(term))
        np.add.at(pieces, i, 4.0 * pc[:, None] * np.abs(d))
    return float(alpha) * total, mag, pieces, clipped


def ref_phase(ep, n_epochs, dens_lambda, dens_frac):
    return bool(dens_lambda > 0 and (ep + 1) / n_epochs > 1.0 - dens_frac)


def ref_densmap_fit(x, k, dim, a, b, n_epochs, seed, dens_lambda, dens_frac=0.3, var_shift=0.1, rate=5, gamma=1.0,
                    learning_rate=1.0):
    """The whole algorithm in float64 with init="random": (y, ro, re at the final positions, fraction of the density
    term components that clipped)."""
    dist, idx = ref_knn(x, k)
    _, _, w, _ = ref_smooth_knn(dist, idx)
    g = ref_union(idx, w)
    q = ref_rates(g.data)
    dists = ref_graph_dists(dist, idx, g)
    ro = ref_graph_radii(g.indptr, g.data, dists, q, n_epochs)
    rad = ref_standardize(ro)
    mu_tot = g.data[ref_live(q, n_epochs)].sum()
    y = ref_random_init(x.shape[0], dim, seed).astype(np.float64)
    clipped = terms_seen = 0
    for ep in range(n_epochs):
        alpha = ref_alpha(learning_rate, ep, n_epochs)
        nxt = ref_layout_epoch(y, g.indptr, g.indices, q, a, b, gamma, alpha, seed, ep, rate)[0]
        if ref_phase(ep, n_epochs, dens_lambda, dens_frac):
            re, big_d, ratio = ref_embedding_radii(y, g.indptr, g.indices, q, a, b, n_epochs)
            terms = ref_density_terms(re, big_d, ratio, rad, mu_tot, dens_lambda, var_shift)
            delta, _, _, clip = ref_density_epoch(y, g.indptr, g.indices, q, g.data, a, b, alpha, ep, terms)
            nxt = nxt + delta
            clipped += clip
            terms_seen += int(ref_sampled(q, ep).sum()) * dim
        y = nxt
    re = ref_embedding_radii(y, g.indptr, g.indices, q, a, b, n_epochs)[0]
    return y, ro, re, clipped / max(terms_seen, 1)


def pearson(u, v):
    return float(np.corrcoef(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))[0, 1])


# ------------------------------------------------------------------------------------------------ tests


def small_graph(n, k, seed):
    x = np.random.default_rng(seed).standard_normal((n, 5))
    dist, idx = ref_knn(x, k)
    _, _, w, _ = ref_smooth_knn(dist, idx)
    g = ref_union(idx, w)
    return g, ref_rates(g.data), ref_graph_dists(dist, idx, g)


def test_density_term_is_the_gradient_of_the_correlation_objective():
    """C(y) = dot(re, R) / ((n - 1) sqrt(var(re) + shift)).  With every entry's unclipped term, sum over the row of
    4 (g_e w_e / (dens_lambda mu_tot)) (y_i - y_j) equals dC/dy_i (central differences, h = 1e-6) within 2 / n of the
    largest component: the two differ by umap-learn's own n-versus-(n - 1) inconsistency, a relative 1 / n (measured
    here: 0.0167 at n = 60)."""
    n, dim, k, n_epochs, a, b, shift = 60, 2, 8, 500, 1.57694, 0.89506, 0.1
    g, q, dists = small_graph(n, k, 3)
    rad = ref_standardize(ref_graph_radii(g.indptr, g.data, dists, q, n_epochs))
    live = ref_live(q, n_epochs)
    assert live.any() and np.abs(rad).max() > 0
    y = 3.0 * np.random.default_rng(4).standard_normal((n, dim))

    def objective(pos):
        re = ref_embedding_radii(pos, g.indptr, g.indices, q, a, b, n_epochs)[0]
        return float(re @ rad) / ((n - 1) * np.sqrt(re.var() + shift))

    numeric = np.zeros((n, dim))
    h = 1e-6
    for i in range(n):
        for c in range(dim):
            up, dn = y.copy(), y.copy()
            up[i, c] += h
            dn[i, c] -= h
            numeric[i, c] = (objective(up) - objective(dn)) / (2 * h)
    re, big_d, ratio = ref_embedding_radii(y, g.indptr, g.indices, q, a, b, n_epochs)
    mu_tot, lam = g.data[live].sum(), 1.0
    terms = ref_density_terms(re, big_d, ratio, rad, mu_tot, lam, shift)
    head = np.repeat(np.arange(n), np.diff(g.indptr))
    e = np.flatnonzero(live)
    d, _, ge, _ = ref_density_g(y, head[e], g.indices[e], g.data[e], a, b, terms["inv_d"], terms["inv_den"], terms["w"],
                                terms["scale"])
    analytic = np.zeros((n, dim))
    np.add.at(analytic, head[e], 4.0 * (ge * g.data[e] / (lam * mu_tot))[:, None] * d)
    top = np.abs(numeric).max()
    assert top > 0
    worst = np.abs(analytic - numeric).max() / top
    print(f"density term against central differences: relative difference {worst:.4f} (1 / n = {1 / n:.4f})")
    assert worst <= 2.0 / n


def test_reference_radii_by_hand():
    """Two vertices at distance 2 (r = 4), one edge, both directions live."""
    a, b = 1.5, 0.9
    y = np.array([[0.0, 0.0], [2.0, 0.0]])
    re, big_d, ratio = ref_embedding_radii(y, [0, 1, 2], [1, 0], [65536, 65536], a, b, 10)
    phi = 1.0 / (1.0 + a * 4.0 ** b)
    assert np.allclose(big_d, 2 * phi, rtol=1e-15) and np.allclose(ratio, 4.0, rtol=1e-15) and np.allclose(re, np.log(EPS + 4.0))
    # an entry that is never sampled in 10 epochs is not live: the row is empty
    re, big_d, _ = ref_embedding_radii(y, [0, 1, 2], [1, 0], [6553, 6553], a, b, 10)
    assert (big_d == 0).all() and np.allclose(re, np.log(EPS))
    assert ref_live([6554], 10).all() and not ref_live([6553], 10).any()
    ro = ref_graph_radii([0, 2, 3, 3], [0.5, 1.0, 1.0], [2.0, 4.0, 3.0], [65536, 65536, 0], 20)
    assert np.allclose(ro, [np.log(EPS + (0.5 * 4 + 16) / 1.5), np.log(EPS), np.log(EPS)])
    assert (ref_standardize([1.0, 1.0, 1.0]) == 0).all()
    assert np.allclose(ref_standardize([1.0, 3.0]), [-1.0, 1.0])


def test_density_phase_predicate():
    from ssl_wafermap_amd.manifold import in_density_phase

    for frac, want in ((0.3, list(range(140, 200))), (0.0, []), (1.0, list(range(200)))):
        assert [ep for ep in range(200) if in_density_phase(ep, 200, 1.0, frac)] == want
        assert [ep for ep in range(200) if ref_phase(ep, 200, 1.0, frac)] == want
    assert not any(in_density_phase(ep, 200, 0.0, 1.0) for ep in range(200))


def test_epoch_default_adds_200():
    from ssl_wafermap_amd.manifold import DensMAP

    model = DensMAP()
    assert (model.dens_lambda, model.dens_frac, model.dens_var_shift) == (2.0, 0.3, 0.1)
    assert model.default_epochs(10000) == 700 and model.default_epochs(10001) == 400
    assert DensMAP(n_epochs=123).default_epochs(50000) == 123
    assert model.rad_orig_ is None and model.rad_emb_ is None and model.embedding_ is None


def test_argument_validation_needs_no_gpu():
    from ssl_wafermap_amd.manifold import UMAP, DensMAP

    for bad in ({"dens_lambda": -0.1}, {"dens_frac": -0.1}, {"dens_frac": 1.1}, {"dens_var_shift": -1.0}, {"n_neighbors": 1},
                {"n_components": 65}, {"densmap": True}, {"densmap": False}):
        with pytest.raises(ValueError):
            DensMAP(**bad)
    DensMAP(dens_lambda=0.0, dens_frac=0.0, dens_var_shift=0.0)
    DensMAP(n_neighbors=30, n_components=50, min_dist=0.0, dens_lambda=0.1, dens_frac=1.0)
    with pytest.raises(NotImplementedError, match="densmap"):
        UMAP(densmap=True)
    with pytest.raises(NotImplementedError, match="DensMAP"):
        UMAP(densmap=True)


def test_refusals_stay():
    import torch

    from ssl_wafermap_amd.manifold import DensMAP

    with pytest.raises(NotImplementedError, match="semi-supervised"):
        DensMAP().fit(torch.zeros(8, 4), y=np.zeros(8))
    with pytest.raises(NotImplementedError, match="transform"):
        DensMAP().transform(torch.zeros(8, 4))


def test_cpu_tensors_are_refused():
    import torch

    from ssl_wafermap_amd import _lib, manifold

    i32 = dict(dtype=torch.int32)
    with pytest.raises(_lib.WaferHipError):
        manifold.DensMAP(n_neighbors=3).fit(torch.zeros(8, 4))
    with pytest.raises(_lib.WaferHipError):
        manifold.fuzzy_simplicial_set(torch.zeros(8, 4), 3, return_dists=True)
    with pytest.raises(_lib.WaferHipError):
        manifold.graph_radii(torch.zeros(9, **i32), torch.zeros(0), torch.zeros(0), torch.zeros(0, **i32), 10)
    with pytest.raises(_lib.WaferHipError):
        manifold.embedding_radii(torch.zeros(8, 2), torch.zeros(9, **i32), torch.zeros(0, **i32), torch.zeros(0, **i32), 1.5, 0.9, 10)
    with pytest.raises(_lib.WaferHipError):
        manifold.optimize_layout_densmap(torch.zeros(8, 2), torch.zeros(9, **i32), torch.zeros(0, **i32), torch.zeros(0, **i32),
                                         torch.zeros(0), torch.zeros(8), 1.5, 0.9, 10)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    assert lib.wm_densmap_layout_workspace_bytes(1) == 0 and lib.wm_densmap_layout_workspace_bytes((1 << 24) + 1) == 0
    assert lib.wm_densmap_layout_workspace_bytes(300) == 4160 + 40 * 300
    assert lib.wm_densmap_graph_radii(None, None, None, None, 4, 10, None, None) == -1
    assert lib.wm_densmap_embedding_radii(None, None, None, None, 4, 2, 1.5, 0.9, 10, None, None, None) == -1
    assert lib.wm_densmap_layout(None, None, None, None, None, None, None, 4, 0, 2, 1.5, 0.9, 1.0, 1.0, 1.0, 0.3, 0.1, 0, 0, 1, 1, 5,
                                 None, 0, None, None) == -1
