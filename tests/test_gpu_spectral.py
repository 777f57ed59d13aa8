"""GPU checks of the Laplacian-eigenmaps kernels (csrc/spectral.hip), the device eigensolver and the estimators built on it
(manifold.laplacian_eigenpairs, spectral_layout, UMAP(init="spectral_device"), SpectralEmbedding; cluster.SpectralClustering)
against numpy float64, the restatement in tests/test_spectral_cpu.py and sklearn.

Bounds are derived, not tuned.  u = 2^-53 (float64), v = 2^-24 (float32).
  (a) Exact cases.  A circulant graph of degree 4 or 16 with unit weights has deg = 4 or 16, dinv = 1/2 or 1/4, and with an
      integer v every product and partial sum is a small dyadic number: any order gives numpy's bits.  The same holds for
      integer V and S in wm_spec_rotate (sums below 2^53), which settles the fragment maps of v_mfma_f64_16x16x4_f64.
  (b) A double sum of K terms, each the product of three factors, computed twice (device, numpy): each side is within
      (K + 2) u sum|terms| of the exact value, so they differ by at most 2 (K + 2) u sum|terms| per row (matvec).  The
      degree is bit-equal to the restatement of its own order (np.cumsum adds strictly in index order).
  (c) wm_spec_orthonormalise against numpy CGS2 (test_spectral_cpu.ref_cgs2), |V_c| = 1.  A dot product of n terms is
      within (n + 1) u sum|V_ic||w_i| <= (n + 1) u |w| of the exact one (Cauchy-Schwarz); two passes, two computations:
      the summed coefficients differ by at most 4 (n + 3) u |w|.  The residual vector carries, per computation, the two
      u-projections (2 ((n + 2) u + 2 u) |w|) and the two updates (2 ((m1 + 2) u sqrt(m1) + sqrt(m1) (n + 2) u) |w|,
      m1 = j + 1 columns), and the norm itself (n + 2) u beta: beta differs by at most
      4 u |w| ((n + 4) + sqrt(m1) (n + m1 + 4)) + 2 (n + 2) u beta.
      The new column: the second pass removes what the first left, so V_c . v is the rounding of ONE dot product and one
      update relative to the vector they act on, whose norm is beta (1 + O(n u rho)), rho = |w| / beta; measuring it adds
      (n + 1) u: |V_c . v|, |u_c . v| <= (3 n + 2 m1 + 10) u (1 + sqrt(m1) (n + 2) u rho).  | |v| - 1 | <= 2 (n + 3) u (the
      kernel's norm, the division, the measurement).
      A basis of j + 1 orthonormal columns orthogonal to `ncomp` trivial vectors leaves room for a new column only when
      n >= j + 2 + ncomp: of the grid n x j x components, those combinations are run (n = 3 with 3 components and the
      large j at small n do not exist).
  (d) The solver.  For a unit y, some eigenvalue of N lies within r = |N y - theta y|; numpy's dense eigh is within
      8 n u |N|, |N| = 1.  Residuals recomputed in float64 must be at most tol + 8 n u (the recomputation's rounding and the
      basis's loss of orthogonality, both O(n u), stand behind the second term).  Eigenvalue i lies within r_i + 8 n u of a
      reference value, the k matches distinct.  Davis-Kahan: the sine of the largest angle between the computed and the
      reference span is at most 2 (max r + 8 n u) / gap, gap = lambda_{k+1} - lambda_k of the REFERENCE; the measurement
      (k dot products of n terms per column, a k x k SVD) adds a floor of 8 n k u.
  (e) SpectralEmbedding against sklearn (arpack, tol 0) column by column: both are brought back to unit eigenvectors
      (times sqrt(deg)); Davis-Kahan per column with gap_i the distance of lambda_i to the rest of the reference
      spectrum gives sin <= 2 (r_i + 8 n u) / gap_i, two unit vectors of one sign at that angle differ by at most sqrt(2)
      sin in norm, and the float32 `embedding_` adds 2 v.
"""
import warnings

import numpy as np
import pytest
import torch
from parity_log import parity

from test_spectral_cpu import (blob_rows, dense_reference, golden_labels, golden_rows, ref_cgs2, ref_components, ref_normalised, ref_trivial)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, V32 = 2.0 ** -53, 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def M():
    from ssl_wafermap_amd import manifold

    return manifold


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def worst(diff, bound):
    """max diff / bound; where the bound is exactly 0 the difference must be."""
    diff, bound = np.asarray(diff, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    zero = bound == 0
    assert (diff[zero] == 0).all(), "a zero bound needs an exact result"
    return float((diff[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def to_csr(g):
    """A scipy matrix as manifold.CSR on the device (sorted columns, float32 data)."""
    g = g.tocsr()
    g.sum_duplicates()
    g.sort_indices()
    return M().CSR(dev(g.indptr.astype(np.int32)), dev(g.indices.astype(np.int32)), dev(g.data.astype(np.float32)))


def circulant(n, degree):
    """Row i is joined to i +- 1 .. i +- degree / 2 (mod n) with weight 1 each; coinciding entries add up, so every row
    sums to exactly `degree` at every n."""
    from scipy.sparse import coo_matrix

    i = np.repeat(np.arange(n), degree)
    off = np.tile(np.concatenate([np.arange(1, degree // 2 + 1), -np.arange(1, degree // 2 + 1)]), n)
    return coo_matrix((np.ones(n * degree, dtype=np.float32), (i, (i + off) % n)), shape=(n, n)).tocsr()


def random_symmetric(n, seed, lengths=()):
    """A symmetric float32 graph: rows 0 .. len(lengths) - 1 get exactly the given numbers of entries (joined to later
    rows only), the other rows about 6 random ones among themselves."""
    from scipy.sparse import coo_matrix

    rng = np.random.default_rng(seed)
    s = len(lengths)
    r, c = [], []
    for i, ln in enumerate(lengths):
        cols = s + rng.choice(n - s, size=ln, replace=False)
        r += [i] * ln
        c += cols.tolist()
    rest = n - s
    if rest >= 2:
        a = s + rng.integers(0, rest, size=3 * rest)
        b = s + rng.integers(0, rest, size=3 * rest)
        keep = a != b
        r += a[keep].tolist()
        c += b[keep].tolist()
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    pairs = np.unique(np.stack([np.minimum(r, c), np.maximum(r, c)], axis=1), axis=0) if r.size else np.zeros((0, 2), dtype=np.int64)
    w = rng.uniform(0.01, 1.0, size=pairs.shape[0]).astype(np.float32)
    g = coo_matrix((np.concatenate([w, w]), (np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]]))),
                   shape=(n, n)).tocsr()
    g.sort_indices()
    return g


# ------------------------------------------------------------------------------------------------ degree, matvec


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("degree", [4, 16])
def test_matvec_and_degree_are_exact_on_circulant_graphs(n, degree):
    g = circulant(n, degree)
    csr = to_csr(g)
    deg, dinv = M().laplacian_degree(csr)
    assert np.array_equal(host(deg), np.full(n, float(degree))) and np.array_equal(host(dinv), np.full(n, 1.0 / np.sqrt(degree)))
    v = np.random.default_rng(n + degree).integers(-512, 513, size=n).astype(np.float64)
    want = host(dinv) * (g.astype(np.float64) @ (host(dinv) * v))
    assert np.array_equal(host(M().laplacian_matvec(csr, dinv, dev(v))), want)
    basis = np.full((n, 7), np.nan)  # a column of a basis: the pitch is honoured, the neighbours are never read
    basis[:, 3] = v
    assert np.array_equal(host(M().laplacian_matvec(csr, dinv, dev(basis), 3)), want)


@pytest.mark.parametrize("n, lengths", [(2, ()), (63, (0, 1)), (64, (0, 1)), (65, (0, 1, 60)), (1000, (0, 1, 64, 65, 300))])
def test_matvec_and_degree_against_float64(n, lengths):
    g = random_symmetric(n, 17 * n, lengths)
    got_len = np.diff(g.indptr)
    assert got_len[:len(lengths)].tolist() == list(lengths)
    csr = to_csr(g)
    deg, dinv = M().laplacian_degree(csr)
    deg_h, dinv_h = host(deg), host(dinv)
    d64 = g.data.astype(np.float64)
    for i in range(n):  # the stated order: the row's entries in storage order, one accumulator
        row = d64[g.indptr[i]:g.indptr[i + 1]]
        assert deg_h[i] == (np.cumsum(row)[-1] if row.size else 0.0)
    empty = deg_h == 0
    assert (dinv_h[empty] == 0).all() and np.array_equal(empty, got_len == 0)
    want_dinv = 1.0 / np.sqrt(deg_h[~empty])
    parity(f"spec dinv n={n} / (2 u relative)", worst(np.abs(dinv_h[~empty] - want_dinv), 2 * U * want_dinv), 1.0)
    v = np.random.default_rng(n).normal(size=n)
    got = host(M().laplacian_matvec(csr, dinv, dev(v)))
    g64 = g.astype(np.float64)
    want = dinv_h * (g64 @ (dinv_h * v))
    mag = dinv_h * (g64 @ np.abs(dinv_h * v))  # sum |terms| per row (the weights are positive)
    parity(f"spec matvec n={n} / bound", worst(np.abs(got - want), 2 * (got_len + 2) * U * mag), 1.0)
    assert (got[got_len == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ orthonormalise


def ortho_case(n, j, ncomp, seed):
    """(labels, unit trivial vectors u, orthonormal V [n, j + 1] orthogonal to them, a random w)."""
    rng = np.random.default_rng(seed)
    labels = np.sort(rng.integers(0, ncomp, size=n)) if ncomp > 1 else np.zeros(n, dtype=np.int64)
    labels[:ncomp] = np.arange(ncomp)  # every component has a row
    labels = rng.permutation(labels) if n > 64 else labels
    deg = rng.uniform(0.5, 4.0, size=n)
    u = ref_trivial(deg, labels, ncomp)
    a = rng.normal(size=(n, j + 1))
    for _ in range(2):
        a = a - u[:, None] * np.stack([np.bincount(labels, weights=u * a[:, c], minlength=ncomp)[labels] for c in range(j + 1)], axis=1)
    basis = np.linalg.qr(a)[0]
    return labels, u, basis, rng.normal(size=n)


def run_ortho(w, basis, j, m, labels, ncomp, u):
    """The kernel on a basis buffer [n, m + 1] whose columns behind j hold NaN (never read); returns (w out, V, T cells)."""
    n = basis.shape[0]
    buf = np.full((n, m + 1), np.nan)
    buf[:, :j + 1] = basis
    wd, vd, td = dev(w), dev(buf), torch.zeros(m * m + 2, dtype=torch.float64, device=DEV)
    M().lanczos_orthonormalise(wd, vd, j, dev(labels.astype(np.int32)), ncomp, dev(u), td, m)
    return host(wd), host(vd), host(td)


ORTHO_CASES = [(n, j, c) for c in (1, 3) for n in (3, 64, 65, 257, 4097) for j in (0, 1, 15, 16, 17, 63, 64, 129) if n >= j + 2 + c]


@pytest.mark.parametrize("n, j, ncomp", ORTHO_CASES)
def test_orthonormalise_against_numpy_cgs2(n, j, ncomp):
    labels, u, basis, w = ortho_case(n, j, ncomp, 1000 * n + 10 * j + ncomp)
    m = j + 2 if j % 2 == 0 else j + 1  # with and without the sub-diagonal cell T[j + 1][j]
    w_out, v_out, t = run_ortho(w, basis, j, m, labels, ncomp, u)
    w_ref, h_ref, beta_ref = ref_cgs2(w, basis, u, labels, ncomp)
    tm, m1, wn = t[:m * m].reshape(m, m), j + 1, np.linalg.norm(w)
    tag = f"n={n} j={j} comps={ncomp}"
    parity(f"spec cgs2 coefficients {tag} / bound", np.abs(tm[:m1, j] - h_ref).max() / (4 * (n + 3) * U * wn), 1.0)
    beta = t[m * m]
    beta_bound = 4 * U * wn * ((n + 4) + np.sqrt(m1) * (n + m1 + 4)) + 2 * (n + 2) * U * beta_ref
    parity(f"spec cgs2 beta {tag} / bound", abs(beta - beta_ref) / beta_bound, 1.0)
    assert t[m * m + 1:].view(np.int64)[0] == 0, "no breakdown"
    if m > m1:
        assert tm[j + 1, j] == beta
    untouched = np.ones((m, m), dtype=bool)
    untouched[:m1, j] = False
    untouched[min(j + 1, m - 1), j] = False
    assert (tm[untouched] == 0).all(), "only column j of T is written"
    assert np.array_equal(bits(v_out[:, :m1]), bits(basis)), "the basis is read only"
    col = v_out[:, j + 1]
    assert np.isfinite(col).all() and np.array_equal(col, w_out / beta), "the new column is w / beta, beta from device memory"
    rho = wn / beta_ref
    orth_bound = (3 * n + 2 * m1 + 10) * U * (1 + np.sqrt(m1) * (n + 2) * U * rho)
    parity(f"spec new column . basis {tag} / bound", np.abs(basis.T @ col).max() / orth_bound, 1.0)
    udots = np.bincount(labels, weights=u * col, minlength=ncomp)
    parity(f"spec new column . trivial {tag} / bound", np.abs(udots).max() / orth_bound, 1.0)
    parity(f"spec new column norm {tag} / bound", abs(np.linalg.norm(col) - 1.0) / (2 * (n + 3) * U), 1.0)


@pytest.mark.parametrize("n, j, ncomp", [(64, 0, 1), (65, 16, 3), (257, 63, 1), (4097, 129, 3)])
def test_orthonormalise_flags_a_breakdown_without_nan(n, j, ncomp):
    labels, u, basis, w = ortho_case(n, j, ncomp, 77 * n + j)
    inside = basis @ np.random.default_rng(j).normal(size=j + 1) + 0.5 * u
    inside *= 0.25 / np.linalg.norm(inside)
    m = j + 2
    w_out, v_out, t = run_ortho(inside, basis, j, m, labels, ncomp, u)
    assert t[m * m + 1:].view(np.int64)[0] == j + 1, "the flag names the step"
    assert t[m * m] < n * U and (v_out[:, j + 1] == 0).all() and np.isfinite(w_out).all()
    # the flag is sticky: a later healthy step does not clear or overwrite it
    wd, vd, td = dev(w), dev(np.concatenate([basis, np.zeros((n, m - j))], axis=1)), dev(t)
    M().lanczos_orthonormalise(wd, vd, j, dev(labels.astype(np.int32)), ncomp, dev(u), td, m)
    assert host(td)[m * m + 1:].view(np.int64)[0] == j + 1 and host(td)[m * m] > 0.01


def test_orthonormalise_gives_the_same_bits_twice():
    labels, u, basis, w = ortho_case(4097, 64, 3, 5)
    a, b = run_ortho(w, basis, 64, 66, labels, 3, u), run_ortho(w, basis, 64, 66, labels, 3, u)
    assert all(np.array_equal(bits(np.nan_to_num(x)), bits(np.nan_to_num(y))) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ rotate


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_rotate_is_exact_on_integer_data(n):
    rng = np.random.default_rng(n)
    for m in (4, 63, 64, 130):
        basis = np.full((n, m + 3), np.nan)  # pitch above m: the columns behind m are never read
        basis[:, :m] = rng.integers(-64, 65, size=(n, m))
        for q in (1, 16, 17, 51):
            s = rng.integers(-64, 65, size=(m, q)).astype(np.float64)
            want = basis[:, :m] @ s
            assert np.array_equal(host(M().basis_rotate(dev(basis), s, m)), want), f"m={m} q={q}"
            out = torch.full((n, q + 2), -7.0, dtype=torch.float64, device=DEV)  # a wider second buffer keeps its other columns
            got = host(M().basis_rotate(dev(basis), dev(s), m, out=out))
            assert np.array_equal(got[:, :q], want) and (got[:, q:] == -7.0).all(), f"m={m} q={q} pitch"


# ------------------------------------------------------------------------------------------------ solver


@pytest.fixture(scope="module")
def graphs():
    """name -> (CSR on the device, float64 N of that same float32 graph, components, labels, reference eigenvalues and
    vectors): the 600-row golden graph at 5 neighbours and the three-blob graph at 10, both by the device's own kNN and
    fuzzy union; one dense eigh each, shared by the tests below."""
    out = {}
    for name, x, k in (("golden", golden_rows(600), 5), ("blobs", blob_rows(), 10)):
        csr = M().fuzzy_simplicial_set(dev(x), k)
        ncomp, labels = ref_components(csr.to_scipy())
        nmat, _ = ref_normalised(csr.to_scipy())
        out[name] = (csr, nmat, ncomp, labels) + dense_reference(nmat, ncomp)
    assert out["golden"][2] == 1 and out["blobs"][2] == 3
    return out


@pytest.mark.parametrize("name, k", [("golden", 2), ("golden", 50), ("blobs", 8)])
def test_solver_against_dense_eigh(graphs, name, k):
    csr, nmat, ncomp, labels, ref_vals, ref_vecs = graphs[name]
    n, tol = nmat.shape[0], 1e-6
    res = M().laplacian_eigenpairs(csr, k, tol=tol)
    assert res.converged and res.n_components == ncomp and res.cycles >= 1 and res.matvecs >= max(2 * k + 2, 64)
    assert np.array_equal(host(res.labels), labels)
    vals, y = res.eigenvalues, host(res.eigenvectors)
    assert vals.shape == (k,) and y.shape == (n, k) and y.dtype == np.float64 and (np.diff(vals) >= 0).all()
    resid = np.linalg.norm(nmat @ y - y * (1.0 - vals), axis=0)
    parity(f"spec solver {name} k={k} residual / (tol + 8 n u)", resid.max() / (tol + 8 * n * U), 1.0)
    near = np.abs(ref_vals[None, :] - vals[:, None]).argmin(axis=1)
    assert np.array_equal(near, np.arange(k)), "every eigenvalue matches its own reference value: none doubled, none missed"
    parity(f"spec solver {name} k={k} eigenvalue error / (residual + 8 n u)",
           worst(np.abs(vals - ref_vals[:k]), resid + 8 * n * U), 1.0)
    gap = ref_vals[k] - ref_vals[k - 1]
    q, _ = np.linalg.qr(y)
    sine = np.linalg.norm(q - ref_vecs[:, :k] @ (ref_vecs[:, :k].T @ q), 2)
    parity(f"spec solver {name} k={k} span sine / bound", sine / (2 * (resid.max() + 8 * n * U) / gap + 8 * n * k * U), 1.0,
           note=f"gap {gap:.3g}, cycles {res.cycles}, matvecs {res.matvecs}")
    # the trivial pairs, separately: unit vectors on their components, in the order of the smallest row
    triv = host(res.trivial_matrix())
    assert triv.shape == (n, ncomp) and all((triv[labels != c, c] == 0).all() for c in range(ncomp))
    parity(f"spec solver {name} trivial residual / (8 n u)", np.abs(nmat @ triv - triv).max() / (8 * n * U), 1.0)
    # u is an exact eigenvector of eigenvalue 1: u . (N y - theta y) = (1 - theta) u . y, so |u . y| <= r / lambda
    parity(f"spec solver {name} k={k} trivial . nontrivial / (r / lambda + n u)",
           worst(np.abs(triv.T @ y).max(axis=0), resid / vals + n * U), 1.0)
    again = M().laplacian_eigenpairs(csr, k, tol=tol)
    assert np.array_equal(bits(vals), bits(again.eigenvalues)) and np.array_equal(bits(y), bits(host(again.eigenvectors)))
    assert (again.cycles, again.matvecs) == (res.cycles, res.matvecs)


def test_solver_reports_when_the_cycles_run_out(graphs):
    res = M().laplacian_eigenpairs(graphs["golden"][0], 2, tol=1e-12, max_cycles=1)
    assert res.converged is False and res.cycles == 1 and res.matvecs == 64
    assert np.isfinite(res.eigenvalues).all() and bool(torch.isfinite(res.eigenvectors).all())


# ------------------------------------------------------------------------------------------------ estimators


def test_spectral_embedding_matches_sklearn(graphs):
    from sklearn.manifold import SpectralEmbedding

    x = golden_rows(600)
    est = M().SpectralEmbedding(n_components=3, n_neighbors=5)
    got = est.fit_transform(dev(x))
    assert got.shape == (600, 3) and got.dtype == torch.float32 and got.is_cuda and est.embedding_ is got
    assert est.converged_ and est.n_connected_components_ == 1 and est.eigenvalues_.shape == (3,)
    aff = est.affinity_matrix_.to_scipy().astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = SpectralEmbedding(n_components=3, affinity="precomputed", eigen_solver="arpack", random_state=0).fit_transform(aff)
    nmat, deg = ref_normalised(aff)
    ref_vals, _ = dense_reference(nmat, 1)
    root = np.sqrt(deg)
    for c in range(3):
        a, b = host(got)[:, c].astype(np.float64) * root, ref[:, c] * root
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
        r = np.linalg.norm(nmat @ a - a * (a @ (nmat @ a)))
        gap = min(ref_vals[c] - (ref_vals[c - 1] if c else 0.0), ref_vals[c + 1] - ref_vals[c])
        bound = np.sqrt(2.0) * 2 * (r + 8 * 600 * U) / gap + 2 * V32
        parity(f"spectral embedding column {c} against sklearn / bound", np.linalg.norm(a - b) / bound, 1.0,
               note=f"residual {r:.3g}, gap {gap:.3g}")
    parity("spectral embedding eigenvalues against dense eigh / (tol + 8 n u)",
           np.abs(est.eigenvalues_ - ref_vals[:3]).max() / (1e-6 + 8 * 600 * U), 1.0)
    conn = M().SpectralEmbedding(n_components=2, n_neighbors=5, affinity="connectivity").fit(dev(x))
    dense = conn.affinity_matrix_.to_scipy().toarray()
    assert np.array_equal(dense, dense.T) and set(np.unique(dense)) <= {0.0, 0.5, 1.0} and (np.diag(dense) == 1.0).all()
    assert bool(torch.isfinite(conn.embedding_).all())


def rings():
    """Two concentric rings of 300 rows each (radii 1 and 3, a little radial noise), shuffled, and their labels."""
    rng = np.random.default_rng(2)
    ang = np.concatenate([np.linspace(0, 2 * np.pi, 300, endpoint=False)] * 2)
    rad = np.repeat([1.0, 3.0], 300) + rng.normal(0.0, 0.02, 600)
    order = rng.permutation(600)
    return (np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)[order]).astype(np.float32), np.repeat([0, 1], 300)[order]


def same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def test_spectral_clustering_separates_rings_that_kmeans_splits():
    from sklearn.cluster import SpectralClustering

    from ssl_wafermap_amd import cluster

    x, truth = rings()
    km = cluster.KMeans(2, n_init=10, random_state=0).fit(dev(x)).labels_
    assert not same_partition(km, truth), "KMeans cuts across the rings"
    est = cluster.SpectralClustering(2, n_neighbors=10)
    got = est.fit_predict(dev(x))
    assert got.shape == (600,) and got is est.labels_ and est.converged_
    assert same_partition(got, truth), "both rings recovered exactly"
    aff = est.affinity_matrix_.to_scipy().astype(np.float64)
    assert aff.shape == (600, 600) and est.embedding_.shape == (600, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = SpectralClustering(2, affinity="precomputed", random_state=0).fit_predict(aff)
    assert same_partition(got, ref)
    fuzzy = cluster.SpectralClustering(2, n_neighbors=10, affinity="fuzzy").fit_predict(dev(x))
    assert same_partition(fuzzy, truth)


# ------------------------------------------------------------------------------------------------ UMAP


def test_umap_spectral_device_lays_out_a_disconnected_graph():
    from scipy.sparse.csgraph import connected_components

    x = dev(golden_rows(12449))
    model = M().UMAP(n_neighbors=15, init="spectral_device", n_epochs=50)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = model.fit_transform(x)
        start = model._initial(x, model.graph_)
    g = model.graph_.to_scipy()
    ncomp = connected_components(g, directed=False)[0]
    assert ncomp > 1, "the default n_neighbors leaves the golden graph disconnected"
    ncomp2, labels = M().graph_components(model.graph_)
    assert ncomp2 == ncomp
    layout = M().spectral_layout(x, model.graph_, 2, model.random_state)
    assert layout is not None and layout.shape == (12449, 2) and layout.dtype == torch.float64
    meta, ranges = M().component_plan(x, labels, ncomp, 2)
    lay = host(layout)
    for c in range(ncomp):
        off = np.abs(lay[labels == c] - meta[c]).max()
        assert off <= ranges[c] * (1 + 4 * U), f"component {c} leaves its data_range"
    start = host(start)
    assert start.shape == (12449, 2) and (start.min(axis=0) == 0).all() and (start.max(axis=0) == 10).all()
    assert got.shape == (12449, 2) and bool(torch.isfinite(got).all())
    again = M().UMAP(n_neighbors=15, init="spectral_device", n_epochs=50).fit_transform(x)
    assert np.array_equal(bits(host(got)), bits(host(again))), "two fits must give the same bits"


def test_umap_spectral_device_ends_no_worse_than_pca():
    """The yardstick of tests/test_gpu_umap.py for its inits: 200 epochs from the start keep neighbourhoods at least as well
    as the 2-D PCA projection of the 1 500 golden rows."""
    from sklearn.manifold import trustworthiness

    x = golden_rows(1500)
    model = M().UMAP(n_neighbors=15, init="spectral_device", n_epochs=200)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = host(model.fit_transform(dev(x)))
    assert np.isfinite(got).all() and got.shape == (1500, 2)
    xc = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    u, sv, _ = np.linalg.svd(xc, full_matrices=False)
    parity("umap init=spectral_device trustworthiness(15), 1500 rows (bound: PCA to 2-D)", trustworthiness(x, got, n_neighbors=15),
           trustworthiness(x, u[:, :2] * sv[:2], n_neighbors=15), higher=True)
    for cls in (M().DensMAP, M().InductiveUMAP):  # the same value works in the other estimators
        start = cls(n_neighbors=15, init="spectral_device", n_epochs=10)._initial(dev(x), model.graph_)
        assert start.shape == (1500, 2) and bool(torch.isfinite(start).all())


def test_spectral_layout_draws_small_components_in_component_order():
    """A hand-built graph of three components, numbered by their smallest row: rows {0, 3} (an edge), rows {1, 2, 4, 5, 6, 7}
    (a ring with one chord) and rows {8, 9, 10} (a path).  In 2-D their meta positions are (1, 0), (0, 1), (-1, 0), each
    sqrt(2) from its nearest other, so every data_range is sqrt(2) / 2.  The first and the last are small (fewer than 4
    rows): their rows are uniform(-data_range, data_range) around the meta position from default_rng(random_state), the
    first component's 2 x 2 numbers drawn before the last one's 3 x 2, bit for bit.  The ring is laid out by its own
    eigenvectors, scaled so that its largest coordinate offset is the data_range."""
    from scipy.sparse import coo_matrix

    edges = [(0, 3), (1, 2), (2, 4), (4, 5), (5, 6), (6, 7), (7, 1), (1, 5), (8, 9), (9, 10)]
    r, c = np.array(edges).T
    g = coo_matrix((np.ones(2 * len(edges), dtype=np.float32), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(11, 11))
    x = dev(np.zeros((11, 4), dtype=np.float32))
    rad = np.sqrt(2.0) / 2.0
    for seed in (0, 7):
        got = host(M().spectral_layout(x, to_csr(g), 2, random_state=seed))
        rng = np.random.default_rng(seed)
        first = rng.uniform(-rad, rad, (2, 2)) + np.array([1.0, 0.0])
        last = rng.uniform(-rad, rad, (3, 2)) + np.array([-1.0, 0.0])
        assert np.array_equal(bits(got[[0, 3]]), bits(first)) and np.array_equal(bits(got[[8, 9, 10]]), bits(last))
        ring = got[[1, 2, 4, 5, 6, 7]] - np.array([0.0, 1.0])
        assert abs(np.abs(ring).max() - rad) <= 4 * U


@pytest.mark.parametrize("name", ["InductiveUMAP", "InductiveDensMAP"])
def test_inductive_fit_with_labels_at_full_target_weight(name):
    """target_weight = 1 makes far_dist 1e12 and exp(-far_dist) exactly 0: every entry across two labels stays stored with
    weight 0 and the graph falls apart by label.  init="spectral_device" lays the pieces out one by one from the
    intersected graph, without a warning and without a PCA fallback."""
    from scipy.sparse.csgraph import connected_components

    x, y = golden_rows(1500), golden_labels(1500).astype(np.int64)  # (every row labelled: nothing bridges two labels)
    assert np.unique(y).size > 1
    model = getattr(M(), name)(n_neighbors=15, init="spectral_device", n_epochs=30, target_weight=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = model.fit(dev(x), y).embedding_
        start = model._initial(dev(x), model.graph_)
    assert got.shape == (1500, 2) and bool(torch.isfinite(got).all())
    g = model.graph_.to_scipy()
    assert (g.data == 0).any(), "explicit zeros between labels"
    g.eliminate_zeros()
    assert connected_components(g, directed=False)[0] > 1
    layout = M().spectral_layout(dev(x), model.graph_, 2, model.random_state)
    assert layout is not None and bool(torch.isfinite(layout).all())
    start = host(start)
    assert (start.min(axis=0) == 0).all() and (start.max(axis=0) == 10).all()
