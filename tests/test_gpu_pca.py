"""GPU checks of the PCA kernels (csrc/pca.hip), their Python layer (decomposition.py) and
scripts/embedding_pca_amd.py against numpy float64 and sklearn.

Bounds are derived, not tuned.  u = 2^-53 (float64), v = 2^-24 (float32).
  (a) Integer-valued data: every product and partial sum is an integer below 2^53, so any summation order gives the same
      bits and the results must EQUAL numpy's.  This is the test of the fragment maps of v_mfma_f64_16x16x4_f64, the
      lower-triangle walk, the mirror, the ragged edges and the slice merge.
  (b) General data: a double sum of K products, each product rounded or fused and each addition rounded, is within
      (K + 1) u sum|a||b| of the exact value to first order; the float64 restatement (numpy) carries as much, so the two
      differ by at most 2 (K + 1) u sum|a||b|.  A float32 result adds its single rounding: at most one float32 ulp of
      the reference.  The means are sums of at most n terms: within n u sum|x| of numpy's, and bit-equal to the
      restatement of the kernel's own order (slabs in row order, slabs in slab order, one division).
  (d) Against sklearn's full-SVD PCA on the golden embeddings.  dC, the error of the covariance in the Frobenius norm,
      follows from (b) entry by entry (plus n |dmean|^2, the whole effect of an inexact mean on a centred Gram matrix);
      both decompositions are backward stable, which adds EIG = 8 d u |C| (LAPACK's c eps |C| with c = 8 d for each of
      the two).  Weyl: eigenvalues move by at most |dC| + EIG.  Davis-Kahan: the sine of the angle of component k is at
      most 2 (|dC| + EIG) / gap_k, with gap_k from the REFERENCE spectrum, and 1 - |cos| <= sine; the cosine itself is
      a float64 dot product of d terms, d u.
"""
import csv
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from parity_log import parity

from test_gpu_cluster import rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "simsiam_preds_subset.npz"
U, V = 2.0 ** -53, 2.0 ** -24

# n in {1, 3, 4, 5, 63, 64, 65, 1000, 4097} x d in {4, 12, 16, 20, 52, 64, 68, 512, 1028, 2052}: below, at and above the
# 16-wide MFMA tile, the 64-wide workgroup tile and the 16-row K step; several tiles, several slices (4097 x 64: 17),
# d above 1024.  Each with a handful of m from {1, 2, 15, 16, 17, 50, d}.
PAIRS = [(1, 4), (3, 12), (4, 16), (5, 20), (63, 52), (64, 64), (65, 68), (1000, 512), (4097, 64), (4097, 20), (1000, 1028),
         (65, 2052)]
M_OF = {4: (1, 2, 4), 12: (1, 2, 12), 16: (2, 15, 16), 20: (1, 17, 20), 52: (16, 17, 50, 52), 64: (1, 15, 50, 64),
        68: (2, 17, 68), 512: (16, 50, 512), 1028: (15, 50, 1028), 2052: (1, 17, 2052)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def D():
    from ssl_wafermap_amd import decomposition

    return decomposition


def integer_rows(n, d, seed, lo=-64, hi=64):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)


def worst(diff, bound):
    """max diff / bound; where the bound is exactly 0 the difference must be."""
    diff, bound = np.asarray(diff, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    zero = bound == 0
    assert (diff[zero] == 0).all(), "a zero bound needs an exact result"
    return float((diff[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def ulp32(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def slab_rows(n):
    """csrc/pca.hip: 256 rows while that gives at most 1024 slabs; above, ceil(n / 1024) rounded up to a multiple of 256."""
    if n <= 256 * 1024:
        return 256
    per = -(-n // 1024)
    return -(-per // 256) * 256


def restated_mean(x):
    """The kernel's order in numpy float64 (cumsum adds strictly in index order): rows of a slab in row order, the slab
    sums in slab order, one division."""
    x64, n, r = x.astype(np.float64), x.shape[0], slab_rows(x.shape[0])
    parts = np.stack([np.cumsum(x64[i:i + r], axis=0)[-1] for i in range(0, n, r)])
    return np.cumsum(parts, axis=0)[-1] / float(n)


# ------------------------------------------------------------------------------------------------ (a) exact


@pytest.mark.parametrize("n, d", PAIRS)
def test_exact_on_integer_data_without_a_mean(n, d):
    x = integer_rows(n, d, 7 * n + d)
    x64 = x.astype(np.float64)
    xd = dev(x)
    assert np.array_equal(host(D().gram(xd)), x64.T @ x64), "gram"
    assert np.array_equal(host(D().column_means(xd)), x64.sum(0) / n), "mean"
    rng = np.random.default_rng(n + d)
    for m in M_OF[d]:
        w = rng.integers(-4096, 4097, size=(m, d)).astype(np.float64)  # sums pass 2^24: the float32 rounding is real
        assert np.array_equal(host(D().project(xd, w)), (x64 @ w.T).astype(np.float32)), f"project m={m}"
        y = integer_rows(n, m, 3 * n + m)
        ws = rng.integers(-64, 65, size=(m, d)).astype(np.float64)  # |sum| <= 2052 * 4096 < 2^24: float32 holds it exactly
        want = y.astype(np.float64) @ ws
        got = host(D().reconstruct(dev(y), ws))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), f"reconstruct m={m}"


@pytest.mark.parametrize("n, d, m", [(65, 68, 17), (1000, 512, 50), (4, 16, 2)])
def test_exact_with_an_exactly_representable_mean(n, d, m):
    """Rows mu + z with the z in +- pairs (and one zero row when n is odd), shuffled: every column sums to n mu."""
    rng = np.random.default_rng(n)
    mu = rng.integers(-16, 17, size=d).astype(np.float64)
    half = rng.integers(-32, 33, size=(n // 2, d)).astype(np.float64)
    z = np.concatenate([half, -half] + ([np.zeros((1, d))] if n % 2 else []))[rng.permutation(n)]
    xd = dev((z + mu).astype(np.float32))
    mean = D().column_means(xd)
    assert np.array_equal(host(mean), mu)
    assert np.array_equal(host(D().gram(xd, mean)), z.T @ z)
    got_mean, cov = D().covariance(xd)
    assert np.array_equal(host(got_mean), mu) and np.array_equal(host(cov), (z.T @ z) / float(n - 1))
    w = rng.integers(-4096, 4097, size=(m, d)).astype(np.float64)
    assert np.array_equal(host(D().project(xd, w, mean)), (z @ w.T).astype(np.float32))
    y = integer_rows(n, m, n + m)
    ws = rng.integers(-64, 65, size=(m, d)).astype(np.float64)
    assert np.array_equal(host(D().reconstruct(dev(y), ws, mean)).astype(np.float64), y.astype(np.float64) @ ws + mu)


# ------------------------------------------------------------------------------------------------ (b) general data


@pytest.mark.parametrize("n, d", PAIRS + [(262400, 4)])  # the last: slabs of 512 rows, 513 of them
def test_means_against_float64(n, d):
    x = rows(n, d, 11 * n + d)
    got = host(D().column_means(dev(x)))
    assert np.array_equal(got, restated_mean(x)), "not the stated slab order"
    x64 = x.astype(np.float64)
    parity(f"pca mean n={n} d={d} / bound", worst(np.abs(got - x64.mean(0)), n * U * np.abs(x64).sum(0)), 1.0)


@pytest.mark.parametrize("n, d", PAIRS)
def test_gram_project_reconstruct_against_float64(n, d):
    x = rows(n, d, 13 * n + d)
    xd = dev(x)
    mean_d = D().column_means(xd)
    xc = x.astype(np.float64) - host(mean_d)  # one rounding per element, the kernel's own
    for tag, a, mu in (("centred", xc, mean_d), ("raw", x.astype(np.float64), None)):
        got = host(D().gram(xd, mu))
        bound = 2 * (n + 1) * U * (np.abs(a).T @ np.abs(a))
        parity(f"pca gram {tag} n={n} d={d} / bound", worst(np.abs(got - a.T @ a), bound), 1.0)
    rng = np.random.default_rng(n * d)
    for m in M_OF[d]:
        w = rng.standard_normal((m, d)) / np.sqrt(d)
        ref = xc @ w.T
        bound = ulp32(ref) + 2 * (d + 1) * U * (np.abs(xc) @ np.abs(w).T)
        parity(f"pca project n={n} d={d} m={m} / bound", worst(np.abs(host(D().project(xd, w, mean_d)) - ref), bound), 1.0)
        y = rng.standard_normal((n, m)).astype(np.float32)
        mu = host(mean_d)
        ref = y.astype(np.float64) @ w + mu
        bound = ulp32(ref) + 2 * (m + 2) * U * (np.abs(y).astype(np.float64) @ np.abs(w) + np.abs(mu))  # (+ mean: one more term)
        got = host(D().reconstruct(dev(y), w, mean_d))
        parity(f"pca reconstruct n={n} d={d} m={m} / bound", worst(np.abs(got - ref), bound), 1.0)


# ------------------------------------------------------------------------------------------------ (c) symmetry, determinism, padding


@pytest.mark.parametrize("n, d, m", [(5, 20, 17), (65, 68, 17), (1000, 512, 50), (4097, 64, 15)])
def test_symmetric_deterministic_and_blind_to_rows_behind_n(n, d, m):
    x = rows(n, d, 17 * n + d)
    xd = dev(x)
    mean = D().column_means(xd)
    g = D().gram(xd, mean)
    assert torch.equal(g, g.t().contiguous()), "out != out^T"
    w = np.random.default_rng(d).standard_normal((m, d))
    p = D().project(xd, w, mean)
    r = D().reconstruct(p, w, mean)
    junk = np.full((70, d), 1e30, dtype=np.float32)
    junk[::2] = np.nan
    for name, again in (("same call", xd), ("rows appended behind n", dev(np.concatenate([x, junk]))[:n])):
        assert torch.equal(D().column_means(again), mean), name
        assert torch.equal(D().gram(again, mean), g), name
        assert torch.equal(D().project(again, w, mean), p), name
    p_big = torch.cat([p, torch.full((70, m), float("nan"), device=DEV)])[:n]
    assert torch.equal(D().reconstruct(p_big, w, mean), r) and torch.equal(D().reconstruct(p, w, mean), r)
    # features padded to a multiple of 4 by the host centre to exact zeros and change nothing
    if d > 4:
        g3 = D().gram(xd[:, : d - 3].contiguous(), mean[: d - 3])
        assert torch.equal(g3, g[: d - 3, : d - 3])


# ------------------------------------------------------------------------------------------------ (d) sklearn, golden embeddings


@pytest.fixture(scope="module")
def golden():
    """The golden embeddings, sklearn's references and the error budget of the covariance, computed once."""
    from sklearn.decomposition import PCA as SkPCA

    z = np.load(GOLDEN)
    x = z["embeddings"].astype(np.float32)
    x64 = x.astype(np.float64)
    n, d = x.shape
    ref = SkPCA(16, svd_solver="full").fit(x64)
    xc = x64 - x64.mean(0)
    spectrum = np.linalg.eigvalsh(xc.T @ xc / (n - 1))[::-1]  # only for the gap behind component 15
    absx = np.abs(xc)
    d_gram = 2 * (n + 1) * U * (absx.T @ absx)
    d_mean = U * np.abs(x64).sum(0)
    dc = (np.linalg.norm(d_gram) + n * float(d_mean @ d_mean)) / (n - 1)
    eig = 8 * d * U * ref.explained_variance_[0]
    lam = np.concatenate([ref.explained_variance_, spectrum[16:17]])
    gap = np.minimum(np.concatenate([[np.inf], lam[:15] - lam[1:16]]), lam[:16] - lam[1:17])
    xd = dev(x)
    return {"x64": x64, "xd": xd, "ref": ref, "tol": dc + eig, "gap": gap, "dk": 2 * (dc + eig) / gap + d * U,
            "labels": z["labels"], "model": D().PCA(16).fit(xd)}


def test_golden_components_against_sklearn(golden):
    ref, tol, x64, model = golden["ref"], golden["tol"], golden["x64"], golden["model"]
    n, d = x64.shape
    assert model.n_components_ == 16 and model.components_.shape == (16, d)
    assert (model.n_samples_, model.n_features_in_) == (n, d)
    parity("pca golden explained_variance_ / (Weyl bound)", np.abs(model.explained_variance_ - ref.explained_variance_).max() / tol, 1.0)
    parity("pca golden mean_ / bound", worst(np.abs(model.mean_ - ref.mean_), 2 * U * np.abs(x64).sum(0)), 1.0)
    # a ratio l / T: l moves by at most tol and the total T, a sum of d eigenvalues, by at most d tol
    total = ref.explained_variance_[0] / ref.explained_variance_ratio_[0]
    parity("pca golden explained_variance_ratio_ / bound",
           np.abs(model.explained_variance_ratio_ - ref.explained_variance_ratio_).max() / ((d + 1) * tol / total), 1.0)
    parity("pca golden singular_values_ rel", np.abs(model.singular_values_ / ref.singular_values_ - 1).max(),
           (tol / ref.explained_variance_[-1]))  # sqrt halves a relative error; the smallest eigenvalue sets it
    parity("pca golden noise_variance_ / bound", abs(model.noise_variance_ - ref.noise_variance_) / tol, 1.0)
    cos = np.abs(np.einsum("kd,kd->k", model.components_, ref.components_))
    parity("pca golden components 1 - |cos| / (Davis-Kahan bound)", ((1 - cos) / golden["dk"]).max(), 1.0)
    # signs: only where the reference's largest entry is not tied with its runner-up
    mags = np.sort(np.abs(ref.components_), axis=1)
    clear = np.flatnonzero(mags[:, -2] / mags[:, -1] <= 0.99)
    assert clear.size >= 14, f"only {clear.size} of 16 reference components have an untied largest entry"
    assert (np.einsum("kd,kd->k", model.components_, ref.components_)[clear] > 0).all()
    lead = np.argmax(np.abs(model.components_), axis=1)
    assert (model.components_[np.arange(16), lead] > 0).all()


def test_golden_variance_fraction_against_sklearn(golden):
    from sklearn.decomposition import PCA as SkPCA

    want = SkPCA(0.95, svd_solver="full").fit(golden["x64"]).n_components_
    got = D().PCA(0.95).fit(golden["xd"]).n_components_
    assert got == want == 16


def test_golden_transform_and_reconstruction_against_sklearn(golden):
    ref, x64, xd, model, dk = golden["ref"], golden["x64"], golden["xd"], golden["model"], golden["dk"]
    n, d = x64.shape
    y = model.transform(xd)
    assert torch.equal(D().PCA(16).fit_transform(xd), y)
    want_ref = ref.transform(x64)
    # a component whose largest entry is tied with its runner-up in the reference has no determined sign (the test above
    # compares signs for the others): compare it up to that sign
    want = want_ref * np.sign(np.einsum("kd,kd->k", model.components_, ref.components_))
    xc = x64 - ref.mean_
    # float32 rounding + accumulation + the rotation of the component inside its Davis-Kahan angle: |w - w_ref| <= sqrt(2) sine
    bound = ulp32(want) + 2 * (d + 1) * U * (np.abs(xc) @ np.abs(ref.components_).T) + np.linalg.norm(xc, axis=1)[:, None] * np.sqrt(2) * dk
    # sklearn centres AFTER projecting (x W^T - mean W^T): its own cancellation, two dot products of d terms
    bound += 2 * (d + 1) * U * (np.abs(x64) @ np.abs(ref.components_).T + np.abs(ref.mean_) @ np.abs(ref.components_).T)
    parity("pca golden transform / bound", worst(np.abs(host(y) - want), bound), 1.0)
    assert np.abs(host(y)).max() > 100  # (the outputs reach about 214: the float32 ulp in the bound is a real one)
    back = host(model.inverse_transform(y)).astype(np.float64)
    rel = np.linalg.norm(x64 - back) / np.linalg.norm(x64)
    rel_ref = np.linalg.norm(x64 - ref.inverse_transform(want_ref)) / np.linalg.norm(x64)
    # y and the reconstruction are each rounded to float32 once: |back - back_ref|_F <= 2 v |x|_F to first order, which moves
    # the quotient by at most 2 v; the components' own error (1e-10) is far below; doubled for the second order
    parity("pca golden relative reconstruction error vs sklearn, abs", abs(rel - rel_ref), 4 * V)


def test_golden_whitened_outputs_have_unit_variance(golden):
    model = D().PCA(16, whiten=True)
    y = host(model.fit_transform(golden["xd"])).astype(np.float64)
    # each output carries one float32 rounding (relative v): the variance moves by at most 2 v to first order; doubled
    parity("pca golden whitened variance - 1, abs", np.abs(y.var(0, ddof=1) - 1.0).max(), 4 * V)
    back = host(model.inverse_transform(model.transform(golden["xd"]))).astype(np.float64)
    plain = D().PCA(16).fit(golden["xd"])
    want = host(plain.inverse_transform(plain.transform(golden["xd"]))).astype(np.float64)
    # the same reconstruction through the whitened coordinates: two more float32 roundings of values up to max |x|
    assert np.abs(back - want).max() <= 8 * V * np.abs(golden["x64"]).max()


# ------------------------------------------------------------------------------------------------ (e) the script


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_on_golden_embeddings(golden, tmp_path, capsys):
    from ssl_wafermap_amd.decomposition import effective_rank, participation_ratio

    summary = load_script("embedding_pca_amd").main(["--embeddings", str(GOLDEN), "--variance", "0.95", "--holdout", "1000",
                                                     "--out", str(tmp_path)])
    x64 = golden["x64"]
    n, d = x64.shape
    fit = x64[: n - 1000]
    m = summary["n_components"]
    z = np.load(tmp_path / "reduced.npz")
    assert z["embeddings"].shape == (n, m) and z["embeddings"].dtype == np.float32 and np.array_equal(z["labels"], golden["labels"])
    assert np.load(tmp_path / "components.npy").shape == (m, d) and np.load(tmp_path / "mean.npy").shape == (d,)
    with open(tmp_path / "spectrum.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == d and list(table[0]) == ["eigenvalue", "ratio", "cumulative"]
    assert json.loads((tmp_path / "summary.json").read_text())["n_components"] == m
    # the references, recomputed from the same rows in float64
    assert (np.ptp(x64, axis=0) == 0).sum() == 393  # (the whole golden matrix; the fitted rows have one more)
    assert summary["zero_variance_columns"] == int((np.ptp(fit, axis=0) == 0).sum())
    fc = fit - fit.mean(0)
    lam = np.clip(np.linalg.eigvalsh(fc.T @ fc / (fit.shape[0] - 1))[::-1], 0, None)
    ratio = lam / lam.sum()
    assert m == int(np.searchsorted(np.cumsum(ratio), 0.95, side="right")) + 1
    # both are smooth functions of the spectrum; eigenvalues at rounding level (1e-16 of the total) weigh p log p ~ 4e-15 each
    assert summary["effective_rank"] == pytest.approx(effective_rank(lam), rel=1e-9)
    assert summary["participation_ratio"] == pytest.approx(participation_ratio(lam), rel=1e-9)
    assert summary["components_for_variance"]["95"] == m and summary["holdout"] == 1000
    # keeping 95 % of the variance leaves sqrt(1 - kept) of the centred norm
    kept = float(ratio[:m].sum())
    # (the two float32 roundings, of y and of the reconstruction, are at most 2 v |x|_F each relative to |x - mean|_F)
    assert summary["relative_reconstruction_error"] == pytest.approx(np.sqrt(1 - kept), abs=4 * V * np.linalg.norm(fit) / np.linalg.norm(fc))
    assert 0 < summary["holdout_relative_reconstruction_error"] < 1
    assert "effective rank" in capsys.readouterr().out
    # the reduced matrix is what the KMeans script reads
    km = load_script("embedding_kmeans_amd").main(["--embeddings", str(tmp_path / "reduced.npz"), "--k", "4", "--n-init", "1",
                                                   "--no-scale", "--out", str(tmp_path / "km")])
    assert km["d"] == m and km["n"] == n and np.load(tmp_path / "km" / "labels.npy").shape == (n,)
