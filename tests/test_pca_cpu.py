"""CPU checks of decomposition.py's host side: `pca_from_covariance` against sklearn's full-SVD PCA on covariances numpy
computes in float64, the rank diagnostics on spectra with known answers, argument errors, and the size limits of the
PCA entry points (no launch).

Tolerances: both routes are backward-stable float64 decompositions of the same data, so eigenvalues agree to a few
eps * ||C|| and a component to eps * ||C|| / gap; the test matrices have well separated spectra (gap / ||C|| above 1e-3),
which leaves 1e-10 with three orders to spare."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["wm_pca_mean", "wm_pca_gram", "wm_pca_project", "wm_pca_reconstruct"]


def data(n, d, seed):
    """float64 rows with a decaying, well separated spectrum."""
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.standard_normal((d, d)))
    scales = 3.0 * 0.7 ** np.arange(d)
    return (rng.standard_normal((n, d)) * scales) @ basis.T + rng.standard_normal(d)


@pytest.mark.parametrize("n, d", [(200, 12), (40, 9), (8, 12)])
@pytest.mark.parametrize("n_components", [None, 1, 3, 0.5, 0.9, 0.999])
def test_pca_from_covariance_against_sklearn_full(n, d, n_components):
    from sklearn.decomposition import PCA as SkPCA

    from ssl_wafermap_amd.decomposition import pca_from_covariance

    x = data(n, d, 100 * n + d)
    ref = SkPCA(n_components, svd_solver="full").fit(x)
    got = pca_from_covariance(np.cov(x, rowvar=False), n, n_components)
    m = ref.n_components_
    assert got.n_components == m and got.components.shape == (m, d)
    scale = ref.explained_variance_[0]
    # behind rank n - 1 the directions are arbitrary and the eigenvalues rounding noise: compare what is determined
    r = min(m, n - 1)
    assert np.abs(got.explained_variance - ref.explained_variance_).max() <= 1e-10 * scale
    assert np.abs(got.explained_variance_ratio - ref.explained_variance_ratio_).max() <= 1e-10
    assert np.abs(got.singular_values - ref.singular_values_).max() <= 1e-6 * ref.singular_values_[0]  # (sqrt near 0)
    assert np.abs(got.singular_values[:r] - ref.singular_values_[:r]).max() <= 1e-10 * ref.singular_values_[0]
    assert abs(got.noise_variance - ref.noise_variance_) <= 1e-10 * scale
    assert np.abs(got.components[:r] - ref.components_[:r]).max() <= 1e-10
    assert (got.explained_variance >= 0).all() and (np.diff(got.explained_variance) <= 0).all()


def test_sign_rule_and_clipping():
    from ssl_wafermap_amd.decomposition import pca_from_covariance

    # eigenvectors (3, -4) / 5 and (4, 3) / 5: the larger entry of each must come out positive
    v = np.array([[3.0, -4.0], [4.0, 3.0]]) / 5.0
    cov = v.T @ np.diag([2.0, 1.0]) @ v
    got = pca_from_covariance(cov, 10)
    assert np.allclose(got.components, [[-0.6, 0.8], [0.8, 0.6]], atol=1e-14)
    lead = np.argmax(np.abs(got.components), axis=1)
    assert (got.components[np.arange(2), lead] > 0).all()
    # a slightly negative eigenvalue (rounding of a singular covariance) is clipped to 0, not passed on
    got = pca_from_covariance(np.diag([1.0, -1e-18, 0.0]), 10)
    assert got.explained_variance.tolist() == [1.0, 0.0, 0.0] and got.explained_variance_ratio.tolist() == [1.0, 0.0, 0.0]
    assert got.singular_values.tolist() == [3.0, 0.0, 0.0]


def test_whiten_scale_matches_sklearn():
    from sklearn.decomposition import PCA as SkPCA

    from ssl_wafermap_amd.decomposition import PCA, pca_from_covariance

    x = data(300, 10, 5)
    ref = SkPCA(4, whiten=True, svd_solver="full").fit(x)
    res = pca_from_covariance(np.cov(x, rowvar=False), 300, 4)
    model = PCA(4, whiten=True)
    model.components_, model.explained_variance_, model.noise_variance_ = res.components, res.explained_variance, res.noise_variance
    got = (x - x.mean(0)) @ model._forward_matrix().T
    assert np.abs(got - ref.transform(x)).max() <= 1e-10 * np.abs(got).max()
    back = got @ model._backward_matrix() + x.mean(0)
    assert np.abs(back - ref.inverse_transform(ref.transform(x))).max() <= 1e-10 * np.abs(x).max()
    assert np.abs(model.get_covariance() - ref.get_covariance()).max() <= 1e-10 * np.abs(ref.get_covariance()).max()
    plain = PCA(4)
    plain.components_, plain.explained_variance_, plain.noise_variance_ = res.components, res.explained_variance, res.noise_variance
    want = SkPCA(4, svd_solver="full").fit(x).get_covariance()
    assert np.abs(plain.get_covariance() - want).max() <= 1e-10 * np.abs(want).max()
    # sklearn's floor: a zero variance divides by the float64 epsilon, not by zero
    model.explained_variance_ = np.array([4.0, 1.0, 0.0, 0.0])
    assert model._scale().tolist() == [2.0, 1.0, np.finfo(np.float64).eps, np.finfo(np.float64).eps]


def test_rank_diagnostics_on_known_spectra():
    from ssl_wafermap_amd.decomposition import effective_rank, participation_ratio

    for k in (1, 2, 7, 512):
        assert effective_rank(np.full(k, 0.37)) == pytest.approx(k, rel=1e-12)
        assert participation_ratio(np.full(k, 0.37)) == pytest.approx(k, rel=1e-12)
    one = np.array([0.0, 5.0, 0.0, 0.0])  # zeros carry no mass: 0 log 0 = 0
    assert effective_rank(one) == 1.0 and participation_ratio(one) == 1.0
    # p = (1/2, 1/4, 1/4): entropy 1.5 ln 2; (sum)^2 / sum of squares = 16 / 6
    assert effective_rank([2.0, 1.0, 1.0]) == pytest.approx(2.0 ** 1.5, rel=1e-12)
    assert participation_ratio([2.0, 1.0, 1.0]) == pytest.approx(16.0 / 6.0, rel=1e-12)
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [np.nan]):
        with pytest.raises(ValueError):
            effective_rank(bad)
        with pytest.raises(ValueError):
            participation_ratio(bad)


def test_argument_errors():
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd import decomposition as D

    cov = np.eye(4)
    with pytest.raises(NotImplementedError, match="mle"):
        D.PCA("mle")
    with pytest.raises(NotImplementedError, match="mle"):
        D.pca_from_covariance(cov, 10, "mle")
    for bad in (0, -1, 5, 0.0, 1.0, 1.5, "auto", True, [2]):
        with pytest.raises(ValueError):
            D.pca_from_covariance(cov, 10, bad)
    with pytest.raises(ValueError):
        D.pca_from_covariance(cov, 3, 4)  # more components than rows
    for bad in (0, -2, 1.0, "auto"):
        with pytest.raises(ValueError):
            D.PCA(bad)
    with pytest.raises(ValueError):
        D.pca_from_covariance(np.zeros((3, 4)), 10)
    with pytest.raises(ValueError):
        D.pca_from_covariance(cov, 1)
    x = torch.zeros(8, 4)
    for call in (lambda: D.column_means(x), lambda: D.covariance(x), lambda: D.gram(x), lambda: D.project(x, np.eye(4)),
                 lambda: D.reconstruct(x, np.eye(4)), lambda: D.PCA(2).fit(x), lambda: D.PCA(2).fit_transform(x)):
        with pytest.raises(_lib.WaferHipError):  # CPU tensors: no fallback, as the rest of the package
            call()
    with pytest.raises(RuntimeError, match="fit"):
        D.PCA(2).transform(x)
    with pytest.raises(RuntimeError, match="fit"):
        D.PCA(2).inverse_transform(x)
    m = D.PCA()
    assert (m.n_components, m.whiten) == (None, False)


def test_new_symbols_are_declared_and_typed():
    from ssl_wafermap_amd import _lib

    header = (ROOT / "include" / "wafer_hip.h").read_text()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        for sym in (name, name + "_workspace_bytes"):
            assert re.search(rf"\b{sym}\s*\(", header), f"{sym} is not declared in wafer_hip.h"
            assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        # workspace, workspace_bytes, stream come last
        assert _lib.SIGNATURES[name][1][-3:] == [_lib.c_void_p, _lib.c_size_t, _lib.c_void_p]


def test_entry_points_refuse_without_a_launch():
    from ssl_wafermap_amd import _lib

    lib = _lib.load()
    for fn in (lib.wm_pca_mean_workspace_bytes, lib.wm_pca_gram_workspace_bytes):
        assert fn(1, 4) > 0 and fn(12449, 512) > 0 and fn(1 << 24, 4096) > 0
        assert fn(0, 512) == 0 and fn((1 << 24) + 1, 512) == 0  # n
        assert fn(100, 510) == 0 and fn(100, 4100) == 0 and fn(100, 0) == 0  # d % 4, d <= 4096
    for fn in (lib.wm_pca_project_workspace_bytes,):
        assert fn(1, 4, 1) > 0 and fn(1000, 512, 512) > 0
        assert fn(1000, 512, 0) == 0 and fn(1000, 512, 513) == 0 and fn(1000, 510, 2) == 0 and fn(0, 512, 2) == 0
    fn = lib.wm_pca_reconstruct_workspace_bytes  # (n, m, d)
    assert fn(1, 1, 4) > 0 and fn(1000, 512, 512) > 0
    assert fn(1000, 0, 512) == 0 and fn(1000, 513, 512) == 0 and fn(1000, 2, 510) == 0 and fn(0, 2, 512) == 0
    # the slice cap: the Gram workspace is whole d x d planes and stays at or below 512 MiB
    for n, d in ((1 << 24, 4096), (811457, 512), (1 << 24, 1024), (300, 4096)):
        b = lib.wm_pca_gram_workspace_bytes(n, d)
        assert b % (d * d * 8) == 0 and b <= 512 << 20
    # the slab rule of the means: 256 rows up to 1024 slabs
    assert lib.wm_pca_mean_workspace_bytes(257, 4) == 2 * 4 * 8
    assert lib.wm_pca_mean_workspace_bytes(262144, 4) == 1024 * 4 * 8
    assert lib.wm_pca_mean_workspace_bytes(262145, 4) == 513 * 4 * 8  # slabs of 512 rows
    assert lib.wm_pca_mean(None, 8, 4, None, None, 0, None) == -1
    assert lib.wm_pca_gram(None, 8, 4, None, None, None, 0, None) == -1
    assert lib.wm_pca_project(None, 8, 4, None, None, 2, None, None, 0, None) == -1
    assert lib.wm_pca_reconstruct(None, 8, 2, None, 4, None, None, None, 0, None) == -1
