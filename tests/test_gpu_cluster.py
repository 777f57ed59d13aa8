"""GPU checks of the clustering kernels (csrc/cluster.hip) and their Python layer (cluster.py,
scripts/embedding_clustering_amd.py) against float64 brute force and sklearn.

Bounds are derived, not tuned.  With u = 2^-24, one float32 distance carries one rounding per difference (twice in a
square), one per accumulation step and, for Euclidean, half of that plus the root's own rounding: at most
eps(d) = (d + 3) u relative (csrc/cluster.hip states the count).  Order statistics, minima and maxima of values within
eps are within eps; a silhouette value (b - a) / max(a, b) of sums within eps moves by at most 4 eps (2 eps from the
numerator relative to max(a, b), 2 eps through the quotient).  Where every distance is exactly representable (integer
lattices, with the Euclidean reference's root taken in float32, which numpy rounds correctly, as the kernel's sqrtf
does) results are equal."""
import numpy as np
import pytest
import torch
from parity_log import parity
from pathlib import Path

from cluster_cases import components, eps, max_rel, rows  # noqa: F401  (shared with the slice-level tests; sibling files import them from here)
from test_cluster_cpu import BLOB_PARAMS, lattice_points, pairwise64, prim_mst, same_clustering

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
METRICS = ["euclidean", "manhattan"]


_CACHE = {}


def reference(n, d, metric):
    """(x float32, float64 distance matrix), computed once per shape and shared."""
    key = (n, d, metric)
    if key not in _CACHE:
        x = rows(n, d, 1000 * n + d)
        _CACHE[key] = (x, pairwise64(x, metric))
    return _CACHE[key]


def lattice32(metric):
    """(x float32, distance matrix exactly as float32 arithmetic gives it) on the integer lattice."""
    x = lattice_points().astype(np.float32)
    diff = x[:, None, :] - x[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1, dtype=np.float32)) if metric == "euclidean" else np.abs(diff).sum(-1, dtype=np.float32)
    assert dist.dtype == np.float32
    return x, dist


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ core distances


@pytest.mark.parametrize("d", [4, 52, 512, 1024])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_core_distance_against_float64(n, d):
    from ssl_wafermap_amd import _lib, cluster

    for metric in METRICS:
        x, dist = reference(n, d, metric)
        ordered = np.sort(dist, axis=1)
        xd = dev(x)
        for k in [k for k in (1, 2, 16, 17, 64) if k <= n]:
            got = cluster.core_distances(xd, k, metric).cpu().numpy().astype(np.float64)
            want = ordered[:, k - 1]
            parity(f"core_distance {metric} n={n} d={d} k={k} rel", max_rel(got, want), eps(d))
            if k == 1:
                assert (got == 0).all()  # the self-distance counts as the first
            if k == 2 and n >= 8:
                assert (got[[0, 3, 5, 7, n - 1]] == 0).all()
        # k = n + 1: the argument error code, from the entry point itself
        lib = _lib.load()
        ws = torch.empty(max(lib.wm_core_distance_workspace_bytes(n, d, 1), 16), dtype=torch.uint8, device=DEV)
        out = torch.empty(n, dtype=torch.float32, device=DEV)
        rc = lib.wm_core_distance(xd.data_ptr(), n, d, cluster.METRICS[metric], n + 1, out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), 0)
        assert rc == -1
        with pytest.raises(ValueError):
            cluster.core_distances(xd, n + 1, metric)


# ------------------------------------------------------------------------------------------------ one Boruvka round


def brute_min_edge(dist, core, comp):
    w = np.maximum(np.maximum(core[:, None], core[None, :]), dist)
    w = np.where(comp[:, None] != comp[None, :], w, np.inf)
    return w, w.min(axis=1), w.argmin(axis=1)


@pytest.mark.parametrize("kind", ["singletons", "halves", "single"])
@pytest.mark.parametrize("n,d", [(65, 4), (65, 512), (300, 52), (300, 512), (2, 4)])
def test_min_edge_against_float64(n, d, kind):
    from ssl_wafermap_amd import cluster

    for metric in METRICS:
        x, dist = reference(n, d, metric)
        core32 = np.sort(dist, axis=1)[:, min(5, n) - 1].astype(np.float32)
        comp = components(n, kind)
        w_all, w_min, _ = brute_min_edge(dist, core32.astype(np.float64), comp)
        got_w, got_j = cluster.min_outgoing_edges(dev(x), dev(core32), dev(comp), metric)
        got_w, got_j = got_w.cpu().numpy().astype(np.float64), got_j.cpu().numpy()
        if kind == "single":
            assert (got_j == -1).all() and np.isposinf(got_w).all()
            continue
        assert (got_j >= 0).all() and (got_j < n).all() and (comp[got_j] != comp).all()
        parity(f"min_edge weight {metric} n={n} d={d} {kind} rel", max_rel(got_w, w_min), eps(d))
        parity(f"min_edge argmin {metric} n={n} d={d} {kind} rel", max_rel(w_all[np.arange(n), got_j], w_min), eps(d))


@pytest.mark.parametrize("kind", ["singletons", "halves", "single"])
@pytest.mark.parametrize("metric", METRICS)
def test_min_edge_exact_on_a_lattice(metric, kind):
    from ssl_wafermap_amd import cluster

    x, dist = lattice32(metric)
    n = x.shape[0]
    core32 = np.sort(dist, axis=1)[:, 3]
    got_core = cluster.core_distances(dev(x), 4, metric).cpu().numpy()
    assert np.array_equal(got_core, core32)
    comp = components(n, kind)
    for alpha in (1.0, 2.0):  # (a power of two scales exactly)
        _, w_min, j_min = brute_min_edge(dist / np.float32(alpha), core32, comp)
        got_w, got_j = cluster.min_outgoing_edges(dev(x), dev(core32), dev(comp), metric, alpha=alpha)
        if kind == "single":
            assert (got_j.cpu().numpy() == -1).all() and np.isposinf(got_w.cpu().numpy()).all()
        else:
            assert np.array_equal(got_w.cpu().numpy(), w_min.astype(np.float32))
            assert np.array_equal(got_j.cpu().numpy(), j_min), "equal weights must resolve to the lowest j"


# ------------------------------------------------------------------------------------------------ spanning tree


def check_tree(u, v, w, n):
    assert u.shape == v.shape == w.shape == (n - 1,)
    assert (u < v).all() and u.min() >= 0 and v.max() < n
    key = np.stack([w, u, v], axis=1)
    assert all(tuple(key[i]) <= tuple(key[i + 1]) for i in range(n - 2)), "edges must be sorted by (w, u, v)"
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        assert ra != rb, "cycle"
        parent[ra] = rb
    assert len({find(a) for a in range(n)}) == 1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [2, 65, 700])
def test_spanning_tree_against_float64_prim(n, metric):
    from ssl_wafermap_amd import cluster

    d, k = 52, min(5, n)
    x = rows(n, d, 7 + n)
    xd = dev(x)
    u, v, w, rounds = cluster.mutual_reachability_mst(xd, k, metric, return_rounds=True)
    check_tree(u, v, w, n)
    assert 1 <= rounds <= max(1, int(np.ceil(np.log2(n))))
    _, _, w_ref = prim_mst(x, k, metric)
    parity(f"mst total weight {metric} n={n} abs", abs(w.sum() - w_ref.sum()), n * eps(d) * w_ref.max())
    u2, v2, w2 = cluster.mutual_reachability_mst(xd, k, metric)
    assert np.array_equal(u, u2) and np.array_equal(v, v2) and np.array_equal(w.view(np.int64), w2.view(np.int64))


@pytest.mark.parametrize("metric", METRICS)
def test_spanning_tree_exact_on_a_lattice(metric):
    from ssl_wafermap_amd import cluster

    x, dist = lattice32(metric)
    n = x.shape[0]
    u, v, w = cluster.mutual_reachability_mst(dev(x), 4, metric)
    check_tree(u, v, w, n)
    # the float32 distances are exact here, so Prim on them in float64 sees the very same weights; every minimum
    # spanning tree has the same sorted weights
    core = np.sort(dist, axis=1)[:, 3].astype(np.float64)
    mr = np.maximum(np.maximum(core[:, None], core[None, :]), dist.astype(np.float64))
    best, seen, total = mr[0].copy(), np.zeros(n, dtype=bool), []
    seen[0] = True
    for _ in range(n - 1):
        j = int(np.argmin(np.where(seen, np.inf, best)))
        total.append(best[j])
        seen[j] = True
        best = np.minimum(best, mr[j])
    assert np.array_equal(np.sort(np.array(total)), w)
    assert np.array_equal(mr[u, v], w)


# ------------------------------------------------------------------------------------------------ labels


def sk_labels(x, min_samples, min_cluster_size, epsilon, **kw):
    from sklearn.cluster import HDBSCAN as SkHDBSCAN

    return SkHDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, cluster_selection_epsilon=epsilon,
                     algorithm="brute", copy=True, **kw).fit(np.asarray(x, dtype=np.float64)).labels_


@pytest.fixture(scope="module")
def blobs32():
    from sklearn.datasets import make_blobs

    x, _ = make_blobs(600, 16, centers=5, cluster_std=1.0, random_state=3)
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def wafers32():
    return np.load(GOLDEN / "simsiam_preds_subset.npz")["embeddings"][:1536].astype(np.float32)


@pytest.mark.parametrize("min_samples,min_cluster_size,epsilon", BLOB_PARAMS)
def test_fit_labels_match_sklearn_on_blobs(blobs32, min_samples, min_cluster_size, epsilon):
    from ssl_wafermap_amd import cluster

    model = cluster.HDBSCAN(min_cluster_size, min_samples, epsilon).fit(dev(blobs32))
    same_clustering(model.labels_, sk_labels(blobs32, min_samples, min_cluster_size, epsilon))
    assert model.minimum_spanning_tree_.shape == (599, 3) and model.probabilities_.shape == (600,)
    assert model.condensed_tree_.dtype.names == ("parent", "child", "lambda_val", "child_size")
    assert np.array_equal(cluster.HDBSCAN(min_cluster_size, min_samples, epsilon).fit_predict(dev(blobs32)), model.labels_)


def test_fit_labels_match_sklearn_on_wafer_embeddings(wafers32):
    from ssl_wafermap_amd import cluster

    ref = sk_labels(wafers32, 26, 75, 1.5)
    assert ref.max() + 1 == 2 and (ref == -1).sum() == 350  # the notebook's chosen parameters on these rows
    model = cluster.HDBSCAN(min_cluster_size=75, min_samples=26, cluster_selection_epsilon=1.5).fit(dev(wafers32))
    same_clustering(model.labels_, ref)
    # min_samples=None means min_cluster_size
    a = cluster.HDBSCAN(min_cluster_size=40).fit(dev(wafers32))
    b = cluster.HDBSCAN(min_cluster_size=40, min_samples=40).fit(dev(wafers32))
    assert np.array_equal(a.labels_, b.labels_) and np.array_equal(a.minimum_spanning_tree_, b.minimum_spanning_tree_)


def test_fit_labels_within_sklearns_own_sensitivity(wafers32):
    """(min_samples, min_cluster_size, epsilon) = (5, 15, 0) on the wafer embeddings: sklearn's own labels move under
    rounding-sized changes of the input, so the bound is sklearn's worst adjusted Rand index against its own labels
    over three seeded 1e-4-relative perturbations, computed here; ours against sklearn must be no lower, with the
    same number of clusters."""
    from sklearn.metrics import adjusted_rand_score

    from ssl_wafermap_amd import cluster

    ref = sk_labels(wafers32, 5, 15, 0.0)
    worst = 1.0
    for seed in range(3):
        noise = np.random.default_rng(seed).uniform(-1.0, 1.0, wafers32.shape)
        worst = min(worst, adjusted_rand_score(ref, sk_labels(wafers32.astype(np.float64) * (1.0 + 1e-4 * noise), 5, 15, 0.0)))
    model = cluster.HDBSCAN(min_cluster_size=15, min_samples=5).fit(dev(wafers32))
    parity("hdbscan (5, 15, 0) ARI vs sklearn (bound: sklearn under 1e-4 perturbations)",
           adjusted_rand_score(ref, model.labels_), worst, higher=True)
    assert model.labels_.max() == ref.max()


def test_refit_equals_a_fresh_fit(wafers32):
    from ssl_wafermap_amd import cluster

    xd = dev(wafers32)
    model = cluster.HDBSCAN(min_cluster_size=15, min_samples=26).fit(xd)
    first = model.labels_.copy()
    model.refit(min_cluster_size=75, cluster_selection_epsilon=1.5)
    fresh = cluster.HDBSCAN(min_cluster_size=75, min_samples=26, cluster_selection_epsilon=1.5).fit(xd)
    assert np.array_equal(model.labels_, fresh.labels_) and np.array_equal(model.probabilities_, fresh.probabilities_)
    assert np.array_equal(model.condensed_tree_, fresh.condensed_tree_)
    assert np.array_equal(model.refit(min_cluster_size=15, cluster_selection_epsilon=0.0).labels_, first)


# ------------------------------------------------------------------------------------------------ scores


def cluster_labels(n, n_clusters, seed):
    """Labels 0..n_clusters-1 in shuffled order, every cluster used, cluster 0 a singleton; then -1 on a few rows."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.arange(n_clusters), rng.integers(1, n_clusters, n - n_clusters)])
    rng.shuffle(lab)
    return lab.astype(np.int64)


@pytest.mark.parametrize("n,d,n_clusters", [(2, 4, 2), (65, 4, 2), (65, 52, 3), (65, 512, 37), (300, 52, 37), (300, 512, 3)])
def test_cluster_distance_sums_against_float64(n, d, n_clusters):
    from ssl_wafermap_amd import cluster

    for metric in METRICS:
        x, dist = reference(n, d, metric)
        lab = cluster_labels(n, n_clusters, n + d)
        if n > 2:
            lab[1::9] = -1
        want = np.stack([dist[:, lab == c].sum(axis=1) for c in range(n_clusters)], axis=1)
        got = cluster.cluster_distance_sums(dev(x), dev(lab.astype(np.int32)), n_clusters, metric).cpu().numpy()
        keep = lab >= 0
        parity(f"dist_sums {metric} n={n} d={d} C={n_clusters} rel", max_rel(got[keep], want[keep]), eps(d))
        again = cluster.cluster_distance_sums(dev(x), dev(lab.astype(np.int32)), n_clusters, metric).cpu().numpy()
        assert np.array_equal(got[keep].view(np.int64), again[keep].view(np.int64))


@pytest.mark.parametrize("n,d,n_clusters", [(65, 4, 2), (65, 52, 3), (65, 512, 37), (300, 4, 37), (300, 52, 2), (300, 512, 3)])
def test_silhouette_against_sklearn(n, d, n_clusters):
    """n = 2 is covered at the kernel (test_cluster_distance_sums_against_float64) and by the error below: a
    silhouette needs n_clusters <= n - 1, here as in sklearn."""
    from sklearn import metrics

    from ssl_wafermap_amd import cluster

    for metric in METRICS:
        x, _ = reference(n, d, metric)
        lab = cluster_labels(n, n_clusters, 3 * n + d)
        lab[np.flatnonzero(lab != 0)[2::11]] = -1  # (the singleton cluster 0 stays)
        keep = lab != -1  # the caller drops noise, as the notebook does
        xs, ls = x[keep], lab[keep]
        want = metrics.silhouette_samples(xs.astype(np.float64), ls, metric=metric)
        got = cluster.silhouette_samples(dev(xs), ls, metric)
        assert got.dtype == torch.float64 and got.is_cuda
        got = got.cpu().numpy()
        counts = np.bincount(ls, minlength=n_clusters)
        assert (counts == 1).any() and (got[counts[ls] == 1] == 0).all()  # singleton clusters score 0
        parity(f"silhouette {metric} n={n} d={d} C={n_clusters} abs", np.max(np.abs(got - want)), 4 * eps(d))
        score = cluster.silhouette_score(dev(xs), torch.from_numpy(ls).to(DEV), metric)
        assert abs(score - want.mean()) <= 4 * eps(d)
    with pytest.raises(ValueError):
        cluster.silhouette_samples(dev(np.zeros((2, 4), dtype=np.float32)), np.array([0, 1]))


def test_other_scores_against_sklearn(blobs32):
    """Calinski-Harabasz, Davies-Bouldin and homogeneity are float64 on the host: 1e-10 relative."""
    from sklearn import metrics

    from ssl_wafermap_amd import cluster

    rng = np.random.default_rng(1)
    lab, truth = rng.integers(0, 6, 600), rng.integers(0, 9, 600)
    x64 = blobs32.astype(np.float64)
    for name, ours, theirs in (
            ("calinski_harabasz", cluster.calinski_harabasz_score(dev(blobs32), lab), metrics.calinski_harabasz_score(x64, lab)),
            ("davies_bouldin", cluster.davies_bouldin_score(dev(blobs32), dev(lab)), metrics.davies_bouldin_score(x64, lab)),
            ("homogeneity", cluster.homogeneity_score(truth, lab), metrics.homogeneity_score(truth, lab))):
        parity(f"{name} rel", abs(ours - theirs) / abs(theirs), 1e-10)


# ------------------------------------------------------------------------------------------------ the script


def test_sweep_script_on_wafer_embeddings(tmp_path, capsys):
    import csv
    import importlib.util

    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", ROOT / "scripts" / "embedding_clustering_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    summary = mod.main(["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "1536", "--trials", "4",
                        "--metrics", "euclidean", "--seed", "0", "--out", str(tmp_path)])
    with open(tmp_path / "trials.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == 4 and list(table[0]) == mod.COLUMNS
    for row in table:
        assert all(np.isfinite(float(row[c])) for c in mod.COLUMNS if c != "metric"), row
        assert int(row["n_clusters"]) >= 2 and -1 <= float(row["silhouette"]) <= 1 and 0 <= float(row["homogeneity"]) <= 1
    assert summary["n_trees"] == len({row["min_samples"] for row in table}) < 4
    with open(tmp_path / "pareto.csv") as fh:
        assert 1 <= len(list(csv.DictReader(fh))) <= 4
    labels = np.load(tmp_path / "labels.npy")
    assert labels.shape == (1536,) and labels.max() + 1 == int(table[summary["chosen"]]["n_clusters"])
    out = capsys.readouterr().out
    assert out.count("nearest (row, L2, failure code)") == labels.max() + 1
    with pytest.raises(NotImplementedError, match="canberra"):
        mod.main(["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--metrics", "canberra", "--out", str(tmp_path)])
