"""GPU checks of the rank primitive and the embedding-quality scores built on it (csrc/cluster.hip: wm_pair_dist,
wm_rank_query; manifold.py: pair_distances, neighbor_ranks, trustworthiness, continuity, embedding_quality;
scripts/embedding_umap_amd.py --quality) against integer counting on the CPU and the float64 restatement of
test_embedding_quality_cpu.

Counts are integers, so wherever the float32 distances are exact (integer coordinates: every squared distance and every
L1 distance is a small integer, and the correctly rounded root keeps distinct integers apart) a rank must EQUAL the
count under (distance, index).  On float data a rank may differ from the float64 one by the orderings float32 may
legitimately flip: the columns l != j within 2 eps(d) d64(i, j) of the threshold (one eps for either distance,
test_gpu_cluster states eps(d)); the bound is computed from the reference alone."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from parity_log import parity

from test_embedding_quality_cpu import SHAPES, quality64, two_spaces
from test_gpu_cluster import dev, eps, lattice32, rows
from test_gpu_umap import wafer_rows  # noqa: F401  (a fixture)
from test_umap_transform_cpu import pairwise64_rect

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
METRICS = ["euclidean", "manhattan"]


def bits(t):
    return t.cpu().numpy().view(np.int32)


def ranks_ref(dist, idx, skip):
    """int64 [m, k]: 1 + #{ l != skip_i : (dist[i, l], l) < (dist[i, j], j) }, j = idx[i, q]; an entry of -1 ranks behind
    every counted column.  dist [m, n] of any dtype (a stable argsort is the (distance, index) order), skip int [m]
    (-1: none)."""
    m, n = dist.shape
    order = np.argsort(dist, axis=1, kind="stable")
    pos = np.empty((m, n), dtype=np.int64)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(n, dtype=np.int64), (m, n)), axis=1)
    idx = np.asarray(idx, dtype=np.int64)
    skip = np.asarray(skip, dtype=np.int64)
    before = np.take_along_axis(pos, np.maximum(idx, 0), axis=1)
    before = np.where(idx < 0, n, before)
    skip_pos = np.where(skip >= 0, pos[np.arange(m), np.maximum(skip, 0)], n + 1)[:, None]  # (n + 1: never before)
    return before - (skip_pos < before) + 1


def int_rows(m, d, seed, high=4):
    """Rows of small integers as float32: every distance between two of them is exact in float32, and many are equal."""
    return np.random.default_rng(seed).integers(0, high, size=(m, d)).astype(np.float32)


def int_dist(xq, x, metric):
    """Exact integer keys of the distances (squared for Euclidean: the same order), one feature at a time."""
    out = np.zeros((xq.shape[0], x.shape[0]), dtype=np.int64)
    for f in range(x.shape[1]):
        t = xq[:, f, None].astype(np.int64) - x[None, :, f].astype(np.int64)
        out += t * t if metric == "euclidean" else np.abs(t)
    return out


def random_lists(m, n, k, seed, holes=True):
    idx = np.random.default_rng(seed).integers(0, n, size=(m, k)).astype(np.int32)
    if holes and k > 1:
        idx[::7, k // 2] = -1
    return idx


# ------------------------------------------------------------------------------------------------ 1. threshold bits


@pytest.mark.parametrize("d", [4, 52, 512, 1024])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_pair_distances_give_the_tile_pass_bits(n, d):
    from ssl_wafermap_amd import manifold

    xd = dev(rows(n, d, 7 * n + d))
    for metric in METRICS:
        for k in sorted({1, min(n, 15), min(n, 64)}):
            dist, idx = manifold.knn_graph(xd, k, metric)
            got = manifold.pair_distances(xd, xd, idx, metric)
            assert got.dtype == torch.float32 and got.shape == (n, k)
            assert np.array_equal(bits(got), bits(dist)), f"{metric} n={n} d={d} k={k}"
    holes = torch.full((n, 3), -1, dtype=torch.int32, device=xd.device)
    holes[:, 1] = n  # outside [0, n): +inf as well, nothing is read
    assert bool(torch.isinf(manifold.pair_distances(xd, xd, holes)).all())


# ------------------------------------------------------------------------------------------------ 2. exact ranks


@pytest.mark.parametrize("metric", METRICS)
def test_ranks_on_the_lattice_equal_the_integer_count(metric):
    from ssl_wafermap_amd import manifold

    x, dist = lattice32(metric)
    n = x.shape[0]
    xd = dev(x)
    none, own = np.full(n, -1), np.arange(n)
    for k, seed in ((1, 0), (9, 1), (64, 2)):
        idx = random_lists(n, n, k, seed)
        for exclude, skip in ((False, none), (True, own)):
            got = manifold.neighbor_ranks(xd, xd, dev(idx), metric, exclude_self=exclude)
            assert got.dtype == torch.int32 and got.shape == (n, k)
            assert np.array_equal(got.cpu().numpy(), ranks_ref(dist, idx, skip)), f"{metric} k={k} exclude_self={exclude}"
    # the kNN lists: the q-th entry has rank q + 1 (the row itself among the candidates)
    knn = manifold.knn_graph(xd, 16, metric)[1]
    got = manifold.neighbor_ranks(xd, xd, knn, metric).cpu().numpy()
    assert np.array_equal(got, np.broadcast_to(np.arange(1, 17), (n, 16)))
    assert np.array_equal(got, ranks_ref(dist, knn.cpu().numpy(), none))
    # rectangular: shifted lattice rows as queries (still integers), no column skipped
    xq = (x[::3] + np.array([1, 0, 2, 0], dtype=np.float32)).astype(np.float32)
    diff = xq[:, None, :] - x[None, :, :]
    rect = np.sqrt((diff * diff).sum(-1, dtype=np.float32)) if metric == "euclidean" else np.abs(diff).sum(-1, dtype=np.float32)
    idx = random_lists(xq.shape[0], n, 9, 3)
    got = manifold.neighbor_ranks(dev(xq), xd, dev(idx), metric).cpu().numpy()
    assert np.array_equal(got, ranks_ref(rect, idx, np.full(xq.shape[0], -1)))


# ------------------------------------------------------------------------------------------------ 3. the complete order


@pytest.mark.parametrize("d", [4, 52])
@pytest.mark.parametrize("n", [2, 17, 64])
def test_ranks_against_the_complete_order(n, d):
    """For n <= 64, knn_graph(x, n) is the whole (distance, index) order of every row: the rank of every j is its position
    in that list, and its position once the row itself is dropped when the row is excluded.  No float64 involved."""
    from ssl_wafermap_amd import manifold

    xd = dev(rows(n, d, 31 * n + d))
    for metric in METRICS:
        full = manifold.knn_graph(xd, n, metric)[1]
        got = manifold.neighbor_ranks(xd, xd, full, metric).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(np.arange(1, n + 1), (n, n))), metric
        lists = full.cpu().numpy()
        others = np.stack([lists[i][lists[i] != i] for i in range(n)]).astype(np.int32)  # every row holds itself once
        assert others.shape == (n, n - 1)
        got = manifold.neighbor_ranks(xd, xd, dev(others), metric, exclude_self=True).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(np.arange(1, n), (n, n - 1))), metric
        assert np.array_equal(manifold.neighbor_lists(xd, n - 1, metric).cpu().numpy(), others)


# ------------------------------------------------------------------------------------------------ 4. float data


def flips_allowed(d64, idx, e):
    """int64 [m, k]: per entry (i, q), j = idx[i, q], the number of columns l != j with
    |d64(i, l) - d64(i, j)| <= 2 e d64(i, j): the orderings float32 distances of relative error e may flip."""
    m, n = d64.shape
    idx = np.asarray(idx, dtype=np.int64)
    t = np.take_along_axis(d64, idx, axis=1)  # [m, k]
    out = np.empty(idx.shape, dtype=np.int64)
    for q in range(idx.shape[1]):
        out[:, q] = (np.abs(d64 - t[:, q, None]) <= 2.0 * e * t[:, q, None]).sum(axis=1) - 1  # (l = j itself is always within)
    return out


@pytest.mark.parametrize("d", [4, 52, 512])
def test_ranks_on_float_data_against_float64(d):
    from ssl_wafermap_amd import manifold

    n, m, k = 257, 130, 15
    x = rows(n, d, 900 + d)
    xq = np.concatenate([x[:40], rows(m - 40, d, 901 + d)])  # fitted rows (exact zeros, duplicates) and new ones
    idx = random_lists(m, n, k, 5, holes=False)
    for metric in METRICS:
        d64 = pairwise64_rect(xq, x, metric)
        want = ranks_ref(d64, idx, np.full(m, -1))
        allowed = flips_allowed(d64, idx, eps(d))
        got = manifold.neighbor_ranks(dev(xq), dev(x), dev(idx), metric).cpu().numpy().astype(np.int64)
        diff = np.abs(got - want)
        print(f"ranks float {metric} d={d}: largest |rank - rank64| {diff.max()}, largest allowance {allowed.max()}, "
              f"entries that differ {int((diff > 0).sum())}")
        parity(f"neighbor_ranks {metric} m={m} n={n} d={d} k={k} largest |rank - rank64| - allowed flips", float((diff - allowed).max()), 0.0)
        assert (diff <= allowed).all()
    # square with the row excluded
    d64 = pairwise64_rect(x, x, "euclidean")
    own = np.arange(n)
    idx = random_lists(n, n, k, 6, holes=False)
    got = manifold.neighbor_ranks(dev(x), dev(x), dev(idx), exclude_self=True).cpu().numpy().astype(np.int64)
    diff = np.abs(got - ranks_ref(d64, idx, own))
    parity(f"neighbor_ranks euclidean square n={n} d={d} k={k} largest |rank - rank64| - allowed flips",
           float((diff - flips_allowed(d64, idx, eps(d))).max()), 0.0)


# ------------------------------------------------------------------------------------------------ 5. shapes

# The rank mode's grid is cl_grid(m, n, 64, sliced): row tiles of 64 rows, column tiles of 64 columns and about
# 1024 / row_tiles column slices, at most one per column tile; tiles_per_slice = ceil(col_tiles / slices wanted).
#   (2100, 2600)   33 row tiles, 41 column tiles; ceil(1024 / 33) = 32 slices wanted: ceil(41 / 32) = 2 tiles per
#                  slice, 21 slices (the last holds one tile): bins carried over the tiles of a slice, the merge;
#   (65473, 200)   1024 row tiles (1023 * 64 = 65472): one slice wanted, which holds all 4 column tiles and stores
#                  straight into the output, no merge.
BIG_SHAPES = [(2100, 2600, 4, 15), (65473, 200, 8, 15)]


def check_int_shape(m, n, d, k, metric, square, seed):
    from ssl_wafermap_amd import manifold

    x = int_rows(n, d, seed)
    xq = x if square else int_rows(m, d, seed + 1)
    idx = random_lists(xq.shape[0], n, k, seed + 2)
    skip = np.arange(n) if square else np.full(m, -1)
    got = manifold.neighbor_ranks(dev(xq), dev(x), dev(idx), metric, exclude_self=square).cpu().numpy()
    want = ranks_ref(int_dist(xq, x, metric), idx, skip)
    assert np.array_equal(got, want), f"m={xq.shape[0]} n={n} d={d} k={k} {metric} square={square}"


@pytest.mark.parametrize("k", [1, 15, 63])
@pytest.mark.parametrize("d", [4, 36, 52, 1024])  # one partial chunk, a second partial chunk, 32 chunks
def test_rank_shapes_around_the_tiles(d, k):
    """Rows around the 64-row tile, columns around the 64-column tile (one slice per column tile at these sizes: the
    merge adds up to three planes), integer data: equality."""
    for m, n in ((1, 63), (63, 64), (64, 65), (65, 130), (129, 1)):
        check_int_shape(m, n, d, k, METRICS[(m + k) % 2], False, 10 * m + n)
    for n in (63, 65, 129):
        check_int_shape(n, n, d, k, METRICS[(n + k) % 2], True, 3 * n)


@pytest.mark.parametrize("m,n,d,k", BIG_SHAPES)
def test_rank_shapes_slices_and_single_slice(m, n, d, k):
    check_int_shape(m, n, d, k, "euclidean", False, m)


def test_rank_square_multi_tile_slices():
    """(2100, 2100) square with the row excluded: 33 row tiles, 33 column tiles, 32 slices wanted: 2 tiles per slice."""
    check_int_shape(2100, 2100, 8, 63, "manhattan", True, 77)


# ------------------------------------------------------------------------------------------------ 6. identities


def test_identities_and_repeatability():
    from ssl_wafermap_amd import manifold

    x = dev(rows(300, 8, 3))
    y = dev(rows(300, 2, 4))
    for k in (1, 15, 63):
        for metric in METRICS:
            t, t_rows = manifold.trustworthiness(x, x, k, metric, metric, return_rows=True)
            c, c_rows = manifold.continuity(x, x, k, metric, metric, return_rows=True)
            assert t == 1.0 and c == 1.0 and (t_rows == 1.0).all() and (c_rows == 1.0).all()
        c, c_rows = manifold.continuity(x, y, k, return_rows=True)
        t, t_rows = manifold.trustworthiness(y, x, k, return_rows=True)
        assert c == t and np.array_equal(c_rows, t_rows) and 0.0 < c < 1.0
        q = manifold.embedding_quality(x, y, k)
        assert q.continuity == c and q.trustworthiness == manifold.trustworthiness(x, y, k)
        again = manifold.embedding_quality(x, y, k)
        for a, b in zip(q, again):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "two runs must give the same bits"
    idx = dev(random_lists(300, 300, 15, 8))
    assert np.array_equal(manifold.neighbor_ranks(x, x, idx).cpu().numpy(), manifold.neighbor_ranks(x, x, idx).cpu().numpy())
    with pytest.raises(ValueError):
        manifold.trustworthiness(x, y, 150)
    with pytest.raises(ValueError):
        manifold.embedding_quality(x, y, [5, 64])


# ------------------------------------------------------------------------------------------------ 7. end to end


def check_end_to_end(name, a, b, ks):
    """embedding_quality against quality64 on the device's own neighbour lists; tolerance unit * near + 1e-12, near the
    total of the flips float32 may make in the ranks that enter the score (test 4's allowance)."""
    from ssl_wafermap_amd import manifold

    a, b = a.astype(np.float32), b.astype(np.float32)
    n, kmax = a.shape[0], max(ks)
    ad, bd = dev(a), dev(b)
    near_a = manifold.neighbor_lists(ad, kmax).cpu().numpy()
    near_b = manifold.neighbor_lists(bd, kmax).cpu().numpy()
    da, db = pairwise64_rect(a, a), pairwise64_rect(b, b)
    flips_t = flips_allowed(da, near_b, eps(a.shape[1]))  # ranks in a of b's neighbours
    flips_c = flips_allowed(db, near_a, eps(b.shape[1]))  # (the zero padding to 4 features adds no rounding)
    many = manifold.embedding_quality(ad, bd, list(ks))
    assert [q.n_neighbors for q in many] == list(ks)
    for q in many:
        k = q.n_neighbors
        ref = quality64(da, db, k, near_a=near_a, near_b=near_b)
        unit = 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
        for what, got, rows_, flips in (("trustworthiness", q.trustworthiness, q.trustworthiness_rows, flips_t[:, :k]),
                                        ("continuity", q.continuity, q.continuity_rows, flips_c[:, :k])):
            err = abs(got - ref[what])
            print(f"{name} k={k} {what}: {got:.6f}, |error| {err:.3g}, flips allowed {int(flips.sum())}")
            parity(f"embedding_quality {name} k={k} {what} abs", err, unit * float(flips.sum()) + 1e-12)
            assert (np.abs(rows_ - ref[what + "_rows"]) <= n * unit * flips.sum(axis=1) + 1e-12).all()
            assert abs(rows_.mean() - got) <= 1e-12
        assert q.neighbor_preservation == ref["preservation"] and np.array_equal(q.preservation_rows, ref["preservation_rows"])
        one = manifold.embedding_quality(ad, bd, k)  # a pass at this k alone: the same lists' first k entries
        assert one.trustworthiness == q.trustworthiness and one.continuity == q.continuity
        assert np.array_equal(one.preservation_rows, q.preservation_rows)
    return many


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_embedding_quality_end_to_end(n, d, k):
    a, b = two_spaces(n, d)
    check_end_to_end(f"n={n} d={d}", a, b, sorted({1, k // 2 + 1, k}))


def test_embedding_quality_of_a_umap_of_golden_rows(wafer_rows):
    from ssl_wafermap_amd import manifold

    x = wafer_rows[0]
    y = manifold.UMAP(n_neighbors=15, n_components=2, init="random", n_epochs=100, random_state=0).fit_transform(dev(x))
    q = check_end_to_end("umap of 1500 golden rows", x, y.cpu().numpy(), [15])[0]
    assert q.trustworthiness > 0.9 and q.continuity > 0.9  # (a fitted UMAP, not noise: sklearn gives 0.989 at 200 epochs)


# ------------------------------------------------------------------------------------------------ 8. the script


def test_script_quality_flag(tmp_path):
    spec = importlib.util.spec_from_file_location("embedding_umap_amd", ROOT / "scripts" / "embedding_umap_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = ["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "600", "--epochs", "100"]
    plain = mod.main(args + ["--out", str(tmp_path / "plain")])
    new = {"trustworthiness_full", "continuity_full", "neighbor_preservation", "quality_seconds"}
    assert not new & set(plain) and not (tmp_path / "plain" / "quality.npz").exists()
    summary = mod.main(args + ["--quality", "--out", str(tmp_path / "q")])
    on_disk = json.loads((tmp_path / "q" / "summary.json").read_text())
    assert set(on_disk) == set(plain) | new and set(summary) == set(on_disk)
    for key in ("trustworthiness_full", "continuity_full", "neighbor_preservation"):
        assert 0.0 <= on_disk[key] <= 1.0 and on_disk[key] == summary[key]
    assert on_disk["trustworthiness_full"] > 0.9 and on_disk["quality_seconds"] > 0
    z = np.load(tmp_path / "q" / "quality.npz")
    for key in ("trustworthiness_rows", "continuity_rows", "preservation_rows"):
        assert z[key].shape == (600,) and z[key].dtype == np.float64
    assert abs(z["trustworthiness_rows"].mean() - on_disk["trustworthiness_full"]) <= 1e-12
