"""GPU checks of HDBSCAN's soft clustering (csrc/cluster.hip: wm_group_min_dist; cluster.py: group_min_distances,
all_points_membership_vectors, membership_vector; scripts/embedding_clustering_amd.py --soft) against float64 brute
force, against wm_knn_query's bits and against the host restatement of test_hdbscan_soft_cpu.

Bounds are derived as in test_gpu_cluster: one float32 distance is within eps(d) = (d + 3) * 2^-24 relative of the exact
distance of the float32 rows, and so is a minimum of such values.  The same pair gives the same bits in every mode of the
panel (one distance function, index order), so a group's nearest column must equal, bit for bit, what wm_knn_query with
k = 1 finds among that group's columns alone.  On the integer lattice every distance is exact in float32."""
import json

import numpy as np
import pytest
import torch
from parity_log import parity
from pathlib import Path

from test_gpu_cluster import dev, eps, lattice32, max_rel, rows
from test_gpu_hdbscan_predict import cross64, four_blobs, queries

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
METRICS = ["euclidean", "manhattan"]

# m around the 64-row tile of this mode, e around the 64-column tile, every d class (one chunk, a partial chunk, many
# chunks, the largest).  The grid has about 1024 / ceil(m / 64) column slices, at most 16 and at most one per column
# tile, so up to m = 4096 every slice of the small shapes is a single tile.  The last three reach the other paths:
#   (2100, 2600, 4)   33 row tiles, 41 column tiles: 14 slices of 3 tiles: the owner's running best carried over the
#                     tiles of a slice, groups that cross tile and slice boundaries, the merge over multi-tile slices;
#   (5000, 1100, 8)   79 row tiles, 18 column tiles: 9 slices of 2 tiles (the slice cap of 16 not reached);
#   (65500, 200, 8)   1024 row tiles: one slice of 4 tiles that stores straight into the outputs, no merge.
SHAPES = [(1, 1, 4), (63, 2, 52), (64, 64, 512), (65, 65, 1024), (300, 300, 52), (1, 300, 512), (300, 1, 4), (129, 130, 4),
          (2100, 2600, 4), (5000, 1100, 8), (65500, 200, 8)]


def cross(xq, x, metric):
    """cross64 looping over the shorter side (the same sums in the same float64 arithmetic)."""
    if xq.shape[0] <= x.shape[0]:
        return cross64(xq, x, metric)
    return np.ascontiguousarray(cross64(x, xq, metric).T)


def layouts(e, seed):
    """(name, group int64 [e], g): one group; every column its own; three runs with an empty group first, in the middle
    and last; a group on columns 60 to 70 across the column-tile boundary; blocks of 100 columns on the even ids (every
    other group empty, block edges off the 64-column tiles and off the slices); the runs in shuffled order."""
    out = [("one", np.zeros(e, dtype=np.int64), 1), ("each", np.arange(e, dtype=np.int64), e)]
    runs = np.array([1, 2, 4])[np.minimum(np.arange(e) * 3 // max(e, 1), 2)]  # ids 0, 3 and 5 stay empty
    out.append(("runs", runs, 6))
    if e > 70:
        span = np.zeros(e, dtype=np.int64)
        span[60:71], span[71:] = 1, 2
        out.append(("span", span, 3))
    if e > 100:
        out.append(("blocks", np.arange(e, dtype=np.int64) // 100 * 2, 2 * ((e - 1) // 100) + 3))
    out.append(("shuffled", np.random.default_rng(seed).permutation(runs), 6))
    return out


def run(xq, xe, group, g, metric):
    from ssl_wafermap_amd import cluster

    dist, j = cluster.group_min_distances(dev(xq), dev(xe), torch.from_numpy(group), g, metric)
    assert dist.dtype == torch.float32 and j.dtype == torch.int32 and dist.shape == j.shape == (xq.shape[0], g)
    assert dist.is_cuda and j.is_cuda
    return dist.cpu().numpy(), j.cpu().numpy()


@pytest.mark.parametrize("m,e,d", SHAPES)
def test_group_min_against_float64_and_knn_query(m, e, d):
    from ssl_wafermap_amd import manifold

    for metric in METRICS:
        xe = rows(e, d, 31 * e + d)
        xq, source = queries(xe, m, 17 * m + e + d)
        dq = cross(xq, xe, metric)
        for name, group, g in layouts(e, m + e + d):
            tag = f"{metric} m={m} e={e} d={d} {name}"
            got_d, got_j = run(xq, xe, group, g, metric)
            present = np.zeros(g, dtype=bool)
            present[group] = True
            assert np.isinf(got_d[:, ~present]).all() and (got_d[:, ~present] > 0).all() and (got_j[:, ~present] == -1).all()
            cols = np.flatnonzero(present)
            assert (got_j[:, cols] >= 0).all() and (group[got_j[:, cols]] == cols[None, :]).all()
            want = np.stack([dq[:, group == c].min(axis=1) for c in cols], axis=1)
            parity(f"group_min dist {tag} rel", max_rel(got_d[:, cols], want), eps(d))
            parity(f"group_min argmin {tag} rel", max_rel(np.take_along_axis(dq, got_j[:, cols].astype(np.int64), axis=1), want), eps(d))
            # the same bits as the k = 1 query among the group's columns alone.  Deliberately sampled: all groups up to
            # six, else six spread from the first to the last (a launch per group: every group of the 2600-group layout
            # would be 2600 launches for what the float64 comparison above already covers for every entry)
            for c in (cols if cols.size <= 6 else cols[np.linspace(0, cols.size - 1, 6).astype(int)]):
                members = np.flatnonzero(group == c)
                kd, ki = manifold.knn_query(dev(xq), dev(xe[members]), 1, metric)
                assert np.array_equal(got_d[:, c].view(np.int32), kd.cpu().numpy()[:, 0].view(np.int32)), tag
                assert np.array_equal(got_j[:, c], members[ki.cpu().numpy()[:, 0]]), tag
            # a query bit-equal to a column finds it at exactly 0, and among its duplicates in the group the lowest index
            twins = np.flatnonzero(source >= 0)
            for i in (twins if twins.size <= 100 else twins[np.linspace(0, twins.size - 1, 100).astype(int)]):
                c = group[source[i]]
                members = np.flatnonzero(group == c)
                same = members[(xe[members].view(np.int32) == xe[source[i]].view(np.int32)).all(axis=1)]
                assert got_d[i, c] == 0 and got_j[i, c] == same.min(), tag
            assert (got_d[twins, group[source[twins]]] == 0).all(), tag
            again = run(xq, xe, group, g, metric)  # no atomics: the same bits
            assert np.array_equal(got_d.view(np.int32), again[0].view(np.int32)) and np.array_equal(got_j, again[1])


@pytest.mark.parametrize("metric", METRICS)
def test_group_min_exact_on_a_lattice(metric):
    """Queries on and between the lattice points: every distance is exact in float32 and most minima are attained by
    several columns; the lowest index must win, in contiguous groups and in interleaved ones (the wrapper's sort)."""
    x, _ = lattice32(metric)
    e = x.shape[0]
    xq = np.concatenate([x, x + np.array([0.5, 0.5, 0, 0], dtype=np.float32)])
    m = xq.shape[0]
    assert m > 128 and e > 64  # several row tiles and several column slices
    diff = xq[:, None, :] - x[None, :, :]
    dq = np.sqrt((diff * diff).sum(-1, dtype=np.float32)) if metric == "euclidean" else np.abs(diff).sum(-1, dtype=np.float32)
    assert dq.dtype == np.float32
    ties = 0
    for group in (np.arange(e) * 4 // e, np.arange(e) % 4, np.zeros(e, dtype=np.int64)):
        g = int(group.max()) + 1
        got_d, got_j = run(xq, x, group.astype(np.int64), g, metric)
        for c in range(g):
            members = np.flatnonzero(group == c)
            sub = dq[:, members]
            assert np.array_equal(got_d[:, c], sub.min(axis=1))
            assert np.array_equal(got_j[:, c], members[sub.argmin(axis=1)]), "ties must resolve to the lowest index"
            ties += int(((sub == sub.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        assert (got_d[:e].min(axis=1) == 0).all()  # a row equal to a column is at exactly 0 from it
    assert ties > m  # (the case is what it claims)


def test_group_min_entry_point_on_the_device():
    from ssl_wafermap_amd import _lib, cluster

    lib = _lib.load()
    xe, xq = dev(rows(65, 8, 1)), dev(rows(9, 8, 2))
    group = torch.from_numpy((np.arange(65) // 30).astype(np.int32)).to(xe.device)
    out_d = torch.empty((9, 3), dtype=torch.float32, device=xe.device)
    out_j = torch.empty((9, 3), dtype=torch.int32, device=xe.device)
    need = lib.wm_group_min_dist_workspace_bytes(9, 65, 8, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=xe.device)

    def call(m=9, e=65, d=8, metric=0, g=3, ws_bytes=need):
        return lib.wm_group_min_dist(xq.data_ptr(), m, xe.data_ptr(), group.data_ptr(), e, d, metric, g, out_d.data_ptr(),
                                     out_j.data_ptr(), ws.data_ptr(), ws_bytes, 0)

    assert call() == 0
    assert call(m=0) == -1 and call(e=0) == -1 and call(g=0) == -1
    assert call(m=(1 << 24) + 1) == -2 and call(e=(1 << 24) + 1) == -2 and call(d=6) == -2 and call(metric=2) == -2
    assert call(ws_bytes=16) == -3
    torch.cuda.synchronize()
    want_d, want_j = cluster.group_min_distances(xq, xe, group, 3)
    assert torch.equal(out_d, want_d) and torch.equal(out_j, want_j)
    with pytest.raises(ValueError):
        cluster.group_min_distances(dev(rows(9, 12, 2)), xe, group, 3)  # feature counts differ
    with pytest.raises(ValueError):
        cluster.group_min_distances(xq, xe, group, 2)  # an id outside [0, n_groups)


# ------------------------------------------------------------------------------------------------ end to end


def exemplar_dist64(xq, x, exemplars, metric):
    return np.stack([cross64(xq, x[rows_c], metric).min(axis=1) for rows_c in exemplars], axis=1)


@pytest.mark.parametrize("metric", METRICS)
def test_membership_vectors_end_to_end(metric):
    """Fitted and new rows against membership_from_tree fed float64 brute-force exemplar distances, the two sides given
    the same tree and, for new rows, the same (neighbor, weight) from the kernels.

    Tolerance, derived: everything from the tree (merge heights, scores, the outlier vector, p) is float64 host code on
    identical inputs and so identical.  The kernel's distances enter through a_c = (1 / D_c) / sum_c' (1 / D_c') only.
    Each 1 / D is within eps(d) relative of the exact one; numerator and denominator (a sum of positive terms each
    within eps) each carry eps: a_c is within 2 eps.  The result a_c o_c / sum_c' (a_c' o_c') * p repeats the step with
    terms within 2 eps: 4 eps(d) relative per entry, d = 8 here; float64 rounding is 2^-29 of that.  An entry that is
    exactly 0 on one side (a one-hot distance vector, an infinite score elsewhere) must be exactly 0 on the other:
    a float32 distance is 0 exactly when the rows are bit-equal."""
    from ssl_wafermap_amd import cluster

    x, blob, xq, q_blob = four_blobs()
    n, d = x.shape
    bound = 4 * eps(d)
    model = cluster.HDBSCAN(min_cluster_size=15, min_samples=5, metric=metric, prediction_data=True).fit(dev(x))
    for mcs in (15, 40):
        model.refit(min_cluster_size=mcs)
        tree, selected, ex = model.condensed_tree_, model.selected_clusters_, model.exemplar_indices_
        n_sel = selected.size
        assert n_sel >= 4 and len(ex) == n_sel and all((model.labels_[r] == c).all() and r.size for c, r in enumerate(ex))
        _, cl_parent, birth, _, _, pt_parent, pt_lam = cluster._tree_tables(tree, n)
        # ---- the fitted rows
        got = cluster.all_points_membership_vectors(model)
        want, parts = cluster.membership_from_tree(tree, n, selected, pt_parent, pt_lam, exemplar_dist64(x, x, ex, metric), return_parts=True)
        assert got.dtype == np.float64 and got.shape == (n, n_sel) and np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
        parity(f"all_points_membership_vectors {metric} mcs={mcs} rel", max_rel(got, want), bound)
        assert np.abs(got.sum(axis=1) - parts["p"]).max() <= 1e-12
        own = model.labels_ >= 0
        assert np.array_equal(got[own].argmax(axis=1), model.labels_[own])
        for c, r in enumerate(ex):  # an exemplar is at distance exactly 0 from its cluster: one-hot in the distance factor
            others = np.delete(got[r], c, axis=1)
            assert (others == 0).all() and (got[r, c] > 0).all()
        # ---- new rows, and copies of exemplars as new rows
        new = np.concatenate([xq, x[np.concatenate(ex)]])
        got = cluster.membership_vector(model, dev(new))
        cq = cluster.query_core_distances(dev(new), dev(x), 5, metric)
        w, _, j = cluster.mreach_query(dev(new), cq, dev(x), cluster.core_distances(dev(x), 5, metric), metric, model.alpha)
        at, lam = cluster._walk(n, cl_parent, birth, pt_parent, pt_lam, j.cpu().numpy().astype(np.int64), w.cpu().numpy().astype(np.float64))
        want = cluster.membership_from_tree(tree, n, selected, at, lam, exemplar_dist64(new, x, ex, metric))
        assert got.shape == (new.shape[0], n_sel) and np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
        parity(f"membership_vector {metric} mcs={mcs} rel", max_rel(got, want), bound)
        labels, _ = cluster.approximate_predict(model, dev(xq))
        near = q_blob >= 0
        assert np.array_equal(got[:68][near].argmax(axis=1), labels[near])
        owner = np.repeat(np.arange(n_sel), [r.size for r in ex])
        copies = got[68:]
        assert (copies[np.arange(owner.size), owner] > 0).all()
        copies[np.arange(owner.size), owner] = 0
        assert (copies == 0).all()
    assert cluster.membership_vector(model, dev(np.zeros((0, d), dtype=np.float32))).shape == (0, n_sel)
    plain = cluster.HDBSCAN(min_cluster_size=15, min_samples=5, metric=metric).fit(dev(x))
    with pytest.raises(ValueError, match="prediction_data"):
        cluster.all_points_membership_vectors(plain)
    with pytest.raises(ValueError):
        cluster.membership_vector(model, dev(np.zeros((3, 12), dtype=np.float32)))


def test_single_root_cluster_has_one_column():
    from sklearn.datasets import make_blobs

    from ssl_wafermap_amd import cluster

    x = make_blobs(300, 8, centers=1, cluster_std=1.0, random_state=5)[0].astype(np.float32)
    model = cluster.HDBSCAN(min_cluster_size=20, min_samples=5, allow_single_cluster=True, prediction_data=True).fit(dev(x))
    assert model.selected_clusters_.tolist() == [300]
    got = cluster.all_points_membership_vectors(model)
    _, _, _, _, _, _, pt_lam = cluster._tree_tables(model.condensed_tree_, 300)
    top = float(model.condensed_tree_["lambda_val"].max())
    assert got.shape == (300, 1) and np.array_equal(got[:, 0], pt_lam / np.maximum(pt_lam, top))


# ------------------------------------------------------------------------------------------------ the script


def test_sweep_script_writes_soft_clustering(tmp_path):
    import importlib.util

    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", ROOT / "scripts" / "embedding_clustering_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "400", "--trials", "6", "--metrics", "euclidean",
              "--design", "grid"]  # (as test_sweep_script_predicts_held_out_rows: two clusters in these 300 rows)
    summary = mod.main(common + ["--holdout", "100", "--soft", "--out", str(tmp_path / "soft")])
    assert summary["chosen"] is not None
    on_disk = json.loads((tmp_path / "soft" / "summary.json").read_text())
    assert {"soft_noise_above_half", "soft_mean_row_sum", "holdout"} <= set(on_disk)
    labels = np.load(tmp_path / "soft" / "labels.npy")
    n_sel = int(labels.max()) + 1
    member = np.load(tmp_path / "soft" / "membership.npy")
    held = np.load(tmp_path / "soft" / "holdout_membership.npy")
    assert member.shape == (300, n_sel) and held.shape == (100, n_sel) and member.dtype == np.float64
    assert ((member >= 0) & (member <= 1)).all() and ((held >= 0) & (held <= 1)).all()
    ex = np.load(tmp_path / "soft" / "exemplars.npz")
    assert ex["rows"].shape == ex["cluster"].shape and ex["rows"].size >= n_sel and set(ex["cluster"].tolist()) == set(range(n_sel))
    assert np.array_equal(labels[ex["rows"]], ex["cluster"])
    assert abs(on_disk["soft_mean_row_sum"] - member.sum(axis=1).mean()) <= 1e-12
    noise = labels == -1
    want = float((member[noise].max(axis=1) > 0.5).mean()) if noise.any() else None
    assert on_disk["soft_noise_above_half"] == want
    # without a hold-out: the fitted rows only
    mod.main(common + ["--soft", "--out", str(tmp_path / "fit_only")])
    assert np.load(tmp_path / "fit_only" / "membership.npy").shape[0] == 400
    assert not (tmp_path / "fit_only" / "holdout_membership.npy").exists()
    # without the flag: none of the files, none of the keys
    mod.main(common + ["--holdout", "100", "--out", str(tmp_path / "plain")])
    plain = json.loads((tmp_path / "plain" / "summary.json").read_text())
    assert set(plain) == {"n", "d", "trials", "n_trees", "sweep_seconds", "pareto", "chosen", "holdout", "holdout_noise",
                          "holdout_homogeneity"}
    for name in ("membership.npy", "exemplars.npz", "holdout_membership.npy"):
        assert not (tmp_path / "plain" / name).exists()
