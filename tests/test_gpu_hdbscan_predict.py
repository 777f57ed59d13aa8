"""GPU checks of HDBSCAN's prediction for new rows (csrc/cluster.hip: wm_mreach_query; cluster.py: mreach_query,
query_core_distances, approximate_predict, approximate_predict_scores; scripts/embedding_clustering_amd.py --holdout)
against float64 brute force and the host restatement of test_hdbscan_predict_cpu.

Bounds are derived as in test_gpu_cluster: one float32 distance is within eps(d) = (d + 3) * 2^-24 relative of the
exact distance of the float32 rows.  The float32 core distances are given to both sides and a power-of-two alpha
scales exactly, so w = max(core_q, core, dist / alpha) carries the distance's error only, and a minimum of values
within eps is within eps.  On the integer lattice every distance is exact in float32 and (w, dist, j) must be equal.
Given the kernel's (j, w) the walk through the condensed tree is float64 host code: equal, not close."""
import json

import numpy as np
import pytest
import torch
from parity_log import parity
from pathlib import Path

from test_gpu_cluster import dev, eps, lattice32, max_rel, rows
from test_hdbscan_predict_cpu import check_self_prediction

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
METRICS = ["euclidean", "manhattan"]

# m around the 128-row tile, n around the 64-column tile (from 65 on several column slices: the merge kernel), every d
# class (one chunk, a partial chunk, many chunks, the largest); each value of each axis at least once
SHAPES = [(1, 1, 4), (127, 2, 52), (128, 64, 512), (129, 65, 1024), (300, 300, 52), (1, 300, 512), (300, 1, 4), (129, 64, 4),
          (128, 65, 52), (127, 300, 1024), (300, 2, 512), (1, 65, 1024)]


def cross64(xq, x, metric):
    xq, x = xq.astype(np.float64), x.astype(np.float64)
    if metric == "euclidean":
        return np.stack([np.sqrt(((x - row) ** 2).sum(axis=1)) for row in xq])
    return np.stack([np.abs(x - row).sum(axis=1) for row in xq])


def queries(x, m, seed):
    """m float32 query rows; every third one is bit-equal to a fitted row (rows 0 and 3 of x, duplicates of each
    other where they exist, among them).  Returns (xq, source) with source[i] = the copied row or -1."""
    n, d = x.shape
    xq = np.random.default_rng(seed).standard_normal((m, d)).astype(np.float32)
    source = np.full(m, -1)
    for i in range(0, m, 3):
        source[i] = (i // 3) % n if i else min(3, n - 1)
        xq[i] = x[source[i]]
    return xq, source


def run(xq, cq, x, core, metric, alpha=1.0):
    from ssl_wafermap_amd import cluster

    w, dist, j = cluster.mreach_query(dev(xq), dev(cq), dev(x), dev(core), metric, alpha)
    assert w.dtype == torch.float32 and dist.dtype == torch.float32 and j.dtype == torch.int32
    return w.cpu().numpy(), dist.cpu().numpy(), j.cpu().numpy()


@pytest.mark.parametrize("m,n,d", SHAPES)
def test_mreach_query_against_float64(m, n, d):
    for metric in METRICS:
        x = rows(n, d, 31 * n + d)
        xq, source = queries(x, m, 17 * m + n + d)
        dq = cross64(xq, x, metric)
        k = min(5, n)
        core = np.sort(cross64(x, x, metric), axis=1)[:, k - 1].astype(np.float32)
        cq = np.sort(np.concatenate([np.zeros((m, 1)), dq], axis=1), axis=1)[:, k - 1].astype(np.float32)
        for alpha in ((1.0, 2.0) if (m, n, d) == (300, 300, 52) else (1.0,)):
            w_all = np.maximum(np.maximum(cq[:, None].astype(np.float64), core[None, :].astype(np.float64)), dq / alpha)
            w_min = w_all.min(axis=1)
            got_w, got_d, got_j = run(xq, cq, x, core, metric, alpha)
            assert (got_j >= 0).all() and (got_j < n).all()
            tag = f"{metric} m={m} n={n} d={d} alpha={alpha:g}"
            parity(f"mreach_query weight {tag} rel", max_rel(got_w, w_min), eps(d))
            parity(f"mreach_query argmin {tag} rel", max_rel(w_all[np.arange(m), got_j], w_min), eps(d))
            parity(f"mreach_query dist {tag} rel", max_rel(got_d, dq[np.arange(m), got_j]), eps(d))
            assert np.array_equal(got_w, np.maximum(np.maximum(cq, core[got_j]), got_d * np.float32(1.0 / alpha)))
            again = run(xq, cq, x, core, metric, alpha)  # no atomics: the same bits
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((got_w, got_d, got_j), again))
        # zero cores: w is the plain distance; a query bit-equal to a fitted row finds it at exactly 0, and among its
        # duplicates the lowest index
        got_w, got_d, got_j = run(xq, np.zeros(m, dtype=np.float32), x, np.zeros(n, dtype=np.float32), metric)
        parity(f"mreach_query nearest {metric} m={m} n={n} d={d} rel", max_rel(got_w, dq.min(axis=1)), eps(d))
        assert np.array_equal(got_w, got_d)
        twins = np.flatnonzero(source >= 0)
        lowest = np.array([min(t for t in range(n) if np.array_equal(x[t].view(np.int32), x[s].view(np.int32))) for s in source[twins]])
        assert (got_d[twins] == 0).all() and (got_w[twins] == 0).all() and np.array_equal(got_j[twins], lowest)
        if n >= 8:
            assert (lowest[source[twins] == 3] == 0).all()  # (the case is what it claims: row 3 duplicates row 0)


def test_mreach_query_argument_errors():
    from ssl_wafermap_amd import _lib, cluster

    lib = _lib.load()
    x, xq = dev(rows(65, 8, 1)), dev(rows(9, 8, 2))
    core, cq = torch.zeros(65, device=x.device), torch.zeros(9, device=x.device)
    out = [torch.empty(9, dtype=t, device=x.device) for t in (torch.float32, torch.float32, torch.int32)]
    ws = torch.empty(lib.wm_mreach_query_workspace_bytes(9, 65, 8), dtype=torch.uint8, device=x.device)

    def call(m=9, n=65, d=8, metric=0, inv_alpha=1.0, ws_bytes=ws.numel()):
        return lib.wm_mreach_query(xq.data_ptr(), cq.data_ptr(), m, x.data_ptr(), core.data_ptr(), n, d, metric, inv_alpha,
                                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws_bytes, 0)

    assert call() == 0
    assert call(m=0) == -1 and call(n=0) == -1 and call(inv_alpha=0.0) == -1
    assert call(m=(1 << 24) + 1) == -2 and call(n=(1 << 24) + 1) == -2 and call(d=6) == -2 and call(metric=2) == -2
    assert call(ws_bytes=16) == -3
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        cluster.mreach_query(dev(rows(9, 12, 2)), cq, x, core)  # feature counts differ
    with pytest.raises(ValueError):
        cluster.mreach_query(xq, cq.double(), x, core)


@pytest.mark.parametrize("metric", METRICS)
def test_mreach_query_exact_on_a_lattice(metric):
    """Queries on and between the lattice points, with core distances that tie many candidates on w: the plain
    distance decides among them, then the index (a query at the centre of a lattice cell has four nearest rows)."""
    from ssl_wafermap_amd import cluster

    x, dist = lattice32(metric)
    n = x.shape[0]
    core = np.sort(dist, axis=1)[:, 3]
    assert np.array_equal(cluster.core_distances(dev(x), 4, metric).cpu().numpy(), core)
    xq = np.concatenate([x, x + np.array([0.5, 0.5, 0, 0], dtype=np.float32), x[:40] + np.array([0, 1.5, 0, 0], dtype=np.float32)])
    m = xq.shape[0]
    assert m > 256 and n > 64  # several row tiles and several column slices
    diff = xq[:, None, :] - x[None, :, :]
    dq = np.sqrt((diff * diff).sum(-1, dtype=np.float32)) if metric == "euclidean" else np.abs(diff).sum(-1, dtype=np.float32)
    assert dq.dtype == np.float32
    cols = np.arange(n)
    for cq in (np.zeros(m, dtype=np.float32), np.full(m, 3.0, dtype=np.float32), (np.arange(m) % 5).astype(np.float32)):
        for alpha in (1.0, 2.0):  # (a power of two scales exactly)
            w = np.maximum(np.maximum(cq[:, None], core[None, :]), dq * np.float32(1.0 / alpha))
            assert w.dtype == np.float32
            want_j = np.array([np.lexsort((cols, dq[i], w[i]))[0] for i in range(m)])
            tied_w = (w == w[np.arange(m), want_j][:, None]).sum(axis=1)
            tied_d = ((w == w[np.arange(m), want_j][:, None]) & (dq == dq[np.arange(m), want_j][:, None])).sum(axis=1)
            if cq[0] == 3.0:
                assert (tied_w > 8).mean() > 0.9 and (tied_d > 1).any() and (tied_d < tied_w).any()  # ties on w, then on dist
            got_w, got_d, got_j = run(xq, cq, x, core, metric, alpha)
            assert np.array_equal(got_j, want_j), "(w, dist, j) must resolve lexicographically"
            assert np.array_equal(got_w, w[np.arange(m), want_j]) and np.array_equal(got_d, dq[np.arange(m), want_j])


# ------------------------------------------------------------------------------------------------ end to end


def four_blobs():
    """(fitted rows [300, 8], their blob, query rows [68, 8], the queries' blob or -1): four unit Gaussians 75 rows
    each on four axes, 64 new draws from them and 4 rows at 50 standard deviations on the far side of the origin."""
    rng = np.random.default_rng(11)
    centers = 12.0 * np.eye(8)[:4]
    blob = np.repeat(np.arange(4), 75)
    x = (centers[blob] + rng.standard_normal((300, 8))).astype(np.float32)
    q_blob = np.concatenate([np.repeat(np.arange(4), 16), np.full(4, -1)])
    xq = np.concatenate([centers[q_blob[:64]] + rng.standard_normal((64, 8)), -50.0 * np.eye(8)[4:]]).astype(np.float32)
    assert np.unique(x, axis=0).shape[0] == 300
    return x, blob, xq, q_blob


def check_prediction(model, x, blob, xq, q_blob):
    from ssl_wafermap_amd import cluster

    n = x.shape[0]
    majority = np.array([np.bincount(model.labels_[blob == b] + 1).argmax() - 1 for b in range(4)])
    assert (majority >= 0).all() and np.unique(majority).size == 4
    labels, prob = cluster.approximate_predict(model, dev(xq))
    score = cluster.approximate_predict_scores(model, dev(xq))
    assert labels.dtype == np.int64 and labels.shape == prob.shape == score.shape == (68,)
    near, far = q_blob >= 0, q_blob < 0
    assert np.array_equal(labels[near], majority[q_blob[near]]) and (prob[near] > 0).all()
    assert (labels[far] == -1).all() and (prob[far] == 0).all()
    # the host walk is deterministic given the kernel's (j, w)
    k = model.min_samples
    cq = cluster.query_core_distances(dev(xq), dev(x), k, model.metric)
    w, _, j = cluster.mreach_query(dev(xq), cq, dev(x), cluster.core_distances(dev(x), k, model.metric), model.metric, model.alpha)
    w64, j64 = w.cpu().numpy().astype(np.float64), j.cpu().numpy().astype(np.int64)
    want = cluster.assign_from_tree(model.condensed_tree_, n, model.selected_clusters_, j64, w64, model.cluster_selection_epsilon)
    assert np.array_equal(labels, want[0]) and np.array_equal(prob, want[1]) and np.array_equal(score, want[2])
    # a far row falls out of the root: 1 - lam / D with D the largest lambda of the whole tree
    lam, top = 1.0 / w64[far], float(model.condensed_tree_["lambda_val"].max())
    assert np.isfinite(top) and np.array_equal(score[far], (top - lam) / top)
    assert (np.abs(score[far] - (1.0 - lam / top)) <= 2.0 ** -52).all() and (score[far] > score[near].max()).all()
    # the fitted rows as queries
    own = cluster.approximate_predict(model, dev(x)) + (cluster.approximate_predict_scores(model, dev(x)),)
    check_self_prediction(model.labels_, model.probabilities_, model.outlier_scores_, own)


def test_predict_new_rows_end_to_end():
    from ssl_wafermap_amd import cluster

    x, blob, xq, q_blob = four_blobs()
    model = cluster.HDBSCAN(min_cluster_size=15, min_samples=5, prediction_data=True).fit(dev(x))
    assert model._train.is_cuda and model._core.is_cuda and model._core.shape == (300,)
    assert np.array_equal(model.outlier_scores_, cluster.glosh(model.condensed_tree_, 300))
    check_prediction(model, x, blob, xq, q_blob)
    model.refit(min_cluster_size=40)
    check_prediction(model, x, blob, xq, q_blob)
    plain = cluster.HDBSCAN(min_cluster_size=15, min_samples=5).fit(dev(x))
    assert plain._train is None and plain._core is None and np.array_equal(plain.labels_, model.refit(min_cluster_size=15).labels_)
    assert np.array_equal(plain.outlier_scores_, model.outlier_scores_)
    with pytest.raises(ValueError, match="prediction_data"):
        cluster.approximate_predict(plain, dev(xq))
    with pytest.raises(ValueError):
        cluster.approximate_predict(model, dev(np.zeros((3, 12), dtype=np.float32)))


def test_min_samples_one_launches_no_knn_pass(monkeypatch):
    from ssl_wafermap_amd import _lib, cluster

    x, blob, xq, q_blob = four_blobs()
    one = cluster.HDBSCAN(min_cluster_size=15, min_samples=1, prediction_data=True).fit(dev(x))
    five = cluster.HDBSCAN(min_cluster_size=15, min_samples=5, prediction_data=True).fit(dev(x))
    calls = []
    real = _lib.load().wm_knn_query

    def counted(*args):
        calls.append(args)
        return real(*args)

    monkeypatch.setattr(_lib.load(), "wm_knn_query", counted)
    labels, prob = cluster.approximate_predict(one, dev(xq))
    assert not calls
    assert (labels[q_blob < 0] == -1).all() and (labels[q_blob >= 0] >= 0).all() and (prob[q_blob >= 0] > 0).all()
    cluster.approximate_predict(five, dev(xq))
    assert len(calls) == 1 and calls[0][6] == 4  # (the stand-in is in the path: min_samples - 1 neighbours)


# ------------------------------------------------------------------------------------------------ the script


def test_sweep_script_predicts_held_out_rows(tmp_path):
    import importlib.util

    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", ROOT / "scripts" / "embedding_clustering_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "400", "--trials", "6", "--metrics", "euclidean",
              "--design", "grid"]  # (the grid's min_samples = 1, min_cluster_size = 10 trials find two clusters in these 300 rows)
    summary = mod.main(common + ["--holdout", "100", "--out", str(tmp_path / "held")])
    assert summary["n"] == 300 and summary["chosen"] is not None
    on_disk = json.loads((tmp_path / "held" / "summary.json").read_text())
    assert {"holdout", "holdout_noise", "holdout_homogeneity"} <= set(on_disk) and on_disk["holdout"] == 100
    labels = np.load(tmp_path / "held" / "holdout_labels.npy")
    prob = np.load(tmp_path / "held" / "holdout_probabilities.npy")
    score = np.load(tmp_path / "held" / "holdout_outlier_scores.npy")
    assert labels.shape == prob.shape == score.shape == (100,)
    fitted = np.load(tmp_path / "held" / "labels.npy")
    assert fitted.shape == (300,) and labels.min() >= -1 and labels.max() <= fitted.max()
    assert ((prob >= 0) & (prob <= 1)).all() and ((score >= 0) & (score <= 1)).all() and (prob[labels == -1] == 0).all()
    assert on_disk["holdout_noise"] == int((labels == -1).sum())
    if (labels >= 0).any():
        assert 0.0 <= on_disk["holdout_homogeneity"] <= 1.0
    else:
        assert on_disk["holdout_homogeneity"] is None
    mod.main(common + ["--out", str(tmp_path / "plain")])
    plain = json.loads((tmp_path / "plain" / "summary.json").read_text())
    assert set(plain) == {"n", "d", "trials", "n_trees", "sweep_seconds", "pareto", "chosen"} and plain["n"] == 400
    assert not list((tmp_path / "plain").glob("holdout_*"))
