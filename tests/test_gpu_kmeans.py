"""GPU checks of KMeans (csrc/kmeans.hip: wm_kmeans_update, wm_kmeans_seed; cluster.py: kmeans_step, kmeans_plusplus,
KMeans; scripts/embedding_kmeans_amd.py) against float64 restatements written here, against wm_knn_query's bits and
against sklearn.cluster.KMeans where the float64 trajectory has margin.

Bounds are derived as in test_gpu_cluster: a float32 distance is within eps(d) = (d + 3) * 2^-24 relative of the exact
distance of the float32 rows, so its square is within 2 * eps(d); a double sum of n such terms adds at most n * 2^-52.  A
centre is a float64 sum divided in double and rounded to float32 once: within one float32 ulp of the exactly summed mean.
On the integer lattice every float32 distance is the correctly rounded root of an exact sum, which numpy restates bit for
bit; the sums of their squares are restated in the kernels' documented order (blocks of 256 rows, the blocks in order)."""
import csv
import importlib.util
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch
from parity_log import parity

from test_gpu_cluster import dev, eps, lattice32, max_rel, rows

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


# ------------------------------------------------------------------------------------------------ the update kernel

# (n, d, k, R): n around the 64-row floor of a slab and with many slabs, every d class (a partial chunk, one chunk, many
# chunks, the largest), k = 300 > the 96 clusters of one LDS tile (four tiles), R in {1, 3}.
UPDATE_SHAPES = [(1, 4, 1, 1), (7, 52, 7, 3), (63, 4, 2, 1), (64, 512, 7, 3), (65, 52, 64, 1), (1000, 512, 64, 3),
                 (1000, 52, 300, 1), (1000, 512, 1, 1), (300, 1024, 300, 1), (4097, 1024, 2, 1), (4097, 4, 300, 3),
                 (65600, 8, 5, 3)]


def label_layouts(n, k, seed):
    """(name, labels int64 [n]): all rows in one cluster; one row per cluster (n <= k); clusters 0, k // 2 and k - 1
    empty; sorted; shuffled."""
    rng = np.random.default_rng(seed)
    out = [("one", np.full(n, k - 1, dtype=np.int64))]
    if n <= k:
        out.append(("each", np.arange(n, dtype=np.int64)))
    used = np.setdiff1d(np.arange(k), [0, k // 2, k - 1])
    if used.size:
        out.append(("empty", used[rng.integers(0, used.size, n)]))
    rand = rng.integers(0, k, n)
    out.append(("sorted", np.sort(rand)))
    out.append(("shuffled", rand))
    return out


def update64(x, labels, dist, prev, old):
    """The update restated: per restart and cluster the count and the sequential float64 sum of the members in row order
    (np.add.reduceat on the rows sorted stably by label), divided in double, rounded to float32 once; an empty cluster
    keeps its old centre.  labels, dist, prev [n, R]; old float32 [R, k, d]."""
    n, r_n = labels.shape
    k = old.shape[1]
    x64 = x.astype(np.float64)
    centres, counts = old.copy(), np.zeros((r_n, k), dtype=np.int64)
    inertia, changed = np.zeros(r_n), np.zeros(r_n, dtype=np.int64)
    for r in range(r_n):
        lab = labels[:, r]
        counts[r] = np.bincount(lab, minlength=k)
        order = np.argsort(lab, kind="stable")
        present = np.flatnonzero(counts[r])
        starts = np.concatenate([[0], np.cumsum(counts[r][present])[:-1]])
        sums = np.add.reduceat(x64[order], starts, axis=0)
        centres[r, present] = (sums / counts[r][present, None]).astype(np.float32)
        inertia[r] = math.fsum((dist[:, r].astype(np.float64) ** 2).tolist())
        changed[r] = n if prev is None else int((prev[:, r] != lab).sum())
    return centres, counts, inertia, changed


def run_update(x, labels, dist, prev, old):
    from ssl_wafermap_amd import cluster

    r_n, k, _ = old.shape
    offs = (np.arange(r_n) * k)[None, :]
    cols = dev((labels + offs).astype(np.int32))
    prev_cols = None if prev is None else dev((prev + offs).astype(np.int32))
    out = cluster._kmeans_update(dev(x), cols, dev(dist), prev_cols, dev(old))
    return [t.cpu().numpy() for t in out]


def check_update(x, labels, dist, prev, old, tag):
    n, d = x.shape
    new, counts, inertia, changed, shift2 = run_update(x, labels, dist, prev, old)
    want_c, want_counts, want_inertia, want_changed = update64(x, labels, dist, prev, old)
    assert np.array_equal(counts, want_counts), tag
    assert np.array_equal(changed, want_changed), tag
    ulp = np.spacing(np.abs(want_c))
    assert (np.abs(new.astype(np.float64) - want_c.astype(np.float64)) <= ulp).all(), tag
    assert np.array_equal(new[counts == 0], old[counts == 0]), tag  # an empty cluster keeps its centre
    bound = 2 * eps(d) + n * 2.0 ** -52
    parity(f"kmeans update inertia {tag}", max_rel(inertia, want_inertia), bound)
    move = new.astype(np.float64) - old.astype(np.float64)
    want_shift = np.array([math.fsum((m * m).ravel().tolist()) for m in move])
    parity(f"kmeans update shift2 {tag}", max_rel(shift2, want_shift), bound)
    return new, counts, inertia, changed, shift2


@pytest.mark.parametrize("n,d,k,r_n", UPDATE_SHAPES)
def test_update_against_float64(n, d, k, r_n):
    x = rows(n, d, 7 * n + d + k)
    rng = np.random.default_rng(n + d + k + r_n)
    old = rng.standard_normal((r_n, k, d)).astype(np.float32)
    dist = np.abs(rng.standard_normal((n, r_n))).astype(np.float32)
    names = [name for name, _ in label_layouts(n, k, 0)]
    for q, name in enumerate(names):
        # every restart its own labels of the layout (restart r: seed q + 100 r)
        labels = np.stack([dict(label_layouts(n, k, q + 100 * r))[name] for r in range(r_n)], axis=1)
        prev = None
        if name in ("sorted", "shuffled"):
            prev = labels.copy()
            flip = rng.random((n, r_n)) < 0.3
            prev[flip] = (prev[flip] + 1 + rng.integers(0, max(k - 1, 1), int(flip.sum()))) % k  # (k = 1: nothing changes)
        first = check_update(x, labels, dist, prev, old, f"n={n} d={d} k={k} R={r_n} {name}")
        if name == "shuffled":
            again = run_update(x, labels, dist, prev, old)
            for a, b in zip(first, again):
                assert a.tobytes() == b.tobytes(), "a second call returns the same bits"
            if r_n > 1:  # a restart alone gives the bits it gives among the others
                alone = run_update(x, labels[:, 1:2], dist[:, 1:2], prev[:, 1:2], old[1:2])
                for a, b in zip(first, alone):
                    assert a[1:2].tobytes() == b.tobytes(), "a restart's bits do not depend on the other restarts"


def test_update_cancellation():
    """rows = 1000 + 1e-3 * noise: a float32 accumulation would lose the noise; the float64 sum keeps the mean to an ulp."""
    n, d, k = 1000, 52, 7
    rng = np.random.default_rng(5)
    x = (1000.0 + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    labels = rng.integers(0, k, (n, 1))
    dist = np.abs(rng.standard_normal((n, 1))).astype(np.float32)
    old = np.full((1, k, d), 1000.0, dtype=np.float32)
    new, _, _, _, _ = check_update(x, labels, dist, None, old, "cancellation")
    exact = np.stack([[math.fsum(col) / (labels[:, 0] == c).sum() for col in x[labels[:, 0] == c].astype(np.float64).T]
                      for c in range(k)]).astype(np.float32)
    assert (np.abs(new[0].astype(np.float64) - exact.astype(np.float64)) <= np.spacing(exact)).all()


# ------------------------------------------------------------------------------------------------ one step


@pytest.fixture(scope="module")
def wafers():
    """The golden embeddings standardised in float64, as float32 rows."""
    e = np.load(GOLDEN / "simsiam_preds_subset.npz")["embeddings"].astype(np.float64)
    return ((e - e.mean(axis=0)) / np.maximum(e.std(axis=0), 1e-12)).astype(np.float32)


def dist64(x, c):
    """Exact-to-float64 Euclidean distances [n, k] of float32 rows and centres (differences first, as the kernels)."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for j in range(c.shape[0]):
        t = x - c[j]
        out[:, j] = np.sqrt((t * t).sum(axis=1))
    return out


def margins(dm):
    """Per row (argmin, second argmin, (second - best) / second) of a distance matrix with at least two columns."""
    part = np.argsort(dm, axis=1, kind="stable")[:, :2]
    best, second = dm[np.arange(dm.shape[0]), part[:, 0]], dm[np.arange(dm.shape[0]), part[:, 1]]
    with np.errstate(invalid="ignore", divide="ignore"):
        return part[:, 0], part[:, 1], np.where(second > 0, (second - best) / second, 0.0)


def init_rows(x, k, seed):
    return x[np.sort(np.random.default_rng(seed).permutation(x.shape[0])[:k])].copy()


@pytest.mark.parametrize("n,k", [(1536, 8), (4000, 25)])
def test_one_step_against_float64(wafers, n, k):
    from ssl_wafermap_amd import cluster, manifold

    x = wafers[:n]
    d = x.shape[1]
    init = init_rows(x, k, n + k)
    step = cluster.kmeans_step(dev(x), dev(init))
    labels, got_d = step.labels.cpu().numpy(), step.distances.cpu().numpy()
    dm = dist64(x, init)
    best, second, margin = margins(dm)
    close = margin < 4 * eps(d)
    assert close.mean() <= 0.01, "precondition: at most 1 % of the rows sit on a float32 tie"
    assert (labels[~close] == best[~close]).all()
    assert ((labels[close] == best[close]) | (labels[close] == second[close])).all()
    parity(f"kmeans step distance n={n} k={k}", max_rel(got_d, dm[np.arange(n), labels]), eps(d))
    # the update of that assignment
    want_c, want_counts, want_inertia, _ = update64(x, labels[:, None].astype(np.int64), got_d[:, None], None, init[None])
    assert np.array_equal(step.counts.cpu().numpy(), want_counts[0]) and int(step.n_changed) == n
    new = step.centres.cpu().numpy()
    assert (np.abs(new.astype(np.float64) - want_c[0].astype(np.float64)) <= np.spacing(np.abs(want_c[0]))).all()
    parity(f"kmeans step inertia n={n} k={k}", max_rel([float(step.inertia)], want_inertia), 2 * eps(d) + n * 2.0 ** -52)
    # the one distance function: knn_query's bits, and predict's choice is knn_query's
    kd, ki = manifold.knn_query(dev(x), dev(init), 1)
    assert np.array_equal(ki.cpu().numpy()[:, 0], labels) and kd.cpu().numpy()[:, 0].tobytes() == got_d.tobytes()
    model = cluster.KMeans(k, init=init, max_iter=2).fit(dev(x))
    kd, ki = manifold.knn_query(dev(x), model.cluster_centers_, 1)
    assert np.array_equal(model.predict(dev(x)), ki.cpu().numpy()[:, 0].astype(np.int64))
    t = model.transform(dev(x))
    assert t.shape == (n, k) and t.min(dim=1).values.cpu().numpy().tobytes() == kd.cpu().numpy()[:, 0].tobytes()
    assert model.score(dev(x)) <= 0 and model.n_features_in_ == d


# ------------------------------------------------------------------------------------------------ fit = the documented composition


def tol_scaled_of(x_d, tol):
    return float(x_d.double().var(dim=0, unbiased=False).mean()) * tol


def fit_by_steps(x_d, init_d, tol, max_iter):
    """KMeans.fit restated as a loop over kmeans_step with the stated stopping rule (no empty cluster may occur here)."""
    from ssl_wafermap_amd import cluster

    tol_s = tol_scaled_of(x_d, tol)
    centres, prev = init_d, None
    for it in range(1, max_iter + 1):
        step = cluster.kmeans_step(x_d, centres, prev)
        assert int(step.counts.min()) > 0
        centres, prev = step.centres, step.labels
        why = cluster.kmeans_stop(int(step.n_changed), float(step.shift2), tol_s)
        if why is not None:
            break
    if why != "labels":  # the closing assignment pass
        step = cluster.kmeans_step(x_d, centres)
    return step.labels.cpu().numpy().astype(np.int64), centres, float(step.inertia), it


@pytest.mark.parametrize("tol,max_iter", [(1e-4, 300), (0.0, 300), (0.0, 3)])
def test_fit_is_the_documented_composition(wafers, tol, max_iter):
    from ssl_wafermap_amd import cluster

    x_d = dev(wafers[:1536])
    init = init_rows(wafers[:1536], 8, 11)
    model = cluster.KMeans(8, init=init, tol=tol, max_iter=max_iter).fit(x_d)
    labels, centres, inertia, n_iter = fit_by_steps(x_d, dev(init), tol, max_iter)
    assert np.array_equal(model.labels_, labels) and model.n_iter_ == n_iter
    assert model.cluster_centers_.cpu().numpy().tobytes() == centres.cpu().numpy().tobytes()
    assert model.inertia_ == inertia
    assert model.labels_.dtype == np.int64 and model.cluster_centers_.is_cuda
    assert np.array_equal(cluster.KMeans(8, init=init, tol=tol, max_iter=max_iter).fit_predict(x_d), labels)


def test_restarts_equal_single_fits(wafers):
    from ssl_wafermap_amd import cluster

    x = wafers[:1536]
    x_d = dev(x)
    inits = np.stack([init_rows(x, 8, s) for s in (21, 22, 23)])
    inits_d = dev(inits)
    many = cluster.KMeans(8, init=inits_d).fit(x_d)
    assert np.array_equal(inits_d.cpu().numpy(), inits), "fit leaves the caller's init as it was"
    singles = [cluster.KMeans(8, init=inits[r]).fit(x_d) for r in range(3)]
    assert many.inertias_.tolist() == [m.inertia_ for m in singles]
    assert many.n_iters_.tolist() == [m.n_iter_ for m in singles]
    assert len(set(many.n_iters_.tolist())) > 1, "the restarts should stop at different iterations for this to test the dropping"
    best = int(np.argmin(many.inertias_))
    assert many.inertia_ == singles[best].inertia_ and many.n_iter_ == singles[best].n_iter_
    assert np.array_equal(many.labels_, singles[best].labels_)
    assert many.cluster_centers_.cpu().numpy().tobytes() == singles[best].cluster_centers_.cpu().numpy().tobytes()
    # "random" and "k-means++" restarts: seeded, reproducible, every row labelled
    for init, n_init in (("random", 3), ("k-means++", 2)):
        a = cluster.KMeans(8, init=init, n_init=n_init, random_state=4).fit(x_d)
        b = cluster.KMeans(8, init=init, n_init=n_init, random_state=4).fit(x_d)
        assert a.inertias_.shape == (n_init,) and a.inertia_ == a.inertias_.min() and a.inertias_.tolist() == b.inertias_.tolist()
        assert np.array_equal(a.labels_, b.labels_) and a.labels_.min() == 0 and a.labels_.max() == 7


def test_empty_cluster_rule_in_fit(wafers):
    """An init with one centre far from every row: iteration 1 has a zero count, and the far cluster takes the row
    farthest from its own centre (restated here in numpy), which leaves its old cluster's sum and count."""
    from ssl_wafermap_amd import cluster

    x = wafers[:1536]
    k, far = 8, 5
    init = init_rows(x, k, 31)
    init[far] = 1.0e3
    step = cluster.kmeans_step(dev(x), dev(init))
    labels, dist, counts = step.labels.cpu().numpy(), step.distances.cpu().numpy(), step.counts.cpu().numpy()
    assert counts[far] == 0 and (np.delete(counts, far) > 1).all()
    taken = int(np.lexsort((np.arange(x.shape[0]), -dist.astype(np.float64)))[0])  # (largest distance, lowest index)
    donor = int(labels[taken])
    want = step.centres.cpu().numpy().copy()
    want[far] = x[taken]
    rest = np.flatnonzero((labels == donor) & (np.arange(x.shape[0]) != taken))
    want[donor] = (np.array([math.fsum(col) for col in x[rest].astype(np.float64).T]) / rest.size).astype(np.float32)
    model = cluster.KMeans(k, init=init, max_iter=1).fit(dev(x))
    assert model.n_iter_ == 1 and model.cluster_centers_.cpu().numpy().tobytes() == want.tobytes()
    full = cluster.KMeans(k, init=init).fit(dev(x))
    assert np.bincount(full.labels_, minlength=k).min() > 0 and full.n_iter_ > 1


# ------------------------------------------------------------------------------------------------ against sklearn


def lloyd64(x, init, max_iter=300):
    """Float64 Lloyd iterations from `init` until the labels stop changing: (labels, centres, n_iter as sklearn counts,
    the smallest margin any row had in any iteration)."""
    x64, c = x.astype(np.float64), init.astype(np.float64)
    prev, worst = None, np.inf
    for it in range(1, max_iter + 1):
        best, _, margin = margins(dist64(x64, c))
        worst = min(worst, float(margin.min()))
        counts = np.bincount(best, minlength=c.shape[0])
        assert counts.min() > 0
        sums = np.zeros_like(c)
        np.add.at(sums, best, x64)
        c = sums / counts[:, None]
        if prev is not None and np.array_equal(prev, best):
            break
        prev = best
    return best, c, it, worst


# (k, seed of make_blobs and of the init rows): chosen on the CPU so that the float64 trajectory keeps every row's margin
# above 16 * eps(8) in every iteration (the precondition asserted below): the smallest margins are 70 and 260 eps(8), over
# 18 and 17 iterations
BLOB_CASES = [(5, 1), (12, 2)]


@pytest.mark.parametrize("k,seed", BLOB_CASES)
def test_fit_matches_sklearn_where_the_trajectory_has_margin(k, seed):
    from sklearn.cluster import KMeans as SkKMeans
    from sklearn.datasets import make_blobs

    from ssl_wafermap_amd import cluster

    n, d = 2000, 8
    x = make_blobs(n, d, centers=k, cluster_std=1.0, random_state=seed)[0].astype(np.float32)
    init = init_rows(x, k, seed)
    labels64, _, n_iter64, worst = lloyd64(x, init)
    assert worst >= 16 * eps(d), f"precondition: the float64 trajectory has margin (smallest {worst:.3g})"
    sk = SkKMeans(k, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=0).fit(x.astype(np.float64))
    assert np.array_equal(sk.labels_, labels64) and sk.n_iter_ == n_iter64  # (the restatement is sklearn's loop)
    model = cluster.KMeans(k, init=init, tol=0.0).fit(dev(x))
    assert np.array_equal(model.labels_, sk.labels_) and model.n_iter_ == sk.n_iter_
    parity(f"kmeans inertia against sklearn k={k}", abs(model.inertia_ - sk.inertia_) / sk.inertia_, 2 * eps(d))


@pytest.mark.parametrize("n,k", [(1536, 8), (4000, 25)])
def test_fit_on_wafer_embeddings_is_a_fixed_point(wafers, n, k):
    from sklearn.cluster import KMeans as SkKMeans

    from ssl_wafermap_amd import cluster

    x = wafers[:n]
    d = x.shape[1]
    init = init_rows(x, k, 3 * n + k)
    model = cluster.KMeans(k, init=init, tol=0.0).fit(dev(x))
    centres = model.cluster_centers_.cpu().numpy()
    dm = dist64(x, centres)
    own = dm[np.arange(n), model.labels_]
    assert (own <= (1 + 2 * eps(d)) * dm.min(axis=1)).all(), "every row sits at its nearest centre"
    want_c, counts, want_inertia, _ = update64(x, model.labels_[:, None], own[:, None].astype(np.float32), None, centres[None])
    assert counts.min() > 0
    assert (np.abs(centres.astype(np.float64) - want_c[0].astype(np.float64)) <= np.spacing(np.abs(want_c[0]))).all()
    parity(f"kmeans fixed point inertia n={n} k={k}", abs(model.inertia_ - float((own * own).sum())) / model.inertia_,
           2 * eps(d) + n * 2.0 ** -52)
    # recorded, not asserted: nothing guarantees sklearn's trajectory at margins below eps(512)
    sk = SkKMeans(k, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=0).fit(x.astype(np.float64))
    parity(f"kmeans label agreement with sklearn n={n} k={k}", float((sk.labels_ == model.labels_).mean()), 0.0, higher=True,
           note=f"n_iter {model.n_iter_} here, {sk.n_iter_} sklearn; recorded only")
    parity(f"kmeans inertia ratio to sklearn n={n} k={k}", model.inertia_ / sk.inertia_, np.inf, note="recorded only")


# ------------------------------------------------------------------------------------------------ seeding

BLOCK = 256  # rows per block of the seeding kernels' sums (include/wafer_hip.h)


def block_scan(v):
    """The kernels' running sums inside blocks of 256 rows (the same doubling tree for every block) and the block sums."""
    n = v.size
    nb = -(-n // BLOCK)
    a = np.zeros(nb * BLOCK)
    a[:n] = v
    a = a.reshape(nb, BLOCK)
    w = 1
    while w < BLOCK:
        b = a.copy()
        b[:, w:] = a[:, :-w] + a[:, w:]
        a, w = b, 2 * w
    return a.reshape(-1)[:n], a[:, -1].copy()


def block_tree_sums(v):
    n = v.size
    nb = -(-n // BLOCK)
    a = np.zeros(nb * BLOCK)
    a[:n] = v
    a = a.reshape(nb, BLOCK)
    w = BLOCK // 2
    while w:
        a = a[:, :w] + a[:, w:2 * w]
        w //= 2
    return a[:, 0]


def ordered_sum(v):
    """The kernels' sum of block values in block order: 256 runs of consecutive values, each added in order, then the runs
    in order; (total, exclusive offsets)."""
    count = v.size
    run = -(-count // BLOCK)
    starts, at = [], 0.0
    for t in range(BLOCK):
        mine = 0.0
        for b in range(min(count, t * run), min(count, t * run + run)):
            mine += float(v[b])
        starts.append(at)
        at = at + mine
    off = np.zeros(count)
    for t in range(BLOCK):
        cur = starts[t]
        for b in range(min(count, t * run), min(count, t * run + run)):
            off[b] = cur
            cur += float(v[b])
    return at, off


def uniform_row(u, n):
    return min(int(math.floor(u * n)), n - 1)


def seed_restatement(dist32, k, u):
    """Greedy k-means++ on a float32 distance matrix (exact on the lattice) in float64 numpy, the sums in the kernels'
    order: (indices [k], candidates [k, T], potentials [k, T])."""
    n, t_n = dist32.shape[0], u.shape[1]
    sq = dist32.astype(np.float64) ** 2
    idx, cands, pots = np.zeros(k, dtype=np.int64), np.full((k, t_n), -1, dtype=np.int64), np.full((k, t_n), np.inf)
    c2 = None
    for c in range(k):
        if c == 0:
            cand = [uniform_row(u[0, 0], n)]
        else:
            scan, bsum = block_scan(c2)
            total, off = ordered_sum(bsum)
            running = off[np.arange(n) // BLOCK] + scan
            cand = []
            for t in range(t_n):
                hit = np.flatnonzero((c2 > 0) & (running > u[c, t] * total))
                pos = np.flatnonzero(c2 > 0)
                cand.append(uniform_row(u[c, t], n) if total == 0 else int(hit[0]) if hit.size else int(pos[-1]))
        planes = [sq[:, j] if c2 is None else np.minimum(sq[:, j], c2) for j in cand]
        pot = [ordered_sum(block_tree_sums(p))[0] for p in planes]
        win = int(np.argmin(pot))
        idx[c], c2 = cand[win], planes[win]
        cands[c, :len(cand)], pots[c, :len(cand)] = cand, pot
    return idx, cands, pots


@pytest.mark.parametrize("k,trials,seed", [(1, None, 0), (6, None, 1), (40, 4, 2), (112, 2, 3)])
def test_seeding_exact_on_a_lattice(k, trials, seed):
    from ssl_wafermap_amd import cluster

    x, dist32 = lattice32("euclidean")
    t_n = 2 + int(math.log(k)) if trials is None else trials
    u = np.random.default_rng(seed).random((k, t_n))
    centres, idx, det = cluster.kmeans_plusplus(dev(x), k, uniforms=u, n_local_trials=trials, return_details=True)
    want_idx, want_cand, want_pot = seed_restatement(dist32, k, u)
    assert np.array_equal(idx, want_idx) and np.array_equal(det["candidates"], want_cand)
    assert det["potentials"].tobytes() == want_pot.tobytes()
    assert np.array_equal(centres.cpu().numpy(), x[idx]) and idx.dtype == np.int64
    if k == x.shape[0]:
        assert np.array_equal(np.sort(idx), np.arange(k)), "k = n returns every (distinct) row"
    # the default draw is numpy's generator, and a second call gives the same rows
    a = cluster.kmeans_plusplus(dev(x), k, random_state=9)[1]
    t_def = 2 + int(math.log(k))
    b = cluster.kmeans_plusplus(dev(x), k, uniforms=np.random.default_rng(9).random((k, t_def)))[1]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("n,d,k", [(1000, 52, 9), (4097, 512, 25), (700, 4, 30)])
def test_seeding_draws_are_valid_on_random_rows(n, d, k):
    """Against exact float64 distances: every candidate is a valid draw for its threshold within 2 * eps(d) of the
    potential, every potential is within 2 * eps(d), the winner is the device's lowest (ties to the lowest t)."""
    from ssl_wafermap_amd import cluster

    x = rows(n, d, 13 * n + d)
    u = np.random.default_rng(n + k).random((k, 2 + int(math.log(k))))
    _, idx, det = cluster.kmeans_plusplus(dev(x), k, uniforms=u, return_details=True)
    cand, pots = det["candidates"], det["potentials"]
    tol = 2 * eps(d) + n * 2.0 ** -52
    assert idx[0] == uniform_row(u[0, 0], n) and cand[0, 0] == idx[0] and (cand[0, 1:] == -1).all()
    sq = lambda j: (dist64(x, x[j:j + 1])[:, 0]) ** 2
    c2 = sq(int(idx[0]))
    parity(f"kmeans++ potential n={n} d={d} step 0", abs(pots[0, 0] - c2.sum()) / c2.sum(), tol)
    for c in range(1, k):
        pot = c2.sum()
        incl = np.cumsum(c2)
        excl = incl - c2
        for t in range(u.shape[1]):
            j = int(cand[c, t])
            thr = u[c, t] * pot
            assert 0 <= j < n and c2[j] > 0, "a row at distance 0 is never drawn"
            assert incl[j] >= thr - tol * pot and excl[j] <= thr + tol * pot, (c, t, j)
            want = np.minimum(c2, sq(j)).sum()
            assert abs(pots[c, t] - want) <= tol * want, (c, t)
        win = int(np.argmin(pots[c]))  # (the first of the lowest)
        assert idx[c] == cand[c, win]
        c2 = np.minimum(c2, sq(int(idx[c])))
    assert len(set(idx.tolist())) == k


def test_seeding_never_draws_a_duplicate_while_the_potential_is_positive():
    from ssl_wafermap_amd import cluster

    base = np.random.default_rng(8).standard_normal((40, 52)).astype(np.float32)
    x = np.repeat(base, 3, axis=0)[np.random.default_rng(9).permutation(120)]
    centres, idx = cluster.kmeans_plusplus(dev(x), 40, random_state=1)
    assert np.unique(x[idx], axis=0).shape[0] == 40  # 40 distinct rows: no row value twice
    centres, idx = cluster.kmeans_plusplus(dev(x), 50, random_state=1)  # the potential reaches 0 after 40: uniform rows follow
    assert np.unique(x[idx[:40]], axis=0).shape[0] == 40 and idx.shape == (50,) and idx.min() >= 0 and idx.max() < 120


# ------------------------------------------------------------------------------------------------ the script


def test_kmeans_script_on_wafer_embeddings(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("embedding_kmeans_amd", ROOT / "scripts" / "embedding_kmeans_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    summary = mod.main(["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "1536", "--k", "6:8", "--n-init", "2",
                        "--holdout", "100", "--out", str(tmp_path)])
    with open(tmp_path / "trials.csv") as fh:
        table = list(csv.DictReader(fh))
    assert [int(r["k"]) for r in table] == [6, 7, 8] and list(table[0]) == mod.COLUMNS
    for row in table:
        assert all(np.isfinite(float(row[c])) for c in mod.COLUMNS), row
        assert -1 <= float(row["silhouette"]) <= 1 and 0 <= float(row["homogeneity"]) <= 1 and float(row["inertia"]) > 0
    chosen = max(table, key=lambda r: float(r["silhouette"]))
    assert summary["chosen_k"] == int(chosen["k"]) == json.loads((tmp_path / "summary.json").read_text())["chosen_k"]
    labels, centers = np.load(tmp_path / "labels.npy"), np.load(tmp_path / "centers.npy")
    assert labels.shape == (1436,) and labels.min() == 0 and labels.max() == summary["chosen_k"] - 1
    assert centers.shape == (summary["chosen_k"], 512) and centers.dtype == np.float32
    hold = np.load(tmp_path / "holdout_labels.npy")
    assert hold.shape == (100,) and hold.min() >= 0 and hold.max() < summary["chosen_k"] and summary["holdout"] == 100
    assert capsys.readouterr().out.count("nearest (row, L2, failure code)") == summary["chosen_k"]
