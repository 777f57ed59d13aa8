"""GPU checks of the DBCV cluster validity (csrc/cluster.hip: wm_allpoints_core, wm_mreach_min_edge_grouped,
wm_group_min_mreach; cluster.py: allpoints_core_distances, grouped_min_outgoing_edges, group_min_mreach, validity_index,
HDBSCAN.relative_validity_; scripts/embedding_clustering_amd.py --validity) against the float64 restatements of
test_dbcv_cpu and against the bits of the square kernels.

Bounds are derived as in test_gpu_cluster: one float32 distance is within eps(d) = (d + 3) * 2^-24 relative of the exact
distance of the float32 rows; minima and maxima of such values are within eps.  What this file adds:

  all-points core   the power mean ((1 / (n_c - 1)) sum dist^-p)^(-1 / p) is homogeneous of degree 1 and monotone in every
                    distance, so distances within a relative eps give a result within eps.  The double arithmetic on top:
                    t = -p log(dist) has |t| <= p |log dist| < 2^13 in every case here (p <= 1024, dist in 1e-3 .. 1e3);
                    log, the product, the subtraction t - M and exp each err by at most 2 ulp of a quantity below 2^13,
                    so an exponent is off by at most 8 * 2^13 * 2^-53 = 2^-37 and every term, and with it S, by that
                    relative amount; n_c additions add n_c 2^-53 < 2^-43; M + log S and the division by p only shrink
                    what came before.  The float64 reference (numpy's logaddexp) errs likewise: DOUBLE = 2^-36 covers
                    both.
  mutual reachability   max(core_i, core_j, dist) with core a float32 rounding (2^-24) of an all-points core: within
                    eps1(d) = eps(d) + 2^-24 + DOUBLE of the float64 value.
  the score         V_c = (sep - sparse) / max(sep, sparse) is +-(1 - lo / hi) of two such weights (a maximum over the
                    same edges, a minimum over the same pairs as the reference's): lo / hi moves by at most
                    2 eps1 / (1 - eps1), the weights n_c / n sum to at most 1, so |score - reference| <= 2 (eps(d) + 2^-23)
                    (2^-23 > 2^-24 + DOUBLE + the second-order term).
"""
import json
import math

import numpy as np
import pytest
import torch
from parity_log import parity
from pathlib import Path

from test_cluster_cpu import pairwise64
from test_dbcv_cpu import allpoints_core64, brute_dbcv, relative_validity64
from test_gpu_cluster import check_tree, components, dev, eps, lattice32, max_rel, reference, rows
from test_gpu_hdbscan_predict import four_blobs, queries
from test_gpu_hdbscan_soft import SHAPES, cross, layouts

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
METRICS = ["euclidean", "manhattan"]
DOUBLE = 2.0 ** -36


def score_bound(d):
    return 2 * (eps(d) + 2.0 ** -23)


def group_layouts(n):
    """(name, group int64 [n] non-decreasing, g): one group; two groups split at row 66 (inside the second 64-row /
    64-column tile); runs of 2, 3, 4, 5 rows (many groups per tile, groups across every tile edge, a last run of
    whatever is left, possibly a single row); 500 + 200 at n = 700 (groups of several tiles and several slices)."""
    out = [("one", np.zeros(n, dtype=np.int64), 1)]
    if n > 70:
        out.append(("split", (np.arange(n) >= 66).astype(np.int64), 2))
    if n > 2:
        small = np.repeat(np.arange(n), np.resize([2, 3, 4, 5], n))[:n]
        out.append(("small", small.astype(np.int64), int(small.max()) + 1))
    if n == 700:
        out.append(("500+200", (np.arange(n) >= 500).astype(np.int64), 2))
    return out


def members_of(group, g):
    starts = np.searchsorted(group, np.arange(g + 1))
    return [np.arange(starts[c], starts[c + 1]) for c in range(g)]


def sample(items, k=6):
    return items if len(items) <= k else [items[i] for i in np.linspace(0, len(items) - 1, k).astype(int)]


# ------------------------------------------------------------------------------------------------ all-points core


def core64_grouped(dist, group, g, p):
    out = np.zeros(dist.shape[0])
    for m in members_of(group, g):
        out[m] = allpoints_core64(dist[np.ix_(m, m)], p)
    return out


def plain_core64(dist, group, g, p):
    """The package's form, dist^-p in plain float64 (0, inf or nan where that leaves the range)."""
    out = np.zeros(dist.shape[0])
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for m in members_of(group, g):
            for i in m:
                pos = dist[i, m][dist[i, m] > 0]
                out[i] = ((pos ** -p).sum() / (m.size - 1)) ** (-1.0 / p) if pos.size else 0.0
    return out


@pytest.mark.parametrize("d", [4, 52, 512, 1024])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 700])
def test_allpoints_core_against_float64_logaddexp(n, d):
    from ssl_wafermap_amd import cluster

    for metric in (METRICS if d <= 52 or n <= 65 else METRICS[:1]):  # (the float64 matrix of 700 x 1024 once)
        x, dist = reference(n, d, metric)
        xd = dev(x)
        for name, group, g in group_layouts(n):
            for p in (float(d), 2.0):
                tag = f"{metric} n={n} d={d} p={p:g} {name}"
                got = cluster.allpoints_core_distances(xd, group, d=p, metric=metric)
                assert got.dtype == torch.float64 and got.is_cuda and got.shape == (n,)
                got = got.cpu().numpy()
                want = core64_grouped(dist, group, g, p)
                parity(f"allpoints_core {tag} rel", max_rel(got, want), eps(d) + DOUBLE)
                plain = plain_core64(dist, group, g, p)
                ok = np.isfinite(plain) & (plain > 0)
                if p == 2.0:
                    assert ok[want > 0].all()  # (the case is what it claims: the plain form is in range here)
                parity(f"allpoints_core {tag} plain form rel", max_rel(got[ok], plain[ok]), eps(d) + DOUBLE)
                if name == "one" and n >= 8:
                    # rows 0, 3, 5, 7 and n - 1 are copies: they see each other at 0 and must not contribute; the
                    # copies share every other distance bit for bit, so they get the same bits
                    assert (got[[3, 5, 7, n - 1]] == got[0]).all() and got[0] > 0
                again = cluster.allpoints_core_distances(xd, group, d=p, metric=metric).cpu().numpy()
                assert np.array_equal(got.view(np.int64), again.view(np.int64)), tag


def test_allpoints_core_default_power_noise_and_unsorted_labels():
    from ssl_wafermap_amd import cluster

    n, d = 257, 50  # 50 features: padded to 52, the default power stays 50
    x = rows(n, d, 5)
    dist = pairwise64(x)
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 5, n) * 3 - 1  # -1 (noise), 2, 5, 8, 11 in any order
    got = cluster.allpoints_core_distances(dev(x), torch.from_numpy(lab)).cpu().numpy()
    assert np.isnan(got[lab < 0]).all() and not np.isnan(got[lab >= 0]).any()
    for c in (2, 5, 8, 11):
        m = np.flatnonzero(lab == c)
        parity(f"allpoints_core wrapper label {c} rel", max_rel(got[m], allpoints_core64(dist[np.ix_(m, m)], 50.0)), eps(52) + DOUBLE)
    assert np.isnan(cluster.allpoints_core_distances(dev(x), np.full(n, -1)).cpu().numpy()).all()


def test_allpoints_core_identical_group_and_wide_spread():
    from ssl_wafermap_amd import cluster

    # a group of 70 identical rows (across the tile edge) next to a random one: exactly 0 for every row of it
    x = rows(130, 52, 3)
    x[:70] = x[0]
    group = (np.arange(130) >= 70).astype(np.int64)
    got = cluster.allpoints_core_distances(dev(x), group).cpu().numpy()
    assert (got[:70] == 0).all() and (got[70:] > 0).all()
    # d = 1024, distances from 1e-3 to 1e3 on a line: the plain float64 power is 0 or inf for most rows (all but those
    # whose nearest row is at a distance within a few percent of 1)
    d, n = 1024, 65
    s = np.concatenate([[0.0], np.logspace(-3, 3, n - 1)])
    x = (s[:, None] / 32.0 * np.ones(d)).astype(np.float32)  # (|e| = 1 for e = ones / 32)
    dist = pairwise64(x)
    pos = dist[dist > 0]
    assert pos.min() < 2e-3 and pos.max() > 5e2
    group = np.zeros(n, dtype=np.int64)
    plain = plain_core64(dist, group, 1, float(d))
    lost = (plain == 0) | ~np.isfinite(plain)
    assert lost.mean() > 0.8 and (plain[:20] == 0).all() and np.isinf(plain[-10:]).all()  # dist^-p overflows, then (.)^(-1/p) gives 0; underflows: inf
    want = core64_grouped(dist, group, 1, float(d))
    assert np.isfinite(want).all() and (want > 0).all()
    got = cluster.allpoints_core_distances(dev(x), group).cpu().numpy()
    parity("allpoints_core d=1024 spread 1e-3..1e3 rel", max_rel(got, want), eps(d) + DOUBLE)
    parity("allpoints_core d=1024 spread, plain form where it is in range, rel", max_rel(got[~lost], plain[~lost]), eps(d) + DOUBLE)


# ------------------------------------------------------------------------------------------------ grouped min edge


def grouped_components(group, kind):
    if kind == "whole":
        return (group * 3 + 1).astype(np.int32)  # every component holds its whole group
    return components(group.shape[0], kind)  # (ids shared across groups: the group condition must still hold)


@pytest.mark.parametrize("kind", ["singletons", "halves", "whole"])
@pytest.mark.parametrize("n,d", [(2, 4), (65, 4), (257, 52), (300, 512), (700, 52)])
def test_grouped_min_edge_equals_the_square_kernel_per_group(n, d, kind):
    from ssl_wafermap_amd import cluster

    for metric in METRICS:
        x, dist = reference(n, d, metric)
        core32 = np.sort(dist, axis=1)[:, min(5, n) - 1].astype(np.float32)
        xd, cd = dev(x), dev(core32)
        for name, group, g in group_layouts(n):
            tag = f"{metric} n={n} d={d} {kind} {name}"
            comp = grouped_components(group, kind)
            got_w, got_j = cluster.grouped_min_outgoing_edges(xd, cd, dev(comp), torch.from_numpy(group), g, metric)
            assert got_w.dtype == torch.float32 and got_j.dtype == torch.int32
            got_w, got_j = got_w.cpu().numpy(), got_j.cpu().numpy()
            w = np.maximum(np.maximum(core32[:, None].astype(np.float64), core32[None, :].astype(np.float64)), dist)
            w = np.where((comp[:, None] != comp[None, :]) & (group[:, None] == group[None, :]), w, np.inf)
            none = np.isinf(w).all(axis=1)
            assert (got_j[none] == -1).all() and np.isposinf(got_w[none]).all(), tag
            if kind == "whole":
                assert none.all()
            has = ~none
            assert (got_j[has] >= 0).all() and (group[got_j[has]] == group[has]).all() and (comp[got_j[has]] != comp[has]).all()
            if has.any():
                parity(f"grouped min_edge weight {tag} rel", max_rel(got_w[has], w.min(axis=1)[has]), eps(d))
                parity(f"grouped min_edge argmin {tag} rel", max_rel(w[np.flatnonzero(has), got_j[has]], w.min(axis=1)[has]), eps(d))
            for m in sample(members_of(group, g)):  # the same bits as the square kernel on the group's rows alone
                sub_w, sub_j = cluster.min_outgoing_edges(dev(x[m]), dev(core32[m]), dev(comp[m]), metric)
                sub_w, sub_j = sub_w.cpu().numpy(), sub_j.cpu().numpy()
                assert np.array_equal(got_w[m].view(np.int32), sub_w.view(np.int32)), tag
                assert np.array_equal(got_j[m], np.where(sub_j >= 0, m[0] + sub_j, -1)), tag
            again = cluster.grouped_min_outgoing_edges(xd, cd, dev(comp), torch.from_numpy(group), g, metric)
            assert np.array_equal(got_w.view(np.int32), again[0].cpu().numpy().view(np.int32)) and np.array_equal(got_j, again[1].cpu().numpy())


@pytest.mark.parametrize("kind", ["singletons", "halves", "whole"])
@pytest.mark.parametrize("metric", METRICS)
def test_grouped_min_edge_exact_on_a_lattice(metric, kind):
    from ssl_wafermap_amd import cluster

    x, dist = lattice32(metric)
    n = x.shape[0]
    core32 = np.sort(dist, axis=1)[:, 3]
    for group in (np.arange(n) * 3 // n, np.arange(n) % 3):  # runs, and interleaved ids (the wrapper's sort)
        comp = grouped_components(group, kind)
        w = np.maximum(np.maximum(core32[:, None], core32[None, :]), dist)
        w = np.where((comp[:, None] != comp[None, :]) & (group[:, None] == group[None, :]), w, np.float32(np.inf))
        got_w, got_j = cluster.grouped_min_outgoing_edges(dev(x), dev(core32), dev(comp), torch.from_numpy(group), 3, metric)
        got_w, got_j = got_w.cpu().numpy(), got_j.cpu().numpy()
        if kind == "whole":
            assert (got_j == -1).all() and np.isposinf(got_w).all()
        else:
            assert np.array_equal(got_w, w.min(axis=1).astype(np.float32))
            assert np.array_equal(got_j, w.argmin(axis=1)), "equal weights must resolve to the lowest j"


# ------------------------------------------------------------------------------------------------ grouped Boruvka


def prim_total(mr):
    n = mr.shape[0]
    best, seen, total = mr[0].copy(), np.zeros(n, dtype=bool), 0.0
    seen[0] = True
    for _ in range(n - 1):
        j = int(np.argmin(np.where(seen, np.inf, best)))
        total += best[j]
        seen[j] = True
        best = np.minimum(best, mr[j])
    return total


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [65, 700])
def test_grouped_boruvka_against_float64_prim(n, metric):
    from ssl_wafermap_amd import cluster

    d = 52
    x, dist = reference(n, d, metric)
    xd = dev(x)
    for name, group, g in group_layouts(n):
        if np.bincount(group).min() < 2:  # (the forest is defined on groups of at least two rows: validity_index drops the rest)
            keep = np.bincount(group)[group] >= 2
            xs, ds, group = x[keep], dist[np.ix_(keep, keep)], group[keep]
            g = int(group.max()) + 1
        else:
            xs, ds = x, dist
        core = cluster.allpoints_core_distances(dev(xs), group, metric=metric).float().contiguous()
        u, v, w, rounds = cluster._boruvka(dev(xs), core, metric, 1.0, dev(group.astype(np.int32)), g)
        assert u.shape == (group.shape[0] - g,) and (group[u] == group[v]).all()
        assert rounds <= max(1, math.ceil(math.log2(np.bincount(group).max()))), (name, rounds)
        c64 = core.cpu().numpy().astype(np.float64)
        for m in members_of(group, g):
            e = group[u] == group[m[0]]
            check_tree(u[e] - m[0], v[e] - m[0], w[e], m.size)
            mr = np.maximum(np.maximum(c64[m][:, None], c64[m][None, :]), ds[np.ix_(m, m)])
            want = prim_total(mr)
            parity(f"grouped mst weight {metric} n={n} {name} group at {m[0]} abs", abs(w[e].sum() - want), m.size * eps(d) * mr.max())
        key = np.stack([w, u, v], axis=1)
        assert all(tuple(key[i]) <= tuple(key[i + 1]) for i in range(key.shape[0] - 1))


# ------------------------------------------------------------------------------------------------ group min of the mutual reachability

GM_SHAPES = SHAPES[:5] + [(2100, 2600, 4)]


def test_group_min_shapes_are_the_small_ones():
    assert GM_SHAPES == [(1, 1, 4), (63, 2, 52), (64, 64, 512), (65, 65, 1024), (300, 300, 52), (2100, 2600, 4)]


@pytest.mark.parametrize("m,e,d", GM_SHAPES)
def test_group_min_mreach_against_float64_and_the_query_kernel(m, e, d):
    from ssl_wafermap_amd import cluster

    for metric in (METRICS if m < 2000 else METRICS[:1]):  # (the large shape is about slices and tiles, not the metric)
        xe = rows(e, d, 31 * e + d)
        xq, _ = queries(xe, m, 17 * m + e + d)
        dq = cross(xq, xe, metric)
        k = min(5, e)
        core = np.sort(cross(xe, xe, metric), axis=1)[:, k - 1].astype(np.float32)
        cq = np.sort(np.concatenate([np.zeros((m, 1)), dq], axis=1), axis=1)[:, k - 1].astype(np.float32)
        w_all = np.maximum(np.maximum(cq[:, None].astype(np.float64), core[None, :].astype(np.float64)), dq)
        xqd, xed, cqd, cd = dev(xq), dev(xe), dev(cq), dev(core)
        zq, ze = torch.zeros(m, device=xqd.device), torch.zeros(e, device=xqd.device)
        for name, group, g in layouts(e, m + e + d):
            tag = f"{metric} m={m} e={e} d={d} {name}"
            gt = torch.from_numpy(group)
            got_w, got_j = cluster.group_min_mreach(xqd, cqd, xed, cd, gt, g, metric)
            assert got_w.dtype == torch.float32 and got_j.dtype == torch.int32 and got_w.shape == got_j.shape == (m, g)
            got_w, got_j = got_w.cpu().numpy(), got_j.cpu().numpy()
            present = np.zeros(g, dtype=bool)
            present[group] = True
            assert np.isposinf(got_w[:, ~present]).all() and (got_j[:, ~present] == -1).all()
            cols = np.flatnonzero(present)
            assert (got_j[:, cols] >= 0).all() and (group[got_j[:, cols]] == cols[None, :]).all()
            want = np.stack([w_all[:, group == c].min(axis=1) for c in cols], axis=1)
            parity(f"group_min_mreach weight {tag} rel", max_rel(got_w[:, cols], want), eps(d))
            parity(f"group_min_mreach argmin {tag} rel", max_rel(np.take_along_axis(w_all, got_j[:, cols].astype(np.int64), axis=1), want), eps(d))
            # wm_mreach_query's weight on the group's columns alone, bit for bit (the lowest index among equal weights is
            # checked on the lattice below, where float32 is exact)
            for c in sample(list(cols)):
                mem = np.flatnonzero(group == c)
                qw, _, _ = cluster.mreach_query(xqd, cqd, dev(xe[mem]), dev(core[mem]), metric)
                assert np.array_equal(got_w[:, c].view(np.int32), qw.cpu().numpy().view(np.int32)), tag
            zw, zj = cluster.group_min_mreach(xqd, zq, xed, ze, gt, g, metric)  # all cores 0: the plain group min
            pd, pj = cluster.group_min_distances(xqd, xed, gt, g, metric)
            assert torch.equal(zw.view(torch.int32), pd.view(torch.int32)) and torch.equal(zj, pj), tag
            again = cluster.group_min_mreach(xqd, cqd, xed, cd, gt, g, metric)
            assert np.array_equal(got_w.view(np.int32), again[0].cpu().numpy().view(np.int32)) and np.array_equal(got_j, again[1].cpu().numpy())


@pytest.mark.parametrize("metric", METRICS)
def test_group_min_mreach_lowest_index_on_a_lattice(metric):
    from ssl_wafermap_amd import cluster

    x, dist = lattice32(metric)
    n = x.shape[0]
    core = np.sort(dist, axis=1)[:, 3]
    w = np.maximum(np.maximum(core[:, None], core[None, :]), dist)
    assert w.dtype == np.float32
    ties = 0
    for group in (np.arange(n) * 4 // n, np.arange(n) % 4):
        got_w, got_j = cluster.group_min_mreach(dev(x), dev(core), dev(x), dev(core), torch.from_numpy(group), 4, metric)
        got_w, got_j = got_w.cpu().numpy(), got_j.cpu().numpy()
        for c in range(4):
            mem = np.flatnonzero(group == c)
            sub = w[:, mem]
            assert np.array_equal(got_w[:, c], sub.min(axis=1))
            assert np.array_equal(got_j[:, c], mem[sub.argmin(axis=1)]), "ties must resolve to the lowest index"
            ties += int(((sub == sub.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties > n  # (the case is what it claims)


# ------------------------------------------------------------------------------------------------ end to end


def forests_of(parts):
    """The device's trees per cluster in the cluster's own row numbering (what brute_dbcv takes in place of Kruskal's)."""
    group, u, v = parts["group"], parts["u"], parts["v"]
    starts = np.searchsorted(group, np.arange(int(group.max()) + 1))
    return [[(int(a - starts[c]), int(b - starts[c])) for a, b in zip(u[group[u] == c], v[group[u] == c])]
            for c in range(starts.size)]


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("p", [4.0, 52.0])
def test_validity_index_on_the_devices_own_trees(p, noise):
    """The float64 restatement recomputes core distances, reachabilities, internal rows, sparseness and separations, but
    on the device's tree edges: mutual-reachability weights tie and nearly tie (many edges out of a row weigh exactly
    its core distance), so two correct trees may differ and with them the internal rows."""
    from ssl_wafermap_amd import cluster

    x, blob, _, _ = four_blobs()
    lab = blob.copy()
    if noise:
        lab[np.random.default_rng(2).permutation(300)[:30]] = -1
    dim = x.shape[1]
    for metric in METRICS:
        score, per, parts = cluster.validity_index(dev(x), lab, metric, d=p, per_cluster_scores=True, return_parts=True)
        assert isinstance(score, float) and -1.0 <= score <= 1.0 and per.shape == (4,) and per.dtype == np.float64
        assert np.array_equal(parts["rows"], np.flatnonzero(lab >= 0)[np.argsort(lab[lab >= 0], kind="stable")])
        ref = brute_dbcv(x, lab, metric, p, forests_of(parts))
        tag = f"{metric} p={p:g} noise={noise}"
        parity(f"validity_index {tag} abs", abs(score - ref["score"]), score_bound(dim))
        parity(f"validity_index per cluster {tag} abs", np.max(np.abs(per - ref["v"])), score_bound(dim))
        parity(f"validity_index cores {tag} rel", max_rel(parts["core"], np.concatenate(ref["cores"])), eps(dim) + DOUBLE)
        assert np.array_equal(np.flatnonzero(parts["internal"]),
                              np.concatenate([m0 + i for m0, i in zip(np.searchsorted(parts["group"], np.arange(4)), ref["internal"])]))
        sizes = np.bincount(lab[lab >= 0], minlength=4)
        assert score == float(np.cumsum(sizes / 300.0 * per)[-1])  # per_cluster_scores sum back with the n_c / n weights
        assert score == cluster.validity_from_parts(parts["sizes"], 300, parts["sparseness"], parts["sep"])[0]
        assert parts["rounds"] <= math.ceil(math.log2(sizes.max()))
        again = cluster.validity_index(dev(x), torch.from_numpy(lab), metric, d=p)
        assert np.float64(again).view(np.int64) == np.float64(score).view(np.int64)  # two runs: the same bits
        if noise:  # the noise rows count in n: the same clusters without them score higher by 300 / 270
            assert cluster.validity_index(dev(x[lab >= 0]), lab[lab >= 0], metric, d=p) == pytest.approx(score * 300 / 270, rel=1e-12)


def chains():
    """Four clusters of 70, 20, 3 and 2 points in 52 dimensions, each a chain on a line along (1, ..., 1) / sqrt(52) with
    gaps that grow by 6 % per step from 1, the clusters 1e4 apart on an axis of their own: more than 100 times the
    largest gap (1.06^68 = 53)."""
    xs, lab = [], []
    for c, size in enumerate([70, 20, 3, 2]):
        s = np.concatenate([[0.0], np.cumsum(1.06 ** np.arange(size - 1))])
        pts = s[:, None] / math.sqrt(52.0) * np.ones(52)
        pts[:, c] += 1e4 * (c + 1)
        xs.append(pts)
        lab += [c] * size
    return np.concatenate(xs).astype(np.float32), np.asarray(lab)


def test_validity_index_on_chains_fully_independent():
    """Here the reference builds its own trees (Kruskal): every cluster's tree is the chain by a wide margin, which is
    asserted on the float64 reference, so both sides must find the same internal rows."""
    from ssl_wafermap_amd import cluster

    x, lab = chains()
    ref = brute_dbcv(x, lab)
    gaps = [np.diff(np.flatnonzero(lab == c)) for c in range(4)]
    assert all((g == 1).all() for g in gaps)
    for c, (edges, core) in enumerate(zip(ref["edges"], ref["cores"])):
        n_c = core.size
        assert sorted((i, j) for i, j, _ in edges) == [(i, i + 1) for i in range(n_c - 1)], "the tree must be the chain"
        rows_c = x[lab == c].astype(np.float64)
        dist = pairwise64(rows_c)
        mr = np.maximum(np.maximum(core[:, None], core[None, :]), dist)
        chain_w = np.array([mr[i, i + 1] for i in range(n_c - 1)])
        for i in range(n_c):
            for j in range(i + 2, n_c):
                assert mr[i, j] >= 1.5 * chain_w[i:j].max(), "every other pair is far heavier than its tree path"
        if n_c > 2:  # the chain's weights are separated too: the order of its edges, and its largest, are not in doubt
            assert (np.diff(chain_w) >= 0.02 * chain_w[:-1]).all()
    off = ref["sep"][~np.eye(4, dtype=bool)]
    assert off.min() >= 100 * 1.06 ** 68
    score, per, parts = cluster.validity_index(dev(x), lab, per_cluster_scores=True, return_parts=True)
    assert sorted(zip(parts["u"].tolist(), parts["v"].tolist())) == sorted((i, i + 1) for i in range(94) if lab[i] == lab[i + 1])
    parity("validity_index chains abs", abs(score - ref["score"]), score_bound(52))
    parity("validity_index chains per cluster abs", np.max(np.abs(per - ref["v"])), score_bound(52))
    parity("validity_index chains sparseness rel", max_rel(parts["sparseness"], ref["sparseness"]), eps(52) + 2.0 ** -24 + DOUBLE)
    parity("validity_index chains separation rel", max_rel(parts["sep"][~np.eye(4, dtype=bool)], off), eps(52) + 2.0 ** -24 + DOUBLE)
    assert -1.0 <= score <= 1.0 and score > 0.9  # (chains 1e4 apart: as valid as a clustering gets)
    assert score == cluster.validity_index(dev(x), lab)
    # the same labelling under other ids, in another row order and with a singleton cluster and noise added: the usable
    # clusters and their trees are the same, n grows by two
    perm = np.random.default_rng(4).permutation(95)
    x2 = np.concatenate([x[perm], x[:2] + 3.0])
    lab2 = np.concatenate([lab[perm] * 5 + 2, [40, -1]])
    s2, per2 = cluster.validity_index(dev(x2), lab2, per_cluster_scores=True)
    assert per2.shape == (41,) and per2[40] == 0 and (np.delete(per2, [2, 7, 12, 17]) == 0).all()
    # (another row order adds the core distances' terms in another order: both runs are within the bound of the reference)
    parity("validity_index chains relabelled per cluster abs", np.max(np.abs(per2[[2, 7, 12, 17]] - ref["v"])), score_bound(52))
    parity("validity_index chains relabelled abs", abs(s2 - ref["score"] * 95 / 97), score_bound(52))


# ------------------------------------------------------------------------------------------------ the model and the script


def test_relative_validity_of_a_fitted_model():
    from ssl_wafermap_amd import cluster

    x = np.load(GOLDEN / "simsiam_preds_subset.npz")["embeddings"][:1536].astype(np.float32)
    model = cluster.HDBSCAN(min_cluster_size=15, min_samples=5)
    assert model.relative_validity_ is None
    model.fit(dev(x))
    first = model.relative_validity_
    assert isinstance(first, float) and -1.0 <= first <= 1.0 and model.labels_.max() >= 1
    assert first == relative_validity64(model.minimum_spanning_tree_.tolist(), model.labels_)
    labels = model.labels_.copy()
    model.refit(min_cluster_size=75, cluster_selection_epsilon=1.5)
    assert not np.array_equal(labels, model.labels_)
    second = model.relative_validity_
    assert second == relative_validity64(model.minimum_spanning_tree_.tolist(), model.labels_) and second != first


def test_sweep_script_with_validity(tmp_path):
    import csv
    import importlib.util

    spec = importlib.util.spec_from_file_location("embedding_clustering_amd", ROOT / "scripts" / "embedding_clustering_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = ["--embeddings", str(GOLDEN / "simsiam_preds_subset.npz"), "--rows", "1536", "--trials", "4", "--metrics", "euclidean",
            "--seed", "0"]
    summary = mod.main(args + ["--out", str(tmp_path / "with"), "--validity"])
    with open(tmp_path / "with" / "trials.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == 4 and list(table[0]) == mod.COLUMNS + ["relative_validity", "dbcv"]
    for row in table:
        assert -1.0 <= float(row["relative_validity"]) <= 1.0
        if int(row["n_clusters"]) >= 2:
            assert np.isfinite(float(row["dbcv"])) and -1.0 <= float(row["dbcv"]) <= 1.0
        else:
            assert np.isnan(float(row["dbcv"]))
    scored = [i for i, row in enumerate(table) if int(row["n_clusters"]) >= 2]
    assert scored and summary["chosen_by_dbcv"] == max(scored, key=lambda i: float(table[i]["dbcv"]))
    assert json.loads((tmp_path / "with" / "summary.json").read_text())["chosen_by_dbcv"] == summary["chosen_by_dbcv"]
    with open(tmp_path / "with" / "pareto.csv") as fh:
        assert list(csv.DictReader(fh).fieldnames) == mod.COLUMNS + ["relative_validity", "dbcv"]
    plain = mod.main(args + ["--out", str(tmp_path / "without")])
    with open(tmp_path / "without" / "trials.csv") as fh:
        old = list(csv.DictReader(fh))
    assert list(old[0]) == mod.COLUMNS and "chosen_by_dbcv" not in plain
    same = mod.COLUMNS[:7]  # the parameters and the counts (the scores' last digits move with the scaler's statistics)
    assert [{c: row[c] for c in same} for row in table] == [{c: row[c] for c in same} for row in old]
