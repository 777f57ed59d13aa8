"""Run every entry point of csrc/cluster.hip through cluster.py / manifold.py on seeded rows and save the outputs: run once
per library build (WM_HIP_LIB selects it) and compare the files (host-side changes that must be bit-identical).

    WM_HIP_LIB=<build A> python tools/probes/cluster_bitexact_probe.py a.pt
    WM_HIP_LIB=<build B> python tools/probes/cluster_bitexact_probe.py b.pt
    python tools/probes/cluster_bitexact_probe.py --compare a.pt b.pt      # exit status 1 if any entry differs

Shapes, after cl_grid: n = 64 (one tile, one slice: rank and group min store straight into the outputs), 65 (two slices of
one tile), 300 (five slices), and at d = 4 only n = 4160 (128-row modes: 33 row tiles x 22 slices of 3 tiles, the last
with 2; 64-row modes: 65 row tiles x 13 slices of 5); group min also at m = 9 rows against e = 1100 columns in g = 7
groups (18 column tiles under the cap of 16 slices: 9 slices of 2).  Both metrics, d = 4 and 52, k = 1, 15, 64 where
there is a k.  The rows hold exact duplicates (zero distances, ties by index); the grouped modes run on three groups of
unequal size, once with the rows in runs and once shuffled (the wrappers sort and map the indices back)."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(a[k], b[k])]
    nans = sum(bool(torch.isnan(v).any()) for v in a.values() if v.is_floating_point())
    print(f"{len(a)} / {len(b)} entries, {sum(v.numel() for v in a.values())} values, {nans} entries with NaN, {len(bad)} differ")
    for k in bad:
        print("DIFFERS:", k)
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from ssl_wafermap_amd import cluster, manifold  # noqa: E402

out = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keep(tag, *tensors):
    for t, v in enumerate(tensors):
        # NaN marks the noise rows of the all-points core distance: a fixed pattern, compared as a number
        out[f"{tag}_{t}"] = torch.nan_to_num(v.cpu(), nan=-1.0) if v.is_floating_point() else v.cpu()


def rows(n, d, rng):
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[5:9] = x[4]  # exact duplicates: zero distances, ties resolved by the index
    x[n - 1] = x[0]
    x[n // 2] = x[n // 2 + 1]
    return x


def three_groups(n, rng):
    """Group ids of three groups of unequal size in runs, and the same multiset shuffled."""
    runs = np.repeat(np.arange(3), [n // 2, n // 3, n - n // 2 - n // 3]).astype(np.int64)
    return runs, rng.permutation(runs)


def square(x, n, metric, tag, rng):
    xd = dev(x)
    for k in (1, 15, 64):
        keep(f"core_{tag}_k{k}", cluster.core_distances(xd, k, metric))
        dist, idx = manifold.knn_graph(xd, k, metric)
        keep(f"knn_graph_{tag}_k{k}", dist, idx)
        keep(f"pair_dist_{tag}_k{k}", manifold.pair_distances(xd, xd, idx, metric))
        keep(f"rank_self_{tag}_k{k}", manifold.neighbor_ranks(xd, xd, idx, metric, exclude_self=True))
    core = cluster.core_distances(xd, 5, metric)
    comp = dev((np.arange(n) // 7).astype(np.int32))
    keep(f"min_edge_{tag}", *cluster.min_outgoing_edges(xd, core, comp, metric))
    keep(f"min_edge_alpha_{tag}", *cluster.min_outgoing_edges(xd, core, comp, metric, alpha=0.75))
    runs, mixed = three_groups(n, rng)
    keep(f"dist_sums_{tag}", cluster.cluster_distance_sums(xd, dev(runs.astype(np.int32)), 3, metric))
    for name, group in (("runs", runs), ("mixed", mixed)):
        labels = group.copy()
        labels[3::11] = -1  # noise rows
        keep(f"silhouette_{tag}_{name}", cluster.silhouette_samples(xd, labels, metric))
        keep(f"apcore_{tag}_{name}", cluster.allpoints_core_distances(xd, labels, None, metric),
             cluster.allpoints_core_distances(xd, labels, 50.0, metric))
        keep(f"min_edge_grouped_{tag}_{name}", *cluster.grouped_min_outgoing_edges(xd, core, comp, torch.from_numpy(group), 3, metric))
    return xd, core


def rectangular(xq, xd, core, n, metric, tag, rng):
    m = xq.shape[0]
    core_q = cluster.query_core_distances(xq, xd, 5, metric)
    for k in (1, 15, 64):
        dist, idx = manifold.knn_query(xq, xd, k, metric)
        keep(f"knn_query_{tag}_k{k}", dist, idx)
        far = dev(rng.integers(-1, n, (m, k)).astype(np.int32))  # any columns, -1 among them
        keep(f"pair_dist_q_{tag}_k{k}", manifold.pair_distances(xq, xd, far, metric))
        keep(f"rank_{tag}_k{k}", manifold.neighbor_ranks(xq, xd, idx, metric), manifold.neighbor_ranks(xq, xd, far, metric))
    keep(f"mreach_query_{tag}", *cluster.mreach_query(xq, core_q, xd, core, metric))
    keep(f"mreach_query_alpha_{tag}", *cluster.mreach_query(xq, core_q, xd, core, metric, alpha=0.75))
    runs, mixed = three_groups(n, rng)
    for name, group in (("runs", runs), ("mixed", mixed)):
        g = torch.from_numpy(group)
        keep(f"group_min_{tag}_{name}", *cluster.group_min_distances(xq, xd, g, 3, metric))
        keep(f"group_min_mreach_{tag}_{name}", *cluster.group_min_mreach(xq, core_q, xd, core, g, 3, metric))
    # a group without columns in the middle and at the end: ids 0 and 2 of 4
    sparse = torch.from_numpy(np.where(runs == 1, 2, runs))
    keep(f"group_min_{tag}_gaps", *cluster.group_min_distances(xq, xd, sparse, 4, metric))


for metric in ("euclidean", "manhattan"):
    for d in (4, 52):
        for n in (64, 65, 300) + ((4160,) if d == 4 else ()):
            rng = np.random.default_rng(1000 * d + n)
            tag = f"{metric[:3]}_d{d}_n{n}"
            x = rows(n, d, rng)
            xd, core = square(x, n, metric, tag, rng)
            # queries: 37 rows, some of them copies of fitted rows; at n = 4160 the fitted rows themselves as well
            q = rng.standard_normal((37, d)).astype(np.float32)
            q[:6] = x[:6]
            q[20] = q[21]
            rectangular(dev(q), xd, core, n, metric, tag + "_m37", rng)
            if n == 4160:
                rectangular(xd, xd, core, n, metric, tag + "_mn", rng)
        # group min under the cap on its slices: 9 rows against 1100 columns in 7 groups
        rng = np.random.default_rng(7000 + d)
        xe, xq = dev(rows(1100, d, rng)), dev(rng.standard_normal((9, d)).astype(np.float32))
        core_e, core_q = cluster.core_distances(xe, 5, metric), cluster.query_core_distances(xq, xe, 5, metric)
        runs = np.sort(rng.integers(0, 7, 1100))
        for name, group in (("runs", runs), ("mixed", rng.permutation(runs))):
            g = torch.from_numpy(group)
            tag = f"{metric[:3]}_d{d}_m9_e1100_{name}"
            keep(f"group_min_{tag}", *cluster.group_min_distances(xq, xe, g, 7, metric))
            keep(f"group_min_mreach_{tag}", *cluster.group_min_mreach(xq, core_q, xe, core_e, g, 7, metric))

torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print(f"saved {len(out)} entries to {sys.argv[1]}")
