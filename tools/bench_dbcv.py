"""DBCV micro-benchmark (cluster.py validity_index; csrc/cluster.hip wm_allpoints_core, wm_mreach_min_edge_grouped,
wm_group_min_mreach): the three block-diagonal passes next to their square neighbours wm_core_distance and
wm_mreach_min_edge on the same rows, and validity_index end to end, on one MI355X.

    python tools/bench_dbcv.py [--out profiles/dbcv.md] [--reps 7] [--window 0.3]
                               [--min-cluster-size 75] [--min-samples 26] [--epsilon 1.5]

Rows: the golden SimSiam subset (12 449 x 512, standardised) under the labels of HDBSCAN(min_cluster_size, min_samples,
cluster_selection_epsilon) on it (the notebook's chosen trial), and two synthetic matrices of 12 449 x 52 and 12 449 x 512
(unit Gaussians around one centre per label) under the same label vector, so that the share of pairs that lie inside a
cluster, sum n_c^2 / n^2, is the same on all three.  Noise rows are dropped and the rest sorted by label, as validity_index
does.  The entry points are called directly on preallocated buffers (their small kernels included, no allocation): one
warm-up call, then --reps rounds, every round timing a window of back-to-back calls of each pass in turn with device events;
the number of calls per window is set from a first timing of 10 calls so that a window lasts about --window seconds;
reported per call: median (min .. max) over the rounds.  validity_index is timed as a whole with the host clock (it has host
work between its launches).  A square pass is 3 n^2 d float32 operations on the vector ALU (157.3 TF peak); a grouped one
does 3 d sum n_c^2 of them, and the expectation is a cost of about sum n_c^2 / n^2 of its square neighbour."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ssl_wafermap_amd import _lib, cluster  # noqa: E402
from ssl_wafermap_amd.retrieval import StandardScaler  # noqa: E402

PEAK_F32_VALU = 157.3e12
DEV = torch.device("cuda:0")


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def summary(ms):
    return statistics.median(ms), min(ms), max(ms)


def tile_share(group, rows):
    """The share of the n^2 pairs that a block-diagonal pass with `rows`-row tiles visits: per row tile the 64-column tiles
    from the first column of its first row's group to the last column of its last row's group."""
    n = group.shape[0]
    g = int(group.max()) + 1
    first, last = np.searchsorted(group, np.arange(g)), np.searchsorted(group, np.arange(g), side="right")
    visited = 0
    for i0 in range(0, n, rows):
        c0, c1 = first[group[i0]], last[group[min(i0 + rows, n) - 1]]
        visited += rows * 64 * (-(-c1 // 64) - c0 // 64)
    return visited / float(n) ** 2


def bench_rows(name, x, labels, k, reps, window, lines):
    """x [n, d] device rows, labels [n] numpy with -1 for noise."""
    lib = _lib.load()
    st = _lib.stream_ptr()
    t0 = time.perf_counter()
    score, parts = cluster.validity_index(x, labels, return_parts=True)  # (also the warm-up of every kernel below)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    rows, group = parts["rows"], parts["group"]
    xs = cluster._prep(x)[torch.from_numpy(rows).to(DEV)].contiguous()
    n, d = xs.shape
    g = int(group.max()) + 1
    sizes = np.bincount(group, minlength=g)
    share = float((sizes.astype(np.float64) ** 2).sum() / float(n) ** 2)
    share64, share128 = tile_share(group, 64), tile_share(group, 128)
    gd = torch.from_numpy(group.astype(np.int32)).to(DEV)
    core = torch.from_numpy(parts["core"]).to(DEV).float().contiguous()
    comp = torch.arange(n, dtype=torch.int32, device=DEV)
    at = torch.from_numpy(np.flatnonzero(parts["internal"])).to(DEV)
    xi, ci, gi = xs[at].contiguous(), core[at].contiguous(), gd[at].contiguous()
    mi = int(at.numel())
    out64 = torch.empty(n, dtype=torch.float64, device=DEV)
    ow, oj = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    gw, gj = torch.empty((mi, g), device=DEV), torch.empty((mi, g), dtype=torch.int32, device=DEV)
    need = {"apcore": lib.wm_allpoints_core_workspace_bytes(n, d, g), "edge_g": lib.wm_mreach_min_edge_grouped_workspace_bytes(n, d, g),
            "gmin": lib.wm_group_min_mreach_workspace_bytes(mi, mi, d, g), "core": lib.wm_core_distance_workspace_bytes(n, d, k),
            "edge": lib.wm_mreach_min_edge_workspace_bytes(n, d)}
    ws = {key: torch.empty(v, dtype=torch.uint8, device=DEV) for key, v in need.items()}
    p = float(x.shape[1])
    passes = {
        "apcore": lambda: _lib.check(lib.wm_allpoints_core(xs.data_ptr(), gd.data_ptr(), n, d, 0, g, p, out64.data_ptr(), ws["apcore"].data_ptr(),
                                                           need["apcore"], st), "wm_allpoints_core"),
        "core": lambda: _lib.check(lib.wm_core_distance(xs.data_ptr(), n, d, 0, k, ow.data_ptr(), ws["core"].data_ptr(), need["core"], st),
                                   "wm_core_distance"),
        "edge_g": lambda: _lib.check(lib.wm_mreach_min_edge_grouped(xs.data_ptr(), core.data_ptr(), comp.data_ptr(), gd.data_ptr(), n, d, 0, g,
                                                                    ow.data_ptr(), oj.data_ptr(), ws["edge_g"].data_ptr(), need["edge_g"], st),
                                     "wm_mreach_min_edge_grouped"),
        "edge": lambda: _lib.check(lib.wm_mreach_min_edge(xs.data_ptr(), core.data_ptr(), comp.data_ptr(), n, d, 0, 1.0, ow.data_ptr(),
                                                          oj.data_ptr(), ws["edge"].data_ptr(), need["edge"], st), "wm_mreach_min_edge"),
        "gmin": lambda: _lib.check(lib.wm_group_min_mreach(xi.data_ptr(), ci.data_ptr(), mi, xi.data_ptr(), ci.data_ptr(), gi.data_ptr(), mi, d,
                                                           0, g, gw.data_ptr(), gj.data_ptr(), ws["gmin"].data_ptr(), need["gmin"], st),
                                   "wm_group_min_mreach"),
    }

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / inner

    inner = {}
    for key, fn in passes.items():
        fn()
        torch.cuda.synchronize()
        inner[key] = max(10, int(window * 1e3 / timed(fn, 10)))
    times = {key: [] for key in passes}
    whole = []
    for _ in range(reps):
        for key, fn in passes.items():
            times[key].append(timed(fn, inner[key]))
        t0 = time.perf_counter()
        again = cluster.validity_index(x, labels)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
        assert again == score, "two runs must give the same bits"
    s = {key: summary(v) for key, v in times.items()}
    s_whole = summary(whole)
    sq, gr, rect = 3.0 * n * n * d, 3.0 * d * float((sizes.astype(np.float64) ** 2).sum()), 3.0 * mi * mi * d

    def row(label, key, flop):
        return f"| {label} | {fmt(s[key])} | {flop / s[key][0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / s[key][0]:.2f} |"

    r_core, r_edge = s["apcore"][0] / s["core"][0], s["edge_g"][0] / s["edge"][0]
    lines += [f"## {name}: n = {n} kept rows of {x.shape[0]} in g = {g} clusters (sizes {sizes.min()} .. {sizes.max()}), d = {d}, "
              f"{mi} internal rows; sum n_c^2 / n^2 = {share:.3f}; DBCV = {score:.4f}", "",
              "| pass | per call | TF (of the pairs it has to visit) | share of 157.3 TF |", "|---|---|---|---|",
              row("all-points core, grouped (`wm_allpoints_core`)", "apcore", gr),
              row(f"core distance, square, k = {k} (`wm_core_distance`)", "core", sq),
              row("one Boruvka round of every cluster's tree, singleton components (`wm_mreach_min_edge_grouped`)", "edge_g", gr),
              row("one Boruvka round, square, singleton components (`wm_mreach_min_edge`)", "edge", sq),
              row("separations, internal rows against internal rows (`wm_group_min_mreach`)", "gmin", rect), "",
              f"`validity_index` end to end ({parts['rounds']} Boruvka rounds, host work included): {fmt(s_whole)}; the first call: "
              f"{first_ms:.1f} ms.", "",
              f"Grouped / square: all-points core {r_core:.3f}, min edge {r_edge:.3f}, against sum n_c^2 / n^2 = {share:.3f} and against "
              f"the share of the pairs that the tiles cover, {share64:.3f} with the all-points core's 64-row tiles and {share128:.3f} with the "
              f"min edge's 128-row tiles "
              f"(the spread of the square timings over the {reps} rounds, (max - min) / median: core {(s['core'][2] - s['core'][1]) / s['core'][0]:.3f}, "
              f"min edge {(s['edge'][2] - s['edge'][1]) / s['edge'][0]:.3f}).", ""]
    rec = {"rows": name, "n": n, "d": d, "g": g, "internal": mi, "share": share, "tile_share_64": share64, "tile_share_128": share128, "dbcv": score, "inner": inner,
           **{f"{key}_ms": v for key, v in s.items()}, "validity_index_ms": s_whole, "rounds": parts["rounds"]}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dbcv.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--min-cluster-size", type=int, default=75)
    ap.add_argument("--min-samples", type=int, default=26)
    ap.add_argument("--epsilon", type=float, default=1.5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dbcv.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    x = StandardScaler().fit_transform(torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV)).contiguous()
    model = cluster.HDBSCAN(min_cluster_size=a.min_cluster_size, min_samples=a.min_samples, cluster_selection_epsilon=a.epsilon).fit(x)
    used = (a.min_cluster_size, a.epsilon)
    for used in ((a.min_cluster_size, a.epsilon), (40, 0.0), (15, 0.0)):  # (a labelling with at least two clusters)
        if model.refit(min_cluster_size=used[0], cluster_selection_epsilon=used[1]).labels_.max() >= 1:
            break
    labels = model.labels_
    if labels.max() < 1:
        raise SystemExit("the fit found fewer than two clusters: nothing to measure")
    lines = ["# DBCV cluster validity: the block-diagonal passes next to their square neighbours", "",
             "Scope: `csrc/cluster.hip` (`wm_allpoints_core`, `wm_mreach_min_edge_grouped`, `wm_group_min_mreach`: the `CL_APCORE`,",
             "`CL_MINEDGE_G` and `CL_GROUPMIN_MR` modes of `cl_pairs` with `cl_group_bounds` and `cl_apcore_merge`) and `cluster.validity_index`,",
             "next to `wm_core_distance` and `wm_mreach_min_edge` on the same rows.  One MI355X.  Written by `tools/bench_dbcv.py`: direct calls",
             f"of the entry points on preallocated buffers, one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls",
             "per pass, device events around a window; per call: median (min .. max) over the rounds.  The TF column counts 3 d float32",
             "operations per pair the pass has to visit (n^2 for a square pass, sum n_c^2 for a grouped one, m_i^2 for the separations); the",
             "share of peak is against the 157.3 TF vector rate.  Per-kernel times from a profiler trace: not measured.",
             f"Labels: HDBSCAN(min_cluster_size={used[0]}, min_samples={a.min_samples}, cluster_selection_epsilon={used[1]:g}) on the",
             f"standardised golden embeddings: {int(labels.max()) + 1} clusters, {int((labels == -1).sum())} of {x.shape[0]} rows noise; "
             f"relative_validity_ = {model.relative_validity_:.4f}.", ""]
    recs = [bench_rows("golden SimSiam subset", x, labels, a.min_samples, a.reps, a.window, lines)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    for d in (52, 512):
        centers = 6.0 * torch.randn(int(labels.max()) + 2, d, generator=gen, device=DEV)  # (the last one: the noise rows')
        xs = (centers[torch.from_numpy(labels).to(DEV)] + torch.randn(x.shape[0], d, generator=gen, device=DEV)).contiguous()
        recs.append(bench_rows(f"synthetic {x.shape[0]} x {d}", xs, labels, a.min_samples, a.reps, a.window, lines))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
