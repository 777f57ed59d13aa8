"""UMAP micro-benchmark (manifold.py; csrc/cluster.hip wm_knn_graph, csrc/umap.hip): the kNN graph, the fuzzy
simplicial set and the layout epochs at the golden 12 449 x 512 embeddings and at a synthetic 172 950 x 512 matrix
(the size of the reference's full WM-811K dump), on one MI355X.

    python tools/bench_umap.py [--out profiles/umap_bench.md] [--densmap-out FILE] [--transform-out FILE] [--reps 5]
                               [--sizes golden synthetic]

Device events around the Python calls, one warm-up call per shape, then --reps calls: median (min .. max).  The kNN
pass is set next to wm_core_distance on the same rows and k: both are one all-pairs pass of 3 n^2 d float32 operations
on the vector ALU (157.3 TF peak).  The layout is reported per epoch and as sampled edges per second (an edge
sample = one attraction and R negative samples, i.e. 1 + R row gathers).  Worst parity figures of the UMAP tests are
appended when the parity log of tests/parity_log.py exists (tests/test_gpu_umap.py writes into it).

With --densmap-out the DensMAP density phase (manifold.optimize_layout_densmap, wm_densmap_layout) is timed at the same
shapes and written to that file: 50 epochs that are all in the phase (dens_frac = 1) next to the same 50 epochs of the
plain layout from the same positions, per epoch, and the once-per-fit graph radii.

With --transform-out the semi-supervised fit and the transform of new rows (manifold.InductiveUMAP) are timed on the
golden rows and written to that file: `fit(x, y)` next to the plain `fit(x)`, and `transform(x)` of all rows split by
step (kNN query, memberships, start, layout: one launch for all epochs), in 2-D and 50-D.  The cost of an epoch inside
the launch is the difference to a call of ten times the epochs, which leaves the call's validation out."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ssl_wafermap_amd import cluster, manifold  # noqa: E402
from ssl_wafermap_amd.retrieval import StandardScaler  # noqa: E402

PEAK_F32_VALU = 157.3e12
DEV = torch.device("cuda:0")


def timed(fn, reps):
    """(median, min, max) milliseconds of fn() by device events after one warm-up call; and fn's last result."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return (statistics.median(ms), min(ms), max(ms)), out


def fmt(t):
    return f"{t[0]:.2f} ms ({t[1]:.2f} .. {t[2]:.2f})"


def synthetic(n, d, seed):
    """Seeded mixture of 38 Gaussians (the MixedWM38 class count), float32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = 4.0 * torch.randn(38, d, generator=g, device=DEV)
    which = torch.randint(0, 38, (n,), generator=g, device=DEV)
    return (centers[which] + torch.randn(n, d, generator=g, device=DEV)).contiguous()


def bench_density(name, dist, idx, w, reps, lines):
    """The density phase next to the plain epoch: epochs [0, 50) of n_epochs, all of them in the phase."""
    graph, dists = manifold.fuzzy_union(idx, w, dist)
    n = graph.shape[0]
    n_epochs, span = (700 if n <= 10000 else 400), 50
    q = manifold.sample_rates(graph.data)
    live = int((q.long() * n_epochs >= 65536).sum())
    a, b = manifold.find_ab_params(1.0, 0.1)
    t_ro, ro = timed(lambda: manifold.graph_radii(graph.indptr, graph.data, dists, q, n_epochs), reps)
    rad = manifold.standardize_radii(ro)
    lines += [f"## {name}: {n} vertices, {int(graph.indices.numel())} entries ({live} live at {n_epochs} epochs)", "",
              f"Graph radii (`wm_densmap_graph_radii`, once per fit): {fmt(t_ro)}.", "",
              f"| layout, epochs [0, {span}) of {n_epochs} | plain (`wm_umap_layout`) | per epoch | density phase (`wm_densmap_layout`, "
              "dens_frac = 1) | per epoch | phase / plain |", "|---|---|---|---|---|---|"]
    rec = {"shape": name, "n": n, "live": live, "graph_radii_ms": t_ro[0], "density": []}
    for dim in (2, 50):
        g = torch.Generator(device="cuda").manual_seed(dim)
        y0 = (10.0 * torch.rand(n, dim, generator=g, device=DEV)).contiguous()
        t_p, _ = timed(lambda: manifold.optimize_layout(y0, graph.indptr, graph.indices, q, a, b, n_epochs, 0, span), reps)
        t_d, _ = timed(lambda: manifold.optimize_layout_densmap(y0, graph.indptr, graph.indices, q, graph.data, rad, a, b, n_epochs, 0,
                                                                span, dens_lambda=1.0, dens_frac=1.0), reps)
        lines.append(f"| {dim}-D | {fmt(t_p)} | {t_p[0] / span * 1e3:.1f} us | {fmt(t_d)} | {t_d[0] / span * 1e3:.1f} us | "
                     f"{t_d[0] / t_p[0]:.2f} x |")
        rec["density"].append({"dim": dim, "epochs": span, "plain_ms": t_p[0], "phase_ms": t_d[0]})
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def bench_shape(name, x, k, reps, lines, dens_lines=None):
    n, d = x.shape
    flop = 3.0 * n * n * d
    t_knn, (dist, idx) = timed(lambda: manifold.knn_graph(x, k), reps)
    t_core, _ = timed(lambda: cluster.core_distances(x, k), reps)
    t_w, w = timed(lambda: manifold.smooth_knn(dist, idx)[2], reps)
    t_u, graph = timed(lambda: manifold.fuzzy_union(idx, w), reps)
    nnz = int(graph.indices.numel())
    deg = torch.diff(graph.indptr.long())
    q = manifold.sample_rates(graph.data)
    lines += [f"## {name}: {n} x {d}, k = {k}", "",
              f"Graph: {nnz} entries, degree {int(deg.min())} .. {int(deg.max())} (median {int(deg.median())}).", "",
              "| step | time | TF | share of 157.3 TF |", "|---|---|---|---|",
              f"| kNN graph with indices (`wm_knn_graph`) | {fmt(t_knn)} | {flop / t_knn[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / t_knn[0]:.2f} |",
              f"| core distance, same rows and k (`wm_core_distance`) | {fmt(t_core)} | {flop / t_core[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / t_core[0]:.2f} |",
              f"| rho, sigma, weights (`wm_umap_smooth_knn`) | {fmt(t_w)} | | |",
              f"| union to CSR (torch sort / unique / searchsorted) | {fmt(t_u)} | | |", "",
              f"kNN graph / core distance: {t_knn[0] / t_core[0]:.2f} x.", ""]
    rec = {"shape": name, "n": n, "d": d, "k": k, "nnz": nnz, "knn_ms": t_knn[0], "core_ms": t_core[0], "weights_ms": t_w[0],
           "union_ms": t_u[0], "layout": []}
    n_epochs = 500 if n <= 10000 else 200
    a, b = manifold.find_ab_params(1.0, 0.1)
    lines += ["| layout | epochs | time | per epoch | sampled edges | edge samples / s |", "|---|---|---|---|---|---|"]
    samples = int(((n_epochs * q.long()) >> 16).sum())
    for dim in (2, 50):
        g = torch.Generator(device="cuda").manual_seed(dim)
        y0 = (10.0 * torch.rand(n, dim, generator=g, device=DEV)).contiguous()
        t_l, _ = timed(lambda: manifold.optimize_layout(y0, graph.indptr, graph.indices, q, a, b, n_epochs), max(2, reps // 2))
        lines.append(f"| {dim}-D (`wm_umap_layout`) | {n_epochs} | {fmt(t_l)} | {t_l[0] / n_epochs * 1e3:.1f} us | {samples} | "
                     f"{samples / t_l[0] * 1e3:.3g} |")
        rec["layout"].append({"dim": dim, "epochs": n_epochs, "ms": t_l[0], "edge_samples": samples,
                              "edge_samples_per_s": samples / t_l[0] * 1e3})
    lines.append("")
    print(json.dumps(rec), flush=True)
    if dens_lines is not None:
        rec["densmap"] = bench_density(name, dist, idx, w, max(2, reps // 2), dens_lines)
    return rec


def bench_transform(name, x, labels, reps, lines):
    """fit(x, y) next to fit(x), and transform(x) by step, with init="random" (no host eigensolver in the timing)."""
    n, d = x.shape
    k = 15
    y = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    rec = {"shape": name, "n": n, "d": d, "k": k, "dims": []}
    t_g, (dist, idx) = timed(lambda: manifold.knn_graph(x, k), reps)
    t_q, (qd, qi) = timed(lambda: manifold.knn_query(x, x, k), reps)
    assert torch.equal(dist, qd) and torch.equal(idx, qi)
    graph = manifold.fuzzy_union(idx, manifold.smooth_knn(dist, idx)[2])
    t_i, _ = timed(lambda: manifold.label_intersect(graph, y, manifold.far_distance(0.5)), reps)
    t_w, w = timed(lambda: manifold.smooth_knn_query(qd)[1], reps)
    lines += [f"## {name}: {n} x {d}, k = {k}, all {n} rows labelled ({int(y.max()) + 1} classes)", "",
              "| step | time |", "|---|---|",
              f"| kNN graph (`wm_knn_graph`), for comparison | {fmt(t_g)} |",
              f"| kNN query of the same rows (`wm_knn_query`; equal to the graph in bits) | {fmt(t_q)} |",
              f"| memberships of the queries (`wm_umap_smooth_knn_query`) | {fmt(t_w)} |",
              f"| label intersection of the graph's {int(graph.indices.numel())} entries (`wm_umap_label_intersect`) | {fmt(t_i)} |", ""]
    rec.update(knn_graph_ms=t_g[0], knn_query_ms=t_q[0], memberships_ms=t_w[0], label_intersect_ms=t_i[0])
    lines += ["| components | `UMAP.fit(x)` | `InductiveUMAP.fit(x, y)` | start (torch, double) | transform layout (`wm_umap_transform_layout`) "
              "| epochs | per further epoch | `transform(x)` whole |", "|---|---|---|---|---|---|---|---|"]
    for dim in (2, 50):
        kw = dict(n_neighbors=k, n_components=dim, init="random", random_state=0)
        t_plain, _ = timed(lambda: manifold.UMAP(**kw).fit(x), max(2, reps // 2))
        t_sup, model = timed(lambda: manifold.InductiveUMAP(**kw).fit(x, y), max(2, reps // 2))
        t_s, start = timed(lambda: model.transform_init(qi, w), reps)
        q = manifold.sample_rates(w)
        epochs = model.transform_epochs(n)
        t_l, _ = timed(lambda: manifold.optimize_transform(start, model.embedding_, qi, q, model.a_, model.b_, epochs), reps)
        # the cost of an epoch inside the launch, without the call's validation: ten times the epochs against the above
        t_x, _ = timed(lambda: manifold.optimize_transform(start, model.embedding_, qi, q, model.a_, model.b_, 10 * epochs), reps)
        per_epoch = (t_x[0] - t_l[0]) / (9 * epochs)
        t_t, _ = timed(lambda: model.transform(x), reps)
        lines.append(f"| {dim} | {fmt(t_plain)} | {fmt(t_sup)} | {fmt(t_s)} | {fmt(t_l)} | {epochs} | {per_epoch * 1e3:.1f} us | {fmt(t_t)} |")
        rec["dims"].append({"dim": dim, "fit_ms": t_plain[0], "fit_y_ms": t_sup[0], "start_ms": t_s[0], "layout_ms": t_l[0],
                            "epochs": epochs, "per_further_epoch_us": per_epoch * 1e3, "transform_ms": t_t[0]})
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def parity_section(lines):
    sys.path.insert(0, str(ROOT / "tests"))
    from parity_log import _PATH  # (relative to the directory the tests ran from: the repository root)

    path = ROOT / _PATH
    if not path.exists():
        return
    worst = {}
    for ln in path.read_text().splitlines():
        r = json.loads(ln)
        if "test_gpu_umap" not in r.get("test", "") or r.get("generic"):
            continue
        key = r["name"].split(" n=")[0].split(" init=")[0]
        frac = (r["bound"] / r["measured"] if r["higher"] else r["measured"] / r["bound"]) if r["bound"] and r["measured"] else 0.0
        cur = worst.setdefault(key, {"count": 0, "frac": 0.0, "measured": None, "bound": None})
        cur["count"] += 1
        if frac >= cur["frac"]:
            cur.update(frac=frac, measured=r["measured"], bound=r["bound"])
    if worst:
        lines += ["## Parity (tests/test_gpu_umap.py, this run)", "",
                  "Worst comparison per check; the bounds are derived in the test module.", "",
                  "| check | comparisons | worst measured | its bound | fraction of the bound |", "|---|---|---|---|---|"]
        for key, c in worst.items():
            lines.append(f"| {key} | {c['count']} | {c['measured']:.6g} | {c['bound']:.6g} | {c['frac']:.3f} |")
        lines.append("")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "umap_bench.md"))
    ap.add_argument("--densmap-out", default="", help="also time the DensMAP density phase and write it to this file")
    ap.add_argument("--transform-out", default="", help="also time fit(x, y) and transform(x) on the golden rows and write them to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["golden", "synthetic"], choices=["golden", "synthetic"])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_umap.py needs the GPU: nothing is measured without one")
    lines = ["# UMAP: kNN graph, fuzzy simplicial set, layout", "",
             "Scope: `csrc/cluster.hip` (`wm_knn_graph`), `csrc/umap.hip` (`wm_umap_smooth_knn`, `wm_umap_layout`), `manifold.py`.",
             "One MI355X.  Written by `tools/bench_umap.py`: device events around the Python call (output allocation and the",
             "small merge kernel included), one warm-up call, then the median (min .. max) of the repeats.  One all-pairs",
             "pass is 3 n^2 d float32 operations; the share of peak is against the 157.3 TF vector rate.  Per-kernel times",
             "from a profiler trace: not measured.", ""]
    recs = []
    dens_lines = None
    if a.densmap_out:
        dens_lines = ["# DensMAP: the density phase next to the plain layout epoch", "",
                      "Scope: `csrc/umap.hip` (`wm_densmap_graph_radii`, `wm_densmap_layout`), `manifold.py`.  One MI355X.  Written by",
                      "`tools/bench_umap.py --densmap-out`: device events around the Python call (validation, workspace and output",
                      "allocation included), one warm-up call, then the median (min .. max) of the repeats.  A phase epoch is the",
                      "plain epoch plus one gather pass over all live entries in double, three small reduction launches and the",
                      "density term's 16-byte gather per sampled entry.", ""]
    if "golden" in a.sizes:
        z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
        emb = z["embeddings"].astype(np.float32)
        x = StandardScaler().fit_transform(torch.from_numpy(emb).to(DEV))
        if a.transform_out:
            tlines = ["# Semi-supervised fit and transform of new rows", "",
                      "Scope: `csrc/cluster.hip` (`wm_knn_query`), `csrc/umap.hip` (`wm_umap_label_intersect`, `wm_umap_smooth_knn_query`,",
                      "`wm_umap_transform_layout`), `manifold.py` (`InductiveUMAP`).  One MI355X.  Written by `tools/bench_umap.py",
                      "--transform-out`: device events around the Python call (validation and allocation included), one warm-up call,",
                      "then the median (min .. max) of the repeats; fits with `init=\"random\"`, default epochs.", ""]
            recs.append(bench_transform("golden SimSiam embeddings, standardised", x, np.asarray(z["labels"]), a.reps, tlines))
            tout = Path(a.transform_out)
            tout.parent.mkdir(parents=True, exist_ok=True)
            tout.write_text("\n".join(tlines) + "\n")
            print(f"wrote {tout}")
        recs.append(bench_shape("golden SimSiam embeddings, standardised", x, 15, a.reps, lines, dens_lines))
    if "synthetic" in a.sizes:
        recs.append(bench_shape("synthetic mixture of 38 Gaussians", synthetic(172950, 512, 0), 15, max(2, a.reps // 2), lines,
                                dens_lines))
    parity_section(lines)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    if dens_lines is not None:
        dout = Path(a.densmap_out)
        dout.parent.mkdir(parents=True, exist_ok=True)
        dout.write_text("\n".join(dens_lines) + "\n")
        print(f"wrote {dout}")
    return recs


if __name__ == "__main__":
    main()
