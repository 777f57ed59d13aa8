"""HDBSCAN soft-clustering micro-benchmark (cluster.py all_points_membership_vectors / membership_vector; csrc/cluster.hip
wm_group_min_dist): the pass that finds, for every row, the nearest exemplar of every cluster, next to wm_knn_query with
k = 1 over the same (m, e, d), on the golden 12 449 x 512 embeddings: all fitted rows, and a 1000-row hold-out, on one
MI355X.

    python tools/bench_hdbscan_soft.py [--out profiles/hdbscan_soft.md] [--reps 9] [--window 0.5] [--holdout 1000]
                                       [--min-cluster-size 30] [--min-samples 10] [--resources FILE]

The exemplars come from a fit of the standardised embeddings (HDBSCAN(min_cluster_size, min_samples)); the rows against
them are the fitted rows themselves and --holdout perturbed copies of random rows.  Both entry points are called directly
on preallocated buffers (their merge kernels included, no allocation).  One warm-up call per shape and kernel, then --reps
rounds in one process, every round timing a window of back-to-back calls of the one and then of the other with device
events (alternating, so that clock and neighbours act on both alike); the number of calls per window is set per shape from
a first timing of 10 calls so that a window lasts about --window seconds (a shorter one measures the clock and the
scheduler as much as the kernel); reported per call: median (min .. max) over the rounds.
Both are one rectangular pass of 3 m e d float32 operations on the vector ALU (157.3 TF peak) and both end in an
owner-thread scan of the 64-column distance tile in LDS, so the yardstick does the same pair work; the ratio of the two
is stated, and what the epilogue costs follows from it.  --resources: the output of tools/kernel_resources.py for
csrc/cluster.hip, copied into the report."""
import argparse
import json
import statistics
import sys
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


def bench_shape(name, xq, xe, group, g, reps, window, lines):
    lib = _lib.load()
    (m, d), e = xq.shape, xe.shape[0]
    st = _lib.stream_ptr()
    od, oj = torch.empty((m, g), device=DEV), torch.empty((m, g), dtype=torch.int32, device=DEV)
    kd, ki = torch.empty((m, 1), device=DEV), torch.empty((m, 1), dtype=torch.int32, device=DEV)
    need_g, need_k = lib.wm_group_min_dist_workspace_bytes(m, e, d, g), lib.wm_knn_query_workspace_bytes(m, e, d, 1)
    ws_g = torch.empty(need_g, dtype=torch.uint8, device=DEV)
    ws_k = torch.empty(need_k, dtype=torch.uint8, device=DEV)

    def group_min():
        _lib.check(lib.wm_group_min_dist(xq.data_ptr(), m, xe.data_ptr(), group.data_ptr(), e, d, 0, g, od.data_ptr(), oj.data_ptr(),
                                         ws_g.data_ptr(), need_g, st), "wm_group_min_dist")

    def knn():
        _lib.check(lib.wm_knn_query(xq.data_ptr(), m, xe.data_ptr(), e, d, 0, 1, kd.data_ptr(), ki.data_ptr(), ws_k.data_ptr(), need_k,
                                    st), "wm_knn_query")

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / inner

    group_min()
    knn()
    torch.cuda.synchronize()
    first = (od.clone(), oj.clone())
    assert torch.equal(od.min(dim=1).values, kd[:, 0]), "the nearest exemplar over all groups is the k = 1 neighbour, in bits"
    inner = max(10, int(window * 1e3 / max(timed(group_min, 10), timed(knn, 10))))
    t_g, t_k = [], []
    for _ in range(reps):
        t_g.append(timed(group_min, inner))
        t_k.append(timed(knn, inner))
    assert torch.equal(first[0], od) and torch.equal(first[1], oj), "two calls must give the same bits"
    s_g, s_k = summary(t_g), summary(t_k)
    flop = 3.0 * m * e * d
    spread = (s_k[2] - s_k[1]) / s_k[0]
    ratio = s_g[0] / s_k[0]
    lines += [f"## {name}: m = {m} rows against e = {e} exemplars in g = {g} groups, d = {d}; {inner} calls per window, workspace "
              f"{need_g / 2 ** 20:.1f} MiB allocated for a result of {m * g * 8 / 2 ** 20:.1f} MiB", "",
              "| pass | per call | TF | share of 157.3 TF |", "|---|---|---|---|",
              f"| nearest exemplar per cluster (`wm_group_min_dist`) | {fmt(s_g)} | {flop / s_g[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / s_g[0]:.2f} |",
              f"| kNN query, k = 1 (`wm_knn_query`) | {fmt(s_k)} | {flop / s_k[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / s_k[0]:.2f} |", "",
              f"`wm_group_min_dist` / `wm_knn_query`: {ratio:.3f} x ({(s_g[0] - s_k[0]) * 1e3:+.1f} us per call); the kNN timing's own spread "
              f"over the {reps} rounds, (max - min) / median: {spread:.3f}.", ""]
    rec = {"shape": name, "m": m, "e": e, "g": g, "d": d, "inner": inner, "workspace_bytes": need_g, "group_min_ms": s_g, "knn_query_ms": s_k, "ratio": ratio, "knn_spread": spread}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hdbscan_soft.md"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--holdout", type=int, default=1000)
    ap.add_argument("--min-cluster-size", type=int, default=30)
    ap.add_argument("--min-samples", type=int, default=10)
    ap.add_argument("--resources", default="", help="output of tools/kernel_resources.py for csrc/cluster.hip, copied into the report")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_hdbscan_soft.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    x = StandardScaler().fit_transform(torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV)).contiguous()
    model = cluster.HDBSCAN(min_cluster_size=a.min_cluster_size, min_samples=a.min_samples, prediction_data=True).fit(x)
    ex = model.exemplar_indices_
    if not ex:
        raise SystemExit("the fit found no cluster: nothing to measure")
    xe = x[torch.from_numpy(np.concatenate(ex)).to(DEV)].contiguous()
    group = torch.from_numpy(np.repeat(np.arange(len(ex)), [r.size for r in ex]).astype(np.int32)).to(DEV)
    lines = ["# HDBSCAN soft clustering: the nearest-exemplar-per-cluster pass", "",
             "Scope: `csrc/cluster.hip` (`wm_group_min_dist`: the `CL_GROUPMIN` mode of `cl_pairs` and `cl_group_min_merge`), next to",
             "`wm_knn_query` with k = 1 over the same (m, e, d).  One MI355X.  Written by `tools/bench_hdbscan_soft.py`: direct calls of",
             f"the entry points on preallocated buffers, one warm-up call, then {a.reps} alternating rounds of about {a.window:g} s of",
             "back-to-back calls each, device events around a round; per call: median (min .. max) over the rounds.  One pass is 3 m e d float32",
             "operations; the share of peak is against the 157.3 TF vector rate.  Per-kernel times from a profiler trace: not measured.",
             f"Exemplars: HDBSCAN(min_cluster_size={a.min_cluster_size}, min_samples={a.min_samples}) on the standardised golden embeddings:",
             f"{len(ex)} clusters, {xe.shape[0]} exemplars, {int((model.labels_ == -1).sum())} of {x.shape[0]} rows noise.", ""]
    recs = [bench_shape("all fitted rows", x, xe, group, len(ex), a.reps, a.window, lines)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    pick = torch.randint(0, x.shape[0], (a.holdout,), generator=gen, device=DEV)
    xq = (x[pick] + 0.1 * torch.randn(a.holdout, x.shape[1], generator=gen, device=DEV)).contiguous()
    recs.append(bench_shape("hold-out", xq, xe, group, len(ex), a.reps, a.window, lines))
    if a.resources:
        lines += ["## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; `tools/kernel_resources.py`)", "", "```"]
        lines += [ln for ln in Path(a.resources).read_text().splitlines() if "cl_" in ln]
        lines += ["```", ""]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
