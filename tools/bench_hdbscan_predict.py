"""HDBSCAN prediction micro-benchmark (cluster.py approximate_predict; csrc/cluster.hip wm_mreach_query): the pass that
finds, for m = 4096 new rows, the fitted row nearest in mutual reachability, next to wm_knn_query with k = min_samples at
the same shape, against the golden 12 449 x 512 embeddings and a synthetic 60 000 x 52 matrix, on one MI355X.

    python tools/bench_hdbscan_predict.py [--out profiles/hdbscan_predict.md] [--reps 9] [--inner 10] [--min-samples 26]
                                          [--resources FILE]

Both entry points are called directly on preallocated buffers (the small merge kernel included, no allocation).  One
warm-up call per shape and kernel, then --reps rounds in one process, every round timing --inner back-to-back calls of
the one and then of the other with device events (alternating, so that clock and neighbours act on both alike); reported
per call: median (min .. max) over the rounds.  Both are one all-pairs pass of 3 m n d float32 operations on the vector
ALU (157.3 TF peak); the kNN pass carries the heavier epilogue (a sorted k-list per row in LDS), so the new pass should
not exceed it by more than the kNN timing's own spread over the rounds, (max - min) / median.  --resources: the output of
tools/kernel_resources.py for csrc/cluster.hip, copied into the report."""
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


def synthetic(n, d, seed):
    """Seeded mixture of 38 Gaussians (the MixedWM38 class count), float32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = 4.0 * torch.randn(38, d, generator=g, device=DEV)
    which = torch.randint(0, 38, (n,), generator=g, device=DEV)
    return (centers[which] + torch.randn(n, d, generator=g, device=DEV)).contiguous()


def bench_shape(name, x, xq, k, reps, inner, lines):
    lib = _lib.load()
    (n, d), m = x.shape, xq.shape[0]
    st = _lib.stream_ptr()
    core = cluster.core_distances(x, k)
    core_q = cluster.query_core_distances(xq, x, k)
    w, dist = torch.empty(m, device=DEV), torch.empty(m, device=DEV)
    j = torch.empty(m, dtype=torch.int32, device=DEV)
    kd, ki = torch.empty((m, k), device=DEV), torch.empty((m, k), dtype=torch.int32, device=DEV)
    need_q, need_k = lib.wm_mreach_query_workspace_bytes(m, n, d), lib.wm_knn_query_workspace_bytes(m, n, d, k)
    ws_q = torch.empty(need_q, dtype=torch.uint8, device=DEV)
    ws_k = torch.empty(need_k, dtype=torch.uint8, device=DEV)

    def mreach():
        _lib.check(lib.wm_mreach_query(xq.data_ptr(), core_q.data_ptr(), m, x.data_ptr(), core.data_ptr(), n, d, 0, 1.0, w.data_ptr(),
                                       dist.data_ptr(), j.data_ptr(), ws_q.data_ptr(), need_q, st), "wm_mreach_query")

    def knn():
        _lib.check(lib.wm_knn_query(xq.data_ptr(), m, x.data_ptr(), n, d, 0, k, kd.data_ptr(), ki.data_ptr(), ws_k.data_ptr(), need_k,
                                    st), "wm_knn_query")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / inner

    mreach()
    knn()
    torch.cuda.synchronize()
    first = (w.clone(), dist.clone(), j.clone())
    t_q, t_k = [], []
    for _ in range(reps):
        t_q.append(timed(mreach))
        t_k.append(timed(knn))
    assert all(torch.equal(a, b) for a, b in zip(first, (w, dist, j))), "two calls must give the same bits"
    s_q, s_k = summary(t_q), summary(t_k)
    flop = 3.0 * m * n * d
    spread = (s_k[2] - s_k[1]) / s_k[0]
    ratio = s_q[0] / s_k[0]
    verdict = "within" if ratio <= 1.0 + spread else "ABOVE"
    lines += [f"## {name}: m = {m} new rows against {n} x {d}, min_samples = {k}", "",
              "| pass | per call | TF | share of 157.3 TF |", "|---|---|---|---|",
              f"| nearest in mutual reachability (`wm_mreach_query`) | {fmt(s_q)} | {flop / s_q[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / s_q[0]:.2f} |",
              f"| kNN query, k = {k} (`wm_knn_query`) | {fmt(s_k)} | {flop / s_k[0] / 1e9:.1f} | {flop / PEAK_F32_VALU * 1e3 / s_k[0]:.2f} |", "",
              f"`wm_mreach_query` / `wm_knn_query`: {ratio:.3f} x; the kNN timing's own spread over the {reps} rounds, (max - min) / median: "
              f"{spread:.3f}; the new pass is {verdict} the kNN pass plus that spread.", ""]
    rec = {"shape": name, "m": m, "n": n, "d": d, "k": k, "mreach_query_ms": s_q, "knn_query_ms": s_k, "ratio": ratio,
           "knn_spread": spread}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hdbscan_predict.md"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--min-samples", type=int, default=26, help="the notebook's chosen min_samples")
    ap.add_argument("--resources", default="", help="output of tools/kernel_resources.py for csrc/cluster.hip, copied into the report")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_hdbscan_predict.py needs the GPU: nothing is measured without one")
    lines = ["# HDBSCAN prediction for new rows: the mutual-reachability query pass", "",
             "Scope: `csrc/cluster.hip` (`wm_mreach_query`: the `CL_MREACHQ` mode of `cl_pairs` and `cl_mreach_query_merge`), next to",
             "`wm_knn_query` at the same shape.  One MI355X.  Written by `tools/bench_hdbscan_predict.py`: direct calls of the entry",
             f"points on preallocated buffers, one warm-up call, then {a.reps} alternating rounds of {a.inner} back-to-back calls each, device",
             "events around a round; per call: median (min .. max) over the rounds.  One pass is 3 m n d float32 operations; the",
             "share of peak is against the 157.3 TF vector rate.  Per-kernel times from a profiler trace: not measured.", ""]
    recs = []
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    x = StandardScaler().fit_transform(torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV))
    g = torch.Generator(device="cuda").manual_seed(1)
    pick = torch.randint(0, x.shape[0], (a.queries,), generator=g, device=DEV)
    xq = (x[pick] + 0.1 * torch.randn(a.queries, x.shape[1], generator=g, device=DEV)).contiguous()
    recs.append(bench_shape("golden SimSiam embeddings, standardised", x, xq, a.min_samples, a.reps, a.inner, lines))
    xs = synthetic(60000 + a.queries, 52, 0)
    recs.append(bench_shape("synthetic mixture of 38 Gaussians", xs[:60000].contiguous(), xs[60000:].contiguous(), a.min_samples,
                            a.reps, a.inner, lines))
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
