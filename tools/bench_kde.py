"""Gaussian log-sum micro-benchmark (density.py; csrc/kde.hip: wm_kde_logsum) on one MI355X, on the golden 12 449 x 512
embeddings (standardised), the same rows after PCA(50), and seeded synthetic 172 950 x 50 rows (32 Gaussian clusters).

    python tools/bench_kde.py [--out profiles/kde.md] [--reps 7] [--window 0.1] [--no-synthetic] [--no-sklearn]
                              [--trace DIR] [--parity FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/bench_kde.py --trace-child

Per matrix, by calls of `density.gaussian_log_sums` on a preallocated output and workspace (launches only, nothing read
back): the leave-one-out pass for one bandwidth and for four, next to `cluster.core_distances` at k = 1 (wm_core_distance:
the same pairs through the same tiling, with a k-list of one in place of the exponentials).  Each is timed on its own in
--reps rounds of about --window seconds of back-to-back calls (at least one call) with device events around a round; per
call: median (min .. max) over the rounds.  The bandwidths are 0.5, 1, 2 and 4 times the median distance to the nearest
neighbour (few terms survive at the first, most at the last; the kernel takes no shortcut for a term that underflows).
The merge kernel alone has no entry point of its own: its time comes from a kernel trace of `--trace-child` (three calls per
matrix and bandwidth count, in a run of its own under rocprofv3) given as --trace DIR; without one it is listed as not
measured.  A whole `KernelDensity(7 bandwidths).fit` + `loo_score_samples` on the golden rows: wall clock, median of --reps
runs.  sklearn.neighbors.KernelDensity (one bandwidth, its default tree, rtol = atol = 0) on this machine's CPUs on the first
2 000 golden rows, fit + score_samples of those rows, next to the same call here.  Measurements to record; nothing here
asserts a ratio.  --parity: the record of a run of tests/test_gpu_kde.py, whose worst fraction of every bound is written
next to the timings."""
import argparse
import collections
import csv
import glob
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests"))
import parity_log  # noqa: E402
from ssl_wafermap_amd import cluster, decomposition, density  # noqa: E402

DEV = torch.device("cuda:0")
FACTORS = [0.5, 1.0, 2.0, 4.0]
SEVEN = [0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0]


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def summary(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def rounds(fn, a):
    fn()  # warm-up
    inner = max(1, int(a.window * 1e3 / timed(fn, 1)))
    return summary([timed(fn, inner) for _ in range(a.reps)])


def golden():
    emb = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")["embeddings"].astype(np.float64)
    std = emb.std(axis=0)
    return torch.from_numpy(((emb - emb.mean(axis=0)) / np.where(std > 0, std, 1.0)).astype(np.float32)).to(DEV)


def synthetic(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = 4.0 * torch.randn((32, d), generator=g, device=DEV)
    which = torch.randint(0, 32, (n,), generator=g, device=DEV)
    return (centres[which] + torch.randn((n, d), generator=g, device=DEV)).contiguous()


def neighbour_scale(x):
    """The median distance to the nearest other row (the second column of the kNN graph), on at most 20 000 rows."""
    from ssl_wafermap_amd import manifold

    dist, _ = manifold.knn_graph(x[:20000].contiguous(), 2)
    return float(dist[:, 1].median())


def matrices(a, load=True):
    """(name, rows) of the matrices in the order they are measured; load=False: the names alone."""
    x = golden() if load else None
    yield "golden embeddings", x
    yield "golden embeddings after PCA(50)", decomposition.PCA(50).fit_transform(x).contiguous() if load else None
    if not a.no_synthetic:
        yield "synthetic, seed 172950", synthetic(172950, 50, 172950) if load else None


def buffers(x, b):
    n, d = x.shape
    dp = d + (-d) % 4
    need = density._lib.load().wm_kde_logsum_workspace_bytes(n, n, dp, min(b, density.MAX_BANDWIDTHS))
    return torch.empty((b, n), dtype=torch.float64, device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV)


def passes(name, x, a, lines):
    n, d = x.shape
    scale = neighbour_scale(x)
    hs = [f * scale for f in FACTORS]
    lines += [f"## {name}: {n} x {d}", "", f"Median distance to the nearest neighbour {scale:.4g}; bandwidths {', '.join(f'{f:g}' for f in FACTORS)} times that.",
              "", "| call | per call |", "|---|---|"]
    rec = {"name": name, "n": n, "d": d, "ms": {}}
    core = rounds(lambda: cluster.core_distances(x, 1), a)
    rec["ms"]["core_distances k=1"] = core
    lines.append(f"| `cluster.core_distances(x, 1)` (the same pairs, no exponential) | {fmt(core)} |")
    ones = []
    for h in hs:
        out, ws = buffers(x, 1)
        s = rounds(lambda: density.gaussian_log_sums(x, x, [h], self_offset=0, out=out, ws=ws), a)
        rec["ms"][f"B=1 h={h / scale:g}"] = s
        ones.append(s[0])
        lines.append(f"| leave-one-out pass, B = 1, h = {h / scale:g} x | {fmt(s)} |")
    out, ws = buffers(x, 4)
    four = rounds(lambda: density.gaussian_log_sums(x, x, hs, self_offset=0, out=out, ws=ws), a)
    rec["ms"]["B=4"] = four
    lines.append(f"| leave-one-out pass, B = 4 (all four in one launch) | {fmt(four)} |")
    mean1 = sum(ones) / len(ones)
    pairs = float(n) * n
    lines += ["", f"One bandwidth costs {mean1 / core[0]:.2f} x the core-distance call (the difference is {100 * (mean1 - core[0]) / mean1:.1f} % of the "
              f"pass); four in one launch cost {four[0] / mean1:.2f} x one and {four[0] / sum(ones):.2f} x the four single passes.  Per pair: "
              f"{1e9 * core[0] / pairs:.3f} ps core, {1e9 * mean1 / pairs:.3f} ps B = 1, {1e9 * four[0] / pairs:.3f} ps B = 4.", ""]
    print(json.dumps(rec), flush=True)
    return rec


def whole_fit(x, a, lines):
    scale = neighbour_scale(x)
    hs = [f * scale for f in SEVEN]
    lines += [f"## A whole fit and leave-one-out scores: golden rows, {len(hs)} bandwidths", "", "| path | wall clock |", "|---|---|"]
    run = lambda: density.KernelDensity(hs).fit(x).loo_log_likelihood()  # noqa: E731
    ll = run()
    out = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    rec = {"device": summary(out), "loo_log_likelihood": ll.tolist(), "factors": SEVEN}
    lines += [f"| `KernelDensity({len(hs)} bandwidths).fit(x).loo_log_likelihood()` (two launches of 4 + 3, copies to the host, sums) | {fmt(rec['device'])} |",
              "", f"Leave-one-out log-likelihood per bandwidth ({', '.join(f'{f:g}' for f in SEVEN)} x the neighbour distance): "
              f"{', '.join(f'{v:.6g}' for v in ll)}; the largest at {SEVEN[int(np.argmax(ll))]:g} x.", ""]
    print(json.dumps(rec), flush=True)
    return rec


def against_sklearn(x, a, lines):
    rows = 2000
    lines += [f"## sklearn on the host: the first {rows} golden rows, one bandwidth, fit + score_samples of those rows", "",
              "| path | wall clock |", "|---|---|"]
    xs = x[:rows].contiguous()
    h = neighbour_scale(xs)
    run = lambda: density.KernelDensity(h).fit(xs).score_samples(xs)  # noqa: E731
    got = run()
    out = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        out.append((time.perf_counter() - t0) * 1e3)
    rec = {"device": summary(out)}
    lines.append(f"| `density.KernelDensity(h).fit(x).score_samples(x)` (one launch, copy to the host) | {fmt(rec['device'])} |")
    if a.no_sklearn:
        lines.append("| sklearn KernelDensity on the host | not measured (--no-sklearn) |")
    else:
        from sklearn.neighbors import KernelDensity

        xh = xs.cpu().numpy().astype(np.float64)
        out = []
        for _ in range(min(a.reps, 3)):
            t0 = time.perf_counter()
            want = KernelDensity(bandwidth=h, rtol=0, atol=0).fit(xh).score_samples(xh)
            out.append((time.perf_counter() - t0) * 1e3)
        rec["sklearn"] = summary(out)
        rec["max_abs_diff"] = float(np.abs(got - want).max())
        lines.append(f"| sklearn `KernelDensity(bandwidth=h, rtol=0, atol=0).fit(x).score_samples(x)` on this host's CPUs (float64, "
                     f"{min(a.reps, 3)} runs) | {fmt(rec['sklearn'])} |")
        lines += ["", f"sklearn takes {rec['sklearn'][0] / rec['device'][0]:.0f} x the device call at this size (a size chosen for sklearn: the device call is one "
                  f"launch of {rec['device'][0]:.2f} ms with its copy, mostly overhead).  Largest absolute difference of the log "
                  f"densities {rec['max_abs_diff']:.2e} (float32 distances here, float64 and a tree's bounds there)."]
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def trace_child():
    """What the kernel trace records: three leave-one-out calls per matrix for one and for four bandwidths."""
    for _, x in matrices(argparse.Namespace(no_synthetic=False)):
        scale = neighbour_scale(x)
        for hs in ([scale], [f * scale for f in FACTORS]):
            out, ws = buffers(x, len(hs))
            for _ in range(3):
                density.gaussian_log_sums(x, x, hs, self_offset=0, out=out, ws=ws)
        torch.cuda.synchronize()


def trace_table(path, lines):
    lines += ["## The merge kernel alone (kernel trace of `--trace-child`, a run of its own)", ""]
    found = glob.glob(f"{path}/**/*_kernel_trace.csv", recursive=True) if path else []
    if not found:
        lines += ["not measured: no kernel trace was given (--trace)", ""]
        return
    # the child issues, per matrix, three B = 1 calls and then three B = 4 calls, each a kde_pairs and a kde_merge launch:
    # a kde_pairs<1> behind a kde_pairs<4> opens the next matrix; a merge belongs to the pairs launch before it
    names = [name for name, _ in matrices(argparse.Namespace(no_synthetic=False), load=False)]
    agg = collections.OrderedDict()
    block, last = 0, ""
    for r in sorted(csv.DictReader(open(found[0])), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        if "kde_" not in name:
            continue
        if "kde_merge" in name:
            kind = f"kde_merge behind {last}"
        else:
            kind = "kde_pairs<" + name.split("kde_pairs<")[-1].split(">")[0] + ">"
            block += int(kind == "kde_pairs<1>" and last == "kde_pairs<4>")
            last = kind
        key = (names[block] if block < len(names) else f"matrix {block}", kind, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))
        agg.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines += ["| matrix | kernel | grid (workgroups) | launches | median us (min .. max) |", "|---|---|---|---|---|"]
    for (matrix, kind, gx, gy), us in agg.items():
        if kind.startswith("kde_merge"):
            lines.append(f"| {matrix} | `{kind}` | {gx} | {len(us)} | {statistics.median(us):.1f} ({min(us):.1f} .. {max(us):.1f}) |")
    lines += ["", "`kde_merge` reads the slices' minima and sums ([slices][m] and [slices][b][m] doubles) and writes [b][m]: a thread per row, "
              "ceil(m / 256) workgroups.  Only the merge is taken from the trace: the `kde_pairs` launches of this run are three cold "
              "calls under the profiler, and their times are the event timings above, not the trace's.", ""]


def parity_table(path, lines):
    lines += ["## Worst measured fraction of each bound (tests/test_gpu_kde.py)", ""]
    p = Path(path)
    worst = {}
    if p.exists():
        for line in p.read_text().splitlines():
            r = json.loads(line)
            if r["name"].startswith("kde "):
                worst[r["name"]] = max(worst.get(r["name"], 0.0), r["measured"])
    if not worst:
        lines += [f"not measured: no record at {path}", ""]
        return
    lines += ["| comparison | measured / bound |", "|---|---|"] + [f"| {k} | {v:.3g} |" for k, v in worst.items()]
    lines += ["", "The bit-equality cases and the sentinel bytes are asserted as equalities and have no fraction.", ""]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kde.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--no-synthetic", action="store_true")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--trace", default="", help="the output directory of a rocprofv3 --kernel-trace run of --trace-child")
    ap.add_argument("--trace-child", action="store_true", help="issue the traced calls and exit")
    ap.add_argument("--parity", default=str(ROOT / parity_log._PATH), help="the record of a run of the GPU tests")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kde.py needs the GPU: nothing is measured without one")
    if a.trace_child:
        trace_child()
        return None
    lines = ["# Gaussian log-sums over all pairs: the pass, the merge and whole fits", "",
             "Scope: `csrc/kde.hip` (`wm_kde_logsum`: `kde_pairs`, `kde_merge`) and `density.KernelDensity`.  One MI355X.",
             "Written by `tools/bench_kde.py`: calls of `density.gaussian_log_sums` on a preallocated output and workspace (launches",
             f"only), one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls each (at least one call), device events",
             "around a round; per call: median (min .. max) over the rounds.  Whole fits: wall clock, median of the runs.", "",
             "Not measured: 811 457 rows; hardware counters; sklearn on the full matrices.", ""]
    recs = []
    x = None
    for name, m in matrices(a):
        x = m if x is None else x
        recs.append(passes(name, m, a, lines))
    if a.no_synthetic:
        lines += ["## synthetic 172 950 x 50", "", "not measured (--no-synthetic)", ""]
    torch.cuda.empty_cache()
    trace_table(a.trace, lines)
    recs.append(whole_fit(x, a, lines))
    recs.append(against_sklearn(x, a, lines))
    parity_table(a.parity, lines)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
