"""Local-outlier-factor micro-benchmark (neighbors.py; csrc/lof.hip: wm_lof_lrd, wm_lof_factor, wm_lof_indegree) on one
MI355X, on the golden 12 449 x 512 embeddings (standardised) and seeded synthetic 172 950 x 512 rows (32 Gaussian
clusters).

    python tools/bench_outliers.py [--out profiles/outliers.md] [--reps 7] [--window 0.1] [--no-synthetic] [--no-sklearn]
                                   [--parity FILE]

Per matrix, by calls of the functional layer on preallocated outputs and workspaces with `checked=True` (launches only,
nothing read back): the lrd pass, the LOF pass and the in-degree pass for one neighbour count (k = 20, lists of 20 columns)
and for a list of four (k = 10, 20, 30, 40, lists of 40 columns), each next to the `knn_graph` call whose lists it reads
(k + 1 columns: 21 and 41).  Each is timed on its own in --reps rounds of about --window seconds of back-to-back calls (at
least one call) with device events around a round; per call: median (min .. max) over the rounds.  A pass next to its
algorithmic bytes (the lists read once, the outputs written once, the gathered values counted as hits) as a share of the
HBM peak of the data sheet (8 TB/s).  A whole fit (LocalOutlierFactor(20).fit: graph, self-removal, three passes, copies to
the host) on the golden rows: wall clock, median of --reps runs, next to sklearn.neighbors.LocalOutlierFactor(20,
algorithm="brute") on this machine's CPUs.  Measurements to record; nothing here asserts a ratio.  What was not run is listed
as not measured.  --parity: the record of a run of tests/test_gpu_outliers.py (the file tests/parity_log.py writes, the
default), whose worst fraction of every bound is written next to the timings."""
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
sys.path.insert(1, str(ROOT / "tests"))
import parity_log  # noqa: E402
from ssl_wafermap_amd import manifold, neighbors  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_TBS = 8.0
ONE, FOUR = [20], [10, 20, 30, 40]


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


def passes(name, x, a, lines):
    """The per-call times of the three passes and of the graph calls on x."""
    n, d = x.shape
    lines += [f"## {name}: {n} x {d}", "", "| call | per call |", "|---|---|"]
    rec = {"name": name, "n": n, "d": d, "ms": {}}
    token = manifold.token_workspace(DEV)
    for ks in (ONE, FOUR):
        R, ld = len(ks), max(ks)
        tag = f"k = {ks[0]}" if R == 1 else f"k = {', '.join(map(str, ks))}"
        graph = rounds(lambda: manifold.knn_graph(x, ld + 1), a)
        rec["ms"][f"knn_graph, {ld + 1} columns"] = graph
        lines.append(f"| `knn_graph` at {ld + 1} columns (the lists of {tag}) | {fmt(graph)} |")
        dist, idx = neighbors.fitted_lists(x, ld)
        lrd = torch.empty((R, n), dtype=torch.float64, device=DEV)
        lof = torch.empty_like(lrd)
        deg = torch.empty((R, n), dtype=torch.int32, device=DEV)
        calls = {
            "lrd": (lambda: neighbors.local_reachability_density(dist, idx, dist, ks, out=lrd, checked=True, ws=token),
                    n * ld * 8 + R * n * 8),
            "LOF": (lambda: neighbors.local_outlier_factor(idx, lrd, lrd, ks, out=lof, checked=True, ws=token),
                    n * ld * 4 + 2 * R * n * 8),
            "in-degree": (lambda: neighbors.in_degree(idx, ks, out=deg, checked=True, ws=token), n * ld * 4 + 2 * R * n * 4),
        }
        total = 0.0
        for key, (fn, algo) in calls.items():
            s = rounds(fn, a)
            rec["ms"][f"{key}, {tag}"] = s
            total += s[0]
            lines.append(f"| {key} pass, {tag} ({algo / 1e6:.2f} MB algorithmic: {algo / s[0] / 1e9:.3f} TB/s = "
                         f"{100 * algo / s[0] / 1e9 / HBM_PEAK_TBS:.2f} % of the HBM peak) | {fmt(s)} |")
        lines.append(f"| ... the three passes together, {tag} | {total:.3f} ms = {100 * total / graph[0]:.2f} % of the graph call |")
    one = sum(rec["ms"][f"{key}, k = 20"][0] for key in ("lrd", "LOF", "in-degree"))
    four = sum(rec["ms"][f"{key}, k = 10, 20, 30, 40"][0] for key in ("lrd", "LOF", "in-degree"))
    lines += ["", f"The passes for four counts take {four / one:.2f} x the passes for one.  The in-degree pass issues one integer atomic per",
              "list entry below max(ks) and then adds the groups up in a second launch (counted in its time).", ""]
    print(json.dumps(rec), flush=True)
    return rec


def whole_fit(x, a, lines):
    lines += ["## A whole fit: golden rows, n_neighbors = 20", "", "| path | wall clock |", "|---|---|"]
    rec = {}
    fit = lambda: neighbors.LocalOutlierFactor(20).fit(x)  # noqa: E731
    model = fit()
    out = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    rec["device"] = summary(out)
    lines.append(f"| `neighbors.LocalOutlierFactor(20).fit` (graph, self-removal, three passes, copies to the host) | {fmt(rec['device'])} |")
    if a.no_sklearn:
        lines.append("| sklearn LocalOutlierFactor on the host | not measured (--no-sklearn) |")
    else:
        from sklearn.neighbors import LocalOutlierFactor

        xh = x.cpu().numpy().astype(np.float64)
        sk = LocalOutlierFactor(n_neighbors=20, algorithm="brute").fit(xh)
        out = []
        for _ in range(min(a.reps, 3)):
            t0 = time.perf_counter()
            LocalOutlierFactor(n_neighbors=20, algorithm="brute").fit(xh)
            out.append((time.perf_counter() - t0) * 1e3)
        rec["sklearn"] = summary(out)
        diff = float(np.max(np.abs(model.negative_outlier_factor_ - sk.negative_outlier_factor_) / np.abs(sk.negative_outlier_factor_)))
        agree = float(((model.negative_outlier_factor_ < -1.5) == (sk.negative_outlier_factor_ < -1.5)).mean())
        rec.update(max_rel_diff=diff, labels_equal=agree)
        lines.append(f"| sklearn `LocalOutlierFactor(20, algorithm=\"brute\").fit` on this host's CPUs (float64, {min(a.reps, 3)} runs) | "
                     f"{fmt(rec['sklearn'])} |")
        lines += ["", f"sklearn's fit takes {rec['sklearn'][0] / rec['device'][0]:.1f} x the device fit.  Largest relative difference of the scores "
                  f"{diff:.2e} (float32 distances here, float64 there; rows with near-tied k-th neighbours included), {100 * agree:.2f} % equal "
                  f"labels at the offset -1.5."]
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def parity_table(path, lines):
    lines += ["## Worst measured fraction of each bound (tests/test_gpu_outliers.py)", ""]
    p = Path(path)
    if not p.exists():
        lines += [f"not measured: no record at {path}", ""]
        return
    worst = {}
    for line in p.read_text().splitlines():
        r = json.loads(line)
        if r["name"].startswith("lof "):
            worst[r["name"]] = max(worst.get(r["name"], 0.0), r["measured"])
    lines += ["| comparison | measured / bound |", "|---|---|"] + [f"| {k} | {v:.3g} |" for k, v in worst.items()]
    lines += ["", "The in-degrees, the bit-equality cases and the sentinel columns are asserted as equalities and have no fraction.",
              "A fraction of 0 for lrd is no accident: up to 63 float32 values of similar magnitude add exactly in float64, so the",
              "kernel's tree and numpy's order give the same sum, and the three operations behind it are rounded alike.", ""]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "outliers.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--no-synthetic", action="store_true")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--parity", default=str(ROOT / parity_log._PATH), help="the record of a run of the GPU tests")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_outliers.py needs the GPU: nothing is measured without one")
    lines = ["# Local outlier factor: the three passes and whole fits", "",
             "Scope: `csrc/lof.hip` (`wm_lof_lrd`, `wm_lof_factor`, `wm_lof_indegree`) and `neighbors.LocalOutlierFactor`.  One MI355X.",
             "Written by `tools/bench_outliers.py`: calls of the functional layer on preallocated outputs (`checked=True`: launches",
             f"only), one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls each (at least one call), device events",
             "around a round; per call: median (min .. max) over the rounds.  Whole fits: wall clock, median of the runs.", "",
             "Not measured: 811 457 rows; hardware counters; a profiler trace; sklearn on the synthetic matrix.", ""]
    x = golden()
    recs = [passes("golden embeddings", x, a, lines)]
    if a.no_synthetic:
        lines += ["## synthetic 172 950 x 512", "", "not measured (--no-synthetic)", ""]
    else:
        xs = synthetic(172950, 512, 172950)
        recs.append(passes("synthetic, seed 172950", xs, a, lines))
        del xs
        torch.cuda.empty_cache()
    recs.append(whole_fit(x, a, lines))
    parity_table(a.parity, lines)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
