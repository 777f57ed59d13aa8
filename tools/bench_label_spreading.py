"""Label-spreading micro-benchmark (semi_supervised.LabelSpreading; csrc/propagate.hip: wm_lp_iterate) on one MI355X, on
two connectivity graphs at 15 neighbours without their diagonals: the golden 12 449 x 512 embeddings (standardised) and
seeded synthetic 172 950 x 64 rows (32 Gaussian clusters).

    python tools/bench_label_spreading.py [--out profiles/label_spreading.md] [--reps 7] [--window 0.1] [--no-synthetic]
                                          [--no-sklearn] [--parity FILE]

Per graph, on preallocated buffers by direct calls of the entry points: one step of wm_lp_iterate (its gather launch and
its residual merge) at C = 9 with one alpha and with 4 alphas (36 columns), for spreading and propagation, and 9 calls of
wm_spec_matvec on a basis of pitch 9, the work one step at C = 9 replaces.  Each is timed on its own in --reps rounds of
about --window seconds of back-to-back calls with device events around a round; per call: median (min .. max) over the
rounds.  A step next to its algorithmic bytes (indices and weights once, dinv, F read and F written once per row, the
gathered F rows counted as hits) as a share of the HBM peak of the data sheet (8 TB/s).  A whole fit (alpha 0.8, 10 % of
the golden labels, tol 1e-3, max_iter 200): wall clock, median of --reps runs, next to sklearn's LabelSpreading with a
callable kernel that returns the same graph on this machine's CPUs.  Measurements to record; nothing here asserts a ratio.
What was not run is listed as not measured.  --parity: the record of a run of tests/test_gpu_label_spreading.py
(the file tests/parity_log.py writes, the default), whose worst fraction of every bound is written next to the timings."""
import argparse
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests"))
import parity_log  # noqa: E402
from ssl_wafermap_amd import manifold, semi_supervised  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_TBS = 8.0
C = 9


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


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return summary(out)


def golden():
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    emb = z["embeddings"].astype(np.float64)
    std = emb.std(axis=0)
    x = torch.from_numpy(((emb - emb.mean(axis=0)) / np.where(std > 0, std, 1.0)).astype(np.float32)).to(DEV)
    return x, np.asarray(z["labels"]).astype(np.int64)


def synthetic(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = 4.0 * torch.randn((32, d), generator=g, device=DEV)
    which = torch.randint(0, 32, (n,), generator=g, device=DEV)
    return (centres[which] + torch.randn((n, d), generator=g, device=DEV)).contiguous(), (which % C).cpu().numpy()


def hide(truth, frac, seed):
    """Label codes 0 .. C - 1 with -1 on the rows a seeded draw hides."""
    keep = np.random.default_rng(seed).random(truth.shape[0]) < frac
    _, codes = np.unique(truth, return_inverse=True)
    return np.where(keep, codes, -1).astype(np.int32)


def steps(name, graph, labels_h, a, lines):
    """The per-call times of one step and of the 9 matvecs on `graph`."""
    n, nnz = graph.shape[0], int(graph.indices.numel())
    classes = int(labels_h.max()) + 1
    _, dinv = manifold.laplacian_degree(graph)
    labels = torch.from_numpy(labels_h).to(DEV)
    lines += [f"## {name}: {n} rows, {nnz} entries ({nnz / n:.1f} per row), {classes} classes, {(labels_h >= 0).sum()} labelled rows", "",
              "| call | per call |", "|---|---|"]
    rec = {"name": name, "n": n, "nnz": nnz, "ms": {}}
    fns = {}
    for groups in (1, 4):
        alpha = torch.linspace(0.2, 0.95, groups, dtype=torch.float64, device=DEV)
        active = torch.ones(groups, dtype=torch.int32, device=DEV)
        Fa = semi_supervised.label_matrix(labels, classes, groups)  # (validates the label codes, once)
        Fa += 0.01  # (no zero columns: every gathered value is live data)
        Fb = torch.empty_like(Fa)
        resid = torch.empty((1, groups), dtype=torch.float64, device=DEV)
        ws = semi_supervised.propagate_workspace(n, classes, groups, DEV)
        for hard in (False, True):
            key = f"one step, {'propagation' if hard else 'spreading'}, R x C = {groups} x {classes}"
            fns[key] = (lambda Fa=Fa, Fb=Fb, alpha=alpha, active=active, resid=resid, ws=ws, hard=hard:
                        semi_supervised.propagate(graph, dinv, labels, classes, alpha, active, Fa, Fb, 1, hard=hard, resid=resid,
                                                  checked=True, ws=ws), groups)  # (checked: no read-back, launches only)
    basis = torch.rand((n, classes), dtype=torch.float64, device=DEV)
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    token = manifold.token_workspace(DEV)

    def matvecs():
        for col in range(classes):
            manifold.laplacian_matvec(graph, dinv, basis, col, out=out, checked=True, ws=token)

    fns[f"{classes} calls of wm_spec_matvec on a basis of pitch {classes}"] = (matvecs, 0)
    for key, (fn, groups) in fns.items():
        fn()
        inner = max(3, int(a.window * 1e3 / timed(fn, 3)))
        s = summary([timed(fn, inner) for _ in range(a.reps)])
        rec["ms"][key] = s
        lines.append(f"| {key} | {fmt(s)} |")
        if groups:
            algo = nnz * 8 + n * (4 + 4 + 8) + 2 * n * groups * classes * 8
            lines.append(f"| ... its algorithmic bytes, {algo / 1e6:.2f} MB | {algo / s[0] / 1e9:.3f} TB/s = "
                         f"{100 * algo / s[0] / 1e9 / HBM_PEAK_TBS:.2f} % of the HBM peak ({HBM_PEAK_TBS} TB/s) |")
    one, nine = rec["ms"][f"one step, spreading, R x C = 1 x {classes}"][0], rec["ms"][f"{classes} calls of wm_spec_matvec on a basis of pitch {classes}"][0]
    four = rec["ms"][f"one step, spreading, R x C = 4 x {classes}"][0]
    lines += ["", f"One spreading step at C = {classes} takes {one / nine:.2f} x the {classes} matvecs it replaces"
              + (" (the step is SLOWER)" if one > nine else "") + f"; the step for 4 alphas takes {four / one:.2f} x the step for one.", ""]
    print(json.dumps(rec), flush=True)
    return rec


def whole_fit(x, truth, a, lines):
    """LabelSpreading.fit next to sklearn's on the same graph (golden rows, 15 neighbours, 10 % of the labels)."""
    y = hide(truth, 0.1, 0)
    graph = manifold.affinity_graph(x, 15, "euclidean", "connectivity")
    kw = dict(alpha=0.8, max_iter=200, tol=1e-3)
    lines += ["## A whole fit: golden rows, 15 neighbours, 10 % of the labels, alpha 0.8, tol 1e-3", "", "| path | wall clock |", "|---|---|"]
    rec = {}
    for every in (1, 8):
        fit = lambda: semi_supervised.LabelSpreading(affinity=graph, check_every=every, **kw).fit(x, y)  # noqa: E731
        model = fit()
        t = wall(fit, a.reps)
        rec[f"device_check_every_{every}"] = {"ms": t, "n_iter": int(model.n_iter_)}
        lines.append(f"| `LabelSpreading(affinity=graph, check_every={every}).fit` ({model.n_iter_} steps; degrees, label matrix, "
                     f"finalize and the copies to the host included) | {fmt(t)} |")
    full = lambda: semi_supervised.LabelSpreading(n_neighbors=15, affinity="connectivity", **kw).fit(x, y)  # noqa: E731
    full()
    t = wall(full, a.reps)
    rec["device_with_graph"] = {"ms": t}
    lines.append(f"| the same with the kNN graph built inside the fit (`affinity=\"connectivity\"`) | {fmt(t)} |")
    if a.no_sklearn:
        lines.append("| sklearn LabelSpreading on the host | not measured (--no-sklearn) |")
    else:
        from sklearn.semi_supervised import LabelSpreading

        g = manifold._without_diagonal(graph).to_scipy().astype(np.float64)
        xh = x.cpu().numpy().astype(np.float64)

        def sk_fit():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return LabelSpreading(kernel=lambda p, q=None: g, **kw).fit(xh, y)

        sk = sk_fit()
        out = []
        for _ in range(min(a.reps, 3)):
            t0 = time.perf_counter()
            sk_fit()
            out.append((time.perf_counter() - t0) * 1e3)
        ts = summary(out)
        model = semi_supervised.LabelSpreading(affinity=graph, check_every=1, **kw).fit(x, y)
        rec["sklearn"] = {"ms": ts, "n_iter": int(sk.n_iter_), "max_diff": float(np.abs(model.label_distributions_ - sk.label_distributions_).max()),
                          "labels_equal": float((model.transduction_ == sk.transduction_).mean())}
        lines.append(f"| sklearn `LabelSpreading(kernel=<callable returning the same graph>)` on this host's CPUs ({sk.n_iter_} steps, "
                     f"{min(a.reps, 3)} runs; the graph is given, not built) | {fmt(ts)} |")
        lines += ["", f"sklearn's fit takes {ts[0] / rec['device_check_every_8']['ms'][0]:.1f} x the device fit at check_every = 8 and "
                  f"{ts[0] / rec['device_check_every_1']['ms'][0]:.1f} x at check_every = 1.  At check_every = 1 the two agree: n_iter_ "
                  f"{model.n_iter_} and {sk.n_iter_}, largest difference of the distributions {rec['sklearn']['max_diff']:.2e}, "
                  f"{100 * rec['sklearn']['labels_equal']:.2f} % equal labels."]
    hidden = y < 0
    _, codes = np.unique(truth, return_inverse=True)
    lines += ["", f"Transductive accuracy on the {hidden.sum()} hidden rows: {(model.transduction_[hidden] == codes[hidden]).mean():.4f} "
              f"({int(model.unreached_.sum())} rows unreached).  No accuracy claim is made for the method.", ""]
    print(json.dumps(rec), flush=True)
    return rec


def parity_table(path, lines):
    lines += ["## Worst measured fraction of each bound (tests/test_gpu_label_spreading.py)", ""]
    p = Path(path)
    if not p.exists():
        lines += [f"not measured: no record at {path}", ""]
        return
    worst = {}
    for line in p.read_text().splitlines():
        r = json.loads(line)
        if r["name"].startswith("lp "):
            worst[r["name"]] = max(worst.get(r["name"], 0.0), r["measured"])
    lines += ["| comparison | measured / bound |", "|---|---|"] + [f"| {k} | {v:.3g} |" for k, v in worst.items()]
    lines += ["", "A fraction of 0 means equal bits: the restatement adds in the kernel's order and the kernels are compiled without",
              "floating-point contraction.  The exact cases (circulant graphs, finalize, frozen groups, a list of alphas against single",
              "fits) assert bit equality and have no fraction.", ""]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label_spreading.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--no-synthetic", action="store_true")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--parity", default=str(ROOT / parity_log._PATH), help="the record of a run of the GPU tests")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_spreading.py needs the GPU: nothing is measured without one")
    lines = ["# Label spreading: the step kernel and whole fits", "",
             "Scope: `csrc/propagate.hip` (`wm_lp_iterate`) and `semi_supervised.LabelSpreading`.  One MI355X.  Written by",
             "`tools/bench_label_spreading.py`: direct calls of the entry points on preallocated buffers, one warm-up call, then",
             f"{a.reps} rounds of about {a.window:g} s of back-to-back calls each, device events around a round; per call: median (min .. max)",
             "over the rounds.  Whole fits: wall clock, median of the runs.  One step = the gather launch and the residual merge launch.", "",
             "Not measured: 811 457 rows; hardware counters; a profiler trace (so no split between the gather and the merge).", ""]
    x, truth = golden()
    graph = manifold._without_diagonal(manifold.affinity_graph(x, 15, "euclidean", "connectivity"))
    recs = [steps("golden embeddings, 15 neighbours", graph, hide(truth, 0.1, 0), a, lines)]
    if a.no_synthetic:
        lines += ["## synthetic 172 950 rows", "", "not measured (--no-synthetic)", ""]
    else:
        xs, ts = synthetic(172950, 64, 172950)
        gs = manifold._without_diagonal(manifold.affinity_graph(xs, 15, "euclidean", "connectivity"))
        recs.append(steps("synthetic, seed 172950, 15 neighbours", gs, hide(ts, 0.1, 0), a, lines))
        del xs, gs
        torch.cuda.empty_cache()
    recs.append(whole_fit(x, truth, a, lines))
    parity_table(a.parity, lines)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
