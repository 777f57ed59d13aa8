"""KMeans micro-benchmark (cluster.py KMeans / kmeans_step; csrc/kmeans.hip wm_kmeans_update; csrc/cluster.hip
wm_group_min_dist as the assignment pass) on the golden 12 449 x 512 embeddings, standardised, at k in {25, 50} and R in
{1, 10} restarts, on one MI355X.

    python tools/bench_kmeans.py [--out profiles/kmeans.md] [--reps 7] [--window 0.3] [--no-sklearn]

Per (k, R), on preallocated buffers by direct calls of the entry points:
  the assignment pass (wm_group_min_dist on the centres [R * k][d], group = restart) and the update (wm_kmeans_update), each
  timed on its own in alternating rounds of about --window seconds of back-to-back calls with device events around a round;
  per call: median (min .. max) over --reps rounds;
  for R = 10 the same two next to R calls with one restart each (the amortisation the restart layout buys);
  the update next to its algorithmic bytes: the rows read once per restart, R n d 4, plus the (column, distance) pairs and,
  with a previous assignment, its columns, R n 12 (the partial sums that the slabs write and the fold reads are the kernel's
  own traffic and are reported beside it, not counted as algorithmic).
A whole fit (k-means++ rows drawn here as `init`, tol 1e-4, max_iter 300) next to sklearn.cluster.KMeans from the same
`init` on the host (n_init = 1, algorithm "lloyd"; the host's own thread count), wall clock, both once after one warm-up of
the device path.  These are measurements to record; nothing here asserts a ratio."""
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

DEV = torch.device("cuda:0")


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


class Step:
    """Preallocated operands of one Lloyd iteration for R restarts: `assign()` and `update()` launch and return."""

    def __init__(self, x, centres):
        lib = self.lib = _lib.load()
        self.x, self.c = x, centres.contiguous()
        (n, d), (r, k, _) = x.shape, centres.shape
        self.n, self.d, self.r, self.k = n, d, r, k
        self.group = torch.arange(r, dtype=torch.int32, device=DEV).repeat_interleave(k).contiguous()
        self.dist = torch.empty((n, r), device=DEV)
        self.cols = torch.empty((n, r), dtype=torch.int32, device=DEV)
        self.prev = torch.zeros((n, r), dtype=torch.int32, device=DEV)
        self.need_a = lib.wm_group_min_dist_workspace_bytes(n, r * k, d, r)
        self.need_u = lib.wm_kmeans_update_workspace_bytes(n, d, k, r)
        self.ws_a = torch.empty(self.need_a, dtype=torch.uint8, device=DEV)
        self.ws_u = torch.empty(self.need_u, dtype=torch.uint8, device=DEV)
        self.new = torch.empty_like(self.c)
        self.counts = torch.empty((r, k), dtype=torch.int32, device=DEV)
        self.inertia = torch.empty(r, dtype=torch.float64, device=DEV)
        self.changed = torch.empty(r, dtype=torch.int32, device=DEV)
        self.shift2 = torch.empty(r, dtype=torch.float64, device=DEV)
        self.st = _lib.stream_ptr()

    def assign(self):
        _lib.check(self.lib.wm_group_min_dist(self.x.data_ptr(), self.n, self.c.data_ptr(), self.group.data_ptr(), self.r * self.k,
                                              self.d, 0, self.r, self.dist.data_ptr(), self.cols.data_ptr(), self.ws_a.data_ptr(),
                                              self.need_a, self.st), "wm_group_min_dist")

    def update(self):
        _lib.check(self.lib.wm_kmeans_update(self.x.data_ptr(), self.n, self.d, self.cols.data_ptr(), self.dist.data_ptr(),
                                             self.prev.data_ptr(), self.r, self.k, self.c.data_ptr(), self.new.data_ptr(),
                                             self.counts.data_ptr(), self.inertia.data_ptr(), self.changed.data_ptr(),
                                             self.shift2.data_ptr(), self.ws_u.data_ptr(), self.need_u, self.st), "wm_kmeans_update")


def bench_shape(x, k, r, reps, window, lines):
    n, d = x.shape
    rng = np.random.default_rng(100 * k + r)
    centres = torch.stack([x[torch.from_numpy(np.sort(rng.permutation(n)[:k])).to(DEV)] for _ in range(r)])
    many = Step(x, centres)
    singles = [Step(x, centres[q:q + 1]) for q in range(r)] if r > 1 else []
    fns = {"assign": many.assign, "update": many.update}
    if singles:
        fns["assign, R calls of one"] = lambda: [s.assign() for s in singles]
        fns["update, R calls of one"] = lambda: [s.update() for s in singles]
    for s in [many] + singles:
        s.assign()
        s.update()
    torch.cuda.synchronize()
    first = (many.new.clone(), many.inertia.clone())
    for q, s in enumerate(singles):
        assert torch.equal(s.new[0], many.new[q]) and torch.equal(s.inertia, many.inertia[q:q + 1]), "a restart alone: the same bits"
    inner = {name: max(5, int(window * 1e3 / timed(fn, 5))) for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(timed(fn, inner[name]))
    assert torch.equal(first[0], many.new) and torch.equal(first[1], many.inertia), "two calls must give the same bits"
    s = {name: summary(v) for name, v in times.items()}
    algo = r * n * d * 4 + r * n * 12
    shape = lib_shape(n, d, k)
    partial = r * shape * k * d * 8
    lines += [f"## k = {k}, R = {r}: {n} x {d} rows against {r * k} centres", "",
              "| pass | per call |", "|---|---|"]
    lines += [f"| {name} | {fmt(v)} |" for name, v in s.items()]
    lines += ["", f"Update: algorithmic bytes {algo / 1e6:.1f} MB (rows once per restart, the pairs and the previous columns) -> "
              f"{algo / s['update'][0] / 1e6:.1f} GB/s at the median; the kernel's own partial sums are {partial / 1e6:.1f} MB written and "
              f"read again ({shape} slabs); workspace {many.need_u / 2 ** 20:.1f} MiB.  Assignment: 3 n (R k) d = "
              f"{3.0 * n * r * k * d / 1e9:.2f} GFLOP -> {3.0 * n * r * k * d / s['assign'][0] / 1e9:.1f} TF (vector float32 peak 157.3)."]
    if singles:
        lines += [f"One call with R = {r} restarts against {r} calls with one: assignment {s['assign, R calls of one'][0] / s['assign'][0]:.2f} x, "
                  f"update {s['update, R calls of one'][0] / s['update'][0]:.2f} x the time of the one call."]
    lines.append("")
    rec = {"k": k, "R": r, "inner": inner, "ms": s, "algorithmic_bytes": algo, "partial_bytes": partial}
    print(json.dumps(rec), flush=True)
    return rec


def lib_shape(n, d, k):
    """The update's slab count, restated from csrc/kmeans.hip (km_shape) for the report."""
    chunks, tiles = -(-d // 64), -(-k // 96)
    want = max(1, min(-(-512 // (chunks * tiles)), -(-n // 64)))
    per = -(-n // want)
    return -(-n // per)


def bench_fit(x, k, with_sklearn, lines):
    n = x.shape[0]
    init = x[torch.from_numpy(cluster.kmeans_plusplus(x, k, random_state=k)[1]).to(DEV)].contiguous()
    cluster.KMeans(k, init=init, max_iter=2).fit(x)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = cluster.KMeans(k, init=init).fit(x)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    cluster.kmeans_plusplus(x, k, random_state=k)
    torch.cuda.synchronize()
    t_seed = time.perf_counter() - t0
    row = f"| {k} | {t_dev * 1e3:.1f} ms, {model.n_iter_} iterations, inertia {model.inertia_:.6g} | {t_seed * 1e3:.1f} ms |"
    rec = {"k": k, "fit_seconds": t_dev, "n_iter": model.n_iter_, "inertia": model.inertia_, "seed_seconds": t_seed}
    if with_sklearn:
        from sklearn.cluster import KMeans as SkKMeans

        xh, ih = x.cpu().numpy().astype(np.float64), init.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        sk = SkKMeans(k, init=ih, n_init=1, algorithm="lloyd").fit(xh)
        t_sk = time.perf_counter() - t0
        agree = float((sk.labels_ == model.labels_).mean())
        row += f" {t_sk * 1e3:.1f} ms, {sk.n_iter_} iterations, inertia {sk.inertia_:.6g} | {t_sk / t_dev:.1f} x | {agree:.4f} |"
        rec.update(sklearn_seconds=t_sk, sklearn_n_iter=int(sk.n_iter_), sklearn_inertia=float(sk.inertia_), label_agreement=agree)
    else:
        row += " not measured | | |"
    lines.append(row)
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kmeans.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    x = StandardScaler().fit_transform(torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV)).contiguous()
    lines = ["# KMeans: the assignment pass, the update, restarts together and a whole fit", "",
             "Scope: `csrc/kmeans.hip` (`wm_kmeans_update`: `km_partial`, `km_fold`, `km_finish`; `wm_kmeans_seed`) and the assignment",
             "pass `wm_group_min_dist` of `csrc/cluster.hip` on the centres of R restarts as R groups of k columns.  One MI355X.  Written",
             f"by `tools/bench_kmeans.py` on the standardised golden embeddings ({x.shape[0]} x {x.shape[1]}): direct calls of the entry",
             f"points on preallocated buffers, one warm-up call, then {a.reps} alternating rounds of about {a.window:g} s of back-to-back",
             "calls each, device events around a round; per call: median (min .. max) over the rounds.  Centres: k random rows per",
             "restart.  Per-kernel times from a profiler trace: not measured.", ""]
    recs = [bench_shape(x, k, r, a.reps, a.window, lines) for k in (25, 50) for r in (1, 10)]
    lines += ["## A whole fit next to sklearn on the host", "",
              "`cluster.KMeans(k, init=rows).fit` (tol 1e-4, max_iter 300; one host synchronisation per iteration for the stopping",
              "rule) against `sklearn.cluster.KMeans(k, init=the same rows, n_init=1, algorithm=\"lloyd\")` in float64 on the host's CPUs, wall",
              "clock, one run each after a warm-up of the device path; `init` = the rows `cluster.kmeans_plusplus` chose (its own time",
              "in the third column).  The label agreement is recorded, not promised: tests/test_gpu_kmeans.py says why.", "",
              "| k | device fit | k-means++ seeding | sklearn fit (host) | sklearn / device | label agreement |", "|---|---|---|---|---|---|"]
    fits = [bench_fit(x, k, not a.no_sklearn, lines) for k in (25, 50)]
    lines.append("")
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs, fits


if __name__ == "__main__":
    main()
