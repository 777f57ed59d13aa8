"""PCA micro-benchmark (decomposition.py; csrc/pca.hip: wm_pca_mean, wm_pca_gram, wm_pca_project) on one MI355X, on
three matrices: the golden 12 449 x 512 embeddings and seeded synthetic 172 950 x 512 and 811 457 x 512 (a rank-32 signal
plus noise, float32).

    python tools/bench_pca.py [--out profiles/pca.md] [--reps 7] [--window 0.2] [--svd-max-rows 200000] [--no-sklearn]

Per matrix, on preallocated buffers by direct calls of the entry points: the mean, the Gram pass (centred) and the
projection onto 50 components, each timed on its own in --reps rounds of about --window seconds of back-to-back calls with
device events around a round; per call: median (min .. max) over the rounds.  The Gram pass next to the flops it executes
(the 64 x 64 tiles on and below the diagonal, 2 n 64 64 each) as a share of the float64 matrix peak of the data sheet
(78.6 TF), and next to its algorithmic bytes (the rows once, n d 4) as a share of the HBM peak (8 TB/s; 6.3 TB/s is what a
streaming copy reaches).  A whole `PCA(50).fit_transform` (wall clock, host eigendecomposition included, median of
--reps runs) next to the only PCA the tree had before, `manifold._pca_init` (torch.linalg.svd of the centred matrix in
float64; for matrices of at most --svd-max-rows rows) and `sklearn.decomposition.PCA(50, svd_solver="covariance_eigh")`
on the host in float64.  Measurements to record; nothing here asserts a ratio.  What was not run is listed as not
measured."""
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
from ssl_wafermap_amd import _lib, decomposition, manifold  # noqa: E402

DEV = torch.device("cuda:0")
F64_MATRIX_PEAK_TF, HBM_PEAK_TBS = 78.6, 8.0
M = 50


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


def synthetic(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    basis = torch.randn((32, d), generator=g, device=DEV) * torch.linspace(3.0, 0.1, 32, device=DEV)[:, None]
    x = torch.randn((n, 32), generator=g, device=DEV) @ basis
    x += 0.05 * torch.randn((n, d), generator=g, device=DEV) + torch.randn((d,), generator=g, device=DEV)
    return x.contiguous()


class Passes:
    """Preallocated operands of the three passes on x [n, d]."""

    def __init__(self, x):
        lib = self.lib = _lib.load()
        self.x = x
        n, d = self.n, self.d = x.shape
        self.mean = torch.empty(d, dtype=torch.float64, device=DEV)
        self.gram = torch.empty((d, d), dtype=torch.float64, device=DEV)
        self.w = torch.linalg.qr(torch.randn((d, M), dtype=torch.float64, device=DEV))[0].t().contiguous()
        self.y = torch.empty((n, M), device=DEV)
        self.need = {"mean": lib.wm_pca_mean_workspace_bytes(n, d), "gram": lib.wm_pca_gram_workspace_bytes(n, d),
                     "project": lib.wm_pca_project_workspace_bytes(n, d, M)}
        self.ws = {k: torch.empty(v, dtype=torch.uint8, device=DEV) for k, v in self.need.items()}
        self.st = _lib.stream_ptr()

    def run_mean(self):
        _lib.check(self.lib.wm_pca_mean(self.x.data_ptr(), self.n, self.d, self.mean.data_ptr(), self.ws["mean"].data_ptr(),
                                        self.need["mean"], self.st), "wm_pca_mean")

    def run_gram(self):
        _lib.check(self.lib.wm_pca_gram(self.x.data_ptr(), self.n, self.d, self.mean.data_ptr(), self.gram.data_ptr(),
                                        self.ws["gram"].data_ptr(), self.need["gram"], self.st), "wm_pca_gram")

    def run_project(self):
        _lib.check(self.lib.wm_pca_project(self.x.data_ptr(), self.n, self.d, self.mean.data_ptr(), self.w.data_ptr(), M,
                                           self.y.data_ptr(), self.ws["project"].data_ptr(), self.need["project"], self.st),
                   "wm_pca_project")


def bench(name, x, a, lines):
    n, d = x.shape
    p = Passes(x)
    fns = {"mean": p.run_mean, "gram": p.run_gram, "project (50 components)": p.run_project}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    first = (p.mean.clone(), p.gram.clone(), p.y.clone())
    inner = {k: max(3, int(a.window * 1e3 / timed(fn, 3))) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            times[k].append(timed(fn, inner[k]))
    assert all(torch.equal(u, v) for u, v in zip(first, (p.mean, p.gram, p.y))), "two calls must give the same bits"
    s = {k: summary(v) for k, v in times.items()}
    tiles = -(-d // 64) * (-(-d // 64) + 1) // 2
    flops = 2.0 * n * 64 * 64 * tiles
    tf = flops / s["gram"][0] / 1e9
    bytes_algo, bytes_read = n * d * 4, tiles * 2 * n * 64 * 4
    model = decomposition.PCA(M)
    model.fit_transform(x)  # warm-up
    fit = wall(lambda: decomposition.PCA(M).fit_transform(x), a.reps)
    lines += [f"## {name}: {n} x {d}", "", "| pass | per call |", "|---|---|"]
    lines += [f"| {k} | {fmt(v)} |" for k, v in s.items()]
    lines += [f"| `PCA({M}).fit_transform`, wall clock with the host eigendecomposition | {fmt(fit)} |", "",
              f"Gram: {tiles} tiles on or below the diagonal, {flops / 1e9:.1f} GFLOP executed -> {tf:.2f} TF at the median = "
              f"{100 * tf / F64_MATRIX_PEAK_TF:.1f} % of the float64 matrix peak ({F64_MATRIX_PEAK_TF} TF, data sheet); algorithmic bytes "
              f"{bytes_algo / 1e6:.1f} MB (the rows once) -> {bytes_algo / s['gram'][0] / 1e9:.3f} TB/s = "
              f"{100 * bytes_algo / s['gram'][0] / 1e9 / HBM_PEAK_TBS:.1f} % of the HBM peak ({HBM_PEAK_TBS} TB/s); the tiles themselves "
              f"request {bytes_read / 1e6:.1f} MB (two 64-column panels per tile, mostly from L2); workspace "
              f"{p.need['gram'] / 2 ** 20:.1f} MiB.  Mean: {bytes_algo / s['mean'][0] / 1e9:.3f} TB/s of the rows.  Project: "
              f"{(bytes_algo + n * M * 4) / s['project (50 components)'][0] / 1e9:.3f} TB/s of rows read and outputs written.", ""]
    rec = {"name": name, "n": n, "d": d, "ms": s, "fit_transform_ms": fit, "gram_tf": tf, "inner": inner}
    cmp_lines = []
    if n <= a.svd_max_rows:
        manifold._pca_init(x, M)  # warm-up
        svd = wall(lambda: manifold._pca_init(x, M), min(a.reps, 3))
        cmp_lines.append(f"`manifold._pca_init` (torch.linalg.svd, float64, {min(a.reps, 3)} runs): {fmt(svd)}, {svd[0] / fit[0]:.1f} x the fit_transform")
        rec["svd_ms"] = svd
    else:
        cmp_lines.append(f"`manifold._pca_init` (torch.linalg.svd, float64): not measured (above --svd-max-rows {a.svd_max_rows})")
    if not a.no_sklearn:
        from sklearn.decomposition import PCA as SkPCA

        xh = x.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        sk = SkPCA(M, svd_solver="covariance_eigh").fit(xh)
        yh = sk.transform(xh)
        t_sk = (time.perf_counter() - t0) * 1e3
        ev = np.abs(model.explained_variance_ / sk.explained_variance_ - 1).max()
        cmp_lines.append(f"`sklearn PCA({M}, svd_solver=\"covariance_eigh\")` fit + transform on the host, float64, one run: {t_sk:.1f} ms, "
                         f"{t_sk / fit[0]:.1f} x the fit_transform; largest relative difference of explained_variance_: {ev:.2e}")
        rec.update(sklearn_ms=t_sk, explained_variance_rel=float(ev))
        del xh, yh
    else:
        cmp_lines.append("sklearn on the host: not measured (--no-sklearn)")
    lines += [f"- {c}" for c in cmp_lines] + [""]
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pca.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--svd-max-rows", type=int, default=200000)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--resources", default="", help="a file with the output of tools/kernel_resources.py for csrc/pca.hip to include")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    lines = ["# PCA: the mean, the Gram pass, the projection and a whole fit", "",
             "Scope: `csrc/pca.hip` (`wm_pca_mean`, `wm_pca_gram`, `wm_pca_project`; `pca_tile` on `v_mfma_f64_16x16x4_f64`) and",
             "`decomposition.PCA`.  One MI355X.  Written by `tools/bench_pca.py`: direct calls of the entry points on preallocated",
             f"buffers, one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls each, device events around a",
             "round; per call: median (min .. max) over the rounds.  Per-kernel times from a profiler trace and hardware counters: not",
             "measured.", ""]
    if a.resources:
        lines += ["## Kernel resources (`tools/kernel_resources.py csrc/pca.hip`)", "", "```"] + Path(a.resources).read_text().splitlines() + ["```", ""]
    recs = [bench("golden embeddings", torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV).contiguous(), a, lines)]
    for n in (172950, 811457):
        recs.append(bench(f"synthetic, seed {n}", synthetic(n, 512, n), a, lines))
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
