"""Gaussian-mixture micro-benchmark (mixture.py; csrc/gmm.hip) on one MI355X, at k = 50 components on two matrices: the
golden 12 449 x 512 embeddings standardised and reduced by `decomposition.PCA(50)`, and a seeded synthetic 172 950 x 50.

    python tools/bench_gmm.py [--out profiles/gmm.md] [--reps 7] [--window 0.2] [--fit-iters 5] [--no-sklearn]

Per matrix, by direct calls of the entry points on preallocated buffers, one warm-up call, then --reps rounds of about
--window seconds of back-to-back calls with device events around a round; per call: median (min .. max) over the rounds:
the six kernels (logprob_diag, logprob_full, normalize, weighted_sums, scatter_diag, scatter_full), `wm_pca_project` at
m = d as the yardstick of logprob_full (which is k projections with half the K range plus an epilogue), the host
Cholesky step (`precision_cholesky` of k d x d matrices, wall clock) and a whole fit of --fit-iters iterations (tol = 0)
for diag and full, next to sklearn.mixture.GaussianMixture from the same initial parameters on the host's CPUs.  The
float64 MFMA rate of logprob_full and scatter_full is the flops their tiles EXECUTE (64 x 64 tiles, zeros included) over
the median time, against the data sheet's 78.6 TF.  Measurements to record; nothing here asserts a ratio.  What was not
run is listed as not measured."""
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
from ssl_wafermap_amd import _lib, decomposition, mixture  # noqa: E402
from ssl_wafermap_amd.retrieval import StandardScaler  # noqa: E402

DEV = torch.device("cuda:0")
F64_MATRIX_PEAK_TF = 78.6
K = 50


NOTE = ["## Reading the yardstick", "",
        "At d = 50 there is one column tile, so logprob_full executes per (row tile, component) the same 64 x 64 x 64 MFMA block as",
        "one `wm_pca_project` call does per row tile: the triangle of P_c saves nothing until d > 64 (column tile tn stops at K =",
        "64 tn + 64).  On top of a projection it fetches the component's means with the rows, squares the accumulators, folds each",
        "row's 32 lane sums through LDS and stores out[i][c] strided by k doubles, and its 156 registers allow 2 waves per SIMD",
        "where the projection has 3.  That accounts for a ratio somewhat above 1 on the large matrix; on the small one the 50",
        "projections are 50 launches of 195 workgroups each, which do not fill the 256 CUs, against one launch of 9 750.  Which",
        "of the named costs weighs most: not measured (no profiler trace, no counters).", ""]


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
    """K separated elliptical blobs, float32."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = 4.0 * torch.randn((K, d), generator=g, device=DEV)
    scales = 0.5 + torch.rand((K, d), generator=g, device=DEV)
    lab = torch.randint(0, K, (n,), generator=g, device=DEV)
    return (centres[lab] + scales[lab] * torch.randn((n, d), generator=g, device=DEV)).contiguous()


class Calls:
    """Preallocated operands of the six kernels on the rows x [n, d] at parameters taken from one M-step."""

    def __init__(self, x):
        lib = self.lib = _lib.load()
        self.xp, self.d = mixture._prep(x, "full")
        n, ld = self.xp.shape
        d, k = self.d, K
        self.n, self.ld = n, ld
        f64 = dict(dtype=torch.float64, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(1)
        lab = torch.randint(0, k, (n,), generator=g, device=DEV)
        resp = torch.full((n, k), 0.1 / k, **f64)
        resp[torch.arange(n, device=DEV), lab] += 0.9
        self.resp = resp.contiguous()
        _, means, cov = mixture._estimate(self.xp, d, self.resp, "full", 1e-6)
        self.mean = means
        self.cov = cov.cpu().numpy()
        self.pchol = torch.from_numpy(mixture.precision_cholesky(self.cov, "full")).to(DEV)
        self.inv_var = (1.0 / cov.diagonal(dim1=1, dim2=2)).contiguous()
        self.cst = torch.zeros(k, **f64)
        self.wlp = torch.empty((n, k), **f64)
        self.lpn, self.label, self.total = torch.empty(n, **f64), torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(1, **f64)
        self.nk, self.sx = torch.empty(k, **f64), torch.empty((k, d), **f64)
        self.sd, self.sf = torch.empty((k, d), **f64), torch.empty((k, d, d), **f64)
        self.w = torch.linalg.qr(torch.randn((ld, ld), **f64))[0].contiguous()
        self.y = torch.empty((n, ld), device=DEV)
        names = ["logprob_diag", "logprob_full", "weighted_sums", "scatter_diag", "scatter_full"]
        self.need = {m: getattr(lib, f"wm_gmm_{m}_workspace_bytes")(n, d, ld, k) for m in names}
        self.need["normalize"] = lib.wm_gmm_normalize_workspace_bytes(n, k)
        self.need["project"] = lib.wm_pca_project_workspace_bytes(n, ld, ld)
        self.ws = {m: torch.empty(v, dtype=torch.uint8, device=DEV) for m, v in self.need.items()}
        self.st = _lib.stream_ptr()

    def p(self, t):
        return t.data_ptr()

    def logprob_diag(self):
        _lib.check(self.lib.wm_gmm_logprob_diag(self.p(self.xp), self.n, self.d, self.ld, self.p(self.mean), self.p(self.inv_var),
                                                self.p(self.cst), K, self.p(self.wlp), self.p(self.ws["logprob_diag"]),
                                                self.need["logprob_diag"], self.st), "logprob_diag")

    def logprob_full(self):
        _lib.check(self.lib.wm_gmm_logprob_full(self.p(self.xp), self.n, self.d, self.ld, self.p(self.mean), self.p(self.pchol),
                                                self.p(self.cst), K, self.p(self.wlp), self.p(self.ws["logprob_full"]),
                                                self.need["logprob_full"], self.st), "logprob_full")

    def normalize(self):  # (on a buffer that holds log-probabilities the first time and responsibilities afterwards:
        # the same loads, exps and stores either way)
        _lib.check(self.lib.wm_gmm_normalize(self.p(self.wlp), self.n, K, self.p(self.lpn), self.p(self.label), self.p(self.total),
                                             self.p(self.ws["normalize"]), self.need["normalize"], self.st), "normalize")

    def weighted_sums(self):
        _lib.check(self.lib.wm_gmm_weighted_sums(self.p(self.xp), self.n, self.d, self.ld, self.p(self.resp), K, self.p(self.nk),
                                                 self.p(self.sx), self.p(self.ws["weighted_sums"]), self.need["weighted_sums"],
                                                 self.st), "weighted_sums")

    def scatter_diag(self):
        _lib.check(self.lib.wm_gmm_scatter_diag(self.p(self.xp), self.n, self.d, self.ld, self.p(self.resp), K, self.p(self.mean),
                                                self.p(self.sd), self.p(self.ws["scatter_diag"]), self.need["scatter_diag"],
                                                self.st), "scatter_diag")

    def scatter_full(self):
        _lib.check(self.lib.wm_gmm_scatter_full(self.p(self.xp), self.n, self.d, self.ld, self.p(self.resp), K, self.p(self.mean),
                                                self.p(self.sf), self.p(self.ws["scatter_full"]), self.need["scatter_full"],
                                                self.st), "scatter_full")

    def project(self):
        _lib.check(self.lib.wm_pca_project(self.p(self.xp), self.n, self.ld, 0, self.p(self.w), self.ld, self.p(self.y),
                                           self.p(self.ws["project"]), self.need["project"], self.st), "wm_pca_project")


def bench(name, x, a, lines):
    c = Calls(x)
    n, d, ld = c.n, c.d, c.ld
    fns = {"logprob_diag": c.logprob_diag, "logprob_full": c.logprob_full, "normalize": c.normalize,
           "weighted_sums": c.weighted_sums, "scatter_diag": c.scatter_diag, "scatter_full": c.scatter_full,
           f"wm_pca_project, m = d = {ld} (one call)": c.project}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    first = (c.sx.clone(), c.sd.clone(), c.sf.clone())
    inner = {m: max(3, int(a.window * 1e3 / max(timed(fn, 3), 1e-3))) for m, fn in fns.items()}
    times = {m: [] for m in fns}
    for _ in range(a.reps):
        for m, fn in fns.items():
            times[m].append(timed(fn, inner[m]))
    assert all(torch.equal(u, v) for u, v in zip(first, (c.sx, c.sd, c.sf))), "two calls must give the same bits"
    s = {m: summary(v) for m, v in times.items()}
    proj = s[f"wm_pca_project, m = d = {ld} (one call)"]
    t_col = -(-d // 64)
    row_tiles = -(-n // 64)
    k_exec = sum(-(-min(d, 64 * (tn + 1)) // 16) * 16 for tn in range(t_col))  # K per column tile, steps of 16
    flops_lp = 2.0 * 64 * 64 * k_exec * row_tiles * K
    tri = t_col * (t_col + 1) // 2
    flops_sc = 2.0 * 64 * 64 * n * tri * K  # (the slices' rows rounded up to 32 are not counted)
    tf_lp, tf_sc = flops_lp / s["logprob_full"][0] / 1e9, flops_sc / s["scatter_full"][0] / 1e9
    useful = float(n) * K * d * (d + 1)
    chol = wall(lambda: mixture.precision_cholesky(c.cov, "full"), a.reps)
    lines += [f"## {name}: {n} x {d}, k = {K}", "", "| kernel | per call |", "|---|---|"]
    lines += [f"| {m} | {fmt(v)} |" for m, v in s.items()]
    e_full, m_full = s["logprob_full"][0] + s["normalize"][0], s["weighted_sums"][0] + s["scatter_full"][0]
    e_diag, m_diag = s["logprob_diag"][0] + s["normalize"][0], s["weighted_sums"][0] + s["scatter_diag"][0]
    lines += [f"| host: `precision_cholesky` of {K} matrices {d} x {d} (scipy, wall clock) | {fmt(chol)} |", "",
              f"One iteration, kernels only: full {e_full + m_full:.3f} ms (E {e_full:.3f}, M {m_full:.3f}), diag "
              f"{e_diag + m_diag:.3f} ms (E {e_diag:.3f}, M {m_diag:.3f}).  The host Cholesky step is "
              f"{100 * chol[0] / (chol[0] + e_full + m_full):.0f} % of a full iteration's kernels plus itself (copies and "
              "synchronisations not counted here; the whole fit below has them).", "",
              f"logprob_full: {flops_lp / 1e9:.1f} GFLOP executed ({useful / 1e9:.1f} useful: the upper triangle) -> {tf_lp:.2f} TF = "
              f"{100 * tf_lp / F64_MATRIX_PEAK_TF:.1f} % of the float64 matrix peak ({F64_MATRIX_PEAK_TF} TF, data sheet).  "
              f"scatter_full: {flops_sc / 1e9:.1f} GFLOP executed ({useful / 1e9:.1f} useful: the lower triangle) -> {tf_sc:.2f} TF = "
              f"{100 * tf_sc / F64_MATRIX_PEAK_TF:.1f} %.", "",
              f"Yardstick: logprob_full / ({K} x wm_pca_project at m = d) = {s['logprob_full'][0] / (K * proj[0]):.2f}.", ""]
    rec = {"name": name, "n": n, "d": d, "ms": s, "cholesky_ms": chol, "logprob_full_tf": tf_lp, "scatter_full_tf": tf_sc,
           "ratio_to_projections": s["logprob_full"][0] / (K * proj[0])}
    # a whole fit of a fixed number of iterations, from the same initial parameters as sklearn's
    xh = c.xp[:, :d].cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(0)
    mu0 = xh[rng.choice(n, K, replace=False)]
    var = xh.var(0)
    for ct, prec in (("diag", np.tile(1.0 / var, (K, 1))), ("full", np.tile(np.diag(1.0 / var), (K, 1, 1)))):
        kw = dict(covariance_type=ct, tol=0.0, max_iter=a.fit_iters, weights_init=np.full(K, 1.0 / K), means_init=mu0,
                  precisions_init=prec)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ours = mixture.GaussianMixture(K, **kw).fit(x)  # warm-up
            fit = wall(lambda: mixture.GaussianMixture(K, **kw).fit(x), min(a.reps, 3))
            line = f"- `GaussianMixture({K}, \"{ct}\", tol=0, max_iter={a.fit_iters})`.fit, wall clock, {min(a.reps, 3)} runs: {fmt(fit)}"
            rec[f"fit_{ct}_ms"] = fit
            if a.no_sklearn:
                line += "; sklearn on the host: not measured (--no-sklearn)"
            else:
                from sklearn.mixture import GaussianMixture as Sk

                t0 = time.perf_counter()
                sk = Sk(K, **kw).fit(xh)
                t_sk = (time.perf_counter() - t0) * 1e3
                line += (f"; sklearn on the host's CPUs from the same parameters, float64, one run: {t_sk:.0f} ms, {t_sk / fit[0]:.1f} x; "
                         f"lower_bound_ {ours.lower_bound_:.12g} against {sk.lower_bound_:.12g}")
                rec[f"sklearn_{ct}_ms"] = t_sk
        lines.append(line)
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gmm.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--resources", default="", help="a file with the compiler's resource report of csrc/gmm.hip to include")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gmm.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    lines = ["# Gaussian mixture: the six kernels, the host Cholesky step and a whole fit", "",
             "Scope: `csrc/gmm.hip` and `mixture.GaussianMixture`.  One MI355X.  Written by `tools/bench_gmm.py`: direct calls of the",
             f"entry points on preallocated buffers, one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls",
             "each, device events around a round; per call: median (min .. max) over the rounds.  Per-kernel times from a profiler",
             "trace and hardware counters: not measured.", ""]
    if a.resources:
        lines += ["## Kernel resources (compiler report)", "", "```"] + Path(a.resources).read_text().splitlines() + ["```", ""]
    emb = torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV)
    golden = decomposition.PCA(50).fit_transform(StandardScaler().fit_transform(emb)).contiguous()
    recs = [bench("golden embeddings, standardised, PCA(50)", golden, a, lines)]
    recs.append(bench("synthetic, 50 blobs, seed 172950", synthetic(172950, 50, 172950), a, lines))
    lines += NOTE
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
