"""Logistic-regression micro-benchmark (linear_model.py; csrc/logreg.hip) on one MI355X, K = 9 classes, for 1 and 4 values
of C, on two matrices: the golden 12 449 x 512 embeddings standardised, and a seeded synthetic 172 950 x 512.

    python tools/bench_logreg.py [--out profiles/logreg.md] [--reps 7] [--window 0.2] [--no-sklearn] [--sklearn-max-iter 300]

tools/bench_gmm.py's method: direct calls of the entry points on preallocated buffers, one warm-up call, then --reps
rounds of about --window seconds of back-to-back calls with device events around a round; per call: median (min .. max)
over the rounds.  Per matrix and number of C: the two kernels of one evaluation (wm_logreg_residual,
wm_logreg_gradient), and at equal sizes the two products it consists of, `wm_pca_project` (m = the columns) and
`wm_gmm_weighted_sums` (k = the columns).  The float64 MFMA rate is the flops the tiles EXECUTE (64 x 64 tiles, zeros
included) over the median time, against the data sheet's 78.6 TF.  On the golden matrix a whole fit (wall clock) next to
sklearn.linear_model.LogisticRegression(solver="lbfgs") on the host's CPUs at the same C, tol and iteration cap, and next
to `evals.fit_linear_probe` (10 epochs of Adam; wall clock only: it solves another problem to another end).
Measurements to record; nothing here asserts a ratio.  What was not run is listed as not measured."""
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
from ssl_wafermap_amd import _lib, linear_model  # noqa: E402
from ssl_wafermap_amd.retrieval import StandardScaler  # noqa: E402

DEV = torch.device("cuda:0")
F64_MATRIX_PEAK_TF = 78.6
K = 9


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


def synthetic(n, d, seed):
    """K overlapping blobs, float32, and their labels."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = 0.3 * torch.randn((K, d), generator=g, device=DEV)
    lab = torch.randint(0, K, (n,), generator=g, device=DEV)
    return (centres[lab] + torch.randn((n, d), generator=g, device=DEV)).contiguous(), lab.to(torch.int32)


class Calls:
    """Preallocated operands of one evaluation of `groups` softmax problems of K classes on the rows x [n, d]."""

    def __init__(self, x, y, groups):
        lib = self.lib = _lib.load()
        self.xp, self.d = linear_model._prep(x)
        self.n, self.ld = self.xp.shape
        n, d, ld = self.n, self.d, self.ld
        self.cols = cols = groups * K
        f64 = dict(dtype=torch.float64, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(2)
        self.w = (0.05 * torch.randn((cols, d + 1), generator=g, **f64)).contiguous()
        self.y = y.contiguous()
        self.resid, self.loss, self.grad = torch.empty((n, cols), **f64), torch.empty(groups, **f64), torch.empty((cols, d + 1), **f64)
        self.nk, self.sx = torch.empty(cols, **f64), torch.empty((cols, d), **f64)
        self.wp = self.w[:, :d].contiguous() if ld == d else torch.nn.functional.pad(self.w[:, :d], (0, ld - d)).contiguous()
        self.proj = torch.empty((n, cols), device=DEV)
        self.need = {"residual": lib.wm_logreg_residual_workspace_bytes(n, d, ld, cols, 0, K),
                     "gradient": lib.wm_logreg_gradient_workspace_bytes(n, d, ld, cols),
                     "weighted_sums": lib.wm_gmm_weighted_sums_workspace_bytes(n, d, ld, cols),
                     "project": lib.wm_pca_project_workspace_bytes(n, ld, cols)}
        self.ws = {m: torch.empty(v, dtype=torch.uint8, device=DEV) for m, v in self.need.items()}
        self.st = _lib.stream_ptr()

    @staticmethod
    def p(t):
        return t.data_ptr()

    def residual(self):
        _lib.check(self.lib.wm_logreg_residual(self.p(self.xp), self.n, self.d, self.ld, self.p(self.w), self.cols, 0, K, self.p(self.y),
                                               0, 0, self.p(self.resid), self.p(self.loss), 0, self.p(self.ws["residual"]),
                                               self.need["residual"], self.st), "wm_logreg_residual")

    def gradient(self):
        _lib.check(self.lib.wm_logreg_gradient(self.p(self.xp), self.n, self.d, self.ld, self.p(self.resid), self.cols,
                                               self.p(self.grad), self.p(self.ws["gradient"]), self.need["gradient"], self.st),
                   "wm_logreg_gradient")

    def weighted_sums(self):
        _lib.check(self.lib.wm_gmm_weighted_sums(self.p(self.xp), self.n, self.d, self.ld, self.p(self.resid), self.cols,
                                                 self.p(self.nk), self.p(self.sx), self.p(self.ws["weighted_sums"]),
                                                 self.need["weighted_sums"], self.st), "wm_gmm_weighted_sums")

    def project(self):
        _lib.check(self.lib.wm_pca_project(self.p(self.xp), self.n, self.ld, 0, self.p(self.wp), self.cols, self.p(self.proj),
                                           self.p(self.ws["project"]), self.need["project"], self.st), "wm_pca_project")


def bench_kernels(name, x, y, groups, a, lines):
    c = Calls(x, y, groups)
    n, d, cols = c.n, c.d, c.cols
    fns = {"wm_logreg_residual": c.residual, "wm_logreg_gradient": c.gradient,
           f"wm_pca_project, m = {cols}": c.project, f"wm_gmm_weighted_sums, k = {cols}": c.weighted_sums}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    first = (c.resid.clone(), c.loss.clone(), c.grad.clone())
    inner = {m: max(3, int(a.window * 1e3 / max(timed(fn, 3), 1e-3))) for m, fn in fns.items()}
    times = {m: [] for m in fns}
    for _ in range(a.reps):
        for m, fn in fns.items():
            times[m].append(timed(fn, inner[m]))
    assert all(torch.equal(u, v) for u, v in zip(first, (c.resid, c.loss, c.grad))), "two calls must give the same bits"
    assert torch.equal(c.grad[:, :d], c.sx) and torch.equal(c.grad[:, d], c.nk), "the gradient is the weighted sums' path"
    s = {m: summary(v) for m, v in times.items()}
    col_tiles, row_tiles = -(-cols // 64), -(-n // 64)
    flops_res = 2.0 * 64 * 64 * (-(-d // 16) * 16) * row_tiles * col_tiles
    flops_grad = 2.0 * 64 * 64 * n * col_tiles * (-(-(d + 1) // 64))  # (the slices' rows rounded up to 32 are not counted)
    useful = 2.0 * n * cols * (d + 1)
    tf_res, tf_grad = flops_res / s["wm_logreg_residual"][0] / 1e9, flops_grad / s["wm_logreg_gradient"][0] / 1e9
    read_gb = n * d * 4 / 1e9
    lines += [f"## {name}: {n} x {d}, K = {K}, {groups} value(s) of C = {cols} columns", "", "| call | per call |", "|---|---|"]
    lines += [f"| {m} | {fmt(v)} |" for m, v in s.items()]
    ev = s["wm_logreg_residual"][0] + s["wm_logreg_gradient"][0]
    two = s[f"wm_pca_project, m = {cols}"][0] + s[f"wm_gmm_weighted_sums, k = {cols}"][0]
    lines += ["", f"One evaluation, kernels only: {ev:.3f} ms; `wm_pca_project` + `wm_gmm_weighted_sums` at equal sizes: {two:.3f} ms "
              f"(ratio {ev / two:.2f}).  Executed float64 MFMA work: residual {flops_res / 1e9:.2f} GFLOP ({useful / 1e9:.2f} useful) -> "
              f"{tf_res:.2f} TF = {100 * tf_res / F64_MATRIX_PEAK_TF:.1f} % of the float64 matrix peak ({F64_MATRIX_PEAK_TF} TF, data "
              f"sheet); gradient {flops_grad / 1e9:.2f} GFLOP ({useful / 1e9:.2f} useful) -> {tf_grad:.2f} TF = "
              f"{100 * tf_grad / F64_MATRIX_PEAK_TF:.1f} %.  Each pass reads the {read_gb * 1e3:.1f} MB of x once: "
              f"{read_gb / s['wm_logreg_residual'][0] * 1e3:.0f} GB/s (residual), {read_gb / s['wm_logreg_gradient'][0] * 1e3:.0f} GB/s "
              "(gradient), algorithmic bytes over time; where they were served from was not measured.", ""]
    rec = {"name": name, "n": n, "d": d, "groups": groups, "ms": s, "residual_tf": tf_res, "gradient_tf": tf_grad,
           "ratio_to_the_two_products": ev / two}
    print(json.dumps(rec), flush=True)
    return rec


def bench_fit(x, y_np, a, lines):
    """Whole fits on the golden matrix: C = 1e-3 alone and [1e-4, 1e-3, 1e-2, 1e-1] in one solve."""
    xh = x.cpu().numpy().astype(np.float64)
    lines += ["## Whole fits on the golden matrix (wall clock, tol = 1e-4)", ""]
    rec = {}
    for cs in ([1e-3], [1e-4, 1e-3, 1e-2, 1e-1]):
        def fit():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return linear_model.LogisticRegression(cs, tol=1e-4, max_iter=a.sklearn_max_iter).fit(x, y_np)
        fit()  # warm-up
        out = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model = fit()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        rec[f"fit_{len(cs)}_ms"] = summary(out)
        lines.append(f"- `LogisticRegression({cs}, tol=1e-4, max_iter={a.sklearn_max_iter})`.fit, 3 runs: {fmt(summary(out))}; "
                     f"n_iter_ {model.n_iter_.tolist()}, converged {model.converged_.tolist()}")
    if a.no_sklearn:
        lines.append("- sklearn on the host: not measured (--no-sklearn)")
    else:
        from sklearn.linear_model import LogisticRegression as Sk

        for c in (1e-3,):
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sk = Sk(C=c, tol=1e-4, max_iter=a.sklearn_max_iter).fit(xh, y_np)
            t_sk = (time.perf_counter() - t0) * 1e3
            rec["sklearn_ms"] = t_sk
            lines.append(f"- `sklearn.linear_model.LogisticRegression(C={c:g}, tol=1e-4, max_iter={a.sklearn_max_iter})` on the host's "
                         f"CPUs, float64, one run: {t_sk:.0f} ms, n_iter_ {sk.n_iter_.tolist()} (its tol is scipy's projected-gradient "
                         "test on the unscaled objective, not this project's max |grad f|: the iteration counts are not comparable "
                         "one to one)")
    try:
        from ssl_wafermap_amd.models.evals import LinearClassifier, fit_linear_probe

        classes = np.unique(y_np)
        labels = torch.from_numpy(np.searchsorted(classes, y_np)).to(DEV)
        torch.manual_seed(0)
        probe = LinearClassifier(x.shape[1], len(classes)).to(DEV)
        fit_linear_probe(probe, x, labels, epochs=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit_linear_probe(probe, x, labels, epochs=10)
        torch.cuda.synchronize()
        t_probe = (time.perf_counter() - t0) * 1e3
        rec["adam_probe_10_epochs_ms"] = t_probe
        lines.append(f"- `evals.fit_linear_probe`, 10 epochs of Adam at batch 256 (wall clock only): {t_probe:.0f} ms")
    except Exception as e:  # the Adam probe is a by-stander here: its failure is reported, not hidden
        lines.append(f"- `evals.fit_linear_probe`: not measured ({type(e).__name__}: {e})")
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "logreg.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-max-iter", type=int, default=300, help="the iteration cap of every whole fit, ours and sklearn's")
    ap.add_argument("--resources", default="", help="a file with the compiler's resource report of csrc/logreg.hip to include")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_logreg.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    lines = ["# Logistic regression: the two kernels of an evaluation, and a whole fit", "",
             "Scope: `csrc/logreg.hip` and `linear_model.LogisticRegression`.  One MI355X.  Written by `tools/bench_logreg.py`: direct",
             f"calls of the entry points on preallocated buffers, one warm-up call, then {a.reps} rounds of about {a.window:g} s of",
             "back-to-back calls each, device events around a round; per call: median (min .. max) over the rounds.", "",
             "Not measured: 811 457 rows; hardware counters; a profiler trace (so no per-kernel split of wm_logreg_residual's two",
             "launches or of the gradient's tile pass and merge); more than 64 columns (the T = 2 .. 4 forms of lr_residual, one",
             "workgroup per CU); the sigmoid mode.", ""]
    if a.resources:
        lines += ["## Kernel resources (compiler report)", "", "```"] + Path(a.resources).read_text().splitlines() + ["```", ""]
    emb = torch.from_numpy(z["embeddings"].astype(np.float32)).to(DEV)
    golden = StandardScaler().fit_transform(emb).contiguous()
    y_np = z["labels"].astype(np.int64)
    y_dev = torch.from_numpy(y_np.astype(np.int32)).to(DEV)
    recs = []
    big, big_y = synthetic(172950, 512, 172950)
    for groups in (1, 4):
        recs.append(bench_kernels("golden embeddings, standardised", golden, y_dev, groups, a, lines))
        recs.append(bench_kernels("synthetic, 9 blobs, seed 172950", big, big_y, groups, a, lines))
    recs.append(bench_fit(golden, y_np, a, lines))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
