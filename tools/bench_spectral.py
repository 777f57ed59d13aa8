"""Laplacian-eigenmaps micro-benchmark (manifold.laplacian_eigenpairs; csrc/spectral.hip: wm_spec_matvec,
wm_spec_orthonormalise, wm_spec_rotate) on one MI355X, on two fuzzy graphs at 15 neighbours: the golden 12 449 x 512
embeddings (standardised) and seeded synthetic 172 950 x 64 rows (32 Gaussian clusters).

    python tools/bench_spectral.py [--out profiles/spectral.md] [--reps 7] [--window 0.1] [--no-synthetic]

Per graph, on preallocated buffers by direct calls of the entry points: the matvec, one Lanczos step's tail
(wm_spec_orthonormalise at the last step j = m - 1, which reads the whole basis, and at j = m / 2) and the rotation of a
restart, at m = 64 and m = 102, each timed on its own in --reps rounds of about --window seconds of back-to-back calls
with device events around a round; per call: median (min .. max) over the rounds.  The matvec next to its algorithmic
bytes (indices and weights once, the five per-row arrays once) as a share of the HBM peak of the data sheet (8 TB/s).
Whole solves (k = 2 and k = 50 at tol 1e-4 and 1e-8): cycles, matvecs and wall clock, median of --reps runs.  The yardstick
of the whole solve is the host path it can replace, `manifold._spectral_init` (scipy eigsh, which="SM", tol 1e-4) on the
connected golden graph at 30 neighbours on this machine's CPUs, next to the device solve at the same tolerance; the two
2-D spaces are compared with the span bound of tests/test_gpu_spectral.py.  Measurements to record; nothing here asserts a
ratio.  What was not run is listed as not measured."""
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
from ssl_wafermap_amd import manifold  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_TBS = 8.0
U = 2.0 ** -53


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
    emb = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")["embeddings"].astype(np.float64)
    std = emb.std(axis=0)
    return torch.from_numpy(((emb - emb.mean(axis=0)) / np.where(std > 0, std, 1.0)).astype(np.float32)).to(DEV)


def synthetic(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = 4.0 * torch.randn((32, d), generator=g, device=DEV)
    which = torch.randint(0, 32, (n,), generator=g, device=DEV)
    return (centres[which] + torch.randn((n, d), generator=g, device=DEV)).contiguous()


def steps(name, graph, a, lines):
    """The per-call times of the step kernels on `graph` at m = 64 and m = 102."""
    n, nnz = graph.shape[0], int(graph.indices.numel())
    ncomp, labels = manifold.graph_components(graph)
    deg, dinv = manifold.laplacian_degree(graph)
    u_h = manifold.trivial_vectors(deg.cpu().numpy(), labels, ncomp)
    u, comp = torch.from_numpy(u_h).to(DEV), torch.from_numpy(labels).to(DEV)
    lines += [f"## {name}: {n} rows, {nnz} entries ({nnz / n:.1f} per row), {ncomp} component(s)", "", "| call | per call |", "|---|---|"]
    rec = {"name": name, "n": n, "nnz": nnz, "components": ncomp, "ms": {}}
    for m in (64, 102):
        basis = torch.linalg.qr(torch.randn((n, m + 1), dtype=torch.float64, device=DEV))[0].contiguous()
        spare = torch.empty_like(basis)
        w0 = torch.randn(n, dtype=torch.float64, device=DEV)
        w = w0.clone()
        t_cells = torch.zeros(m * m + 2, dtype=torch.float64, device=DEV)
        ws = manifold.lanczos_workspace(n, m + 1, ncomp, DEV)
        rot = torch.linalg.qr(torch.randn((m, m), dtype=torch.float64, device=DEV))[0][:, :2 + (m - 2) // 2].contiguous()

        def tail(j):
            w.copy_(w0)
            manifold.lanczos_orthonormalise(w, basis, j, comp, ncomp, u, t_cells, m, ws)

        fns = {f"matvec (m = {m}: a column of pitch {m + 1})": lambda: manifold.laplacian_matvec(graph, dinv, basis, m - 1, out=w, checked=True),
               f"orthonormalise, m = {m}, j = {m - 1} (13 launches, with the copy that restores w)": lambda: tail(m - 1),
               f"orthonormalise, m = {m}, j = {m // 2}": lambda: tail(m // 2),
               f"rotate, m = {m}, q = {rot.shape[1]}": lambda: manifold.basis_rotate(basis, rot, m, out=spare)}
        for key, fn in fns.items():
            fn()
            inner = max(3, int(a.window * 1e3 / timed(fn, 3)))
            s = summary([timed(fn, inner) for _ in range(a.reps)])
            rec["ms"][key] = s
            lines.append(f"| {key} | {fmt(s)} |")
            if key.startswith("matvec"):
                algo = nnz * 8 + n * (4 + 8 + 8 + 8 + 8)
                rec[f"matvec_tbs_m{m}"] = algo / s[0] / 1e9
                lines.append(f"| ... its algorithmic bytes, {algo / 1e6:.2f} MB | {algo / s[0] / 1e9:.3f} TB/s = "
                             f"{100 * algo / s[0] / 1e9 / HBM_PEAK_TBS:.2f} % of the HBM peak ({HBM_PEAK_TBS} TB/s) |")
        del basis, spare
    lines.append("")
    for k in (2, 50):
        for tol in (1e-4, 1e-8):
            res = manifold.laplacian_eigenpairs(graph, k, tol=tol)  # warm-up, and the counts
            t = wall(lambda: manifold.laplacian_eigenpairs(graph, k, tol=tol), a.reps)
            rec[f"solve_k{k}_tol{tol:g}"] = {"ms": t, "cycles": res.cycles, "matvecs": res.matvecs, "converged": res.converged}
            lines.append(f"- whole solve, k = {k}, tol = {tol:g}: {res.cycles} cycles, {res.matvecs} matvecs, converged = {res.converged}, "
                         f"wall clock {fmt(t)} (the host's component search and eigh of T included)")
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec


def yardstick(x, a, lines):
    """`_spectral_init` against the device solve on the connected golden graph at 30 neighbours."""
    graph = manifold.fuzzy_simplicial_set(x, 30)
    n = graph.shape[0]
    ncomp, _ = manifold.graph_components(graph)
    lines += [f"## Yardstick: the host path on the golden graph at 30 neighbours ({n} rows, {ncomp} component)", ""]
    if ncomp != 1:
        lines += ["not measured: the graph is not connected, `_spectral_init` returns None", ""]
        return {}
    host_vecs = manifold._spectral_init(graph, 2)
    t_host = wall(lambda: manifold._spectral_init(graph, 2), min(a.reps, 3))
    res = manifold.laplacian_eigenpairs(graph, 2, tol=1e-4)
    t_dev = wall(lambda: manifold.laplacian_eigenpairs(graph, 2, tol=1e-4), a.reps)
    tight = manifold.laplacian_eigenpairs(graph, 3, tol=1e-9)
    gap = float(tight.eigenvalues[2] - tight.eigenvalues[1])
    g = graph.to_scipy().astype(np.float64)
    dinv = 1.0 / np.sqrt(np.asarray(g.sum(axis=1)).ravel())
    nmat = g.multiply(dinv[:, None]).multiply(dinv[None, :]).tocsr()

    def resid(y):
        q = np.linalg.qr(y)[0]
        theta = np.linalg.eigvalsh(q.T @ (nmat @ q))
        return q, float(np.linalg.norm(nmat @ q - q @ (q.T @ (nmat @ q)), 2)), theta

    qd, rd, _ = resid(res.eigenvectors.cpu().numpy())
    qh, rh, _ = resid(host_vecs)
    sine = float(np.linalg.norm(qd - qh @ (qh.T @ qd), 2))
    bound = 2 * (rd + rh + 8 * n * U) / gap + 8 * n * 2 * U
    rec = {"host_ms": t_host, "device_ms": t_dev, "ratio": t_host[0] / t_dev[0], "sine": sine, "bound": bound, "gap": gap,
           "resid_device": rd, "resid_host": rh, "cycles": res.cycles, "matvecs": res.matvecs}
    lines += ["| path | wall clock |", "|---|---|",
              f"| `manifold._spectral_init` (scipy eigsh which=\"SM\", tol 1e-4, {min(a.reps, 3)} runs) | {fmt(t_host)} |",
              f"| `manifold.laplacian_eigenpairs(graph, 2, tol=1e-4)` ({res.cycles} cycles, {res.matvecs} matvecs) | {fmt(t_dev)} |", "",
              f"The host path takes {rec['ratio']:.1f} x the device solve" + (" (the device solve is SLOWER)." if rec["ratio"] < 1 else "."),
              f"The two 2-D spaces: sine of the largest angle {sine:.3e}; bound 2 (r_device + r_host + 8 n u) / gap + 16 n u = {bound:.3e} with "
              f"block residuals {rd:.3e} (device) and {rh:.3e} (host) and gap lambda_3 - lambda_2 = {gap:.3e} (device solve at tol 1e-9): "
              + ("inside the bound." if sine <= bound else "OUTSIDE the bound."), ""]
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spectral.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--no-synthetic", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral.py needs the GPU: nothing is measured without one")
    lines = ["# Laplacian eigenmaps: the Lanczos step kernels and whole solves", "",
             "Scope: `csrc/spectral.hip` (`wm_spec_matvec`, `wm_spec_orthonormalise`, `wm_spec_rotate`) and",
             "`manifold.laplacian_eigenpairs`.  One MI355X.  Written by `tools/bench_spectral.py`: direct calls of the entry points on",
             f"preallocated buffers, one warm-up call, then {a.reps} rounds of about {a.window:g} s of back-to-back calls each, device events",
             "around a round; per call: median (min .. max) over the rounds.  Whole solves: wall clock, median of the runs.", "",
             "Not measured: 811 457 rows; hardware counters; a profiler trace (so no time per kernel INSIDE wm_spec_orthonormalise,",
             "only the entry point's 13 launches together).", ""]
    x = golden()
    recs = [steps("golden embeddings, 15 neighbours", manifold.fuzzy_simplicial_set(x, 15), a, lines)]
    if a.no_synthetic:
        lines += ["## synthetic 172 950 rows", "", "not measured (--no-synthetic)", ""]
    else:
        recs.append(steps("synthetic, seed 172950, 15 neighbours", manifold.fuzzy_simplicial_set(synthetic(172950, 64, 172950), 15), a, lines))
        torch.cuda.empty_cache()
    recs.append(yardstick(x, a, lines))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return recs


if __name__ == "__main__":
    main()
