"""Embedding-quality micro-benchmark (manifold.py embedding_quality; csrc/cluster.hip wm_rank_query, wm_pair_dist): the
rank pass next to wm_knn_graph at the same k over the same pairs, in the 512-D feature space and in the 2-D embedding
(padded to d = 4), embedding_quality end to end, and sklearn's trustworthiness on the script's 5 000-row sample, on one
MI355X.

    python tools/bench_embedding_quality.py [--out profiles/embedding_quality.md] [--reps 7] [--window 0.3] [--epochs 200]

Rows: the golden SimSiam subset (12 449 x 512, standardised) and a UMAP(n_neighbors=15) of it to two dimensions.  The
thresholds of a rank pass are what embedding_quality gives it: the neighbour lists of the OTHER space (trustworthiness
counts in the feature space before the embedding's neighbours, continuity in the embedding before the feature space's),
their distances from wm_pair_dist, sorted per row.  The entry points are called directly on preallocated buffers: one
warm-up call, then --reps rounds, every round timing a window of back-to-back calls of each pass in turn with device
events; the number of calls per window is set from a first timing of 10 calls so that a window lasts about --window
seconds; reported per call: median (min .. max) over the rounds.  embedding_quality is timed as a whole with the host
clock (it sorts the thresholds with torch and scores on the host), sklearn with the host clock, once.  A pass over n^2
pairs is 3 n^2 d float32 operations on the vector ALU (157.3 TF peak)."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ssl_wafermap_amd import _lib, manifold  # noqa: E402
from ssl_wafermap_amd.retrieval import StandardScaler  # noqa: E402

PEAK_F32_VALU = 157.3e12
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


def sorted_thresholds(xc, lists, k):
    """(t, tj) of the rank pass that counts in the space xc before the entries of `lists`, sorted per row by (t, tj)."""
    idx = lists[:, :k].contiguous()
    thr = manifold.pair_distances(xc, xc, idx)
    by_j = torch.sort(idx, dim=1, stable=True).indices
    order = by_j.gather(1, torch.sort(thr.gather(1, by_j), dim=1, stable=True).indices)
    return thr.gather(1, order).contiguous(), idx.gather(1, order).contiguous()


def bench_space(name, xc, other_lists, ks, reps, window, lines):
    """The rank pass in the space xc [n, d] before the other space's neighbours, next to wm_knn_graph on xc."""
    lib = _lib.load()
    st = _lib.stream_ptr()
    n, d = xc.shape
    skip = torch.arange(n, dtype=torch.int32, device=DEV)
    passes, keep = {}, []
    for k in ks:
        t, tj = sorted_thresholds(xc, other_lists, k)
        count = torch.empty((n, k), dtype=torch.int32, device=DEV)
        need_r, need_k = lib.wm_rank_query_workspace_bytes(n, n, d, k), lib.wm_knn_graph_workspace_bytes(n, d, k)
        ws_r, ws_k = torch.empty(need_r, dtype=torch.uint8, device=DEV), torch.empty(need_k, dtype=torch.uint8, device=DEV)
        kd, ki = torch.empty((n, k), device=DEV), torch.empty((n, k), dtype=torch.int32, device=DEV)
        # thresholds no pair is before: the same launch without a single search or add (staging, pairs, root, filter)
        t_none, tj_none = torch.full_like(t, -1.0), torch.zeros_like(tj)
        count_none = torch.empty_like(count)
        keep.append((t, tj, count, ws_r, ws_k, kd, ki, t_none, tj_none, count_none))
        passes[f"floor{k}"] = (lambda t=t_none, tj=tj_none, count=count_none, ws_r=ws_r, need_r=need_r, k=k: _lib.check(
            lib.wm_rank_query(xc.data_ptr(), n, xc.data_ptr(), n, d, 0, t.data_ptr(), tj.data_ptr(), skip.data_ptr(), k, count.data_ptr(),
                              ws_r.data_ptr(), need_r, st), "wm_rank_query"))
        passes[f"rank{k}"] = (lambda t=t, tj=tj, count=count, ws_r=ws_r, need_r=need_r, k=k: _lib.check(
            lib.wm_rank_query(xc.data_ptr(), n, xc.data_ptr(), n, d, 0, t.data_ptr(), tj.data_ptr(), skip.data_ptr(), k, count.data_ptr(),
                              ws_r.data_ptr(), need_r, st), "wm_rank_query"))
        passes[f"knn{k}"] = (lambda kd=kd, ki=ki, ws_k=ws_k, need_k=need_k, k=k: _lib.check(
            lib.wm_knn_graph(xc.data_ptr(), n, d, 0, k, kd.data_ptr(), ki.data_ptr(), ws_k.data_ptr(), need_k, st), "wm_knn_graph"))
    inner = {}
    for key, fn in passes.items():
        fn()
        torch.cuda.synchronize()
        inner[key] = max(10, int(window * 1e3 / timed(fn, 10)))
    times = {key: [] for key in passes}
    for _ in range(reps):
        for key, fn in passes.items():
            times[key].append(timed(fn, inner[key]))
    s = {key: summary(v) for key, v in times.items()}
    flop, pairs = 3.0 * n * n * d, float(n) * n
    lines += [f"## {name}: n = {n}, d = {d}", "",
              "| pass | per call | G pairs / s | TF | share of 157.3 TF |", "|---|---|---|---|---|"]
    rec = {"space": name, "n": n, "d": d, "inner": inner}
    for k in ks:
        for key, label in ((f"rank{k}", f"rank pass, k = {k} thresholds per row (`wm_rank_query`)"),
                           (f"floor{k}", f"the same launch with thresholds no pair is before (no search, no add), k = {k}"),
                           (f"knn{k}", f"kNN graph, k = {k} (`wm_knn_graph`)")):
            lines.append(f"| {label} | {fmt(s[key])} | {pairs / s[key][0] / 1e6:.1f} | {flop / s[key][0] / 1e9:.2f} | "
                         f"{flop / PEAK_F32_VALU * 1e3 / s[key][0]:.3f} |")
            rec[f"{key}_ms"] = s[key]
    lines.append("")
    for k in ks:
        r, q = s[f"rank{k}"], s[f"knn{k}"]
        rec[f"ratio{k}"] = r[0] / q[0]
        mean_rank = float(keep[ks.index(k)][2].double().mean())
        lines.append(f"`wm_rank_query` / `wm_knn_graph` at k = {k}: {r[0] / q[0]:.3f} x; the kNN timing's own spread over the {reps} rounds, "
                     f"(max - min) / median: {(q[2] - q[1]) / q[0]:.3f}.  Mean count per (row, threshold): {mean_rank:.1f} of {n - 1} columns "
                     f"(the pairs that pass the last-threshold filter and are searched and added are at most k times that per row).  "
                     f"Searches and adds: {r[0] - s[f'floor{k}'][0]:.3f} ms of the {r[0]:.3f} ms "
                     f"({(r[0] - s[f'floor{k}'][0]) / r[0]:.0%}).")
        assert int(keep[ks.index(k)][9].abs().sum()) == 0, "thresholds no pair is before must count nothing"
    lines.append("")
    print(json.dumps(rec), flush=True)
    return rec, s


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "embedding_quality.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--rows", type=int, default=0, help="use the first N rows only (a rehearsal)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_embedding_quality.py needs the GPU: nothing is measured without one")
    z = np.load(ROOT / "tests" / "golden" / "simsiam_preds_subset.npz")
    emb = z["embeddings"].astype(np.float32)
    if a.rows:
        emb = emb[:a.rows]
    x = StandardScaler().fit_transform(torch.from_numpy(emb).to(DEV)).contiguous()
    n = int(x.shape[0])
    y = manifold.UMAP(n_neighbors=15, n_components=2, n_epochs=a.epochs, random_state=0).fit_transform(x)
    xp, yp = manifold._prep(x), manifold._prep(y)
    ks = [15, 63]
    near_x, near_y = manifold.neighbor_lists(xp, max(ks)), manifold.neighbor_lists(yp, max(ks))
    lines = ["# Embedding quality: the rank pass next to the kNN graph", "",
             "Scope: `csrc/cluster.hip` (`wm_rank_query`: the `CL_RANK` mode of `cl_pairs` with `cl_rank_merge`; `wm_pair_dist`) and",
             "`manifold.embedding_quality`, next to `wm_knn_graph` at the same k over the same pairs.  One MI355X.  Written by",
             f"`tools/bench_embedding_quality.py`: direct calls of the entry points on preallocated buffers, one warm-up call, then {a.reps} rounds",
             f"of about {a.window:g} s of back-to-back calls per pass, device events around a window; per call: median (min .. max) over the",
             "rounds.  The TF column counts 3 d float32 operations per pair; the share of peak is against the 157.3 TF vector rate.  Per-kernel",
             "times from a profiler trace: not measured.",
             f"Rows: the {n} standardised golden embeddings (d = {x.shape[1]}) and their UMAP(n_neighbors=15, n_epochs={a.epochs}) to 2-D, which the",
             "kernels see padded to d = 4.  The thresholds are embedding_quality's: the other space's neighbour lists.", ""]
    rec_x, s_x = bench_space("feature space (the trustworthiness pass)", xp, near_y, ks, a.reps, a.window, lines)
    rec_y, s_y = bench_space("2-D embedding (the continuity pass)", yp, near_x, ks, a.reps, a.window, lines)

    # what bounds the pass at d = 4: the arithmetic of a pair is 8 VALU instructions there (a subtract and a fused
    # multiply-add per feature); the measured pair rate is set next to the rate at which the vector ALUs could issue them,
    # and the launch without searches next to the launch with them
    lane_rate = PEAK_F32_VALU / 2.0  # lane-instructions per second (the peak counts a fused multiply-add as two operations)
    lines += ["## What bounds the pass at d = 4", ""]
    for k in ks:
        r4, f4 = s_y[f"rank{k}"][0], s_y[f"floor{k}"][0]
        lines.append(f"* k = {k}: {float(n) * n / r4 / 1e6:.1f} G pairs / s, {lane_rate * r4 * 1e-3 / (float(n) * n):.0f} vector lane-instruction "
                     f"slots per pair at the 157.3 TF issue rate, of which the distance arithmetic of a pair needs 8.  Without a single search "
                     f"or add the launch takes {f4:.3f} ms of the {r4:.3f} ms: the searches and adds are {(r4 - f4) / r4:.0%} of the pass.")
    lines += ["",
              "So the pass is not bound by the pair arithmetic at d = 4; two parts bound it.  (1) What surrounds a pair per 64 x 64 tile even "
              "when nothing is searched (the rows \"no search, no add\"): both operands are staged through LDS with two workgroup barriers per "
              "tile for a single 4-feature step, the first fetch of a tile is not overlapped with the tile before, and every pair takes the "
              "correctly rounded square root and the three-instruction compare with the row's last threshold.  (2) The binary searches, whose "
              "share grows with k: only a few pairs per row pass the last-threshold filter, but a wave runs the search for one of its 16 "
              "pairs per lane whenever ANY of its 64 lanes passed there, the other lanes idle, and every search is a chain of up to 6 "
              "dependent LDS reads that the two or three resident waves per SIMD do not hide.  "
              f"`wm_knn_graph` at d = 4 ({s_y['knn15'][0]:.3f} ms at k = 15) pays the same staging and adds its owner scan per tile.  Profiler "
              "counters (LDS stalls, barrier waits): not measured.", ""]

    whole, first = [], None
    for _ in range(max(3, a.reps)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = manifold.embedding_quality(x, y, 15)
        whole.append((time.perf_counter() - t0) * 1e3)
        first = first or q
        assert q.trustworthiness == first.trustworthiness and q.continuity == first.continuity, "two runs must give the same bits"
    s_whole = summary(whole)
    t0 = time.perf_counter()
    many = manifold.embedding_quality(x, y, [5, 15, 30, 63])
    sweep_ms = (time.perf_counter() - t0) * 1e3

    from sklearn.manifold import trustworthiness

    pick = np.sort(np.random.default_rng(0).permutation(n)[:5000])
    xs, ys = x[torch.from_numpy(pick).to(DEV)].cpu().numpy(), y.cpu().numpy()[pick]
    t0 = time.perf_counter()
    sk = float(trustworthiness(xs, ys, n_neighbors=15))
    sk_ms = (time.perf_counter() - t0) * 1e3
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    lines += ["## End to end", "",
              f"`embedding_quality(x, y, 15)` on all {n} rows (two kNN graphs at k = 16, two `wm_pair_dist`, two rank passes, torch sorts of",
              f"the thresholds, the copy of the ranks to the host and the float64 scores there): {fmt(s_whole)} by the host clock, "
              f"{len(whole)} calls.  One call for n_neighbors = [5, 15, 30, 63] (one pass at k = 63): {sweep_ms:.1f} ms.", "",
              f"Scores on all rows at k = 15: trustworthiness {first.trustworthiness:.4f}, continuity {first.continuity:.4f}, neighbour "
              f"preservation {first.neighbor_preservation:.4f}; at k = " + ", ".join(
                  f"{q.n_neighbors}: T {q.trustworthiness:.4f} C {q.continuity:.4f} P {q.neighbor_preservation:.4f}" for q in many) + ".", "",
              f"`sklearn.manifold.trustworthiness` on the script's sample of {pick.size} seeded rows (n_neighbors = 15, OMP_NUM_THREADS = "
              f"{threads}), one call by the host clock: {sk_ms:.0f} ms, score {sk:.4f} (a different quantity: the neighbourhoods of the sample, "
              "trustworthiness only).  Ratio sklearn on the sample / embedding_quality on all rows: "
              f"{sk_ms / s_whole[0]:.1f} x.", ""]
    rec = {"n": n, "embedding_quality_ms": s_whole, "sweep_ms": sweep_ms, "sklearn_ms": sk_ms, "sklearn_rows": int(pick.size), "sklearn_score": sk,
           "trustworthiness": first.trustworthiness, "continuity": first.continuity, "neighbor_preservation": first.neighbor_preservation}
    print(json.dumps(rec), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return [rec_x, rec_y, rec]


if __name__ == "__main__":
    main()
