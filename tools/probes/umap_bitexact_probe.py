"""Run every entry point of csrc/umap.hip through manifold.py on seeded inputs and save the outputs: run once per library
build (WM_HIP_LIB selects it) and compare the files (kernel-restructuring changes that must be bit-identical).

    WM_HIP_LIB=<build A> python tools/probes/umap_bitexact_probe.py a.pt
    WM_HIP_LIB=<build B> python tools/probes/umap_bitexact_probe.py b.pt
    python tools/probes/umap_bitexact_probe.py --compare a.pt b.pt      # exit status 1 if any entry differs

Shapes: n = 2, 65, 300 vertices and the dims 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 64 (every padded dimension the three
dimension-templated kernels are instantiated for, and both sides of every step from one padded dimension to the next).
The memberships, the label intersection and the graph radii run on the kNN graph of seeded rows, some of them duplicates
(zero distances); the layouts on a hand-made symmetric graph whose last vertex has no entries, with
negative_sample_rate 0 and 5, whole and split into two calls; the DensMAP layout over an epoch range that crosses into
the density phase, with its DensityTerms; the query memberships and the transform layout also at k = 64."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = [k for k in sorted(set(a) | set(b))
           if k not in a or k not in b or not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    print(f"{len(a)} / {len(b)} entries, {sum(torch.is_tensor(v) for v in a.values())} tensors, {len(bad)} differ")
    for k in bad:
        print("DIFFERS:", k)
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from ssl_wafermap_amd import manifold  # noqa: E402

DIMS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 64)
A, B = 1.57694, 0.89506
EPOCHS, SPLIT = 20, 16  # dens_frac = 0.3: the phase is epochs 14 .. 19, so [0, 16) + [16, 20) splits inside it
out = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keep(tag, *tensors):
    for t, v in enumerate(tensors):
        out[f"{tag}_{t}"] = v.cpu()


def hand_graph(n, rng):
    """Symmetric CSR on n vertices: a ring with chords over vertices 0 .. n - 2, the last vertex without entries (n > 2);
    rates with 65536, 32768, 21845, 1 and 0 among them, weights in keeping with the rates."""
    if n == 2:
        pairs = {(0, 1)}
    else:
        live = n - 1
        pairs = {(i, (i + 1) % live) for i in range(live)} | {(int(i), int(j)) for i, j in rng.integers(0, live, (3 * n, 2))}
        pairs = {(min(p), max(p)) for p in pairs if p[0] != p[1]}
    special = [65536, 32768, 21845, 1, 0]
    rate = {p: special[t % 5] if t < 10 else int(rng.integers(0, 65537)) for t, p in enumerate(sorted(pairs))}
    adj = [[] for _ in range(n)]
    for (i, j), r in rate.items():
        adj[i].append((j, r))
        adj[j].append((i, r))
    indptr = np.concatenate([[0], np.cumsum([len(a) for a in adj])]).astype(np.int32)
    flat = [e for a in adj for e in sorted(a)]
    indices = np.array([e[0] for e in flat], dtype=np.int32)
    q = np.array([e[1] for e in flat], dtype=np.int32)
    return dev(indptr), dev(indices), dev(q), dev((np.maximum(q, 1) / 65536.0).astype(np.float32))


for n in (2, 65, 300):
    rng = np.random.default_rng(n)
    # ---- memberships, label intersection, graph radii on the kNN graph of seeded rows with duplicates
    x = rng.standard_normal((n, 8)).astype(np.float32)
    if n > 2:
        x[5:9] = x[4]
        x[n - 1] = x[0]
    k = min(15, n)
    dist, idx = manifold.knn_graph(dev(x), k)
    rho, sigma, w = manifold.smooth_knn(dist, idx)
    keep(f"smooth_knn_n{n}", rho, sigma, w)
    graph, gd = manifold.fuzzy_union(idx, w, dist)
    labels = dev(rng.integers(-1, 4, n).astype(np.int32))
    inter = manifold.label_intersect(graph, labels, manifold.far_distance(0.5))
    keep(f"label_intersect_n{n}", inter.data, manifold.label_intersect(graph, labels, manifold.far_distance(1.0), 0.3).data)
    for g in (graph, inter):
        keep(f"graph_radii_n{n}_{'plain' if g is graph else 'labels'}",
             *(manifold.graph_radii(g.indptr, g.data, gd, manifold.sample_rates(g.data), e) for e in (20, 500)))
    # ---- memberships of new rows: k = 15 (or n) and 64, sorted distances with leading zeros
    for kq in sorted({k, 64}):
        dq = np.sort(np.abs(rng.standard_normal((n + 3, kq))).astype(np.float32), axis=1)
        dq[::4, :2] = 0.0
        dq[1] = 0.0
        keep(f"smooth_knn_query_n{n}_k{kq}", *manifold.smooth_knn_query(dev(dq)))
    # ---- layouts on the hand-made graph
    ip, ix, q, data = hand_graph(n, rng)
    rad = dev((1.0 + rng.standard_normal(n)).astype(np.float32))
    for dim in DIMS:
        y0 = (3.0 * rng.standard_normal((n, dim))).astype(np.float32)
        y0[1] = y0[0]  # a coincident pair: r = 0
        y0d = dev(y0)
        tag = f"n{n}_d{dim}"
        keep("embedding_radii_" + tag, *manifold.embedding_radii(y0d, ip, ix, q, A, B, EPOCHS))
        for rate in (0, 5):
            kw = dict(gamma=1.0, learning_rate=1.0, seed=7 + n, negative_sample_rate=rate)
            whole = manifold.optimize_layout(y0d, ip, ix, q, A, B, EPOCHS, **kw)
            part = manifold.optimize_layout(y0d, ip, ix, q, A, B, EPOCHS, 0, SPLIT, **kw)
            keep(f"layout_{tag}_r{rate}", whole, part, manifold.optimize_layout(part, ip, ix, q, A, B, EPOCHS, SPLIT, EPOCHS, **kw))
            dkw = dict(kw, dens_lambda=2.0, dens_frac=0.3, dens_var_shift=0.1, return_terms=True)
            whole, terms = manifold.optimize_layout_densmap(y0d, ip, ix, q, data, rad, A, B, EPOCHS, **dkw)
            part, t1 = manifold.optimize_layout_densmap(y0d, ip, ix, q, data, rad, A, B, EPOCHS, 0, SPLIT, **dkw)
            rest, t2 = manifold.optimize_layout_densmap(part, ip, ix, q, data, rad, A, B, EPOCHS, SPLIT, EPOCHS, **dkw)
            keep(f"densmap_{tag}_r{rate}", whole, part, rest)
            for name, t in (("whole", terms), ("part", t1), ("rest", t2)):
                keep(f"densmap_terms_{name}_{tag}_r{rate}", t.inv_d, t.inv_den, t.w, t.re,
                     torch.tensor([t.scale, t.mu_tot, t.mean, t.var, t.cov, t.std], dtype=torch.float64))
        # ---- transform: m new points among the n positions, k entries each
        m = n + 3
        for kt in sorted({min(15, n), min(64, n)}):
            ti = np.stack([rng.permutation(n)[:kt] for _ in range(m)]).astype(np.int32)
            tq = rng.choice([65536, 32768, 21845, 1, 0, int(rng.integers(0, 65537))], size=(m, kt)).astype(np.int32)
            tq[m - 1] = 0
            yn = (3.0 * rng.standard_normal((m, dim))).astype(np.float32)
            yn[0] = y0[ti[0, 0]]  # on top of its first neighbour: r = 0
            tq[0, 0] = 65536
            ynd, tid, tqd = dev(yn), dev(ti), dev(tq)
            for rate in (0, 5):
                kw = dict(gamma=1.0, learning_rate=1.0, seed=11 + n, negative_sample_rate=rate)
                whole = manifold.optimize_transform(ynd, y0d, tid, tqd, A, B, EPOCHS, **kw)
                part = manifold.optimize_transform(ynd, y0d, tid, tqd, A, B, EPOCHS, 0, 7, **kw)
                keep(f"transform_{tag}_k{kt}_r{rate}", whole, part,
                     manifold.optimize_transform(part, y0d, tid, tqd, A, B, EPOCHS, 7, EPOCHS, **kw))

torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print(f"saved {len(out)} entries to {sys.argv[1]}")
