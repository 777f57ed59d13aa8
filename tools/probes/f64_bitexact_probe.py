"""Run every entry point of the float64 kernel files (csrc/pca.hip, gmm.hip, kmeans.hip, spectral.hip, propagate.hip)
on seeded rows and save the outputs: run once per library build (WM_HIP_LIB selects it) and compare the files (changes
that must be bit-identical: these kernels promise the same bits for the same sizes).

    WM_HIP_LIB=<build A> python tools/probes/f64_bitexact_probe.py a.pt
    WM_HIP_LIB=<build B> python tools/probes/f64_bitexact_probe.py b.pt
    python tools/probes/f64_bitexact_probe.py --compare a.pt b.pt      # exit status 1 if any entry differs

Shapes: the smallest of the GPU tests' lists that reach each path.  PCA (n, d): one partial tile; two tiles with a
partial one; 36 Gram tiles in several slices; 17 slices of one tile; 512-row mean slabs.  Mixture (n, d, k): a partial
tile, the straddling diagonal tile of logprob_full, four column tiles, several slices, several component batches and
tiles.  KMeans (n, d, k, R): one slab and many, one restart and three; seeding with k = 30 centres.  Lanczos (n, j,
ncomp): one slab and 17, basis columns across the 64-lane chunk.  Label spreading: two groups of alphas, soft and hard."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(a[k], b[k])]
    print(f"{len(a)} / {len(b)} entries, {sum(v.numel() for v in a.values())} values, {len(bad)} differ")
    for k in bad:
        print("DIFFERS:", k)
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from ssl_wafermap_amd import cluster, decomposition, manifold, mixture, semi_supervised  # noqa: E402

out = {}
M_OF = {20: (1, 17, 20), 68: (2, 17, 68), 512: (16, 50, 512), 64: (1, 15, 50, 64)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keep(tag, *tensors):
    for t, v in enumerate(tensors):
        v = v.cpu()
        # compared as bits: torch.equal on the integer view tells -0.0 from 0.0 and equal NaNs as equal
        out[f"{tag}_{t}"] = v.view(torch.int64 if v.dtype == torch.float64 else torch.int32) if v.is_floating_point() else v


# ------------------------------------------------------------------------------------------------ pca.hip
for n, d in ((5, 20), (65, 68), (1000, 512), (4097, 64)):
    rng = np.random.default_rng(100 * n + d)
    x = dev((rng.standard_normal((n, d)) * 3 + rng.standard_normal(d)).astype(np.float32))
    mean = decomposition.column_means(x)
    keep(f"pca_mean_n{n}_d{d}", mean)
    keep(f"pca_gram_n{n}_d{d}", decomposition.gram(x, mean), decomposition.gram(x))
    for m in M_OF[d]:
        w = rng.standard_normal((m, d))
        y = decomposition.project(x, w, mean)
        keep(f"pca_project_n{n}_d{d}_m{m}", y, decomposition.project(x, w))
        keep(f"pca_reconstruct_n{n}_d{d}_m{m}", decomposition.reconstruct(y, w, mean), decomposition.reconstruct(y, w))
keep("pca_mean_n262400_d4", decomposition.column_means(dev(np.random.default_rng(9).standard_normal((262400, 4)).astype(np.float32))))


# ------------------------------------------------------------------------------------------------ gmm.hip
def gmm_case(n, d, k, seed):
    rng = np.random.default_rng(seed)
    xp, d_ = mixture._prep(dev(rng.standard_normal((n, d)).astype(np.float32)), "diag")
    resp = rng.random((n, k)) + 1e-3
    resp /= resp.sum(axis=1, keepdims=True)
    return rng, xp, dev(resp), dev(rng.standard_normal((k, d)))


for n, d, k in ((33, 5, 7), (63, 64, 3), (255, 65, 2), (32, 256, 2)):
    rng, xp, _, mean = gmm_case(n, d, k, 1000 * n + d)
    pchol = np.triu(rng.standard_normal((k, d, d))) / np.sqrt(d)  # (the kernel reads the upper triangle only)
    keep(f"gmm_logprob_full_n{n}_d{d}_k{k}", mixture._logprob_full(xp, d, mean, dev(pchol), dev(rng.standard_normal(k))))
for n, d, k in ((33, 5, 7), (65, 63, 65), (4097, 17, 130)):
    rng, xp, resp, mean = gmm_case(n, d, k, 2000 * n + d)
    keep(f"gmm_weighted_sums_n{n}_d{d}_k{k}", *mixture._weighted_sums(xp, d, resp))
    keep(f"gmm_scatter_diag_n{n}_d{d}_k{k}", mixture._scatter_diag(xp, d, resp, mean))
for n, d, k in ((65, 64, 2), (257, 65, 3), (1000, 130, 2)):
    rng, xp, resp, mean = gmm_case(n, d, k, 3000 * n + d)
    keep(f"gmm_scatter_full_n{n}_d{d}_k{k}", mixture._scatter_full(xp, d, resp, mean))
for n, k in ((257, 65), (65600, 2)):
    wlp = dev(np.random.default_rng(n + k).standard_normal((n, k)) * 5 - 40)
    keep(f"gmm_normalize_n{n}_k{k}", *mixture._normalize(wlp), wlp)
rng, xp, _, mean = gmm_case(65, 17, 65, 4)
keep("gmm_logprob_diag_n65_d17_k65", mixture._logprob_diag(xp, 17, mean, dev(rng.random((65, 17)) + 0.5), dev(rng.standard_normal(65))))

# ------------------------------------------------------------------------------------------------ kmeans.hip
for n, d, k, r in ((65, 52, 64, 1), (1000, 512, 64, 3)):
    rng = np.random.default_rng(n + d + k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[n // 2] = x[n // 2 + 1]  # a duplicate row: equal distances, the tie goes to the lower centre
    centres = x[rng.choice(n, size=(r, k))]  # (centres drawn with replacement: empty clusters keep their centre)
    step = cluster.kmeans_step(dev(x), dev(centres))
    keep(f"kmeans_step_n{n}_d{d}_k{k}_r{r}", *step)
    keep(f"kmeans_step2_n{n}_d{d}_k{k}_r{r}", *cluster.kmeans_step(dev(x), step.centres, prev=step.labels))  # (prev given)
x = dev(np.random.default_rng(700).standard_normal((700, 4)).astype(np.float32))
centres, idx, details = cluster.kmeans_plusplus(x, 30, random_state=3, return_details=True)
keep("kmeans_seed_n700_d4_k30", centres, torch.from_numpy(idx), torch.from_numpy(details["candidates"]),
     torch.from_numpy(details["potentials"]))


# ------------------------------------------------------------------------------------------------ spectral.hip
def random_graph(n, seed, per_row=6):
    """A symmetric float32 graph as manifold.CSR, and two groups of rows that no edge joins."""
    from scipy.sparse import coo_matrix

    rng = np.random.default_rng(seed)
    half = n // 2
    i = np.repeat(np.arange(n), per_row)
    j = np.where(i < half, rng.integers(0, max(half, 1), i.size), half + rng.integers(0, n - half, i.size))
    g = coo_matrix((rng.random(i.size).astype(np.float32) + 0.1, (i, j)), shape=(n, n)).tocsr()
    g = (g + g.T).tocsr()
    g.sum_duplicates()
    g.sort_indices()
    return manifold.CSR(dev(g.indptr.astype(np.int32)), dev(g.indices.astype(np.int32)), dev(g.data.astype(np.float32)))


for n, j, ncomp in ((65, 16, 3), (4097, 129, 3)):
    rng = np.random.default_rng(77 * n + j)
    labels = rng.integers(0, ncomp, n).astype(np.int32)
    labels[:ncomp] = np.arange(ncomp)
    u = rng.random(n) + 0.5
    u /= np.sqrt(np.bincount(labels, weights=u * u, minlength=ncomp))[labels]
    m = j + 2
    basis = np.zeros((n, m + 1))
    basis[:, :j + 1] = np.linalg.qr(rng.standard_normal((n, j + 1)))[0]
    w, V, T = dev(rng.standard_normal(n)), dev(basis), torch.zeros(m * m + 2, dtype=torch.float64, device="cuda")
    manifold.lanczos_orthonormalise(w, V, j, dev(labels), ncomp, dev(u), T, m)
    keep(f"spec_ortho_n{n}_j{j}", w, V, T)
for n in (17, 4097):
    rng = np.random.default_rng(n)
    graph = random_graph(n, n)
    deg, dinv = manifold.laplacian_degree(graph)
    keep(f"spec_degree_matvec_n{n}", deg, dinv, manifold.laplacian_matvec(graph, dinv, dev(rng.standard_normal(n))))
    for m, q in ((4, 1), (63, 17), (130, 51)):
        keep(f"spec_rotate_n{n}_m{m}_q{q}", manifold.basis_rotate(dev(rng.standard_normal((n, m + 3))), rng.standard_normal((m, q)), m))

# ------------------------------------------------------------------------------------------------ propagate.hip
n, classes = 1000, 9
rng = np.random.default_rng(5)
graph = random_graph(n, 11)
_, dinv = manifold.laplacian_degree(graph)
labels = dev(np.where(rng.random(n) < 0.1, rng.integers(0, classes, n), -1).astype(np.int32))
for hard in (False, True):
    for alphas in ((0.2,), (0.2, 0.5, 0.99)):  # 9 and 27 columns: 16 and 32 lanes per row
        groups = len(alphas)
        Fa = semi_supervised.label_matrix(labels, classes, groups)
        F, resid = semi_supervised.propagate(graph, dinv, labels, classes, dev(np.asarray(alphas)), dev(np.ones(groups, dtype=np.int32)),
                                             Fa, torch.zeros_like(Fa), 5, hard=hard)
        keep(f"lp_hard{int(hard)}_g{groups}", F, resid)
        fin = semi_supervised.finalize_labels(F, classes, groups - 1)
        keep(f"lp_finalize_hard{int(hard)}_g{groups}", *(t.to(torch.uint8) if t.dtype == torch.bool else t for t in fin))
        idx = dev(rng.integers(0, n, (37, 15)).astype(np.int32))
        keep(f"lp_neighbor_mean_hard{int(hard)}_g{groups}", semi_supervised.neighbor_mean(idx, fin[0]))

torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print(f"saved {len(out)} entries to {sys.argv[1]}")
