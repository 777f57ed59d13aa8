// The float64 pieces shared by pca.hip, gmm.hip, spectral.hip and kmeans.hip: what the kernels on
// v_mfma_f64_16x16x4_f64 have in common, the fixed-tree sum of a workgroup and the host's cut of the rows -- code whose
// order of summation is part of the contract ("same bits every call").  The bf16 files include common.h alone and do
// not pay for any of this.
//
// ---- the tile (pca_tile; gm_logprob_full and gm_rows_tile of gmm.hip).  A workgroup is F64_THREADS = 4 waves and owns
// a 64 x 64 tile of C = A B; wave w owns the 32 x 32 quadrant (wm, wn) = (w >> 1, w & 1) as 2 x 2 MFMA tiles: 4 x 4
// doubles = 32 accumulator registers per lane.  Both panels of a K step are staged in LDS as doubles, panel[k][64 + 2]
// with the tile index contiguous: lane l of a fragment read takes panel[4 kk + (l >> 4)][16 t + (l & 15)], sixteen
// consecutive doubles per k.  The pad of 2 keeps the transposing stores of K-contiguous operands off a single bank.
// What a kernel stages, how deep its K step is and what its epilogue does with a cell are the kernel's own; the next
// step's elements are requested into registers before the MFMAs of the current one.  With fk = l >> 4, fc = l & 15 an
// epilogue walks its lane's 2 x 2 x 4 cells as register r of acc[i][j] = row wm * 32 + i * 16 + fk + 4 r, column
// wn * 32 + j * 16 + fc of the tile.
// Fragment maps of v_mfma_f64_16x16x4_f64 (they differ from every other MFMA here; tests/test_gpu_pca.py,
// tests/test_gpu_mixture.py and tests/test_gpu_spectral.py settle them with exact integer data): A: lane l holds
// A[l & 15][k = l >> 4]; B: lane l holds B[k = l >> 4][l & 15]; C/D: register r of lane l is row (l >> 4) + 4 r, column
// l & 15.  Order of every sum: k ascending in steps of 4 (one MFMA each; inside an MFMA the hardware's fixed order).
// What is NOT here, because the shared form measured slower or changed a kernel's device code, which would then have
// to be timed (profiles/f64_refactor.md has every figure): the staged multiply (gm_mma in gmm.hip, written out in
// pca_tile: 0.5 - 2.5 % on the projection); the symmetric plane merges (pca_gram_merge, gm_scatter_full_merge) and the
// tree of lp_resid_merge (outside the run-to-run spread by 0.2 - 0.4 us); the lane coordinates and the accumulator
// clear (as helpers they reorder the prologues of gm_logprob_full and gm_rows_tile); the epilogue walk (with the
// multiply shared it changed pca_tile's register count).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

constexpr int F64_TILE = 64;             // C tile of a workgroup (4 waves, 32 x 32 each)
constexpr int F64_LD = F64_TILE + 2;     // LDS row stride in doubles
constexpr int F64_THREADS = 256;

// Workgroup b of a grid that walks the tiles on and below the diagonal, row by row: tile (ti, tj), tj <= ti.
__device__ __forceinline__ void f64_tri_tile(int b, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
  tj = b - ti * (ti + 1) / 2;
}

// ---- a sum in a documented order: a workgroup's THREADS values in a fixed tree, sh[t] += sh[t + w] for
// w = THREADS / 2 .. 1 (the result in every thread).  sh: THREADS doubles.
template <int THREADS>
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  const double out = sh[0];
  __syncthreads();
  return out;
}

// ---- the host's cut of the rows into slices whose partial results are merged in slice order: `want` slices at most,
// never more than `by_rows` nor than the byte cap allows (`by_bytes`); rows per slice rounded up to `round`.  A
// function of the sizes alone, never of the device.
struct F64Slices {
  int slices, slice_rows;
};
static inline F64Slices f64_cut(int n, long long want, long long by_rows, long long by_bytes, int round) {
  if (want > by_rows) want = by_rows;
  if (want > by_bytes) want = by_bytes;
  if (want < 1) want = 1;
  const long long rows = (n + want - 1) / want;
  F64Slices s;
  s.slice_rows = (int)((rows + round - 1) / round * round);
  s.slices = (n + s.slice_rows - 1) / s.slice_rows;
  return s;
}
