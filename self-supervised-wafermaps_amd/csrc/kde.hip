// Gaussian log-sums over all pairs (density.py: KernelDensity, KDEClassifier, uniformity):
//   wm_kde_logsum   out[q][i] = log sum_j exp(-a_q * s_ij)  for up to WM_KDE_MAX_BANDWIDTHS values a_q = 1 / (2 h_q^2) in
//                   one pass, s_ij the SQUARED Euclidean distance of xr[i] and x[j], the column j + self_offset == i left
//                   out when self_offset >= 0.
// s_ij is cluster.hip's distance before its root: cl_accum<0> (cl_dist.h) over the features in index order in one
// float32 accumulator, widened exactly to double.  So s_ij and s_ji are the same bits, equal rows give exactly 0, and the
// relative error against the exact squared distance of the float32 rows is at most (d + 2) 2^-24 (first order).
//
// A file of its own and not a tenth mode of cl_pairs: the epilogue is templated on the number of bandwidths (their sums
// live in registers, so the count must be a compile-time constant), which would give cl_pairs a third template
// dimension that only this mode uses, and nothing of cl_pairs' per-mode state, LDS tiles or merge planes is shared.
// What IS shared is what the contract needs: the distance function (cl_dist.h), and the tiling, which is cl_pairs' at
// TM = 4 line for line (so the bits of s_ij are those of the other all-pairs modes).
//
// Shape: a workgroup of 256 threads owns 64 rows i and walks 64-row column tiles j of its column slice; both row sets
// are staged in LDS in chunks of 32 features ([row][36] floats); thread (ty, tx) accumulates the 4 x 4 pairs
// (ty + 16 r, tx + 16 c).  Per tile every thread turns ITS OWN 16 pairs into exponentials in double: all 256 threads
// work, there is no owner-wave scan of a distance tile and no LDS tile at all.
// ---- the shared minimum.  A thread keeps per row r ONE running minimum smin[r] of the s it has met and B sums
//   sum[r][q] = sum_j exp(-a_q (s_ij - smin[r])).
// The log-sum-exp shift of bandwidth q is max_j(-a_q s_ij) = -a_q min_j s_ij for EVERY a_q > 0, so one minimum serves
// all bandwidths, every term is exp of a number <= 0 (no overflow), the term of the minimum is exp(0) = 1 exactly, and
// the minimum depends on s alone: nothing a neighbouring bandwidth does reaches it, so a bandwidth has the same bits
// alone, inside any list and in a list cut into launches.  When a tile lowers the minimum (rare after the first tiles)
// the thread rescales its B sums by exp(-a_q (smin_old - smin_new)); smin starts at +inf with sum = 0, where the factor
// is exp(-inf) = 0 and 0 * 0 = 0: no inf - inf anywhere.  A pair whose s is not finite contributes nothing (its term is
// exp(-inf) = 0).
// ---- order of the sums, a function of (m, n, d) alone (the grid is): a thread adds its columns in ascending order
// (tile by tile, c = 0 .. 3 within a tile); at the end of a slice the 16 lanes tx of a row -- they sit side by side in
// one wave -- take the row's minimum (a minimum does not depend on the order), rescale their sums to it and are added
// in lane order tx = 0 .. 15 (every lane reads the 16 values by lane index and adds them in that order); kde_merge takes
// the minimum over the slices and adds the slices' rescaled sums in slice order, then out = -a_q M + log S.  No
// floating-point atomics, no atomics at all: two calls give the same bits.  Contraction is off in both kernels, so every
// product, sum and exp argument is rounded once whatever the instantiation.
// A row without an included column keeps smin = +inf through both kernels and gets -inf.
#include <math.h>

#include "cl_dist.h"
#include "common.h"

namespace {

constexpr int KDE_THREADS = 256;
constexpr int KDE_TM = 4;
constexpr int KDE_ROWS = 16 * KDE_TM;  // rows i per workgroup
constexpr int KDE_COLS = 64;           // rows j per column tile
constexpr int KDE_KC = 32;             // features per staged chunk
constexpr int KDE_LDK = KDE_KC + 4;    // LDS row pitch of a staged chunk (floats): cl_pairs' layout
constexpr int KDE_MAX_N = 1 << 24;
constexpr int KDE_MAXB = WM_KDE_MAX_BANDWIDTHS;
static_assert(KDE_MAXB == 4, "wm_kde_logsum dispatches on b = 1 .. 4");

struct KdeScales {  // a_q = 1 / (2 h_q^2), by value in the kernel arguments (wave-uniform scalar reads)
  double a[KDE_MAXB];
};

struct KdeArgs {
  const float* xr;  // the row operand [m][d]
  const float* x;   // the column operand [n][d]
  int m, n, d, tiles_per_slice, col_tiles, self_offset;
  KdeScales s;
  double* part_min;  // [slices][m]
  double* part_sum;  // [slices][b][m]
};

template <int B>
__global__ __launch_bounds__(KDE_THREADS) void kde_pairs(const KdeArgs p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float smem[(KDE_ROWS + KDE_COLS) * KDE_LDK];
  constexpr int TM = KDE_TM;
  constexpr int APASS = KDE_ROWS / 32, BPASS = KDE_COLS / 32;
  float* As = smem;
  float* Bs = As + KDE_ROWS * KDE_LDK;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lq = (t & 7) * 4, lr = t >> 3;  // staging: float4 at feature lq of row lr (+ 32 per pass)
  const int n = p.n, m = p.m, d = p.d, so = p.self_offset;
  const int i0 = blockIdx.x * KDE_ROWS;
  const int tile0 = blockIdx.y * p.tiles_per_slice;
  const int tile1 = min(tile0 + p.tiles_per_slice, p.col_tiles);
  const int nchunks = (d + KDE_KC - 1) / KDE_KC;

  float smin[TM];
  double sum[TM][B];
#pragma unroll
  for (int r = 0; r < TM; ++r) {
    smin[r] = INFINITY;
#pragma unroll
    for (int q = 0; q < B; ++q) sum[r][q] = 0.0;
  }

  for (int tile = tile0; tile < tile1; ++tile) {
    const int j0 = tile * KDE_COLS;
    float acc[TM][4];
#pragma unroll
    for (int r = 0; r < TM; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    float4 ra[APASS], rb[BPASS];
    auto fetch = [&](int ch) {
      const int kq = ch * KDE_KC + lq;
#pragma unroll
      for (int s = 0; s < APASS; ++s) {
        const int row = i0 + lr + 32 * s;
        ra[s] = (row < m && kq < d) ? *reinterpret_cast<const float4*>(p.xr + (size_t)row * d + kq)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int s = 0; s < BPASS; ++s) {
        const int row = j0 + lr + 32 * s;
        rb[s] = (row < n && kq < d) ? *reinterpret_cast<const float4*>(p.x + (size_t)row * d + kq)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    fetch(0);
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();  // the previous chunk is done with the staging buffers
#pragma unroll
      for (int s = 0; s < APASS; ++s) *reinterpret_cast<float4*>(As + (lr + 32 * s) * KDE_LDK + lq) = ra[s];
#pragma unroll
      for (int s = 0; s < BPASS; ++s) *reinterpret_cast<float4*>(Bs + (lr + 32 * s) * KDE_LDK + lq) = rb[s];
      __syncthreads();
      if (ch + 1 < nchunks) fetch(ch + 1);
#pragma unroll 2
      for (int kk = 0; kk < KDE_KC; kk += 4) {
        float4 a[TM], b[4];
#pragma unroll
        for (int r = 0; r < TM; ++r) a[r] = *reinterpret_cast<const float4*>(As + (ty + 16 * r) * KDE_LDK + kk);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(Bs + (tx + 16 * c) * KDE_LDK + kk);
        // index order within every pair: x, y, z, w of this float4 follow the earlier features
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<0>(a[r].x, b[c].x, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<0>(a[r].y, b[c].y, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<0>(a[r].z, b[c].z, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<0>(a[r].w, b[c].w, acc[r][c]);
      }
    }

    // ---- the tile's epilogue: this thread's 4 x 4 pairs, in registers
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int i = i0 + ty + 16 * r;
      bool ok[4];
      float tmin = INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        ok[c] = i < m && j < n && !(so >= 0 && j + so == i) && acc[r][c] < INFINITY;
        if (ok[c]) tmin = fminf(tmin, acc[r][c]);
      }
      if (tmin < smin[r]) {
        const double drop = (double)smin[r] - (double)tmin;  // +inf the first time: the factor is 0 and the sums are 0
#pragma unroll
        for (int q = 0; q < B; ++q) sum[r][q] *= exp(-p.s.a[q] * drop);
        smin[r] = tmin;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (ok[c]) {
          const double gap = (double)acc[r][c] - (double)smin[r];  // >= 0, exact in double
#pragma unroll
          for (int q = 0; q < B; ++q) sum[r][q] += exp(-p.s.a[q] * gap);
        }
      }
    }
  }

  // ---- the slice's end: the 16 lanes tx of a row are 16 neighbouring lanes of one wave
  const int first = t & 48;  // (of the wave's 64 lanes) the row's lane tx = 0
#pragma unroll
  for (int r = 0; r < TM; ++r) {
    const int i = i0 + ty + 16 * r;
    float mrow = smin[r];
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) mrow = fminf(mrow, __shfl_xor(mrow, s, WM_WAVE));
    const double back = (double)smin[r] - (double)mrow;  // only read where smin[r] is finite (then mrow is)
#pragma unroll
    for (int q = 0; q < B; ++q) {
      const double v = smin[r] < INFINITY ? sum[r][q] * exp(-p.s.a[q] * back) : 0.0;
      double S = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) S += __shfl(v, first + k, WM_WAVE);
      if (tx == 0 && i < m) p.part_sum[((size_t)blockIdx.y * B + q) * m + i] = S;
    }
    if (tx == 0 && i < m) p.part_min[(size_t)blockIdx.y * m + i] = (double)mrow;
  }
}

// The minimum over a row's slices, the slices' sums rescaled to it and added in slice order, then -a M + log S.
__global__ __launch_bounds__(KDE_THREADS) void kde_merge(const double* __restrict__ pmin, const double* __restrict__ psum,
                                                         int slices, int m, int b, KdeScales sc, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * KDE_THREADS + threadIdx.x;
  if (i >= m) return;
  double M = INFINITY;
  for (int s = 0; s < slices; ++s) M = fmin(M, pmin[(size_t)s * m + i]);
  for (int q = 0; q < b; ++q) {
    if (M == INFINITY) {  // no included column
      out[(size_t)q * m + i] = -INFINITY;
      continue;
    }
    const double a = sc.a[q];
    double S = 0.0;
    for (int s = 0; s < slices; ++s) {
      const double ms = pmin[(size_t)s * m + i];
      if (ms < INFINITY) S += psum[((size_t)s * b + q) * m + i] * exp(-a * (ms - M));
    }
    out[(size_t)q * m + i] = -a * M + log(S);
  }
}

struct KdeGrid {
  int row_tiles, col_tiles, slices, tiles_per_slice;
};
// cluster.hip's rule: column slices so that about a thousand workgroups exist; every slice holds at least one tile.
inline KdeGrid kde_grid(int m, int n) {
  KdeGrid g;
  g.row_tiles = wm_cdiv(m, KDE_ROWS);
  g.col_tiles = wm_cdiv(n, KDE_COLS);
  int want = wm_cdiv(1024, g.row_tiles);
  if (want > g.col_tiles) want = g.col_tiles;
  g.tiles_per_slice = wm_cdiv(g.col_tiles, want);
  g.slices = wm_cdiv(g.col_tiles, g.tiles_per_slice);
  return g;
}
inline bool kde_sizes_ok(int m, int n, int d, int b) {
  return m > 0 && m <= KDE_MAX_N && n > 0 && n <= KDE_MAX_N && d > 0 && d % 4 == 0 && d <= 1024 && b >= 1 && b <= KDE_MAXB;
}
// of the planes: [slices][m] minima, then [slices][b][m] sums
inline size_t kde_plane_bytes(const KdeGrid& g, int m, int b) { return (size_t)g.slices * m * (1 + (size_t)b) * sizeof(double); }

}  // namespace

extern "C" size_t wm_kde_logsum_workspace_bytes(int m, int n, int d, int b) {
  if (!kde_sizes_ok(m, n, d, b)) return 0;
  return kde_plane_bytes(kde_grid(m, n), m, b) + 256;
}

extern "C" int wm_kde_logsum(const float* xr, int m, const float* x, int n, int d, const double* inv_two_h2, int b, int self_offset,
                             double* out, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(xr && x && inv_two_h2 && out && workspace, WM_EINVAL);
  WM_REQUIRE(m > 0 && n > 0 && d > 0 && b >= 1 && b <= KDE_MAXB && self_offset >= -1, WM_EINVAL);
  KdeArgs a = {};
  for (int q = 0; q < KDE_MAXB; ++q) {
    a.s.a[q] = q < b ? inv_two_h2[q] : 1.0;
    WM_REQUIRE(a.s.a[q] > 0.0 && a.s.a[q] < (double)INFINITY, WM_EINVAL);  // (a NaN fails the first comparison)
  }
  WM_REQUIRE(kde_sizes_ok(m, n, d, b) && self_offset <= KDE_MAX_N, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(xr, 15) && wm_aligned(x, 15) && wm_aligned(out, 7) && wm_aligned(workspace, 15), WM_EALIGN);
  const KdeGrid g = kde_grid(m, n);
  WM_REQUIRE(workspace_bytes >= kde_plane_bytes(g, m, b), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  a.xr = xr;
  a.x = x;
  a.m = m;
  a.n = n;
  a.d = d;
  a.tiles_per_slice = g.tiles_per_slice;
  a.col_tiles = g.col_tiles;
  a.self_offset = self_offset;
  a.part_min = static_cast<double*>(workspace);
  a.part_sum = a.part_min + (size_t)g.slices * m;
  const dim3 grid(g.row_tiles, g.slices);
  switch (b) {
    case 1: kde_pairs<1><<<grid, KDE_THREADS, 0, st>>>(a); break;
    case 2: kde_pairs<2><<<grid, KDE_THREADS, 0, st>>>(a); break;
    case 3: kde_pairs<3><<<grid, KDE_THREADS, 0, st>>>(a); break;
    default: kde_pairs<4><<<grid, KDE_THREADS, 0, st>>>(a); break;
  }
  WM_LAUNCH_CHECK();
  kde_merge<<<wm_cdiv(m, KDE_THREADS), KDE_THREADS, 0, st>>>(a.part_min, a.part_sum, g.slices, m, b, a.s, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
