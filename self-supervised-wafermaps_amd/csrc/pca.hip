// PCA of an embedding matrix (decomposition.py; sklearn.decomposition.PCA): the passes over the rows.  The d x d
// eigendecomposition is host code; what needs the GPU is
//   wm_pca_mean         column means in float64;
//   wm_pca_gram         sum_i (x_i - mean)(x_i - mean)^T in float64, centred BEFORE it is multiplied (X^T X - n mu mu^T
//                       cancels; cl_dist.h makes the same choice for distances);
//   wm_pca_project      (x - mean) W^T, float32 out;
//   wm_pca_reconstruct  y W + mean, float32 out.
// The last three are one tile routine, pca_tile<MODE>: C[M][N] = sum_k A[m][k] B[k][n] on v_mfma_f64_16x16x4_f64, with
// operands fetched as float32 or float64, widened to double (minus a float64 mean where the mode has one) while they
// are staged, accumulated in double.
//
// ---- the tile routine.  The workgroup tile of f64.h (64 x 64 per workgroup of 4 waves, LDS panels [k][64 + 2] doubles,
// the fragment maps and the tests that settle them are stated there) over ONE slice of K.  K goes in steps of 32 (gram)
// or 16 (project, reconstruct): every thread requests its share of the A and B panels of the NEXT step into registers
// before the MFMAs of the current one, and widens, centres and stores it to LDS behind the barrier that follows.
//   Why 64 x 64 and not wider: a f64 16x16x4 MFMA is 2048 flops over 16 passes, so 4 fragment reads of 8 bytes per 4
//   MFMAs hide behind it; a wider tile would save traffic that is not the limit and would leave d = 512 (8 x 8 tiles, 36
//   on or below the diagonal) with too few tiles to cut.
//   Why K steps of 32 and float4 loads in the Gram pass (measured, 811 457 x 512, profiles/pca.md): with steps of 16 and
//   eight scalar loads per thread and step the pass took 16.2 ms, 14.7 TF: three or four waves per SIMD, each with one
//   step's loads in flight, did not cover the latency of the loads.  Twice the MFMAs per step behind a quarter of the
//   load instructions: 6.4 ms, 37.6 TF, 48 % of the 78.6 TF float64 matrix peak.  The row passes keep steps of 16 (the
//   projection of the same matrix: 1.77 ms with 16, 2.21 ms with 32, whose 16 staged doubles per panel cost a wave of
//   occupancy).
//   Why LDS holds doubles: the widening and the mean subtraction are then done ONCE per staged element (by the thread
//   that fetched it) and not once per MFMA that reads it (each element feeds 2 MFMAs of each of 2 waves), and a
//   fragment read is one ds_read_b64 with no conversion between it and the MFMA.  Cost: 2 panels x 32 x 66 x 8 bytes =
//   33 KB per workgroup (gram; half of it for the row passes): four workgroups in a CU's 160 KB, and the registers
//   (136 with the accumulators) allow three waves per SIMD.
// Padding: a position behind the operand's rows, columns or the slice's end is staged as an exact 0.0 and the mean is
// NOT subtracted there (a padded row centred to -mean would corrupt every entry); stores are guarded by the same limits.
// The Gram pass has no branch around a load: the address of such a position is clamped to the slice's last row / the
// tile's first column, which exist, and the value is dropped when it is staged.
//
// ---- the modes.
//   gram         M = N = d, K = the rows.  Only tiles (ti, tj) with tj <= ti are computed.  The rows are cut into
//                S = min(ceil(1024 / tiles), ceil(n / 256), max(1, 256 MiB / (d d 8))) slices (tiles = T (T + 1) / 2,
//                T = ceil(d / 64)) of ceil(n / S) rows rounded up to a multiple of 32: a function of (n, d) alone, never
//                of the device.  About 1024 workgroups fill the 256 CUs four times over; the workspace is S planes of
//                d x d doubles and stays at or below 256 MiB (d = 512: 29 slices, 58 MiB at most; d = 4096: one slice,
//                128 MiB).  Workgroup (tile, slice) stores its partial tile into plane `slice` with plain stores (one
//                writer per cell); pca_gram_merge adds the planes in slice order and writes out[i][j] and out[j][i]
//                from the SAME cell of the lower triangle, so out is symmetric bit for bit.  No atomics anywhere.
//   project      M = the rows, N = the m components, K = the d features, one slice: the double sum is rounded to
//                float32 once in the epilogue, no merge.
//   reconstruct  M = the rows, N = the d features, K = the m components, one slice: + mean in double, rounded once.
// Order of every sum: k ascending in steps of 4 (one MFMA each; inside an MFMA the hardware's fixed order).  It depends
// on the sizes only, so two calls give the same bits.
//
// ---- the means.  pca_mean_partial: thread (feature f, slab s) adds x[i][f] for the slab's rows in row order, in double
// (64 consecutive features per wave: coalesced); pca_mean_merge adds the slabs' sums in slab order and divides by n in
// double.  Slab size: 256 rows while that gives at most 1024 slabs (n <= 262 144); above, ceil(n / 1024) rounded up to a
// multiple of 256.  The workspace is slabs x d doubles (at most 32 MiB).
#include "f64.h"

namespace {

constexpr int PCA_MAX_N = 1 << 24;
constexpr int PCA_MAX_D = 4096;
constexpr int PCA_KT_GRAM = 32;          // K per staged step of the Gram pass (8 MFMAs deep)
constexpr int PCA_KT_ROWS = 16;          // ... of project / reconstruct (4 deep)
constexpr int PCA_TARGET_WG = 1024;      // workgroups the Gram slice count aims at
constexpr size_t PCA_GRAM_WS_CAP = (size_t)256 << 20;
constexpr int PCA_SLAB = 256;            // rows per slab of the mean
constexpr int PCA_MAX_SLABS = 1024;

enum { PCA_GRAM = 0, PCA_PROJECT = 1, PCA_RECON = 2 };

inline bool pca_nd_ok(int n, int d) { return n >= 1 && n <= PCA_MAX_N && d >= 4 && d % 4 == 0 && d <= PCA_MAX_D; }
inline int pca_slab_rows(int n) {
  if (n <= PCA_SLAB * PCA_MAX_SLABS) return PCA_SLAB;
  const int r = (n + PCA_MAX_SLABS - 1) / PCA_MAX_SLABS;
  return (r + PCA_SLAB - 1) / PCA_SLAB * PCA_SLAB;
}
struct PcaGramShape {
  int T, tiles, slices, slice_rows;
};
inline PcaGramShape pca_gram_shape(int n, int d) {
  PcaGramShape s;
  s.T = (d + F64_TILE - 1) / F64_TILE;
  s.tiles = s.T * (s.T + 1) / 2;
  const F64Slices c = f64_cut(n, (PCA_TARGET_WG + s.tiles - 1) / s.tiles, (n + 255) / 256,
                              (long long)(PCA_GRAM_WS_CAP / ((size_t)d * d * sizeof(double))), PCA_KT_GRAM);
  s.slices = c.slices;
  s.slice_rows = c.slice_rows;
  return s;
}

struct PcaArgs {
  const float* x;      // gram / project: the rows [n][d]; reconstruct: y [n][m]
  const double* w;     // project / reconstruct: W [m][d]
  const double* mean;  // [d] or nullptr
  double* planes;      // gram: [slices][d][d]
  float* out;          // project [n][m], reconstruct [n][d]
  int n, d, m, slice_rows;
};

// A[row of C][k] and B[k][column of C] of each mode as doubles; exact zeros outside the operands (k1: the slice's end).
template <int MODE>
__device__ __forceinline__ double pca_a(const PcaArgs& a, int r, int k, int k1) {
  if constexpr (MODE == PCA_GRAM) {
    if (r >= a.d || k >= k1) return 0.0;
    const double v = (double)a.x[(size_t)k * a.d + r];
    return a.mean ? v - a.mean[r] : v;
  } else if constexpr (MODE == PCA_PROJECT) {
    if (r >= a.n || k >= k1) return 0.0;
    const double v = (double)a.x[(size_t)r * a.d + k];
    return a.mean ? v - a.mean[k] : v;
  } else {
    if (r >= a.n || k >= k1) return 0.0;
    return (double)a.x[(size_t)r * a.m + k];
  }
}
template <int MODE>
__device__ __forceinline__ double pca_b(const PcaArgs& a, int k, int c, int k1) {
  if constexpr (MODE == PCA_GRAM) {
    return pca_a<PCA_GRAM>(a, c, k, k1);
  } else if constexpr (MODE == PCA_PROJECT) {
    if (c >= a.m || k >= k1) return 0.0;
    return a.w[(size_t)c * a.d + k];
  } else {
    if (c >= a.d || k >= k1) return 0.0;
    return a.w[(size_t)k * a.d + c];
  }
}

template <int MODE>
__global__ __launch_bounds__(F64_THREADS) void pca_tile(PcaArgs a) {
  constexpr int PCA_KT = MODE == PCA_GRAM ? PCA_KT_GRAM : PCA_KT_ROWS;
  constexpr int PCA_EL = PCA_KT * F64_TILE / F64_THREADS;  // single elements per thread, panel and step
  __shared__ __attribute__((aligned(16))) double As[PCA_KT][F64_LD];
  __shared__ __attribute__((aligned(16))) double Bs[PCA_KT][F64_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn, k0, k1;
  if constexpr (MODE == PCA_GRAM) {
    f64_tri_tile(blockIdx.x, tm, tn);
    k0 = blockIdx.y * a.slice_rows;
    k1 = min(a.n, k0 + a.slice_rows);
  } else {
    tm = blockIdx.x;
    tn = blockIdx.y;
    k0 = 0;
    k1 = MODE == PCA_PROJECT ? a.d : a.m;
  }
  const int m0 = tm * F64_TILE, n0 = tn * F64_TILE;
  // ---- staging.  fetch(kb) requests the step's elements into registers, stage(kb) widens, centres and stores them.
  // gram: both panels are 64 consecutive floats of a row of x per k.  A thread takes ONE float4 per 16 rows and panel:
  // 16 lanes cover a row's 256 bytes, a wave instruction four rows.  The load's address is clamped into the slice and
  // the tile's first column where the position is outside (no branch around a load; the value is dropped in stage()),
  // and the thread's four means per panel are fetched once, before the loop.
  const int c4 = (t & 15) * 4, kr = t >> 4;
  [[maybe_unused]] bool a_in = false, b_in = false;
  [[maybe_unused]] double ma[4] = {0.0, 0.0, 0.0, 0.0}, mb[4] = {0.0, 0.0, 0.0, 0.0};
  [[maybe_unused]] const float *pa = nullptr, *pb = nullptr;
  [[maybe_unused]] f32x4_t va[PCA_KT / 16], vb[PCA_KT / 16];
  // project / reconstruct: PCA_EL single elements per thread and panel; which index is contiguous in memory decides
  // which one the lanes of a wave walk
  constexpr bool A_K_FAST = MODE != PCA_GRAM, B_K_FAST = MODE == PCA_PROJECT;
  [[maybe_unused]] double ra[PCA_EL], rb[PCA_EL];
  auto ai = [&](int u) { return A_K_FAST ? (t / PCA_KT) + (F64_THREADS / PCA_KT) * u : (t & 63); };
  auto ak = [&](int u) { return A_K_FAST ? (t % PCA_KT) : (t >> 6) + 4 * u; };
  auto bi = [&](int u) { return B_K_FAST ? (t / PCA_KT) + (F64_THREADS / PCA_KT) * u : (t & 63); };
  auto bk = [&](int u) { return B_K_FAST ? (t % PCA_KT) : (t >> 6) + 4 * u; };
  if constexpr (MODE == PCA_GRAM) {
    a_in = m0 + c4 < a.d;  // (d % 4 == 0: a float4 is inside or outside as a whole)
    b_in = n0 + c4 < a.d;
    pa = a.x + (a_in ? m0 + c4 : m0);
    pb = a.x + (b_in ? n0 + c4 : n0);
    if (a.mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a_in) ma[e] = a.mean[m0 + c4 + e];
        if (b_in) mb[e] = a.mean[n0 + c4 + e];
      }
    }
  }
  auto fetch = [&](int kb) {
    if constexpr (MODE == PCA_GRAM) {
#pragma unroll
      for (int u = 0; u < PCA_KT / 16; ++u) {
        const size_t row = (size_t)min(kb + kr + 16 * u, k1 - 1) * a.d;
        va[u] = *reinterpret_cast<const f32x4_t*>(pa + row);
        vb[u] = *reinterpret_cast<const f32x4_t*>(pb + row);
      }
    } else {
#pragma unroll
      for (int u = 0; u < PCA_EL; ++u) {
        ra[u] = pca_a<MODE>(a, m0 + ai(u), kb + ak(u), k1);
        rb[u] = pca_b<MODE>(a, kb + bk(u), n0 + bi(u), k1);
      }
    }
  };
  auto stage = [&](int kb) {
    if constexpr (MODE == PCA_GRAM) {
#pragma unroll
      for (int u = 0; u < PCA_KT / 16; ++u) {
        const bool live = kb + kr + 16 * u < k1;  // behind the slice: exact zeros, the mean NOT subtracted
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          As[kr + 16 * u][c4 + e] = live && a_in ? (double)va[u][e] - ma[e] : 0.0;
          Bs[kr + 16 * u][c4 + e] = live && b_in ? (double)vb[u][e] - mb[e] : 0.0;
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < PCA_EL; ++u) {
        As[ak(u)][ai(u)] = ra[u];
        Bs[bk(u)][bi(u)] = rb[u];
      }
    }
  };
  f64x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  const int fk = lane >> 4, fc = lane & 15;
  fetch(k0);
  for (int kb = k0; kb < k1; kb += PCA_KT) {
    __syncthreads();  // the previous step's fragment reads are done
    stage(kb);
    __syncthreads();
    if (kb + PCA_KT < k1) fetch(kb + PCA_KT);  // in flight during the MFMAs
    // gmm.hip's gm_mma<PCA_KT> written out: as a call of a shared helper the projection of 172 950 x 512 onto 50
    // components took 0.417 ms against 0.407 ms (2.5 %; 0.5 % at 811 457 rows), twice in alternation with this form --
    // same instruction counts, another register allocation (profiles/f64_refactor.md)
#pragma unroll
    for (int kk = 0; kk < PCA_KT / 4; ++kk) {
      double fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = As[4 * kk + fk][wm * 32 + i * 16 + fc];
        fb[i] = Bs[4 * kk + fk][wn * 32 + i * 16 + fc];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 32 + i * 16 + fk + 4 * r, col = n0 + wn * 32 + j * 16 + fc;
        const double v = acc[i][j][r];
        if constexpr (MODE == PCA_GRAM) {
          if (row < a.d && col < a.d) a.planes[((size_t)blockIdx.y * a.d + row) * a.d + col] = v;
        } else if constexpr (MODE == PCA_PROJECT) {
          if (row < a.n && col < a.m) a.out[(size_t)row * a.m + col] = (float)v;
        } else {
          if (row < a.n && col < a.d) a.out[(size_t)row * a.d + col] = (float)(a.mean ? v + a.mean[col] : v);
        }
      }
}

// out[i][j] = sum over the slices, in slice order, of the lower triangle's cell (max(i, j), min(i, j)).
// (gmm.hip's gm_scatter_full_merge at batch 1, kept apart: that kernel pays a 64-bit division per thread for its batch
// index, and with it the Gram pass of 12 449 x 512 was not inside the run-to-run spread -- profiles/f64_refactor.md.)
__global__ __launch_bounds__(F64_THREADS) void pca_gram_merge(const double* __restrict__ planes, int slices, int d,
                                                              double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * F64_THREADS + threadIdx.x;
  if (e >= (long long)d * d) return;
  const int i = (int)(e / d), j = (int)(e - (long long)i * d);
  const size_t cell = (size_t)max(i, j) * d + min(i, j);
  double sum = 0.0;
  for (int s = 0; s < slices; ++s) sum += planes[(size_t)s * d * d + cell];
  out[e] = sum;
}

__global__ __launch_bounds__(64) void pca_mean_partial(const float* __restrict__ x, int n, int d, int slab_rows,
                                                       double* __restrict__ part) {
  const int f = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (f >= d) return;
  const int i0 = s * slab_rows, i1 = min(n, i0 + slab_rows);
  double acc = 0.0;
  for (int i = i0; i < i1; ++i) acc += (double)x[(size_t)i * d + f];
  part[(size_t)s * d + f] = acc;
}

__global__ __launch_bounds__(64) void pca_mean_merge(const double* __restrict__ part, int slabs, int n, int d,
                                                     double* __restrict__ mean) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= d) return;
  double sum = 0.0;
  for (int s = 0; s < slabs; ++s) sum += part[(size_t)s * d + f];
  mean[f] = sum / (double)n;
}

}  // namespace

extern "C" size_t wm_pca_mean_workspace_bytes(int n, int d) {
  if (!pca_nd_ok(n, d)) return 0;
  const int rows = pca_slab_rows(n);
  return (size_t)((n + rows - 1) / rows) * d * sizeof(double);
}

extern "C" int wm_pca_mean(const float* x, int n, int d, double* mean_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
  WM_REQUIRE(x && mean_out && workspace && n > 0 && d > 0, WM_EINVAL);
  WM_REQUIRE(pca_nd_ok(n, d), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 3) && wm_aligned(mean_out, 7) && wm_aligned(workspace, 15), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_pca_mean_workspace_bytes(n, d), WM_EWORKSPACE);
  const int rows = pca_slab_rows(n), slabs = (n + rows - 1) / rows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  pca_mean_partial<<<dim3((d + 63) / 64, slabs), 64, 0, st>>>(x, n, d, rows, part);
  WM_LAUNCH_CHECK();
  pca_mean_merge<<<(d + 63) / 64, 64, 0, st>>>(part, slabs, n, d, mean_out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_pca_gram_workspace_bytes(int n, int d) {
  if (!pca_nd_ok(n, d)) return 0;
  return (size_t)pca_gram_shape(n, d).slices * d * d * sizeof(double);
}

extern "C" int wm_pca_gram(const float* x, int n, int d, const double* mean, double* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && out && workspace && n > 0 && d > 0, WM_EINVAL);
  WM_REQUIRE(pca_nd_ok(n, d), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(mean, 7) && wm_aligned(out, 7) && wm_aligned(workspace, 15), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_pca_gram_workspace_bytes(n, d), WM_EWORKSPACE);
  const PcaGramShape s = pca_gram_shape(n, d);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PcaArgs a{x, nullptr, mean, static_cast<double*>(workspace), nullptr, n, d, 0, s.slice_rows};
  pca_tile<PCA_GRAM><<<dim3(s.tiles, s.slices), F64_THREADS, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  pca_gram_merge<<<(int)(((long long)d * d + F64_THREADS - 1) / F64_THREADS), F64_THREADS, 0, st>>>(a.planes, s.slices, d, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_pca_project_workspace_bytes(int n, int d, int m) {
  return pca_nd_ok(n, d) && m >= 1 && m <= d ? WM_TOKEN_WS : 0;
}

extern "C" int wm_pca_project(const float* x, int n, int d, const double* mean, const double* w, int m, float* out,
                              void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && w && out && workspace && n > 0 && d > 0 && m > 0, WM_EINVAL);
  WM_REQUIRE(pca_nd_ok(n, d) && m <= d, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 3) && wm_aligned(mean, 7) && wm_aligned(w, 7) && wm_aligned(out, 3), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PcaArgs a{x, w, mean, nullptr, out, n, d, m, 0};
  pca_tile<PCA_PROJECT><<<dim3((n + F64_TILE - 1) / F64_TILE, (m + F64_TILE - 1) / F64_TILE), F64_THREADS, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_pca_reconstruct_workspace_bytes(int n, int m, int d) {
  return pca_nd_ok(n, d) && m >= 1 && m <= d ? WM_TOKEN_WS : 0;
}

extern "C" int wm_pca_reconstruct(const float* y, int n, int m, const double* w, int d, const double* mean, float* out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(y && w && out && workspace && n > 0 && d > 0 && m > 0, WM_EINVAL);
  WM_REQUIRE(pca_nd_ok(n, d) && m <= d, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(y, 3) && wm_aligned(mean, 7) && wm_aligned(w, 7) && wm_aligned(out, 3), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PcaArgs a{y, w, mean, nullptr, out, n, d, m, 0};
  pca_tile<PCA_RECON><<<dim3((n + F64_TILE - 1) / F64_TILE, (d + F64_TILE - 1) / F64_TILE), F64_THREADS, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
