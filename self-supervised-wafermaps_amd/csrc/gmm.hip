// Gaussian mixture on an embedding matrix (mixture.py; sklearn.mixture.GaussianMixture): the passes over the rows of
// the E-step and the M-step, all in float64 on float32 rows.  The Cholesky factors of the k covariance matrices, their
// triangular inverses and the log-determinants are host code (k d^3 / 3 flops, small next to one E-step).
//   E-step   wm_gmm_logprob_diag   out[i][c] = cst[c] - 0.5 sum_f (x_if - mean_cf)^2 inv_var_cf          (VALU)
//            wm_gmm_logprob_full   out[i][c] = cst[c] - 0.5 ||(x_i - mean_c) P_c||^2, P_c upper triangular (MFMA)
//            wm_gmm_normalize      log-sum-exp per row, responsibilities, labels, the sum of the rows' log-likelihoods
//   M-step   wm_gmm_weighted_sums  nk = resp^T 1, sx = resp^T x                                            (MFMA)
//            wm_gmm_scatter_diag   sum_i resp_ic (x_if - mean_cf)^2                                        (VALU)
//            wm_gmm_scatter_full   sum_i resp_ic (x_i - mean_c)(x_i - mean_c)^T                            (MFMA)
// Two passes over the rows in the M-step (sums, then the scatter centred on the NEW mean) and a row that is centred
// BEFORE it is multiplied in the E-step: avg_X2 - 2 avg_X mu + mu^2 and x P - mu P cancel (pca.hip and cl_dist.h make
// the same choice).
//
// ---- operands.  x is float32 [n][ld] with the true feature count d <= ld, ld % 4 == 0.  Whatever columns d .. ld-1
// hold is never loaded: a position f >= d is staged as an exact 0.0 (the mean is NOT subtracted there) and takes part
// in nothing.  That matters here as it does not for distances: a padded column that reached a covariance would add
// log reg_covar to every log-determinant.  The parameters are float64 with pitch d.
//
// ---- the MFMA kernels run on the workgroup tile of f64.h (64 x 64 per workgroup, panels [k][64 + 2] doubles in LDS,
// the fragment maps and the order of the sum over k are stated there).  An element is widened, centred and
// (scatter_full) weighted ONCE, by the thread that fetched it.
//
//   logprob_full    grid (row tiles, k).  M = 64 rows, N = K = d.  The workgroup walks the column tiles tn = 0, 1, ..
//                   in ascending order; column tile tn needs only K < min(d, 64 tn + 64), because P_c[f][j] with f > j
//                   is never read: tiles wholly below the diagonal are skipped (half the work at d = 256) and the
//                   straddling tile stages zeros there.  After a column tile every lane squares its 2 x 2 x 4
//                   accumulators and adds them to its 8 row sums (j ascending); at the end the 32 lane sums of a row go
//                   through LDS and are added in (column half, lane) order.  K steps of 16, as pca.hip's row passes.
//                   The A panel is fetched again for every column tile (at most 4 times; the rows of a tile stay in L2)
//                   rather than kept whole in LDS (64 x 256 doubles = 128 KB would leave one workgroup per CU).  The
//                   stores of out[i][c] are strided by k doubles: not measured against a transposed store.  Measured
//                   (profiles/gmm.md, k = 50, d = 50): 0.194 ms on 12 449 rows, 2.60 ms on 172 950, 26 - 27 TF of executed
//                   MFMA work = 34 % of the 78.6 TF peak, 1.2 x fifty wm_pca_project calls at m = d on the large matrix;
//                   156 registers leave 2 waves per SIMD.
//   weighted_sums   M = the k components, N = d + 1 columns (column d of B is an exact 1.0: nk comes out of the same
//                   product, in the same order as sx), K = the rows in steps of 32.  Grid (component tiles, column
//                   tiles, slices).  The rows are cut into S = min(ceil(1024 / column tiles), ceil(n / 256),
//                   max(1, 256 MiB / (1024 (d + 1) 8))) slices of ceil(n / S) rows rounded up to a multiple of 32: a
//                   function of (n, d) alone -- NOT of k, so a component's sums are the same bits alone and among
//                   others -- and never of the device.  The byte cap uses the LARGEST k, which keeps the workspace
//                   (S planes of k x (d + 1) doubles) at or below 256 MiB for every k.  The merge adds the planes in
//                   slice order.
//   scatter_full    per component the weighted centred Gram: A[r][i] = resp_ic * (x_ir - mean_cr) (one rounding for the
//                   difference, one for the product), B[i][c'] = x_ic' - mean_cc'.  Grid (tiles on and below the
//                   diagonal, slices, components of a batch).  S = min(ceil(1024 / tiles), ceil(n / 256),
//                   max(1, 256 MiB / (d d 8))): a function of (n, d) alone.  The components are taken in batches of
//                   max(1, 256 MiB / (S d d 8)) so that the planes [S][batch][d][d] stay at or below 256 MiB; batches
//                   run one after the other on the stream.  The merge adds the planes in slice order and writes
//                   out[c][i][j] and out[c][j][i] from the SAME cell of the lower triangle: symmetric bit for bit.
//   The K = rows passes fetch single elements under a branch (64 consecutive floats / doubles per wave instruction,
//   coalesced), not pca.hip's clamped float4 form: the resp panel has pitch k, which is not a multiple of anything.
//   What that costs against the float4 form is not measured; the passes themselves (profiles/gmm.md, k = 50, d = 50,
//   172 950 rows): weighted_sums 0.207 ms, scatter_full 3.62 ms = 20 TF of executed MFMA work, 25 % of the peak.
//
// ---- the VALU kernels.
//   logprob_diag    a workgroup of 256 threads owns 64 rows x 64 components; thread (ty, tx) owns rows 4 ty + u and
//                   components tx + 16 v as a 4 x 4 register tile.  Steps of 16 features: x, mean and inv_var panels
//                   staged in LDS as doubles ([f][64 + 2]); a thread reads 4 + 4 + 4 doubles per feature for 16
//                   (subtract, multiply, multiply, add).  One accumulator per output, f ascending.  12 flops per 96 LDS
//                   bytes: the LDS reads, not the float64 VALU, are the likely limit; not measured.
//   scatter_diag    a workgroup is ONE wave and owns (64-feature chunk, tile of 16 components, slab of rows).  Lane l
//                   owns feature 64 chunk + l and walks the slab's rows in row order; the 16 accumulators and means are
//                   registers, the row's 16 responsibilities are wave-uniform loads.  Slabs: S = min(ceil(512 / chunks),
//                   ceil(n / 64), max(1, 256 MiB / (1024 d 8))) of ceil(n / S) rows: a function of (n, d) alone.  The
//                   fold adds the slabs in slab order.  Every component tile reads the slab's rows again (k / 16 times,
//                   from L2): not measured against a wider tile.
//   normalize       a thread per row, three walks over the row's k doubles (max and argmax; sum of exp in component
//                   order; the responsibilities).  A workgroup is a slab of 256 rows and adds its 256 lpn in a fixed
//                   tree; one more workgroup adds the slabs' sums in slab order (thread t a run of consecutive slabs,
//                   thread 0 the 256 run sums).  A lane's row is k doubles away from its neighbour's, so the loads do
//                   not coalesce; the rows are short (k <= 1024) and walked three times out of L1 / L2.  Not measured
//                   against a transposing LDS stage.
#include "f64.h"
#include "rows_sums.h"

namespace {

constexpr int GM_MAX_N = 1 << 24;
constexpr int GM_MAX_K = 1024;
constexpr int GM_MAX_D_DIAG = 1024;
constexpr int GM_MAX_D_FULL = 256;
constexpr int GM_TILE = F64_TILE;   // logprob_diag's VALU tile has the MFMA tile's shape, pitch and thread count
constexpr int GM_LD = F64_LD;
constexpr int GM_THREADS = F64_THREADS;
constexpr int GM_KT_FEAT = 16;      // K per staged step where K = the features
constexpr int GM_KT_ROWS = 32;      // ... where K = the rows
constexpr int GM_TARGET_WG = 1024;
constexpr size_t GM_WS_CAP = (size_t)256 << 20;
constexpr int GM_CT = 16;           // components per tile of scatter_diag
constexpr int GM_SLAB_TARGET = 512;
constexpr int GM_NORM_SLAB = 256;

inline bool gm_ok(int n, int d, int ld, int k, int dmax) {
  return n >= 1 && n <= GM_MAX_N && k >= 1 && k <= GM_MAX_K && d >= 1 && d <= dmax && ld >= d && ld % 4 == 0 &&
         ld <= dmax + 3;
}

inline F64Slices gm_wsum_shape(int n, int d) {
  const int tn = (d + 1 + GM_TILE - 1) / GM_TILE;
  return f64_cut(n, (GM_TARGET_WG + tn - 1) / tn, (n + 255) / 256,
                 (long long)(GM_WS_CAP / ((size_t)GM_MAX_K * (d + 1) * sizeof(double))), GM_KT_ROWS);
}
struct GmScatterShape {
  int tiles, slices, slice_rows, batch;
};
inline GmScatterShape gm_scatter_full_shape(int n, int d, int k) {
  GmScatterShape s;
  const int T = (d + GM_TILE - 1) / GM_TILE;
  s.tiles = T * (T + 1) / 2;
  const size_t plane = (size_t)d * d * sizeof(double);
  const F64Slices c = f64_cut(n, (GM_TARGET_WG + s.tiles - 1) / s.tiles, (n + 255) / 256, (long long)(GM_WS_CAP / plane),
                              GM_KT_ROWS);
  s.slices = c.slices;
  s.slice_rows = c.slice_rows;
  long long b = (long long)(GM_WS_CAP / (plane * c.slices));
  if (b < 1) b = 1;
  s.batch = (int)(b < k ? b : k);
  return s;
}
inline F64Slices gm_scatter_diag_shape(int n, int d) {
  const int chunks = (d + 63) / 64;
  return f64_cut(n, (GM_SLAB_TARGET + chunks - 1) / chunks, (n + 63) / 64,
                 (long long)(GM_WS_CAP / ((size_t)GM_MAX_K * d * sizeof(double))), 1);
}

// One staged step of a workgroup's 64 x 64 tile: KT / 4 MFMAs deep, 2 x 2 tiles per wave.  (pca_tile has this loop
// written out: as a call of this function, shared, its projection measured 0.5 - 2.5 % slower, profiles/f64_refactor.md.)
template <int KT>
__device__ __forceinline__ void gm_mma(const double (*As)[GM_LD], const double (*Bs)[GM_LD], f64x4_t (&acc)[2][2], int wm,
                                       int wn, int fk, int fc) {
#pragma unroll
  for (int kk = 0; kk < KT / 4; ++kk) {
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

// ------------------------------------------------------------------------------------------------ E-step

__global__ __launch_bounds__(GM_THREADS) void gm_logprob_diag(const float* __restrict__ x, int n, int d, int ld,
                                                              const double* __restrict__ mean,
                                                              const double* __restrict__ inv_var,
                                                              const double* __restrict__ cst, int k,
                                                              double* __restrict__ out) {
  constexpr int KT = GM_KT_FEAT, EL = KT * GM_TILE / GM_THREADS;
  __shared__ double Xs[KT][GM_LD];
  __shared__ double Ms[KT][GM_LD];
  __shared__ double Vs[KT][GM_LD];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int m0 = blockIdx.x * GM_TILE, c0 = blockIdx.y * GM_TILE;
  const int sf = t % KT, si = t / KT;  // staging: feature sf of tile entries si + 16 u (the features are contiguous in memory)
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int kb = 0; kb < d; kb += KT) {
    double rx[EL], rm[EL], rv[EL];
    const int f = kb + sf;
#pragma unroll
    for (int u = 0; u < EL; ++u) {
      const int row = m0 + si + (GM_THREADS / KT) * u, c = c0 + si + (GM_THREADS / KT) * u;
      rx[u] = f < d && row < n ? (double)x[(size_t)row * ld + f] : 0.0;
      rm[u] = f < d && c < k ? mean[(size_t)c * d + f] : 0.0;
      rv[u] = f < d && c < k ? inv_var[(size_t)c * d + f] : 0.0;
    }
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int u = 0; u < EL; ++u) {
      Xs[sf][si + (GM_THREADS / KT) * u] = rx[u];
      Ms[sf][si + (GM_THREADS / KT) * u] = rm[u];
      Vs[sf][si + (GM_THREADS / KT) * u] = rv[u];
    }
    __syncthreads();
#pragma unroll
    for (int ff = 0; ff < KT; ++ff) {
      double xv[4], mv[4], iv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = Xs[ff][ty * 4 + u];
        mv[u] = Ms[ff][tx + 16 * u];
        iv[u] = Vs[ff][tx + 16 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double df = xv[u] - mv[v];
          acc[u][v] += df * df * iv[v];
        }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = m0 + ty * 4 + u, c = c0 + tx + 16 * v;
      if (row < n && c < k) out[(size_t)row * k + c] = cst[c] - 0.5 * acc[u][v];
    }
}

__global__ __launch_bounds__(GM_THREADS) void gm_logprob_full(const float* __restrict__ x, int n, int d, int ld,
                                                              const double* __restrict__ mean,
                                                              const double* __restrict__ pchol,
                                                              const double* __restrict__ cst, int k,
                                                              double* __restrict__ out) {
  constexpr int KT = GM_KT_FEAT, EL = KT * GM_TILE / GM_THREADS;
  __shared__ __attribute__((aligned(16))) double As[KT][GM_LD];
  __shared__ __attribute__((aligned(16))) double Bs[KT][GM_LD];
  __shared__ double red[GM_TILE][33];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, fk = lane >> 4, fc = lane & 15;
  const int c = blockIdx.y, m0 = blockIdx.x * GM_TILE;
  const double* __restrict__ mu = mean + (size_t)c * d;
  const double* __restrict__ P = pchol + (size_t)c * d * d;
  // A: the features are contiguous (thread: feature t % 16 of rows t / 16 + 16 u); B: the columns are (thread: column
  // t & 63 of features (t >> 6) + 4 u)
  const int af = t % KT, ar = t / KT, bc = t & 63, bf = t >> 6;
  double rs[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[i][r] = 0.0;
  const int T = (d + GM_TILE - 1) / GM_TILE;
  for (int tn = 0; tn < T; ++tn) {
    const int n0 = tn * GM_TILE, k1 = min(d, n0 + GM_TILE);  // features behind the tile's last column meet zeros only
    double ra[EL], rb[EL];
    auto fetch = [&](int kb) {
#pragma unroll
      for (int u = 0; u < EL; ++u) {
        const int row = m0 + ar + (GM_THREADS / KT) * u, f = kb + af;
        ra[u] = row < n && f < k1 ? (double)x[(size_t)row * ld + f] - mu[f] : 0.0;
        const int col = n0 + bc, g = kb + bf + 4 * u;
        rb[u] = col < d && g <= col && g < k1 ? P[(size_t)g * d + col] : 0.0;
      }
    };
    f64x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int kb = 0; kb < k1; kb += KT) {
      __syncthreads();
#pragma unroll
      for (int u = 0; u < EL; ++u) {
        As[af][ar + (GM_THREADS / KT) * u] = ra[u];
        Bs[bf + 4 * u][bc] = rb[u];
      }
      __syncthreads();
      if (kb + KT < k1) fetch(kb + KT);
      gm_mma<KT>(As, Bs, acc, wm, wn, fk, fc);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) rs[i][r] += acc[i][j][r] * acc[i][j][r];
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wm * 32 + i * 16 + fk + 4 * r][wn * 16 + fc] = rs[i][r];
  __syncthreads();
  if (t < GM_TILE && m0 + t < n) {
    double s = 0.0;
    for (int q = 0; q < 32; ++q) s += red[t][q];
    out[(size_t)(m0 + t) * k + c] = cst[c] - 0.5 * s;
  }
}

__global__ __launch_bounds__(GM_THREADS) void gm_normalize(double* __restrict__ wlp, int n, int k, double* __restrict__ lpn,
                                                           int* __restrict__ label, double* __restrict__ part) {
  __shared__ double sh[GM_THREADS];
  const int i = blockIdx.x * GM_NORM_SLAB + threadIdx.x;
  double lp = 0.0;
  if (i < n) {
    double* __restrict__ row = wlp + (size_t)i * k;
    double m = row[0];
    int arg = 0;
    for (int c = 1; c < k; ++c) {
      const double v = row[c];
      if (v > m) m = v, arg = c;
    }
    double s = 0.0;
    for (int c = 0; c < k; ++c) s += exp(row[c] - m);
    lp = m + log(s);
    for (int c = 0; c < k; ++c) row[c] = exp(row[c] - lp);
    lpn[i] = lp;
    label[i] = arg;
  }
  const double tot = block_tree_sum<GM_THREADS>(lp, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// One workgroup: thread t adds its run of ceil(count / 256) consecutive values in order, thread 0 the 256 run sums.
// (kmeans.hip's km_ordered_sum without the offsets.  As a call of that function wm_gmm_normalize took 1.3 - 1.7 us
// longer per call, 0.7 % .. 5 %: its thread 0 also stores every running total for the offsets' sake --
// profiles/f64_refactor.md.)
__global__ __launch_bounds__(GM_THREADS) void gm_ordered_total(const double* __restrict__ v, int count, double* __restrict__ out) {
  __shared__ double sh[GM_THREADS];
  const int t = threadIdx.x;
  const int run = (count + GM_THREADS - 1) / GM_THREADS;
  const int b0 = min(count, t * run), b1 = min(count, b0 + run);
  double mine = 0.0;
  for (int b = b0; b < b1; ++b) mine += v[b];
  sh[t] = mine;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int q = 0; q < GM_THREADS; ++q) tot += sh[q];
    *out = tot;
  }
}

// ------------------------------------------------------------------------------------------------ M-step

enum { GM_WSUM = 0, GM_SCATTER = 1 };

struct GmRowsArgs {
  const float* x;
  const double* resp;
  const double* mean;  // scatter: [k][d]
  double* planes;      // wsum: [slices][k][d + 1]; scatter: [slices][batch][d][d]
  int n, d, ld, k, slice_rows, c0;  // c0: the batch's first component (scatter)
};

template <int MODE>
__global__ __launch_bounds__(GM_THREADS) void gm_rows_tile(GmRowsArgs a) {
  constexpr int KT = GM_KT_ROWS, EL = KT * GM_TILE / GM_THREADS;
  __shared__ __attribute__((aligned(16))) double As[KT][GM_LD];
  __shared__ __attribute__((aligned(16))) double Bs[KT][GM_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, fk = lane >> 4, fc = lane & 15;
  int tm, tn, slice, comp = 0;
  if constexpr (MODE == GM_WSUM) {
    tm = blockIdx.x, tn = blockIdx.y, slice = blockIdx.z;
  } else {
    f64_tri_tile(blockIdx.x, tm, tn);
    slice = blockIdx.y;
    comp = a.c0 + blockIdx.z;
  }
  const int k0 = slice * a.slice_rows, k1 = min(a.n, k0 + a.slice_rows);
  const int m0 = tm * GM_TILE, n0 = tn * GM_TILE;
  // a thread stages tile entry t & 63 of rows (t >> 6) + 4 u: 64 consecutive doubles / floats per wave instruction
  const int idx = t & 63, kq = t >> 6;
  const int ai = m0 + idx, bi = n0 + idx;
  const bool a_in = ai < (MODE == GM_WSUM ? a.k : a.d), b_in = bi < a.d;
  [[maybe_unused]] const bool b_one = bi == a.d;
  [[maybe_unused]] double ma = 0.0, mb = 0.0;
  if constexpr (MODE == GM_SCATTER) {
    if (a_in) ma = a.mean[(size_t)comp * a.d + ai];
    if (b_in) mb = a.mean[(size_t)comp * a.d + bi];
  }
  double ra[EL], rb[EL];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < EL; ++u) {
      const int i = kb + kq + 4 * u;
      const bool live = i < k1;  // behind the slice: exact zeros
      if constexpr (MODE == GM_WSUM) {
        ra[u] = live && a_in ? a.resp[(size_t)i * a.k + ai] : 0.0;
        rb[u] = live ? (b_in ? (double)a.x[(size_t)i * a.ld + bi] : (b_one ? 1.0 : 0.0)) : 0.0;
      } else {
        const double r = live ? a.resp[(size_t)i * a.k + comp] : 0.0;
        const double da = live && a_in ? (double)a.x[(size_t)i * a.ld + ai] - ma : 0.0;
        ra[u] = r * da;
        rb[u] = live && b_in ? (double)a.x[(size_t)i * a.ld + bi] - mb : 0.0;
      }
    }
  };
  f64x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  fetch(k0);
  for (int kb = k0; kb < k1; kb += KT) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < EL; ++u) {
      As[kq + 4 * u][idx] = ra[u];
      Bs[kq + 4 * u][idx] = rb[u];
    }
    __syncthreads();
    if (kb + KT < k1) fetch(kb + KT);
    gm_mma<KT>(As, Bs, acc, wm, wn, fk, fc);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 32 + i * 16 + fk + 4 * r, col = n0 + wn * 32 + j * 16 + fc;
        const double v = acc[i][j][r];
        if constexpr (MODE == GM_WSUM) {
          const int W = a.d + 1;
          if (row < a.k && col < W) a.planes[((size_t)slice * a.k + row) * W + col] = v;
        } else {
          if (row < a.d && col < a.d)
            a.planes[(((size_t)slice * gridDim.z + blockIdx.z) * a.d + row) * a.d + col] = v;
        }
      }
}

// The planes [slices][k][d + 1] added in slice order: columns 0 .. d-1 -> sx (pitch sx_ld), column d -> nk (pitch
// nk_ld; wm_logreg_gradient stores both into one array of pitch d + 1, which the two pointers may not be told apart by).
__global__ __launch_bounds__(GM_THREADS) void gm_wsum_merge(const double* __restrict__ planes, int slices, int k, int d,
                                                            double* nk, int nk_ld, double* sx, int sx_ld) {
  const int W = d + 1;
  const long long e = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
  if (e >= (long long)k * W) return;
  const int c = (int)(e / W), f = (int)(e - (long long)c * W);
  double sum = 0.0;
  for (int s = 0; s < slices; ++s) sum += planes[(size_t)s * k * W + e];
  if (f < d) sx[(size_t)c * sx_ld + f] = sum;
  else nk[(size_t)c * nk_ld] = sum;
}

// out[c][i][j] = the sum over the slices, in slice order, of the lower triangle's cell (max(i, j), min(i, j)).
__global__ __launch_bounds__(GM_THREADS) void gm_scatter_full_merge(const double* __restrict__ planes, int slices, int batch,
                                                                    int d, double* __restrict__ out) {
  const long long dd = (long long)d * d;
  const long long e = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
  if (e >= dd * batch) return;
  const int cb = (int)(e / dd);
  const int q = (int)(e - cb * dd);
  const int i = q / d, j = q - i * d;
  const size_t cell = (size_t)cb * dd + (size_t)max(i, j) * d + min(i, j);
  double sum = 0.0;
  for (int s = 0; s < slices; ++s) sum += planes[(size_t)s * batch * dd + cell];
  out[e] = sum;
}

__global__ __launch_bounds__(64) void gm_scatter_diag_partial(const float* __restrict__ x, int n, int d, int ld,
                                                              const double* __restrict__ resp, int k,
                                                              const double* __restrict__ mean, int rows_per_slab, int ctiles,
                                                              double* __restrict__ part) {
  const int lane = threadIdx.x;
  const int chunk = blockIdx.x / ctiles, ct = blockIdx.x - chunk * ctiles, s = blockIdx.y;
  const int f = chunk * 64 + lane;
  const bool live = f < d;
  const int fe = live ? f : d - 1;  // (a lane behind d reads the last feature into sums nobody stores)
  const int c0 = ct * GM_CT;
  double acc[GM_CT], mu[GM_CT];
  int cc[GM_CT];
#pragma unroll
  for (int c = 0; c < GM_CT; ++c) {
    cc[c] = min(c0 + c, k - 1);  // (a component behind k repeats the last one, not stored either)
    acc[c] = 0.0;
    mu[c] = mean[(size_t)cc[c] * d + fe];
  }
  const int i0 = s * rows_per_slab, i1 = min(n, i0 + rows_per_slab);
  for (int i = i0; i < i1; ++i) {
    const double xv = (double)x[(size_t)i * ld + fe];
    const double* __restrict__ r = resp + (size_t)i * k;
#pragma unroll
    for (int c = 0; c < GM_CT; ++c) {
      const double df = xv - mu[c];
      acc[c] += r[cc[c]] * (df * df);
    }
  }
  if (live) {
#pragma unroll
    for (int c = 0; c < GM_CT; ++c)
      if (c0 + c < k) part[((size_t)s * k + c0 + c) * d + f] = acc[c];
  }
}

__global__ __launch_bounds__(GM_THREADS) void gm_slab_fold(const double* __restrict__ part, int slabs, long long cells,
                                                           double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
  if (e >= cells) return;
  double sum = 0.0;
  for (int s = 0; s < slabs; ++s) sum += part[(size_t)s * cells + e];
  out[e] = sum;
}

}  // namespace

extern "C" size_t wm_gmm_logprob_diag_workspace_bytes(int n, int d, int ld, int k) {
  return gm_ok(n, d, ld, k, GM_MAX_D_DIAG) ? WM_TOKEN_WS : 0;
}

extern "C" int wm_gmm_logprob_diag(const float* x, int n, int d, int ld, const double* mean, const double* inv_var,
                                   const double* cst, int k, double* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  WM_REQUIRE(x && mean && inv_var && cst && out && workspace && n > 0 && d > 0 && k > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(gm_ok(n, d, ld, k, GM_MAX_D_DIAG), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(mean, 7) && wm_aligned(inv_var, 7) && wm_aligned(cst, 7) && wm_aligned(out, 7),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  gm_logprob_diag<<<dim3((n + GM_TILE - 1) / GM_TILE, (k + GM_TILE - 1) / GM_TILE), GM_THREADS, 0, st>>>(x, n, d, ld, mean,
                                                                                                       inv_var, cst, k, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_gmm_logprob_full_workspace_bytes(int n, int d, int ld, int k) {
  return gm_ok(n, d, ld, k, GM_MAX_D_FULL) ? WM_TOKEN_WS : 0;
}

extern "C" int wm_gmm_logprob_full(const float* x, int n, int d, int ld, const double* mean, const double* pchol,
                                   const double* cst, int k, double* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  WM_REQUIRE(x && mean && pchol && cst && out && workspace && n > 0 && d > 0 && k > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(gm_ok(n, d, ld, k, GM_MAX_D_FULL), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(mean, 7) && wm_aligned(pchol, 7) && wm_aligned(cst, 7) && wm_aligned(out, 7),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  gm_logprob_full<<<dim3((n + GM_TILE - 1) / GM_TILE, k), GM_THREADS, 0, st>>>(x, n, d, ld, mean, pchol, cst, k, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_gmm_normalize_workspace_bytes(int n, int k) {
  if (n < 1 || n > GM_MAX_N || k < 1 || k > GM_MAX_K) return 0;
  return (size_t)((n + GM_NORM_SLAB - 1) / GM_NORM_SLAB) * sizeof(double);
}

extern "C" int wm_gmm_normalize(double* wlp_inout, int n, int k, double* lpn, int32_t* label, double* lpn_sum,
                                void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(wlp_inout && lpn && label && lpn_sum && workspace && n > 0 && k > 0, WM_EINVAL);
  WM_REQUIRE(n <= GM_MAX_N && k <= GM_MAX_K, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(wlp_inout, 7) && wm_aligned(lpn, 7) && wm_aligned(label, 3) && wm_aligned(lpn_sum, 7) &&
                 wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_gmm_normalize_workspace_bytes(n, k), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = (n + GM_NORM_SLAB - 1) / GM_NORM_SLAB;
  double* part = static_cast<double*>(workspace);
  gm_normalize<<<slabs, GM_THREADS, 0, st>>>(wlp_inout, n, k, lpn, label, part);
  WM_LAUNCH_CHECK();
  gm_ordered_total<<<1, GM_THREADS, 0, st>>>(part, slabs, lpn_sum);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

size_t wm_rows_sums_workspace_bytes(int n, int d, int ld, int k) {
  if (!gm_ok(n, d, ld, k, GM_MAX_D_DIAG)) return 0;
  return (size_t)gm_wsum_shape(n, d).slices * k * (d + 1) * sizeof(double);
}

int wm_rows_sums_launch(const float* x, int n, int d, int ld, const double* resp, int k, double* nk, int nk_ld, double* sx,
                        int sx_ld, void* workspace, hipStream_t st) {
  const F64Slices s = gm_wsum_shape(n, d);
  GmRowsArgs a{x, resp, nullptr, static_cast<double*>(workspace), n, d, ld, k, s.slice_rows, 0};
  gm_rows_tile<GM_WSUM><<<dim3((k + GM_TILE - 1) / GM_TILE, (d + 1 + GM_TILE - 1) / GM_TILE, s.slices), GM_THREADS, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  const long long cells = (long long)k * (d + 1);
  gm_wsum_merge<<<(int)((cells + GM_THREADS - 1) / GM_THREADS), GM_THREADS, 0, st>>>(a.planes, s.slices, k, d, nk, nk_ld, sx,
                                                                                   sx_ld);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_gmm_weighted_sums_workspace_bytes(int n, int d, int ld, int k) {
  return wm_rows_sums_workspace_bytes(n, d, ld, k);
}

extern "C" int wm_gmm_weighted_sums(const float* x, int n, int d, int ld, const double* resp, int k, double* nk, double* sx,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && resp && nk && sx && workspace && n > 0 && d > 0 && k > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(gm_ok(n, d, ld, k, GM_MAX_D_DIAG), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(resp, 7) && wm_aligned(nk, 7) && wm_aligned(sx, 7) && wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_gmm_weighted_sums_workspace_bytes(n, d, ld, k), WM_EWORKSPACE);
  return wm_rows_sums_launch(x, n, d, ld, resp, k, nk, 1, sx, d, workspace, static_cast<hipStream_t>(stream));
}

extern "C" size_t wm_gmm_scatter_diag_workspace_bytes(int n, int d, int ld, int k) {
  if (!gm_ok(n, d, ld, k, GM_MAX_D_DIAG)) return 0;
  return (size_t)gm_scatter_diag_shape(n, d).slices * k * d * sizeof(double);
}

extern "C" int wm_gmm_scatter_diag(const float* x, int n, int d, int ld, const double* resp, int k, const double* mean,
                                   double* out, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && resp && mean && out && workspace && n > 0 && d > 0 && k > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(gm_ok(n, d, ld, k, GM_MAX_D_DIAG), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(resp, 7) && wm_aligned(mean, 7) && wm_aligned(out, 7) && wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_gmm_scatter_diag_workspace_bytes(n, d, ld, k), WM_EWORKSPACE);
  const F64Slices s = gm_scatter_diag_shape(n, d);
  const int chunks = (d + 63) / 64, ctiles = (k + GM_CT - 1) / GM_CT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  gm_scatter_diag_partial<<<dim3(chunks * ctiles, s.slices), 64, 0, st>>>(x, n, d, ld, resp, k, mean, s.slice_rows, ctiles, part);
  WM_LAUNCH_CHECK();
  const long long cells = (long long)k * d;
  gm_slab_fold<<<(int)((cells + GM_THREADS - 1) / GM_THREADS), GM_THREADS, 0, st>>>(part, s.slices, cells, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_gmm_scatter_full_workspace_bytes(int n, int d, int ld, int k) {
  if (!gm_ok(n, d, ld, k, GM_MAX_D_FULL)) return 0;
  const GmScatterShape s = gm_scatter_full_shape(n, d, k);
  return (size_t)s.slices * s.batch * d * d * sizeof(double);
}

extern "C" int wm_gmm_scatter_full(const float* x, int n, int d, int ld, const double* resp, int k, const double* mean,
                                   double* out, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && resp && mean && out && workspace && n > 0 && d > 0 && k > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(gm_ok(n, d, ld, k, GM_MAX_D_FULL), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(resp, 7) && wm_aligned(mean, 7) && wm_aligned(out, 7) && wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_gmm_scatter_full_workspace_bytes(n, d, ld, k), WM_EWORKSPACE);
  const GmScatterShape s = gm_scatter_full_shape(n, d, k);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long dd = (long long)d * d;
  for (int c0 = 0; c0 < k; c0 += s.batch) {  // (the batch's merge is behind its tiles and before the next batch's on the stream)
    const int nb = k - c0 < s.batch ? k - c0 : s.batch;
    GmRowsArgs a{x, resp, mean, static_cast<double*>(workspace), n, d, ld, k, s.slice_rows, c0};
    gm_rows_tile<GM_SCATTER><<<dim3(s.tiles, s.slices, nb), GM_THREADS, 0, st>>>(a);
    WM_LAUNCH_CHECK();
    gm_scatter_full_merge<<<(int)((dd * nb + GM_THREADS - 1) / GM_THREADS), GM_THREADS, 0, st>>>(a.planes, s.slices, nb, d,
                                                                                              out + (size_t)c0 * dd);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}
