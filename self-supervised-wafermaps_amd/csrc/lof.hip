// Local outlier factor over neighbour lists (neighbors.py: LocalOutlierFactor, outlier_scores, hubness): the three
// passes that follow manifold.knn_graph / knn_query, for R neighbour counts k_r at once.  A list is a row of float32
// distances and int32 indices, ordered by (distance, index), so its first k_r columns are the k_r-neighbourhood and one
// graph at max(k_r) serves every group.
//   wm_lof_lrd       lrd[r][i] = 1 / (mean_{t < k_r} max(dist_q[i][t], dist_fit[idx_q[i][t]][k_r - 1]) + 1e-10);
//   wm_lof_factor    lof[r][i] = (mean_{t < k_r} lrd_fit[r][idx_q[i][t]]) / lrd_q[r][i];
//   wm_lof_indegree  indeg[r][j] = #{ (i, t) : t < k_r, idx[i][t] == j }.
// No float atomics, no allocation, no synchronisation with the host; the order of every sum depends on k_r alone, so
// two calls give the same bits and a k_r gives the same bits alone as inside any list.  Floating-point contraction is
// off in the kernels: every sum, quotient and reciprocal is rounded once, as numpy rounds it.
//
// ---- mapping.  ld <= 63 entries fit one wave64 with one entry per lane: a wave owns a row (a workgroup of 256 threads
// four consecutive rows), lane t loads dist_q[i][t] and idx_q[i][t] once (two coalesced segments of at most 252 bytes),
// widens the distance to float64 once, and keeps both in registers for all R groups.  Per group lane t < k_r gathers
// the k-distance dist_fit[j][k_r - 1] (for the R groups these are addresses inside one 252-byte row of dist_fit, fetched
// once) or lrd_fit[r][j].  Lanes t >= k_r hold +0.0 and gather nothing, so the columns behind max(k_r) are never part of
// a sum whatever they hold.  An index outside [0, n_fit) gathers nothing either: its k-distance / lrd counts as 0.
// ---- sums and their order.  The 64 lane values v[t] (v[t] = +0.0 for t >= k_r) are added by the xor butterfly
//   v[t] += v[t ^ 1];  v[t] += v[t ^ 2];  v[t] += v[t ^ 4];  ...  v[t] += v[t ^ 32]
// i.e. the balanced tree ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) ... over the lanes; IEEE addition is
// commutative, so every lane ends with the same bits, and adding +0.0 to a non-negative number is exact: the result is
// the balanced tree over the first k_r terms padded to the next power of two with zeros.  Lane 0 then forms
//   lrd = 1.0 / (s / (double)k_r + 1e-10)        (one division, one addition, one reciprocal, each rounded once)
//   lof = (s / (double)k_r) / lrd_q[r][i]        (two divisions)
// and stores it.  R results per row are R strided 8-byte stores; against the R gathers of 63 lanes they do not count.
// ---- in-degree.  The groups that count entry (i, t) are those with k_r > t: with the counts sorted, a suffix.  So the
// host sorts the groups by k_r (ties by position), which cuts the columns into bands [k_(b-1), k_(b)); one thread per list
// entry in storage order (fully coalesced) finds the band b of its column and adds 1 to indeg[group of band b][idx[i][t]]
// with an integer atomic -- max(k_r) atomics per row, not sum(k_r) -- and a second kernel, one thread per j, adds the
// bands up in sorted order (indeg of band b += indeg of band b - 1; groups with equal k_r have an empty band and come
// out equal).  Integer addition is associative: the counts do not depend on the order of arrival.  The counts are cleared
// first by wm_zero_async (a kernel; the library issues no memset).
#include <algorithm>

#include "common.h"

namespace {

constexpr int LOF_MAX_ROWS = 1 << 24;
constexpr int LOF_MAX_LD = 63;            // one entry per lane, lane 63 idle
constexpr int LOF_THREADS = 256;
constexpr int LOF_ROWS = LOF_THREADS / WM_WAVE;  // rows of a workgroup, one wave each

struct LofKs {  // the neighbour counts, passed by value in the kernel arguments (wave-uniform scalar reads)
  int32_t k[WM_LOF_MAX_GROUPS];
};

inline bool lof_sizes_ok(int rows, int ld, int groups) {
  return rows >= 1 && rows <= LOF_MAX_ROWS && ld >= 1 && ld <= LOF_MAX_LD && groups >= 1 && groups <= WM_LOF_MAX_GROUPS;
}
// every k_r in [1, limit]
inline bool lof_ks_ok(const int32_t* ks, int groups, int limit, LofKs& out) {
  for (int r = 0; r < groups; ++r) {
    if (ks[r] < 1 || ks[r] > limit) return false;
    out.k[r] = ks[r];
  }
  for (int r = groups; r < WM_LOF_MAX_GROUPS; ++r) out.k[r] = 0;
  return true;
}

__device__ __forceinline__ double lof_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int m = 1; m < WM_WAVE; m <<= 1) v += __shfl_xor(v, m, WM_WAVE);
  return v;
}

__global__ __launch_bounds__(LOF_THREADS) void lof_lrd(const float* __restrict__ dist_q, const int32_t* __restrict__ idx_q, int rows,
                                                       int ld, const float* __restrict__ dist_fit, int n_fit, int ld_fit, LofKs ks,
                                                       int groups, double* __restrict__ lrd) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (WM_WAVE - 1);
  const int i = blockIdx.x * LOF_ROWS + (threadIdx.x >> 6);
  if (i >= rows) return;  // (wave-uniform: a wave owns one row)
  const bool have = lane < ld;
  const double d = have ? (double)dist_q[(size_t)i * ld + lane] : 0.0;
  const int j = have ? idx_q[(size_t)i * ld + lane] : -1;
  const bool ok = (unsigned)j < (unsigned)n_fit;
  const float* __restrict__ frow = dist_fit + (size_t)(ok ? j : 0) * ld_fit;
  for (int r = 0; r < groups; ++r) {
    const int k = ks.k[r];
    double term = 0.0;
    if (lane < k) {
      const double kd = ok ? (double)frow[k - 1] : 0.0;
      term = d > kd ? d : kd;
    }
    const double s = lof_wave_sum(term);
    if (lane == 0) lrd[(size_t)r * rows + i] = 1.0 / (s / (double)k + 1e-10);
  }
}

__global__ __launch_bounds__(LOF_THREADS) void lof_factor(const int32_t* __restrict__ idx_q, int rows, int ld,
                                                          const double* __restrict__ lrd_q, const double* __restrict__ lrd_fit,
                                                          int n_fit, LofKs ks, int groups, double* __restrict__ lof) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (WM_WAVE - 1);
  const int i = blockIdx.x * LOF_ROWS + (threadIdx.x >> 6);
  if (i >= rows) return;
  const int j = lane < ld ? idx_q[(size_t)i * ld + lane] : -1;
  const bool ok = (unsigned)j < (unsigned)n_fit;
  for (int r = 0; r < groups; ++r) {
    const int k = ks.k[r];
    const double term = lane < k && ok ? lrd_fit[(size_t)r * n_fit + j] : 0.0;
    const double s = lof_wave_sum(term);
    if (lane == 0) lof[(size_t)r * rows + i] = (s / (double)k) / lrd_q[(size_t)r * rows + i];
  }
}

struct LofBands {  // the groups sorted by neighbour count: band b holds the columns [bound[b - 1], bound[b]) and is counted into group slot[b]
  int32_t bound[WM_LOF_MAX_GROUPS];
  int32_t slot[WM_LOF_MAX_GROUPS];
};

__global__ __launch_bounds__(LOF_THREADS) void lof_indegree(const int32_t* __restrict__ idx, long long cells, int ld, int n, LofBands bands,
                                                            int groups, int32_t* __restrict__ indeg) {
  const long long p = (long long)blockIdx.x * LOF_THREADS + threadIdx.x;
  if (p >= cells) return;
  const int t = (int)(p % ld), j = idx[p];
  if ((unsigned)j >= (unsigned)n) return;
  int b = 0;
  while (b < groups && t >= bands.bound[b]) ++b;
  if (b < groups) atomicAdd(indeg + (size_t)bands.slot[b] * n + j, 1);
}

// indeg of band b += indeg of band b - 1, in sorted order: group r then holds the count of the columns below k_r
__global__ __launch_bounds__(LOF_THREADS) void lof_indegree_prefix(int n, LofBands bands, int groups, int32_t* __restrict__ indeg) {
  const int j = blockIdx.x * LOF_THREADS + threadIdx.x;
  if (j >= n) return;
  int32_t acc = 0;
  for (int b = 0; b < groups; ++b) {
    int32_t* cell = indeg + (size_t)bands.slot[b] * n + j;
    acc += *cell;
    *cell = acc;
  }
}

}  // namespace

extern "C" size_t wm_lof_lrd_workspace_bytes(int rows, int ld, int groups) { return lof_sizes_ok(rows, ld, groups) ? WM_TOKEN_WS : 0; }

extern "C" int wm_lof_lrd(const float* dist_q, const int32_t* idx_q, int rows, int ld, const float* dist_fit, int n_fit, int ld_fit,
                          const int32_t* ks, int groups, double* lrd, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(dist_q && idx_q && dist_fit && ks && lrd && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && ld > 0 && n_fit > 0 && ld_fit > 0 && groups > 0, WM_EINVAL);
  WM_REQUIRE(lof_sizes_ok(rows, ld, groups) && lof_sizes_ok(n_fit, ld_fit, groups), WM_EUNSUPPORTED);
  LofKs k;
  WM_REQUIRE(lof_ks_ok(ks, groups, ld < ld_fit ? ld : ld_fit, k), WM_EINVAL);
  WM_REQUIRE(wm_aligned(dist_q, 3) && wm_aligned(idx_q, 3) && wm_aligned(dist_fit, 3) && wm_aligned(lrd, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  lof_lrd<<<wm_cdiv(rows, LOF_ROWS), LOF_THREADS, 0, static_cast<hipStream_t>(stream)>>>(dist_q, idx_q, rows, ld, dist_fit, n_fit,
                                                                                         ld_fit, k, groups, lrd);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_lof_factor_workspace_bytes(int rows, int ld, int groups) { return lof_sizes_ok(rows, ld, groups) ? WM_TOKEN_WS : 0; }

extern "C" int wm_lof_factor(const int32_t* idx_q, int rows, int ld, const double* lrd_q, const double* lrd_fit, int n_fit,
                             const int32_t* ks, int groups, double* lof, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(idx_q && lrd_q && lrd_fit && ks && lof && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && ld > 0 && n_fit > 0 && groups > 0 && lof != lrd_q && lof != lrd_fit, WM_EINVAL);
  WM_REQUIRE(lof_sizes_ok(rows, ld, groups) && n_fit <= LOF_MAX_ROWS, WM_EUNSUPPORTED);
  LofKs k;
  WM_REQUIRE(lof_ks_ok(ks, groups, ld, k), WM_EINVAL);
  WM_REQUIRE(wm_aligned(idx_q, 3) && wm_aligned(lrd_q, 7) && wm_aligned(lrd_fit, 7) && wm_aligned(lof, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  lof_factor<<<wm_cdiv(rows, LOF_ROWS), LOF_THREADS, 0, static_cast<hipStream_t>(stream)>>>(idx_q, rows, ld, lrd_q, lrd_fit, n_fit, k,
                                                                                            groups, lof);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_lof_indegree_workspace_bytes(int rows, int ld, int groups) { return lof_sizes_ok(rows, ld, groups) ? WM_TOKEN_WS : 0; }

extern "C" int wm_lof_indegree(const int32_t* idx, int rows, int ld, int n, const int32_t* ks, int groups, int32_t* indeg,
                               void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(idx && ks && indeg && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && ld > 0 && n > 0 && groups > 0, WM_EINVAL);
  WM_REQUIRE(lof_sizes_ok(rows, ld, groups) && n <= LOF_MAX_ROWS, WM_EUNSUPPORTED);
  LofKs k;
  WM_REQUIRE(lof_ks_ok(ks, groups, ld, k), WM_EINVAL);
  WM_REQUIRE(wm_aligned(idx, 3) && wm_aligned(indeg, 3), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = wm_zero_async(indeg, (size_t)groups * n * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  LofBands bands;
  for (int r = 0; r < WM_LOF_MAX_GROUPS; ++r) bands.slot[r] = r < groups ? r : 0;
  std::stable_sort(bands.slot, bands.slot + groups, [&](int32_t a, int32_t b) { return k.k[a] < k.k[b]; });
  for (int b = 0; b < WM_LOF_MAX_GROUPS; ++b) bands.bound[b] = b < groups ? k.k[bands.slot[b]] : 0;
  const long long cells = (long long)rows * ld;
  lof_indegree<<<(unsigned)((cells + LOF_THREADS - 1) / LOF_THREADS), LOF_THREADS, 0, st>>>(idx, cells, ld, n, bands, groups, indeg);
  WM_LAUNCH_CHECK();
  if (groups > 1) {
    lof_indegree_prefix<<<wm_cdiv(n, LOF_THREADS), LOF_THREADS, 0, st>>>(n, bands, groups, indeg);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}
