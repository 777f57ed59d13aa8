// Downstream evaluation kernels: the multi-label AUROC of the reference's probes (torchmetrics MultilabelAUROC,
// src/ssl_wafermap/models/evals.py:88-96; scripts/MixedWM38_evals.py:103-111) and the inverted dropout of its two-layer
// probe (evals.py:162).
//
// AUROC, per label l with P positives and Q negatives: AUC = U / (P Q), U = #{(pos, neg): s_pos > s_neg} + #ties / 2 --
// what sklearn's roc_auc_score and torchmetrics' exact ROC + trapezoid rule give.  Sort-free: every (pos, neg) pair is
// compared once.  Launches:
//   1. clear the workspace header (a kernel, never a memset: csrc/common.h wm_zero_async);
//   2. auroc_range: one flag word, set when any score lies outside [0, 1] (torchmetrics then ranks the float32 sigmoid of
//      every score; the flag decides it on the device, no host round trip);
//   3. auroc_split: one workgroup per label compacts that label's (sigmoided) scores, positives from the front of its
//      row [0, P), negatives from the back [P, rows), and stores P;
//   4. auroc_count: grid (positive tiles, negative slices, labels).  A thread holds AU_PPT positives in registers, the
//      workgroup streams its slice of negatives through LDS; each pair adds 2 (greater) or 1 (equal) to twice U.  The
//      workgroup's count is added with ONE 64-bit integer atomic per label: integer addition does not depend on order,
//      so the result is the same bits on every call (no floating-point atomics anywhere);
//   5. auroc_finish: auc[l] = 2U / (2 P Q) in double, 0 for a label without positives or without negatives.
// Cost O(P Q) per label: 26 609 rows x 8 labels is at most ~1.4e9 compares.
#include "common.h"

namespace {

constexpr int AU_THREADS = 256;
constexpr int AU_PPT = 4;                                // positives per thread
constexpr int AU_POS_TILE = AU_THREADS * AU_PPT;         // positives per workgroup
constexpr int AU_NEG_SLICE = 4096;                       // negatives per workgroup
constexpr int AU_MAX_LABELS = 1024;

// workspace: [0, 256) flag word + P[L] ints (L <= 1024 -> 4 KiB + 4 B: rounded to AU_HDR); then u2[L] uint64; then
// the compacted scores vals[L][rows] f32
constexpr size_t AU_HDR = 8192;

__device__ __forceinline__ float au_load(const void* s, int dtype, long long i) {
  return dtype == WM_BF16 ? bf2f(static_cast<const uint16_t*>(s)[i]) : static_cast<const float*>(s)[i];
}

__global__ __launch_bounds__(AU_THREADS) void auroc_range(const void* __restrict__ s, int dtype, long long n,
                                                          int* __restrict__ flag) {
  int out = 0;
  for (long long i = (long long)blockIdx.x * AU_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * AU_THREADS) {
    const float v = au_load(s, dtype, i);
    out |= (v < 0.f || v > 1.f) ? 1 : 0;
  }
  if (__syncthreads_or(out) && threadIdx.x == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(AU_THREADS) void auroc_split(const void* __restrict__ s, int dtype,
                                                          const int8_t* __restrict__ t, int rows, int L,
                                                          const int* __restrict__ flag, int* __restrict__ pcount,
                                                          float* __restrict__ vals) {
  __shared__ int npos, nneg;
  const int l = blockIdx.x;
  if (threadIdx.x == 0) npos = nneg = 0;
  __syncthreads();
  const bool sig = *flag != 0;
  const int lane = threadIdx.x & 63;
  float* row = vals + (size_t)l * rows;
  for (int r0 = 0; r0 < rows; r0 += AU_THREADS) {
    const int r = r0 + threadIdx.x;
    const bool on = r < rows;
    float v = 0.f;
    bool pos = false;
    if (on) {
      v = au_load(s, dtype, (long long)r * L + l);
      if (sig) v = 1.f / (1.f + expf(-v));
      pos = t[(size_t)r * L + l] != 0;
    }
    // wave-level compaction: one LDS atomic per wave and class reserves the wave's slots
    const unsigned long long bp = __ballot(on && pos), bn = __ballot(on && !pos);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int basep = 0, basen = 0;
    if (lane == 0) {
      basep = atomicAdd(&npos, __popcll(bp));
      basen = atomicAdd(&nneg, __popcll(bn));
    }
    basep = __shfl(basep, 0);
    basen = __shfl(basen, 0);
    if (on) {
      if (pos) row[basep + __popcll(bp & below)] = v;
      else row[rows - 1 - (basen + __popcll(bn & below))] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) pcount[l] = npos;
}

__global__ __launch_bounds__(AU_THREADS) void auroc_count(const float* __restrict__ vals, int rows,
                                                          const int* __restrict__ pcount,
                                                          unsigned long long* __restrict__ u2) {
  __shared__ float neg[AU_THREADS];
  __shared__ unsigned long long red[AU_THREADS / 64];
  const int l = blockIdx.z;
  const int P = pcount[l], Q = rows - P;
  const int p0 = blockIdx.x * AU_POS_TILE, n0 = blockIdx.y * AU_NEG_SLICE;
  if (p0 >= P || n0 >= Q) return;   // uniform per workgroup: the grid covers the worst split of `rows`
  const float* row = vals + (size_t)l * rows;
  const float* negs = row + P;
  const float nanf_ = __builtin_nanf("");
  float pv[AU_PPT];
#pragma unroll
  for (int k = 0; k < AU_PPT; ++k) {
    const int i = p0 + k * AU_THREADS + threadIdx.x;
    pv[k] = i < P ? row[i] : nanf_;   // NaN compares false both ways: a padding slot counts nothing
  }
  const int n1 = min(Q, n0 + AU_NEG_SLICE);
  uint32_t c = 0;   // <= 2 * AU_PPT * AU_NEG_SLICE per thread
  for (int j0 = n0; j0 < n1; j0 += AU_THREADS) {
    const int j = j0 + threadIdx.x;
    neg[threadIdx.x] = j < n1 ? negs[j] : nanf_;
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < AU_THREADS; q += 4) {
      const float4 nv = *reinterpret_cast<const float4*>(neg + q);   // same address in every lane: a broadcast
#pragma unroll
      for (int k = 0; k < AU_PPT; ++k) {
        c += (pv[k] > nv.x) + (pv[k] >= nv.x);
        c += (pv[k] > nv.y) + (pv[k] >= nv.y);
        c += (pv[k] > nv.z) + (pv[k] >= nv.z);
        c += (pv[k] > nv.w) + (pv[k] >= nv.w);
      }
    }
    __syncthreads();
  }
  unsigned long long w = c;
  for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int i = 0; i < AU_THREADS / 64; ++i) tot += red[i];
    if (tot) atomicAdd(u2 + l, tot);
  }
}

__global__ void auroc_finish(const int* __restrict__ pcount, const unsigned long long* __restrict__ u2, int rows, int L,
                             double* __restrict__ auc, int* __restrict__ pos_out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const int P = pcount[l], Q = rows - P;
  auc[l] = (P > 0 && Q > 0) ? (double)u2[l] / (2.0 * (double)P * (double)Q) : 0.0;
  if (pos_out) pos_out[l] = P;
}

// ------------------------------------------------------------------------------------ dropout
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, long long n, float p, float scale,
                                                      uint32_t seed, T* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const bool keep = rand01(seed, (uint32_t)i) >= p;
    if constexpr (sizeof(T) == 2) {
      y[i] = keep ? f2bf(bf2f(x[i]) * scale) : (uint16_t)0;
    } else {
      y[i] = keep ? x[i] * scale : 0.f;
    }
  }
}

int dropout_launch(const void* x, int dtype, long long n, float p, uint32_t seed, void* y, void* stream) {
  WM_REQUIRE(x && y && n > 0 && n <= (1ll << 32), WM_EINVAL);
  WM_REQUIRE(p >= 0.f && p <= 1.f, WM_EINVAL);   // (NaN fails both)
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  const float scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == WM_BF16)
    dropout_kernel<uint16_t><<<(int)blocks, 256, 0, st>>>(static_cast<const uint16_t*>(x), n, p, scale, seed,
                                                           static_cast<uint16_t*>(y));
  else
    dropout_kernel<float><<<(int)blocks, 256, 0, st>>>(static_cast<const float*>(x), n, p, scale, seed,
                                                        static_cast<float*>(y));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

}  // namespace

extern "C" size_t wm_multilabel_auroc_workspace_bytes(int rows, int L) {
  if (rows <= 0 || L <= 0 || L > AU_MAX_LABELS || (long long)rows * L >= (1ll << 31)) return 0;
  return AU_HDR + (size_t)L * 8 + (size_t)L * rows * 4 + 16;
}

extern "C" int wm_multilabel_auroc(const void* scores, int dtype, const int8_t* targets, int rows, int L, double* auc,
                                   int* pos_count, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(scores && targets && auc && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && L > 0, WM_EINVAL);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  const size_t need = wm_multilabel_auroc_workspace_bytes(rows, L);
  WM_REQUIRE(need > 0, WM_EUNSUPPORTED);
  WM_REQUIRE(workspace_bytes >= need, WM_EWORKSPACE);
  WM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, WM_EALIGN);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  int* flag = reinterpret_cast<int*>(ws);
  int* pcount = flag + 64;
  unsigned long long* u2 = reinterpret_cast<unsigned long long*>(ws + AU_HDR);
  float* vals = reinterpret_cast<float*>(ws + AU_HDR + (size_t)L * 8);
  hipError_t e = wm_zero_async(ws, AU_HDR + (size_t)L * 8, st);
  if (e != hipSuccess) return (int)e;
  const long long n = (long long)rows * L;
  long long rb = (n + AU_THREADS - 1) / AU_THREADS;
  if (rb > 1024) rb = 1024;
  auroc_range<<<(int)rb, AU_THREADS, 0, st>>>(scores, dtype, n, flag);
  WM_LAUNCH_CHECK();
  auroc_split<<<L, AU_THREADS, 0, st>>>(scores, dtype, targets, rows, L, flag, pcount, vals);
  WM_LAUNCH_CHECK();
  dim3 grid(wm_cdiv(rows, AU_POS_TILE), wm_cdiv(rows, AU_NEG_SLICE), L);
  auroc_count<<<grid, AU_THREADS, 0, st>>>(vals, rows, pcount, u2);
  WM_LAUNCH_CHECK();
  auroc_finish<<<wm_cdiv(L, 64), 64, 0, st>>>(pcount, u2, rows, L, auc, pos_count);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_dropout_fwd(const void* x, int dtype, long long n, float p, uint32_t seed, void* y, void* stream) {
  return dropout_launch(x, dtype, n, p, seed, y, stream);
}

extern "C" int wm_dropout_bwd(const void* dy, int dtype, long long n, float p, uint32_t seed, void* dx, void* stream) {
  return dropout_launch(dy, dtype, n, p, seed, dx, stream);
}
