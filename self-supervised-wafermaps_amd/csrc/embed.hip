// Embedding-space kernels: row L2-normalisation (fwd/bwd) and NT-Xent (fwd/bwd).
//
// NT-Xent replaces lightly.loss.NTXentLoss()(z0, z1) as called at
// scripts/WM811k_benchmark.py:234,246 (T = 0.5, no memory bank).  The reference builds four
// [B,B] logit blocks, masks two diagonals, concatenates to [2B, 2B-1] and calls CrossEntropyLoss;
// here one pass over column tiles keeps an online log-sum-exp per row, so no logits reach HBM.
// All arithmetic is float32 (the loss tolerance is 1e-4 relative); the work is 2*(2B)^2*d FLOP,
// i.e. microseconds at B = 256, so the kernels are laid out for clarity and LDS-conflict freedom
// rather than MFMA.
#include "common.h"

namespace {

// ------------------------------------------------------------------ L2 normalise: one wave / row
template <typename TIn, typename TOut>
__global__ __launch_bounds__(256) void l2norm_fwd(const TIn* __restrict__ x, int rows, int d,
                                                  float eps, TOut* __restrict__ y,
                                                  float* __restrict__ inv_norm) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const TIn* xr = x + (size_t)row * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) {
    float v;
    if constexpr (sizeof(TIn) == 2) v = bf2f(xr[c]); else v = xr[c];
    ss += v * v;
  }
  ss = wave_sum(ss);
  const float denom = fmaxf(sqrtf(ss), eps);  // F.normalize: x / max(||x||_2, eps)
  for (int c = lane; c < d; c += 64) {
    float v;
    if constexpr (sizeof(TIn) == 2) v = bf2f(xr[c]); else v = xr[c];
    const float o = v / denom;
    if constexpr (sizeof(TOut) == 2) y[(size_t)row * d + c] = f2bf(o); else y[(size_t)row * d + c] = o;
  }
  if (inv_norm && lane == 0) inv_norm[row] = 1.0f / denom;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void l2norm_bwd(const TI* __restrict__ dy,
                                                  const float* __restrict__ y,
                                                  const float* __restrict__ inv_norm, int rows,
                                                  int d, TO* __restrict__ dx, const float* __restrict__ scale) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const TI* dyr = dy + (size_t)row * d;
  const float* yr = y + (size_t)row * d;
  auto ld = [&](int c) -> float {
    if constexpr (sizeof(TI) == 2) return bf2f(dyr[c]);
    else return dyr[c];
  };
  float dot = 0.f, yy = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float yv = yr[c];
    dot += ld(c) * yv;
    yy += yv * yv;
  }
  dot = wave_sum(dot);
  yy = wave_sum(yy);
  // a row the forward clamped (||x|| < eps) is y = x / eps with ||y|| < 1; F.normalize's clamp passes no gradient to the
  // norm there: dx = dy / eps without the projection (an unclamped row has ||y||^2 = 1 within float32 rounding).  eps is not
  // known here: a clamped row with ||x|| in [0.9995 eps, eps) passes for unclamped and keeps the projection.
  if (yy < 0.999f) dot = 0.f;
  // scale: the (device) gradient of the scalar loss this normalisation feeds -- dy is then the unscaled gradient
  const float s = inv_norm[row] * (scale != nullptr ? *scale : 1.f);
  for (int c = lane; c < d; c += 64) {
    const float v = (ld(c) - yr[c] * dot) * s;
    if constexpr (sizeof(TO) == 2) dx[(size_t)row * d + c] = f2bf(v);
    else dx[(size_t)row * d + c] = v;
  }
}

// ------------------------------------------------------------------ NT-Xent
constexpr int NX_RT = 32;   // local rows per block (8 per wave)
constexpr int NX_CT = 64;   // global rows per column tile (one per lane)
constexpr int NX_PAD = 4;   // floats of padding per column-tile row: 16-B slots rotate by 1 per row

struct NxIds {
  int self_g, pos_g;
};

__device__ __forceinline__ NxIds nx_ids(int local_row, int b_local, int b_global, int rank_offset) {
  const int v = local_row / b_local, i = local_row - v * b_local;
  NxIds r;
  r.self_g = v * b_global + rank_offset + i;
  r.pos_g = (1 - v) * b_global + rank_offset + i;
  return r;
}

__device__ __forceinline__ void nx_load_rows(const float* __restrict__ src, int first, int count,
                                             int limit, int d, int stride, float* dst, int tid,
                                             int nthreads = 256) {
  const int d4 = d >> 2;
  const int total = count * d4;
  for (int p = tid; p < total; p += nthreads) {
    const int row = p / d4, c4 = p - row * d4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (first + row < limit) v = *reinterpret_cast<const float4*>(src + (size_t)(first + row) * d + c4 * 4);
    *reinterpret_cast<float4*>(dst + (size_t)row * stride + c4 * 4) = v;
  }
}

// dots of this wave's R rows against column `lane` of the staged tile
template <int R>
__device__ __forceinline__ void nx_dots(const float* rowt, const float* colt, int d, int cstride,
                                        int wave, int lane, float (&acc)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  const float* cp = colt + (size_t)lane * cstride;
  const float* rp = rowt + (size_t)(wave * R) * d;
  for (int kk = 0; kk < d; kk += 4) {
    const float4 c = *reinterpret_cast<const float4*>(cp + kk);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 a = *reinterpret_cast<const float4*>(rp + (size_t)r * d + kk);
      acc[r] = fmaf(a.x, c.x, acc[r]);
      acc[r] = fmaf(a.y, c.y, acc[r]);
      acc[r] = fmaf(a.z, c.z, acc[r]);
      acc[r] = fmaf(a.w, c.w, acc[r]);
    }
  }
}

// four waves per block, RPW local rows per wave: RPW = 2 gives 4x the blocks of RPW = 8 for small batches (the
// 512-row problem of the headline configuration ran on 16 CUs)
template <int RPW>
__global__ __launch_bounds__(256) void ntxent_fwd_kernel(const float* __restrict__ zn,
                                                         const float* __restrict__ zall,
                                                         int b_local, int b_global,
                                                         int rank_offset, int d, float temp,
                                                         float* __restrict__ lse_out,
                                                         float* __restrict__ loss_rows) {
  extern __shared__ __attribute__((aligned(16))) float nx_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nlocal = 2 * b_local, nglobal = 2 * b_global;
  constexpr int RT = 4 * RPW, NTH = 256;
  const int row0 = blockIdx.x * RT;
  const int cstride = d + NX_PAD;
  float* rowt = nx_smem;                 // [NX_RT][d]
  float* colt = nx_smem + RT * d;        // [NX_CT][d + pad]

  nx_load_rows(zn, row0, RT, nlocal, d, d, rowt, tid, NTH);

  float m[RPW], l[RPW], pos[RPW];
  int self_g[RPW], pos_g[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
    pos[r] = 0.f;
    const int lr = row0 + wave * RPW + r;
    const NxIds ids = nx_ids(lr < nlocal ? lr : 0, b_local, b_global, rank_offset);
    self_g[r] = ids.self_g;
    pos_g[r] = ids.pos_g;
  }

  for (int j0 = 0; j0 < nglobal; j0 += NX_CT) {
    __syncthreads();  // previous tile fully consumed (and rowt visible on the first pass)
    nx_load_rows(zall, j0, NX_CT, nglobal, d, cstride, colt, tid, NTH);
    __syncthreads();
    float acc[RPW];
    nx_dots<RPW>(rowt, colt, d, cstride, wave, lane, acc);
    const int g = j0 + lane;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const float s = acc[r] / temp;
      if (g == pos_g[r]) pos[r] = s;
      if (g < nglobal && g != self_g[r]) {
        const float mn = fmaxf(m[r], s);
        l[r] = l[r] * __expf(m[r] - mn) + __expf(s - mn);
        m[r] = mn;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const float mm = wave_max(m[r]);
    const float part = (m[r] == -INFINITY) ? 0.f : l[r] * expf(m[r] - mm);
    const float ll = wave_sum(part);
    const float pp = wave_sum(pos[r]);
    const int lr = row0 + wave * RPW + r;
    if (lane == 0 && lr < nlocal) {
      const float lse = mm + logf(ll);
      lse_out[lr] = lse;
      loss_rows[lr] = lse - pp;
    }
  }
}

// blockIdx.y = column split (tiles_per_split column tiles each): with one block per 32 local rows the
// 512 x 512 problem of the headline configuration ran on 16 CUs for 160 us.  Split blocks store their
// partial row gradients into slab blockIdx.y of a workspace; ntxent_bwd_reduce sums the slabs in order.
__global__ __launch_bounds__(256) void ntxent_bwd_kernel(
    const float* __restrict__ zn, const float* __restrict__ zall,
    const float* __restrict__ lse_all, int b_local, int b_global, int rank_offset, int d,
    float temp, float grad_scale, int tiles_per_split, int nsplit, float* __restrict__ dzn) {
  extern __shared__ __attribute__((aligned(16))) float nx_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nlocal = 2 * b_local, nglobal = 2 * b_global;
  const int row0 = blockIdx.x * NX_RT;
  const int cstride = d + NX_PAD;
  constexpr int MS = NX_CT + 1;
  float* rowt = nx_smem;
  float* colt = rowt + NX_RT * d;
  float* mt = colt + NX_CT * cstride;  // [NX_RT][NX_CT + 1]

  nx_load_rows(zn, row0, NX_RT, nlocal, d, d, rowt, tid);

  float lse_i[8];
  int self_g[8], pos_g[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int lr = row0 + wave * 8 + r;
    const NxIds ids = nx_ids(lr < nlocal ? lr : 0, b_local, b_global, rank_offset);
    self_g[r] = ids.self_g;
    pos_g[r] = ids.pos_g;
    lse_i[r] = lse_all[ids.self_g];
  }

  // phase-2 ownership: row rr, float4 granules (tid&7) + 8u
  const int rr = tid >> 3, gsel = tid & 7;
  const int nu = d >> 5;  // float4 granules per thread (d/32)
  float4 out[8];          // d <= 256
#pragma unroll
  for (int u = 0; u < 8; ++u) out[u] = make_float4(0.f, 0.f, 0.f, 0.f);

  const int jbegin = blockIdx.y * tiles_per_split * NX_CT;
  const int jend = min(nglobal, jbegin + tiles_per_split * NX_CT);
  for (int j0 = jbegin; j0 < jend; j0 += NX_CT) {
    __syncthreads();
    nx_load_rows(zall, j0, NX_CT, nglobal, d, cstride, colt, tid);
    __syncthreads();
    float acc[8];
    nx_dots<8>(rowt, colt, d, cstride, wave, lane, acc);
    const int g = j0 + lane;
    const float lse_j = g < nglobal ? lse_all[g] : 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float s = acc[r] / temp;
      float mv = 0.f;
      if (g < nglobal && g != self_g[r]) {
        mv = __expf(s - lse_i[r]) + __expf(s - lse_j);
        if (g == pos_g[r]) mv -= 2.f;
      }
      mt[(wave * 8 + r) * MS + lane] = mv;
    }
    __syncthreads();
    for (int j = 0; j < NX_CT; ++j) {
      const float w = mt[rr * MS + j];
      const float* cz = colt + (size_t)j * cstride + gsel * 4;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (u < nu) {
          const float4 c = *reinterpret_cast<const float4*>(cz + u * 32);
          out[u].x = fmaf(w, c.x, out[u].x);
          out[u].y = fmaf(w, c.y, out[u].y);
          out[u].z = fmaf(w, c.z, out[u].z);
          out[u].w = fmaf(w, c.w, out[u].w);
        }
      }
    }
  }
  const int lr = row0 + rr;
  if (lr < nlocal) {
    const float sc = grad_scale / temp;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < nu) {
        float4 o = out[u];
        o.x *= sc; o.y *= sc; o.z *= sc; o.w *= sc;
        // nsplit > 1: dzn is the partial-sum workspace [nsplit][2 b_local][d]; ntxent_bwd_reduce adds the splits in
        // order (no atomics: the gradient is bit-reproducible)
        float* dst = dzn + ((size_t)blockIdx.y * nlocal + lr) * d + gsel * 4 + u * 32;
        *reinterpret_cast<float4*>(dst) = o;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ntxent_bwd_reduce(const float4* __restrict__ part, int nsplit, long long n4,
                                                         float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = part[i];
  for (int sp = 1; sp < nsplit; ++sp) {
    const float4 t = part[(size_t)sp * n4 + i];
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  out[i] = v;
}

}  // namespace

extern "C" int wm_l2_normalize(const void* x, int in_dtype, int rows, int d, float eps, void* y,
                               int out_dtype, float* inv_norm, void* stream) {
  WM_REQUIRE(x && y, WM_EINVAL);
  WM_REQUIRE(rows > 0 && d > 0, WM_EINVAL);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = wm_cdiv(rows, 4);
  if (in_dtype == WM_F32 && out_dtype == WM_F32)
    l2norm_fwd<float, float><<<grid, 256, 0, st>>>((const float*)x, rows, d, eps, (float*)y, inv_norm);
  else if (in_dtype == WM_F32 && out_dtype == WM_BF16)
    l2norm_fwd<float, uint16_t><<<grid, 256, 0, st>>>((const float*)x, rows, d, eps, (uint16_t*)y, inv_norm);
  else if (in_dtype == WM_BF16 && out_dtype == WM_F32)
    l2norm_fwd<uint16_t, float><<<grid, 256, 0, st>>>((const uint16_t*)x, rows, d, eps, (float*)y, inv_norm);
  else if (in_dtype == WM_BF16 && out_dtype == WM_BF16)
    l2norm_fwd<uint16_t, uint16_t><<<grid, 256, 0, st>>>((const uint16_t*)x, rows, d, eps, (uint16_t*)y, inv_norm);
  else
    return WM_EUNSUPPORTED;
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_l2_normalize_bwd(const void* dy, int dy_dtype, const float* y, const float* inv_norm, int rows,
                                   int d, void* dx, int out_dtype, const float* scale_dev, void* stream) {
  WM_REQUIRE(dy && y && inv_norm && dx, WM_EINVAL);
  WM_REQUIRE(rows > 0 && d > 0, WM_EINVAL);
  WM_REQUIRE((out_dtype == WM_F32 || out_dtype == WM_BF16) && (dy_dtype == WM_F32 || dy_dtype == WM_BF16), WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(wm_cdiv(rows, 4));
  if (dy_dtype == WM_F32 && out_dtype == WM_F32)
    l2norm_bwd<float, float><<<grid, 256, 0, st>>>(static_cast<const float*>(dy), y, inv_norm, rows, d, static_cast<float*>(dx), scale_dev);
  else if (dy_dtype == WM_F32)
    l2norm_bwd<float, uint16_t><<<grid, 256, 0, st>>>(static_cast<const float*>(dy), y, inv_norm, rows, d, static_cast<uint16_t*>(dx), scale_dev);
  else if (out_dtype == WM_F32)
    l2norm_bwd<uint16_t, float><<<grid, 256, 0, st>>>(static_cast<const uint16_t*>(dy), y, inv_norm, rows, d, static_cast<float*>(dx), scale_dev);
  else
    l2norm_bwd<uint16_t, uint16_t><<<grid, 256, 0, st>>>(static_cast<const uint16_t*>(dy), y, inv_norm, rows, d, static_cast<uint16_t*>(dx), scale_dev);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

static int nx_check(const void* a, const void* b, const void* c, const void* e, int b_local,
                    int b_global, int rank_offset, int d, float temperature) {
  WM_REQUIRE(a && b && c && e, WM_EINVAL);
  WM_REQUIRE(b_local > 0 && b_global >= b_local && d > 0 && temperature > 0.f, WM_EINVAL);
  WM_REQUIRE(rank_offset >= 0 && rank_offset + b_local <= b_global, WM_EINVAL);
  WM_REQUIRE(d % 32 == 0 && d <= 256, WM_EUNSUPPORTED);
  return WM_OK;
}

extern "C" int wm_ntxent_fwd(const float* zn, const float* zall, int b_local, int b_global,
                             int rank_offset, int d, float temperature, float* lse,
                             float* loss_rows, void* stream) {
  const int rc = nx_check(zn, zall, lse, loss_rows, b_local, b_global, rank_offset, d, temperature);
  if (rc != WM_OK) return rc;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ntxent_fwd_kernel<8>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ntxent_fwd_kernel<2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (2 * b_local <= 2048) {  // few rows: 8-row blocks (2 per wave) so that the grid covers more of the chip
    const size_t lds = ((size_t)8 * d + (size_t)NX_CT * (d + NX_PAD)) * sizeof(float);
    ntxent_fwd_kernel<2><<<wm_cdiv(2 * b_local, 8), 256, lds, st>>>(zn, zall, b_local, b_global, rank_offset, d,
                                                                    temperature, lse, loss_rows);
  } else {
    const size_t lds = ((size_t)NX_RT * d + (size_t)NX_CT * (d + NX_PAD)) * sizeof(float);
    ntxent_fwd_kernel<8><<<wm_cdiv(2 * b_local, NX_RT), 256, lds, st>>>(zn, zall, b_local, b_global, rank_offset, d,
                                                                        temperature, lse, loss_rows);
  }
  WM_LAUNCH_CHECK();
  return WM_OK;
}

static void nx_bwd_plan(int b_local, int b_global, int& rowtiles, int& nsplit, int& tiles_per_split) {
  rowtiles = wm_cdiv(2 * b_local, NX_RT);
  const int coltiles = wm_cdiv(2 * b_global, NX_CT);
  nsplit = 256 / rowtiles;  // about one block per CU
  if (nsplit < 1) nsplit = 1;
  if (nsplit > coltiles) nsplit = coltiles;
  tiles_per_split = wm_cdiv(coltiles, nsplit);
  nsplit = wm_cdiv(coltiles, tiles_per_split);
}

extern "C" size_t wm_ntxent_bwd_workspace_bytes(int b_local, int b_global, int d) {
  if (b_local <= 0 || b_global < b_local || d <= 0) return 0;
  int rowtiles, nsplit, tps;
  nx_bwd_plan(b_local, b_global, rowtiles, nsplit, tps);
  return nsplit > 1 ? (size_t)nsplit * 2 * b_local * d * sizeof(float) : 16;
}

extern "C" int wm_ntxent_bwd(const float* zn, const float* zall, const float* lse_all, int b_local,
                             int b_global, int rank_offset, int d, float temperature,
                             float grad_scale, float* dzn, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = nx_check(zn, zall, lse_all, dzn, b_local, b_global, rank_offset, d, temperature);
  if (rc != WM_OK) return rc;
  const size_t lds =
      ((size_t)NX_RT * d + (size_t)NX_CT * (d + NX_PAD) + (size_t)NX_RT * (NX_CT + 1)) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ntxent_bwd_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 147456);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  int rowtiles, nsplit, tiles_per_split;
  nx_bwd_plan(b_local, b_global, rowtiles, nsplit, tiles_per_split);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* target = dzn;
  if (nsplit > 1) {
    WM_REQUIRE(workspace && workspace_bytes >= wm_ntxent_bwd_workspace_bytes(b_local, b_global, d), WM_EWORKSPACE);
    WM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(dzn) & 15) == 0, WM_EALIGN);
    target = static_cast<float*>(workspace);
  }
  ntxent_bwd_kernel<<<dim3(rowtiles, nsplit), 256, lds, st>>>(
      zn, zall, lse_all, b_local, b_global, rank_offset, d, temperature, grad_scale, tiles_per_split, nsplit, target);
  WM_LAUNCH_CHECK();
  if (nsplit > 1) {
    const long long n4 = (long long)2 * b_local * d / 4;
    ntxent_bwd_reduce<<<wm_cdiv(n4, 256), 256, 0, st>>>(reinterpret_cast<const float4*>(target), nsplit, n4,
                                                        reinterpret_cast<float4*>(dzn));
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}

// ------------------------------------------------------------------------------------ MoCo bank
// NT-Xent against a memory bank (lightly.loss.NTXentLoss(memory_bank_size > 0), the reference's MoCo:
// scripts/WM811k_benchmark.py:305-307,337-338).  Per query row i:
//   logits = [ <q_i, k_i> , <q_i, bank[:, 0..K)> ] / T,  label 0,  loss = mean_i (lse_i - logit_i0)
//   dq_i = ((p_i0 - 1) k_i + sum_k p_ik bank[:, k]) / (B T),   dk_i = (p_i0 - 1) q_i / (B T)
// bank is lightly's [D][K] (column = one stored key).  One block per query row: threads stride over
// the K columns (coalesced across k for every d), the K logits live in LDS between the two passes.
namespace {
constexpr int MB_THREADS = 256;

__device__ __forceinline__ float mb_block_reduce(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(MB_THREADS) void ntxent_bank_kernel(const float* __restrict__ q, const float* __restrict__ kpos,
                                                                 const float* __restrict__ bank, int B, int D, int K,
                                                                 float inv_t, float* __restrict__ loss,
                                                                 float* __restrict__ dq, float* __restrict__ dk) {
  extern __shared__ float mb_smem[];  // q[D], kp[D], s[K]
  __shared__ float red[4];
  float* sq = mb_smem;
  float* skp = sq + D;
  float* ss = skp + D;
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int d = tid; d < D; d += MB_THREADS) {
    sq[d] = q[(size_t)i * D + d];
    skp[d] = kpos[(size_t)i * D + d];
  }
  __syncthreads();
  float part = 0.f;
  for (int d = tid; d < D; d += MB_THREADS) part = fmaf(sq[d], skp[d], part);
  const float s0 = mb_block_reduce(part, red, false) * inv_t;
  float m = s0;
  for (int k = tid; k < K; k += MB_THREADS) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(sq[d], bank[(size_t)d * K + k], s);
    s *= inv_t;
    ss[k] = s;
    m = fmaxf(m, s);
  }
  m = mb_block_reduce(m, red, true);
  float sum = 0.f;
  for (int k = tid; k < K; k += MB_THREADS) sum += expf(ss[k] - m);
  sum = mb_block_reduce(sum, red, false) + expf(s0 - m);
  const float lse = m + logf(sum);
  const float w = inv_t / (float)B;
  const float p0 = expf(s0 - lse);
  if (tid == 0) atomicAdd(loss, (lse - s0) / (float)B);
  for (int k = tid; k < K; k += MB_THREADS) ss[k] = expf(ss[k] - lse);  // own entries only: no sync needed yet
  __syncthreads();
  // dq[d] = w ((p0 - 1) kp[d] + sum_k p_k bank[d][k]): a wave per d, lanes stride over k (coalesced)
  const int lane = tid & 63, wave = tid >> 6;
  for (int d = wave; d < D; d += MB_THREADS / 64) {
    float acc = 0.f;
    const float* row = bank + (size_t)d * K;
    for (int k = lane; k < K; k += 64) acc = fmaf(ss[k], row[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) {
      dq[(size_t)i * D + d] = w * ((p0 - 1.f) * skp[d] + acc);
      dk[(size_t)i * D + d] = w * (p0 - 1.f) * sq[d];
    }
  }
}
}  // namespace

extern "C" int wm_ntxent_bank_fwd_bwd(const float* q, const float* kpos, const float* bank, int B, int D, int K,
                                      float temperature, float* loss, float* dq, float* dk, void* stream) {
  WM_REQUIRE(q && kpos && bank && loss && dq && dk, WM_EINVAL);
  WM_REQUIRE(B > 0 && D > 0 && K > 0 && temperature > 1e-8f, WM_EINVAL);
  const size_t lds = ((size_t)2 * D + K) * sizeof(float);
  WM_REQUIRE(lds <= 64 * 1024, WM_EUNSUPPORTED);  // K + 2 D <= 16384 floats
  ntxent_bank_kernel<<<B, MB_THREADS, lds, static_cast<hipStream_t>(stream)>>>(q, kpos, bank, B, D, K, 1.f / temperature,
                                                                              loss, dq, dk);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ -cos
// lightly.loss.NegativeCosineSimilarity (BYOL / SimSiam in the reference, scripts/WM811k_benchmark.py:
// 446,613): loss = -mean_i cos(x0_i, x1_i) with torch's cosine_similarity (each norm clamped at eps).
// One wave per row; x bf16 or f32 [B][D]; gradients f32, either may be NULL (SimSiam detaches z).
namespace {
template <typename T>
__device__ __forceinline__ float nc_ld(const T* p, size_t i);
template <>
__device__ __forceinline__ float nc_ld<float>(const float* p, size_t i) { return p[i]; }
template <>
__device__ __forceinline__ float nc_ld<uint16_t>(const uint16_t* p, size_t i) { return bf2f(p[i]); }

template <typename T>
__global__ __launch_bounds__(256) void neg_cosine_kernel(const T* __restrict__ x0, const T* __restrict__ x1, int B, int D,
                                                         float eps, float* __restrict__ loss, float* __restrict__ d0,
                                                         float* __restrict__ d1) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  float dot = 0.f, n0 = 0.f, n1 = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float a = nc_ld<T>(x0, (size_t)row * D + d), b = nc_ld<T>(x1, (size_t)row * D + d);
    dot = fmaf(a, b, dot);
    n0 = fmaf(a, a, n0);
    n1 = fmaf(b, b, n1);
  }
  dot = wave_sum(dot);
  n0 = wave_sum(n0);
  n1 = wave_sum(n1);
  const float l0 = sqrtf(n0), l1 = sqrtf(n1);
  const float c0 = fmaxf(l0, eps), c1 = fmaxf(l1, eps);
  const float cosv = dot / (c0 * c1);
  if (lane == 0) atomicAdd(loss, -cosv / (float)B);
  // d(-cos/B)/dx0 = -(x1 / (c0 c1) - cos x0 / c0^2 [if l0 > eps]) / B
  const float w = -1.f / (float)B, inv = 1.f / (c0 * c1);
  const float k0 = l0 > eps ? cosv / (c0 * c0) : 0.f, k1 = l1 > eps ? cosv / (c1 * c1) : 0.f;
  for (int d = lane; d < D; d += 64) {
    const float a = nc_ld<T>(x0, (size_t)row * D + d), b = nc_ld<T>(x1, (size_t)row * D + d);
    if (d0) d0[(size_t)row * D + d] = w * (b * inv - k0 * a);
    if (d1) d1[(size_t)row * D + d] = w * (a * inv - k1 * b);
  }
}
}  // namespace

extern "C" int wm_neg_cosine_fwd_bwd(const void* x0, const void* x1, int dtype, int B, int D, float eps, float* loss,
                                     float* dx0, float* dx1, void* stream) {
  WM_REQUIRE(x0 && x1 && loss, WM_EINVAL);
  WM_REQUIRE(B > 0 && D > 0 && eps >= 0.f, WM_EINVAL);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == WM_F32)
    neg_cosine_kernel<float><<<wm_cdiv(B, 4), 256, 0, st>>>(static_cast<const float*>(x0), static_cast<const float*>(x1), B,
                                                            D, eps, loss, dx0, dx1);
  else
    neg_cosine_kernel<uint16_t><<<wm_cdiv(B, 4), 256, 0, st>>>(static_cast<const uint16_t*>(x0),
                                                               static_cast<const uint16_t*>(x1), B, D, eps, loss, dx0, dx1);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ classification
// torch.nn.CrossEntropyLoss(weight=w) / F.nll_loss(log_softmax) and torch.nn.BCEWithLogitsLoss(pos_weight) as the
// reference's supervised baseline and linear probes use them (scripts/WM811k_benchmark.py:211-217;
// src/ssl_wafermap/models/evals.py:20,93).  Logits float32 or bf16 [B][C] compact; gradients float32.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void cross_entropy_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                            const float* __restrict__ weight, int B, int C,
                                                            float* __restrict__ acc, float* __restrict__ dlogits) {
  // acc[0] += w_y * nll, acc[1] += w_y (the weighted mean divides the two; gradients are scaled later)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, nc_ld<T>(logits, (size_t)row * C + c));
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(nc_ld<T>(logits, (size_t)row * C + c) - m);
  s = wave_sum(s);
  const float lse = m + logf(s);
  const long long y = labels[row];
  const bool valid = y >= 0 && y < C;
  const float wy = valid ? (weight ? weight[y] : 1.f) : 0.f;
  if (lane == 0 && valid) {
    atomicAdd(acc, wy * (lse - nc_ld<T>(logits, (size_t)row * C + y)));
    atomicAdd(acc + 1, wy);
  }
  for (int c = lane; c < C; c += 64) {
    const float p = expf(nc_ld<T>(logits, (size_t)row * C + c) - lse);
    dlogits[(size_t)row * C + c] = wy * (p - (c == y ? 1.f : 0.f));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bce_logits_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                         const float* __restrict__ pos_weight, long long n, int C,
                                                         float* __restrict__ loss, float* __restrict__ dlogits) {
  __shared__ float red[4];
  const float inv = 1.f / (float)n;
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float x = nc_ld<T>(logits, (size_t)i), t = target[i];
    const float pw = pos_weight ? pos_weight[i % C] : 1.f;
    // loss = (1 - t) x + (1 + (pw - 1) t) softplus(-x)   (torch's stable form)
    const float lw = 1.f + (pw - 1.f) * t;
    const float sp = fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
    s += (1.f - t) * x + lw * sp;
    const float sig = 1.f / (1.f + expf(-x));
    dlogits[i] = ((1.f - t) - lw * (1.f - sig)) * inv;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
}
}  // namespace

extern "C" int wm_cross_entropy_fwd_bwd(const void* logits, int dtype, const long long* labels, const float* weight,
                                        int B, int C, float* acc2, float* dlogits, void* stream) {
  WM_REQUIRE(logits && labels && acc2 && dlogits, WM_EINVAL);
  WM_REQUIRE(B > 0 && C > 0, WM_EINVAL);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == WM_F32)
    cross_entropy_kernel<float><<<wm_cdiv(B, 4), 256, 0, st>>>(static_cast<const float*>(logits), labels, weight, B, C, acc2,
                                                               dlogits);
  else
    cross_entropy_kernel<uint16_t><<<wm_cdiv(B, 4), 256, 0, st>>>(static_cast<const uint16_t*>(logits), labels, weight, B, C,
                                                                  acc2, dlogits);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_bce_logits_fwd_bwd(const void* logits, int dtype, const float* target, const float* pos_weight, int B,
                                     int C, float* loss, float* dlogits, void* stream) {
  WM_REQUIRE(logits && target && loss && dlogits, WM_EINVAL);
  WM_REQUIRE(B > 0 && C > 0, WM_EINVAL);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n = (long long)B * C;
  const int blocks = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
  if (dtype == WM_F32)
    bce_logits_kernel<float><<<blocks, 256, 0, st>>>(static_cast<const float*>(logits), target, pos_weight, n, C, loss,
                                                     dlogits);
  else
    bce_logits_kernel<uint16_t><<<blocks, 256, 0, st>>>(static_cast<const uint16_t*>(logits), target, pos_weight, n, C, loss,
                                                        dlogits);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ DCL / DCLW
// lightly.loss.DCLLoss / DCLWLoss (decoupled contrastive learning, the reference's DCLW model:
// scripts/WM811k_benchmark.py:258-287).  For L2-normalised z0, z1 [B][D], per direction (a, b) in
// {(z0, z1), (z1, z0)} and row i:
//     l_i = -w_i <a_i, b_i>/T + lse_{k != i} <a_i, a_k>/T + lse_{k != i} <a_i, b_k>/T
// w_i = 1 (DCL) or 2 - B softmax_i(<z0_i, z1_i>/sigma) (DCLW, detached);  loss = mean over rows and directions.
// Kernel 1 (block = direction x row): the two similarity rows, their log-sum-exps, the softmax rows P_aa, P_ab
// into global memory, the loss.  Kernel 2 (block = row i): the gradient as small matrix products with P.
namespace {
__global__ __launch_bounds__(256) void dcl_rows_kernel(const float* __restrict__ z0, const float* __restrict__ z1, int B, int D,
                                                       float inv_t, float sigma_inv, int weighted,
                                                       float* __restrict__ P, float* __restrict__ wts,
                                                       float* __restrict__ loss) {
  extern __shared__ float dc_smem[];  // a_i[D], s_aa[B], s_ab[B]
  __shared__ float red[4];
  float* sa = dc_smem;
  float* saa = sa + D;
  float* sab = saa + B;
  const int dir = blockIdx.x / B, i = blockIdx.x - dir * B, tid = threadIdx.x;
  const float* a = dir == 0 ? z0 : z1;
  const float* b = dir == 0 ? z1 : z0;
  for (int d = tid; d < D; d += 256) sa[d] = a[(size_t)i * D + d];
  __syncthreads();
  // mises-fisher weight of row i: needs the softmax over the whole batch of the positive similarities
  float w = 1.f;
  if (weighted) {
    float m = -INFINITY;
    for (int k = tid; k < B; k += 256) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(z0[(size_t)k * D + d], z1[(size_t)k * D + d], s);
      saa[k] = s * sigma_inv;
      m = fmaxf(m, saa[k]);
    }
    m = mb_block_reduce(m, red, true);
    float sum = 0.f;
    for (int k = tid; k < B; k += 256) sum += expf(saa[k] - m);
    sum = mb_block_reduce(sum, red, false);
    w = 2.f - (float)B * expf(saa[i] - m) / sum;
    __syncthreads();
  }
  float maa = -INFINITY, mab = -INFINITY;
  for (int k = tid; k < B; k += 256) {
    float s0 = 0.f, s1 = 0.f;
    for (int d = 0; d < D; ++d) {
      s0 = fmaf(sa[d], a[(size_t)k * D + d], s0);
      s1 = fmaf(sa[d], b[(size_t)k * D + d], s1);
    }
    saa[k] = s0 * inv_t;
    sab[k] = s1 * inv_t;
    if (k != i) {
      maa = fmaxf(maa, saa[k]);
      mab = fmaxf(mab, sab[k]);
    }
  }
  maa = mb_block_reduce(maa, red, true);
  mab = mb_block_reduce(mab, red, true);
  float eaa = 0.f, eab = 0.f;
  for (int k = tid; k < B; k += 256)
    if (k != i) {
      eaa += expf(saa[k] - maa);
      eab += expf(sab[k] - mab);
    }
  eaa = mb_block_reduce(eaa, red, false);
  eab = mb_block_reduce(eab, red, false);
  const float lse_aa = maa + logf(eaa), lse_ab = mab + logf(eab);
  float* paa = P + ((size_t)(dir * 2 + 0) * B + i) * B;
  float* pab = P + ((size_t)(dir * 2 + 1) * B + i) * B;
  for (int k = tid; k < B; k += 256) {
    paa[k] = k == i ? 0.f : expf(saa[k] - lse_aa);
    pab[k] = k == i ? 0.f : expf(sab[k] - lse_ab);
  }
  if (tid == 0) {
    wts[dir * B + i] = w;
    atomicAdd(loss, (-w * sab[i] + lse_aa + lse_ab) * 0.5f / (float)B);
  }
}

// d loss / d z0_i and d z1_i.  With direction 0 = (a, b) = (z0, z1) and direction 1 = (z1, z0):
//   dz0_i = c [ sum_k (Paa0[i][k] + Paa0[k][i]) z0_k + sum_k Pab0[i][k] z1_k - w0_i z1_i        (direction 0, a role)
//             + sum_j Pab1[j][i] z1_j - w1_i z1_i ]                                              (direction 1, b role)
//   dz1_i likewise with the directions exchanged;  c = 0.5 / (T B).
__global__ __launch_bounds__(256) void dcl_grad_kernel(const float* __restrict__ z0, const float* __restrict__ z1, int B, int D,
                                                       float inv_t, const float* __restrict__ P,
                                                       const float* __restrict__ wts, float* __restrict__ dz0,
                                                       float* __restrict__ dz1) {
  const int which = blockIdx.x / B, i = blockIdx.x - which * B;  // which: 0 -> dz0, 1 -> dz1
  const float* a = which == 0 ? z0 : z1;                          // the tensor whose row i we differentiate
  const float* b = which == 0 ? z1 : z0;
  const int da = which, db = 1 - which;                           // direction where `a` is the anchor / where it is the target
  const float* Paa = P + (size_t)(da * 2 + 0) * B * B;
  const float* Pab = P + (size_t)(da * 2 + 1) * B * B;
  const float* Qab = P + (size_t)(db * 2 + 1) * B * B;           // anchor b, target a
  const float c = 0.5f * inv_t / (float)B;
  for (int d = threadIdx.x; d < D; d += 256) {
    float g = 0.f;
    for (int k = 0; k < B; ++k) {
      g = fmaf(Paa[(size_t)i * B + k] + Paa[(size_t)k * B + i], a[(size_t)k * D + d], g);
      g = fmaf(Pab[(size_t)i * B + k] + Qab[(size_t)k * B + i], b[(size_t)k * D + d], g);
    }
    g -= (wts[da * B + i] + wts[db * B + i]) * b[(size_t)i * D + d];
    (which == 0 ? dz0 : dz1)[(size_t)i * D + d] = c * g;
  }
}
}  // namespace

extern "C" size_t wm_dcl_workspace_bytes(int B) { return B > 0 ? ((size_t)4 * B * B + (size_t)2 * B) * sizeof(float) : 0; }

extern "C" int wm_dcl_fwd_bwd(const float* z0, const float* z1, int B, int D, float temperature, float sigma, int weighted,
                              float* loss, float* dz0, float* dz1, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(z0 && z1 && loss && dz0 && dz1 && workspace, WM_EINVAL);
  WM_REQUIRE(B > 1 && D > 0 && temperature > 1e-8f && (!weighted || sigma > 1e-8f), WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_dcl_workspace_bytes(B), WM_EWORKSPACE);
  const size_t lds = ((size_t)D + 2 * B) * sizeof(float);
  WM_REQUIRE(lds <= 64 * 1024, WM_EUNSUPPORTED);
  float* P = static_cast<float*>(workspace);
  float* wts = P + (size_t)4 * B * B;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dcl_rows_kernel<<<2 * B, 256, lds, st>>>(z0, z1, B, D, 1.f / temperature, weighted ? 1.f / sigma : 0.f, weighted, P, wts,
                                          loss);
  WM_LAUNCH_CHECK();
  dcl_grad_kernel<<<2 * B, 256, 0, st>>>(z0, z1, B, D, 1.f / temperature, P, wts, dz0, dz1);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ Barlow Twins
// lightly.loss.BarlowTwinsLoss (the reference's BarlowTwins model, scripts/WM811k_benchmark.py:364-366):
// c = scale * raw  (raw [D][D] = za_norm^T zb_norm summed over the batch, from the weight-gradient GEMM);
// loss = sum_i (c_ii - 1)^2 + lambda sum_{i != j} c_ij^2;  dc/draw folded in: draw = scale * dloss/dc.
namespace {
__global__ __launch_bounds__(256) void barlow_kernel(const float* __restrict__ raw, int D, float scale, float lambda,
                                                     float diag_weight, float* __restrict__ loss,
                                                     float* __restrict__ draw) {
  __shared__ float red[4];
  const long long n = (long long)D * D;
  float s = 0.f;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const int i = (int)(t / D), j = (int)(t - (long long)i * D);
    const float c = raw[t] * scale;
    float g;
    if (i == j) {
      s = fmaf(diag_weight * (c - 1.f), c - 1.f, s);
      g = 2.f * diag_weight * (c - 1.f);
    } else {
      s = fmaf(lambda * c, c, s);
      g = 2.f * lambda * c;
    }
    draw[t] = g * scale;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, red[0] + red[1] + red[2] + red[3]);
}
}  // namespace

extern "C" int wm_barlow_twins_fwd_bwd(const float* raw_cc, int D, float scale, float lambda, float diag_weight,
                                       float* loss, float* draw_cc, void* stream) {
  WM_REQUIRE(raw_cc && loss && draw_cc && D > 0, WM_EINVAL);
  const long long n = (long long)D * D;
  const int blocks = (int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
  barlow_kernel<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(raw_cc, D, scale, lambda, diag_weight, loss,
                                                                      draw_cc);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ VICReg pieces
// lightly.loss.VICRegLoss (the reference's VICReg model, scripts/WM811k_benchmark.py:401): per branch
//   centred = z - mean_0(z)   (wm_center_columns; its covariance is the weight-gradient GEMM + wm_barlow_twins_fwd_bwd
//                              with diag_weight 0, lambda 1/D, scale 1/(N-1))
//   variance term = mean_d relu(1 - sqrt(var_unbiased_d + eps)) and its derivative with respect to centred[n][d],
//                   coef_d * centred[n][d]  (wm_vicreg_variance).
namespace {
__global__ __launch_bounds__(256) void center_columns_kernel(const uint16_t* __restrict__ z, const float* __restrict__ mean,
                                                             long long rows, int C, uint16_t* __restrict__ out) {
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    out[i] = f2bf(bf2f(z[i]) - mean[i % C]);
}

__global__ __launch_bounds__(256) void vicreg_variance_kernel(const float* __restrict__ var_biased, int N, int D, float eps,
                                                              float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ float red[4];
  float s = 0.f;
  for (int d = blockIdx.x * 256 + threadIdx.x; d < D; d += gridDim.x * 256) {
    const float var = var_biased[d] * (float)N / (float)(N - 1);
    const float sd = sqrtf(var + eps);
    const float hinge = fmaxf(1.f - sd, 0.f);
    s += hinge;
    // d mean_d relu(1 - sd_d) / d centred[n][d] = -[sd < 1] / D * centred[n][d] / ((N - 1) sd)
    coef[d] = hinge > 0.f ? -1.f / ((float)D * (float)(N - 1) * sd) : 0.f;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) / (float)D);
}
}  // namespace

extern "C" int wm_center_columns(const void* z, const float* mean, long long rows, int C, void* out, void* stream) {
  WM_REQUIRE(z && mean && out && rows > 0 && C > 0, WM_EINVAL);
  const long long n = rows * C;
  const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  center_columns_kernel<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const uint16_t*>(z), mean, rows, C,
                                                                              static_cast<uint16_t*>(out));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_vicreg_variance(const float* var_biased, int N, int D, float eps, float* loss, float* coef,
                                  void* stream) {
  WM_REQUIRE(var_biased && loss && coef && N > 1 && D > 0 && eps >= 0.f, WM_EINVAL);
  vicreg_variance_kernel<<<wm_cdiv(D, 256) > 64 ? 64 : wm_cdiv(D, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      var_biased, N, D, eps, loss, coef);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------------ SwaV Sinkhorn
// lightly.loss.swav_loss.sinkhorn (the reference's SwaV, scripts/WM811k_benchmark.py:832-834): Q = exp(out / eps)^T,
// then `iters` rounds of { every prototype's row sums to 1/K ; every sample's column sums to 1/B }, finally * B.
// E = exp(out / eps) stays fixed; the normalisations only rescale prototypes (c[k]) and samples (r[b]):
// Q[b][k] = E[b][k] r[b] c[k].  Two tiny reductions per round, one launch each.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void sk_proto_kernel(const T* __restrict__ out, const float* __restrict__ r, int B, int K,
                                                       float inv_eps, float* __restrict__ c) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s = fmaf(expf(nc_ld<T>(out, (size_t)b * K + k) * inv_eps), r[b], s);
  c[k] = 1.f / (s * (float)K);   // after this, sum_b E r c = 1 / K for every prototype
}

template <typename T>
__global__ __launch_bounds__(256) void sk_sample_kernel(const T* __restrict__ out, const float* __restrict__ c, int B, int K,
                                                        float inv_eps, float* __restrict__ r) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) s = fmaf(expf(nc_ld<T>(out, (size_t)b * K + k) * inv_eps), c[k], s);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) r[b] = 1.f / ((red[0] + red[1] + red[2] + red[3]) * (float)B);
}

template <typename T>
__global__ __launch_bounds__(256) void sk_write_kernel(const T* __restrict__ out, const float* __restrict__ r,
                                                       const float* __restrict__ c, int B, int K, float inv_eps,
                                                       float* __restrict__ Q) {
  const long long n = (long long)B * K;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / K), k = (int)(i - (long long)b * K);
    Q[i] = expf(nc_ld<T>(out, (size_t)i) * inv_eps) * r[b] * c[k] * (float)B;
  }
}

// iters = 0: lightly's initial Q /= sum(Q) is all that happens (with iters > 0 the first prototype pass absorbs it).
// r[b] holds 1 / (B sum_k E[b][k]) from sk_sample_kernel with c = 1; every r[b] becomes 1 / sum_{b,k} E.  One block.
__global__ __launch_bounds__(256) void sk_total_kernel(float* __restrict__ r, int B) {
  __shared__ float red[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) s += 1.f / r[b];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float inv_total = (float)B / (red[0] + red[1] + red[2] + red[3]);
  for (int b = threadIdx.x; b < B; b += 256) r[b] = inv_total;   // (a thread rewrites only the entries it read)
}

__global__ void sk_fill_kernel(float* p, int n, float v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

template <typename T>
int sinkhorn_impl(const void* out, int B, int K, float eps, int iters, float* Q, float* ws, hipStream_t st) {
  const T* x = static_cast<const T*>(out);
  float* r = ws;
  float* c = ws + B;
  const float inv = 1.f / eps;
  // r = 1, c = 1 (the initial Q /= sum(Q) is absorbed by the first prototype pass; iters = 0 applies it on its own)
  sk_fill_kernel<<<wm_cdiv(B + K, 256), 256, 0, st>>>(ws, B + K, 1.f);
  WM_LAUNCH_CHECK();
  if (iters == 0) {
    sk_sample_kernel<T><<<B, 256, 0, st>>>(x, c, B, K, inv, r);
    WM_LAUNCH_CHECK();
    sk_total_kernel<<<1, 256, 0, st>>>(r, B);
    WM_LAUNCH_CHECK();
  }
  for (int it = 0; it < iters; ++it) {
    sk_proto_kernel<T><<<wm_cdiv(K, 256), 256, 0, st>>>(x, r, B, K, inv, c);
    WM_LAUNCH_CHECK();
    sk_sample_kernel<T><<<B, 256, 0, st>>>(x, c, B, K, inv, r);
    WM_LAUNCH_CHECK();
  }
  const long long n = (long long)B * K;
  sk_write_kernel<T><<<(int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256), 256, 0, st>>>(x, r, c, B, K, inv, Q);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
}  // namespace

extern "C" int wm_sinkhorn(const void* out, int dtype, int B, int K, float eps, int iters, float* Q, float* workspace,
                           void* stream) {
  WM_REQUIRE(out && Q && workspace, WM_EINVAL);
  WM_REQUIRE(B > 0 && K > 0 && eps > 0.f && iters >= 0 && iters <= 100, WM_EINVAL);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == WM_F32 ? sinkhorn_impl<float>(out, B, K, eps, iters, Q, workspace, st)
                         : sinkhorn_impl<uint16_t>(out, B, K, eps, iters, Q, workspace, st);
}
