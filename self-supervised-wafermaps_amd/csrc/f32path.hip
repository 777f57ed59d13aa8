// Float32 "parity" preset: the forward pass of the three models of the path with EVERY activation, weight and
// accumulator in float32 (fmaf chains, double for the normalisation statistics).
//
// Why it exists (profiles/r04_error_budget_bf16.md): north_star asks the whole-step loss within 1e-4 relative and the
// embeddings within 1e-3 cosine of the reference's float32 CPU path.  The production kernels keep activations and
// MFMA operands in bf16 (2^-9 per stored value); the error budget shows that this storage -- not a kernel defect --
// puts the SimCLR / DINO / MAE step losses 0.4e-4 .. 3.4e-4 from the float32 oracle, the same distance torch's own
// bf16 autocast of the oracle code lands at (profiles/r04_bf16_gradient_noise.md).  This file is the preset that keeps
// those activations in float32: same module tree, same state_dict, same call sites
// (scripts/WM811k_benchmark.py:236-248 SimCLR, :578-588 DINOViT, :902-947 MAE), plain loops instead of MFMA tiles.
// It is a validation preset (~50x slower than the bf16 path): forward for all three models, backward for the ResNet-18 /
// projection-head ops (whole SimCLR optimiser steps follow the oracle to 1e-5) and for the MAE / SimMIM transformer ops
// (LayerNorm, GELU, attention, MSE / L1; DINO's loss has no backward here yet).
//
// Layouts: activations NHWC float32 ([rows][C] for token / feature matrices), weights in their float32 master layout
// (OIHW / [K][C]); the implicit-GEMM kernel reads them through a [R*S*C][K] copy made per call.
#include "common.h"
#include <math.h>

namespace {

constexpr int FT = 256;

__global__ __launch_bounds__(FT) void f32_weights_qk(const float* __restrict__ w, int K, int C, int RS, float* __restrict__ wt) {
  const size_t total = (size_t)K * C * RS;
  for (size_t i = (size_t)blockIdx.x * FT + threadIdx.x; i < total; i += (size_t)gridDim.x * FT) {
    const int k = (int)(i % K);
    const size_t q = i / K;
    const int c = (int)(q % C), rs = (int)(q / C);
    wt[i] = w[((size_t)k * C + c) * RS + rs];
  }
}

__device__ __forceinline__ float f32_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

struct F32Conv {
  const float* x;    // source tensor [N][SH][SW][SC]: the input (forward) or the output gradient (input gradient)
  const float* wt;   // [R*S*SC][DC]
  const float* bias; // [DC] or null
  const float* res;  // [M][DC] or null
  float* y;          // [M][DC], M = N*DH*DW
  int N, SH, SW, SC, DH, DW, DC, R, S, stride, pad, act;
};

// weights OIHW [K][C][R][S] -> [R*S*K][C] (the input gradient reduces over (tap, output channel))
__global__ __launch_bounds__(FT) void f32_weights_qc(const float* __restrict__ w, int K, int C, int RS, float* __restrict__ wt) {
  const size_t total = (size_t)K * C * RS;
  for (size_t i = (size_t)blockIdx.x * FT + threadIdx.x; i < total; i += (size_t)gridDim.x * FT) {
    const int c = (int)(i % C);
    const size_t q = i / C;
    const int k = (int)(q % K), rs = (int)(q / K);
    wt[i] = w[((size_t)k * C + c) * RS + rs];
  }
}

// Implicit GEMM, 64 x 64 output tile per block, 16-deep reduction steps over the flattened (r, s, source channel) index,
// 4 x 4 outputs per thread; the reduction runs in increasing index order as one fmaf chain per output.
// DGRAD = false: forward, source pixel of tap (r, s) = (dh * stride - pad + r, dw * stride - pad + s).
// DGRAD = true : input gradient, source = output-gradient pixel ((dh + pad - r) / stride, (dw + pad - s) / stride) where
//                both divide exactly (a tap that does not hit an output pixel contributes nothing).
template <bool DGRAD>
__global__ __launch_bounds__(FT) void f32_conv_kernel(const F32Conv a) {
  __shared__ __attribute__((aligned(16))) float As[16][68];
  __shared__ __attribute__((aligned(16))) float Bs[16][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long M = (long long)a.N * a.DH * a.DW;
  const long long m0 = (long long)blockIdx.x * 64;
  const int n0 = blockIdx.y * 64;
  const int Kd = a.R * a.S * a.SC;
  const int ql = tid & 15;
  long long rbase[4];
  int rh[4], rw[4];
  bool rv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long m = m0 + (tid >> 4) + 16 * i;
    rv[i] = m < M;
    const long long mm = rv[i] ? m : 0;
    const int n = (int)(mm / ((long long)a.DH * a.DW));
    const int pq = (int)(mm - (long long)n * a.DH * a.DW);
    const int p = pq / a.DW, q = pq - p * a.DW;
    rh[i] = DGRAD ? p + a.pad : p * a.stride - a.pad;
    rw[i] = DGRAD ? q + a.pad : q * a.stride - a.pad;
    rbase[i] = (long long)n * a.SH * a.SW;
  }
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < Kd; k0 += 16) {
    const int qg = k0 + ql;
    const bool qv = qg < Kd;
    const int qq = qv ? qg : 0;
    const int r = qq / (a.S * a.SC);
    const int rem = qq - r * a.S * a.SC;
    const int s = rem / a.SC, c = rem - s * a.SC;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int h, w;
      bool ok = rv[i] && qv;
      if constexpr (DGRAD) {
        const int th = rh[i] - r, tw = rw[i] - s;
        ok = ok && th >= 0 && tw >= 0 && th % a.stride == 0 && tw % a.stride == 0;
        h = th / a.stride;
        w = tw / a.stride;
      } else {
        h = rh[i] + r;
        w = rw[i] + s;
      }
      float v = 0.f;
      if (ok && (unsigned)h < (unsigned)a.SH && (unsigned)w < (unsigned)a.SW)
        v = a.x[((rbase[i] + (long long)h * a.SW + w) * a.SC) + c];
      As[ql][(tid >> 4) + 16 * i] = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * FT;
      const int col = e & 63, qr = e >> 6;
      float v = 0.f;
      if (k0 + qr < Kd && n0 + col < a.DC) v = a.wt[(size_t)(k0 + qr) * a.DC + n0 + col];
      Bs[qr][col] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float4 av = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]);
      const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long m = m0 + ty * 4 + i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = n0 + tx * 4 + j;
      if (k >= a.DC) continue;
      float v = acc[i][j];
      if (a.bias) v += a.bias[k];
      if (a.act == 1) v = f32_gelu(v);
      else if (a.act == 2) v = fmaxf(v, 0.f);
      if (a.res) v += a.res[m * a.DC + k];
      a.y[m * a.DC + k] = v;
    }
  }
}

// Weight gradient: dw[k][(r, s, c)] = sum over output pixels m of dy[m][k] * x[pixel m shifted by tap (r, s)][c].
// 64 x 64 tile of (k, column) per block, pixel range z of Z per block (its partial sums go to slab z: ordered sum afterwards).
struct F32Wgrad {
  const float* dy;  // [M][K]
  const float* x;   // [N][H][W][C]
  float* slabs;     // [Z][K][R*S*C]
  int N, H, W, C, K, R, S, P, Q, stride, pad;
  long long chunk;  // pixels per slab
};
__global__ __launch_bounds__(FT) void f32_conv_wgrad(const F32Wgrad a) {
  __shared__ __attribute__((aligned(16))) float As[16][68];
  __shared__ __attribute__((aligned(16))) float Bs[16][68];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long M = (long long)a.N * a.P * a.Q;
  const int RSC = a.R * a.S * a.C;
  const int k0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  const long long mb = (long long)blockIdx.z * a.chunk;
  long long me = mb + a.chunk;
  if (me > M) me = M;
  // this thread's column (tap, channel) for the B fetch: fixed for the whole block
  const int jl = tid & 63;
  const int j = j0 + jl;
  const bool jv = j < RSC;
  const int jj = jv ? j : 0;
  const int r = jj / (a.S * a.C);
  const int rem = jj - r * a.S * a.C;
  const int s = rem / a.C, c = rem - s * a.C;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
  for (long long m0 = mb; m0 < me; m0 += 16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = (tid >> 6) + 4 * i;          // pixel of the step: 0 .. 15
      const long long m = m0 + kk;
      float va = 0.f, vb = 0.f;
      if (m < me) {
        if (k0 + jl < a.K) va = a.dy[m * a.K + k0 + jl];
        if (jv) {
          const int n = (int)(m / ((long long)a.P * a.Q));
          const int pq = (int)(m - (long long)n * a.P * a.Q);
          const int p = pq / a.Q, q = pq - p * a.Q;
          const int h = p * a.stride - a.pad + r, w = q * a.stride - a.pad + s;
          if ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W)
            vb = a.x[(((long long)n * a.H + h) * a.W + w) * a.C + c];
        }
      }
      As[kk][jl] = va;
      Bs[kk][jl] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float4 av = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]);
      const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(aa[i], bb[q], acc[i][q]);
    }
    __syncthreads();
  }
  float* slab = a.slabs + (size_t)blockIdx.z * a.K * RSC;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + ty * 4 + i;
    if (k >= a.K) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = j0 + tx * 4 + q;
      if (col < RSC) slab[(size_t)k * RSC + col] = acc[i][q];
    }
  }
}

// dw OIHW [K][C][R][S] = sum over slabs (in slab order, double) of slab[z][k][(r, s, c)]
__global__ __launch_bounds__(FT) void f32_wgrad_finalize(const float* __restrict__ slabs, int Z, int K, int C, int RS,
                                                        float* __restrict__ dw) {
  const size_t total = (size_t)K * C * RS;
  for (size_t i = (size_t)blockIdx.x * FT + threadIdx.x; i < total; i += (size_t)gridDim.x * FT) {
    const int rs = (int)(i % RS);
    const size_t t = i / RS;
    const int c = (int)(t % C), k = (int)(t / C);
    double v = 0.0;
    for (int z = 0; z < Z; ++z) v += (double)slabs[((size_t)z * K + k) * ((size_t)RS * C) + (size_t)rs * C + c];
    dw[i] = (float)v;
  }
}

// ---- BatchNorm: per (group, channel) sums in double over row slices, ordered finalize, element-wise apply
__global__ __launch_bounds__(FT) void f32_colsums(const float* __restrict__ y, long long rpg, int C, int RB,
                                                 double* __restrict__ part) {  // part [G][RB][2][C]
  __shared__ double red[2][8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + tx, g = blockIdx.y, rb = blockIdx.z;
  double s = 0.0, ss = 0.0;
  if (c < C) {
    for (long long r = (long long)rb * 8 + ty; r < rpg; r += (long long)RB * 8) {
      const double v = (double)y[((long long)g * rpg + r) * C + c];
      s += v;
      ss += v * v;
    }
  }
  red[0][ty][tx] = s;
  red[1][ty][tx] = ss;
  __syncthreads();
  if (ty == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 8; ++i) {
      a += red[0][i][tx];
      b += red[1][i][tx];
    }
    part[(((size_t)g * RB + rb) * 2 + 0) * C + c] = a;
    part[(((size_t)g * RB + rb) * 2 + 1) * C + c] = b;
  }
}

__global__ __launch_bounds__(FT) void f32_bn_finalize(const double* __restrict__ part, int RB, int G, int C, long long rpg,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                     long long* __restrict__ counter, float* __restrict__ mean,
                                                     float* __restrict__ invstd, float* __restrict__ scale,
                                                     float* __restrict__ shift) {
  const int c = blockIdx.x * FT + threadIdx.x;
  if (counter != nullptr && c == 0) *counter += G;
  if (c >= C) return;
  float rm = rmean ? rmean[c] : 0.f, rv = rvar ? rvar[c] : 0.f;
  for (int g = 0; g < G; ++g) {
    double s = 0.0, ss = 0.0;
    for (int rb = 0; rb < RB; ++rb) {
      s += part[(((size_t)g * RB + rb) * 2 + 0) * C + c];
      ss += part[(((size_t)g * RB + rb) * 2 + 1) * C + c];
    }
    const double m = s / (double)rpg;
    double var = ss / (double)rpg - m * m;
    if (var < 0.0) var = 0.0;
    const float fm = (float)m, is = (float)(1.0 / sqrt(var + (double)eps));
    mean[(size_t)g * C + c] = fm;
    invstd[(size_t)g * C + c] = is;
    const float sc = (gamma ? gamma[c] : 1.f) * is;
    scale[(size_t)g * C + c] = sc;
    shift[(size_t)g * C + c] = (beta ? beta[c] : 0.f) - fm * sc;
    const double unb = rpg > 1 ? var * (double)rpg / (double)(rpg - 1) : var;
    rm = (1.f - momentum) * rm + momentum * fm;
    rv = (1.f - momentum) * rv + momentum * (float)unb;
  }
  if (rmean) rmean[c] = rm;
  if (rvar) rvar[c] = rv;
}

__global__ __launch_bounds__(FT) void f32_bn_eval_coef(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ rmean, const float* __restrict__ rvar, int C,
                                                      float eps, float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * FT + threadIdx.x;
  if (c >= C) return;
  const float is = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
  const float sc = (gamma ? gamma[c] : 1.f) * is;
  scale[c] = sc;
  shift[c] = (beta ? beta[c] : 0.f) - rmean[c] * sc;
}

__global__ __launch_bounds__(FT) void f32_affine_rows(const float* __restrict__ y, const float* __restrict__ res,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     long long rows, int C, long long rpg, int relu, float* __restrict__ out) {
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const int g = (int)(r / rpg);
    float v = fmaf(y[i], scale[(size_t)g * C + c], shift[(size_t)g * C + c]);
    if (res) v += res[i];
    if (relu) v = fmaxf(v, 0.f);
    out[i] = v;
  }
}

__global__ __launch_bounds__(FT) void f32_maxpool3x3s2(const float* __restrict__ x, int N, int H, int W, int C, int P, int Q,
                                                      float* __restrict__ y) {
  const long long total = (long long)N * P * Q * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    const int c = (int)(i % C);
    long long t = i / C;
    const int q = (int)(t % Q);
    t /= Q;
    const int p = (int)(t % P), n = (int)(t / P);
    float m = -INFINITY;
    for (int r = 0; r < 3; ++r)
      for (int s = 0; s < 3; ++s) {
        const int h = 2 * p - 1 + r, w = 2 * q - 1 + s;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) m = fmaxf(m, x[(((long long)n * H + h) * W + w) * C + c]);
      }
    y[i] = m;
  }
}

__global__ __launch_bounds__(FT) void f32_gap(const float* __restrict__ x, int N, int HW, int C, float* __restrict__ y) {
  const int i = blockIdx.x * FT + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  double s = 0.0;
  for (int p = 0; p < HW; ++p) s += (double)x[((long long)n * HW + p) * C + c];
  y[i] = (float)(s / (double)HW);
}

// one wave per row: mean, biased variance (double), normalise
__global__ __launch_bounds__(64) void f32_layernorm(const float* __restrict__ x, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, int C, float* __restrict__ y) {
  const long long row = blockIdx.x;
  const float* xr = x + row * C;
  double s = 0.0;
  for (int c = threadIdx.x; c < C; c += 64) s += (double)xr[c];
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const double mean = s / C;
  double q = 0.0;
  for (int c = threadIdx.x; c < C; c += 64) {
    const double d = (double)xr[c] - mean;
    q += d * d;
  }
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = (float)(1.0 / sqrt(q / C + (double)eps)), fm = (float)mean;
  for (int c = threadIdx.x; c < C; c += 64) y[row * C + c] = (xr[c] - fm) * rstd * gamma[c] + beta[c];
}

__global__ __launch_bounds__(FT) void f32_bias_act(const float* __restrict__ x, const float* __restrict__ bias,
                                                  const float* __restrict__ res, int act, long long rows, int C,
                                                  float* __restrict__ y) {
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    float v = x[i];
    if (bias) v += bias[i % C];
    if (act == 1) v = f32_gelu(v);
    else if (act == 2) v = fmaxf(v, 0.f);
    if (res) v += res[i];
    y[i] = v;
  }
}

// Attention of one (image, head): K and V of the head in LDS, one query per thread (strided), softmax in two passes
// over the keys (maximum, then exponentials) exactly as torch's softmax does.  qkv [B*S][3][H][HD], out [B*S][H*HD].
template <int HD>
__global__ __launch_bounds__(FT) void f32_attention(const float* __restrict__ qkv, int S, int H, float scale,
                                                   float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float f32_smem[];
  float* ks = f32_smem;
  float* vs = f32_smem + (size_t)S * HD;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const size_t rs = (size_t)3 * H * HD;
  for (int i = threadIdx.x; i < S * HD; i += FT) {
    const int j = i / HD, d = i - j * HD;
    const float* base = qkv + ((size_t)b * S + j) * rs + (size_t)h * HD + d;
    ks[i] = base[(size_t)H * HD];
    vs[i] = base[(size_t)2 * H * HD];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S; i += FT) {
    float q[HD], o[HD];
    const float* qp = qkv + ((size_t)b * S + i) * rs + (size_t)h * HD;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      q[d] = qp[d];
      o[d] = 0.f;
    }
    float mx = -INFINITY;
    for (int j = 0; j < S; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) s = fmaf(q[d], ks[j * HD + d], s);
      mx = fmaxf(mx, s * scale);
    }
    float l = 0.f;
    for (int j = 0; j < S; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) s = fmaf(q[d], ks[j * HD + d], s);
      const float p = expf(s * scale - mx);
      l += p;
#pragma unroll
      for (int d = 0; d < HD; ++d) o[d] = fmaf(p, vs[j * HD + d], o[d]);
    }
    const float inv = 1.f / l;
    float* op = out + ((size_t)b * S + i) * ((size_t)H * HD) + (size_t)h * HD;
#pragma unroll
    for (int d = 0; d < HD; ++d) op[d] = o[d] * inv;
  }
}

// rows of softmax((x - sub) * inv_temp) or its logarithm; one block per row
__global__ __launch_bounds__(FT) void f32_softmax_rows(const float* __restrict__ x, const float* __restrict__ sub, float inv_temp,
                                                      int logp, int D, float* __restrict__ y) {
  __shared__ float red[FT];
  const long long row = blockIdx.x;
  const float* xr = x + row * D;
  float m = -INFINITY;
  for (int d = threadIdx.x; d < D; d += FT) m = fmaxf(m, (xr[d] - (sub ? sub[d] : 0.f)) * inv_temp);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = FT / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += FT) s += expf((xr[d] - (sub ? sub[d] : 0.f)) * inv_temp - m);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = FT / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  s = red[0];
  const float ls = logf(s);
  for (int d = threadIdx.x; d < D; d += FT) {
    const float z = (xr[d] - (sub ? sub[d] : 0.f)) * inv_temp - m;
    y[row * D + d] = logp ? z - ls : expf(z) / s;
  }
}

// out[i] = -sum_d p[rows_p(i)][d] * lq[rows_q(i)][d] for the pair list of the DINO / soft cross-entropy losses:
// pair i = (t, s, b), t < T teacher views, s < SV student views, 0 on the diagonal t == s.  One block per pair.
__global__ __launch_bounds__(FT) void f32_pair_ce(const float* __restrict__ p, const float* __restrict__ lq, int T, int SV, int B,
                                                 int D, float* __restrict__ out) {
  __shared__ double red[FT];
  const int i = blockIdx.x;
  const int b = i % B, s = (i / B) % SV, t = i / (B * SV);
  double acc = 0.0;
  if (t != s) {
    const float* pr = p + ((size_t)t * B + b) * D;
    const float* qr = lq + ((size_t)s * B + b) * D;
    for (int d = threadIdx.x; d < D; d += FT) acc += (double)pr[d] * (double)qr[d];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = FT / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[i] = (float)(-red[0]);
}

// *out = scale * sum_i f(a[i], b[i]): mode 0 a[i] (b unused), 1 (a - b)^2, 2 |a - b|; one block, ordered, double
__global__ __launch_bounds__(1024) void f32_reduce(const float* __restrict__ a, const float* __restrict__ b, long long n, int mode,
                                                  double scale, float* __restrict__ out) {
  __shared__ double red[1024];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const double x = (double)a[i];
    if (mode == 0) acc += x;
    else {
      const double d = x - (double)b[i];
      acc += mode == 1 ? d * d : fabs(d);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = (float)(red[0] * scale);
}

// center = center * momentum + (1 - momentum) * column mean of t [rows][D]
__global__ __launch_bounds__(FT) void f32_center_update(float* __restrict__ center, const float* __restrict__ t, int rows, int D,
                                                       float momentum) {
  const int d = blockIdx.x * FT + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += (double)t[(size_t)r * D + d];
  center[d] = center[d] * momentum + (1.f - momentum) * (float)(s / rows);
}

// ---- backward pieces of the ResNet / head path (the float32 preset can take a whole SimCLR optimiser step)
// BatchNorm backward sums: per (group, channel) s1 = sum gm, s2 = sum gm * xhat over the group's rows, gm = the incoming
// gradient taken through the ReLU (out > 0) when `out` is given; doubles, row slices as f32_colsums.
__global__ __launch_bounds__(FT) void f32_bn_bwd_sums(const float* __restrict__ y, const float* __restrict__ g,
                                                     const float* __restrict__ out, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, long long rpg, int C, int RB,
                                                     double* __restrict__ part) {  // [G][RB][2][C]
  __shared__ double red[2][8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + tx, gi = blockIdx.y, rb = blockIdx.z;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float mu = mean[(size_t)gi * C + c], is = invstd[(size_t)gi * C + c];
    for (long long r = (long long)rb * 8 + ty; r < rpg; r += (long long)RB * 8) {
      const size_t o = ((size_t)gi * rpg + r) * C + c;
      float gv = g[o];
      if (out != nullptr && !(out[o] > 0.f)) gv = 0.f;
      s1 += (double)gv;
      s2 += (double)gv * (double)((y[o] - mu) * is);
    }
  }
  red[0][ty][tx] = s1;
  red[1][ty][tx] = s2;
  __syncthreads();
  if (ty == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 8; ++i) {
      a += red[0][i][tx];
      b += red[1][i][tx];
    }
    part[(((size_t)gi * RB + rb) * 2 + 0) * C + c] = a;
    part[(((size_t)gi * RB + rb) * 2 + 1) * C + c] = b;
  }
}

// coef [G][2][C] = (s1 / rows, s2 / rows); dgamma = sum over groups of s2, dbeta = sum of s1
__global__ __launch_bounds__(FT) void f32_bn_bwd_finalize(const double* __restrict__ part, int RB, int G, int C, long long rpg,
                                                         float* __restrict__ coef, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta) {
  const int c = blockIdx.x * FT + threadIdx.x;
  if (c >= C) return;
  double tg = 0.0, tb = 0.0;
  for (int g = 0; g < G; ++g) {
    double s1 = 0.0, s2 = 0.0;
    for (int rb = 0; rb < RB; ++rb) {
      s1 += part[(((size_t)g * RB + rb) * 2 + 0) * C + c];
      s2 += part[(((size_t)g * RB + rb) * 2 + 1) * C + c];
    }
    coef[((size_t)g * 2 + 0) * C + c] = (float)(s1 / (double)rpg);
    coef[((size_t)g * 2 + 1) * C + c] = (float)(s2 / (double)rpg);
    tb += s1;
    tg += s2;
  }
  if (dgamma) dgamma[c] = (float)tg;
  if (dbeta) dbeta[c] = (float)tb;
}

// dy = gamma * invstd * (gm - mean(gm) - xhat * mean(gm * xhat)); dz (gradient of the residual branch) = gm
__global__ __launch_bounds__(FT) void f32_bn_bwd_apply(const float* __restrict__ y, const float* __restrict__ g,
                                                      const float* __restrict__ out, const float* __restrict__ gamma,
                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ coef, long long rows, int C, long long rpg,
                                                      float* __restrict__ dy, float* __restrict__ dz) {
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const int gi = (int)(r / rpg);
    float gv = g[i];
    if (out != nullptr && !(out[i] > 0.f)) gv = 0.f;
    const float is = invstd[(size_t)gi * C + c];
    const float xh = (y[i] - mean[(size_t)gi * C + c]) * is;
    const float c1 = coef[((size_t)gi * 2 + 0) * C + c], c2 = coef[((size_t)gi * 2 + 1) * C + c];
    dy[i] = (gamma ? gamma[c] : 1.f) * is * (gv - c1 - xh * c2);
    if (dz) dz[i] = gv;
  }
}

// max-pool 3x3 / stride 2 / pad 1 backward: every input element collects the gradient of the windows whose FIRST maximum
// (scan order, strict >, as torch's forward records it) it is
__global__ __launch_bounds__(FT) void f32_maxpool3x3s2_bwd(const float* __restrict__ x, const float* __restrict__ dy, int N,
                                                          int H, int W, int C, int P, int Q, float* __restrict__ dx) {
  const long long total = (long long)N * H * W * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    const int c = (int)(i % C);
    long long t = i / C;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H), n = (int)(t / H);
    float acc = 0.f;
    // windows p with 2p - 1 <= h <= 2p + 1: p in {ceil((h - 1) / 2), ..., floor((h + 1) / 2)} (the loop re-checks)
    const int p_lo = h / 2, p_hi = (h + 1) / 2;
    const int q_lo = w / 2, q_hi = (w + 1) / 2;
    for (int p = p_lo; p <= p_hi; ++p) {
      if (p >= P || 2 * p - 1 > h || 2 * p + 1 < h) continue;
      for (int q = q_lo; q <= q_hi; ++q) {
        if (q >= Q || 2 * q - 1 > w || 2 * q + 1 < w) continue;
        float best = -INFINITY;
        int bh = -1, bw = -1;
        for (int r = 0; r < 3; ++r)
          for (int s = 0; s < 3; ++s) {
            const int hh = 2 * p - 1 + r, ww = 2 * q - 1 + s;
            if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) {
              const float v = x[(((long long)n * H + hh) * W + ww) * C + c];
              if (v > best || bh < 0) {
                best = v;
                bh = hh;
                bw = ww;
              }
            }
          }
        if (bh == h && bw == w) acc += dy[(((long long)n * P + p) * Q + q) * C + c];
      }
    }
    dx[i] = acc;
  }
}

__global__ __launch_bounds__(FT) void f32_gap_bwd(const float* __restrict__ dy, int N, int HW, int C, float* __restrict__ dx) {
  const long long total = (long long)N * HW * C;
  const float inv = 1.f / (float)HW;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    const int c = (int)(i % C);
    const int n = (int)(i / ((long long)HW * C));
    dx[i] = dy[(size_t)n * C + c] * inv;
  }
}

// out[c] = sum over rows of x[r][c] (bias gradients): one thread per column, double
__global__ __launch_bounds__(FT) void f32_colsum(const float* __restrict__ x, long long rows, int C, float* __restrict__ out) {
  const int c = blockIdx.x * FT + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (long long r = 0; r < rows; ++r) s += (double)x[r * C + c];
  out[c] = (float)s;
}

// ---- backward pieces of the transformer path (MAE / SimMIM optimiser steps under the preset)
// LayerNorm backward, one wave per row: the forward's statistics recomputed with the same arithmetic (double sums, float
// mean / rstd); gg = dy * gamma, dx = rstd * (gg - mean(gg) - xhat * mean(gg * xhat)) with the two means in double.  The
// row's (mean, rstd) go to `stats` [rows][2] for the parameter sums.
__global__ __launch_bounds__(64) void f32_layernorm_bwd(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ dy, float eps, int C, float* __restrict__ dx,
                                                       float* __restrict__ stats) {
  const long long row = blockIdx.x;
  const float* xr = x + row * C;
  const float* gr = dy + row * C;
  double s = 0.0;
  for (int c = threadIdx.x; c < C; c += 64) s += (double)xr[c];
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const double mean = s / C;
  double q = 0.0;
  for (int c = threadIdx.x; c < C; c += 64) {
    const double d = (double)xr[c] - mean;
    q += d * d;
  }
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = (float)(1.0 / sqrt(q / C + (double)eps)), fm = (float)mean;
  double a = 0.0, b = 0.0;
  for (int c = threadIdx.x; c < C; c += 64) {
    const float gg = gr[c] * gamma[c];
    a += (double)gg;
    b += (double)gg * (double)((xr[c] - fm) * rstd);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const float ma = (float)(a / C), mb = (float)(b / C);
  for (int c = threadIdx.x; c < C; c += 64) {
    const float xh = (xr[c] - fm) * rstd;
    dx[row * C + c] = rstd * (gr[c] * gamma[c] - ma - xh * mb);
  }
  if (threadIdx.x == 0) {
    stats[row * 2 + 0] = fm;
    stats[row * 2 + 1] = rstd;
  }
}

// LayerNorm parameter sums over row slices (f32_bn_bwd_sums' layout with G = 1, per-row statistics):
// part [RB][2][C] = (sum dy, sum dy * xhat) of slice rb; f32_bn_bwd_finalize adds the slices in order.
__global__ __launch_bounds__(FT) void f32_ln_param_sums(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ stats, long long rows, int C, int RB,
                                                       double* __restrict__ part) {
  __shared__ double red[2][8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + tx, rb = blockIdx.y;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    for (long long r = (long long)rb * 8 + ty; r < rows; r += (long long)RB * 8) {
      const size_t o = (size_t)r * C + c;
      const float gv = dy[o];
      s1 += (double)gv;
      s2 += (double)gv * (double)((x[o] - stats[r * 2 + 0]) * stats[r * 2 + 1]);
    }
  }
  red[0][ty][tx] = s1;
  red[1][ty][tx] = s2;
  __syncthreads();
  if (ty == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 8; ++i) {
      a += red[0][i][tx];
      b += red[1][i][tx];
    }
    part[((size_t)rb * 2 + 0) * C + c] = a;
    part[((size_t)rb * 2 + 1) * C + c] = b;
  }
}

// dx = dy * act'(x + bias): exact GELU' = Phi(v) + v * phi(v), ReLU' = (v > 0); act 0 copies dy
__global__ __launch_bounds__(FT) void f32_act_bwd(const float* __restrict__ x, const float* __restrict__ bias,
                                                 const float* __restrict__ dy, int act, long long rows, int C,
                                                 float* __restrict__ dx) {
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < total; i += (long long)gridDim.x * FT) {
    float g = dy[i];
    if (act != 0) {
      float v = x[i];
      if (bias) v += bias[i % C];
      if (act == 1) {
        const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
        g *= cdf + v * pdf;
      } else if (!(v > 0.f)) {
        g = 0.f;
      }
    }
    dx[i] = g;
  }
}

// d pred = f'(pred - target) * scale * g: mode 1 (MSE) 2 (pred - target), mode 2 (L1) sign(pred - target) (0 at 0);
// g = *grad_out (the loss's incoming gradient, on the device) or 1
__global__ __launch_bounds__(FT) void f32_loss_bwd(const float* __restrict__ pred, const float* __restrict__ target, long long n,
                                                  int mode, float scale, const float* __restrict__ grad_out,
                                                  float* __restrict__ dpred) {
  const float gs = (grad_out ? grad_out[0] : 1.f) * scale;
  for (long long i = (long long)blockIdx.x * FT + threadIdx.x; i < n; i += (long long)gridDim.x * FT) {
    const float d = pred[i] - target[i];
    const float f = mode == 1 ? 2.f * d : (float)((d > 0.f) - (d < 0.f));
    dpred[i] = f * gs;
  }
}

// Attention backward of one (image, head), no atomics.  Every row (query or key) is served by L = HD / 16 adjacent lanes,
// each holding 16 of its head dimensions; dot products are 16-term fmaf chains joined by an xor butterfly (every lane of
// the group ends with the same bits).
//   pass 1 (queries, K and V in LDS): the softmax statistics as the forward takes them (row maximum of s * scale, then the
//          sum of the exponentials), D_i = dO_i . O_i, dq_i = scale * sum_j p_ij (dO_i . v_j - D_i) k_j.
//   pass 2 (keys, Q and dO in LDS in place of K and V, statistics beside them): dv_j = sum_i p_ij dO_i,
//          dk_j = scale * sum_i p_ij (dO_i . v_j - D_i) q_i -- p_ij recomputed from the same operands in the same order.
// LDS: 2 * S * HD + 3 * S floats.  qkv / dqkv [B*S][3][H][HD], out / dout [B*S][H*HD].
template <int L>
__device__ __forceinline__ float f32_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void f32_load16(float* r, const float* p) {
#pragma unroll
  for (int d = 0; d < 16; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + d);
    r[d] = v.x;
    r[d + 1] = v.y;
    r[d + 2] = v.z;
    r[d + 3] = v.w;
  }
}

__device__ __forceinline__ float f32_dot16(const float* r, const float* p) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 16; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + d);
    s = fmaf(r[d], v.x, s);
    s = fmaf(r[d + 1], v.y, s);
    s = fmaf(r[d + 2], v.z, s);
    s = fmaf(r[d + 3], v.w, s);
  }
  return s;
}

template <int HD>
__global__ __launch_bounds__(FT) void f32_attention_bwd(const float* __restrict__ qkv, const float* __restrict__ out,
                                                       const float* __restrict__ dout, int S, int H, float scale,
                                                       float* __restrict__ dqkv) {
  constexpr int L = HD / 16;
  constexpr int RPI = FT / L;  // rows served per iteration
  extern __shared__ __attribute__((aligned(16))) float f32_smem[];
  float* sa = f32_smem;                     // pass 1: K, pass 2: Q
  float* sb = f32_smem + (size_t)S * HD;    // pass 1: V, pass 2: dO
  float* st = f32_smem + (size_t)2 * S * HD;  // [S][3]: row maximum, 1 / sum, D
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
  const int t = threadIdx.x % L, r0 = threadIdx.x / L;
  const int dof = t * 16;
  for (int i = threadIdx.x; i < S * HD; i += FT) {
    const int j = i / HD, d = i - j * HD;
    const float* base = qkv + ((size_t)b * S + j) * rs + (size_t)h * HD + d;
    sa[i] = base[(size_t)H * HD];
    sb[i] = base[(size_t)2 * H * HD];
  }
  __syncthreads();
  for (int i = r0; i < S; i += RPI) {
    float q[16], g[16], acc[16];
    const size_t row = (size_t)b * S + i;
    f32_load16(q, qkv + row * rs + (size_t)h * HD + dof);
    f32_load16(g, dout + row * os + (size_t)h * HD + dof);
    const float dd = f32_group_sum<L>(f32_dot16(g, out + row * os + (size_t)h * HD + dof));
    float mx = -INFINITY;
    for (int j = 0; j < S; ++j) mx = fmaxf(mx, f32_group_sum<L>(f32_dot16(q, sa + (size_t)j * HD + dof)) * scale);
    float l = 0.f;
    for (int j = 0; j < S; ++j) l += expf(f32_group_sum<L>(f32_dot16(q, sa + (size_t)j * HD + dof)) * scale - mx);
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] = 0.f;
    for (int j = 0; j < S; ++j) {
      const float* kj = sa + (size_t)j * HD + dof;
      const float p = expf(f32_group_sum<L>(f32_dot16(q, kj)) * scale - mx) * inv;
      const float dp = f32_group_sum<L>(f32_dot16(g, sb + (size_t)j * HD + dof));
      const float ds = p * (dp - dd);
#pragma unroll
      for (int d = 0; d < 16; ++d) acc[d] = fmaf(ds, kj[d], acc[d]);
    }
    float* dq = dqkv + row * rs + (size_t)h * HD + dof;
#pragma unroll
    for (int d = 0; d < 16; ++d) dq[d] = acc[d] * scale;
    if (t == 0) {
      st[i * 3 + 0] = mx;
      st[i * 3 + 1] = inv;
      st[i * 3 + 2] = dd;
    }
  }
  __syncthreads();  // K and V are read no more: Q and dO take their place
  for (int i = threadIdx.x; i < S * HD; i += FT) {
    const int j = i / HD, d = i - j * HD;
    sa[i] = qkv[((size_t)b * S + j) * rs + (size_t)h * HD + d];
    sb[i] = dout[((size_t)b * S + j) * os + (size_t)h * HD + d];
  }
  __syncthreads();
  for (int j = r0; j < S; j += RPI) {
    float k[16], v[16], dk[16], dv[16];
    const size_t row = (size_t)b * S + j;
    f32_load16(k, qkv + row * rs + (size_t)H * HD + (size_t)h * HD + dof);
    f32_load16(v, qkv + row * rs + (size_t)2 * H * HD + (size_t)h * HD + dof);
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      dk[d] = 0.f;
      dv[d] = 0.f;
    }
    for (int i = 0; i < S; ++i) {
      const float* qi = sa + (size_t)i * HD + dof;
      const float* gi = sb + (size_t)i * HD + dof;
      // the same fmaf chain as pass 1's q . k_j (query operand first)
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) s = fmaf(qi[d], k[d], s);
      const float p = expf(f32_group_sum<L>(s) * scale - st[i * 3 + 0]) * st[i * 3 + 1];
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) dp = fmaf(gi[d], v[d], dp);
      const float ds = p * (f32_group_sum<L>(dp) - st[i * 3 + 2]);
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        dv[d] = fmaf(p, gi[d], dv[d]);
        dk[d] = fmaf(ds, qi[d], dk[d]);
      }
    }
    float* dkp = dqkv + row * rs + (size_t)H * HD + (size_t)h * HD + dof;
    float* dvp = dqkv + row * rs + (size_t)2 * H * HD + (size_t)h * HD + dof;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      dkp[d] = dk[d] * scale;
      dvp[d] = dv[d];
    }
  }
}

inline int grid_for(long long items) {
  long long b = (items + FT - 1) / FT;
  if (b > 65535) b = 65535;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" size_t wm_f32_conv2d_workspace_bytes(int C, int K, int R, int S) {
  if (C <= 0 || K <= 0 || R <= 0 || S <= 0) return 0;
  return (size_t)R * S * C * K * sizeof(float);
}

extern "C" int wm_f32_conv2d_fwd(const float* x, const float* w_oihw, const float* bias, const float* residual, float* y, int N,
                                 int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad, int act,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && w_oihw && y && workspace, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0 && stride > 0 && pad >= 0, WM_EINVAL);
  WM_REQUIRE(P == (H + 2 * pad - R) / stride + 1 && Q == (W + 2 * pad - S) / stride + 1 && P > 0 && Q > 0, WM_EINVAL);
  WM_REQUIRE(act >= 0 && act <= 2, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_conv2d_workspace_bytes(C, K, R, S), WM_EWORKSPACE);
  const long long M = (long long)N * P * Q;
  WM_REQUIRE((M + 63) / 64 < (1ll << 31) && (long long)R * S * C < (1ll << 31), WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* wt = static_cast<float*>(workspace);
  f32_weights_qk<<<grid_for((long long)K * C * R * S), FT, 0, st>>>(w_oihw, K, C, R * S, wt);
  WM_LAUNCH_CHECK();
  F32Conv a{x, wt, bias, residual, y, N, H, W, C, P, Q, K, R, S, stride, pad, act};
  f32_conv_kernel<false><<<dim3((unsigned)((M + 63) / 64), (unsigned)((K + 63) / 64)), FT, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_f32_bn_workspace_bytes(long long rows, int C, int G) {
  if (rows <= 0 || C <= 0 || G <= 0) return 0;
  const int RB = 64;
  return ((size_t)G * RB * 2 * C) * sizeof(double) + (size_t)2 * G * C * sizeof(float) + 64;
}

extern "C" int wm_f32_bn_fwd(const float* y, const float* residual, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, long long* num_batches_tracked, long long rows, int C, int G, int training,
                             float eps, float momentum, int relu, float* save_mean, float* save_invstd, float* out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(y && out && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && C > 0 && G > 0 && rows % G == 0, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_bn_workspace_bytes(rows, C, G), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int RB = 64;
  double* part = static_cast<double*>(workspace);
  float* scale = reinterpret_cast<float*>(part + (size_t)G * RB * 2 * C);
  float* shift = scale + (size_t)G * C;
  const long long rpg = rows / G;
  if (training) {
    WM_REQUIRE(save_mean && save_invstd, WM_EINVAL);
    f32_colsums<<<dim3((C + 31) / 32, G, RB), FT, 0, st>>>(y, rpg, C, RB, part);
    WM_LAUNCH_CHECK();
    f32_bn_finalize<<<(C + FT - 1) / FT, FT, 0, st>>>(part, RB, G, C, rpg, gamma, beta, eps, momentum, running_mean, running_var,
                                                     num_batches_tracked, save_mean, save_invstd, scale, shift);
    WM_LAUNCH_CHECK();
    f32_affine_rows<<<grid_for(rows * C), FT, 0, st>>>(y, residual, scale, shift, rows, C, rpg, relu, out);
  } else {
    WM_REQUIRE(running_mean && running_var, WM_EINVAL);
    f32_bn_eval_coef<<<(C + FT - 1) / FT, FT, 0, st>>>(gamma, beta, running_mean, running_var, C, eps, scale, shift);
    WM_LAUNCH_CHECK();
    f32_affine_rows<<<grid_for(rows * C), FT, 0, st>>>(y, residual, scale, shift, rows, C, rows, relu, out);
  }
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_maxpool3x3s2(const float* x, int N, int H, int W, int C, float* y, void* stream) {
  WM_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0, WM_EINVAL);
  const int P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  f32_maxpool3x3s2<<<grid_for((long long)N * P * Q * C), FT, 0, static_cast<hipStream_t>(stream)>>>(x, N, H, W, C, P, Q, y);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_gap(const float* x, int N, int HW, int C, float* y, void* stream) {
  WM_REQUIRE(x && y && N > 0 && HW > 0 && C > 0, WM_EINVAL);
  f32_gap<<<(N * C + FT - 1) / FT, FT, 0, static_cast<hipStream_t>(stream)>>>(x, N, HW, C, y);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_layernorm(const float* x, const float* gamma, const float* beta, float eps, long long rows, int C, float* y,
                                void* stream) {
  WM_REQUIRE(x && gamma && beta && y && rows > 0 && rows < (1ll << 31) && C > 0, WM_EINVAL);
  f32_layernorm<<<(unsigned)rows, 64, 0, static_cast<hipStream_t>(stream)>>>(x, gamma, beta, eps, C, y);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_bias_act(const float* x, const float* bias, const float* residual, int act, long long rows, int C, float* y,
                               void* stream) {
  WM_REQUIRE(x && y && rows > 0 && C > 0 && act >= 0 && act <= 2, WM_EINVAL);
  f32_bias_act<<<grid_for(rows * C), FT, 0, static_cast<hipStream_t>(stream)>>>(x, bias, residual, act, rows, C, y);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_attention(const float* qkv, int B, int S, int H, int HD, float scale, float* out, void* stream) {
  WM_REQUIRE(qkv && out && B > 0 && S > 0 && H > 0, WM_EINVAL);
  WM_REQUIRE(HD == 64 || HD == 32, WM_EUNSUPPORTED);
  const size_t lds = (size_t)2 * S * HD * sizeof(float);
  WM_REQUIRE(lds <= 160 * 1024, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (HD == 64) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&f32_attention<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    f32_attention<64><<<B * H, FT, lds, st>>>(qkv, S, H, scale, out);
  } else {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&f32_attention<32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    f32_attention<32><<<B * H, FT, lds, st>>>(qkv, S, H, scale, out);
  }
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_softmax_rows(const float* x, const float* subtract, float inv_temp, int log_softmax, long long rows, int D,
                                   float* y, void* stream) {
  WM_REQUIRE(x && y && rows > 0 && rows < (1ll << 31) && D > 0, WM_EINVAL);
  f32_softmax_rows<<<(unsigned)rows, FT, 0, static_cast<hipStream_t>(stream)>>>(x, subtract, inv_temp, log_softmax, D, y);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_pair_ce(const float* probs, const float* logq, int T, int SV, int B, int D, float* pair_loss, void* stream) {
  WM_REQUIRE(probs && logq && pair_loss && T > 0 && SV > 0 && B > 0 && D > 0, WM_EINVAL);
  f32_pair_ce<<<T * SV * B, FT, 0, static_cast<hipStream_t>(stream)>>>(probs, logq, T, SV, B, D, pair_loss);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_reduce(const float* a, const float* b, long long n, int mode, double scale, float* out, void* stream) {
  WM_REQUIRE(a && out && n > 0 && mode >= 0 && mode <= 2 && (mode == 0 || b), WM_EINVAL);
  f32_reduce<<<1, 1024, 0, static_cast<hipStream_t>(stream)>>>(a, b, n, mode, scale, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_center_update(float* center, const float* teacher, int rows, int D, float momentum, void* stream) {
  WM_REQUIRE(center && teacher && rows > 0 && D > 0, WM_EINVAL);
  f32_center_update<<<(D + FT - 1) / FT, FT, 0, static_cast<hipStream_t>(stream)>>>(center, teacher, rows, D, momentum);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_conv2d_dgrad(const float* dy, const float* w_oihw, float* dx, int N, int H, int W, int C, int K, int R, int S,
                                   int P, int Q, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(dy && w_oihw && dx && workspace, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0 && stride > 0 && pad >= 0, WM_EINVAL);
  WM_REQUIRE(P == (H + 2 * pad - R) / stride + 1 && Q == (W + 2 * pad - S) / stride + 1 && P > 0 && Q > 0, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_conv2d_workspace_bytes(C, K, R, S), WM_EWORKSPACE);
  const long long M = (long long)N * H * W;
  WM_REQUIRE((M + 63) / 64 < (1ll << 31) && (long long)R * S * K < (1ll << 31), WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* wt = static_cast<float*>(workspace);
  f32_weights_qc<<<grid_for((long long)K * C * R * S), FT, 0, st>>>(w_oihw, K, C, R * S, wt);
  WM_LAUNCH_CHECK();
  // rows = input pixels, source = the output gradient [N][P][Q][K], reduction over (tap, output channel)
  F32Conv a{dy, wt, nullptr, nullptr, dx, N, P, Q, K, H, W, C, R, S, stride, pad, 0};
  f32_conv_kernel<true><<<dim3((unsigned)((M + 63) / 64), (unsigned)((C + 63) / 64)), FT, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// Pixel ranges of the weight gradient: 4096 pixels per slab for the convolutions; 256 rows for a Linear layer (the 1 x 1 case
// on a 1 x 1 image, rows = tokens).  A transformer's weight gradients are the bulk of its gradient, and one 1576-term float
// chain per weight (the MAE decoder's 8 x 197 tokens) put them 3x further from float64 than a blocked float32 GEMM lands;
// slabs of 256 rows summed in double do not.  (A SimCLR projection head at batch 64, 128 rows, stays in one slab.)
static int f32_wgrad_slabs(long long M, bool linear) {
  const long long chunk = linear ? 256 : 4096;
  long long z = (M + chunk - 1) / chunk;
  if (z > 256) z = 256;
  if (z < 1) z = 1;
  return (int)z;
}

extern "C" size_t wm_f32_conv2d_wgrad_workspace_bytes(int N, int P, int Q, int C, int K, int R, int S) {
  if (N <= 0 || P <= 0 || Q <= 0 || C <= 0 || K <= 0 || R <= 0 || S <= 0) return 0;
  const bool linear = P == 1 && Q == 1 && R == 1 && S == 1;
  return (size_t)f32_wgrad_slabs((long long)N * P * Q, linear) * K * R * S * C * sizeof(float);
}

extern "C" int wm_f32_conv2d_wgrad(const float* dy, const float* x, float* dw_oihw, int N, int H, int W, int C, int K, int R,
                                   int S, int P, int Q, int stride, int pad, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  WM_REQUIRE(dy && x && dw_oihw && workspace, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0 && stride > 0 && pad >= 0, WM_EINVAL);
  WM_REQUIRE(P == (H + 2 * pad - R) / stride + 1 && Q == (W + 2 * pad - S) / stride + 1 && P > 0 && Q > 0, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_conv2d_wgrad_workspace_bytes(N, P, Q, C, K, R, S), WM_EWORKSPACE);
  const long long M = (long long)N * P * Q;
  const int Z = f32_wgrad_slabs(M, P == 1 && Q == 1 && R == 1 && S == 1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  F32Wgrad a{dy, x, static_cast<float*>(workspace), N, H, W, C, K, R, S, P, Q, stride, pad, (M + Z - 1) / Z};
  f32_conv_wgrad<<<dim3((K + 63) / 64, (R * S * C + 63) / 64, Z), FT, 0, st>>>(a);
  WM_LAUNCH_CHECK();
  f32_wgrad_finalize<<<grid_for((long long)K * C * R * S), FT, 0, st>>>(static_cast<const float*>(workspace), Z, K, C, R * S, dw_oihw);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_colsum(const float* x, long long rows, int C, float* out, void* stream) {
  WM_REQUIRE(x && out && rows > 0 && C > 0, WM_EINVAL);
  f32_colsum<<<(C + FT - 1) / FT, FT, 0, static_cast<hipStream_t>(stream)>>>(x, rows, C, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_bn_bwd(const float* y, const float* dout, const float* out_relu, const float* gamma, const float* save_mean,
                             const float* save_invstd, long long rows, int C, int G, float* dgamma, float* dbeta, float* dy,
                             float* dz, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(y && dout && save_mean && save_invstd && dy && workspace, WM_EINVAL);
  WM_REQUIRE(rows > 0 && C > 0 && G > 0 && rows % G == 0, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_bn_workspace_bytes(rows, C, G), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int RB = 64;
  double* part = static_cast<double*>(workspace);
  float* coef = reinterpret_cast<float*>(part + (size_t)G * RB * 2 * C);   // [G][2][C]: the forward's scale / shift space
  const long long rpg = rows / G;
  f32_bn_bwd_sums<<<dim3((C + 31) / 32, G, RB), FT, 0, st>>>(y, dout, out_relu, save_mean, save_invstd, rpg, C, RB, part);
  WM_LAUNCH_CHECK();
  f32_bn_bwd_finalize<<<(C + FT - 1) / FT, FT, 0, st>>>(part, RB, G, C, rpg, coef, dgamma, dbeta);
  WM_LAUNCH_CHECK();
  f32_bn_bwd_apply<<<grid_for(rows * C), FT, 0, st>>>(y, dout, out_relu, gamma, save_mean, save_invstd, coef, rows, C, rpg, dy, dz);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_maxpool3x3s2_bwd(const float* x, const float* dy, int N, int H, int W, int C, float* dx, void* stream) {
  WM_REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && C > 0, WM_EINVAL);
  const int P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  f32_maxpool3x3s2_bwd<<<grid_for((long long)N * H * W * C), FT, 0, static_cast<hipStream_t>(stream)>>>(x, dy, N, H, W, C, P, Q, dx);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_gap_bwd(const float* dy, int N, int HW, int C, float* dx, void* stream) {
  WM_REQUIRE(dy && dx && N > 0 && HW > 0 && C > 0, WM_EINVAL);
  f32_gap_bwd<<<grid_for((long long)N * HW * C), FT, 0, static_cast<hipStream_t>(stream)>>>(dy, N, HW, C, dx);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_f32_layernorm_bwd_workspace_bytes(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  const int RB = 64;
  return (size_t)RB * 2 * C * sizeof(double) + (size_t)2 * C * sizeof(float) + (size_t)rows * 2 * sizeof(float);
}

extern "C" int wm_f32_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, long long rows, int C,
                                    float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  WM_REQUIRE(x && gamma && dy && dx && workspace && rows > 0 && rows < (1ll << 31) && C > 0, WM_EINVAL);
  WM_REQUIRE(workspace_bytes >= wm_f32_layernorm_bwd_workspace_bytes(rows, C), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int RB = 64;
  double* part = static_cast<double*>(workspace);                        // [RB][2][C]
  float* coef = reinterpret_cast<float*>(part + (size_t)RB * 2 * C);      // [2][C] (finalize's by-product, unused)
  float* stats = coef + (size_t)2 * C;                                    // [rows][2]
  f32_layernorm_bwd<<<(unsigned)rows, 64, 0, st>>>(x, gamma, dy, eps, C, dx, stats);
  WM_LAUNCH_CHECK();
  if (dgamma || dbeta) {
    f32_ln_param_sums<<<dim3((C + 31) / 32, RB), FT, 0, st>>>(x, dy, stats, rows, C, RB, part);
    WM_LAUNCH_CHECK();
    f32_bn_bwd_finalize<<<(C + FT - 1) / FT, FT, 0, st>>>(part, RB, 1, C, rows, coef, dgamma, dbeta);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}

extern "C" int wm_f32_bias_act_bwd(const float* x, const float* bias, const float* dy, int act, long long rows, int C, float* dx,
                                   void* stream) {
  WM_REQUIRE(dy && dx && rows > 0 && C > 0 && act >= 0 && act <= 2 && (act == 0 || x), WM_EINVAL);
  f32_act_bwd<<<grid_for(rows * C), FT, 0, static_cast<hipStream_t>(stream)>>>(x, bias, dy, act, rows, C, dx);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_attention_bwd(const float* qkv, const float* out, const float* dout, int B, int S, int H, int HD,
                                    float scale, float* dqkv, void* stream) {
  WM_REQUIRE(qkv && out && dout && dqkv && B > 0 && S > 0 && H > 0, WM_EINVAL);
  WM_REQUIRE(HD == 64 || HD == 32, WM_EUNSUPPORTED);
  const size_t lds = ((size_t)2 * S * HD + (size_t)3 * S) * sizeof(float);
  WM_REQUIRE(lds <= 160 * 1024, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (HD == 64) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&f32_attention_bwd<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return (int)e;
    f32_attention_bwd<64><<<B * H, FT, lds, st>>>(qkv, out, dout, S, H, scale, dqkv);
  } else {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&f32_attention_bwd<32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return (int)e;
    f32_attention_bwd<32><<<B * H, FT, lds, st>>>(qkv, out, dout, S, H, scale, dqkv);
  }
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_f32_loss_bwd(const float* pred, const float* target, long long n, int mode, double scale, const float* grad_out,
                               float* dpred, void* stream) {
  WM_REQUIRE(pred && target && dpred && n > 0 && (mode == 1 || mode == 2), WM_EINVAL);
  f32_loss_bwd<<<grid_for(n), FT, 0, static_cast<hipStream_t>(stream)>>>(pred, target, n, mode, (float)scale, grad_out, dpred);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
