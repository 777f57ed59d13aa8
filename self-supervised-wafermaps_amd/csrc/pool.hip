// Max-pool 3x3/2 (ResNet stem) and global average pool, NHWC bf16.
//
// Replaces nn.MaxPool2d(3, 2, 1) and the SelectAdaptivePool2d(avg) of timm's resnet18 in the
// reference (scripts/WM811k_benchmark.py:231).  The forward records the winning window position
// per output element (first maximum in (kh, kw) scan order, as PyTorch's max_pool2d does — ReLU
// outputs tie at 0 all the time), and the backward is a gather over the <= 4 windows covering an
// input pixel, so no atomics are needed.  Roofline: HBM.
#include "common.h"

namespace {

constexpr int PL_THREADS = 256;
typedef short s16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void up8(const uint4 v, float (&f)[8]) {
  f[0] = bf2f((uint16_t)(v.x & 0xffff)); f[1] = bf2f((uint16_t)(v.x >> 16));
  f[2] = bf2f((uint16_t)(v.y & 0xffff)); f[3] = bf2f((uint16_t)(v.y >> 16));
  f[4] = bf2f((uint16_t)(v.z & 0xffff)); f[5] = bf2f((uint16_t)(v.z >> 16));
  f[6] = bf2f((uint16_t)(v.w & 0xffff)); f[7] = bf2f((uint16_t)(v.w >> 16));
}

__global__ __launch_bounds__(PL_THREADS) void maxpool_fwd(const uint16_t* __restrict__ x, int N, int H,
                                                          int W, int C, int P, int Q,
                                                          uint16_t* __restrict__ y,
                                                          uint8_t* __restrict__ idx) {
  const int cpr = C >> 3;
  const long long total = (long long)N * P * Q * cpr;
  for (long long t = (long long)blockIdx.x * PL_THREADS + threadIdx.x; t < total;
       t += (long long)gridDim.x * PL_THREADS) {
    const int c0 = (int)(t % cpr) * 8;
    long long pix = t / cpr;
    const int q = (int)(pix % Q);
    pix /= Q;
    const int p = (int)(pix % P), n = (int)(pix / P);
    float best[8];
    int bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      best[e] = -INFINITY;
      bi[e] = 0;
    }
    bool first = true;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int h = p * 2 - 1 + kh, w = q * 2 - 1 + kw;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
          float f[8];
          up8(*reinterpret_cast<const uint4*>(x + ((size_t)(n * H + h) * W + w) * C + c0), f);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (first || f[e] > best[e]) {
              best[e] = f[e];
              bi[e] = kh * 3 + kw;
            }
          first = false;
        }
      }
    const size_t o = ((size_t)(n * P + p) * Q + q) * C + c0;
    *reinterpret_cast<uint4*>(y + o) = make_uint4(pack_bf2(best[0], best[1]), pack_bf2(best[2], best[3]),
                                                  pack_bf2(best[4], best[5]), pack_bf2(best[6], best[7]));
    uint2 pk;
    pk.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    pk.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
    *reinterpret_cast<uint2*>(idx + o) = pk;
  }
}

// Stem: relu(y*scale + shift) is pooled on the fly, so the 112x112x64 activation (the largest tensor
// of the network) is never written or re-read.  scale/shift are [G][C]; a row group = N/G images.
//
// Work assignment.  A window over pooled row p reads the input rows 2p-1, 2p, 2p+1, and row 2p+1 is read again for
// pooled row p+1: with one thread per window, 3 rows are fetched per 2 distinct ones (1.5 x the tensor, which is what
// the one-window form of this kernel measured: 1 246 MB for 822 MB, its two readers of a row sitting 1.75 blocks apart
// in a grid-stride walk, i.e. on two XCDs with two L2s).  Here one thread owns the two vertically adjacent windows
// (2j, q) and (2j+1, q) x 8 channels: five input rows x three columns = 15 loads and 15 transforms for two outputs
// instead of 18 + 18, and the shared row 4j+1 is read and reduced once.  What is left to a cache is row 4j+3, which
// the pair j+1 reads too (5 rows fetched per 4 distinct), and the column 2q+1 shared with the neighbouring lanes.  For
// those, a block owns 256 consecutive items (channel chunk fastest, then q, then j, then n) and the hardware block ids
// are remapped (wm_xcd_swizzle) so that each XCD walks a contiguous range of them: the pairs j and j+1 of one image run
// at the same time on one L2.  When P is odd the last pair's second window does not exist; the same code runs and its
// stores are masked.
//
// Selection.  out = max over the valid window positions of v = bf16(max(fma(y, scale, shift), 0)), idx = kh * 3 + kw of
// the FIRST position in (kh, kw) scan order that attains it, xsel = the raw input there.  v is in [+0, +inf], where the
// bf16 pattern is monotonic as an integer, so a candidate is the integer key (pattern << 16) + (9 - code): the largest
// key is the largest value and, among equal values, the smallest code.  9 - code = (3 - kw) + 3 (2 - kh): the first
// part, 1..3, is added in the step over a row's three columns, the second in the step over the three rows.  The ReLU is
// taken on the pattern as a signed integer, so a -0 becomes +0 like every negative value.  A position outside the image is
// loaded from the clamped address -- row -1 reads row 0, row H reads row H-1, column -1 reads column 0, column W reads
// column W-1: always a valid member of the SAME window with a later code -- and gets 0 in place of its part of the
// code: it carries the value of a position whose key is larger, so it never wins, and no load is conditional.
// NaN: the one-window form took max(NaN, 0) = 0 in float32; here a NaN of fma(y, scale, shift) keeps its bf16 pattern, so
// one with a clear sign bit is the largest candidate and is stored in out, one with the sign bit set becomes 0.  For every
// input whose transform is not NaN the three outputs are those of the one-window form, bit for bit.
template <bool XSEL>
__global__ __launch_bounds__(PL_THREADS, 4) void bn_relu_maxpool_fwd(const uint16_t* __restrict__ x,
                                                                     const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, int N,
                                                                     int H, int W, int C, int P, int Q,
                                                                     uint16_t* __restrict__ y,
                                                                     uint8_t* __restrict__ idx,
                                                                     uint16_t* __restrict__ xsel, const WmDiv d_cpr,
                                                                     const WmDiv d_q, const WmDiv d_p2, const WmDiv d_ipg) {
  // 32-bit arithmetic on 16-byte chunk indices (the host checks N*H*W*C/8 < 2^31): the kernel is VALU-bound
  const uint32_t cpr = (uint32_t)C >> 3;
  const uint32_t total = (uint32_t)N * d_p2.d * (uint32_t)Q * cpr;  // d_p2.d = ceil(P / 2) window pairs per column
  const uint32_t t = wm_xcd_swizzle(blockIdx.x, gridDim.x) * PL_THREADS + threadIdx.x;
  if (t >= total) return;
  uint32_t rc, rq, rj;
  uint32_t pix = wm_divmod(t, d_cpr, rc);
  pix = wm_divmod(pix, d_q, rq);
  const uint32_t n = wm_divmod(pix, d_p2, rj);
  const uint32_t g = wm_div(n, d_ipg);
  const int q = (int)rq, p0 = 2 * (int)rj;  // the windows (p0, q) and (p0 + 1, q)
  float sc[8], sh[8];
  {
    const float* ps = scale + (size_t)g * C + rc * 8;
    const float* ph = shift + (size_t)g * C + rc * 8;
    const float4 sa = *reinterpret_cast<const float4*>(ps), sb = *reinterpret_cast<const float4*>(ps + 4);
    const float4 ha = *reinterpret_cast<const float4*>(ph), hb = *reinterpret_cast<const float4*>(ph + 4);
    sc[0] = sa.x; sc[1] = sa.y; sc[2] = sa.z; sc[3] = sa.w; sc[4] = sb.x; sc[5] = sb.y; sc[6] = sb.z; sc[7] = sb.w;
    sh[0] = ha.x; sh[1] = ha.y; sh[2] = ha.z; sh[3] = ha.w; sh[4] = hb.x; sh[5] = hb.y; sh[6] = hb.z; sh[7] = hb.w;
  }
  // input rows 2 p0 - 1 + r, r = 0..4 (r = 0..2: first window, 2..4: second), columns 2q - 1 + kw; clamped addresses
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  const int h0 = 2 * p0 - 1, w0 = 2 * q - 1;
  uint32_t colc[3], kwpart[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int w = w0 + kw;
    colc[kw] = (uint32_t)(w < 0 ? 0 : w >= W ? W - 1 : w) * cpr;
    kwpart[kw] = (unsigned)w < (unsigned)W ? (uint32_t)(3 - kw) : 0u;
  }
  uint4 v[5][3];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int h = h0 + r;
    const uint32_t rowc = ((n * (uint32_t)H + (uint32_t)(h < 0 ? 0 : h >= H ? H - 1 : h)) * (uint32_t)W) * cpr + rc;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) v[r][kw] = x4[rowc + colc[kw]];
  }
  // one input row -> per channel the best of its three columns: key = (bf16 pattern << 16) + (3 - kw), and the raw input.
  // Two channels at a time: one conversion packs both patterns into a word, and the ReLU is a packed signed 16-bit maximum
  // with 0 on the patterns -- bf16(max(v, 0)) = max_i16(bf16(v), 0) for every v that is not NaN (rounding is symmetric in
  // the sign, a negative pattern and -0 are negative integers), which also leaves no sign bit to drop.
  auto row_best = [&](const uint4 (&rv)[3], uint32_t (&rk)[8], float (&rx)[8]) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      float f[8];
      up8(rv[kw], f);
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        // exactly what bn_apply would have stored: bf16(relu(fma(y, scale, shift)))
        const s16x2_t pat = __builtin_bit_cast(s16x2_t, pack_bf2(fmaf(f[e], sc[e], sh[e]), fmaf(f[e + 1], sc[e + 1], sh[e + 1])));
        const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(pat, s16x2_t{0, 0}));
        const uint32_t key[2] = {(pk << 16) | kwpart[kw], (pk & 0xffff0000u) | kwpart[kw]};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (kw == 0) {
            rk[e + u] = key[u];
            rx[e + u] = f[e + u];
          } else {
            const bool take = key[u] > rk[e + u];
            rk[e + u] = take ? key[u] : rk[e + u];
            rx[e + u] = take ? f[e + u] : rx[e + u];
          }
        }
      }
    }
  };
  // a window's running best <- the better of it and a row's result with the row's part 3 (2 - kh) of the code added
  auto merge = [&](uint32_t (&bk)[8], float (&bx)[8], const uint32_t (&rk)[8], const float (&rx)[8], uint32_t khpart) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t c = rk[e] + khpart;
      const bool take = c > bk[e];
      bk[e] = take ? c : bk[e];
      bx[e] = take ? rx[e] : bx[e];
    }
  };
  auto emit = [&](const uint32_t (&bk)[8], const float (&bx)[8], uint32_t pp) {
    const uint32_t o = ((n * (uint32_t)P + pp) * (uint32_t)Q + (uint32_t)q) * cpr + rc;
    reinterpret_cast<uint4*>(y)[o] =
        make_uint4((bk[0] >> 16) | (bk[1] & 0xffff0000u), (bk[2] >> 16) | (bk[3] & 0xffff0000u),
                   (bk[4] >> 16) | (bk[5] & 0xffff0000u), (bk[6] >> 16) | (bk[7] & 0xffff0000u));
    uint32_t code[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) code[e] = 9u - (bk[e] & 0xfu);
    uint2 pk;
    pk.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
    pk.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
    reinterpret_cast<uint2*>(idx)[o] = pk;
    // the selected INPUT values: with them the backward's per-channel sums run over the pooled tensor
    // only (sum_pixels dz f(x) = sum_windows dy_pooled f(x at argmax), dz being a scatter of dy_pooled)
    if constexpr (XSEL)
      reinterpret_cast<uint4*>(xsel)[o] = make_uint4(pack_bf2(bx[0], bx[1]), pack_bf2(bx[2], bx[3]),
                                                     pack_bf2(bx[4], bx[5]), pack_bf2(bx[6], bx[7]));
  };
  // Row by row: all 15 loads are in flight from the start, and a row's 12 registers are free once it is reduced.
  // Row kh = 0 of the first window adds 6, or 0 when it is outside the image; rows kh = 1 add 3; rows kh = 2 add 0 inside the
  // image and outside.
  uint32_t bk[8], rk[8], sk[8];
  float bx[8], rx[8], sx[8];
  row_best(v[0], bk, bx);
  {
    const uint32_t khpart0 = p0 > 0 ? 6u : 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) bk[e] += khpart0;
  }
  row_best(v[1], rk, rx);
  merge(bk, bx, rk, rx, 3u);
  row_best(v[2], sk, sx);  // the shared row: kh = 2 of the first window, kh = 0 of the second
  merge(bk, bx, sk, sx, 0u);
  emit(bk, bx, (uint32_t)p0);
  if (p0 + 1 < P) {  // (its rows kh = 0 and 1 are inside the image whenever the second window exists)
#pragma unroll
    for (int e = 0; e < 8; ++e) sk[e] += 6u;
    row_best(v[3], rk, rx);
    merge(sk, sx, rk, rx, 3u);
    row_best(v[4], rk, rx);
    merge(sk, sx, rk, rx, 0u);
    emit(sk, sx, (uint32_t)p0 + 1u);
  }
}

__global__ __launch_bounds__(PL_THREADS) void maxpool_bwd(const uint16_t* __restrict__ dy,
                                                          const uint8_t* __restrict__ idx, int N, int H,
                                                          int W, int C, int P, int Q,
                                                          uint16_t* __restrict__ dx) {
  const int cpr = C >> 3;
  const long long total = (long long)N * H * W * cpr;
  for (long long t = (long long)blockIdx.x * PL_THREADS + threadIdx.x; t < total;
       t += (long long)gridDim.x * PL_THREADS) {
    const int c0 = (int)(t % cpr) * 8;
    long long pix = t / cpr;
    const int w = (int)(pix % W);
    pix /= W;
    const int h = (int)(pix % H), n = (int)(pix / H);
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = 0.f;
    // windows p with 2p-1 <= h <= 2p+1
    const int p_lo = h >> 1, p_hi = (h + 1) >> 1, q_lo = w >> 1, q_hi = (w + 1) >> 1;
    for (int p = p_lo; p <= p_hi; ++p) {
      if (p >= P) continue;
      const int kh = h - (2 * p - 1);
      for (int q = q_lo; q <= q_hi; ++q) {
        if (q >= Q) continue;
        const int code = kh * 3 + (w - (2 * q - 1));
        const size_t o = ((size_t)(n * P + p) * Q + q) * C + c0;
        const uint2 pk = *reinterpret_cast<const uint2*>(idx + o);
        float d[8];
        up8(*reinterpret_cast<const uint4*>(dy + o), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int ie = (int)(((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 0xff);
          g[e] += ie == code ? d[e] : 0.f;
        }
      }
    }
    *reinterpret_cast<uint4*>(dx + ((size_t)(n * H + h) * W + w) * C + c0) =
        make_uint4(pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3]), pack_bf2(g[4], g[5]), pack_bf2(g[6], g[7]));
  }
}

// x [N][HW][C] -> y [N][C] (mean over HW).  One thread per (n, 8 channels).
__global__ __launch_bounds__(PL_THREADS) void gap_fwd(const uint16_t* __restrict__ x, int N, int HW, int C,
                                                      uint16_t* __restrict__ y) {
  const int cpr = C >> 3;
  const int t = blockIdx.x * PL_THREADS + threadIdx.x;
  if (t >= N * cpr) return;
  const int n = t / cpr, c0 = (t - n * cpr) * 8;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  for (int i = 0; i < HW; ++i) {
    float f[8];
    up8(*reinterpret_cast<const uint4*>(x + ((size_t)n * HW + i) * C + c0), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += f[e];
  }
  const float inv = 1.0f / (float)HW;
  *reinterpret_cast<uint4*>(y + (size_t)n * C + c0) =
      make_uint4(pack_bf2(s[0] * inv, s[1] * inv), pack_bf2(s[2] * inv, s[3] * inv),
                 pack_bf2(s[4] * inv, s[5] * inv), pack_bf2(s[6] * inv, s[7] * inv));
}

__global__ __launch_bounds__(PL_THREADS) void gap_bwd(const uint16_t* __restrict__ dy, int N, int HW, int C,
                                                      uint16_t* __restrict__ dx) {
  const int cpr = C >> 3;
  const long long total = (long long)N * HW * cpr;
  const float inv = 1.0f / (float)HW;
  for (long long t = (long long)blockIdx.x * PL_THREADS + threadIdx.x; t < total;
       t += (long long)gridDim.x * PL_THREADS) {
    const int c0 = (int)(t % cpr) * 8;
    const long long pix = t / cpr;
    const int n = (int)(pix / HW);
    float d[8];
    up8(*reinterpret_cast<const uint4*>(dy + (size_t)n * C + c0), d);
    *reinterpret_cast<uint4*>(dx + (size_t)pix * C + c0) =
        make_uint4(pack_bf2(d[0] * inv, d[1] * inv), pack_bf2(d[2] * inv, d[3] * inv),
                   pack_bf2(d[4] * inv, d[5] * inv), pack_bf2(d[6] * inv, d[7] * inv));
  }
}

inline int grid_for(long long items) {
  long long b = (items + PL_THREADS - 1) / PL_THREADS;
  if (b > 4096) b = 4096;
  return b < 1 ? 1 : (int)b;
}

}  // namespace

extern "C" int wm_maxpool3x3s2_fwd(const void* x, int N, int H, int W, int C, void* y, void* idx, void* stream) {
  WM_REQUIRE(x && y && idx, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 1 && W > 1 && C > 0, WM_EINVAL);
  WM_REQUIRE(C % 8 == 0, WM_EUNSUPPORTED);
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  maxpool_fwd<<<grid_for((long long)N * P * Q * (C >> 3)), PL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(x), N, H, W, C, P, Q, static_cast<uint16_t*>(y), static_cast<uint8_t*>(idx));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_bn_relu_maxpool3x3s2_fwd(const void* x, const float* scale, const float* shift, int N, int H,
                                           int W, int C, int G, void* y, void* idx, void* xsel, void* stream) {
  WM_REQUIRE(x && scale && shift && y && idx, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 1 && W > 1 && C > 0 && G > 0, WM_EINVAL);
  WM_REQUIRE(C % 8 == 0 && N % G == 0, WM_EUNSUPPORTED);
  WM_REQUIRE((long long)N * H * W * (C / 8) < (1ll << 31), WM_EUNSUPPORTED);  // 32-bit item indices
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  // one thread per pair of vertically adjacent windows x 8 channels, one block per 256 consecutive items (no grid-stride
  // walk: the kernel remaps the block ids so that neighbouring blocks share an L2)
  const int P2 = (P + 1) / 2;
  // (two instantiations: behind a run-time test of xsel hipcc sinks every selection of a raw input to the end of the kernel
  // and keeps all 120 of them in registers until then)
  (xsel ? bn_relu_maxpool_fwd<true> : bn_relu_maxpool_fwd<false>)<<<wm_cdiv((long long)N * P2 * Q * (C >> 3), PL_THREADS), PL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(x), scale, shift, N, H, W, C, P, Q, static_cast<uint16_t*>(y),
      static_cast<uint8_t*>(idx), static_cast<uint16_t*>(xsel), wm_div_make((uint32_t)(C >> 3)), wm_div_make((uint32_t)Q),
      wm_div_make((uint32_t)P2), wm_div_make((uint32_t)(N / G)));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_maxpool3x3s2_bwd(const void* dy, const void* idx, int N, int H, int W, int C, void* dx,
                                   void* stream) {
  WM_REQUIRE(dy && idx && dx, WM_EINVAL);
  WM_REQUIRE(N > 0 && H > 1 && W > 1 && C > 0, WM_EINVAL);
  WM_REQUIRE(C % 8 == 0, WM_EUNSUPPORTED);
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  maxpool_bwd<<<grid_for((long long)N * H * W * (C >> 3)), PL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(dy), static_cast<const uint8_t*>(idx), N, H, W, C, P, Q,
      static_cast<uint16_t*>(dx));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_gap_fwd(const void* x, int N, int HW, int C, void* y, void* stream) {
  WM_REQUIRE(x && y, WM_EINVAL);
  WM_REQUIRE(N > 0 && HW > 0 && C > 0, WM_EINVAL);
  WM_REQUIRE(C % 8 == 0, WM_EUNSUPPORTED);
  gap_fwd<<<wm_cdiv((long long)N * (C >> 3), PL_THREADS), PL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(x), N, HW, C, static_cast<uint16_t*>(y));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_gap_bwd(const void* dy, int N, int HW, int C, void* dx, void* stream) {
  WM_REQUIRE(dy && dx, WM_EINVAL);
  WM_REQUIRE(N > 0 && HW > 0 && C > 0, WM_EINVAL);
  WM_REQUIRE(C % 8 == 0, WM_EUNSUPPORTED);
  gap_bwd<<<grid_for((long long)N * HW * (C >> 3)), PL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(dy), N, HW, C, static_cast<uint16_t*>(dx));
  WM_LAUNCH_CHECK();
  return WM_OK;
}
