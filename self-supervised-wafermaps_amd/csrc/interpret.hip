// Model-inspection kernels: the attention maps and the EigenCAM of the reference's report figures
// (notebooks/2.0-Figures-DINO-attention.ipynb: dino's get_last_selfattention + visualize_attention.py's --threshold mask;
// notebooks/2.0-Figures-GradCAM.ipynb: pytorch_grad_cam.EigenCAM on backbone.layer4[-1]).  Inference only, no atomics:
// two calls give the same bits.
//
// attention probabilities: softmax(scale q k^T) per (image, head), written out as float32 rows -- what the streaming
//   forward kernel (attention.hip) normalises and never stores.  bf16 qkv: one block per (image, head), K of the head in
//   LDS, 16-query strips per wave on v_mfma_f32_16x16x32_bf16 with the forward kernel's operand order, so the scores are
//   the ones it normalises; row max and row sum in f32.  float32 qkv (the parity preset): one wave per query row, a lane
//   per key, fmaf chains over the head dimension as f32path.hip's attention.  Either way a row's values do not depend on
//   which other rows are computed, so the class-token-only mode (R = 1) gives row 0 of the full mode bit for bit.
//   Bound by its writes: B H R S 4 bytes.
//
// mass mask (visualize_attention.py --threshold): entry i of a row is kept when the share of the row's mass held by the
//   entries that a stable ascending sort puts at or before it exceeds 1 - t.  No sort: every entry compares itself with
//   the whole row (<= 256 values in LDS) and sums the smaller ones (ties broken by index) in double.
//
// EigenCAM (pytorch_grad_cam get_2d_projection + BaseCAM + scale_cam_image), one block per image: centred activations
//   A [HW][C] (NaN -> 0) staged in channel chunks, Gram matrix G = A A^T [HW][HW] in double, cyclic Jacobi in double
//   (round-robin ordering: HW/2 disjoint rotations per step) for its leading eigenpair (lambda, u): the projection
//   A v1 = sqrt(lambda) u.  Jacobi converges whatever the eigengap.  The sign is fixed so that the projection correlates
//   non-negatively with the per-position channel sums of the UNCENTRED activations (LAPACK's sign is arbitrary); then
//   ReLU, min-max, bilinear resize (half-pixel centres, edges clamped) and min-max again.
#include "attn_frag.h"
#include "common.h"

namespace {

// ------------------------------------------------------------------------------- attention probabilities
constexpr int AP_THREADS = 512;   // full mode: 8 waves share the query strips of one (image, head)

template <int NT, int HD>
__global__ __launch_bounds__(AP_THREADS) void attn_probs_bf16(const uint16_t* __restrict__ qkv, int S, int H, int R,
                                                              float scale, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ap_smem[];
  constexpr int SP = NT * 16, KS = HD / 32;
  uint8_t* sk = ap_smem;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const size_t rs = (size_t)3 * H * HD;
  const uint16_t* base = qkv + (size_t)b * S * rs + h * HD;
  stage_rows<HD>(base + (size_t)H * HD, rs, S, SP, sk);
  __syncthreads();
  const bool vec = (S & 3) == 0;   // a lane's 4 keys are consecutive: one 16-byte store when rows start 16-byte aligned
  for (int qs = wave; qs * 16 < R; qs += (int)(blockDim.x >> 6)) {
    const int q = qs * 16 + fr;
    bf16x8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_global(base, rs, q, S, ks, fg);
    f32x4_t sc[NT];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<HD>(sk, t * 16 + fr, ks, fg), qf[ks], a, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = t * 16 + 4 * fg + e;
        a[e] = key < S ? a[e] * scale : -INFINITY;
        m = fmaxf(m, a[e]);
      }
      sc[t] = a;
    }
    m = wm_xor32_max(wm_xor16_max(m));
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[t][e] = expf(sc[t][e] - m);
        l += sc[t][e];
      }
    l = wm_xor32_sum(wm_xor16_sum(l));
    if (q < R) {
      const float inv = 1.f / l;
      float* dst = out + ((size_t)blockIdx.x * R + q) * S;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int key0 = t * 16 + 4 * fg;
        if (key0 >= S) continue;
        if (vec) {
          *reinterpret_cast<float4*>(dst + key0) =
              make_float4(sc[t][0] * inv, sc[t][1] * inv, sc[t][2] * inv, sc[t][3] * inv);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (key0 + e < S) dst[key0 + e] = sc[t][e] * inv;
        }
      }
    }
  }
}

template <int NT, int HD>
int launch_probs_bf16(const void* qkv, int B, int S, int H, int R, float scale, float* out, hipStream_t st) {
  constexpr int lds = NT * 16 * AT_ROWB;   // <= 36 KiB
  const int threads = R == 1 ? 64 : AP_THREADS;
  attn_probs_bf16<NT, HD><<<B * H, threads, lds, st>>>(static_cast<const uint16_t*>(qkv), S, H, R, scale, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

template <int HD>
int dispatch_probs_bf16(const void* qkv, int B, int S, int H, int R, float scale, float* out, hipStream_t st) {
  // the forward kernel's tile counts (attention.hip dispatch_fwd)
  if (S <= 32) return launch_probs_bf16<2, HD>(qkv, B, S, H, R, scale, out, st);
  if (S <= 64) return launch_probs_bf16<4, HD>(qkv, B, S, H, R, scale, out, st);
  if (S <= 128) return launch_probs_bf16<8, HD>(qkv, B, S, H, R, scale, out, st);
  if (S <= 224) return launch_probs_bf16<14, HD>(qkv, B, S, H, R, scale, out, st);
  return launch_probs_bf16<16, HD>(qkv, B, S, H, R, scale, out, st);
}

constexpr int APF_THREADS = 256;
constexpr int APF_KPL = 4;   // keys per lane: S <= 256

// K of the head in LDS as [S][HD + 1] floats (odd row pitch: the 64 lanes' rows land on distinct banks)
template <int HD>
__global__ __launch_bounds__(APF_THREADS) void attn_probs_f32(const float* __restrict__ qkv, int S, int H, int R,
                                                             float scale, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float apf_smem[];
  constexpr int KP = HD + 1;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t rs = (size_t)3 * H * HD;
  const float* base = qkv + (size_t)b * S * rs + (size_t)h * HD;
  for (int i = threadIdx.x; i < S * HD; i += APF_THREADS) {
    const int j = i / HD, d = i - j * HD;
    apf_smem[j * KP + d] = base[(size_t)j * rs + (size_t)H * HD + d];
  }
  __syncthreads();
  for (int q = wave; q < R; q += APF_THREADS / 64) {
    float qv[HD];
    const float* qp = base + (size_t)q * rs;
#pragma unroll
    for (int d = 0; d < HD; ++d) qv[d] = qp[d];
    float s[APF_KPL];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < APF_KPL; ++t) {
      const int j = t * 64 + lane;
      float a = 0.f;
      if (j < S) {
#pragma unroll
        for (int d = 0; d < HD; ++d) a = fmaf(qv[d], apf_smem[j * KP + d], a);
        a *= scale;
      } else {
        a = -INFINITY;
      }
      s[t] = a;
      m = fmaxf(m, a);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < APF_KPL; ++t) {
      s[t] = expf(s[t] - m);
      l += s[t];
    }
    l = wave_sum(l);
    const float inv = 1.f / l;
    float* dst = out + ((size_t)blockIdx.x * R + q) * S;
#pragma unroll
    for (int t = 0; t < APF_KPL; ++t)
      if (t * 64 + lane < S) dst[t * 64 + lane] = s[t] * inv;
  }
}

template <int HD>
int launch_probs_f32(const void* qkv, int B, int S, int H, int R, float scale, float* out, hipStream_t st) {
  const int lds = S * (HD + 1) * (int)sizeof(float);   // <= 65 KiB
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_probs_f32<HD>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (HD + 1) * (int)sizeof(float));
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  attn_probs_f32<HD><<<B * H, APF_THREADS, lds, st>>>(static_cast<const float*>(qkv), S, H, R, scale, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// ------------------------------------------------------------------------------- mass mask
constexpr int MM_MAX = 256;

__global__ __launch_bounds__(MM_MAX) void mass_mask(const float* __restrict__ a, int n, long long ld, double limit,
                                                    uint8_t* __restrict__ keep) {
  __shared__ float v[MM_MAX];
  const long long row = blockIdx.x;
  const int i = threadIdx.x;
  v[i] = i < n ? a[row * ld + i] : 0.f;
  __syncthreads();
  if (i >= n) return;
  const float ai = v[i];
  double below = 0.0, total = 0.0;   // every thread sums the row in the same order: one total for all of them
  for (int j = 0; j < n; ++j) {
    const float aj = v[j];
    total += (double)aj;
    if (aj < ai || (aj == ai && j <= i)) below += (double)aj;
  }
  keep[row * n + i] = below / total > limit ? 1 : 0;
}

// ------------------------------------------------------------------------------- EigenCAM
constexpr int EC_THREADS = 256;
constexpr int EC_MAXHW = 64;
constexpr int EC_LD = EC_MAXHW + 1;      // row pitch (doubles) of G and V
constexpr int EC_CH = 32;                // channels per staged chunk
constexpr int EC_ACC = EC_MAXHW * EC_MAXHW / EC_THREADS;
constexpr int EC_MAX_SWEEPS = 40;
constexpr double EC_TOL = 1e-26;         // stop when sum(offdiag^2) <= EC_TOL sum(all^2): off-norm ~1e-13 relative
constexpr int EC_LDS = (2 * EC_MAXHW * EC_LD + EC_THREADS + 4 * (EC_MAXHW / 2) + 3 * EC_MAXHW) * 8 + 2 * EC_MAXHW * 4;

__device__ __forceinline__ double ec_load(const void* x, int dtype, size_t i) {
  const float v = dtype == WM_BF16 ? bf2f(static_cast<const uint16_t*>(x)[i]) : static_cast<const float*>(x)[i];
  return v != v ? 0.0 : (double)v;   // NaN -> 0
}

// deterministic block reductions through red[EC_THREADS]; every thread returns the result
__device__ double ec_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = EC_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ void ec_minmax(double lo, double hi, double* red, double& mn, double& mx) {
  red[threadIdx.x] = lo;
  __syncthreads();
  for (int o = EC_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  mn = red[0];
  __syncthreads();
  red[threadIdx.x] = hi;
  __syncthreads();
  for (int o = EC_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
}

// bilinear sample of the HxW map at output pixel (oy, ox) of an OHxOW grid: F.interpolate(mode="bilinear",
// align_corners=False) -- source = (dst + 0.5) in / out - 0.5, clamped at 0; the far neighbour clamped at the edge
__device__ __forceinline__ double ec_bilinear(const double* m, int H, int W, int OH, int OW, int oy, int ox) {
  const double sy = fmax(((double)oy + 0.5) * ((double)H / (double)OH) - 0.5, 0.0);
  const double sx = fmax(((double)ox + 0.5) * ((double)W / (double)OW) - 0.5, 0.0);
  const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const double ly = sy - y0, lx = sx - x0;
  return (1.0 - ly) * ((1.0 - lx) * m[y0 * W + x0] + lx * m[y0 * W + x1]) +
         ly * ((1.0 - lx) * m[y1 * W + x0] + lx * m[y1 * W + x1]);
}

__global__ __launch_bounds__(EC_THREADS) void eigencam_kernel(const void* __restrict__ act, int dtype, int C, int H, int W,
                                                              int OH, int OW, float* __restrict__ cam) {
  extern __shared__ __attribute__((aligned(16))) double ec_smem[];
  double* G = ec_smem;                       // [n][EC_LD]
  double* V = G + EC_MAXHW * EC_LD;          // [n][EC_LD]; during the Gram pass: the chunk A [HW][EC_CH]
  double* red = V + EC_MAXHW * EC_LD;        // [EC_THREADS]
  double* pc = red + EC_THREADS;             // rotation cosines [n / 2]
  double* ps = pc + EC_MAXHW / 2;            // sines
  double* cmean = ps + EC_MAXHW / 2;         // chunk channel means [EC_CH] (EC_CH <= EC_MAXHW)
  double* rsum = cmean + EC_MAXHW;           // uncentred channel sums per position [HW]
  double* prj = rsum + EC_MAXHW;             // projection / map [HW]
  int* pa = reinterpret_cast<int*>(prj + EC_MAXHW);   // rotation pairs [n / 2]
  int* pb = pa + EC_MAXHW;
  __shared__ double s_scalar[2];
  const int tid = threadIdx.x;
  const int HW = H * W;
  const int n = HW + (HW & 1);               // even order for the round-robin pairing; the pad index stays zero
  const size_t img = blockIdx.x;
  double* A = V;

  // ---- Gram matrix of the centred activations
  double acc[EC_ACC];
#pragma unroll
  for (int k = 0; k < EC_ACC; ++k) acc[k] = 0.0;
  double rown = 0.0;   // thread i < HW: channel sum of position i (uncentred)
  for (int c0 = 0; c0 < C; c0 += EC_CH) {
    for (int e = tid; e < HW * EC_CH; e += EC_THREADS) {
      const int i = e / EC_CH, cc = e - i * EC_CH;
      A[e] = c0 + cc < C ? ec_load(act, dtype, (img * HW + i) * (size_t)C + c0 + cc) : 0.0;
    }
    __syncthreads();
    if (tid < EC_CH) {
      double s = 0.0;
      for (int i = 0; i < HW; ++i) s += A[i * EC_CH + tid];
      cmean[tid] = s / (double)HW;
    } else if (tid >= 64 && tid - 64 < HW) {
      const int i = tid - 64;
      for (int cc = 0; cc < EC_CH; ++cc) rown += A[i * EC_CH + cc];
    }
    __syncthreads();
    for (int e = tid; e < HW * EC_CH; e += EC_THREADS) {
      const int cc = e % EC_CH;
      A[e] = c0 + cc < C ? A[e] - cmean[cc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EC_ACC; ++k) {
      const int e = tid + k * EC_THREADS;
      if (e < HW * HW) {
        const int i = e / HW, j = e - i * HW;
        const double* ai = A + i * EC_CH;
        const double* aj = A + j * EC_CH;
        double g = acc[k];
        for (int cc = 0; cc < EC_CH; ++cc) g = fma(ai[cc], aj[cc], g);
        acc[k] = g;
      }
    }
    __syncthreads();
  }
  if (tid >= 64 && tid - 64 < HW) rsum[tid - 64] = rown;
  for (int e = tid; e < n * n; e += EC_THREADS) {
    const int i = e / n, j = e - i * n;
    G[i * EC_LD + j] = 0.0;
    V[i * EC_LD + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EC_ACC; ++k) {
    const int e = tid + k * EC_THREADS;
    if (e < HW * HW) G[(e / HW) * EC_LD + e % HW] = acc[k];
  }
  __syncthreads();

  // ---- cyclic Jacobi, round-robin ordering (position 0 fixed, the others rotate)
  const int half = n / 2;
  for (int sweep = 0; sweep < EC_MAX_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int e = tid; e < n * n; e += EC_THREADS) {
      const int i = e / n, j = e - i * n;
      const double g = G[i * EC_LD + j];
      all += g * g;
      if (i != j) off += g * g;
    }
    off = ec_sum(off, red);
    all = ec_sum(all, red);
    if (off <= EC_TOL * all) break;   // (also the all-zero matrix)
    for (int r = 0; r < n - 1; ++r) {
      if (tid < half) {
        const int p0 = tid, p1 = n - 1 - tid;
        const int a = p0 == 0 ? 0 : 1 + (p0 - 1 + r) % (n - 1);
        const int b = 1 + (p1 - 1 + r) % (n - 1);
        const double gab = G[a * EC_LD + b];
        double c = 1.0, s = 0.0;
        if (gab != 0.0) {
          const double tau = (G[b * EC_LD + b] - G[a * EC_LD + a]) / (2.0 * gab);
          const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
        }
        pa[tid] = a;
        pb[tid] = b;
        pc[tid] = c;
        ps[tid] = s;
      }
      __syncthreads();
      for (int w = tid; w < half * n; w += EC_THREADS) {   // rows a, b of G <- J^T G
        const int p = w / n, k = w - p * n;
        const double c = pc[p], s = ps[p];
        double* ra = G + pa[p] * EC_LD;
        double* rb = G + pb[p] * EC_LD;
        const double x = ra[k], y = rb[k];
        ra[k] = c * x - s * y;
        rb[k] = s * x + c * y;
      }
      __syncthreads();
      for (int w = tid; w < half * n; w += EC_THREADS) {   // columns a, b of G and V <- (.) J
        const int p = w / n, k = w - p * n;
        const double c = pc[p], s = ps[p];
        const int a = pa[p], b = pb[p];
        double x = G[k * EC_LD + a], y = G[k * EC_LD + b];
        G[k * EC_LD + a] = c * x - s * y;
        G[k * EC_LD + b] = s * x + c * y;
        x = V[k * EC_LD + a];
        y = V[k * EC_LD + b];
        V[k * EC_LD + a] = c * x - s * y;
        V[k * EC_LD + b] = s * x + c * y;
      }
      __syncthreads();
    }
  }

  // ---- leading eigenpair -> signed projection -> ReLU -> min-max
  if (tid == 0) {
    int kmax = 0;
    for (int i = 1; i < HW; ++i)
      if (G[i * EC_LD + i] > G[kmax * EC_LD + kmax]) kmax = i;
    const double lam = G[kmax * EC_LD + kmax];
    double ok = 0.0;
    if (lam > 0.0) {
      const double sl = sqrt(lam);
      double dot = 0.0;
      for (int i = 0; i < HW; ++i) {
        prj[i] = sl * V[i * EC_LD + kmax];
        dot += prj[i] * rsum[i];
      }
      const double sg = dot < 0.0 ? -1.0 : 1.0;
      double mn = INFINITY, mx;
      for (int i = 0; i < HW; ++i) {
        prj[i] = fmax(sg * prj[i], 0.0);
        mn = fmin(mn, prj[i]);
      }
      mx = -INFINITY;
      for (int i = 0; i < HW; ++i) {
        prj[i] -= mn;
        mx = fmax(mx, prj[i]);
      }
      for (int i = 0; i < HW; ++i) prj[i] /= 1e-7 + mx;
      ok = 1.0;
    }
    s_scalar[0] = ok;
  }
  __syncthreads();
  float* dst = cam + img * (size_t)OH * OW;
  const int npix = OH * OW;
  if (s_scalar[0] == 0.0) {   // lambda_1 = 0: no variation to project
    for (int o = tid; o < npix; o += EC_THREADS) dst[o] = 0.f;
    return;
  }
  // ---- resize, then min-max again (BaseCAM.aggregate_multi_layers)
  double lo = INFINITY, hi = -INFINITY;
  for (int o = tid; o < npix; o += EC_THREADS) {
    const double v = ec_bilinear(prj, H, W, OH, OW, o / OW, o % OW);
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  double mn, mx;
  ec_minmax(lo, hi, red, mn, mx);
  const double inv = 1.0 / (1e-7 + (mx - mn));
  for (int o = tid; o < npix; o += EC_THREADS)
    dst[o] = (float)((ec_bilinear(prj, H, W, OH, OW, o / OW, o % OW) - mn) * inv);
}

}  // namespace

extern "C" int wm_attention_probs(const void* qkv, int dtype, int B, int S, int H, int head_dim, float scale,
                                  int cls_only, float* probs, void* stream) {
  WM_REQUIRE(B > 0 && S > 0 && H > 0 && (long long)B * H < (1ll << 31), WM_EINVAL);
  WM_REQUIRE(S <= 256 && (head_dim == 64 || head_dim == 32), WM_EUNSUPPORTED);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  WM_REQUIRE(qkv && probs, WM_EINVAL);
  WM_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(probs) & 15) == 0, WM_EALIGN);
  const int R = cls_only ? 1 : S;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == WM_BF16) {
    if (head_dim == 64) return dispatch_probs_bf16<64>(qkv, B, S, H, R, scale, probs, st);
    return dispatch_probs_bf16<32>(qkv, B, S, H, R, scale, probs, st);
  }
  if (head_dim == 64) return launch_probs_f32<64>(qkv, B, S, H, R, scale, probs, st);
  return launch_probs_f32<32>(qkv, B, S, H, R, scale, probs, st);
}

extern "C" int wm_attention_mass_mask(const float* attn, long long rows, int n, long long ld, double threshold,
                                      uint8_t* keep, void* stream) {
  WM_REQUIRE(rows > 0 && rows < (1ll << 31) && n > 0 && ld >= n, WM_EINVAL);
  WM_REQUIRE(threshold >= 0.0 && threshold <= 1.0, WM_EINVAL);   // (NaN fails both)
  WM_REQUIRE(n <= MM_MAX, WM_EUNSUPPORTED);
  WM_REQUIRE(attn && keep, WM_EINVAL);
  mass_mask<<<(int)rows, MM_MAX, 0, static_cast<hipStream_t>(stream)>>>(attn, n, ld, 1.0 - threshold, keep);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_eigencam(const void* act, int dtype, int N, int C, int H, int W, int out_h, int out_w, float* cam,
                           void* stream) {
  WM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, WM_EINVAL);
  WM_REQUIRE(H * W <= EC_MAXHW && out_h <= 4096 && out_w <= 4096, WM_EUNSUPPORTED);
  WM_REQUIRE((long long)N * H * W * C < (1ll << 40), WM_EUNSUPPORTED);
  WM_REQUIRE(dtype == WM_F32 || dtype == WM_BF16, WM_EUNSUPPORTED);
  WM_REQUIRE(act && cam, WM_EINVAL);
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eigencam_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, EC_LDS);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  eigencam_kernel<<<N, EC_THREADS, EC_LDS, static_cast<hipStream_t>(stream)>>>(act, dtype, C, H, W, out_h, out_w, cam);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
