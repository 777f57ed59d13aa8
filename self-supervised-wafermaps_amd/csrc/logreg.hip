// Logistic regression on an embedding matrix (linear_model.py; sklearn.linear_model.LogisticRegression with lbfgs): one
// evaluation of the loss and its gradient for `cols` independent columns, in float64 on float32 rows.  The penalty, the
// division by the weight sum and the L-BFGS recursion are host arithmetic on [cols][d + 1] arrays: the kernels never
// see C, so a list of C rides on one pass over the rows.
//   wm_logreg_residual   z = x w^T + b (MFMA), the row-wise softmax / sigmoid, the weighted residuals, the loss
//   wm_logreg_gradient   grad = resid^T [x | 1]: gmm.hip's weighted-sums path (rows_sums.h), nothing of its own here
//
// ---- operands: gmm.hip's.  x float32 [n][ld], true feature count d, a position f >= d is staged as an exact 0.0 and
// never loaded.  w float64 [cols][d + 1], column d the intercept.
//
// ---- lr_residual<T>.  The workgroup tile of f64.h (64 x 64, 4 waves, panels [k][64 + 2] doubles, fragment maps and
// the order of the sum over k stated there); M = 64 rows, N = the columns, K = d in steps of 16 (pca.hip's row passes).
// A workgroup owns 64 rows and ALL T = ceil(cols / 64) column tiles, walked in ascending order as gm_logprob_full walks
// its own (the A panel is fetched again per column tile, from L2).  After a column tile every lane adds the intercept
// to its 2 x 2 x 4 accumulators and stores them into Zs[64][64 T + 1] doubles in LDS: the logits of the workgroup's rows
// stay there until the residuals leave, and never go through memory.  T is a template parameter because Zs is static:
// 33 KB at T = 1 (with the panels: 50 KB, three workgroups per CU), 132 KB at T = 4 (one workgroup per CU: 160 KB of
// LDS).  The odd pitch puts the 64 rows of a column on 32 different bank pairs.
//   epilogue   lane l of wave v owns row l of the tile and the problems v, v + 4, ...: a softmax group (its `classes`
//              consecutive doubles of the row, walked three times: max; sum of exp in class order; p) or a sigmoid
//              column.  The residuals overwrite the logits in Zs.  A problem's 64 row losses sit in the 64 lanes of ONE
//              wave: they are added by the butterfly (partners 32, 16, .. 1 away; both partners add the same two values,
//              so every lane ends with the same bits) and lane 0 stores the tile's sum into part[problem][tile].
//   stores     z_out (before the epilogue) and resid (after it) leave Zs row by row, wave v rows v, v + 4, ..., lane l
//              columns l, l + 64, ...: 64 consecutive doubles per wave instruction.
// lr_loss_total: one workgroup per problem; slab s = (t0 + t1) + (t2 + t3) of its four tiles (a tile behind the last
// counts as an exact 0), thread t adds its run of ceil(slabs / 256) consecutive slabs in order, thread 0 the 256 run
// sums (gm_ordered_total's rule).  Everything depends on n alone: a problem's loss is the same bits in any company.
// A problem's residual columns depend on its own columns of w and on (n, d): the MFMA sum over k is per cell.
// Measured (profiles/logreg.md, 172 950 x 512): 0.403 ms at 9 columns, 0.415 ms at 36, 1.24 - 1.27 x wm_pca_project at
// equal sizes; 28 TF of executed MFMA work, 36 % of the 78.6 TF peak.  Not measured against: a narrower N tile for
// cols <= 16 (9 classes fill 9 of the 64 columns the MFMAs compute), keeping the A panel across column tiles, and the
// T = 2 .. 4 forms at all.
#include "f64.h"
#include "rows_sums.h"

namespace {

constexpr int LR_MAX_N = 1 << 24;
constexpr int LR_MAX_D = 1024;
constexpr int LR_MAX_COLS = 256;
constexpr int LR_KT = 16;
constexpr int LR_SLAB_TILES = 4;  // a slab of 256 rows

inline bool lr_ok(int n, int d, int ld, int cols) {
  return n >= 1 && n <= LR_MAX_N && d >= 1 && d <= LR_MAX_D && ld >= d && ld % 4 == 0 && ld <= LR_MAX_D + 3 && cols >= 1 &&
         cols <= LR_MAX_COLS;
}
inline bool lr_mode_ok(int cols, int mode, int classes) {
  return (mode == 0 || mode == 1) && classes >= 1 && classes <= cols && cols % classes == 0;
}
inline int lr_problems(int cols, int mode, int classes) { return mode == 0 ? cols / classes : cols; }

struct LrArgs {
  const float* x;
  const double* w;
  const int32_t* y32;      // mode 0
  const int8_t* y8;        // mode 1
  const double* sw;
  const double* pos_weight;
  double* resid;
  double* z_out;
  double* part;            // [problems][tiles]
  int n, d, ld, cols, mode, classes, tiles;
  bool fit;                // labels given
};

__device__ __forceinline__ double lr_wave_sum(double v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
  return v;
}

template <int T>
__global__ __launch_bounds__(F64_THREADS) void lr_residual(LrArgs a) {
  constexpr int KT = LR_KT, EL = KT * F64_TILE / F64_THREADS, ZLD = F64_TILE * T + 1;
  __shared__ __attribute__((aligned(16))) double As[KT][F64_LD];
  __shared__ __attribute__((aligned(16))) double Bs[KT][F64_LD];
  __shared__ double Zs[F64_TILE][ZLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, fk = lane >> 4, fc = lane & 15;
  const int m0 = blockIdx.x * F64_TILE;
  const int W = a.d + 1;
  // both operands have the features contiguous: a thread stages feature t % 16 of tile entries t / 16 + 16 u
  const int sf = t % KT, se = t / KT;
  for (int tn = 0; tn < T; ++tn) {
    const int n0 = tn * F64_TILE;
    if (n0 >= a.cols) break;
    double ra[EL], rb[EL];
    auto fetch = [&](int kb) {
      const int f = kb + sf;
#pragma unroll
      for (int u = 0; u < EL; ++u) {
        const int row = m0 + se + (F64_THREADS / KT) * u, col = n0 + se + (F64_THREADS / KT) * u;
        ra[u] = f < a.d && row < a.n ? (double)a.x[(size_t)row * a.ld + f] : 0.0;
        rb[u] = f < a.d && col < a.cols ? a.w[(size_t)col * W + f] : 0.0;
      }
    };
    f64x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int kb = 0; kb < a.d; kb += KT) {
      __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
      for (int u = 0; u < EL; ++u) {
        As[sf][se + (F64_THREADS / KT) * u] = ra[u];
        Bs[sf][se + (F64_THREADS / KT) * u] = rb[u];
      }
      __syncthreads();
      if (kb + KT < a.d) fetch(kb + KT);
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 32 + j * 16 + fc;  // (< 64 T: inside Zs; a column behind cols holds a zero nobody reads)
      const double b = col < a.cols ? a.w[(size_t)col * W + a.d] : 0.0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) Zs[wm * 32 + i * 16 + fk + 4 * r][col] = acc[i][j][r] + b;
    }
  }
  __syncthreads();
  const int live_rows = min(F64_TILE, a.n - m0);
  if (a.z_out) {
    for (int r = wave; r < live_rows; r += 4)
      for (int c = lane; c < a.cols; c += 64) a.z_out[(size_t)(m0 + r) * a.cols + c] = Zs[r][c];
    __syncthreads();
  }
  // ---- the epilogue: lane = row of the tile, wave = problems wave, wave + 4, ...
  const int row = m0 + lane;
  const bool in = row < a.n;
  const double s = in && a.fit ? (a.sw ? a.sw[row] : 1.0) : 0.0;
  double* zr = Zs[lane];
  if (a.mode == 0) {
    const int K = a.classes, G = a.cols / K;
    const int yi = in && a.fit ? a.y32[row] : -1;
    for (int g = wave; g < G; g += 4) {
      double* __restrict__ z = zr + g * K;
      double m = z[0];
      for (int c = 1; c < K; ++c) m = fmax(m, z[c]);
      double sum = 0.0;
      for (int c = 0; c < K; ++c) sum += exp(z[c] - m);
      const double lse = m + log(sum);
      double li = 0.0;
      if (!a.fit) {
        for (int c = 0; c < K; ++c) z[c] = exp(z[c] - lse);
      } else if (yi < 0 || yi >= K) {  // unlabelled (and a label outside the contract): weight 0
        for (int c = 0; c < K; ++c) z[c] = 0.0;
      } else {
        li = s * (lse - z[yi]);
        for (int c = 0; c < K; ++c) z[c] = s * (exp(z[c] - lse) - (c == yi ? 1.0 : 0.0));
      }
      if (a.fit) {
        const double tot = lr_wave_sum(li);
        if (lane == 0) a.part[(size_t)g * a.tiles + blockIdx.x] = tot;
      }
    }
  } else {
    const int L = a.classes;
    for (int q = wave; q < a.cols; q += 4) {
      const int l = q % L;
      const double z = zr[q];
      const double e = exp(-fabs(z));          // in (0, 1]: never an exp of a positive argument
      const double inv = 1.0 / (1.0 + e);
      const double sig_pos = z >= 0.0 ? inv : e * inv;   // sigma(z)
      const double sig_neg = z >= 0.0 ? e * inv : inv;   // sigma(-z)
      double li = 0.0;
      if (!a.fit) {
        zr[q] = sig_pos;
      } else {
        const bool pos = in && a.y8[(size_t)row * L + l] != 0;
        const double lp = log1p(e);
        if (pos) {
          const double aw = a.pos_weight ? a.pos_weight[l] : 1.0;
          li = s * (aw * (fmax(-z, 0.0) + lp));
          zr[q] = -(s * (aw * sig_neg));
        } else {
          li = s * (fmax(z, 0.0) + lp);
          zr[q] = s * sig_pos;
        }
        const double tot = lr_wave_sum(li);
        if (lane == 0) a.part[(size_t)q * a.tiles + blockIdx.x] = tot;
      }
    }
  }
  __syncthreads();
  for (int r = wave; r < live_rows; r += 4)
    for (int c = lane; c < a.cols; c += 64) a.resid[(size_t)(m0 + r) * a.cols + c] = Zs[r][c];
}

__global__ __launch_bounds__(F64_THREADS) void lr_loss_total(const double* __restrict__ part, int tiles, double* __restrict__ loss) {
  __shared__ double sh[F64_THREADS];
  const int t = threadIdx.x;
  const double* __restrict__ p = part + (size_t)blockIdx.x * tiles;
  const int slabs = (tiles + LR_SLAB_TILES - 1) / LR_SLAB_TILES;
  const int run = (slabs + F64_THREADS - 1) / F64_THREADS;
  const int b0 = min(slabs, t * run), b1 = min(slabs, b0 + run);
  double mine = 0.0;
  for (int b = b0; b < b1; ++b) {
    double v[LR_SLAB_TILES];
#pragma unroll
    for (int q = 0; q < LR_SLAB_TILES; ++q) v[q] = 4 * b + q < tiles ? p[4 * b + q] : 0.0;
    mine += (v[0] + v[1]) + (v[2] + v[3]);
  }
  sh[t] = mine;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int q = 0; q < F64_THREADS; ++q) tot += sh[q];
    loss[blockIdx.x] = tot;
  }
}

}  // namespace

extern "C" size_t wm_logreg_residual_workspace_bytes(int n, int d, int ld, int cols, int mode, int classes) {
  if (!lr_ok(n, d, ld, cols) || !lr_mode_ok(cols, mode, classes)) return 0;
  const size_t tiles = (size_t)(n + F64_TILE - 1) / F64_TILE;
  const size_t bytes = (size_t)lr_problems(cols, mode, classes) * tiles * sizeof(double);
  return bytes < WM_TOKEN_WS ? WM_TOKEN_WS : bytes;
}

extern "C" int wm_logreg_residual(const float* x, int n, int d, int ld, const double* w, int cols, int mode, int classes,
                                  const void* y, const double* sw, const double* pos_weight, double* resid, double* loss,
                                  double* z_out, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && w && resid && workspace && n > 0 && d > 0 && cols > 0 && ld >= d && (!y || loss), WM_EINVAL);
  WM_REQUIRE((mode == 0 || mode == 1) && classes >= 1 && classes <= cols && cols % classes == 0, WM_EINVAL);
  WM_REQUIRE(lr_ok(n, d, ld, cols), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(w, 7) && wm_aligned(y, mode == 0 ? 3 : 0) && wm_aligned(sw, 7) &&
                 wm_aligned(pos_weight, 7) && wm_aligned(resid, 7) && wm_aligned(loss, 7) && wm_aligned(z_out, 7) &&
                 wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_logreg_residual_workspace_bytes(n, d, ld, cols, mode, classes), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = (n + F64_TILE - 1) / F64_TILE;
  LrArgs a{x, w, mode == 0 ? static_cast<const int32_t*>(y) : nullptr, mode == 1 ? static_cast<const int8_t*>(y) : nullptr,
           sw, pos_weight, resid, z_out, static_cast<double*>(workspace), n, d, ld, cols, mode, classes, tiles, y != nullptr};
  switch ((cols + F64_TILE - 1) / F64_TILE) {
    case 1: lr_residual<1><<<tiles, F64_THREADS, 0, st>>>(a); break;
    case 2: lr_residual<2><<<tiles, F64_THREADS, 0, st>>>(a); break;
    case 3: lr_residual<3><<<tiles, F64_THREADS, 0, st>>>(a); break;
    default: lr_residual<4><<<tiles, F64_THREADS, 0, st>>>(a); break;
  }
  WM_LAUNCH_CHECK();
  if (y) {
    lr_loss_total<<<lr_problems(cols, mode, classes), F64_THREADS, 0, st>>>(a.part, tiles, loss);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}

extern "C" size_t wm_logreg_gradient_workspace_bytes(int n, int d, int ld, int cols) {
  return lr_ok(n, d, ld, cols) ? wm_rows_sums_workspace_bytes(n, d, ld, cols) : 0;
}

extern "C" int wm_logreg_gradient(const float* x, int n, int d, int ld, const double* resid, int cols, double* grad,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && resid && grad && workspace && n > 0 && d > 0 && cols > 0 && ld >= d, WM_EINVAL);
  WM_REQUIRE(lr_ok(n, d, ld, cols), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(x, 15) && wm_aligned(resid, 7) && wm_aligned(grad, 7) && wm_aligned(workspace, 15), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_logreg_gradient_workspace_bytes(n, d, ld, cols), WM_EWORKSPACE);
  return wm_rows_sums_launch(x, n, d, ld, resid, cols, grad + d, d + 1, grad, d + 1, workspace, static_cast<hipStream_t>(stream));
}
