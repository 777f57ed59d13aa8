// Label spreading and propagation over a graph (semi_supervised.py: LabelSpreading, LabelPropagation): the iteration
// F <- alpha S F + (1 - alpha) Y, S = D^-1/2 G D^-1/2 (spreading), or F <- D^-1 G F with the labelled rows clamped
// (propagation), for R alpha groups of C class columns at once.  G is a symmetric CSR graph with float32 weights,
// everything else float64.
//   wm_lp_init           F = the one-hot label matrix, repeated per group;
//   wm_lp_iterate        `iters` steps that ping-pong between two F buffers, and per step and group the residual
//                        sum |Fout - Fin|;
//   wm_lp_finalize       one group's row sums, normalised distributions, arg-max labels and the unreached mask;
//   wm_lp_neighbor_mean  the normalised mean of fitted distributions over the neighbour lists of new rows.
// No atomics, no allocation, no synchronisation with the host; the order of every sum depends on the sizes alone, so
// two calls give the same bits.  Floating-point contraction is off in the kernels: every product and every sum below is
// rounded once, as numpy rounds it.
//
// ---- sums and their orders.
//   gather    cols = R C columns; a row is served by W = min(64, max(8, cols rounded up to a power of two)) consecutive
//             lanes, lane l owning the columns l, l + 64, l + 128, l + 192 below cols (one column per lane up to 64).
//             Every lane walks ALL entries p of its row in storage order and adds data[p] * (cs[col[p]] * Fin[col[p]][q])
//             into one double per owned column: the order per (row, column) is the storage order whatever W is.  The W
//             lanes read W consecutive doubles of the neighbour's F row (one 64 .. 512 byte segment); indices, weights
//             and cs are the same address for the whole group.  No cross-lane sum is needed.
//   update    spreading: alpha * (dinv[i] * s) + (1 - alpha) * y, two products and one sum.  Propagation: y itself for a
//             labelled row (its gather is skipped); for an unlabelled one t = (dinv[i] * dinv[i]) * s goes to LDS, every
//             lane adds the C values of its column's group in class order, and Fout = t / that sum (t itself where the
//             sum is 0): sklearn's LabelPropagation renormalises every row at every step, and its n_iter_ and its
//             distributions at a finite tol can only be met by doing the same.
//             Columns of a group with active[g] == 0 are copied; lanes that own only such columns skip the gather.
//   residual  |Fout - Fin| per (row, column) goes to LDS.  Rows are cut into quads 4 j .. 4 j + 3 (a workgroup of 256
//             threads holds 256 / W rows, a whole number of quads).  Per quad and group one thread adds the C classes of
//             a row in class order, and the four row sums as ((r0 + r1) + r2) + r3; rows behind n count as +0.0.  The
//             quad sums are stored with plain stores at part[g][j].  The merge takes one workgroup of 256 threads per
//             group: thread t adds the quads t, t + 256, t + 512, ... in that order, then the 256 values are folded in
//             LDS, s[t] += s[t + h] for h = 128, 64, .. 1.  Nothing of this depends on W or R: a group's residual has
//             the same bits alone as among other groups.  (One thread per result, as csrc/spectral.hip merges its
//             slabs, would be ceil(n / 4) dependent additions per step here; this is ceil(n / 1024) + 8.)
//   finalize  one thread per row; the row sum and the running maximum go over the classes in column order.
//   mean      one thread per (new row, class) adds dist[idx[r][t]][c] for t = 0 .. k - 1 in that order and stores it;
//             a second kernel, one thread per row, adds the stored sums in class order and divides by the total.
#include "common.h"

namespace {

constexpr int LP_MAX_N = 1 << 24;
constexpr int LP_MAX_COLS = 256;     // groups * classes (a lane owns at most LP_MAX_COLS / 64 columns)
constexpr int LP_MAX_K = 64;         // neighbours per new row (manifold.MAX_NEIGHBORS)
constexpr int LP_THREADS = 256;
constexpr int LP_QUAD = 4;           // rows per residual partial

inline int lp_quads(int n) { return (n + LP_QUAD - 1) / LP_QUAD; }
inline bool lp_sizes_ok(int n, int classes, int groups) {
  return n >= 1 && n <= LP_MAX_N && classes >= 1 && groups >= 1 && classes <= LP_MAX_COLS && groups <= LP_MAX_COLS &&
         classes * groups <= LP_MAX_COLS;
}
inline int lp_width(int cols) {
  int w = 8;
  while (w < cols && w < 64) w *= 2;
  return w;
}

__global__ __launch_bounds__(LP_THREADS) void lp_init(const int32_t* __restrict__ labels, int n, int classes, int cols, int ldf,
                                                      double* __restrict__ F) {
  const long long t = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  const int i = (int)(t / cols), q = (int)(t % cols);
  if (i >= n) return;
  F[(size_t)i * ldf + q] = labels[i] == q % classes ? 1.0 : 0.0;
}

// NC: columns per lane (cols <= 64 NC); W lanes per row, W == 64 when NC > 1
template <int NC, bool HARD>
__global__ __launch_bounds__(LP_THREADS) void lp_step(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ data, const double* __restrict__ dinv,
                                                      const int32_t* __restrict__ labels, int n, int classes, int groups, int W,
                                                      const double* __restrict__ alpha, const int32_t* __restrict__ active,
                                                      const double* __restrict__ Fin, double* __restrict__ Fout, int ldf,
                                                      double* __restrict__ part, int quads) {
#pragma clang fp contract(off)
  __shared__ double diff[(LP_THREADS / 64) * LP_MAX_COLS];  // [rows of the workgroup][cols]; rows * cols <= 1024
  const int cols = classes * groups, rows = LP_THREADS / W;
  const int r = threadIdx.x / W, l = threadIdx.x % W;
  const int i = blockIdx.x * rows + r;
  const bool live = i < n;
  const int label = live ? labels[i] : -1;
  bool own[NC], on[NC];
  int grp[NC], cls[NC];
  bool any_on = false;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int q = l + 64 * k;
    own[k] = live && q < cols;
    grp[k] = own[k] ? q / classes : 0;
    cls[k] = own[k] ? q % classes : 0;
    on[k] = own[k] && active[grp[k]] != 0;
    any_on = any_on || on[k];
  }
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  if (any_on && !(HARD && label >= 0)) {
    for (int p = indptr[i], e = indptr[i + 1]; p < e; ++p) {
      const int j = indices[p];
      const double w = (double)data[p];
      const double c = HARD ? 1.0 : dinv[j];
      const double* __restrict__ row = Fin + (size_t)j * ldf + l;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (on[k]) acc[k] += w * (c * row[64 * k]);
    }
  }
  const double di = live ? dinv[i] : 0.0;
  double val[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) val[k] = HARD ? (di * di) * acc[k] : di * acc[k];
  if (HARD) {  // sklearn's LabelPropagation divides every row by its sum at every step (a zero sum divides by 1)
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (l + 64 * k < cols) diff[r * cols + l + 64 * k] = val[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (!on[k]) continue;
      const double* d = diff + r * cols + grp[k] * classes;
      double s = 0.0;
      for (int c = 0; c < classes; ++c) s += d[c];
      val[k] = val[k] / (s == 0.0 ? 1.0 : s);
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int q = l + 64 * k;
    double d = 0.0;
    if (own[k]) {
      const double old = Fin[(size_t)i * ldf + q];
      const double y = label == cls[k] ? 1.0 : 0.0;
      double out;
      if (!on[k]) {
        out = old;
      } else if (HARD) {
        out = label >= 0 ? y : val[k];
      } else {
        const double a = alpha[grp[k]];
        out = a * val[k] + (1.0 - a) * y;
      }
      Fout[(size_t)i * ldf + q] = out;
      d = fabs(out - old);
    }
    if (q < cols) diff[r * cols + q] = d;
  }
  __syncthreads();
  const int t = threadIdx.x, bq = rows / LP_QUAD;  // quads of this workgroup
  if (t < bq * groups) {
    const int jq = t / groups, g = t % groups;
    const int quad = blockIdx.x * bq + jq;
    if (quad < quads) {
      double rs[LP_QUAD];
#pragma unroll
      for (int rr = 0; rr < LP_QUAD; ++rr) {
        const double* d = diff + (jq * LP_QUAD + rr) * cols + g * classes;
        double s = 0.0;
        for (int c = 0; c < classes; ++c) s += d[c];
        rs[rr] = s;
      }
      part[(size_t)g * quads + quad] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
    }
  }
}

__global__ __launch_bounds__(LP_THREADS) void lp_resid_merge(const double* __restrict__ part, int quads, double* __restrict__ resid) {
#pragma clang fp contract(off)
  __shared__ double s[LP_THREADS];
  const int t = threadIdx.x, g = blockIdx.x;
  const double* p = part + (size_t)g * quads;
  double sum = 0.0;
  for (int j = t; j < quads; j += LP_THREADS) sum += p[j];
  // (the tree of f64.h's block_tree_sum without its last barrier, which leaves the result in every thread: with it a step
  // measured 0.2 - 0.4 us outside the run-to-run spread, profiles/f64_refactor.md)
  s[t] = sum;
  __syncthreads();
  for (int h = LP_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  if (t == 0) resid[g] = s[0];
}

__global__ __launch_bounds__(LP_THREADS) void lp_finalize(const double* __restrict__ F, int ldf, int n, int classes,
                                                          double* __restrict__ dist, double* __restrict__ rowsum,
                                                          int32_t* __restrict__ pred, uint8_t* __restrict__ unreached) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= n) return;
  const double* f = F + (size_t)i * ldf;
  double sum = 0.0, best = f[0];
  int arg = 0;
  for (int c = 0; c < classes; ++c) {
    const double x = f[c];
    sum += x;
    if (x > best) {
      best = x;
      arg = c;
    }
  }
  rowsum[i] = sum;
  pred[i] = arg;
  unreached[i] = sum == 0.0 ? 1 : 0;
  double* o = dist + (size_t)i * classes;
  for (int c = 0; c < classes; ++c) o[c] = sum == 0.0 ? 0.0 : f[c] / sum;
}

__global__ __launch_bounds__(LP_THREADS) void lp_neighbor_sum(const int32_t* __restrict__ idx, int m, int k,
                                                              const double* __restrict__ dist, int classes,
                                                              double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  const int r = (int)(t / classes), c = (int)(t % classes);
  if (r >= m) return;
  const int32_t* row = idx + (size_t)r * k;
  double sum = 0.0;
  for (int j = 0; j < k; ++j) sum += dist[(size_t)row[j] * classes + c];
  out[(size_t)r * classes + c] = sum;
}

__global__ __launch_bounds__(LP_THREADS) void lp_row_normalise(double* __restrict__ out, int m, int classes) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * LP_THREADS + threadIdx.x;
  if (r >= m) return;
  double* o = out + (size_t)r * classes;
  double sum = 0.0;
  for (int c = 0; c < classes; ++c) sum += o[c];
  if (sum == 0.0) return;
  for (int c = 0; c < classes; ++c) o[c] = o[c] / sum;
}

template <bool HARD>
void lp_launch_step(int nc, dim3 grid, hipStream_t st, const int32_t* indptr, const int32_t* indices, const float* data,
                    const double* dinv, const int32_t* labels, int n, int classes, int groups, int W, const double* alpha,
                    const int32_t* active, const double* Fin, double* Fout, int ldf, double* part, int quads) {
#define LP_STEP(NC)                                                                                                          \
  lp_step<NC, HARD><<<grid, LP_THREADS, 0, st>>>(indptr, indices, data, dinv, labels, n, classes, groups, W, alpha, active, \
                                                 Fin, Fout, ldf, part, quads)
  switch (nc) {
    case 1: LP_STEP(1); break;
    case 2: LP_STEP(2); break;
    case 3: LP_STEP(3); break;
    default: LP_STEP(4); break;
  }
#undef LP_STEP
}

}  // namespace

extern "C" size_t wm_lp_init_workspace_bytes(int n, int classes, int groups) { return lp_sizes_ok(n, classes, groups) ? WM_TOKEN_WS : 0; }

extern "C" int wm_lp_init(const int32_t* labels, int n, int classes, int groups, double* F, int ldf, void* workspace,
                          size_t workspace_bytes, void* stream) {
  WM_REQUIRE(labels && F && workspace && n > 0 && classes > 0 && groups > 0, WM_EINVAL);
  WM_REQUIRE(lp_sizes_ok(n, classes, groups), WM_EUNSUPPORTED);
  WM_REQUIRE(ldf >= classes * groups, WM_EINVAL);
  WM_REQUIRE(wm_aligned(labels, 3) && wm_aligned(F, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  const int cols = classes * groups;
  const long long cells = (long long)n * cols;
  lp_init<<<(unsigned)((cells + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, static_cast<hipStream_t>(stream)>>>(labels, n, classes,
                                                                                                                  cols, ldf, F);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// workspace: part [groups][quads] doubles, quads = ceil(n / 4)
extern "C" size_t wm_lp_iterate_workspace_bytes(int n, int classes, int groups) {
  return lp_sizes_ok(n, classes, groups) ? (size_t)groups * lp_quads(n) * sizeof(double) : 0;
}

extern "C" int wm_lp_iterate(const int32_t* indptr, const int32_t* indices, const float* data, const double* dinv,
                             const int32_t* labels, int n, int classes, int groups, const double* alpha, const int32_t* active,
                             int hard, int iters, double* Fa, double* Fb, int ldf, double* resid, void* workspace,
                             size_t workspace_bytes, void* stream) {
  WM_REQUIRE(indptr && indices && data && dinv && labels && alpha && active && Fa && Fb && resid && workspace, WM_EINVAL);
  WM_REQUIRE(n > 0 && classes > 0 && groups > 0 && iters >= 1 && Fa != Fb, WM_EINVAL);
  WM_REQUIRE(lp_sizes_ok(n, classes, groups), WM_EUNSUPPORTED);
  WM_REQUIRE(ldf >= classes * groups, WM_EINVAL);
  WM_REQUIRE(wm_aligned(indptr, 3) && wm_aligned(indices, 3) && wm_aligned(data, 3) && wm_aligned(dinv, 7) && wm_aligned(labels, 3) &&
                 wm_aligned(alpha, 7) && wm_aligned(active, 3) && wm_aligned(Fa, 7) && wm_aligned(Fb, 7) && wm_aligned(resid, 7) &&
                 wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_lp_iterate_workspace_bytes(n, classes, groups), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cols = classes * groups, W = lp_width(cols), nc = (cols + 63) / 64, quads = lp_quads(n);
  const dim3 grid(wm_cdiv(n, LP_THREADS / W));
  double* part = static_cast<double*>(workspace);
  for (int step = 0; step < iters; ++step) {
    const double* Fin = step % 2 == 0 ? Fa : Fb;
    double* Fout = step % 2 == 0 ? Fb : Fa;
    if (hard)
      lp_launch_step<true>(nc, grid, st, indptr, indices, data, dinv, labels, n, classes, groups, W, alpha, active, Fin, Fout, ldf,
                           part, quads);
    else
      lp_launch_step<false>(nc, grid, st, indptr, indices, data, dinv, labels, n, classes, groups, W, alpha, active, Fin, Fout, ldf,
                            part, quads);
    WM_LAUNCH_CHECK();
    lp_resid_merge<<<groups, LP_THREADS, 0, st>>>(part, quads, resid + (size_t)step * groups);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}

extern "C" size_t wm_lp_finalize_workspace_bytes(int n, int classes) { return lp_sizes_ok(n, classes, 1) ? WM_TOKEN_WS : 0; }

extern "C" int wm_lp_finalize(const double* F, int ldf, int n, int classes, double* dist, double* rowsum, int32_t* pred,
                              uint8_t* unreached, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(F && dist && rowsum && pred && unreached && workspace && n > 0 && classes > 0, WM_EINVAL);
  WM_REQUIRE(lp_sizes_ok(n, classes, 1), WM_EUNSUPPORTED);
  WM_REQUIRE(ldf >= classes && F != dist, WM_EINVAL);
  WM_REQUIRE(wm_aligned(F, 7) && wm_aligned(dist, 7) && wm_aligned(rowsum, 7) && wm_aligned(pred, 3), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  lp_finalize<<<wm_cdiv(n, LP_THREADS), LP_THREADS, 0, static_cast<hipStream_t>(stream)>>>(F, ldf, n, classes, dist, rowsum, pred,
                                                                                          unreached);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_lp_neighbor_mean_workspace_bytes(int m, int k, int classes) {
  return lp_sizes_ok(m, classes, 1) && k >= 1 && k <= LP_MAX_K ? WM_TOKEN_WS : 0;
}

extern "C" int wm_lp_neighbor_mean(const int32_t* idx, int m, int k, const double* dist, int n, int classes, double* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(idx && dist && out && workspace && m > 0 && k > 0 && n > 0 && classes > 0 && dist != out, WM_EINVAL);
  WM_REQUIRE(wm_lp_neighbor_mean_workspace_bytes(m, k, classes) != 0 && n <= LP_MAX_N, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(idx, 3) && wm_aligned(dist, 7) && wm_aligned(out, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long cells = (long long)m * classes;
  lp_neighbor_sum<<<(unsigned)((cells + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, st>>>(idx, m, k, dist, classes, out);
  WM_LAUNCH_CHECK();
  lp_row_normalise<<<wm_cdiv(m, LP_THREADS), LP_THREADS, 0, st>>>(out, m, classes);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
