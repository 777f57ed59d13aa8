// UMAP on the exact kNN graph (manifold.py; reference notebooks 3.0-Embeddings-inference, 3.1-Embeddings-clustering,
// 3.2-Embeddings-SSL-categories and the 2.0 figure notebooks: umap.UMAP(...).fit_transform(data)):
//   wm_umap_smooth_knn   per row of the kNN graph (csrc/cluster.hip: wm_knn_graph) the fuzzy-simplicial-set parameters
//                        rho, sigma and the membership weights;
//   wm_umap_layout       the layout optimisation, the hot path: one launch per epoch over every graph entry.
// The symmetrisation between the two (G = P + P^T - P o P^T as CSR) is a one-off index build in torch (manifold.py).
//
// ---- smooth kNN (umap-learn's smooth_knn_dist + compute_membership_strengths, local_connectivity = 1)
// Row i holds its k distances d_0 <= ... <= d_{k-1} (float32, the row itself among them) and their indices.
//   rho_i   = the first positive d_j (0 when all are 0);
//   sigma_i : bisection on S(s) = sum_{j >= 1} (d_j - rho > 0 ? exp(-(d_j - rho) / s) : 1) towards log2(k): start at
//             s = 1, lo = 0, hi = inf; at most 64 steps; stop once |S - log2 k| < 1e-5; S > target: hi = s,
//             s = (lo + hi) / 2; else lo = s and s = 2 s while hi = inf, (lo + hi) / 2 after;
//             then s >= 1e-3 * mean_j d_j of the row (rho > 0) or 1e-3 * the mean of all n k distances (rho = 0);
//   w_ij    = 0 where the neighbour is i itself, 1 where d_j - rho <= 0, else exp(-(d_j - rho) / sigma_i).
// One thread per row, in double (it runs once per fit); rho is the float32 distance itself, sigma is rounded to
// float32 and the weights are computed from that rounded value, so (rho, sigma) as returned reproduce them.
//
// ---- layout (umap-learn's optimize_layout_euclidean restated as a deterministic gather)
// umap-learn runs a racy loop: every sampled edge moves both its ends in place.  Here positions are double-buffered:
// every gradient of epoch ep reads the positions from before that epoch, every vertex has one writer, there are no
// atomics, and two runs give the same bits.  G is symmetric and the two directions of an edge share a schedule, so
// "move the head, move the tail" becomes twice the attraction at the head.  For vertex i at epoch ep, over its CSR
// entries e = (i -> j), e the entry's position in `indices`, with a, b, gamma = repulsion_strength, R = neg_rate:
//   sampled(e, ep) = ((ep + 1) q_e >> 16) > (ep q_e >> 16)                       (64-bit products)
//       q_e = rint(65536 w_e / max w) as uint32, computed by the caller in double: an entry is sampled exactly
//       (E q_e) >> 16 times in E epochs, and one with q_e < 65536 / n_epochs never, so nothing is dropped physically;
//   att(i, j) = clip(-2ab r^(b-1) / (a r^b + 1) * (y_i - y_j)),  r = |y_i - y_j|^2;  0 when r = 0
//   rep(i, k) = clip(2 gamma b / ((0.001 + r)(a r^b + 1)) * (y_i - y_k)),  r = |y_i - y_k|^2;  0 when r = 0 or k = i
//   y_i'      = y_i + alpha_ep * sum_{sampled e = (i -> j)} [2 att(i, j) + sum_{t < R} rep(i, k(e, ep, t))]
//   clip      per component to [-4, 4];
//   alpha_ep  = float32(learning_rate * (1 - ep / n_epochs)), computed on the host in double;
//   k(e, ep, t) = (uint64(h) * n) >> 32,  h = mix(mix(mix(seed ^ ep * 0x9e3779b9) + e) + t)     (uint32, wrapping)
//   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (common.h: lowbias32)
// (umap-learn draws a number of negatives per positive sample that accumulates to R up to floor jitter; here it is R.)
//
// Float32 arithmetic of one term, as the tests count it (u = 2^-24): d_c = y_i[c] - y_j[c]; r = the sum of d_c * d_c over
// the padded components in butterfly order; p = powf(r, b); att coefficient = (c_att * p) / (r * (a * p + 1)) with
// c_att = float32(-2ab), so r^(b-1) is p / r; rep coefficient = c_rep / ((0.001f + r) * (a * p + 1)) with
// c_rep = float32(2 gamma b); the term is clip(coefficient * d_c).
//
// Shape of the work: one wave per vertex; the wave's 64 lanes are EPP = 64 / DP entry slots of DP lanes, DP the
// dimension padded to a power of two (dim 2: 32 entries at a time; dim 50: one).  A slot's lanes hold one component
// each: the gathers of a row are contiguous, r is a DPP sum over the slot.  Passes without a sampled entry are
// skipped (a wave-uniform branch).  Every lane adds its terms in entry order, then the slots of a component are added
// in slot order through LDS by the lanes of slot 0, which write y'.  y (1.4 MB at 172 950 x 2) lives in L2: the kernel
// is bound by gather latency, which the many resident waves cover.
#include "common.h"

namespace {

constexpr int UM_THREADS = 256;
constexpr int UM_MAX_DIM = 64;
constexpr int UM_MAX_NEG = 64;

__global__ __launch_bounds__(UM_THREADS) void umap_smooth_knn_kernel(const float* __restrict__ dist, const int* __restrict__ idx,
                                                                     int n, int k, const double* __restrict__ mean_all,
                                                                     float* __restrict__ rho, float* __restrict__ sigma,
                                                                     float* __restrict__ w) {
  const int i = blockIdx.x * UM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* dr = dist + (size_t)i * k;
  float rho_f = 0.f;
  double sum = 0.0;
  for (int j = 0; j < k; ++j) {
    const float v = dr[j];
    sum += (double)v;
    if (rho_f == 0.f && v > 0.f) rho_f = v;
  }
  const double rho_d = (double)rho_f, target = log2((double)k);
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int it = 0; it < 64; ++it) {
    double psum = 0.0;
    for (int j = 1; j < k; ++j) {
      const double d = (double)dr[j] - rho_d;
      psum += d > 0.0 ? exp(-d / mid) : 1.0;
    }
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      mid = 0.5 * (lo + hi);
    } else {
      lo = mid;
      mid = hi == INFINITY ? 2.0 * mid : 0.5 * (lo + hi);
    }
  }
  const double floor_s = 1e-3 * (rho_f > 0.f ? sum / (double)k : *mean_all);
  if (mid < floor_s) mid = floor_s;
  const float sg = (float)mid;
  rho[i] = rho_f;
  sigma[i] = sg;
  for (int j = 0; j < k; ++j) {
    const double d = (double)dr[j] - rho_d;
    double val;
    if (idx[(size_t)i * k + j] == i)
      val = 0.0;
    else if (d <= 0.0 || sg == 0.f)
      val = 1.0;
    else
      val = exp(-d / (double)sg);
    w[(size_t)i * k + j] = (float)val;
  }
}

struct UmLayoutArgs {
  const float* y;
  float* y_out;
  const int* indptr;
  const int* indices;
  const uint32_t* q;
  int n, dim, neg_rate;
  uint32_t ep, ep_key;  // ep_key = mix(seed ^ ep * 0x9e3779b9)
  float a, b, c_att, c_rep, alpha;
};

__device__ __forceinline__ float um_clip(float v) { return fminf(4.f, fmaxf(-4.f, v)); }

template <int DP>
__global__ __launch_bounds__(UM_THREADS) void umap_layout_kernel(const UmLayoutArgs p) {
  constexpr int EPP = 64 / DP;
  __shared__ float red[UM_THREADS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & (DP - 1), es = lane / DP;
  const int i = blockIdx.x * (UM_THREADS / 64) + __builtin_amdgcn_readfirstlane(wave);
  const bool live = i < p.n;  // (a whole wave at once: no early return, the block meets at the barrier below)
  const bool comp = c < p.dim;
  float yi = 0.f, acc = 0.f;
  if (live) {
    const float* yrow = p.y + (size_t)i * p.dim;
    yi = comp ? yrow[c] : 0.f;
    const int beg = p.indptr[i], end = p.indptr[i + 1];
    for (int e0 = beg; e0 < end; e0 += EPP) {
      const int e = e0 + es;
      const uint32_t qe = e < end ? p.q[e] : 0u;
      const bool hit = (((uint64_t)(p.ep + 1u) * qe) >> 16) > (((uint64_t)p.ep * qe) >> 16);
      if (__ballot(hit) == 0ull) continue;
      {
        const int j = hit ? p.indices[e] : i;
        const float yj = comp ? p.y[(size_t)j * p.dim + c] : 0.f;
        const float d = yi - yj;
        const float r = group_sum<DP>(d * d);
        const float pb = powf(r, p.b);
        const float coef = (p.c_att * pb) / (r * (p.a * pb + 1.f));
        if (hit && r > 0.f) acc += 2.f * um_clip(coef * d);
      }
      const uint32_t key = lowbias32(p.ep_key + (uint32_t)e);
      for (int t = 0; t < p.neg_rate; ++t) {
        const uint32_t h = lowbias32(key + (uint32_t)t);
        const int kk = hit ? (int)(((uint64_t)h * (uint32_t)p.n) >> 32) : i;
        const float yk = comp ? p.y[(size_t)kk * p.dim + c] : 0.f;
        const float d = yi - yk;
        const float r = group_sum<DP>(d * d);
        const float pb = powf(r, p.b);
        const float coef = p.c_rep / ((0.001f + r) * (p.a * pb + 1.f));
        if (hit && kk != i && r > 0.f) acc += um_clip(coef * d);
      }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (live && es == 0 && comp) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < EPP; ++q) s += red[wave * 64 + q * DP + c];
    p.y_out[(size_t)i * p.dim + c] = yi + p.alpha * s;
  }
}

template <int DP>
void um_launch(const UmLayoutArgs& a, hipStream_t st) {
  umap_layout_kernel<DP><<<wm_cdiv(a.n, UM_THREADS / 64), UM_THREADS, 0, st>>>(a);
}

inline uint32_t um_mix_host(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

}  // namespace

extern "C" int wm_umap_smooth_knn(const float* dist, const int32_t* idx, int n, int k, const double* mean_dist, float* rho,
                                  float* sigma, float* weights, void* stream) {
  WM_REQUIRE(dist && idx && mean_dist && rho && sigma && weights, WM_EINVAL);
  WM_REQUIRE(n > 0 && k > 0 && k <= n, WM_EINVAL);
  WM_REQUIRE(k <= 64 && n <= (1 << 24), WM_EUNSUPPORTED);
  umap_smooth_knn_kernel<<<wm_cdiv(n, UM_THREADS), UM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      dist, idx, n, k, mean_dist, rho, sigma, weights);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_umap_layout(float* y_a, float* y_b, const int32_t* indptr, const int32_t* indices, const uint32_t* q, int n,
                              int dim, double a, double b, double gamma, double learning_rate, uint32_t seed, int epoch_begin,
                              int epoch_end, int n_epochs, int neg_rate, int* result_buffer, void* stream) {
  WM_REQUIRE(y_a && y_b && y_a != y_b && indptr && indices && q && result_buffer, WM_EINVAL);
  WM_REQUIRE(n > 0 && dim > 0 && n_epochs > 0 && epoch_begin >= 0 && epoch_begin <= epoch_end && epoch_end <= n_epochs,
             WM_EINVAL);
  WM_REQUIRE(a > 0.0 && b > 0.0 && gamma >= 0.0 && learning_rate >= 0.0 && neg_rate >= 0, WM_EINVAL);
  WM_REQUIRE(dim <= UM_MAX_DIM && neg_rate <= UM_MAX_NEG && n <= (1 << 24), WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  UmLayoutArgs p = {};
  p.indptr = indptr;
  p.indices = indices;
  p.q = q;
  p.n = n;
  p.dim = dim;
  p.neg_rate = neg_rate;
  p.a = (float)a;
  p.b = (float)b;
  p.c_att = (float)(-2.0 * a * b);
  p.c_rep = (float)(2.0 * gamma * b);
  float* cur = y_a;
  float* nxt = y_b;
  for (int ep = epoch_begin; ep < epoch_end; ++ep) {
    p.y = cur;
    p.y_out = nxt;
    p.ep = (uint32_t)ep;
    p.ep_key = um_mix_host(seed ^ ((uint32_t)ep * 0x9e3779b9U));
    p.alpha = (float)(learning_rate * (1.0 - (double)ep / (double)n_epochs));
    if (dim == 1) um_launch<1>(p, st);
    else if (dim == 2) um_launch<2>(p, st);
    else if (dim <= 4) um_launch<4>(p, st);
    else if (dim <= 8) um_launch<8>(p, st);
    else if (dim <= 16) um_launch<16>(p, st);
    else if (dim <= 32) um_launch<32>(p, st);
    else um_launch<64>(p, st);
    WM_LAUNCH_CHECK();
    float* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  *result_buffer = cur == y_a ? 0 : 1;
  return WM_OK;
}
