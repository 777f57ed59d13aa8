// UMAP on the exact kNN graph (manifold.py; reference notebooks 3.0-Embeddings-inference, 3.1-Embeddings-clustering,
// 3.2-Embeddings-SSL-categories and the 2.0 figure notebooks: umap.UMAP(...).fit_transform(data)):
//   wm_umap_smooth_knn   per row of the kNN graph (csrc/cluster.hip: wm_knn_graph) the fuzzy-simplicial-set parameters
//                        rho, sigma and the membership weights;
//   wm_umap_layout       the layout optimisation, the hot path: one launch per epoch over every graph entry;
//   wm_umap_label_intersect, wm_umap_smooth_knn_query, wm_umap_transform_layout
//                        semi-supervised fits (y=) and the transform of new rows: stated at the end of this comment.
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
//
// ---- DensMAP (umap-learn's densmap=True: _optimize_layout_euclidean_densmap_epoch_init and the densmap branch of its
// epoch loop, restated for the gather above; manifold.DensMAP).  With w_e the graph's float32 weight of entry e,
// eps = 1e-8, r = |y_i - y_j|^2, p = r^b:
//   live(e)   = uint64(q_e) * n_epochs >= 65536: the entry is sampled at least once (umap-learn prunes weights below
//               max / n_epochs; here nothing is dropped physically, entries that are not live take part in no sum);
//   dist_e    = max(d_ij, d_ji) over the kNN distances, a missing direction counting 0 (float32, aligned with the CSR);
//   ro_i      = log(eps + sum_live w_e dist_e^2 / sum_live w_e), log eps for a row without live entries
//               (wm_densmap_graph_radii, once per fit, one thread per row in double, rounded once);
//   R         = (ro - mean) / std (population std; 0 when std = 0), formed by the caller;  mu_tot = sum_live w_e;
//   phase(ep) = dens_lambda > 0 and (ep + 1) / n_epochs > 1 - dens_frac, in double exactly as written.
// At the start of a phase epoch, from the positions before that epoch (phi_e = 1 / (1 + a p)):
//   D_i = 2 sum_live phi_e,  N_i = 2 sum_live phi_e r,  re_i = log(eps + N_i / D_i), log eps when D_i = 0
//         (densmap_radii_kernel: one wave per vertex with the slot layout of the layout kernel, everything in double;
//         of every 64 consecutive entries each lane takes one, adds its terms in entry order, then the 64 lanes are
//         added in lane order; r = 0 gives phi = 1 and adds to D only);
//   mean = sum re / n,  var = sum (re - mean)^2 / n (two passes),  std = sqrt(var + dens_var_shift),
//   cov  = sum re_i R_i / (n - 1),  W_i = R_i - cov (re_i - mean) / std^2
//         (densmap_sum1 / sum2 / terms kernels: every thread adds its strided elements in order, a block adds its 256
//         threads in a fixed tree and stores the partial into its slot, the next kernel adds the slots in the same way:
//         no atomics, no host synchronisation, two runs give the same bits).
// The terms kernel leaves per vertex the four float32 values the layout reads, each formed in double and rounded
// once: 1 / D_i (0 when D_i = 0), 1 / (eps + N_i / D_i), W_i (R_i when std = 0), re_i; and the scalar
// s = dens_lambda mu_tot / (std n) (0 when std = 0).  In a phase epoch every sampled entry e = (i -> j) then adds
//   dens(i, j) = 2 clip(2 g_e (y_i - y_j)), 0 when r = 0;   g_e = s (W_i dr_i + W_j dr_j) / w_e,
//   dr_v = (phi_e / D_v) ((1 - b (1 - phi_e)) / (eps + N_v / D_v) + a b p / (r (1 + a p)))
// to the terms of vertex i: g_e is symmetric in (i, j), so as for the attraction the move of the head and of the tail
// become twice the term at the head.  Outside the phase an epoch is the plain epoch above, by the same kernel.
// Float32 arithmetic of the density term: phi = 1 / (a p + 1); 1 - b (1 - phi) as fma(b, phi, 1 - b) (two positive
// parts, no cancellation); t2 = (float32(ab) p) / (r (a p + 1)); dr_v = (phi * invD_v) * (t1 * invden_v + t2);
// g = (s * (W_i dr_i + W_j dr_j)) / w_e; the term is 2 clip((2 g) d_c).
//
// Workspace of wm_densmap_layout (16-byte aligned, wm_densmap_layout_workspace_bytes(n) = 4160 + 40 n bytes):
//   [0, 64)        double mu_tot, mean, var, cov, std; float s at byte 40 (written in every phase epoch)
//   [64, 4160)     double slots[4][128]: partial sums of mu_tot, re, (re - mean)^2, re R
//   [4160, +16 n)  float32 [n][4]: 1 / D, 1 / (eps + N / D), W, re
//   then           double re[n], D[n], N / D [n]
//
// ---- label intersection (umap-learn's discrete_metric_simplicial_set_intersection + reset_local_connectivity for a
// categorical target; manifold.InductiveUMAP.fit(x, y)).  G is the symmetric-pattern CSR of the union above, labels
// int32 [n] with -1 = unknown, f_far = exp(-far_dist), f_unk = exp(-unknown_dist) formed by the host in double:
//   f_e   = f_unk if either label of e = (i -> j) is -1, f_far if the labels differ, else 1;   v_e = double(w_e) f_e
//   max_i = max_e v_e over row i;   m_e = v_e / max_i, 0 when max_i = 0          (normalize(norm="max"): a zero row stays
//           zero, no NaN appears)
//   g_e   = (m_e + m_t) - m_e m_t in double, t the entry (j -> i), found by binary search in row j's sorted columns
//           (m_t = 0 if absent); rounded once to float32.
// Both directions evaluate the same expression on the same two numbers (sum and product commute; contraction is
// switched off so that neither direction fuses what the other does not): the result is symmetric in bits.  The
// pattern is unchanged: an entry that becomes 0 stays as an explicit zero whose rate is 0.  Two kernels of one thread
// per row, no atomics; the workspace is max_i, one double per row.
//
// ---- memberships of new rows (umap-learn's smooth_knn_dist(local_connectivity = 0) + compute_membership_strengths
// (bipartite=True) as UMAP.transform calls them).  Row i holds the k distances of a new row to its nearest fitted rows:
//   rho_i = 0;   sigma_i: the bisection above on S(s) = sum_{j >= 1} (d_j > 0 ? exp(-d_j / s) : 1) (the first neighbour
//   is skipped exactly as umap-learn skips it), then s >= 1e-3 * the mean of all m k distances;
//   w_ij = 1 where d_j <= 0, else exp(-d_j / sigma_i); there is no self test.
// In double; sigma is rounded to float32 and the weights are computed from the rounded value.
//
// ---- transform layout (umap-learn's optimize_layout_euclidean(move_other=False) of UMAP.transform, restated as above)
// y_train float32 [n][dim] are the fitted positions, read only; new point i has k entries e = i k + j with neighbour
// idx_e in [0, n) and rate q_e.  With sampled, att, rep, clip and mix of the layout above:
//   y_i'      = y_i + alpha_ep * sum_{sampled e} [att(y_i, Y[idx_e]) + sum_{t < R} rep(y_i, Y[k(e, ep, t)])]
//   alpha_ep  = float32((learning_rate / 4) * (1 - ep / n_epochs)), in double exactly as written, in the kernel;
//   k(e, ep, t) = (uint64(h) * n) >> 32,  h = mix(mix(mix(seed ^ ep * 0x9e3779b9) + e) + t).
// The attraction counts once: only the head moves.  Negatives are drawn from the n fitted points; the force is 0 at
// r = 0 (umap-learn's j == k skip compares a new index with a fitted one and is not restated).  All terms of an epoch read
// the position from before that epoch.
// No new point reads another new point, so nothing orders the epochs of different points: ONE launch runs all epochs
// of [epoch_begin, epoch_end), one wave per new point with the slot layout of the layout kernel (EPP = 64 / DP entry
// slots of DP component lanes), y_i in registers throughout (every slot holds the same bits of it), the epoch key and
// alpha_ep computed in the kernel, the point's idx / q rows staged once in a strip of LDS that only this wave touches,
// the result written once at the end.  No block barrier, no atomics, no traffic between waves.  An epoch of a wave is
// bound by the vector ALU (one powf per term on all 64 lanes) like the fit kernel's: fetching the rows of a pass's
// 1 + R terms together before using the first, and one-wave workgroups, were tried and were no faster
// (profiles/umap_transform.md).
// Order of the additions of an epoch: every lane adds the terms of its entries in entry order (per entry the
// attraction, then the R repulsions); then the EPP slots of a component are added by an xor butterfly over the lane
// strides DP, 2 DP, ..., 32 in that order (strides 1 and 2: quad_perm; 4 and 8: __shfl_xor; 16 and 32:
// v_permlane16/32_swap) -- true xor exchanges, so both partners add the same two numbers and, float addition being
// commutative, every slot ends with the same bits; log2(EPP) additions.  An epoch without a sampled entry leaves y_i as
// it is.
#include <type_traits>

#include "common.h"

namespace {

constexpr int UM_THREADS = 256;
constexpr int UM_MAX_DIM = 64;
constexpr int UM_MAX_NEG = 64;

// ---- smooth kNN: one thread per row, in double.  FIT: the rows of a fit (rho is subtracted, the row itself weighs 0);
// otherwise the rows of new points (rho = 0 is not subtracted, there is no self test).

template <bool FIT>
__device__ __forceinline__ double um_excess(float d, double rho) {
  if constexpr (FIT) return (double)d - rho;
  else return (double)d;
}

// The bisection of the header on the row dr[0 .. k), then the floor; rounded to float32.
template <bool FIT>
__device__ __forceinline__ float um_sigma(const float* __restrict__ dr, int k, double rho, double floor_s) {
  const double target = log2((double)k);
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int it = 0; it < 64; ++it) {
    double psum = 0.0;
    for (int j = 1; j < k; ++j) {
      const double d = um_excess<FIT>(dr[j], rho);
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
  if (mid < floor_s) mid = floor_s;
  return (float)mid;
}

// The memberships of row i from the rounded sigma; idx_row is read only with FIT.
template <bool FIT>
__device__ __forceinline__ void um_weights(const float* __restrict__ dr, const int* __restrict__ idx_row, int i, int k, double rho,
                                           float sg, float* __restrict__ w_row) {
  for (int j = 0; j < k; ++j) {
    const double d = um_excess<FIT>(dr[j], rho);
    double val;
    if (FIT && idx_row[j] == i)
      val = 0.0;
    else if (d <= 0.0 || sg == 0.f)
      val = 1.0;
    else
      val = exp(-d / (double)sg);
    w_row[j] = (float)val;
  }
}

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
  const double rho_d = (double)rho_f;
  const float sg = um_sigma<true>(dr, k, rho_d, 1e-3 * (rho_f > 0.f ? sum / (double)k : *mean_all));
  rho[i] = rho_f;
  sigma[i] = sg;
  um_weights<true>(dr, idx + (size_t)i * k, i, k, rho_d, sg, w + (size_t)i * k);
}

__global__ __launch_bounds__(UM_THREADS) void umap_smooth_knn_query_kernel(const float* __restrict__ dist, int m, int k,
                                                                           const double* __restrict__ mean_all,
                                                                           float* __restrict__ sigma, float* __restrict__ w) {
  const int i = blockIdx.x * UM_THREADS + threadIdx.x;
  if (i >= m) return;
  const float* dr = dist + (size_t)i * k;
  const float sg = um_sigma<false>(dr, k, 0.0, 1e-3 * *mean_all);
  sigma[i] = sg;
  um_weights<false>(dr, nullptr, i, k, 0.0, sg, w + (size_t)i * k);
}

// ---- layout and transform layout
// Both kernels write the attraction and the repulsion of the header out in place.  Shared force-inlined helpers for
// them (eight shapes tried) gave the same bits, but hipcc then lays the layout kernel's loops out differently and its
// 50-D epoch at 172 950 vertices took 0.9 - 2.6 % longer (profiles/umap_refactor.md): keep the four copies in step.

// The scalars of a term, which the arguments P of both kernels carry under these names.
template <class P>
void um_fill_force(P& p, int dim, int neg_rate, double a, double b, double gamma) {
  p.dim = dim;
  p.neg_rate = neg_rate;
  p.a = (float)a;
  p.b = (float)b;
  p.c_att = (float)(-2.0 * a * b);
  p.c_rep = (float)(2.0 * gamma * b);
}

__device__ __forceinline__ float um_clip(float v) { return fminf(4.f, fmaxf(-4.f, v)); }

// The padded dimension DP of `dim` (1, 2, 4, ..., 64) picks the instantiation: fn(std::integral_constant<int, DP>).
template <class F>
void um_with_dp(int dim, F&& fn) {
  if (dim == 1) fn(std::integral_constant<int, 1>{});
  else if (dim == 2) fn(std::integral_constant<int, 2>{});
  else if (dim <= 4) fn(std::integral_constant<int, 4>{});
  else if (dim <= 8) fn(std::integral_constant<int, 8>{});
  else if (dim <= 16) fn(std::integral_constant<int, 16>{});
  else if (dim <= 32) fn(std::integral_constant<int, 32>{});
  else fn(std::integral_constant<int, 64>{});
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
  // density phase only (DENS)
  const float* data;    // w_e
  const float4* vert;   // per vertex: 1 / D, 1 / (eps + N / D), W, re
  const float* scale;   // s = dens_lambda mu_tot / (std n), on the device
  float ab, omb;        // float32(a b), float32(1 - b)
};

// DENS = false is the plain UMAP epoch; DENS = true adds the density term of a DensMAP phase epoch to every sampled entry.
template <int DP, bool DENS>
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
    float4 vi = {0.f, 0.f, 0.f, 0.f};
    float scale = 0.f;
    if constexpr (DENS) {
      vi = p.vert[i];
      scale = *p.scale;
    }
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
        if constexpr (DENS) {
          const float4 vj = hit ? p.vert[j] : vi;
          const float we = hit ? p.data[e] : 1.f;
          const float apb1 = p.a * pb + 1.f;
          const float phi = 1.f / apb1;
          const float t1 = fmaf(p.b, phi, p.omb);
          const float t2 = (p.ab * pb) / (r * apb1);
          const float dri = (phi * vi.x) * (t1 * vi.y + t2);
          const float drj = (phi * vj.x) * (t1 * vj.y + t2);
          const float g = (scale * (vi.z * dri + vj.z * drj)) / we;
          if (hit && r > 0.f) acc += 2.f * um_clip((2.f * g) * d);
        }
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

// ---- DensMAP: radii, statistics, per-vertex terms

constexpr int DM_THREADS = 256;
constexpr int DM_SLOTS = 128;
constexpr size_t DM_HEAD = 64 + 4 * DM_SLOTS * sizeof(double);  // scalars and slots: 4160 bytes
constexpr double DM_EPS = 1e-8;

__device__ __forceinline__ bool dm_live(uint32_t q, uint32_t n_epochs) { return (uint64_t)q * n_epochs >= 65536ull; }

__global__ __launch_bounds__(DM_THREADS) void densmap_graph_radii_kernel(const int* __restrict__ indptr,
                                                                         const float* __restrict__ data,
                                                                         const float* __restrict__ dists,
                                                                         const uint32_t* __restrict__ q, int n,
                                                                         uint32_t n_epochs, float* __restrict__ ro) {
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i >= n) return;
  double num = 0.0, den = 0.0;
  for (int e = indptr[i]; e < indptr[i + 1]; ++e) {
    if (!dm_live(q[e], n_epochs)) continue;
    const double w = (double)data[e], d = (double)dists[e];
    num += w * d * d;
    den += w;
  }
  ro[i] = (float)log(DM_EPS + (den > 0.0 ? num / den : 0.0));
}

template <int W>
__device__ __forceinline__ double dm_group_sum(double v) {
#pragma unroll
  for (int m = 1; m < W; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// D_i, N_i / D_i and re_i of the positions y; outputs that are null are not written.
template <int DP>
__global__ __launch_bounds__(UM_THREADS) void densmap_radii_kernel(const float* __restrict__ y, const int* __restrict__ indptr,
                                                                   const int* __restrict__ indices,
                                                                   const uint32_t* __restrict__ q, int n, int dim, double a,
                                                                   double b, uint32_t n_epochs, double* __restrict__ re_d,
                                                                   double* __restrict__ d_d, double* __restrict__ ratio_d,
                                                                   float* __restrict__ re_f, float* __restrict__ d_f) {
  constexpr int EPP = 64 / DP;
  __shared__ double red[2][UM_THREADS / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & (DP - 1), es = lane / DP;
  const int i = blockIdx.x * (UM_THREADS / 64) + __builtin_amdgcn_readfirstlane(wave);
  const bool live = i < n;
  const bool comp = c < dim;
  double sd = 0.0, sn = 0.0;
  if (live) {
    const double yi = comp ? (double)y[(size_t)i * dim + c] : 0.0;
    const int beg = indptr[i], end = indptr[i + 1];
    // A batch of 64 entries is DP passes of EPP entries; pass ps leaves the r of slot es's entry in lane (es, c = ps), so
    // that after the batch every lane holds one entry and the wave pays for one pow per 64 entries, not one per pass.
    for (int b0 = beg; b0 < end; b0 += 64) {
      double rm = 0.0;
      bool lm = false;
      for (int ps = 0; ps < DP && b0 + ps * EPP < end; ++ps) {
        const int e = b0 + ps * EPP + es;
        const bool lv = e < end && dm_live(q[e], n_epochs);
        if (__ballot(lv) == 0ull) continue;
        const int j = lv ? indices[e] : i;
        const double yj = comp ? (double)y[(size_t)j * dim + c] : 0.0;
        const double d = yi - yj;
        const double r = dm_group_sum<DP>(d * d);
        if (c == ps) {
          rm = r;
          lm = lv;
        }
      }
      if (lm) {
        const double phi = 1.0 / (1.0 + a * pow(rm, b));
        sd += phi;
        sn += phi * rm;
      }
    }
  }
  red[0][wave][lane] = sd;
  red[1][wave][lane] = sn;
  __syncthreads();
  if (live && lane == 0) {
    double dsum = 0.0, nsum = 0.0;
    for (int s = 0; s < 64; ++s) {
      dsum += red[0][wave][s];
      nsum += red[1][wave][s];
    }
    dsum *= 2.0;
    nsum *= 2.0;
    const double ratio = dsum > 0.0 ? nsum / dsum : 0.0;
    const double re = log(DM_EPS + ratio);
    if (re_d) re_d[i] = re;
    if (d_d) d_d[i] = dsum;
    if (ratio_d) ratio_d[i] = ratio;
    if (re_f) re_f[i] = (float)re;
    if (d_f) d_f[i] = (float)dsum;
  }
}

// The sum of one value per thread over a block of DM_THREADS threads, in a fixed tree; every thread gets it.
__device__ __forceinline__ double dm_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = DM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double dm_slot_total(const double* __restrict__ slots, int nb, double* lds) {
  return dm_block_sum((int)threadIdx.x < nb ? slots[threadIdx.x] : 0.0, lds);
}
static_assert(DM_SLOTS <= DM_THREADS, "one slot per thread");

// slots[0][block] = the block's part of mu_tot = sum_live w_e
__global__ __launch_bounds__(DM_THREADS) void densmap_mu_kernel(const float* __restrict__ data, const uint32_t* __restrict__ q,
                                                                long long nnz, uint32_t n_epochs, double* __restrict__ slots) {
  __shared__ double lds[DM_THREADS];
  double v = 0.0;
  for (long long e = (long long)blockIdx.x * DM_THREADS + threadIdx.x; e < nnz; e += (long long)gridDim.x * DM_THREADS)
    if (dm_live(q[e], n_epochs)) v += (double)data[e];
  const double t = dm_block_sum(v, lds);
  if (threadIdx.x == 0) slots[blockIdx.x] = t;
}

// slots[1][block] = the block's part of sum re
__global__ __launch_bounds__(DM_THREADS) void densmap_sum1_kernel(const double* __restrict__ re, int n, double* __restrict__ slots) {
  __shared__ double lds[DM_THREADS];
  double v = 0.0;
  for (int i = blockIdx.x * DM_THREADS + threadIdx.x; i < n; i += gridDim.x * DM_THREADS) v += re[i];
  const double t = dm_block_sum(v, lds);
  if (threadIdx.x == 0) slots[DM_SLOTS + blockIdx.x] = t;
}

// slots[2][block], slots[3][block] = the block's parts of sum (re - mean)^2 and sum re R
__global__ __launch_bounds__(DM_THREADS) void densmap_sum2_kernel(const double* __restrict__ re, const float* __restrict__ rad, int n,
                                                                  double* __restrict__ slots) {
  __shared__ double lds[DM_THREADS];
  const double mean = dm_slot_total(slots + DM_SLOTS, gridDim.x, lds) / (double)n;
  double v = 0.0, cv = 0.0;
  for (int i = blockIdx.x * DM_THREADS + threadIdx.x; i < n; i += gridDim.x * DM_THREADS) {
    const double x = re[i];
    v += (x - mean) * (x - mean);
    cv += x * (double)rad[i];
  }
  const double tv = dm_block_sum(v, lds), tc = dm_block_sum(cv, lds);
  if (threadIdx.x == 0) {
    slots[2 * DM_SLOTS + blockIdx.x] = tv;
    slots[3 * DM_SLOTS + blockIdx.x] = tc;
  }
}

// The per-vertex float32 values and the scalar s the density layout reads; one thread per vertex.
__global__ __launch_bounds__(DM_THREADS) void densmap_terms_kernel(const double* __restrict__ re, const double* __restrict__ dd,
                                                                   const double* __restrict__ ratio, const float* __restrict__ rad,
                                                                   int n, int nb_vertex, int nb_entry, double dens_lambda,
                                                                   double var_shift, const double* __restrict__ slots,
                                                                   float4* __restrict__ vert, double* __restrict__ scal) {
  __shared__ double lds[DM_THREADS];
  const double mu = dm_slot_total(slots, nb_entry, lds);
  const double mean = dm_slot_total(slots + DM_SLOTS, nb_vertex, lds) / (double)n;
  const double var = dm_slot_total(slots + 2 * DM_SLOTS, nb_vertex, lds) / (double)n;
  const double cov = dm_slot_total(slots + 3 * DM_SLOTS, nb_vertex, lds) / (double)(n - 1);
  const double sd = sqrt(var + var_shift);
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i < n) {
    const double d = dd[i], x = re[i], r = (double)rad[i];
    float4 v;
    v.x = (float)(d > 0.0 ? 1.0 / d : 0.0);
    v.y = (float)(1.0 / (DM_EPS + ratio[i]));
    v.z = (float)(sd > 0.0 ? r - cov * (x - mean) / (sd * sd) : r);
    v.w = (float)x;
    vert[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scal[0] = mu;
    scal[1] = mean;
    scal[2] = var;
    scal[3] = cov;
    scal[4] = sd;
    reinterpret_cast<float*>(scal + 5)[0] = (float)(sd > 0.0 ? dens_lambda * mu / (sd * (double)n) : 0.0);
  }
}

void dm_radii_launch(const float* y, const int* indptr, const int* indices, const uint32_t* q, int n, int dim, double a, double b,
                     int n_epochs, double* re_d, double* d_d, double* ratio_d, float* re_f, float* d_f, hipStream_t st) {
  um_with_dp(dim, [&](auto dp) {
    densmap_radii_kernel<decltype(dp)::value><<<wm_cdiv(n, UM_THREADS / 64), UM_THREADS, 0, st>>>(
        y, indptr, indices, q, n, dim, a, b, (uint32_t)n_epochs, re_d, d_d, ratio_d, re_f, d_f);
  });
}

inline int dm_blocks(long long count) {
  const int nb = wm_cdiv(count, DM_THREADS);
  return nb < 1 ? 1 : (nb > DM_SLOTS ? DM_SLOTS : nb);
}

// ---- label intersection

__device__ __forceinline__ double um_label_factor(int li, int lj, double f_far, double f_unk) {
  return (li < 0 || lj < 0) ? f_unk : (li != lj ? f_far : 1.0);
}

// ws[i] = max_e double(w_e) f_e over row i
__global__ __launch_bounds__(UM_THREADS) void umap_label_max_kernel(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                                    const float* __restrict__ data, const int* __restrict__ labels,
                                                                    int n, double f_far, double f_unk, double* __restrict__ ws) {
  const int i = blockIdx.x * UM_THREADS + threadIdx.x;
  if (i >= n) return;
  const int li = labels[i];
  double mx = 0.0;
  for (int e = indptr[i]; e < indptr[i + 1]; ++e) {
    const double v = (double)data[e] * um_label_factor(li, labels[indices[e]], f_far, f_unk);
    mx = v > mx ? v : mx;
  }
  ws[i] = mx;
}

__global__ __launch_bounds__(UM_THREADS) void umap_label_intersect_kernel(const int* __restrict__ indptr,
                                                                          const int* __restrict__ indices,
                                                                          const float* __restrict__ data,
                                                                          const int* __restrict__ labels, int n, double f_far,
                                                                          double f_unk, const double* __restrict__ ws,
                                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * UM_THREADS + threadIdx.x;
  if (i >= n) return;
  const int li = labels[i];
  const double mi = ws[i];
  for (int e = indptr[i]; e < indptr[i + 1]; ++e) {
    const int j = indices[e];
    const double f = um_label_factor(li, labels[j], f_far, f_unk);
    const double me = mi > 0.0 ? ((double)data[e] * f) / mi : 0.0;
    int lo = indptr[j], hi = indptr[j + 1];  // the first entry of row j whose column is not below i
    const int end = hi;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (indices[mid] < i) lo = mid + 1; else hi = mid;
    }
    const double mj = ws[j];
    const double mt = (lo < end && indices[lo] == i && mj > 0.0) ? ((double)data[lo] * f) / mj : 0.0;
    out[e] = (float)((me + mt) - me * mt);
  }
}

// ---- transform layout

struct UmTransformArgs {
  const float* y_in;
  float* y_out;
  const float* y_train;
  const int* idx;
  const uint32_t* q;
  int m, n, k, dim, neg_rate;
  uint32_t seed;
  int ep_begin, ep_end;
  double lr4, n_epochs;  // learning_rate / 4 and n_epochs, as alpha_ep reads them
  float a, b, c_att, c_rep;
};

// The sum over the EPP slots of a component, the same bits in every slot: xor exchanges at the strides DP .. 32.
template <int DP>
__device__ __forceinline__ float um_slot_sum(float v) {
  if constexpr (DP <= 1) v += wm_dpp<0xB1>(v);
  if constexpr (DP <= 2) v += wm_dpp<0x4E>(v);
  if constexpr (DP <= 4) v += __shfl_xor(v, 4, 64);
  if constexpr (DP <= 8) v += __shfl_xor(v, 8, 64);
  if constexpr (DP <= 16) v = wm_xor16_sum(v);
  if constexpr (DP <= 32) v = wm_xor32_sum(v);
  return v;
}

template <int DP>
__global__ __launch_bounds__(UM_THREADS) void umap_transform_kernel(const UmTransformArgs p) {
  constexpr int EPP = 64 / DP;
  constexpr int WAVES = UM_THREADS / 64;
  __shared__ int s_idx[WAVES][64];
  __shared__ uint32_t s_q[WAVES][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & (DP - 1), es = lane / DP;
  const int i = blockIdx.x * WAVES + wave;
  if (i >= p.m) return;  // (a whole wave at once; the kernel has no barrier)
  const bool comp = c < p.dim;
  const int k = p.k;
  // the point's entries: written and read by this wave alone, whose LDS operations execute in order
  s_idx[wave][lane] = lane < k ? p.idx[(size_t)i * k + lane] : 0;
  s_q[wave][lane] = lane < k ? p.q[(size_t)i * k + lane] : 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float yi = comp ? p.y_in[(size_t)i * p.dim + c] : 0.f;
  const uint32_t e_base = (uint32_t)i * (uint32_t)k;
  for (int ep = p.ep_begin; ep < p.ep_end; ++ep) {
    const uint32_t uep = (uint32_t)ep;
    const uint32_t ep_key = lowbias32(p.seed ^ (uep * 0x9e3779b9U));
    float acc = 0.f;
    bool any = false;
    for (int j0 = 0; j0 < k; j0 += EPP) {
      const int jl = j0 + es;
      const uint32_t qe = jl < k ? s_q[wave][jl] : 0u;
      const bool hit = (((uint64_t)(uep + 1u) * qe) >> 16) > (((uint64_t)uep * qe) >> 16);
      if (__ballot(hit) == 0ull) continue;
      any = true;
      {
        const int j = hit ? s_idx[wave][jl] : 0;
        const float yj = comp ? p.y_train[(size_t)j * p.dim + c] : 0.f;
        const float d = yi - yj;
        const float r = group_sum<DP>(d * d);
        const float pb = powf(r, p.b);
        const float coef = (p.c_att * pb) / (r * (p.a * pb + 1.f));
        if (hit && r > 0.f) acc += um_clip(coef * d);
      }
      const uint32_t key = lowbias32(ep_key + e_base + (uint32_t)jl);
      for (int t = 0; t < p.neg_rate; ++t) {
        const uint32_t h = lowbias32(key + (uint32_t)t);
        const int kk = hit ? (int)(((uint64_t)h * (uint32_t)p.n) >> 32) : 0;
        const float yk = comp ? p.y_train[(size_t)kk * p.dim + c] : 0.f;
        const float d = yi - yk;
        const float r = group_sum<DP>(d * d);
        const float pb = powf(r, p.b);
        const float coef = p.c_rep / ((0.001f + r) * (p.a * pb + 1.f));
        if (hit && r > 0.f) acc += um_clip(coef * d);
      }
    }
    if (!any) continue;  // (wave-uniform)
    const float alpha = (float)(p.lr4 * (1.0 - (double)ep / p.n_epochs));
    yi = yi + alpha * um_slot_sum<DP>(acc);
  }
  if (es == 0 && comp) p.y_out[(size_t)i * p.dim + c] = yi;
}

// ---- host: what the three layout entry points share

// Their requirements on the shared arguments.
int um_check_layout(int dim, double a, double b, double gamma, double learning_rate, int epoch_begin, int epoch_end, int n_epochs,
                    int neg_rate) {
  WM_REQUIRE(dim > 0 && n_epochs > 0 && epoch_begin >= 0 && epoch_begin <= epoch_end && epoch_end <= n_epochs, WM_EINVAL);
  WM_REQUIRE(a > 0.0 && b > 0.0 && gamma >= 0.0 && learning_rate >= 0.0 && neg_rate >= 0, WM_EINVAL);
  WM_REQUIRE(dim <= UM_MAX_DIM && neg_rate <= UM_MAX_NEG, WM_EUNSUPPORTED);
  return WM_OK;
}

// What wm_densmap_layout adds to wm_umap_layout.
struct UmDensity {
  const float* data;
  const float* rad;
  int nnz;
  double lambda, frac, var_shift;
  char* ws;  // the workspace of the header
};

// Epochs [epoch_begin, epoch_end) of the layout, double-buffered between y_a and y_b; with `dens`, the epochs of its phase
// first compute the radii, their statistics and the per-vertex terms, and run the kernel with the density term.
int um_run_epochs(float* y_a, float* y_b, const int32_t* indptr, const int32_t* indices, const uint32_t* q, int n, int dim, double a,
                  double b, double gamma, double learning_rate, uint32_t seed, int epoch_begin, int epoch_end, int n_epochs,
                  int neg_rate, const UmDensity* dens, int* result_buffer, hipStream_t st) {
  UmLayoutArgs p = {};
  p.indptr = indptr;
  p.indices = indices;
  p.q = q;
  p.n = n;
  um_fill_force(p, dim, neg_rate, a, b, gamma);
  double *scal = nullptr, *slots = nullptr, *re_d = nullptr, *d_d = nullptr, *ratio_d = nullptr;
  float4* vert = nullptr;
  if (dens) {
    scal = reinterpret_cast<double*>(dens->ws);
    slots = reinterpret_cast<double*>(dens->ws + 64);
    vert = reinterpret_cast<float4*>(dens->ws + DM_HEAD);
    re_d = reinterpret_cast<double*>(dens->ws + DM_HEAD + (size_t)n * sizeof(float4));
    d_d = re_d + n;
    ratio_d = d_d + n;
    p.data = dens->data;
    p.vert = vert;
    p.scale = reinterpret_cast<const float*>(scal + 5);
    p.ab = (float)(a * b);
    p.omb = (float)(1.0 - b);
  }
  const int grid = wm_cdiv(n, UM_THREADS / 64);
  const int nb_vertex = dm_blocks(n);
  int nb_entry = 0;  // (mu_tot is summed before the call's first phase epoch)
  float* cur = y_a;
  float* nxt = y_b;
  for (int ep = epoch_begin; ep < epoch_end; ++ep) {
    p.y = cur;
    p.y_out = nxt;
    p.ep = (uint32_t)ep;
    p.ep_key = lowbias32(seed ^ ((uint32_t)ep * 0x9e3779b9U));
    p.alpha = (float)(learning_rate * (1.0 - (double)ep / (double)n_epochs));
    const bool phase = dens && dens->lambda > 0.0 && (double)(ep + 1) / (double)n_epochs > 1.0 - dens->frac;
    if (phase) {
      if (nb_entry == 0) {
        nb_entry = dm_blocks(dens->nnz);
        densmap_mu_kernel<<<nb_entry, DM_THREADS, 0, st>>>(dens->data, q, (long long)dens->nnz, (uint32_t)n_epochs, slots);
        WM_LAUNCH_CHECK();
      }
      dm_radii_launch(cur, indptr, indices, q, n, dim, a, b, n_epochs, re_d, d_d, ratio_d, nullptr, nullptr, st);
      WM_LAUNCH_CHECK();
      densmap_sum1_kernel<<<nb_vertex, DM_THREADS, 0, st>>>(re_d, n, slots);
      WM_LAUNCH_CHECK();
      densmap_sum2_kernel<<<nb_vertex, DM_THREADS, 0, st>>>(re_d, dens->rad, n, slots);
      WM_LAUNCH_CHECK();
      densmap_terms_kernel<<<wm_cdiv(n, DM_THREADS), DM_THREADS, 0, st>>>(re_d, d_d, ratio_d, dens->rad, n, nb_vertex, nb_entry,
                                                                         dens->lambda, dens->var_shift, slots, vert, scal);
      WM_LAUNCH_CHECK();
    }
    um_with_dp(dim, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      if (phase) umap_layout_kernel<DP, true><<<grid, UM_THREADS, 0, st>>>(p);
      else umap_layout_kernel<DP, false><<<grid, UM_THREADS, 0, st>>>(p);
    });
    WM_LAUNCH_CHECK();
    float* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  *result_buffer = cur == y_a ? 0 : 1;
  return WM_OK;
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
  WM_REQUIRE(y_a && y_b && y_a != y_b && indptr && indices && q && result_buffer && n > 0, WM_EINVAL);
  if (const int rc = um_check_layout(dim, a, b, gamma, learning_rate, epoch_begin, epoch_end, n_epochs, neg_rate)) return rc;
  WM_REQUIRE(n <= (1 << 24), WM_EUNSUPPORTED);
  return um_run_epochs(y_a, y_b, indptr, indices, q, n, dim, a, b, gamma, learning_rate, seed, epoch_begin, epoch_end, n_epochs,
                       neg_rate, nullptr, result_buffer, static_cast<hipStream_t>(stream));
}

extern "C" int wm_densmap_graph_radii(const int32_t* indptr, const float* data, const float* dists, const uint32_t* q, int n,
                                      int n_epochs, float* ro, void* stream) {
  WM_REQUIRE(indptr && data && dists && q && ro, WM_EINVAL);
  WM_REQUIRE(n > 0 && n_epochs > 0, WM_EINVAL);
  WM_REQUIRE(n <= (1 << 24), WM_EUNSUPPORTED);
  densmap_graph_radii_kernel<<<wm_cdiv(n, DM_THREADS), DM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      indptr, data, dists, q, n, (uint32_t)n_epochs, ro);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_densmap_embedding_radii(const float* y, const int32_t* indptr, const int32_t* indices, const uint32_t* q, int n,
                                          int dim, double a, double b, int n_epochs, float* re, float* d, void* stream) {
  WM_REQUIRE(y && indptr && indices && q && re && d, WM_EINVAL);
  WM_REQUIRE(n > 0 && dim > 0 && n_epochs > 0 && a > 0.0 && b > 0.0, WM_EINVAL);
  WM_REQUIRE(dim <= UM_MAX_DIM && n <= (1 << 24), WM_EUNSUPPORTED);
  dm_radii_launch(y, indptr, indices, q, n, dim, a, b, n_epochs, nullptr, nullptr, nullptr, re, d, static_cast<hipStream_t>(stream));
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_densmap_layout_workspace_bytes(int n) {
  if (n < 2 || n > (1 << 24)) return 0;
  return DM_HEAD + (size_t)n * (sizeof(float4) + 3 * sizeof(double));
}

extern "C" int wm_densmap_layout(float* y_a, float* y_b, const int32_t* indptr, const int32_t* indices, const uint32_t* q,
                                 const float* data, const float* rad, int n, int nnz, int dim, double a, double b,
                                 double gamma, double learning_rate, double dens_lambda, double dens_frac, double dens_var_shift, uint32_t seed,
                                 int epoch_begin, int epoch_end, int n_epochs, int neg_rate, void* workspace,
                                 size_t workspace_bytes, int* result_buffer, void* stream) {
  WM_REQUIRE(y_a && y_b && y_a != y_b && indptr && indices && q && data && rad && workspace && result_buffer, WM_EINVAL);
  WM_REQUIRE(n > 1 && nnz >= 0, WM_EINVAL);
  WM_REQUIRE(dens_lambda >= 0.0 && dens_frac >= 0.0 && dens_frac <= 1.0 && dens_var_shift >= 0.0, WM_EINVAL);
  if (const int rc = um_check_layout(dim, a, b, gamma, learning_rate, epoch_begin, epoch_end, n_epochs, neg_rate)) return rc;
  WM_REQUIRE(n <= (1 << 24), WM_EUNSUPPORTED);
  WM_REQUIRE(workspace_bytes >= wm_densmap_layout_workspace_bytes(n), WM_EWORKSPACE);
  WM_REQUIRE(((uintptr_t)workspace & 15u) == 0, WM_EALIGN);
  const UmDensity dens = {data, rad, nnz, dens_lambda, dens_frac, dens_var_shift, static_cast<char*>(workspace)};
  return um_run_epochs(y_a, y_b, indptr, indices, q, n, dim, a, b, gamma, learning_rate, seed, epoch_begin, epoch_end, n_epochs,
                       neg_rate, &dens, result_buffer, static_cast<hipStream_t>(stream));
}

extern "C" int wm_umap_label_intersect(const int32_t* indptr, const int32_t* indices, const float* data, const int32_t* labels,
                                       int n, double f_far, double f_unk, float* out, double* workspace, void* stream) {
  WM_REQUIRE(indptr && indices && data && labels && out && workspace && out != data, WM_EINVAL);
  WM_REQUIRE(n > 0 && f_far >= 0.0 && f_far <= 1.0 && f_unk >= 0.0 && f_unk <= 1.0, WM_EINVAL);
  WM_REQUIRE(n <= (1 << 24), WM_EUNSUPPORTED);
  WM_REQUIRE(((uintptr_t)workspace & 7u) == 0, WM_EALIGN);
  hipStream_t st = static_cast<hipStream_t>(stream);
  umap_label_max_kernel<<<wm_cdiv(n, UM_THREADS), UM_THREADS, 0, st>>>(indptr, indices, data, labels, n, f_far, f_unk, workspace);
  WM_LAUNCH_CHECK();
  umap_label_intersect_kernel<<<wm_cdiv(n, UM_THREADS), UM_THREADS, 0, st>>>(indptr, indices, data, labels, n, f_far, f_unk,
                                                                            workspace, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_umap_smooth_knn_query(const float* dist, int m, int k, const double* mean_dist, float* sigma, float* weights,
                                        void* stream) {
  WM_REQUIRE(dist && mean_dist && sigma && weights, WM_EINVAL);
  WM_REQUIRE(m > 0 && k > 0, WM_EINVAL);
  WM_REQUIRE(k <= 64 && m <= (1 << 24), WM_EUNSUPPORTED);
  umap_smooth_knn_query_kernel<<<wm_cdiv(m, UM_THREADS), UM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(dist, m, k, mean_dist,
                                                                                                         sigma, weights);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_umap_transform_layout(const float* y_in, float* y_out, const float* y_train, const int32_t* idx,
                                        const uint32_t* q, int m, int n, int k, int dim, double a, double b, double gamma,
                                        double learning_rate, uint32_t seed, int epoch_begin, int epoch_end, int n_epochs,
                                        int neg_rate, void* stream) {
  WM_REQUIRE(y_in && y_out && y_train && idx && q && y_out != y_train, WM_EINVAL);
  WM_REQUIRE(m > 0 && n > 0 && k > 0, WM_EINVAL);
  if (const int rc = um_check_layout(dim, a, b, gamma, learning_rate, epoch_begin, epoch_end, n_epochs, neg_rate)) return rc;
  WM_REQUIRE(k <= 64 && m <= (1 << 24) && n <= (1 << 24), WM_EUNSUPPORTED);
  UmTransformArgs p = {};
  p.y_in = y_in;
  p.y_out = y_out;
  p.y_train = y_train;
  p.idx = idx;
  p.q = q;
  p.m = m;
  p.n = n;
  p.k = k;
  um_fill_force(p, dim, neg_rate, a, b, gamma);
  p.seed = seed;
  p.ep_begin = epoch_begin;
  p.ep_end = epoch_end;
  p.lr4 = learning_rate / 4.0;
  p.n_epochs = (double)n_epochs;
  hipStream_t st = static_cast<hipStream_t>(stream);
  um_with_dp(dim, [&](auto dp) {
    umap_transform_kernel<decltype(dp)::value><<<wm_cdiv(m, UM_THREADS / 64), UM_THREADS, 0, st>>>(p);
  });
  WM_LAUNCH_CHECK();
  return WM_OK;
}
