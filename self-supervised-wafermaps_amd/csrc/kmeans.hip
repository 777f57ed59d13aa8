// KMeans on the embedding matrix (cluster.KMeans; the reference's sklearn.cluster.KMeans(n_clusters=k) of notebook
// 1.0-Preprocess-WM811K): everything around the assignment pass.  The assignment itself is wm_group_min_dist
// (cluster.hip) on the centres of R restarts laid out as R groups of k columns -- one pass over the rows assigns them for
// all restarts -- and is not repeated here.
//   wm_kmeans_update   from the rows and the (column, distance) pairs that pass wrote: per restart and cluster the member
//                      count and the new centre, per restart the inertia, the number of changed rows and the squared
//                      centre shift;
//   wm_kmeans_seed     greedy k-means++ seeding driven by a host-drawn table of uniforms.
//
// ---- the update.  Definition: centre = the float64 sum of the members' float32 rows, divided in double by the count,
// rounded to float32 once.  No floating-point atomics and none on global memory, so every cell of every floating-point
// sum has ONE writer and a fixed order (the member counts are integer adds in LDS, whose sum has no order to depend on):
//   km_partial  a workgroup is ONE wave and owns (restart r, slab s of rows, 64-feature chunk, tile of KM_KT clusters).
//               Lane l owns feature 64 * chunk + l and walks the slab's rows in row order; the row's cluster c is the same
//               for the whole wave, so the branch on it is a scalar one, and the lane adds its float to the LDS cell
//               acc[c][l] (double).  No two lanes share a cell and one lane meets its cells in row order: the order of
//               the sum is the row order whatever the machine does.  A step is 64 rows: lane l fetches the label of row
//               i + l with ONE vector load, requested a step ahead, and a row's label reaches the wave by v_readlane; the
//               row fragments come in batches of eight, the next batch requested before the current one is added.  What was
//               measured on the way (12 449 x 512, k = 50, update per call at R = 1 / R = 10): one label per row at a
//               wave-uniform address, eight rows a step: 0.131 / 0.602 ms -- hipcc makes those scalar loads with a wait
//               and a branch per row, and `live ? x[..] : 0` a branch around every row load with vmcnt(0) behind it; the
//               same with the next steps requested early: 0.074 / 0.290 ms; this form, with no per-lane branch around a
//               load (a lane behind d reads feature d - 1 into a cell nobody stores, a row of another tile or behind the
//               slab reads the slab's first row, an L1 hit, and adds nothing): 0.036 / 0.119 ms (profiles/kmeans.md).  The
//               chain that remains is LDS read -> v_add_f64 -> LDS write per row, which the resident waves overlap.
//               Why the reads coalesce: the 64 lanes of a row step read 64 consecutive floats, one aligned 256-byte
//               segment of the row (rows are 16-byte aligned and a chunk starts at a multiple of 256 bytes from the row's
//               start); with d % 64 != 0 the last chunk's tail lanes repeat feature d - 1.  A row is read by exactly one cluster tile
//               (the one its cluster is in) and once per restart: the algorithmic bytes are R * n * d * 4 plus the pairs.
//               LDS budget against the CU's 160 KB: acc is kt * 64 * 8 bytes plus 512 for the lanes' inertia and kt
//               counters, kt = min(k, KM_KT): 13 KB at k = 25 (12 workgroups per CU), 26 KB at k = 50 (6 per CU), 49 KB at
//               the cap KM_KT = 96 (3 per CU).  k * 64 * 8 bytes stops fitting one workgroup at k = 320 and would leave one wave per CU long before
//               that, so a k above 96 is cut into ceil(k / 96) cluster tiles: each tile's workgroup walks the slab's labels
//               again (4 bytes per row) and loads only the rows of its own clusters, so the row traffic does not grow.
//               The chunk-0 workgroups also count their clusters' members (ds_add_u32 on an LDS counter per cluster, 64
//               rows per instruction) and the tile-0 one of them adds the slab's (double)dist^2 -- lane l the rows l,
//               l + 64, ... of the slab in order, then the 64 lane sums in lane order -- and counts the rows that changed.
//               The slabs: S = min(ceil(512 / (chunks * tiles)), ceil(n / 64)) slabs of ceil(n / S) rows -- a function of
//               (n, d, k) and of nothing else.  NOT of R: a restart must give the same bits alone and among others, and
//               not of the device: the bits must not depend on the free CU count.  512 * R one-wave workgroups fill the
//               256 CUs from R = 1 on, and the partial sums stay small (S * R * k * d * 8 bytes: 13 MB per restart at
//               k = 50, d = 512).
//   km_fold     a thread per (restart, cluster, feature) adds the S partial sums in slab order, divides and rounds, keeps
//               the old centre where the count is 0, and the 256 squared moves of a workgroup are added in a fixed tree
//               (block_tree_sum, f64.h).
//   km_finish   a workgroup per restart adds the slabs' inertia and changed counts and the fold's shift partials: thread t
//               takes the values t, t + 256, ... in index order and the 256 sums go through the same fixed tree.
//
// ---- the seeding.  Per new centre seven small launches chained on the stream, no host round trip (the host has drawn
// the uniforms before):
//   km_seed_scan     closest2's running sums inside blocks of 256 rows (a fixed-order scan in LDS) and the block sums;
//   km_seed_offsets  one workgroup: the blocks' exclusive offsets in block order, pot, and the thresholds u * pot;
//   km_seed_pick     per block and trial the first row with closest2 > 0 whose running sum exceeds the threshold;
//   km_seed_cands    one workgroup: the lowest such row over the blocks (none: the last row with closest2 > 0; pot == 0:
//                    row min(floor(u * n), n - 1));
//   km_seed_eval     a thread per (row, trial): the library's one distance function (cl_dist.h: float32, index order) to
//                    the candidate, squared in double, min with closest2 -> the trial's plane of minima; the block's sum;
//   km_seed_commit   one workgroup: every trial's potential (block sums in block order), the winner (lowest potential,
//                    then lowest t), the outputs of the step;
//   km_seed_apply    closest2 <- the winner's plane; the winner's row -> the centre.
// In km_seed_eval a thread reads its own row front to back (float4 steps; its 64-byte lines stay in L1 / L2 for the three
// steps that follow) because the distance must be the in-order float32 accumulation every other kernel here returns for
// the pair; the candidate's row is the same address in every lane (a broadcast).
#include <limits.h>

#include "cl_dist.h"
#include "f64.h"

namespace {

constexpr int KM_MAX_N = 1 << 24;
constexpr int KM_MAX_K = 1 << 16;
constexpr int KM_MAX_R = 1024;
constexpr int KM_KT = 96;        // clusters per tile of the update (LDS: KM_KT * 64 doubles + KM_KT counters)
constexpr int KM_TARGET = 512;   // workgroups per restart the slab count aims at
constexpr int KM_ROWS = 8;       // rows per batch of km_partial (two batches in flight; 64 % (2 * KM_ROWS) == 0)
constexpr int KM_BLOCK = 256;    // threads of the fold and seeding kernels; rows per seeding block
constexpr int KM_MAX_T = 16;

struct KmShape {
  int chunks, tiles, kta, slabs, rows_per_slab, fold_blocks;
};
inline bool km_shape_ok(int n, int d, int k, int R) {
  return n > 0 && n <= KM_MAX_N && d > 0 && d % 4 == 0 && d <= 1024 && k > 0 && k <= KM_MAX_K && R > 0 && R <= KM_MAX_R;
}
inline KmShape km_shape(int n, int d, int k) {
  KmShape s;
  s.chunks = (d + 63) / 64;
  s.tiles = (k + KM_KT - 1) / KM_KT;
  s.kta = k < KM_KT ? k : KM_KT;
  int want = (KM_TARGET + s.chunks * s.tiles - 1) / (s.chunks * s.tiles);
  const int most = (n + 63) / 64;
  if (want > most) want = most;
  if (want < 1) want = 1;
  s.rows_per_slab = (n + want - 1) / want;
  s.slabs = (n + s.rows_per_slab - 1) / s.rows_per_slab;
  s.fold_blocks = (int)(((long long)k * d + KM_BLOCK - 1) / KM_BLOCK);
  return s;
}
inline size_t km_align(size_t b) { return (b + 255) & ~(size_t)255; }
struct KmUpdateWs {
  size_t psum, pcnt, pin, pch, pshift, total;
};
inline KmUpdateWs km_update_ws(const KmShape& s, int d, int k, int R) {
  KmUpdateWs w;
  size_t at = 0;
  w.psum = at, at += km_align((size_t)R * s.slabs * k * d * sizeof(double));
  w.pcnt = at, at += km_align((size_t)R * s.slabs * k * sizeof(int));
  w.pin = at, at += km_align((size_t)R * s.slabs * sizeof(double));
  w.pch = at, at += km_align((size_t)R * s.slabs * sizeof(int));
  w.pshift = at, at += km_align((size_t)R * s.fold_blocks * sizeof(double));
  w.total = at;
  return w;
}

__global__ __launch_bounds__(64) void km_partial(const float* __restrict__ x, const int* __restrict__ assign,
                                                 const float* __restrict__ dist, const int* __restrict__ prev, int n, int d,
                                                 int k, int R, int rows_per_slab, int tiles, int kta,
                                                 double* __restrict__ psum, int* __restrict__ pcnt, double* __restrict__ pin,
                                                 int* __restrict__ pch) {
  extern __shared__ double km_lds[];  // acc [kta][64] doubles, red [64] doubles, then cnt [kta] ints
  double* acc = km_lds;
  double* red = km_lds + (size_t)kta * 64;
  int* cnt = reinterpret_cast<int*>(red + 64);
  const int lane = threadIdx.x;
  const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
  const int s = blockIdx.y, S = gridDim.y, r = blockIdx.z;
  const int c0 = tile * KM_KT;
  const int ktn = min(KM_KT, k - c0);  // (<= kta)
  for (int c = 0; c < ktn; ++c) acc[c * 64 + lane] = 0.0;
  for (int c = lane; c < ktn; c += 64) cnt[c] = 0;
  __syncthreads();
  const int f = chunk * 64 + lane;
  const bool live = f < d;
  const int fe = live ? f : d - 1;  // (a lane behind d reads the last feature and adds it to a cell nobody stores: no branch)
  const bool counts_here = chunk == 0, stats_here = chunk == 0 && tile == 0;
  const int i0 = s * rows_per_slab, i1 = min(n, i0 + rows_per_slab);
  const unsigned base = (unsigned)(r * k + c0);
  double inertia = 0.0;
  int changed = 0;
  // A step is 64 rows.  Lane l fetches the label of row i + l (ONE vector load per step, requested a step ahead; a load
  // of one label per row at a wave-uniform address becomes a scalar load with a wait and a branch per row), and the
  // label of a row reaches the whole wave by v_readlane.  The row fragments come in batches of KM_ROWS, the next batch
  // requested before the current one is added.  A row of another cluster tile (or behind the slab) fetches the slab's
  // first row instead -- an L1 hit, no branch around the load -- and adds nothing.
  auto label_of = [&](int i) {  // the cluster of row i + lane inside this tile; anything outside [0, ktn): not here
    // (the row clamped and the result masked to -1 behind the slab, not selected: hipcc turns a select back into a branch
    // around the load, with a wait at its end)
    const int a = assign[(size_t)min(i + lane, i1 - 1) * R + r];
    return (int)((unsigned)a - base) | -(int)(i + lane >= i1);
  };
  auto fetch = [&](float (&v)[KM_ROWS], int i, int lab, int l0) {  // rows i + l0 + u: their labels sit in lanes l0 + u
#pragma unroll
    for (int u = 0; u < KM_ROWS; ++u) {
      const int c = __builtin_amdgcn_readlane(lab, l0 + u);
      const int row = (unsigned)c < (unsigned)ktn ? i + l0 + u : i0;
      v[u] = x[(size_t)row * d + fe];
    }
  };
  auto add = [&](const float (&v)[KM_ROWS], int lab, int l0) {
#pragma unroll
    for (int u = 0; u < KM_ROWS; ++u) {
      const int c = __builtin_amdgcn_readlane(lab, l0 + u);
      if ((unsigned)c < (unsigned)ktn) acc[c * 64 + lane] += (double)v[u];  // (uniform over the wave: a scalar branch)
    }
  };
  int lab = label_of(i0);
  for (int i = i0; i < i1; i += 64) {
    const int lab_next = label_of(i + 64);
    if (counts_here && (unsigned)lab < (unsigned)ktn) atomicAdd(&cnt[lab], 1);  // (integers, in LDS: no order to depend on)
    if (stats_here) {  // lane l: rows i0 + l, i0 + l + 64, ... in order
      const size_t at = (size_t)min(i + lane, i1 - 1) * R + r;
      const bool in = i + lane < i1;
      const double t = in ? (double)dist[at] : 0.0;
      inertia += t * t;
      const int was = prev ? prev[at] : ~assign[at];
      changed += in && was != assign[at] ? 1 : 0;
    }
    float va[KM_ROWS], vb[KM_ROWS];
    fetch(va, i, lab, 0);
#pragma unroll
    for (int b = 0; b < 64 / KM_ROWS; b += 2) {
      if (i + b * KM_ROWS >= i1) break;
      fetch(vb, i, lab, (b + 1) * KM_ROWS);
      add(va, lab, b * KM_ROWS);
      if (b + 2 < 64 / KM_ROWS) fetch(va, i, lab, (b + 2) * KM_ROWS);
      add(vb, lab, (b + 1) * KM_ROWS);
    }
    lab = lab_next;
  }
  __syncthreads();
  const size_t slot = (size_t)r * S + s;
  if (live)
    for (int c = 0; c < ktn; ++c) psum[(slot * k + c0 + c) * d + f] = acc[c * 64 + lane];
  if (counts_here)
    for (int c = lane; c < ktn; c += 64) pcnt[slot * k + c0 + c] = cnt[c];
  if (stats_here) {  // the 64 lane sums in lane order
    red[lane] = inertia;
    __syncthreads();
    if (lane == 0) {
      double tot = 0.0;
      for (int l = 0; l < 64; ++l) tot += red[l];
      pin[slot] = tot;
    }
    for (int w = 32; w > 0; w >>= 1) changed += __shfl_xor(changed, w);
    if (lane == 0) pch[slot] = changed;
  }
}

__global__ __launch_bounds__(KM_BLOCK) void km_fold(const double* __restrict__ psum, const int* __restrict__ pcnt, int S,
                                                    int k, int d, const float* __restrict__ old, float* __restrict__ out,
                                                    int* __restrict__ counts, double* __restrict__ pshift) {
  __shared__ double sh[KM_BLOCK];
  const int r = blockIdx.y;
  const long long e = (long long)blockIdx.x * KM_BLOCK + threadIdx.x;
  double sq = 0.0;
  if (e < (long long)k * d) {
    const int c = (int)(e / d);
    double sum = 0.0;
    int cn = 0;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
      sum += psum[((size_t)r * S + s) * k * d + e];
      cn += pcnt[((size_t)r * S + s) * k + c];
    }
    const float was = old[(size_t)r * k * d + e];
    const float now = cn > 0 ? (float)(sum / (double)cn) : was;
    out[(size_t)r * k * d + e] = now;
    if (e - (long long)c * d == 0) counts[(size_t)r * k + c] = cn;
    const double mv = (double)now - (double)was;
    sq = mv * mv;
  }
  const double tot = block_tree_sum<KM_BLOCK>(sq, sh);
  if (threadIdx.x == 0) pshift[(size_t)r * gridDim.x + blockIdx.x] = tot;
}

// One workgroup per restart: thread t adds the values t, t + 256, ... in index order, then the 256 sums go through the
// fixed tree (the loads run side by side; one thread walking a list of global values pays a latency per value).
__global__ __launch_bounds__(KM_BLOCK) void km_finish(const double* __restrict__ pin, const int* __restrict__ pch,
                                                      const double* __restrict__ pshift, int S, int fold_blocks,
                                                      double* __restrict__ inertia, int* __restrict__ n_changed,
                                                      double* __restrict__ shift2) {
  __shared__ double sh[KM_BLOCK];
  const int r = blockIdx.x, t = threadIdx.x;
  double in = 0.0, ch = 0.0, sf = 0.0;  // (the changed counts are integers below 2^53: exact in double)
  for (int s = t; s < S; s += KM_BLOCK) {
    in += pin[(size_t)r * S + s];
    ch += (double)pch[(size_t)r * S + s];
  }
  for (int b = t; b < fold_blocks; b += KM_BLOCK) sf += pshift[(size_t)r * fold_blocks + b];
  in = block_tree_sum<KM_BLOCK>(in, sh);
  ch = block_tree_sum<KM_BLOCK>(ch, sh);
  sf = block_tree_sum<KM_BLOCK>(sf, sh);
  if (t == 0) {
    inertia[r] = in;
    n_changed[r] = (int)ch;
    shift2[r] = sf;
  }
}

// ------------------------------------------------------------------------------------------------ seeding

struct KmSeedWs {
  size_t c2, scan, planes, bsum, boff, bpot, bcand, thr, pot, cand, winner, total;
};
inline KmSeedWs km_seed_ws(int n, int T) {
  const size_t nb = (size_t)(n + KM_BLOCK - 1) / KM_BLOCK;
  KmSeedWs w;
  size_t at = 0;
  w.c2 = at, at += km_align((size_t)n * 8);
  w.scan = at, at += km_align((size_t)n * 8);
  w.planes = at, at += km_align((size_t)T * n * 8);
  w.bsum = at, at += km_align(nb * 8);
  w.boff = at, at += km_align(nb * 8);
  w.bpot = at, at += km_align((size_t)T * nb * 8);
  w.bcand = at, at += km_align((size_t)(T + 1) * nb * 4);
  w.thr = at, at += km_align((size_t)T * 8);
  w.pot = at, at += km_align(8);
  w.cand = at, at += km_align((size_t)T * 4);
  w.winner = at, at += km_align(4);
  w.total = at;
  return w;
}

// One workgroup: the sum of v[0 .. count) in index order up to a fixed blocking -- thread t adds its run of
// ceil(count / KM_BLOCK) consecutive values in order, thread 0 adds the KM_BLOCK run sums in order.  With `off` the
// exclusive offsets are stored too (off[i] = the total before i: the sum of the runs before i's, plus i's own run up to i).
__device__ __forceinline__ double km_ordered_sum(const double* __restrict__ v, int count, double* __restrict__ off,
                                                 double* sh) {
  const int t = threadIdx.x;
  const int run = (count + KM_BLOCK - 1) / KM_BLOCK;
  const int b0 = min(count, t * run), b1 = min(count, b0 + run);
  double mine = 0.0;
  for (int b = b0; b < b1; ++b) mine += v[b];
  sh[t] = mine;
  __syncthreads();
  if (t == 0) {
    double at = 0.0;
    for (int q = 0; q < KM_BLOCK; ++q) {
      const double next = at + sh[q];
      sh[q] = at;
      at = next;
    }
    sh[KM_BLOCK] = at;
  }
  __syncthreads();
  const double total = sh[KM_BLOCK];
  if (off) {
    double at = sh[t];
    for (int b = b0; b < b1; ++b) {
      off[b] = at;
      at += v[b];
    }
  }
  __syncthreads();
  return total;
}

__device__ __forceinline__ int km_uniform_row(double u, int n) {
  const long long i = (long long)floor(u * (double)n);
  return (int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i));
}

__global__ __launch_bounds__(KM_BLOCK) void km_seed_scan(const double* __restrict__ c2, int n, double* __restrict__ scan,
                                                         double* __restrict__ bsum) {
  __shared__ double sh[2][KM_BLOCK];
  const int t = threadIdx.x, i = blockIdx.x * KM_BLOCK + t;
  int cur = 0;
  sh[0][t] = i < n ? c2[i] : 0.0;
  __syncthreads();
  for (int w = 1; w < KM_BLOCK; w <<= 1) {  // (inclusive scan, the same tree for every block)
    sh[cur ^ 1][t] = t >= w ? sh[cur][t - w] + sh[cur][t] : sh[cur][t];
    cur ^= 1;
    __syncthreads();
  }
  if (i < n) scan[i] = sh[cur][t];
  if (t == KM_BLOCK - 1) bsum[blockIdx.x] = sh[cur][t];
}

__global__ __launch_bounds__(KM_BLOCK) void km_seed_offsets(const double* __restrict__ bsum, int nb, const double* __restrict__ u,
                                                            int T, double* __restrict__ boff, double* __restrict__ pot,
                                                            double* __restrict__ thr) {
  __shared__ double sh[KM_BLOCK + 1];
  const double total = km_ordered_sum(bsum, nb, boff, sh);
  if (threadIdx.x == 0) *pot = total;
  if (threadIdx.x < T) thr[threadIdx.x] = u[threadIdx.x] * total;
}

// bcand [T + 1][nb]: per trial the block's first row behind the threshold (INT_MAX: none); plane T: the block's last row
// with closest2 > 0 (-1: none).
__global__ __launch_bounds__(KM_BLOCK) void km_seed_pick(const double* __restrict__ c2, const double* __restrict__ scan,
                                                         const double* __restrict__ boff, const double* __restrict__ thr, int n,
                                                         int T, int* __restrict__ bcand) {
  __shared__ int sh[KM_BLOCK];
  const int t = threadIdx.x, i = blockIdx.x * KM_BLOCK + t, nb = gridDim.x;
  const bool pos = i < n && c2[i] > 0.0;
  const double running = i < n ? boff[blockIdx.x] + scan[i] : 0.0;
  for (int q = 0; q <= T; ++q) {
    int v;
    if (q < T) v = pos && running > thr[q] ? i : INT_MAX;
    else v = pos ? -i : 1;  // (the minimum of -i is the last row)
    sh[t] = v;
    __syncthreads();
    for (int w = KM_BLOCK / 2; w > 0; w >>= 1) {
      if (t < w) sh[t] = min(sh[t], sh[t + w]);
      __syncthreads();
    }
    if (t == 0) bcand[(size_t)q * nb + blockIdx.x] = q < T ? sh[0] : (sh[0] > 0 ? -1 : -sh[0]);
    __syncthreads();
  }
}

// One workgroup.  first: centre 0, the row of u[0] whatever closest2 holds (one candidate).
__global__ __launch_bounds__(KM_BLOCK) void km_seed_cands(const int* __restrict__ bcand, int nb, const double* __restrict__ pot,
                                                          const double* __restrict__ u, int n, int T, int first,
                                                          int* __restrict__ cand) {
  __shared__ int sh[KM_BLOCK];
  const int t = threadIdx.x;
  if (first || *pot == 0.0) {
    if (t < T) cand[t] = km_uniform_row(u[t], n);
    return;
  }
  int last = -1;
  for (int q = T; q >= 0; --q) {  // (plane T first: the fall-back row)
    int v = q < T ? INT_MAX : -1;
    for (int b = t; b < nb; b += KM_BLOCK) {
      const int w = bcand[(size_t)q * nb + b];
      v = q < T ? min(v, w) : max(v, w);
    }
    sh[t] = v;
    __syncthreads();
    for (int w = KM_BLOCK / 2; w > 0; w >>= 1) {
      if (t < w) sh[t] = q < T ? min(sh[t], sh[t + w]) : max(sh[t], sh[t + w]);
      __syncthreads();
    }
    if (q == T) last = sh[0];
    else if (t == 0) cand[q] = sh[0] != INT_MAX ? sh[0] : (last >= 0 ? last : km_uniform_row(u[q], n));
    __syncthreads();
  }
}

// grid (nb, T).  c2 == nullptr: no centre yet (the minima are the squared distances themselves).
__global__ __launch_bounds__(KM_BLOCK) void km_seed_eval(const float* __restrict__ x, int n, int d, const double* __restrict__ c2,
                                                         const int* __restrict__ cand, double* __restrict__ planes,
                                                         double* __restrict__ bpot) {
  __shared__ double sh[KM_BLOCK];
  const int t = threadIdx.x, i = blockIdx.x * KM_BLOCK + t, q = blockIdx.y, nb = gridDim.x;
  const int j = cand[q];
  double m = 0.0;
  if (i < n && j >= 0 && j < n) {
    const float4* __restrict__ a = reinterpret_cast<const float4*>(x + (size_t)i * d);
    const float4* __restrict__ b = reinterpret_cast<const float4*>(x + (size_t)j * d);
    float acc = 0.0f;
    for (int f = 0; f < d / 4; ++f) {
      const float4 p = a[f], w = b[f];
      acc = cl_accum<0>(p.x, w.x, acc);
      acc = cl_accum<0>(p.y, w.y, acc);
      acc = cl_accum<0>(p.z, w.z, acc);
      acc = cl_accum<0>(p.w, w.w, acc);
    }
    const double dist = (double)cl_finish<0>(acc);
    m = dist * dist;
    if (c2) m = fmin(m, c2[i]);
    planes[(size_t)q * n + i] = m;
  }
  const double tot = block_tree_sum<KM_BLOCK>(m, sh);
  if (t == 0) bpot[(size_t)q * nb + blockIdx.x] = tot;
}

// One workgroup: the trials' potentials, the winner, the step's outputs (step = the centre's number).
__global__ __launch_bounds__(KM_BLOCK) void km_seed_commit(const double* __restrict__ bpot, int nb, const int* __restrict__ cand,
                                                           int T, int T_all, int step, int* __restrict__ winner,
                                                           int* __restrict__ idx, int* __restrict__ out_cand,
                                                           double* __restrict__ out_pots) {
  __shared__ double sh[KM_BLOCK + 1];
  __shared__ double pots[KM_MAX_T];
  for (int q = 0; q < T; ++q) {
    const double p = km_ordered_sum(bpot + (size_t)q * nb, nb, nullptr, sh);
    if (threadIdx.x == 0) pots[q] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int q = 1; q < T; ++q)
      if (pots[q] < pots[best]) best = q;
    *winner = best;
    idx[step] = cand[best];
    for (int q = 0; q < T_all; ++q) {
      if (out_cand) out_cand[(size_t)step * T_all + q] = q < T ? cand[q] : -1;
      if (out_pots) out_pots[(size_t)step * T_all + q] = q < T ? pots[q] : (double)INFINITY;
    }
  }
}

// grid nb + copy blocks: closest2 <- the winner's plane; the trailing blocks copy the winner's row into the centre.
__global__ __launch_bounds__(KM_BLOCK) void km_seed_apply(const float* __restrict__ x, int n, int d, const double* __restrict__ planes,
                                                          const int* __restrict__ winner, const int* __restrict__ cand, int nb,
                                                          double* __restrict__ c2, float* __restrict__ centre) {
  const int q = *winner;
  if ((int)blockIdx.x < nb) {
    const int i = blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i < n) c2[i] = planes[(size_t)q * n + i];
    return;
  }
  const int j = cand[q];
  const int f = (blockIdx.x - nb) * KM_BLOCK + threadIdx.x;
  if (f < d && j >= 0 && j < n) centre[f] = x[(size_t)j * d + f];
}

}  // namespace

extern "C" size_t wm_kmeans_update_workspace_bytes(int n, int d, int k, int R) {
  if (!km_shape_ok(n, d, k, R)) return 0;
  return km_update_ws(km_shape(n, d, k), d, k, R).total;
}

extern "C" int wm_kmeans_update(const float* x, int n, int d, const int32_t* assign, const float* dist, const int32_t* prev,
                                int R, int k, const float* centres_old, float* centres_new, int32_t* counts, double* inertia,
                                int32_t* n_changed, double* shift2, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && assign && dist && centres_old && centres_new && counts && inertia && n_changed && shift2 && workspace,
             WM_EINVAL);
  WM_REQUIRE(n > 0 && d > 0 && k > 0 && R > 0 && centres_old != centres_new, WM_EINVAL);
  WM_REQUIRE(km_shape_ok(n, d, k, R) && (long long)R * k <= INT_MAX, WM_EUNSUPPORTED);
  WM_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(inertia) & 7) == 0 && (reinterpret_cast<uintptr_t>(shift2) & 7) == 0,
             WM_EALIGN);
  const KmShape s = km_shape(n, d, k);
  const KmUpdateWs w = km_update_ws(s, d, k, R);
  WM_REQUIRE(workspace_bytes >= w.total, WM_EWORKSPACE);
  WM_REQUIRE((long long)s.chunks * s.tiles <= INT_MAX && s.slabs <= 65535 && s.fold_blocks >= 1, WM_EUNSUPPORTED);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  double* psum = reinterpret_cast<double*>(ws + w.psum);
  int* pcnt = reinterpret_cast<int*>(ws + w.pcnt);
  double* pin = reinterpret_cast<double*>(ws + w.pin);
  int* pch = reinterpret_cast<int*>(ws + w.pch);
  double* pshift = reinterpret_cast<double*>(ws + w.pshift);
  const size_t lds = ((size_t)s.kta + 1) * 64 * sizeof(double) + (size_t)s.kta * sizeof(int);
  km_partial<<<dim3(s.chunks * s.tiles, s.slabs, R), 64, lds, st>>>(x, assign, dist, prev, n, d, k, R, s.rows_per_slab, s.tiles,
                                                                   s.kta, psum, pcnt, pin, pch);
  WM_LAUNCH_CHECK();
  km_fold<<<dim3(s.fold_blocks, R), KM_BLOCK, 0, st>>>(psum, pcnt, s.slabs, k, d, centres_old, centres_new, counts, pshift);
  WM_LAUNCH_CHECK();
  km_finish<<<R, KM_BLOCK, 0, st>>>(pin, pch, pshift, s.slabs, s.fold_blocks, inertia, n_changed, shift2);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_kmeans_seed_workspace_bytes(int n, int d, int k, int T) {
  if (!km_shape_ok(n, d, k, 1) || k > n || T < 1 || T > KM_MAX_T) return 0;
  return km_seed_ws(n, T).total;
}

extern "C" int wm_kmeans_seed(const float* x, int n, int d, int k, int T, const double* u, float* centres, int32_t* idx,
                              int32_t* cand, double* pots, void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(x && u && centres && idx && workspace, WM_EINVAL);
  WM_REQUIRE(n > 0 && d > 0 && k > 0 && k <= n && T >= 1, WM_EINVAL);
  WM_REQUIRE(km_shape_ok(n, d, k, 1) && T <= KM_MAX_T, WM_EUNSUPPORTED);
  WM_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(u) & 7) == 0 && (pots == nullptr || (reinterpret_cast<uintptr_t>(pots) & 7) == 0),
             WM_EALIGN);
  const KmSeedWs w = km_seed_ws(n, T);
  WM_REQUIRE(workspace_bytes >= w.total, WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  double* c2 = reinterpret_cast<double*>(ws + w.c2);
  double* scan = reinterpret_cast<double*>(ws + w.scan);
  double* planes = reinterpret_cast<double*>(ws + w.planes);
  double* bsum = reinterpret_cast<double*>(ws + w.bsum);
  double* boff = reinterpret_cast<double*>(ws + w.boff);
  double* bpot = reinterpret_cast<double*>(ws + w.bpot);
  int* bcand = reinterpret_cast<int*>(ws + w.bcand);
  double* thr = reinterpret_cast<double*>(ws + w.thr);
  double* pot = reinterpret_cast<double*>(ws + w.pot);
  int* cnd = reinterpret_cast<int*>(ws + w.cand);
  int* winner = reinterpret_cast<int*>(ws + w.winner);
  const int nb = (n + KM_BLOCK - 1) / KM_BLOCK;
  const int copy_blocks = (d + KM_BLOCK - 1) / KM_BLOCK;
  for (int c = 0; c < k; ++c) {
    const int Tc = c == 0 ? 1 : T;
    const double* uc = u + (size_t)c * T;
    if (c > 0) {
      km_seed_scan<<<nb, KM_BLOCK, 0, st>>>(c2, n, scan, bsum);
      WM_LAUNCH_CHECK();
      km_seed_offsets<<<1, KM_BLOCK, 0, st>>>(bsum, nb, uc, Tc, boff, pot, thr);
      WM_LAUNCH_CHECK();
      km_seed_pick<<<nb, KM_BLOCK, 0, st>>>(c2, scan, boff, thr, n, Tc, bcand);
      WM_LAUNCH_CHECK();
    }
    km_seed_cands<<<1, KM_BLOCK, 0, st>>>(bcand, nb, pot, uc, n, Tc, c == 0 ? 1 : 0, cnd);
    WM_LAUNCH_CHECK();
    km_seed_eval<<<dim3(nb, Tc), KM_BLOCK, 0, st>>>(x, n, d, c == 0 ? nullptr : c2, cnd, planes, bpot);
    WM_LAUNCH_CHECK();
    km_seed_commit<<<1, KM_BLOCK, 0, st>>>(bpot, nb, cnd, Tc, T, c, winner, idx, cand, pots);
    WM_LAUNCH_CHECK();
    km_seed_apply<<<nb + copy_blocks, KM_BLOCK, 0, st>>>(x, n, d, planes, winner, cnd, nb, c2, centres + (size_t)c * d);
    WM_LAUNCH_CHECK();
  }
  return WM_OK;
}
