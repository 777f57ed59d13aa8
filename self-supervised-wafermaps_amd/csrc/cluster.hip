// All-pairs distance kernels of the embedding-clustering flow (reference notebooks 3.1-Embeddings-clustering and
// 3.2-Embeddings-SSL-categories: HDBSCAN on the dumped embedding matrix, scored by silhouette):
//   wm_core_distance      k-th smallest distance of every row (the HDBSCAN core distance, self included);
//   wm_mreach_min_edge    one Boruvka round on the mutual-reachability graph: per row the lightest edge that
//                         leaves the row's component;
//   wm_cluster_dist_sums  per row the sum of its distances to the members of every cluster (silhouette);
//   wm_knn_graph          the k nearest rows of every row with their indices, ordered by (distance, index), the row
//                         itself among its candidates (the exact kNN graph that manifold.UMAP starts from);
//   wm_knn_query          the same for the rows of a second matrix against x (the rectangular form that the transform of
//                         new rows starts from): cl_pairs takes its rows from a row operand of its own (xr, nr), which
//                         every square mode sets to (x, n);
//   wm_mreach_query       for the rows of a second matrix the row of x nearest in mutual reachability
//                         max(core_q[i], core[c], dist * inv_alpha), equal weights resolved by the plain distance and then
//                         by the index (what HDBSCAN's prediction for new rows starts from);
//   wm_group_min_dist     for the rows of a second matrix, per group of columns (runs of equal group ids: the exemplars
//                         of one cluster) the nearest column and its distance (what HDBSCAN's soft clustering starts
//                         from);
//   wm_allpoints_core, wm_mreach_min_edge_grouped, wm_group_min_mreach
//                         the three all-pairs parts of DBCV (density-based cluster validity) on rows sorted by cluster:
//                         the all-points core distance (a power mean of a row's distances inside its own cluster), one
//                         Boruvka round of every cluster's own mutual-reachability tree at once, and the group min with
//                         the mutual reachability in place of the plain distance (the clusters' separations);
//   wm_pair_dist          the distances of listed pairs, out[i][q] = dist(xq[i], x[idx[i][q]]): a gather kernel of its own
//                         (cl_pair_dist, a thread per pair) that calls the same cl_accum / cl_finish over the features in
//                         index order, so a pair has the bits the tile pass gives it (the tile pass only adds the exact
//                         zeros of the padding behind d);
//   wm_rank_query         for the rows of a second matrix and k thresholds (t, tj) per row the number of columns l before
//                         each threshold in the row's (distance, index) order -- the rank primitive of trustworthiness and
//                         continuity (manifold.py); integer results.
//
// ONE distance function serves all of them (cl_accum / cl_finish, cl_dist.h): the float32 differences a_k - b_k are
// accumulated in float32 in index order k = 0, 1, ..., d-1 in a single accumulator (Euclidean: fma(t, t, acc), then a
// correctly rounded square root; Manhattan: acc + |t|).  Not ||a||^2 + ||b||^2 - 2ab: wafer embeddings contain
// near-duplicates, whose distance that form cancels away.  Two properties the host code and the tests rely on:
//   (1) dist(i, j) and dist(j, i) are the same bits: a - b = -(b - a) exactly, t * t and |t| do not see the sign, and
//       both directions add the same terms in the same order.  (Zero padding of the feature dimension adds exact
//       zeros.)  So an edge has ONE weight whichever endpoint finds it, which Boruvka needs.
//   (2) the relative error against the exact distance of the float32 rows is at most (d + 3) * 2^-24 (first order):
//       one rounding per difference (twice in the square), one per accumulation step (d for the fused
//       multiply-adds, d - 1 for the Manhattan additions), halved by the square root, plus the root's own rounding:
//       Euclidean (d + 2) / 2 + 1, Manhattan d.  Equal rows give t = 0 in every term: the distance is exactly 0.
//
// Shape of the work: a register-tiled all-pairs pass on the float32 VALU (no MFMA: the distance is not a product).
// A workgroup of 256 threads owns 16 * TM rows i and walks 64-row column tiles j; both row sets are staged in LDS in
// chunks of 32 features ([row][36] floats: the 16 rows a wave reads with one ds_read_b128 start 36 dwords apart, on
// 16 distinct 4-bank slots); thread (ty, tx) accumulates the TM x 4 pairs (ty + 16 r, tx + 16 c).  The next chunk is
// fetched into registers while the current one is consumed.  Per column tile the mode's epilogue runs:
//   core      distances -> LDS tile; one owner thread per row inserts those below its current k-th into the row's
//             sorted k-list (LDS; after the first tiles an insertion is rare);
//   knn       the same with the column index carried next to the distance; a slice scans its columns in ascending
//             order and a candidate goes behind its equals, so a list is ordered by (distance, index);
//   min edge  every thread keeps the best (w, j) of its TM rows in registers; one LDS reduction at the end;
//   query     the same without the component filter and with the plain distance carried between w and j;
//   sums      distances -> LDS tile; the row's owner adds them in column order, in double, and flushes the running sum
//             to out[i][label] whenever the label changes (rows sorted by label: once per cluster);
//   group min the sums shape with a running (best distance, its column) in place of the running sum: distances -> LDS
//             tile; the row's owner scans the 64 columns in ascending order (a later column replaces the best only when
//             strictly nearer: the lowest index wins a tie) and, when the group id changes, stores the finished group's
//             pair and +inf / -1 for the ids it skipped.  Group ids do not decrease, so every out[i][c] is stored
//             exactly once: no memset.  What was chosen and why: the work is m rows (12 k .. 811 k) against a few
//             hundred to a few thousand columns, so the rows carry the parallelism.  TM = 4 (64-row tiles, 35 KB of
//             LDS, four workgroups per CU): the owners are then exactly one full wave, the LDS array stays far from
//             its limit (8 ds_read_b128 = 32 LDS cycles per wave against 128 VALU instructions = 512 cycles per 4
//             features), and 12 449 rows give 195 row tiles.  That alone would leave CUs idle, so the columns are cut
//             into slices as in the other modes (about a thousand workgroups in all, but at most 16 slices: the
//             workspace holds one [m][g] plane of pairs per slice, 16 x the result at the most, of which a slice
//             touches only its own groups; 1000 rows against 59 column tiles then still give 240 workgroups).  A slice stores only the groups
//             it meets (the first slice also the empty ones before, the last those behind), into its own [m][g] plane
//             of the workspace; cl_group_min_merge takes, per (row, group), the slices whose id range holds the group
//             in slice order -- ascending columns, so "strictly nearer" again keeps the lowest index.  With one slice
//             (m >= 64 k rows) the kernel stores straight into the outputs and nothing is merged.  Against the
//             keep-best-in-registers shape: a thread's four columns (tx + 16 c) interleave the groups, so it would need
//             a best per (row, group in the tile) and a reduction per group; the owner scan costs one wave 64 LDS reads
//             and compares per tile, about a quarter of the pair work at d = 52 and a fortieth at d = 512.
//   all-points core  (DBCV) the sums shape on rows sorted by group: every thread turns its pairs into
//             t = -p * log(dist) in double (-inf for a pair of two groups, a zero distance or a padded column) and stores
//             t into a double tile in LDS, so that the 4096 logarithms of a tile are spread over all 256 threads; the
//             row's owner folds its 64 values in column order into an online log-sum-exp (running maximum M and
//             S = sum exp(t - M), one exp per value).  dist^-p itself leaves float64 for p = 50 .. 1024; M + log S does
//             not.  cl_apcore_merge folds the slices' (M, S) in slice order and finishes the power mean.
//   grouped min edge, group min of the mutual reachability: the min-edge mode with `group[j] == group[i]` as a further
//             condition, and the group-min mode with max(core_q[i], core[j], dist) stored into the distance tile.
//   rank      what is needed: per (row, q) the count of the columns l with (dist(i, l), l) < (t[i][q], tj[i][q]).  Two
//             shapes were weighed.  (a) every thread compares each of its TM x 4 pairs with all k thresholds of the pair's
//             row and the 16 lanes of a row are reduced by DPP: about 4 VALU instructions per (pair, threshold), 250 per
//             pair at k = 63, against the 8 of the pair itself at d = 4 (2 per feature) and 1024 at d = 512 -- the
//             epilogue would be 30 x the pair work in the 2-D embedding and still a quarter of it at d = 512.  (b), chosen:
//             the caller passes every row's thresholds SORTED by (t, tj); a pair is then before the thresholds
//             pos, pos + 1, ..., k - 1, pos = the first threshold behind the pair, so a thread finds pos by a binary
//             search of the row's list in LDS (at most 6 steps of one ds_read of t, one of tj and 4 VALU) and adds 1 to
//             the bin H[row][pos]; the row's counts are the prefix sums of its bins, taken once at the end of the slice.
//             Before the search every pair is compared with the row's LAST threshold, kept in registers (3 VALU): a pair
//             behind it counts nowhere and costs nothing more, and for a neighbour list those are all but about
//             rank(last) of the n columns of a row, so the search and the add run for a small share of the pairs (a wave
//             skips them when none of its 64 lanes needs them; when one does, the others idle through its chain of
//             dependent LDS reads).  Measured on 12 449 rows (profiles/embedding_quality.md): the searches and adds are
//             6 % of the pass at d = 512, k = 15 (0.66 x the kNN graph at the same k) and 48 % at d = 4, k = 15 (0.23 x
//             the kNN graph), where staging, barriers and the root make up the rest.  All 256 threads take part; there
//             is no owner scan per tile.  The bins are LDS integers with many writers: ds_add_u32 (integer atomics in
//             LDS; integer sums do not depend on the order).  LDS at TM = 4: 18 KB of staging and 3 x 64 x (k | 1) x 4
//             bytes for t, tj and the bins, 30 KB at k = 15 (three workgroups per CU: the 134 VGPRs bound it, not the
//             LDS) and 66 KB at k = 63 (two per CU of 160 KB, 8 waves; TM = 8 would allow one).  TM = 4 keeps the LDS
//             array far from its limit (the group-min note above) and gives 195 row tiles on 12 449 rows.
//             A slice stores its counts into its own plane and cl_rank_merge adds the planes; with one slice the
//             kernel stores straight into the output (`direct` in cl_mode).
// Block-diagonal walk (all-points core, grouped min edge): with the rows sorted by group a row tile needs only the
// columns from the first column of its first row's group to the last column of its last row's group.  cl_group_bounds
// writes every present group's [first, last + 1) into the workspace (one thread per row, the run boundaries store);
// cl_pairs reads the two ends for its row tile and cuts THAT tile range into the grid's slices, so the cost is the sum
// of n_c^2 over the groups (rounded up to tiles) and not n^2.  Pairs of two groups inside a shared tile are masked.
// Every mode but the sums splits the columns into slices (grid.y) whose partial results a second small kernel combines
// in a fixed order; the sums kernel keeps one workgroup per row tile so that every out[i][c] has a single writer.  The
// tile height of a mode, the cap on its slices, the bytes a slice keeps per entry and whether a single slice stores
// straight into the outputs are the mode's line in cl_mode (host side, below): cl_plan makes the grid and the workspace
// layout from it for the size function and for the entry point alike.  No
// floating-point atomics and no atomics on global memory anywhere; the only atomics are the rank mode's integer adds
// into its LDS bins, whose sums do not depend on the order: two calls give the same bits.
// Roofline: float32 VALU, 3 flops (2 instructions) per pair and feature; operands come from L2 / Infinity Cache
// ((16 TM + 64) rows per 16 TM x 64 pairs).
#include <limits.h>

#include "cl_dist.h"
#include "common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_COLS = 64;          // rows j per column tile
constexpr int CL_KC = 32;            // features per staged chunk
constexpr int CL_LDK = CL_KC + 4;    // LDS row pitch of a staged chunk (floats)
constexpr int CL_LDD = CL_COLS + 1;  // LDS row pitch of a distance tile (floats)
constexpr int CL_MAXK = 64;
constexpr int CL_GROUPMIN_SLICES = 16;  // group min: at most this many column slices (the workspace: as many result planes)
constexpr int CL_CORE = 0, CL_MINEDGE = 1, CL_SUMS = 2, CL_KNN = 3, CL_MREACHQ = 4, CL_GROUPMIN = 5;
constexpr int CL_APCORE = 6, CL_MINEDGE_G = 7, CL_GROUPMIN_MR = 8;  // DBCV: the grouped forms
constexpr int CL_RANK = 9;  // counts before per-row thresholds (no distance tile: thresholds and bins in its place)
constexpr bool cl_is_minedge(int mode) { return mode == CL_MINEDGE || mode == CL_MINEDGE_G; }
constexpr bool cl_is_groupmin(int mode) { return mode == CL_GROUPMIN || mode == CL_GROUPMIN_MR; }
// the modes whose per-row best stays in registers (no distance tile in LDS)
constexpr bool cl_keeps_best(int mode) { return cl_is_minedge(mode) || mode == CL_MREACHQ; }
// the modes on rows sorted by group that walk only the column tiles of the row tile's own groups
constexpr bool cl_block_diagonal(int mode) { return mode == CL_APCORE || mode == CL_MINEDGE_G; }

// cl_accum / cl_finish: cl_dist.h

struct ClArgs {
  const float* x;   // the column operand [n][d]
  const float* xr;  // the row operand [nr][d]: x itself in the square modes, the query rows in wm_knn_query
  int n, nr, d, tiles_per_slice, col_tiles;
  // core
  int k, kl;
  float* part_lists;  // [slices][nr][k]
  int* part_idx;      // knn: the lists' column indices, same shape (-1 pads a slice with fewer than k columns)
  // min edge
  const float* core;
  const int* comp;
  float inv_alpha;
  float* part_w;  // [slices][nr]
  int* part_j;
  // query (with core, inv_alpha, part_w, part_j)
  const float* core_q;  // [nr]
  float* part_d;        // [slices][nr]
  // sums; group min: the columns' group ids, non-decreasing, and the number of groups
  const int* labels;
  int n_clusters;
  double* out;  // [n][n_clusters]
  // group min: [slices][nr][n_clusters] (the outputs themselves when there is one slice)
  float* group_d;
  int* group_j;
  // block-diagonal modes (labels: the rows' group ids, non-decreasing; n_clusters: their number): per group the
  // columns [bounds[2 c], bounds[2 c + 1]) (cl_group_bounds)
  const int* bounds;
  // all-points core: the power and the slices' running maximum / scaled sum [slices][nr]
  double pw;
  double* part_m;
  double* part_s;
  // rank (no field of its own, so that the other modes' argument block is what it was): core_q holds the rows' k
  // thresholds sorted by (t, j) [nr][k], comp their column indices [nr][k], labels the column never counted [nr] and
  // part_idx the counts [slices][nr][k] (the output itself when there is one slice)
};

template <int MODE, int TM>
constexpr size_t cl_lds_bytes(int kl) {
  size_t f = (size_t)(16 * TM + CL_COLS) * CL_LDK;
  if (!cl_keeps_best(MODE) && MODE != CL_RANK) f += (size_t)16 * TM * CL_LDD;
  if (MODE == CL_RANK) f += (size_t)3 * 16 * TM * kl;  // thresholds, their indices, the bins
  if (MODE == CL_CORE) f += (size_t)16 * TM * kl;
  if (MODE == CL_KNN) f += (size_t)2 * 16 * TM * kl;
  if (MODE == CL_APCORE) f += (size_t)16 * TM * CL_LDD;  // (the tile holds doubles)
  if (MODE == CL_SUMS || cl_is_groupmin(MODE)) f += CL_COLS;
  return f * sizeof(float);
}

template <int MODE, int METRIC, int TM>
__global__ __launch_bounds__(CL_THREADS) void cl_pairs(const ClArgs p) {
  extern __shared__ __attribute__((aligned(16))) float cl_smem[];
  constexpr int ROWS = 16 * TM;
  constexpr int APASS = ROWS / 32, BPASS = CL_COLS / 32;
  float* As = cl_smem;
  float* Bs = As + ROWS * CL_LDK;
  [[maybe_unused]] float* Dt = Bs + CL_COLS * CL_LDK;  // (core, sums) the tile's distances [ROWS][CL_LDD]
  [[maybe_unused]] float* extra = Dt + ROWS * CL_LDD;  // core, knn: the k-lists [ROWS][kl]; sums: the tile's labels [64]
  [[maybe_unused]] int* extra_j = reinterpret_cast<int*>(extra) + ROWS * p.kl;  // knn: the lists' indices [ROWS][kl]
  // rank: the rows' sorted thresholds, their column indices and the bins [ROWS][kl] each, where the other modes' tile is
  [[maybe_unused]] float* Th = Dt;
  [[maybe_unused]] int* Tj = reinterpret_cast<int*>(Dt) + ROWS * p.kl;
  [[maybe_unused]] int* Hb = Tj + ROWS * p.kl;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lq = (t & 7) * 4, lr = t >> 3;  // staging: float4 at feature lq of row lr (+ 32 per pass)
  const int n = p.n, nr = p.nr, d = p.d;
  const int i0 = blockIdx.x * ROWS;
  int tile0 = blockIdx.y * p.tiles_per_slice;
  int tile1 = min(tile0 + p.tiles_per_slice, p.col_tiles);
  if constexpr (cl_block_diagonal(MODE)) {
    // the columns of the groups of this row tile's first and last row (uniform over the workgroup); an id outside
    // [0, n_clusters) or bounds that do not fit (rows not sorted: out of contract) give no tile or clamped ones
    const int ga = p.labels[i0], gb = p.labels[min(i0 + ROWS, nr) - 1];
    int c0 = 0, c1 = 0;
    if ((unsigned)ga < (unsigned)p.n_clusters && (unsigned)gb < (unsigned)p.n_clusters) {
      c0 = max(p.bounds[2 * ga], 0);
      c1 = min(p.bounds[2 * gb + 1], n);
    }
    const int t0 = c0 / CL_COLS, t1 = c1 > c0 ? (c1 + CL_COLS - 1) / CL_COLS : t0;
    const int per = (t1 - t0 + (int)gridDim.y - 1) / (int)gridDim.y;
    tile0 = t0 + (int)blockIdx.y * per;
    tile1 = min(tile0 + per, t1);
  }
  const int nchunks = (d + CL_KC - 1) / CL_KC;

  // ---- per-mode state
  float ci[TM], bw[TM];
  [[maybe_unused]] float bd[TM];  // query: the plain distance of the best
  [[maybe_unused]] int cpi[TM];
  int bj[TM];
  int cur = -1;
  double run = 0.0;
  [[maybe_unused]] float gbest = INFINITY;  // group min: the owner's best of the group `cur` so far and its column
  [[maybe_unused]] int gj = -1;
  [[maybe_unused]] int gi[TM];  // block-diagonal modes: the rows' groups
  [[maybe_unused]] double lm = -INFINITY, ls = 0.0;  // all-points core: the owner's running maximum and scaled sum
  if constexpr (cl_block_diagonal(MODE)) {
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int i = i0 + ty + 16 * r;
      gi[r] = i < nr ? p.labels[i] : -1;
    }
  }
  if constexpr (cl_is_minedge(MODE)) {
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int i = i0 + ty + 16 * r;
      ci[r] = i < nr ? p.core[i] : 0.f;
      cpi[r] = i < nr ? p.comp[i] : 0;
      bw[r] = INFINITY;
      bj[r] = -1;
    }
  }
  if constexpr (MODE == CL_MREACHQ || MODE == CL_GROUPMIN_MR) {
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int i = i0 + ty + 16 * r;
      ci[r] = i < nr ? p.core_q[i] : 0.f;
      bw[r] = INFINITY;
      if constexpr (MODE == CL_MREACHQ) bd[r] = INFINITY;
      bj[r] = -1;
    }
  }
  [[maybe_unused]] float tmx[TM];  // rank: the row's last (largest) threshold, its index and the column not counted
  [[maybe_unused]] int tmj[TM], sk[TM];
  if constexpr (MODE == CL_RANK) {
    // +inf or an index of -1 stands for "behind every column": (+inf, INT_MAX).  Rows past the end get a last
    // threshold no pair is before.  (The LDS lists are ordered by the chunk loop's barriers.)
    const int k = p.k;
    for (int q = t; q < ROWS * k; q += CL_THREADS) {
      const int row = q / k, e = q - row * k;
      float tv = INFINITY;
      int jv = INT_MAX;
      if (i0 + row < nr) {
        tv = p.core_q[(size_t)(i0 + row) * k + e];
        jv = p.comp[(size_t)(i0 + row) * k + e];
        if (jv < 0 || tv == INFINITY) {
          tv = INFINITY;
          jv = INT_MAX;
        }
      }
      Th[row * p.kl + e] = tv;
      Tj[row * p.kl + e] = jv;
      Hb[row * p.kl + e] = 0;
    }
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int i = i0 + ty + 16 * r;
      tmx[r] = -INFINITY;
      tmj[r] = -1;
      sk[r] = -1;
      if (i < nr) {
        tmx[r] = p.core_q[(size_t)i * k + k - 1];
        tmj[r] = p.comp[(size_t)i * k + k - 1];
        if (tmj[r] < 0 || tmx[r] == INFINITY) {
          tmx[r] = INFINITY;
          tmj[r] = INT_MAX;
        }
        sk[r] = p.labels[i];
      }
    }
  }
  if constexpr (MODE == CL_CORE || MODE == CL_KNN) {
    for (int q = t; q < ROWS * p.kl; q += CL_THREADS) extra[q] = INFINITY;  // (ordered by the chunk loop's barriers)
  }
  if constexpr (MODE == CL_KNN) {
    for (int q = t; q < ROWS * p.kl; q += CL_THREADS) extra_j[q] = -1;
  }

  for (int tile = tile0; tile < tile1; ++tile) {
    const int j0 = tile * CL_COLS;
    float acc[TM][4];
#pragma unroll
    for (int r = 0; r < TM; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    float4 ra[APASS], rb[BPASS];
    auto fetch = [&](int ch) {
      const int kq = ch * CL_KC + lq;
#pragma unroll
      for (int s = 0; s < APASS; ++s) {
        const int row = i0 + lr + 32 * s;
        ra[s] = (row < nr && kq < d) ? *reinterpret_cast<const float4*>(p.xr + (size_t)row * d + kq)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int s = 0; s < BPASS; ++s) {
        const int row = j0 + lr + 32 * s;
        rb[s] = (row < n && kq < d) ? *reinterpret_cast<const float4*>(p.x + (size_t)row * d + kq)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    fetch(0);
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();  // the previous chunk (or the previous tile's epilogue) is done with the staging buffers
#pragma unroll
      for (int s = 0; s < APASS; ++s) *reinterpret_cast<float4*>(As + (lr + 32 * s) * CL_LDK + lq) = ra[s];
#pragma unroll
      for (int s = 0; s < BPASS; ++s) *reinterpret_cast<float4*>(Bs + (lr + 32 * s) * CL_LDK + lq) = rb[s];
      __syncthreads();
      if (ch + 1 < nchunks) fetch(ch + 1);
#pragma unroll 2
      for (int kk = 0; kk < CL_KC; kk += 4) {
        float4 a[TM], b[4];
#pragma unroll
        for (int r = 0; r < TM; ++r) a[r] = *reinterpret_cast<const float4*>(As + (ty + 16 * r) * CL_LDK + kk);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(Bs + (tx + 16 * c) * CL_LDK + kk);
        // index order within every pair: x, y, z, w of this float4 follow the earlier features
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<METRIC>(a[r].x, b[c].x, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<METRIC>(a[r].y, b[c].y, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<METRIC>(a[r].z, b[c].z, acc[r][c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cl_accum<METRIC>(a[r].w, b[c].w, acc[r][c]);
      }
    }

    // ---- the tile's epilogue
    if constexpr (cl_is_minedge(MODE)) {
      float cj[4];
      int cpj[4];
      [[maybe_unused]] int gc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        cj[c] = j < n ? p.core[j] : 0.f;
        cpj[c] = j < n ? p.comp[j] : 0;
        if constexpr (MODE == CL_MINEDGE_G) gc[c] = j < n ? p.labels[j] : -2;
      }
#pragma unroll
      for (int r = 0; r < TM; ++r) {
        const bool iv = i0 + ty + 16 * r < nr;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + tx + 16 * c;
          const float w = fmaxf(fmaxf(ci[r], cj[c]), cl_finish<METRIC>(acc[r][c]) * p.inv_alpha);
          bool ok = iv && j < n && cpj[c] != cpi[r];
          if constexpr (MODE == CL_MINEDGE_G) ok = ok && gc[c] == gi[r];
          if (ok && (w < bw[r] || (w == bw[r] && j < bj[r]))) {
            bw[r] = w;
            bj[r] = j;
          }
        }
      }
    } else if constexpr (MODE == CL_MREACHQ) {
      float cj[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        cj[c] = j < n ? p.core[j] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < TM; ++r) {
        const bool iv = i0 + ty + 16 * r < nr;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + tx + 16 * c;
          const float dist = cl_finish<METRIC>(acc[r][c]);
          const float w = fmaxf(fmaxf(ci[r], cj[c]), dist * p.inv_alpha);
          // (a thread meets its columns in ascending j, so a full tie keeps the earlier one)
          if (iv && j < n && (w < bw[r] || (w == bw[r] && dist < bd[r]))) {
            bw[r] = w;
            bd[r] = dist;
            bj[r] = j;
          }
        }
      }
    } else if constexpr (MODE == CL_RANK) {
#pragma unroll
      for (int r = 0; r < TM; ++r) {
        const float* th = Th + (ty + 16 * r) * p.kl;
        const int* tj = Tj + (ty + 16 * r) * p.kl;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int l = j0 + tx + 16 * c;
          const float dv = cl_finish<METRIC>(acc[r][c]);
          if (l < n && l != sk[r] && (dv < tmx[r] || (dv == tmx[r] && l < tmj[r]))) {
            // the first threshold behind (dv, l): the last one is, so the answer lies in [0, k - 1]
            int lo = 0, hi = p.k - 1;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              const float u = th[mid];
              if (dv < u || (dv == u && l < tj[mid])) hi = mid; else lo = mid + 1;
            }
            atomicAdd(&Hb[(ty + 16 * r) * p.kl + lo], 1);
          }
        }
      }
    } else if constexpr (MODE == CL_APCORE) {
      double* Dd = reinterpret_cast<double*>(Dt);  // (8-byte aligned: the staging buffers are a multiple of 16 bytes)
      int gc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        gc[c] = j < n ? p.labels[j] : -2;
      }
#pragma unroll
      for (int r = 0; r < TM; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float dist = cl_finish<METRIC>(acc[r][c]);
          // a zero distance (the row itself, an exact duplicate) and a pair of two groups contribute nothing
          Dd[(ty + 16 * r) * CL_LDD + tx + 16 * c] = (gc[c] == gi[r] && dist > 0.f) ? -p.pw * log((double)dist) : -INFINITY;
        }
      __syncthreads();
      // (the next write of the tile lies behind the next tile's chunk barriers, which the owners reach after this scan)
      if (t < ROWS && i0 + t < nr) {
        const double* row = Dd + t * CL_LDD;
        for (int c = 0; c < CL_COLS; ++c) {
          const double v = row[c];
          if (v == -INFINITY) continue;
          if (v > lm) {
            ls = ls * exp(lm - v) + 1.0;  // (lm = -inf at the first value: exp gives 0)
            lm = v;
          } else {
            ls += exp(v - lm);
          }
        }
      }
    } else {
      [[maybe_unused]] float cj[4];
      if constexpr (MODE == CL_GROUPMIN_MR) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + tx + 16 * c;
          cj[c] = j < n ? p.core[j] : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < TM; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = cl_finish<METRIC>(acc[r][c]);
          if constexpr (MODE == CL_GROUPMIN_MR) v = fmaxf(fmaxf(ci[r], cj[c]), v);  // wm_mreach_query's weight at inv_alpha 1
          Dt[(ty + 16 * r) * CL_LDD + tx + 16 * c] = j0 + tx + 16 * c < n ? v : INFINITY;
        }
      if constexpr (MODE == CL_SUMS || cl_is_groupmin(MODE)) {
        if (t < CL_COLS) reinterpret_cast<int*>(extra)[t] = j0 + t < n ? p.labels[j0 + t] : -1;
      }
      __syncthreads();
      // (the next write of Dt / the labels lies behind the next tile's chunk barriers, which the owners reach only
      // after this scan)
      if (t < ROWS && i0 + t < nr) {
        const float* row = Dt + t * CL_LDD;
        if constexpr (MODE == CL_CORE || MODE == CL_KNN) {
          float* L = extra + t * p.kl;
          [[maybe_unused]] int* J = extra_j + t * p.kl;
          const int k = p.k;
          float kth = L[k - 1];
          for (int c = 0; c < CL_COLS; ++c) {
            const float v = row[c];
            if (v < kth) {
              int pos = k - 1;
              while (pos > 0 && L[pos - 1] > v) {
                L[pos] = L[pos - 1];
                if constexpr (MODE == CL_KNN) J[pos] = J[pos - 1];
                --pos;
              }
              L[pos] = v;
              if constexpr (MODE == CL_KNN) J[pos] = j0 + c;
              kth = L[k - 1];
            }
          }
        } else if constexpr (cl_is_groupmin(MODE)) {
          const int* lab = reinterpret_cast<const int*>(extra);
          const size_t at = ((size_t)blockIdx.y * nr + i0 + t) * p.n_clusters;
          float* od = p.group_d + at;
          int* oj = p.group_j + at;
          for (int c = 0; c < CL_COLS; ++c) {
            const int l = lab[c];
            if (l < 0 || l >= p.n_clusters) continue;
            if (l != cur) {
              if (cur >= 0) {
                od[cur] = gbest;
                oj[cur] = gj;
              }
              // the ids skipped are empty groups; the first slice also owns those before its first column
              for (int q = cur >= 0 ? cur + 1 : (blockIdx.y == 0 ? 0 : l); q < l; ++q) {
                od[q] = INFINITY;
                oj[q] = -1;
              }
              cur = l;
              gbest = INFINITY;
              gj = -1;
            }
            const float v = row[c];
            if (gj < 0 || v < gbest) {
              gbest = v;
              gj = j0 + c;
            }
          }
        } else {
          const int* lab = reinterpret_cast<const int*>(extra);
          double* orow = p.out + (size_t)(i0 + t) * p.n_clusters;
          for (int c = 0; c < CL_COLS; ++c) {
            const int l = lab[c];
            if (l < 0 || l >= p.n_clusters) continue;
            if (l != cur) {
              if (cur >= 0) orow[cur] += run;
              cur = l;
              run = 0.0;
            }
            run += (double)row[c];
          }
        }
      }
    }
  }

  // ---- the slice's result
  if constexpr (MODE == CL_SUMS) {
    if (t < ROWS && i0 + t < nr && cur >= 0) p.out[(size_t)(i0 + t) * p.n_clusters + cur] += run;
  }
  if constexpr (MODE == CL_RANK) {
    __syncthreads();  // every wave's adds are in the bins
    if (t < ROWS && i0 + t < nr) {
      const int* h = Hb + t * p.kl;
      int* o = p.part_idx + ((size_t)blockIdx.y * nr + i0 + t) * p.k;
      int before = 0;  // a pair in bin q is before the thresholds q, q + 1, ..., k - 1
      for (int q = 0; q < p.k; ++q) {
        before += h[q];
        o[q] = before;
      }
    }
  }
  if constexpr (MODE == CL_APCORE) {
    if (t < ROWS && i0 + t < nr) {
      p.part_m[(size_t)blockIdx.y * nr + i0 + t] = lm;
      p.part_s[(size_t)blockIdx.y * nr + i0 + t] = ls;
    }
  }
  if constexpr (cl_is_groupmin(MODE)) {
    if (t < ROWS && i0 + t < nr) {
      const size_t at = ((size_t)blockIdx.y * nr + i0 + t) * p.n_clusters;
      if (cur >= 0) {
        p.group_d[at + cur] = gbest;
        p.group_j[at + cur] = gj;
      }
      if (blockIdx.y == gridDim.y - 1) {  // the last slice owns the empty groups behind its last column
        for (int q = cur + 1; q < p.n_clusters; ++q) {
          p.group_d[at + q] = INFINITY;
          p.group_j[at + q] = -1;
        }
      }
    }
  }
  if constexpr (MODE == CL_CORE || MODE == CL_KNN) {
    if (t < ROWS && i0 + t < nr) {
      const float* L = extra + t * p.kl;
      float* o = p.part_lists + ((size_t)blockIdx.y * nr + i0 + t) * p.k;
      for (int q = 0; q < p.k; ++q) o[q] = L[q];
      if constexpr (MODE == CL_KNN) {
        const int* J = extra_j + t * p.kl;
        int* oj = p.part_idx + ((size_t)blockIdx.y * nr + i0 + t) * p.k;
        for (int q = 0; q < p.k; ++q) oj[q] = J[q];
      }
    }
  }
  if constexpr (cl_is_minedge(MODE)) {
    __syncthreads();  // the staging buffers become the reduction scratch: [ROWS][17] weights, then indices
    float* rw = cl_smem;
    int* rj = reinterpret_cast<int*>(cl_smem + ROWS * 17);
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      rw[(ty + 16 * r) * 17 + tx] = bw[r];
      rj[(ty + 16 * r) * 17 + tx] = bj[r];
    }
    __syncthreads();
    if (t < ROWS && i0 + t < nr) {
      float w = rw[t * 17];
      int j = rj[t * 17];
      for (int q = 1; q < 16; ++q) {
        const float wq = rw[t * 17 + q];
        const int jq = rj[t * 17 + q];
        if (jq >= 0 && (j < 0 || wq < w || (wq == w && jq < j))) {
          w = wq;
          j = jq;
        }
      }
      p.part_w[(size_t)blockIdx.y * nr + i0 + t] = w;
      p.part_j[(size_t)blockIdx.y * nr + i0 + t] = j;
    }
  }
  if constexpr (MODE == CL_MREACHQ) {
    static_assert(3 * ROWS * 17 <= (ROWS + CL_COLS) * CL_LDK, "the reduction scratch must fit the staging buffers");
    __syncthreads();  // the staging buffers become the reduction scratch: [ROWS][17] weights, distances, indices
    float* rw = cl_smem;
    float* rd = cl_smem + ROWS * 17;
    int* rj = reinterpret_cast<int*>(cl_smem + 2 * ROWS * 17);
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      rw[(ty + 16 * r) * 17 + tx] = bw[r];
      rd[(ty + 16 * r) * 17 + tx] = bd[r];
      rj[(ty + 16 * r) * 17 + tx] = bj[r];
    }
    __syncthreads();
    if (t < ROWS && i0 + t < nr) {
      float w = rw[t * 17], dist = rd[t * 17];
      int j = rj[t * 17];
      for (int q = 1; q < 16; ++q) {
        const float wq = rw[t * 17 + q], dq = rd[t * 17 + q];
        const int jq = rj[t * 17 + q];
        if (jq >= 0 && (j < 0 || wq < w || (wq == w && (dq < dist || (dq == dist && jq < j))))) {
          w = wq;
          dist = dq;
          j = jq;
        }
      }
      const size_t at = (size_t)blockIdx.y * nr + i0 + t;
      p.part_w[at] = w;
      p.part_d[at] = dist;
      p.part_j[at] = j;
    }
  }
}

// k-th smallest of the slices' k-lists of a row, by rank counting (ties ordered by position, so exactly one candidate
// has rank k - 1): one wave per row.
__global__ __launch_bounds__(CL_THREADS) void cl_core_merge(const float* __restrict__ parts, int slices, int n, int k,
                                                            float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (CL_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= n) return;
  const int m = slices * k;
  for (int q = lane; q < m; q += 64) {
    const float v = parts[((size_t)(q / k) * n + row) * k + q % k];
    int rank = 0;
    for (int s = 0; s < slices; ++s) {
      const float* l = parts + ((size_t)s * n + row) * k;
      for (int e = 0; e < k; ++e) {
        const float u = l[e];
        rank += (u < v || (u == v && s * k + e < q)) ? 1 : 0;
      }
    }
    if (rank == k - 1) out[row] = v;
  }
}

// The k smallest of the slices' k-lists of a row under (distance, index), in that order: one wave per row, a lane per
// candidate.  Every list is sorted by (distance, index), so a candidate's rank is the sum over the lists of the number
// of entries before it (a binary search each); the -1 pads of a short slice sit at +inf behind every row index and are
// told apart by their position.  The at least k real candidates fill the ranks 0 .. k-1, each exactly once.  n: the
// number of rows of the lists (the row operand's).
__global__ __launch_bounds__(CL_THREADS) void cl_knn_merge(const float* __restrict__ pd, const int* __restrict__ pj,
                                                           int slices, int n, int k, float* __restrict__ out_d,
                                                           int* __restrict__ out_j) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (CL_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= n) return;
  const int m = slices * k;
  for (int q = lane; q < m; q += 64) {
    const int sq = q / k;
    const size_t at = ((size_t)sq * n + row) * k + q % k;
    const float v = pd[at];
    const int j = pj[at];
    if (j < 0) continue;
    int rank = 0;
    for (int s = 0; s < slices && rank < k; ++s) {
      const float* ld = pd + ((size_t)s * n + row) * k;
      const int* lj = pj + ((size_t)s * n + row) * k;
      int lo = 0, hi = k;  // first entry of list s that is not before (v, j)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float u = ld[mid];
        const int ju = lj[mid];
        if (ju >= 0 && (u < v || (u == v && ju < j))) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      out_d[(size_t)row * k + rank] = v;
      out_j[(size_t)row * k + rank] = j;
    }
  }
}

__global__ __launch_bounds__(CL_THREADS) void cl_minedge_merge(const float* __restrict__ pw, const int* __restrict__ pj,
                                                               int slices, int n, float* __restrict__ out_w,
                                                               int* __restrict__ out_j) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  float w = INFINITY;
  int j = -1;
  for (int s = 0; s < slices; ++s) {
    const float ws = pw[(size_t)s * n + i];
    const int js = pj[(size_t)s * n + i];
    if (js >= 0 && (j < 0 || ws < w || (ws == w && js < j))) {
      w = ws;
      j = js;
    }
  }
  out_w[i] = j < 0 ? INFINITY : w;
  out_j[i] = j;
}

// The slices' best (w, dist, j) of a query row in the fixed slice order, lexicographic.
__global__ __launch_bounds__(CL_THREADS) void cl_mreach_query_merge(const float* __restrict__ pw, const float* __restrict__ pd,
                                                                    const int* __restrict__ pj, int slices, int m,
                                                                    float* __restrict__ out_w, float* __restrict__ out_d,
                                                                    int* __restrict__ out_j) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= m) return;
  float w = INFINITY, dist = INFINITY;
  int j = -1;
  for (int s = 0; s < slices; ++s) {
    const float ws = pw[(size_t)s * m + i], ds = pd[(size_t)s * m + i];
    const int js = pj[(size_t)s * m + i];
    if (js >= 0 && (j < 0 || ws < w || (ws == w && (ds < dist || (ds == dist && js < j))))) {
      w = ws;
      dist = ds;
      j = js;
    }
  }
  out_w[i] = j < 0 ? INFINITY : w;
  out_d[i] = j < 0 ? INFINITY : dist;
  out_j[i] = j;
}

// Per (row, group) the slices' (distance, column) in slice order.  A slice has stored the ids from its first column's
// group to its last column's (the first slice from 0, the last up to g - 1) and nothing else, so only those planes are
// read; a group no slice holds is empty.  Slices ascend in the columns: "strictly nearer" keeps the lowest column.
__global__ __launch_bounds__(CL_THREADS) void cl_group_min_merge(const float* __restrict__ pd, const int* __restrict__ pj,
                                                                 const int* __restrict__ group, int slices,
                                                                 int tiles_per_slice, int m, int e, int g,
                                                                 float* __restrict__ out_d, int* __restrict__ out_j) {
  const size_t total = (size_t)m * g;
  for (size_t q = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; q < total; q += (size_t)gridDim.x * CL_THREADS) {
    const int c = (int)(q % g);
    float best = INFINITY;
    int j = -1;
    for (int s = 0; s < slices; ++s) {
      const int first = s * tiles_per_slice * CL_COLS;
      const int last = min(first + tiles_per_slice * CL_COLS, e) - 1;
      const int lo = s == 0 ? 0 : group[first];
      const int hi = s == slices - 1 ? g - 1 : group[last];
      if (c < lo || c > hi) continue;
      const float ds = pd[(size_t)s * total + q];
      const int js = pj[(size_t)s * total + q];
      if (js >= 0 && (j < 0 || ds < best)) {
        best = ds;
        j = js;
      }
    }
    out_d[q] = j < 0 ? INFINITY : best;
    out_j[q] = j;
  }
}

// The slices' counts of every (row, threshold), added (integers: any order gives the same sum).
__global__ __launch_bounds__(CL_THREADS) void cl_rank_merge(const int* __restrict__ parts, int slices, size_t total,
                                                            int* __restrict__ out) {
  for (size_t q = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; q < total; q += (size_t)gridDim.x * CL_THREADS) {
    int sum = 0;
    for (int s = 0; s < slices; ++s) sum += parts[(size_t)s * total + q];
    out[q] = sum;
  }
}

// out[e] = dist(xq[e / k], x[idx[e]]) by the tile pass's own arithmetic: the same cl_accum over the features in index
// order in one accumulator (the tile pass adds only exact zeros behind d), the same cl_finish.  An index outside [0, n)
// gives +inf and reads nothing.
template <int METRIC>
__global__ __launch_bounds__(CL_THREADS) void cl_pair_dist(const float* __restrict__ xq, const float* __restrict__ x,
                                                           const int* __restrict__ idx, int n, int d, int k, size_t total,
                                                           float* __restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * CL_THREADS) {
    const int j = idx[e];
    float v = INFINITY;
    if ((unsigned)j < (unsigned)n) {
      const float4* a = reinterpret_cast<const float4*>(xq + (e / k) * d);
      const float4* b = reinterpret_cast<const float4*>(x + (size_t)j * d);
      float acc = 0.f;
      for (int q = 0; q < d / 4; ++q) {
        const float4 u = a[q], w = b[q];
        acc = cl_accum<METRIC>(u.x, w.x, acc);
        acc = cl_accum<METRIC>(u.y, w.y, acc);
        acc = cl_accum<METRIC>(u.z, w.z, acc);
        acc = cl_accum<METRIC>(u.w, w.w, acc);
      }
      v = cl_finish<METRIC>(acc);
    }
    out[e] = v;
  }
}

// Per group present among the sorted ids its columns [first, last + 1): the two rows at a run's ends store them.  An id
// outside [0, g) stores nothing.
__global__ __launch_bounds__(CL_THREADS) void cl_group_bounds(const int* __restrict__ group, int n, int g,
                                                              int* __restrict__ bounds) {
  const int j = blockIdx.x * CL_THREADS + threadIdx.x;
  if (j >= n) return;
  const int v = group[j];
  if ((unsigned)v >= (unsigned)g) return;
  if (j == 0 || group[j - 1] != v) bounds[2 * v] = j;
  if (j == n - 1 || group[j + 1] != v) bounds[2 * v + 1] = j + 1;
}

// The slices' (running maximum, scaled sum) of a row in slice order, then the power mean of the definition:
// ((1 / (n_c - 1)) sum dist^-p)^(-1 / p) = exp(-(M + log S - log(n_c - 1)) / p); 0 for a row without a positive distance.
__global__ __launch_bounds__(CL_THREADS) void cl_apcore_merge(const double* __restrict__ pm, const double* __restrict__ ps,
                                                              int slices, int n, const int* __restrict__ group,
                                                              const int* __restrict__ bounds, int g, double pw,
                                                              double* __restrict__ out) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  double m = -INFINITY, s = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double mq = pm[(size_t)q * n + i], sq = ps[(size_t)q * n + i];
    if (mq == -INFINITY) continue;
    if (mq > m) {
      s = s * exp(m - mq) + sq;
      m = mq;
    } else {
      s += sq * exp(mq - m);
    }
  }
  const int v = group[i];
  const int nc = (unsigned)v < (unsigned)g ? bounds[2 * v + 1] - bounds[2 * v] : 0;
  out[i] = (m == -INFINITY || nc < 2) ? 0.0 : exp(-(m + log(s) - log((double)(nc - 1))) / pw);
}

// ---- host side: one plan per mode, one set of checks, one argument head ---------------------------------------------

struct ClGrid {
  int row_tiles, col_tiles, slices, tiles_per_slice;
};
// Column slices so that about a thousand workgroups exist (four per CU); every slice holds at least one tile.  m rows
// (the row operand) against n columns; the square modes pass n for both.  max_slices: the group-min mode's cap (its
// workspace is a whole [m][g] plane per slice).
inline ClGrid cl_grid(int m, int n, int rows, bool sliced, int max_slices = 1 << 30) {
  ClGrid g;
  g.row_tiles = wm_cdiv(m, rows);
  g.col_tiles = wm_cdiv(n, CL_COLS);
  int want = sliced ? wm_cdiv(1024, g.row_tiles) : 1;
  if (want > g.col_tiles) want = g.col_tiles;
  if (want > max_slices) want = max_slices;
  g.tiles_per_slice = wm_cdiv(g.col_tiles, want);
  g.slices = wm_cdiv(g.col_tiles, g.tiles_per_slice);
  return g;
}

// What the host knows about a mode, written here once and nowhere else: the TM that cl_launch instantiates (a row tile
// is 16 * tm rows, which is what cl_grid gets), how the columns are sliced, and what every slice keeps in the workspace
// for the merge kernel.  A new mode adds its line to cl_mode; its size function and its entry point both go through
// cl_plan, so they cannot disagree.
enum ClPer { CL_PER_ROW, CL_PER_ROW_K, CL_PER_ROW_GROUP };  // a slice's entries: per row, per (row, k), per (row, group)
struct ClMode {
  int tm;
  bool sliced;
  int max_slices;
  ClPer per;
  int entry_bytes;  // of one entry over all of the mode's planes; the planes lie one behind the other
  bool direct;      // a single slice stores straight into the outputs and needs no plane (and no merge)
  bool bounds;      // behind the planes: g pairs [first, last + 1) of ints (cl_group_bounds)
};
constexpr int CL_ANY_SLICES = 1 << 30;
constexpr ClMode cl_mode(int mode) {
  switch (mode) {  //            tm, sliced, max_slices, per, entry_bytes, direct, bounds
    case CL_CORE:        return {8, true, CL_ANY_SLICES, CL_PER_ROW_K, 4, false, false};  // the k-list's distances
    case CL_KNN:         return {8, true, CL_ANY_SLICES, CL_PER_ROW_K, 8, false, false};  // distances, then indices
    case CL_MINEDGE:     return {8, true, CL_ANY_SLICES, CL_PER_ROW, 8, false, false};    // w, then j
    case CL_MINEDGE_G:   return {8, true, CL_ANY_SLICES, CL_PER_ROW, 8, false, true};
    case CL_MREACHQ:     return {8, true, CL_ANY_SLICES, CL_PER_ROW, 12, false, false};   // w, dist, j
    case CL_APCORE:      return {4, true, CL_ANY_SLICES, CL_PER_ROW, 16, false, true};    // M, then S (doubles)
    case CL_RANK:        return {4, true, CL_ANY_SLICES, CL_PER_ROW_K, 4, true, false};   // counts
    case CL_GROUPMIN:
    case CL_GROUPMIN_MR: return {4, true, CL_GROUPMIN_SLICES, CL_PER_ROW_GROUP, 8, true, false};  // distances, then columns
    case CL_SUMS:        return {4, false, 1, CL_PER_ROW, 0, false, false};  // one workgroup per row tile, no workspace
  }
  return {};  // (tm = 0: cl_launch refuses to compile)
}

struct ClPlan {
  ClGrid grid;
  bool direct;     // the kernel's results are final: pass the outputs, launch no merge
  size_t entries;  // of one plane: slices * m [* k or * g]; 0 when direct
  size_t bytes;    // what the entry point needs of the workspace (the size function adds its slack of 256)
};
template <int MODE>
ClPlan cl_plan(int m, int n, int k, int g) {
  constexpr ClMode md = cl_mode(MODE);
  ClPlan p;
  p.grid = cl_grid(m, n, 16 * md.tm, md.sliced, md.max_slices);
  p.direct = md.direct && p.grid.slices == 1;
  const size_t width = md.per == CL_PER_ROW_K ? k : md.per == CL_PER_ROW_GROUP ? g : 1;
  p.entries = p.direct ? 0 : (size_t)p.grid.slices * m * width;
  p.bytes = p.entries * md.entry_bytes + (md.bounds ? (size_t)g * 8 : 0);
  return p;
}

// The planes of a workspace in the order in which they lie in it.
struct ClCarve {
  char* at;
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(at);
    at += count * sizeof(T);
    return p;
  }
};

template <int MODE>
int cl_launch(const ClArgs& a, const ClGrid& g, int metric, hipStream_t st) {
  constexpr int TM = cl_mode(MODE).tm;
  static_assert(TM == 4 || TM == 8, "the mode has no line in cl_mode");
  const size_t lds = cl_lds_bytes<MODE, TM>(a.kl);
  constexpr size_t lds_max = cl_lds_bytes<MODE, TM>(CL_MAXK | 1);  // the mode's largest request, allowed once
  static bool attr_set[2] = {false, false};  // per metric; idempotent; a race only repeats the call
  if (lds_max > 64 * 1024 && !attr_set[metric]) {
    const void* fn = metric == 0 ? reinterpret_cast<const void*>(&cl_pairs<MODE, 0, TM>)
                                 : reinterpret_cast<const void*>(&cl_pairs<MODE, 1, TM>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    if (e != hipSuccess) return (int)e;
    attr_set[metric] = true;
  }
  const dim3 grid(g.row_tiles, g.slices);
  if (metric == 0)
    cl_pairs<MODE, 0, TM><<<grid, CL_THREADS, lds, st>>>(a);
  else
    cl_pairs<MODE, 1, TM><<<grid, CL_THREADS, lds, st>>>(a);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

inline bool cl_shape_ok(int d, int metric) { return d % 4 == 0 && d <= 1024 && (metric == 0 || metric == 1); }
constexpr int CL_MAX_N = 1 << 24;  // (row * d and slice * n + row stay far inside size_t; tile indices inside int)
inline bool cl_count_ok(int v) { return v > 0 && v <= CL_MAX_N; }

// The checks every entry point makes before it touches the device, in the order the callers rely on.  `valid`: the
// entry point's own part of the first stage (no null pointer, k <= n, ...); `aligned`: its pointers' alignment.  An
// entry point without a k or without groups passes 1.
inline int cl_check(bool valid, int m, int n, int d, int metric, int k, int g, bool aligned) {
  WM_REQUIRE(valid && m > 0 && n > 0 && d > 0 && k > 0 && g > 0, WM_EINVAL);
  WM_REQUIRE(k <= CL_MAXK && m <= CL_MAX_N && n <= CL_MAX_N && g <= CL_MAX_N && cl_shape_ok(d, metric), WM_EUNSUPPORTED);
  WM_REQUIRE(aligned, WM_EALIGN);
  return WM_OK;
}
// The same and, last, the workspace against the mode's plan, which it hands back.
template <int MODE>
int cl_prepare(bool valid, int m, int n, int d, int metric, int k, int g, bool aligned, size_t workspace_bytes, ClPlan* plan) {
  const int rc = cl_check(valid, m, n, d, metric, k, g, aligned);
  if (rc != WM_OK) return rc;
  *plan = cl_plan<MODE>(m, n, k, g);
  WM_REQUIRE(workspace_bytes >= plan->bytes, WM_EWORKSPACE);
  return WM_OK;
}
// The size functions: 0 outside the sizes the plan is made for (d and the metric are the entry point's to refuse).
template <int MODE>
size_t cl_workspace_bytes(int m, int n, int d, int k, int g) {
  if (!(cl_count_ok(m) && cl_count_ok(n) && d > 0 && k > 0 && k <= CL_MAXK && cl_count_ok(g))) return 0;
  return cl_plan<MODE>(m, n, k, g).bytes + 256;
}

// The head of every mode's arguments: nr rows of xr against the n rows of x (the square modes pass x, n twice).
inline ClArgs cl_args(const float* xr, int nr, const float* x, int n, int d, const ClGrid& g) {
  ClArgs a = {};
  a.x = x;
  a.n = n;
  a.xr = xr;
  a.nr = nr;
  a.d = d;
  a.tiles_per_slice = g.tiles_per_slice;
  a.col_tiles = g.col_tiles;
  return a;
}

// The grid of the grid-stride kernels (cl_pair_dist, cl_rank_merge, cl_group_min_merge): a thread per element, capped.
inline unsigned cl_grid_1d(size_t total) {
  const size_t blocks = (total + CL_THREADS - 1) / CL_THREADS;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace

extern "C" size_t wm_core_distance_workspace_bytes(int n, int d, int k) { return cl_workspace_bytes<CL_CORE>(n, n, d, k, 1); }

extern "C" int wm_core_distance(const float* x, int n, int d, int metric, int k, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<CL_CORE>(x && out && workspace && k <= n, n, n, d, metric, k, 1,
                                     wm_aligned(x, 15) && wm_aligned(workspace, 15), workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClArgs a = cl_args(x, n, x, n, d, pl.grid);
  a.k = k;
  a.kl = k | 1;  // odd pitch: the owners' list accesses fall on distinct banks
  a.part_lists = static_cast<float*>(workspace);
  const int lrc = cl_launch<CL_CORE>(a, pl.grid, metric, st);
  if (lrc != WM_OK) return lrc;
  cl_core_merge<<<wm_cdiv(n, CL_THREADS / 64), CL_THREADS, 0, st>>>(a.part_lists, pl.grid.slices, n, k, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

namespace {

// wm_knn_graph (xq = x, m = n) and wm_knn_query.
int cl_knn_run(const float* xq, int m, const float* x, int n, int d, int metric, int k, float* dist, int32_t* idx,
               void* workspace, size_t workspace_bytes, void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<CL_KNN>(xq && x && dist && idx && workspace && k <= n, m, n, d, metric, k, 1,
                                    wm_aligned(xq, 15) && wm_aligned(x, 15) && wm_aligned(workspace, 15), workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClCarve ws{static_cast<char*>(workspace)};
  ClArgs a = cl_args(xq, m, x, n, d, pl.grid);
  a.k = k;
  a.kl = k | 1;  // odd pitch: the owners' list accesses fall on distinct banks
  a.part_lists = ws.take<float>(pl.entries);
  a.part_idx = ws.take<int>(pl.entries);
  const int lrc = cl_launch<CL_KNN>(a, pl.grid, metric, st);
  if (lrc != WM_OK) return lrc;
  cl_knn_merge<<<wm_cdiv(m, CL_THREADS / 64), CL_THREADS, 0, st>>>(a.part_lists, a.part_idx, pl.grid.slices, m, k, dist, idx);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

}  // namespace

extern "C" size_t wm_knn_graph_workspace_bytes(int n, int d, int k) { return cl_workspace_bytes<CL_KNN>(n, n, d, k, 1); }

extern "C" int wm_knn_graph(const float* x, int n, int d, int metric, int k, float* dist, int32_t* idx, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return cl_knn_run(x, n, x, n, d, metric, k, dist, idx, workspace, workspace_bytes, stream);
}

extern "C" size_t wm_knn_query_workspace_bytes(int m, int n, int d, int k) { return cl_workspace_bytes<CL_KNN>(m, n, d, k, 1); }

extern "C" int wm_knn_query(const float* xq, int m, const float* x, int n, int d, int metric, int k, float* dist, int32_t* idx,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return cl_knn_run(xq, m, x, n, d, metric, k, dist, idx, workspace, workspace_bytes, stream);
}

extern "C" int wm_pair_dist(const float* xq, int m, const float* x, int n, int d, int metric, const int32_t* idx, int k,
                            float* out, void* stream) {
  const int rc = cl_check(xq && x && idx && out, m, n, d, metric, k, 1, wm_aligned(xq, 15) && wm_aligned(x, 15));
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t total = (size_t)m * k;
  if (metric == 0)
    cl_pair_dist<0><<<cl_grid_1d(total), CL_THREADS, 0, st>>>(xq, x, idx, n, d, k, total, out);
  else
    cl_pair_dist<1><<<cl_grid_1d(total), CL_THREADS, 0, st>>>(xq, x, idx, n, d, k, total, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_rank_query_workspace_bytes(int m, int n, int d, int k) { return cl_workspace_bytes<CL_RANK>(m, n, d, k, 1); }

extern "C" int wm_rank_query(const float* xq, int m, const float* x, int n, int d, int metric, const float* t, const int32_t* tj,
                             const int32_t* skip, int k, int32_t* count, void* workspace, size_t workspace_bytes,
                             void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<CL_RANK>(xq && x && t && tj && skip && count && workspace, m, n, d, metric, k, 1,
                                     wm_aligned(xq, 15) && wm_aligned(x, 15) && wm_aligned(workspace, 15), workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClArgs a = cl_args(xq, m, x, n, d, pl.grid);
  a.k = k;
  a.kl = k | 1;  // odd pitch: the owners' prefix sums fall on distinct banks
  a.core_q = t;
  a.comp = tj;
  a.labels = skip;
  a.part_idx = pl.direct ? count : static_cast<int*>(workspace);
  const int lrc = cl_launch<CL_RANK>(a, pl.grid, metric, st);
  if (lrc != WM_OK || pl.direct) return lrc;
  const size_t total = (size_t)m * k;
  cl_rank_merge<<<cl_grid_1d(total), CL_THREADS, 0, st>>>(a.part_idx, pl.grid.slices, total, count);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

namespace {

// wm_mreach_min_edge (group = nullptr, g = 1) and wm_mreach_min_edge_grouped (inv_alpha = 1: dist * 1 is dist, so the
// weights are wm_mreach_min_edge's bits at alpha 1).
template <int MODE>
int cl_min_edge_run(const float* x, const float* core, const int32_t* comp, const int32_t* group, int n, int d, int metric,
                    int g, float inv_alpha, float* out_w, int32_t* out_j, void* workspace, size_t workspace_bytes,
                    void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<MODE>(x && core && comp && (MODE == CL_MINEDGE || group) && out_w && out_j && workspace &&
                                      inv_alpha > 0.f,
                                  n, n, d, metric, 1, g, wm_aligned(x, 15) && wm_aligned(workspace, 15), workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClCarve ws{static_cast<char*>(workspace)};
  ClArgs a = cl_args(x, n, x, n, d, pl.grid);
  a.core = core;
  a.comp = comp;
  a.inv_alpha = inv_alpha;
  a.part_w = ws.take<float>(pl.entries);
  a.part_j = ws.take<int>(pl.entries);
  if constexpr (MODE == CL_MINEDGE_G) {
    int* bounds = ws.take<int>(2 * (size_t)g);
    a.labels = group;
    a.n_clusters = g;
    a.bounds = bounds;
    cl_group_bounds<<<wm_cdiv(n, CL_THREADS), CL_THREADS, 0, st>>>(group, n, g, bounds);
    WM_LAUNCH_CHECK();
  }
  const int lrc = cl_launch<MODE>(a, pl.grid, metric, st);
  if (lrc != WM_OK) return lrc;
  cl_minedge_merge<<<wm_cdiv(n, CL_THREADS), CL_THREADS, 0, st>>>(a.part_w, a.part_j, pl.grid.slices, n, out_w, out_j);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

}  // namespace

extern "C" size_t wm_mreach_min_edge_workspace_bytes(int n, int d) { return cl_workspace_bytes<CL_MINEDGE>(n, n, d, 1, 1); }

extern "C" int wm_mreach_min_edge(const float* x, const float* core, const int32_t* comp, int n, int d, int metric,
                                  float inv_alpha, float* out_w, int32_t* out_j, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return cl_min_edge_run<CL_MINEDGE>(x, core, comp, nullptr, n, d, metric, 1, inv_alpha, out_w, out_j, workspace,
                                     workspace_bytes, stream);
}

extern "C" size_t wm_mreach_min_edge_grouped_workspace_bytes(int n, int d, int g) {
  return cl_workspace_bytes<CL_MINEDGE_G>(n, n, d, 1, g);
}

extern "C" int wm_mreach_min_edge_grouped(const float* x, const float* core, const int32_t* comp, const int32_t* group, int n,
                                          int d, int metric, int g, float* out_w, int32_t* out_j, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return cl_min_edge_run<CL_MINEDGE_G>(x, core, comp, group, n, d, metric, g, 1.f, out_w, out_j, workspace, workspace_bytes,
                                       stream);
}

extern "C" size_t wm_allpoints_core_workspace_bytes(int n, int d, int g) { return cl_workspace_bytes<CL_APCORE>(n, n, d, 1, g); }

extern "C" int wm_allpoints_core(const float* x, const int32_t* group, int n, int d, int metric, int g, double p, double* out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<CL_APCORE>(x && group && out && workspace && p > 0.0 && p < (double)INFINITY, n, n, d, metric, 1, g,
                                       wm_aligned(x, 15) && wm_aligned(workspace, 15) && wm_aligned(out, 7), workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClCarve ws{static_cast<char*>(workspace)};
  ClArgs a = cl_args(x, n, x, n, d, pl.grid);
  a.labels = group;
  a.n_clusters = g;
  a.pw = p;
  a.part_m = ws.take<double>(pl.entries);
  a.part_s = ws.take<double>(pl.entries);
  int* bounds = ws.take<int>(2 * (size_t)g);
  a.bounds = bounds;
  cl_group_bounds<<<wm_cdiv(n, CL_THREADS), CL_THREADS, 0, st>>>(group, n, g, bounds);
  WM_LAUNCH_CHECK();
  const int lrc = cl_launch<CL_APCORE>(a, pl.grid, metric, st);
  if (lrc != WM_OK) return lrc;
  cl_apcore_merge<<<wm_cdiv(n, CL_THREADS), CL_THREADS, 0, st>>>(a.part_m, a.part_s, pl.grid.slices, n, group, bounds, g, p, out);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_mreach_query_workspace_bytes(int m, int n, int d) { return cl_workspace_bytes<CL_MREACHQ>(m, n, d, 1, 1); }

extern "C" int wm_mreach_query(const float* xq, const float* core_q, int m, const float* x, const float* core, int n, int d,
                               int metric, float inv_alpha, float* out_w, float* out_dist, int32_t* out_j, void* workspace,
                               size_t workspace_bytes, void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<CL_MREACHQ>(xq && core_q && x && core && out_w && out_dist && out_j && workspace && inv_alpha > 0.f, m,
                                        n, d, metric, 1, 1, wm_aligned(xq, 15) && wm_aligned(x, 15) && wm_aligned(workspace, 15),
                                        workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClCarve ws{static_cast<char*>(workspace)};
  ClArgs a = cl_args(xq, m, x, n, d, pl.grid);
  a.core = core;
  a.core_q = core_q;
  a.inv_alpha = inv_alpha;
  a.part_w = ws.take<float>(pl.entries);
  a.part_d = ws.take<float>(pl.entries);
  a.part_j = ws.take<int>(pl.entries);
  const int lrc = cl_launch<CL_MREACHQ>(a, pl.grid, metric, st);
  if (lrc != WM_OK) return lrc;
  cl_mreach_query_merge<<<wm_cdiv(m, CL_THREADS), CL_THREADS, 0, st>>>(a.part_w, a.part_d, a.part_j, pl.grid.slices, m, out_w,
                                                                      out_dist, out_j);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" int wm_cluster_dist_sums(const float* x, const int32_t* labels, int n, int d, int metric, int n_clusters,
                                    double* out, void* stream) {
  const int rc = cl_check(x && labels && out && n_clusters >= 2 && n_clusters <= n, n, n, d, metric, 1, 1,
                          wm_aligned(x, 15) && wm_aligned(out, 7));
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = wm_zero_async(out, (size_t)n * n_clusters * sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  const ClPlan pl = cl_plan<CL_SUMS>(n, n, 1, n_clusters);
  ClArgs a = cl_args(x, n, x, n, d, pl.grid);
  a.labels = labels;
  a.n_clusters = n_clusters;
  a.out = out;
  return cl_launch<CL_SUMS>(a, pl.grid, metric, st);
}

namespace {

// wm_group_min_dist (core_q = core = nullptr) and wm_group_min_mreach.
template <int MODE>
int cl_group_min_run(const float* xq, const float* core_q, int m, const float* xe, const float* core, const int32_t* group,
                     int e, int d, int metric, int g, float* out_dist, int32_t* out_j, void* workspace, size_t workspace_bytes,
                     void* stream) {
  ClPlan pl;
  const int rc = cl_prepare<MODE>(xq && xe && group && out_dist && out_j && workspace && (MODE == CL_GROUPMIN || (core_q && core)),
                                  m, e, d, metric, 1, g, wm_aligned(xq, 15) && wm_aligned(xe, 15) && wm_aligned(workspace, 15),
                                  workspace_bytes, &pl);
  if (rc != WM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ClCarve ws{static_cast<char*>(workspace)};
  ClArgs a = cl_args(xq, m, xe, e, d, pl.grid);
  a.core_q = core_q;
  a.core = core;
  a.labels = group;
  a.n_clusters = g;
  a.group_d = pl.direct ? out_dist : ws.take<float>(pl.entries);
  a.group_j = pl.direct ? out_j : ws.take<int>(pl.entries);
  const int lrc = cl_launch<MODE>(a, pl.grid, metric, st);
  if (lrc != WM_OK || pl.direct) return lrc;
  cl_group_min_merge<<<cl_grid_1d((size_t)m * g), CL_THREADS, 0, st>>>(a.group_d, a.group_j, group, pl.grid.slices,
                                                                      pl.grid.tiles_per_slice, m, e, g, out_dist, out_j);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

}  // namespace

extern "C" size_t wm_group_min_dist_workspace_bytes(int m, int e, int d, int g) {
  return cl_workspace_bytes<CL_GROUPMIN>(m, e, d, 1, g);
}

extern "C" int wm_group_min_dist(const float* xq, int m, const float* xe, const int32_t* group, int e, int d, int metric, int g,
                                 float* out_dist, int32_t* out_j, void* workspace, size_t workspace_bytes, void* stream) {
  return cl_group_min_run<CL_GROUPMIN>(xq, nullptr, m, xe, nullptr, group, e, d, metric, g, out_dist, out_j, workspace,
                                       workspace_bytes, stream);
}

extern "C" size_t wm_group_min_mreach_workspace_bytes(int m, int e, int d, int g) {
  return wm_group_min_dist_workspace_bytes(m, e, d, g);
}

extern "C" int wm_group_min_mreach(const float* xq, const float* core_q, int m, const float* xe, const float* core,
                                   const int32_t* group, int e, int d, int metric, int g, float* out_w, int32_t* out_j,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return cl_group_min_run<CL_GROUPMIN_MR>(xq, core_q, m, xe, core, group, e, d, metric, g, out_w, out_j, workspace,
                                          workspace_bytes, stream);
}

