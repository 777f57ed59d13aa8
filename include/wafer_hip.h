/*
 * wafer_hip.h — C ABI of libwafer_hip.so, the MI355X (gfx950) hot path for the
 * self-supervised wafer-map pipeline of faris-k/self-supervised-wafermaps.
 *
 * The reference has no FFI of its own (pure Python on torch/lightly/timm/torchvision); its seam is
 * the set of Python callables listed in SURVEY.md §8(b).  Every entry point below names the
 * reference call site (file:line under the reference checkout) whose device work it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory owned by the caller
 *     (the library never allocates, frees or retains device memory);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no implicit sync;
 *   - return 0 on success, a negative WM_E* code for bad arguments, a positive hipError_t value
 *     when the HIP runtime reports a launch failure;
 *   - re-entrant, no mutable global state.
 *   - activation tensors are NHWC ("channels_last"); bf16 tensors are raw uint16 bit patterns.
 */
#ifndef WAFER_HIP_H
#define WAFER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_ABI_VERSION 4

/* error codes */
#define WM_OK 0
#define WM_EINVAL (-1)       /* null pointer / non-positive size */
#define WM_EUNSUPPORTED (-2) /* shape/dtype combination the kernels do not implement */
#define WM_EWORKSPACE (-3)   /* workspace too small */
#define WM_EALIGN (-4)       /* pointer or row pitch not aligned as required */

/* dtypes */
#define WM_F32 0
#define WM_BF16 1

int wm_version(void);
const char* wm_error_string(int code);
/* Small device-side pieces that keep framework launches out of the captured training step: clear a buffer (the flat
 * gradient arena of optimizer.zero_grad; a kernel, never a memset node: profiles/r02_nan_root_cause.md) and
 * out[0] = mean_i f(x_i), f = identity or sqrt(scale * x_i) (mean of the NT-Xent row losses, scripts/WM811k_benchmark.py:247;
 * lightly's std_of_l2_normalized monitor, :239), one block, fixed summation order. */
int wm_fill_zero(void* p, size_t bytes, void* stream);
int wm_mean_f32(const float* x, long long n, float scale, int sqrt_of, float* out, void* stream);
/* y = x * *scale_dev over n bf16 elements (n % 8 == 0, 16-byte aligned): the device-resident upstream gradient of a scalar
 * loss applied to the gradient tensor its forward pass saved (no host read of the scalar, no f32 round trip through HBM). */
int wm_scale_bf16(const void* x, long long n, const float* scale_dev, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Two-view augmentation.
 * Replaces the per-sample CPU pipeline
 *   get_base_transforms          src/ssl_wafermap/transforms/augmentations.py:253-332
 *   get_inference_transforms     src/ssl_wafermap/transforms/augmentations.py:335-357
 *   DieNoise.__call__            augmentations.py:27-36
 *   MedianFilter.__call__        augmentations.py:103-107
 *   DPWTransform.dpw_transform   augmentations.py:182-227
 *   MultiCropViewTransform       src/ssl_wafermap/transforms/wafer_multicrop_transform.py:16-85
 *   WaferMapDataset.__getitem__  src/ssl_wafermap/data/dataset.py:29-34
 * with one launch over a ragged HBM-resident wafer store.  Every random decision is an input
 * (drawn on the host by the transform classes), so the CPU oracle sees identical choices.
 * ------------------------------------------------------------------------------------------- */

#define WM_AUG_NONE 0
#define WM_AUG_DIENOISE 1
#define WM_AUG_DPW 2
#define WM_AUG_MEDIAN3 3

#define WM_IMG_NCHW_F32 0  /* [n][3][S][S] float32 (the reference's tensor layout)            */
#define WM_IMG_NHWC_BF16 1 /* [n][S][S][3] bf16     (channels_last, feeds the conv kernels)   */
#define WM_IMG_HW_U8 2     /* [n][S][S]    uint8    (pre-ToTensor grey image, for parity checks) */
#define WM_IMG_S2D_BF16 3  /* [n][S/2][S/2][16] bf16: 2x2 space-to-depth of the NHWC image, channel = dh*6 + dw*3 + c,
                              12..15 zero -- the layout the stem convolution consumes (wm_image_to_s2d's output) */

typedef struct WmViewParams {
  int32_t sample;      /* index into the wafer store                                         */
  int32_t out_slot;    /* image index inside `out`                                           */
  int32_t op;          /* WM_AUG_*                                                           */
  uint32_t noise_seed; /* DieNoise: key of the counter RNG (rand(r,c) = wm_rand01(seed, r*W+c)) */
  float noise_p;       /* DieNoise flip probability                                          */
  int32_t dpw_h;       /* DPW: int(H*scale), computed on the host in double like the reference */
  int32_t dpw_w;       /* DPW: int(W*scale)                                                  */
  int32_t rot90;       /* 1 = rotate 90 deg counter-clockwise after the resize               */
  int32_t vflip;       /* 1 = vertical flip   (after rot90)                                   */
  int32_t hflip;       /* 1 = horizontal flip (after vflip)                                   */
  int32_t crop;        /* 1 = RandomResizedCrop box (i,j,h,w) of the img_size image           */
  int32_t crop_i, crop_j, crop_h, crop_w;
  int32_t reserved;
} WmViewParams;

/* wafers: concatenated uint8 maps; wafer s is rows-major heights[s] x widths[s] at offsets[s].
 * params: n_views entries (device).  img_size: side of the square Resize target (224).
 * out_size: side of the emitted image (== img_size unless crop; % 8 == 0).  mean/std: Normalize
 * stats.  max_wafer_elems: largest H*W in the store (host-known; sizes the LDS images; a wafer
 * above it is skipped).  Largest supported wafer side, img_size and out_size: 256.
 * DieNoise RNG: rand(r,c) = (lowbias32(idx ^ lowbias32(seed ^ 0x9E3779B9)) >> 8) * 2^-24 with
 * idx = r*W + c; the flip test is rand < noise_p in float32 (oracle/augment.py: rand01). */
int wm_augment_views(const uint8_t* wafers, const int64_t* offsets, const int32_t* heights,
                     const int32_t* widths, int n_wafers, int max_wafer_elems,
                     const WmViewParams* params, int n_views, int img_size, int out_size,
                     int out_format, int normalize, float mean, float std, void* out,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * kNN retrieval.
 * Replaces lightly.utils.benchmarking.knn_predict as called at
 *   src/ssl_wafermap/models/knn.py:91-98   (mm -> topk -> gather -> exp -> one-hot -> argsort)
 * and the bank build's F.normalize at src/ssl_wafermap/models/knn.py:76-80.
 * Blocked pairwise-dot on MFMA with a running in-register top-k; the [B,N] similarity matrix is
 * never written to HBM.
 * ------------------------------------------------------------------------------------------- */

/* query [nq][d], bank [n][d] row-major, both `dtype` (WM_F32 or WM_BF16); row bytes % 256 == 0; d <= 512 (k <= 8 when a row exceeds 1 KB).
 * out_sim [nq][k] float32 descending, out_idx [nq][k] int32 (ties: lower bank index first).
 * 1 <= k <= 16, k <= n.  bank_index_base is added to every emitted index (sharded banks). */
size_t wm_knn_topk_workspace_bytes(int nq, int n, int d, int k);
int wm_knn_topk(const void* query, const void* bank, int nq, int n, int d, int dtype, int k,
                int bank_index_base, float* out_sim, int32_t* out_idx, void* workspace,
                size_t workspace_bytes, void* stream);

/* General-shape variant for the retrieval flow: float32, any d <= 1024 (d % 4 == 0), k <= 16, score =
 * q.x + bias[row] (bias may be NULL).  With bias = -||x||^2 / 2 the ranking is the Euclidean one
 * (sklearn NearestNeighbors on the dumped embeddings, notebooks/2.0-Figures-nearest-neighbors cell 2). */
size_t wm_knn_topk_general_workspace_bytes(int nq, int n, int d, int k);
int wm_knn_topk_general(const float* query, const float* bank, const float* bias, int nq, int n, int d, int k,
                        int bank_index_base, float* out_sim, int32_t* out_idx, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The next page: top-k among the rows strictly AFTER the cursor (after_sim[q], after_idx[q]) in the list order
 * (score descending, index ascending; after_idx in the output index space, i.e. including bank_index_base).
 * Calling it with the last entry of the previous page walks a top-K of any length in pages of <= 16
 * (lightly's knn_predict default knn_k = 200; the reference itself uses 5).  NULL cursors = the first page. */
int wm_knn_topk_general_after(const float* query, const float* bank, const float* bias, int nq, int n, int d, int k,
                              int bank_index_base, const float* after_sim, const int32_t* after_idx, float* out_sim,
                              int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* wm_knn_topk for nq queries in batches of `batch` rows, batch i (streaming + selection kernel) on
 * streams[i % n_streams] with slice i % n_streams of `workspaces` (n_streams slices of workspace_bytes_per_lane >=
 * wm_knn_topk_workspace_bytes(batch, ...) bytes, a multiple of 256), every launch queued by this one call: the
 * selection kernel of a batch overlaps the streaming kernels queued behind it on the other streams.  The caller
 * orders the streams against its own (fork before, join after).  (Embedding retrieval over a whole set:
 * notebooks/3.0-Embeddings-inference.ipynb cell 7; BASELINE configs[4].) */
int wm_knn_topk_many(const void* query, const void* bank, int nq, int n, int d, int dtype, int k, int bank_index_base,
                     float* out_sim, int32_t* out_idx, int batch, void* workspaces, size_t workspace_bytes_per_lane,
                     void* const* streams, int n_streams);

/* Merge `parts` candidate lists per query ([parts][nq][k], e.g. all-gathered shard results)
 * into the global top-k.  in_* and out_* may not alias. */
int wm_knn_merge(const float* in_sim, const int32_t* in_idx, int parts, int nq, int k,
                 float* out_sim, int32_t* out_idx, void* stream);

/* Weighted vote: w = exp(sim/t); score[c] = sum_j w_j [labels[idx_j]==c]; classes sorted by score
 * descending (ties: lower class id first) into pred_labels [nq][num_classes] int64 — the tensor
 * knn_predict returns; scores [nq][num_classes] float32 optional (may be NULL).  bank_labels holds
 * n_labels entries; a neighbour index outside [0, n_labels) (the padding of a shard list shorter than k)
 * casts no vote. */
int wm_knn_vote(const float* sim, const int32_t* idx, const int64_t* bank_labels, long long n_labels, int nq, int k,
                int num_classes, float temperature, int64_t* pred_labels, float* scores,
                void* stream);

/* Row-wise L2 normalisation y = x / max(||x||, eps)  (torch.nn.functional.normalize, dim=1),
 * x float32 or bf16 [rows][d] -> y `out_dtype`; inv_norm [rows] float32 optional. */
int wm_l2_normalize(const void* x, int in_dtype, int rows, int d, float eps, void* y,
                    int out_dtype, float* inv_norm, void* stream);
/* Backward of the above: dx = (dy - y * <dy,y>) * inv_norm ; all float32. */
/* dx (out_dtype WM_F32 or WM_BF16) = (dy (dy_dtype WM_F32 or WM_BF16) - y <dy, y>) * inv_norm (* *scale_dev when non-NULL: the device-resident
 * gradient of the scalar loss the normalised rows feed, so that no separate scaling pass is needed).  A row the forward
 * clamped (||x|| < eps, seen as ||y||^2 < 0.999) gets dx = dy * inv_norm: the clamp passes no gradient to the norm.
 * eps is not an argument here, so a clamped row with ||x|| in [0.9995 eps, eps) is taken for an unclamped one and keeps
 * the projection (relative difference of dx at the most 1: the band where F.normalize itself is discontinuous). */
int wm_l2_normalize_bwd(const void* dy, int dy_dtype, const float* y, const float* inv_norm, int rows, int d,
                        void* dx, int out_dtype, const float* scale_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NT-Xent.  Replaces lightly.loss.NTXentLoss()(z0, z1) at
 *   scripts/WM811k_benchmark.py:234,246
 * zn: L2-normalised local rows [2*b_local][d] float32 (z0 rows then z1 rows);
 * zall: all rows the loss contrasts against, [2][b_global][d] float32 (view-major; == zn when
 *   not gathered); rank_offset = rank * b_local (lightly gather_distributed label offset).
 * Global row id of (view v, sample m) is v*b_global + m; local row (v,i) is global
 * (v, rank_offset+i); its positive is (1-v, rank_offset+i); it is excluded from its own softmax.
 * Forward emits, per local row, lse_i = log sum_{j != i} exp(s_ij/T) and
 * loss_rows_i = lse_i - s_{i,pos(i)}/T  (the loss is their mean: CrossEntropyLoss(mean) over the
 * [2B, 2B-1] logits the reference builds, which are never materialised here).
 * Backward emits d(sum over ALL ranks' losses)/d zn for the local rows, i.e. lightly's
 * GatherLayer semantics (row part + column part):
 *   dzn_i = grad_scale/T * sum_{j != i} (p_ij + p_ji - 2*[j == pos(i)]) * zall_j,
 *   p_ij = exp(s_ij/T - lse_i);  lse_all [2][b_global] holds lse for every global row
 *   (all-gathered when distributed; == lse when not).  grad_scale = dL/dloss / (2*b_local).
 * d % 32 == 0, d <= 256.
 * ------------------------------------------------------------------------------------------- */
int wm_ntxent_fwd(const float* zn, const float* zall, int b_local, int b_global, int rank_offset,
                  int d, float temperature, float* lse, float* loss_rows, void* stream);
/* The backward splits the columns over ~one block per CU; the splits' partial row gradients go to `workspace`
 * (wm_ntxent_bwd_workspace_bytes) and are summed in split order: no atomics, bit-reproducible. */
size_t wm_ntxent_bwd_workspace_bytes(int b_local, int b_global, int d);
int wm_ntxent_bwd(const float* zn, const float* zall, const float* lse_all, int b_local,
                  int b_global, int rank_offset, int d, float temperature, float grad_scale,
                  float* dzn, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ResNet-18 / projection-head building blocks: bf16 NHWC activations, f32
 * accumulation, f32 parameters.  They replace the cuDNN/ATen kernels behind
 *   timm.create_model("resnet18", num_classes=0)      scripts/WM811k_benchmark.py:231
 *   heads.SimCLRProjectionHead(512, 512, 128)          scripts/WM811k_benchmark.py:233
 *   SimCLR.forward / training_step                     scripts/WM811k_benchmark.py:236-248
 *   torch.optim.SGD(lr, momentum 0.9, wd 5e-4)         scripts/WM811k_benchmark.py:250-255
 * Geometry arguments always describe the FORWARD convolution: input x [N][H][W][C], output
 * y [N][P][Q][K], filter R x S, stride 1|2, zero padding `pad`.
 * ------------------------------------------------------------------------------------------- */

/* y = conv(x, w): w_krsc bf16 [K][R][S][C].  K % 64 == 0; C % 64 == 0, or C == 16 with S == 4
 * (the space-to-depth stem).  A Linear layer is the 1x1 convolution with H = W = P = Q = 1. */
int wm_conv2d_fwd(const void* x, const void* w_krsc, void* y, int N, int H, int W, int C, int K,
                  int R, int S, int P, int Q, int stride, int pad, void* stream);
/* The same convolution, also leaving the per-channel (sum, sum of squares) of its bf16 outputs in stat_part: f32
 * [G][stat_tiles][2 statistics][K] (G = N*P*Q / rows_per_group row groups).  Every 128-row output tile STORES its
 * column sums into its own slot (no atomics, nothing to zero); wm_bn_train_fwd_from_stats adds the slots in slot
 * order, so the statistics -- and everything downstream -- are bit-reproducible from run to run.
 * stat_tiles = wm_conv2d_fwd_stats_tiles(same geometry): rows_per_group / 128, except for the persistent stem
 * kernel, whose workgroups sum over their tiles and write one slot each.  rows_per_group % 128 == 0. */
int wm_conv2d_fwd_stats_tiles(int N, int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad,
                              int rows_per_group);
int wm_conv2d_fwd_stats(const void* x, const void* w_krsc, void* y, int N, int H, int W, int C, int K,
                        int R, int S, int P, int Q, int stride, int pad, float* stat_part,
                        int stat_tiles, int rows_per_group, void* stream);
/* dx = conv_transpose(dy, w): w_crsk bf16 [C][R][S][K]; C % 64 == 0. */
int wm_conv2d_dgrad(const void* dy, const void* w_crsk, void* dx, int N, int H, int W, int C, int K,
                    int R, int S, int P, int Q, int stride, int pad, void* stream);
/* dx = conv_transpose(dy, w) + residual: `residual` (bf16, shape of dx) is the gradient that reached
 * the same input through another path (the identity shortcut of a residual block); adding it in the
 * epilogue replaces a separate three-pass elementwise add. */
int wm_conv2d_dgrad_add(const void* dy, const void* w_crsk, const void* residual, void* dx, int N, int H,
                        int W, int C, int K, int R, int S, int P, int Q, int stride, int pad, void* stream);
/* dgrad whose input was relu(BN(bn_y) (+ shortcut)) -- i.e. the convolution that FOLLOWS a BatchNorm + ReLU
 * (timm BasicBlock: conv2 after bn1/act1, and the next block's conv1 after bn2 + shortcut + act2;
 * scripts/WM811k_benchmark.py:231): the epilogue takes the gradient through the ReLU and accumulates the
 * BatchNorm-backward sums, so that BatchNorm's backward needs no reduction pass and no mask:
 *   g  = (conv_transpose(dy, w) (+ residual)) * mask          -> dx (the MASKED gradient, bf16)
 *   stat_part f32 [G][stat_tiles][2][C] = per-tile (sum g, sum g * (bn_y - mean)) per channel, stat_tiles = rows of dx
 *        per group / 128 (plain stores into the tile's slot; wm_bn_train_bwd_from_stats adds the slots in order and
 *        scales the second sum by invstd to sum g * xhat; centred per element, so no cancellation when |mean| >> std)
 * mask = relu_x > 0 when relu_x (the convolution's own forward input, shape of dx) is given; or the bits of relu_mask
 * ([pixels][C / 8] bytes written by wm_bn_train_fwd* for that tensor: 1/16 of its bytes; give one of the two); else
 * recomputed from bn_y as bf16(bn_y * gamma * invstd + beta - mean * gamma * invstd) > 0 (a BatchNorm without shortcut).
 * bn_y has the shape of dx; save_mean / save_invstd [G][C] over G equal groups of images.
 * wm_conv2d_dgrad_bnstat_ok: 1 when the shape is served (every 128-row tile inside one statistics group). */
int wm_conv2d_dgrad_bnstat_ok(int N, int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad,
                              int G);
int wm_conv2d_dgrad_bnstat(const void* dy, const void* w_crsk, const void* residual, void* dx, int N, int H, int W,
                           int C, int K, int R, int S, int P, int Q, int stride, int pad, const void* bn_y,
                           const void* relu_x, const void* relu_mask, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, int G, float* stat_part, int stat_tiles,
                           void* stream);
/* Weight gradient: sum over pixels of dy (x) x, split over pixel ranges.  Split z STORES its partial sums into slab z
 * of dw_slabs (f32 [nsplit][K][R][S][C], nsplit = wm_conv2d_wgrad_splits(same geometry)): no atomics, nothing to zero;
 * wm_wgrad_fold / wm_wgrad_finalize / wm_stem_wgrad_finalize sum the slabs in a fixed order (bit-reproducible). */
int wm_conv2d_wgrad_splits(int N, int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad);
int wm_conv2d_wgrad(const void* dy, const void* x, float* dw_slabs, int N, int H, int W, int C, int K,
                    int R, int S, int P, int Q, int stride, int pad, void* stream);
/* Which kernel serves a launch: the code of the kernel instantiation that the entry points above launch for this
 * pass (0 forward, 1 input gradient, 2 weight gradient), geometry and operand set, or a negative WM_E* where they
 * would refuse it.  The launches choose through the same function and switch on its answer, as the weight-gradient
 * launch and wm_conv2d_wgrad_splits share one plan.  It launches nothing and touches no device.
 *   flags      WM_ROUTE_F_STATS     forward with statistics slots (wm_conv2d_fwd_stats), group_arg = rows_per_group
 *              WM_ROUTE_F_RESIDUAL  a residual / shortcut-gradient operand (fwd_bias_res, dgrad_add, dgrad_bnstat)
 *              WM_ROUTE_F_BIAS      a bias (forward) or a bias gradient (weight gradient)
 *              WM_ROUTE_F_BNB       the BatchNorm-backward epilogue (wm_conv2d_dgrad_bnstat), group_arg = G
 *              WM_ROUTE_F_ACT       the GELU forms (wm_linear_bias_gelu_fwd, wm_linear_dgrad_gelu)
 *   group_arg  rows per statistics group (STATS) or the number of groups G (BNB); else ignored
 * Codes, one per instantiation the host can launch:
 *   WM_ROUTE_PANEL                              the 192-wide panel kernel (panel.hip)
 *   WM_ROUTE_STEM_PATCH                         conv_stem_patch
 *   WM_ROUTE_WGRAD_PATCH64                      conv_wgrad_patch64
 *   WM_ROUTE_PATCH(MODE, BNB)                   conv3x3_patch<MODE, BNB>: (0, 0) forward, (1, 0) and (1, 1) input gradient
 *   WM_ROUTE_IGEMM(BN, CPT, MODE, EPI, BNB)     conv_igemm<128, BN, CPT, MODE, EPI, BNB>, BN 64 or 128:
 *        forward (2, 0, 0, 0) the stem, (8, 0, 0, 0), (8, 0, 1, 0) with bias / residual / GELU;
 *        input gradient (8, 3, 0, 0) stride 1, (8, 2, 0, 0) stride 2 by parity class, (8, 1, 0, 0) any other stride 2,
 *        (8, 3, 1, 0) times gelu', (8, 3, 0, 1) and (8, 2, 0, 1) with the BatchNorm-backward epilogue
 *   WM_ROUTE_WGRAD(BMO, CPT, NT, BIAS)          conv_wgrad<BMO, CPT, NT, BIAS>: (64, 8, 3 | 1), (128, 8, 3 | 2 | 1), each
 *        with BIAS 0 or 1; the stem forms (64, 2, 4 | 1, 0) and (128, 2, 2 | 1, 0) */
#define WM_ROUTE_F_STATS 1
#define WM_ROUTE_F_RESIDUAL 2
#define WM_ROUTE_F_BIAS 4
#define WM_ROUTE_F_BNB 8
#define WM_ROUTE_F_ACT 16
#define WM_ROUTE_PANEL 1
#define WM_ROUTE_STEM_PATCH 2
#define WM_ROUTE_WGRAD_PATCH64 3
#define WM_ROUTE_PATCH(MODE, BNB) (10 + 2 * (MODE) + ((BNB) ? 1 : 0))
#define WM_ROUTE_IGEMM(BN, CPT, MODE, EPI, BNB) \
  (10000 + ((BN) / 64) * 1000 + (CPT) * 100 + (MODE) * 10 + ((EPI) ? 2 : 0) + ((BNB) ? 1 : 0))
#define WM_ROUTE_WGRAD(BMO, CPT, NT, BIAS) (20000 + ((BMO) / 64) * 1000 + (CPT) * 100 + (NT) * 10 + ((BIAS) ? 1 : 0))
int wm_conv2d_route(int pass, int N, int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad,
                    int flags, int group_arg);
/* Forward with y = conv(x) + bias[k] (+ residual, same shape as y), both optional, added in the
 * epilogue: a Linear layer's bias and the residual add of a transformer block cost no extra pass. */
int wm_conv2d_fwd_bias_res(const void* x, const void* w_krsc, const float* bias, const void* residual, void* y,
                           int N, int H, int W, int C, int K, int R, int S, int P, int Q, int stride, int pad,
                           void* stream);
/* Same, and dbias_slabs [nsplit][K] = per-split sums over pixels of dy (may be NULL): a Linear layer's bias gradient
 * comes out of the weight-gradient launch (one extra MFMA per dY fragment in the first column group's blocks)
 * instead of a separate reduction pass over dy. */
int wm_conv2d_wgrad_bias(const void* dy, const void* x, float* dw_slabs, float* dbias_slabs, int N, int H, int W, int C,
                         int K, int R, int S, int P, int Q, int stride, int pad, void* stream);

/* The two Linear layers around a GELU (ViT MLP: dino vision_transformer.py Mlp, torchvision MLPBlock; reference
 * call sites scripts/WM811k_benchmark.py:548-550, :881-899) with the activation inside the GEMM epilogues:
 *   wm_linear_bias_gelu_fwd: pre = x W^T + bias -> pre_out [rows][K] bf16 (kept for the backward pass),
 *                            gelu(pre) -> y [rows][K]            (x [rows][C], w_krsc [K][C] bf16, bias [K] f32)
 *   wm_linear_dgrad_gelu:    dx = (dy W) * gelu'(pre)            (dy [rows][K], w_crsk [C][K] bf16; pre, dx [rows][C])
 * i.e. the input gradient of the layer that FOLLOWS the activation, already taken through the activation.
 * Replaces a separate bias + GELU pass (forward) and a GELU-gradient + column-sum pass (backward). */
int wm_linear_bias_gelu_fwd(const void* x, const void* w_krsc, const float* bias, void* pre_out, void* y, int rows,
                            int C, int K, void* stream);
int wm_linear_dgrad_gelu(const void* dy, const void* w_crsk, const void* pre, void* dx, int rows, int C, int K,
                         void* stream);

/* The whole transformer MLP block in ONE launch, for forward passes that keep nothing for a backward pass (the DINO
 * teacher, kNN / embedding inference, validation): y = fc2(gelu(fc1(x) + b1)) + b2 (+ residual), with the hidden
 * activation living in LDS only (128 token rows per workgroup, 128 hidden units at a time).  x, y, residual
 * [rows][C] bf16; w1_krsc [H][C], w2_krsc [C][H] bf16 (forward layouts); b1 [H], b2 [C] f32.  Bit-identical to
 * wm_linear_bias_gelu_fwd followed by wm_conv2d_fwd_bias_res.  wm_mlp_fused_fwd_ok: 1 for the served shapes (C = 192,
 * H % 128 == 0, rows <= 32 768: ViT-Tiny; one workgroup per CU -- beyond one round of the chip the two launches win). */
int wm_mlp_fused_fwd_ok(int rows, int C, int H);
int wm_mlp_fused_fwd(const void* x, const void* w1_krsc, const float* b1, const void* w2_krsc, const float* b2,
                     const void* residual, void* y, int rows, int C, int H, void* stream);
/* The same with the block's LayerNorm folded in (forward passes that keep nothing for a backward pass): the normalised
 * rows exist only as register fragments of the workgroup that multiplies them.
 *   wm_ln_linear_fwd     y = LayerNorm(x) W^T + bias                      (norm1 -> qkv; served: C = 192, N >= 384, N % 64 == 0)
 *   wm_ln_mlp_fused_fwd  y = fc2(gelu(fc1(LayerNorm(x)) + b1)) + b2 (+ residual)   (norm2 -> MLP; shapes of wm_mlp_fused_fwd)
 * Same arithmetic as wm_layernorm_fwd followed by the unfused launches (two-pass statistics, bf16 rounding of the
 * normalised rows). */
int wm_ln_linear_fwd_ok(int rows, int C, int N);
int wm_ln_linear_fwd(const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w_krsc,
                     const float* bias, void* y, int rows, int C, int N, void* stream);
int wm_ln_mlp_fused_fwd(const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w1_krsc,
                        const float* b1, const void* w2_krsc, const float* b2, const void* residual, void* y, int rows,
                        int C, int H, void* stream);

/* f32 OIHW master weights -> bf16 [K][R][S][C] and/or [C][R][S][K] (either may be NULL). */
int wm_weights_prepare(const float* w_oihw, int K, int C, int R, int S, void* w_krsc, void* w_crsk,
                       void* stream);
/* Batched forms of the two layout passes: one launch for every convolution / Linear parameter of a model.
 * descs (DEVICE, n_desc entries, tile0 ascending).
 * wm_layouts_refresh: w = f32 OIHW master weights [K][C][RS]; krsc / crsk = bf16 [K][RS][C] / [C][RS][K] kernel
 *   layouts (either may be NULL); RS = R*S in {1, 9}; tiles_c = ceil(C / 32); tile0 = index of the parameter's first
 *   32 x 32 (k, c) tile in the launch; total_tiles = sum over parameters of ceil(K / 32) * tiles_c.
 * wm_wgrad_fold: ws = f32 weight-gradient slabs [nsplit][K][RS][C] (wm_conv2d_wgrad), nsplit slabs summed in order;
 *   grad = f32 OIHW gradient (grad += sum); nsplit <= 32: a block owns an 8 x 128 (k, c) tile with all its taps
 *   (tiles_c = ceil(C / 128), tiles = ceil(K / 8) * tiles_c); else a 4 x 64 tile of ONE tap (tiles_c = ceil(C / 64),
 *   tiles = ceil(K / 4) * tiles_c * RS) with the slab range cut in four, summed in order; C % 4 == 0.  Optional bias: w = f32 bias slabs [nsplit][K], krsc = (float*) bias gradient [K]
 *   (+=), both NULL when absent (crsk unused).
 * Replaces 24-100 wm_weights_prepare / 19 wm_wgrad_finalize launches per training step. */
typedef struct WmLayoutDesc {
  const float* w;
  uint16_t* krsc;
  uint16_t* crsk;
  float* ws;
  float* grad;
  int32_t K, C, RS, tiles_c, tile0, nsplit;
} WmLayoutDesc; /* 64 bytes */
int wm_layouts_refresh(const WmLayoutDesc* descs_dev, int n_desc, int total_tiles, void* stream);
int wm_wgrad_fold(const WmLayoutDesc* descs_dev, int n_desc, int total_tiles, void* stream);

/* weight-gradient slabs [nsplit][K][R][S][C] f32 -> OIHW gradient (= or += the sum of the slabs, in order). */
int wm_wgrad_finalize(const float* dw_slabs, int nsplit, int K, int C, int R, int S, float* grad_oihw,
                      int accumulate, void* stream);
/* The 7x7/2 pad-3 stem on 3 channels run as a 4x4/1 pad-2 convolution over the 2x2 space-to-depth
 * image [N][H/2][W/2][16] (channel (dh*2+dw)*3+c, 12 used): weights [K][3][7][7] f32 ->
 * [K][4][4][16] bf16, its gradient back, and the image transform (fmt WM_IMG_NCHW_F32 or
 * WM_IMG_NHWC_BF16 with 3 channels). */
int wm_stem_weights_prepare(const float* w_oihw, int K, void* w_s2d, void* stream);
int wm_stem_wgrad_finalize(const float* dw_s2d_slabs, int nsplit, int K, float* grad_oihw, int accumulate, void* stream);
int wm_image_to_s2d(const void* img, int fmt, int N, int H, int W, void* out, void* stream);
int wm_cast_f32_bf16(const float* x, long long n, void* y, void* stream);

/* BatchNorm over a [rows][C] bf16 tensor cut into G equal row groups with independent statistics
 * (G = 2 reproduces the reference's two separate forward(x0), forward(x1) calls on the
 * concatenated batch).  out = relu?(bn(y) (+ residual)).  running_* are updated once per group in
 * order (torch momentum convention, unbiased variance); save_mean/save_invstd are [G][C].
 * num_batches_tracked (torch's int64 buffer, may be NULL) is incremented by G inside the finalize kernel.
 * relu_mask (may be NULL): [rows][C / 8] bytes, bit e of byte (row, chunk) = output channel 8 chunk + e is > 0 -- the
 * ReLU's backward mask for wm_conv2d_dgrad_bnstat at 1/16 of the tensor's bytes.
 * C % 8 == 0, C <= 2048, rows % G == 0. */
size_t wm_bn_workspace_bytes(long long rows, int C, int G);
int wm_bn_train_fwd(const void* y, const void* residual, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long long* num_batches_tracked, long long rows, int C, int G, float eps,
                    float momentum, int relu, float* save_mean, float* save_invstd, void* out, void* relu_mask,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Training forward whose statistics were accumulated by wm_conv2d_fwd_stats. */
int wm_bn_train_fwd_from_stats(const void* y, const void* residual, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, long long* num_batches_tracked,
                               long long rows, int C, int G, float eps, float momentum, int relu, float* save_mean,
                               float* save_invstd,
                               void* out, void* relu_mask, const float* stat_part, int stat_tiles, void* workspace,
                               size_t workspace_bytes, void* stream);
/* Statistics only: mean / invstd / running stats and the [G][C] scale, shift of the normalisation, for a
 * consumer that applies it itself (the fused stem below).  stat_part NULL: computed from y here. */
int wm_bn_train_stats(const void* y, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, long long* num_batches_tracked, long long rows, int C, int G, float eps, float momentum,
                      float* save_mean, float* save_invstd, float* scale, float* shift, const float* stat_part,
                      int stat_tiles, void* workspace, size_t workspace_bytes, void* stream);
int wm_bn_eval_scale_shift(const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, int C, float eps, float* scale, float* shift, void* stream);
int wm_bn_eval_fwd(const void* y, const void* residual, const float* gamma, const float* beta,
                   const float* running_mean, const float* running_var, long long rows, int C, float eps,
                   int relu, void* out, void* workspace, size_t workspace_bytes, void* stream);
/* dz = dout * mask; dy = dBN(dz); dgamma/dbeta (= or +=); dz is also written when non-NULL (the
 * gradient of the residual branch).  mask: (out_relu > 0) when out_relu is given; else, when
 * relu_from_y != 0, recomputed from y as bf16(y*gamma*invstd + beta - mean*gamma*invstd) > 0 (valid
 * for a ReLU'd BN without residual; saves reading its output); else no ReLU. */
int wm_bn_train_bwd(const void* y, const void* dout, const void* out_relu, int relu_from_y,
                    const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                    long long rows, int C, int G, float* dgamma, float* dbeta, int accumulate, void* dy,
                    void* dz, void* workspace, size_t workspace_bytes, void* stream);
/* Backward whose per-tile sums were stored by wm_conv2d_dgrad_bnstat: g is the gradient ALREADY taken through the ReLU
 * (it is also the gradient of the shortcut branch, if any): add the slots in order, dgamma / dbeta (= or +=), then one
 * pass dy = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)).  workspace >= (7 + 256) * G * C floats. */
int wm_bn_train_bwd_from_stats(const void* y, const void* g, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, long long rows, int C, int G,
                               float* dgamma, float* dbeta, int accumulate, void* dy, const float* stat_part,
                               int stat_tiles, void* workspace, size_t workspace_bytes, void* stream);
/* Synchronised BatchNorm (torch.nn.SyncBatchNorm; the reference's `sync_batchnorm` flag, scripts/WM811k_benchmark.py:62,
 * :1103): statistics over the batches of all ranks.  The library holds no communicator, so each pass is cut at the
 * point where the CALLER all-reduces (sum) a [G][2][C] f32 vector: forward (sum y, sum y^2), backward (sum g,
 * sum g * xhat).  group_count = rows per statistics group summed over the ranks (equal per-rank batches).  dgamma /
 * dbeta stay this rank's local sums, as torch's do (the gradient exchange averages them).  C <= 2048.
 * wm_bn_sync_fwd_sums: stat_part NULL -> computed from y (workspace: wm_bn_workspace_bytes), else the slots of
 * wm_conv2d_fwd_stats.  wm_bn_sync_bwd_sums / _apply: mask arguments as wm_bn_train_bwd. */
int wm_bn_sync_fwd_sums(const void* y, long long rows, int C, int G, const float* stat_part, int stat_tiles,
                        float* sums, void* workspace, size_t workspace_bytes, void* stream);
int wm_bn_sync_fwd_apply(const void* y, const void* residual, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked, long long rows, int C,
                         int G, long long group_count, float eps, float momentum, int relu, float* save_mean,
                         float* save_invstd, void* out, const float* sums, void* workspace, size_t workspace_bytes,
                         void* stream);
int wm_bn_sync_bwd_sums(const void* y, const void* dout, const void* out_relu, int relu_from_y, const float* gamma,
                        const float* beta, const float* save_mean, const float* save_invstd, long long rows, int C,
                        int G, float* dgamma, float* dbeta, int accumulate, float* sums, void* workspace,
                        size_t workspace_bytes, void* stream);
int wm_bn_sync_bwd_apply(const void* y, const void* dout, const void* out_relu, int relu_from_y, const float* gamma,
                         const float* beta, const float* save_mean, const float* save_invstd, long long rows, int C,
                         int G, long long group_count, const float* sums, void* dy, void* dz, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Backward of the fused stem tail max_pool3x3s2(relu(BN(y))): y [N][H][W][C]; the gradient entering
 * the BN is gathered from pooled_dy / pool_idx [N][P][Q][C] inside the apply pass; with ysel (the
 * inputs at the selected positions, from the forward; may be NULL) the per-channel sums run over the
 * pooled tensors alone. */
int wm_bn_relu_maxpool_bwd(const void* y, const void* ysel, const void* pooled_dy, const void* pool_idx, int N,
                           int H, int W, int C, const float* gamma, const float* beta, const float* save_mean,
                           const float* save_invstd, int G, float* dgamma, float* dbeta, int accumulate,
                           void* dy, void* workspace, size_t workspace_bytes, void* stream);
int wm_add_bf16(const void* a, const void* b, long long n, void* out, void* stream);

/* MaxPool2d(3, stride 2, padding 1) with recorded window positions (uint8, first maximum in scan
 * order as torch does), and global average pooling [N][HW][C] -> [N][C]. */
int wm_maxpool3x3s2_fwd(const void* x, int N, int H, int W, int C, void* y, void* idx, void* stream);
/* ResNet stem: maxpool(relu(x*scale + shift)) in one pass (scale/shift [G][C], G groups of N/G
 * images); the normalised 112x112 activation is never materialised.  Same idx semantics. */
int wm_bn_relu_maxpool3x3s2_fwd(const void* x, const float* scale, const float* shift, int N, int H, int W, int C,
                                int G, void* y, void* idx, void* xsel, void* stream);
int wm_maxpool3x3s2_bwd(const void* dy, const void* idx, int N, int H, int W, int C, void* dx, void* stream);
int wm_gap_fwd(const void* x, int N, int HW, int C, void* y, void* stream);
int wm_gap_bwd(const void* dy, int N, int HW, int C, void* dx, void* stream);

/* torch.optim.SGD step over flat f32 arenas: d = g*hyper[3] + hyper[2]*p; buf = hyper[1]*buf + d;
 * p -= hyper[0]*buf.  hyper is a 4-float DEVICE array {lr, momentum, weight_decay, grad_scale} so a
 * captured graph picks up a new learning rate without re-capture. */
int wm_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, const float* hyper,
                void* stream);

/* torch.nn.CrossEntropyLoss(weight) (= nll_loss(log_softmax)) for the supervised baseline and the linear probe
 * (scripts/WM811k_benchmark.py:211-217; src/ssl_wafermap/models/evals.py:20): logits WM_F32 / WM_BF16 [B][C],
 * labels int64 [B] (outside [0, C): ignored), weight [C] or NULL.  acc2[0] += sum w_y nll, acc2[1] += sum w_y
 * (zero both first; loss = acc2[0] / acc2[1]); dlogits [B][C] f32 = w_y (softmax - onehot), to be divided by
 * acc2[1] by the caller. */
int wm_cross_entropy_fwd_bwd(const void* logits, int dtype, const long long* labels, const float* weight, int B, int C,
                             float* acc2, float* dlogits, void* stream);
/* torch.nn.BCEWithLogitsLoss(pos_weight) (multi-label linear probe, evals.py:93): target f32 [B][C], pos_weight [C]
 * or NULL; loss[0] += mean (zero it first); dlogits [B][C] f32 = d loss / d logits. */
int wm_bce_logits_fwd_bwd(const void* logits, int dtype, const float* target, const float* pos_weight, int B, int C,
                          float* loss, float* dlogits, void* stream);

/* lightly.loss.NegativeCosineSimilarity (BYOL, SimSiam: scripts/WM811k_benchmark.py:446,613):
 * loss[0] += -mean_i cos(x0_i, x1_i) (zero it first; norms clamped at eps as torch.cosine_similarity does);
 * dx0 / dx1 [B][D] float32 gradients, either may be NULL.  x0, x1: WM_F32 or WM_BF16 [B][D]. */
int wm_neg_cosine_fwd_bwd(const void* x0, const void* x1, int dtype, int B, int D, float eps, float* loss, float* dx0,
                          float* dx1, void* stream);

/* lightly.loss.DCLLoss / DCLWLoss (decoupled contrastive learning; the reference's DCLW model,
 * scripts/WM811k_benchmark.py:258-287): z0, z1 L2-normalised [B][D] float32.  Per direction (a, b) and row i:
 * -w_i <a_i,b_i>/T + lse_{k!=i} <a_i,a_k>/T + lse_{k!=i} <a_i,b_k>/T, averaged over rows and both directions;
 * w_i = 1, or 2 - B softmax_i(<z0_i,z1_i>/sigma) when weighted.  loss[0] += the loss (zero it first);
 * dz0, dz1 [B][D] gradients.  Workspace: wm_dcl_workspace_bytes(B). */
size_t wm_dcl_workspace_bytes(int B);
int wm_dcl_fwd_bwd(const float* z0, const float* z1, int B, int D, float temperature, float sigma, int weighted,
                   float* loss, float* dz0, float* dz1, void* workspace, size_t workspace_bytes, void* stream);

/* lightly.loss.BarlowTwinsLoss on the cross-correlation matrix (scripts/WM811k_benchmark.py:364-366):
 * raw_cc [D][D] f32 = sum over the batch of za_norm (x) zb_norm (wm_conv2d_wgrad on the two standardised
 * projections); c = scale * raw_cc; loss[0] += diag_weight sum_i (c_ii - 1)^2 + lambda sum_{i!=j} c_ij^2 (zero it
 * first); draw_cc = d loss / d raw_cc.  Barlow Twins: diag_weight 1; VICReg's covariance term: diag_weight 0,
 * lambda 1/D, scale 1/(N-1) on the covariance of the centred projection. */
int wm_barlow_twins_fwd_bwd(const float* raw_cc, int D, float scale, float lambda, float diag_weight, float* loss,
                            float* draw_cc, void* stream);
/* VICReg pieces (lightly.loss.VICRegLoss, scripts/WM811k_benchmark.py:401): out = z - mean (bf16 [rows][C]);
 * variance term loss[0] += mean_d relu(1 - sqrt(var_biased_d N/(N-1) + eps)) with coef[d] such that
 * d term / d centred[n][d] = coef[d] * centred[n][d]. */
int wm_center_columns(const void* z, const float* mean, long long rows, int C, void* out, void* stream);
int wm_vicreg_variance(const float* var_biased, int N, int D, float eps, float* loss, float* coef, void* stream);

/* lightly's SwaV Sinkhorn-Knopp (scripts/WM811k_benchmark.py:832-834 via lightly.loss.SwaVLoss): out WM_F32 / WM_BF16
 * [B][K] prototype scores; Q [B][K] f32 = the transport plan (rows sum to 1) after `iters` rounds at
 * temperature eps (iters = 0: exp(out / eps) * B / sum, lightly's initial normalisation alone); workspace: B + K floats. */
int wm_sinkhorn(const void* out, int dtype, int B, int K, float eps, int iters, float* Q, float* workspace,
                void* stream);

/* NT-Xent against a memory bank (lightly NTXentLoss(memory_bank_size > 0), the reference's MoCo:
 * scripts/WM811k_benchmark.py:305-307).  q, kpos: L2-normalised [B][D] float32; bank [D][K] float32
 * (lightly's layout, one stored key per column).  logits_i = [<q_i,kpos_i>, <q_i,bank>] / T, label 0.
 * loss[0] += mean CE (zero it first); dq, dk [B][D] = d loss / d q, d kpos.  K + 2 D <= 16384. */
int wm_ntxent_bank_fwd_bwd(const float* q, const float* kpos, const float* bank, int B, int D, int K,
                           float temperature, float* loss, float* dq, float* dk, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vision-transformer path (SURVEY §8 a13 DINOViT, a14 MAE).
 * Replaces, in the reference: the facebookresearch/dino `dino_vits16` backbone called at
 * scripts/WM811k_benchmark.py:548-550,566-576 (MixedWM38_pretrain.py:141-143), torchvision's
 * vit_b_32 inside lightly's MAEBackbone/MAEDecoder (:881-899, :903-947), lightly.loss.DINOLoss
 * (:564,586), lightly.models.utils.update_momentum (:579-581), torch.optim.AdamW (:591-598) and
 * torch.nn.MSELoss on the masked patches (:900,949-954).
 * Activations are bf16 [rows][C] (rows = tokens, token-major); parameters float32.
 * ------------------------------------------------------------------------------------------- */

/* nn.LayerNorm over the last dim (biased variance, two-pass in registers).  C % 8 == 0, C <= 2048.
 * mean / rstd [rows] are saved for the backward.  dgamma / dbeta are ACCUMULATED (f32 atomics). */
int wm_layernorm_fwd(const void* x, const float* gamma, const float* beta, float eps, long long rows, int C,
                     void* y, float* mean, float* rstd, void* stream);
int wm_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd,
                     long long rows, int C, void* dx, float* dgamma, float* dbeta, void* stream);
/* Same with the gradient of the residual connection around the normalised branch (x -> LN -> f -> + x; timm / dino
 * Block.forward, the reference's DINOViT backbone, scripts/WM811k_benchmark.py:548-550) added in the same pass:
 * dx = bf16(LN'(dy)) + dres, dres bf16 [rows][C].  Replaces the accumulation pass autograd runs for the two uses of x. */
int wm_layernorm_bwd_add(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd,
                         long long rows, int C, const void* dres, void* dx, float* dgamma, float* dbeta, void* stream);
/* LayerNorm backward with the parameter-gradient sums as per-block SLOTS instead of f32 atomics (bit-reproducible):
 * part [2][wm_layernorm_bwd_blocks(rows, C)][C] f32 -- the dgamma slots, then the dbeta slots, every slot overwritten; the
 * caller adds them in slot order (wm_wgrad_fold / wm_wgrad_finalize with K = 1, RS = 1).  dres as in
 * wm_layernorm_bwd_add, may be NULL. */
/* Column sums likewise: wm_bias_act_bwd_parts = wm_bias_act_bwd with the bias gradient as per-block slots
 * part [wm_colsum_blocks(rows, C)][C] f32 (act WM_ACT_NONE: the plain column sum of dy; x, bias, dx unused). */
int wm_colsum_blocks(long long rows, int C);
int wm_bias_act_bwd_parts(const void* x, const float* bias, const void* dy, int act, long long rows, int C, void* dx,
                          float* part, void* stream);
int wm_layernorm_bwd_blocks(long long rows, int C);
int wm_layernorm_bwd_parts(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd,
                           long long rows, int C, const void* dres, void* dx, float* part, void* stream);

/* y = act(x + bias) (+ residual).  act: 0 identity, 1 exact GELU (erf), 2 ReLU (the bias-carrying heads:
 * lightly MoCoProjectionHead), 3 Mish x tanh(softplus(x)), softplus(x) = x above 20 as in torch (nn.Mish of the
 * reference's TwoLayerMultilabelClassifier, src/ssl_wafermap/models/evals.py:155-165).  bias / residual may be NULL. */
#define WM_ACT_NONE 0
#define WM_ACT_GELU 1
#define WM_ACT_RELU 2
#define WM_ACT_MISH 3
int wm_bias_act_fwd(const void* x, const float* bias, const void* residual, int act, long long rows, int C,
                    void* y, void* stream);
/* dx = dy * act'(x + bias) (dx may be NULL for act 0: only the bias gradient is wanted);
 * dbias[C] += column sums of dx (NULL: skipped). */
int wm_bias_act_bwd(const void* x, const float* bias, const void* dy, int act, long long rows, int C, void* dx,
                    float* dbias, void* stream);
/* out[C] (+)= sum over rows of x[rows][C] (bf16 in, f32 out). */
int wm_colsum_bf16(const void* x, long long rows, int C, float* out, int accumulate, void* stream);

/* tokens[n][0] = cls + pos[0]; tokens[n][1+i] = patches[n][i] + pos[1+i]  (cls [D], pos [1+np][D] f32). */
int wm_tokens_assemble(const void* patches, const float* cls, const float* pos, int N, int np, int D, void* tokens,
                       void* stream);
/* images [N][S][S][3] bf16 -> rows [N*(S/p)^2][p*p*3] in (ph, pw, c) order: the patch-embedding
 * convolution (kernel = stride = p) becomes a GEMM against the [D][p][p][3] weight layout. */
int wm_patchify(const void* images, int N, int S, int p, void* rows, void* stream);

/* Multi-head self-attention, head_dim 64 or 32, S <= 256, softmax(scale * q k^T) v.
 * qkv [B][S][3][H][head_dim] (the qkv / in_proj Linear's output as is), out / dout [B][S][H][head_dim],
 * lse [B][H][S] f32.  bwd writes dqkv in the layout of qkv. */
int wm_attention_fwd(const void* qkv, int B, int S, int H, int head_dim, float scale, void* out, float* lse,
                     void* stream);
int wm_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, int B, int S, int H,
                     int head_dim, float scale, void* dqkv, void* stream);

/* Row gather / scatter on [B][S][C] bf16 by per-batch token indices idx [B][K] (int64, as
 * torch.argsort returns): lightly's get_at_index / set_at_index.  scatter writes only the indexed
 * rows (caller pre-fills the rest). */
int wm_gather_rows(const void* x, const long long* idx, int B, int S, int K, int C, void* out, void* stream);
int wm_scatter_rows(const void* src, const long long* idx, int B, int S, int K, int C, void* dst, void* stream);

/* MSE over n elements: loss[0] = mean((pred - target)^2); dpred = 2 (pred - target) / n (bf16).
 * loss must be zeroed by the caller. */
int wm_mse_fwd_bwd(const void* pred, const void* target, long long n, float* loss, void* dpred, void* stream);
/* torch.nn.L1Loss() (SimMIM, scripts/WM811k_benchmark.py:976): loss[0] += mean |pred - target|; dpred = sign / n. */
int wm_l1_fwd_bwd(const void* pred, const void* target, long long n, float* loss, void* dpred, void* stream);

/* DINO loss (lightly.loss.DINOLoss).  teacher [Vt*B][D] bf16 -> probs f32 = softmax((t - center)/temp_t). */
int wm_dino_teacher_probs(const void* teacher, const float* center, float temp_t, long long rows, int D,
                          float* probs, void* stream);
/* student [Vs][B][D] bf16, probs [Vt][B][D]: loss[0] += sum_{t != s} -<probs_t, log_softmax(student_s/temp_s)>
 * / (n_terms * B); dstudent = d loss / d student (bf16).  Views with equal index are the same crop. */
int wm_dino_loss_fwd_bwd(const void* student, const float* probs, int Vs, int Vt, int B, int D, float temp_s,
                         float* loss, void* dstudent, void* stream);
/* Cross-entropy against soft targets (MSN / PMSN, scripts/WM811k_benchmark.py:684,705): student [Vs][B][D] bf16 logits,
 * probs [B][D] f32 targets shared by the Vs views; loss[0] += mean over (view, sample) of
 * -<probs_b, log_softmax(student_vb / temp_s)>; dstudent bf16. */
int wm_soft_cross_entropy_fwd_bwd(const void* student, const float* probs, int Vs, int B, int D, float temp_s,
                                  float* loss, void* dstudent, void* stream);
/* Mean-entropy regulariser of lightly's MSNLoss / PMSNLoss on logits [N][K] bf16: p = softmax(logits / T),
 * m = mean over rows; loss[0] += sum_k m_k (log m_k - log_prior_k) (log_prior NULL: MSN's me-max term
 * sum m log m); dlogits [N][K] f32; mean_ws: K floats of scratch. */
int wm_mean_entropy_reg_fwd_bwd(const void* logits, const float* log_prior, int N, int K, float temperature,
                                float* loss, float* dlogits, float* mean_ws, void* stream);
/* center = momentum * center + (1 - momentum) * mean over rows of teacher[rows][D]. */
int wm_dino_center_update(const void* teacher, long long rows, int D, float momentum, float* center, void* stream);

/* Column statistics and standardisation of a feature matrix x [rows][C] (float32 or bf16: WM_F32 /
 * WM_BF16), the sklearn StandardScaler the reference applies to dumped embeddings
 * (notebooks/3.0-Embeddings-inference.ipynb cell 7): mean[c], var[c] = biased variance (two passes:
 * sums, then squared deviations from the mean).  mean and var must be zeroed by the caller.
 * wm_standardize: out[r][c] = (x[r][c] - mean[c]) * inv_scale[c], float32. */
int wm_colstats(const void* x, int dtype, long long rows, int C, float* mean, float* var, void* stream);
int wm_standardize(const void* x, int dtype, long long rows, int C, const float* mean, const float* inv_scale,
                   float* out, void* stream);

/* torch.optim.AdamW / Adam step over flat f32 arenas; hyper = DEVICE {lr, beta1, beta2, eps, weight_decay,
 * bias_correction1, bias_correction2, grad_scale, l2_mode}: l2_mode 0 = decoupled decay (AdamW), 1 = the
 * decay added to the gradient (torch.optim.Adam). */
int wm_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                  const float* hyper, void* stream);
/* lightly update_momentum: ema = ema * m + p * (1 - m). */
int wm_ema_update(float* ema, const float* params, long long n, float m, void* stream);
/* out[r][:] = ascending argsort of keys[r][0..S) (S <= 256; ties to the lower index): the token permutation of
 * lightly.models.utils.random_token_mask (reference scripts/WM811k_benchmark.py:930, MixedWM38_pretrain.py:208). */
int wm_argsort_rows(const float* keys, int rows, int S, long long* out, void* stream);
/* y = x * g[column] on bf16 [rows][C] with f32 g[C], and its backward (dx = dy * g, dg = / += column sums of dy * x):
 * the trainable gain of the weight-normalised last layer of lightly's DINOProjectionHead(norm_last_layer=False)
 * (reference scripts/WM811k_benchmark.py:553-559). */
int wm_colscale_fwd(const void* x, const float* g, long long rows, int C, void* y, void* stream);
int wm_colscale_bwd(const void* x, const float* g, const void* dy, long long rows, int C, void* dx, float* dg,
                    int accumulate, void* stream);

/* timm.optim.lars.Lars step (BarlowTwins / VICReg in the reference, scripts/WM811k_benchmark.py:383-392,
 * 418-427) over a flat arena: seg_offsets [n_seg + 1] int64 = element offsets of the parameters; per parameter
 * r = trust_coeff |w| / (|g| + wd |w| + eps) (1 if either norm is 0; no adaptation when wd == 0),
 * g <- (g + wd w) r, buf = momentum buf + g, p -= lr buf.  hyper (device) = {lr, momentum, weight_decay,
 * trust_coeff, eps, grad_scale}; norms_ws: 2 * n_seg floats of scratch. */
int wm_lars_step(float* params, const float* grads, float* momentum_buf, const long long* seg_offsets, int n_seg,
                 const float* hyper, float* norms_ws, void* stream);

/* Small float32 matmul c [M][N] = op(a) b, op(a) = a [M][K] (trans_a = 0) or a^T with a stored [K][M] (trans_a = 1);
 * b [K][N]; row-major.  The positional-embedding resize of dino / lightly (interpolate_pos_encoding, reference call
 * sites scripts/WM811k_benchmark.py:548-550, utilities via lightly MAEBackbone) as a fixed matrix product, and its
 * gradient. */
int wm_matmul_f32(const float* a, const float* b, float* c, int M, int N, int K, int trans_a, void* stream);

/* ---- Float32 "parity" preset (csrc/f32path.hip): the forward pass (and, below, the backward pieces) of the SimCLR / DINO /
 * MAE steps with every activation, weight and accumulator in float32 (reference call sites scripts/WM811k_benchmark.py:236-248,
 * :578-588, :902-947).  The production kernels keep activations in bf16; profiles/r04_error_budget_bf16.md shows that storage
 * puts the step losses 0.4e-4 .. 3.4e-4 from the float32 reference (north_star: 1e-4).  These entry points keep them in
 * float32: a validation preset (forward for all three models; backward for the ResNet-18 / head ops and the MAE / SimMIM
 * transformer ops), selected by ssl_wafermap_amd.precision("float32").  Activations NHWC float32 / [rows][C]. */
size_t wm_f32_conv2d_workspace_bytes(int C, int K, int R, int S);
/* y = act(conv(x, w) + bias) + residual: x [N][H][W][C], w_oihw [K][C][R][S] (the float32 master layout), bias [K] or NULL,
 * residual [N][P][Q][K] or NULL, act 0 none / 1 GELU (erf) / 2 ReLU.  A Linear layer is the 1x1 case on a 1x1 image. */
int wm_f32_conv2d_fwd(const float* x, const float* w_oihw, const float* bias, const float* residual, float* y, int N, int H,
                      int W, int C, int K, int R, int S, int P, int Q, int stride, int pad, int act, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t wm_f32_bn_workspace_bytes(long long rows, int C, int G);
/* out = relu?(BN(y) (+ residual)) over G equal row groups with their own batch statistics (training != 0: running
 * statistics and the batch counter are updated as by G consecutive nn.BatchNorm calls) or with the running statistics. */
int wm_f32_bn_fwd(const float* y, const float* residual, const float* gamma, const float* beta, float* running_mean,
                  float* running_var, long long* num_batches_tracked, long long rows, int C, int G, int training, float eps,
                  float momentum, int relu, float* save_mean, float* save_invstd, float* out, void* workspace,
                  size_t workspace_bytes, void* stream);
int wm_f32_maxpool3x3s2(const float* x, int N, int H, int W, int C, float* y, void* stream);
int wm_f32_gap(const float* x, int N, int HW, int C, float* y, void* stream);
int wm_f32_layernorm(const float* x, const float* gamma, const float* beta, float eps, long long rows, int C, float* y,
                     void* stream);
/* y = act(x + bias) + residual, element-wise on [rows][C] (bias, residual optional). */
int wm_f32_bias_act(const float* x, const float* bias, const float* residual, int act, long long rows, int C, float* y,
                    void* stream);
/* softmax(q k^T * scale) v per (image, head): qkv [B*S][3][H][HD] -> out [B*S][H*HD]; HD 64 or 32. */
int wm_f32_attention(const float* qkv, int B, int S, int H, int HD, float scale, float* out, void* stream);
/* rows of softmax((x - subtract) * inv_temp) (log_softmax != 0: its logarithm); subtract [D] or NULL. */
int wm_f32_softmax_rows(const float* x, const float* subtract, float inv_temp, int log_softmax, long long rows, int D,
                        float* y, void* stream);
/* pair_loss[(t * SV + s) * B + b] = -sum_d probs[t][b][d] * logq[s][b][d], 0 where t == s (lightly DINOLoss's zeroed diagonal). */
int wm_f32_pair_ce(const float* probs, const float* logq, int T, int SV, int B, int D, float* pair_loss, void* stream);
/* *out = scale * sum_i f(a_i, b_i): mode 0 a_i, 1 (a_i - b_i)^2, 2 |a_i - b_i|; one ordered double-precision sum. */
int wm_f32_reduce(const float* a, const float* b, long long n, int mode, double scale, float* out, void* stream);
/* Backward pieces of the convolution / BatchNorm / pooling / Linear path (the float32 preset can take a whole SimCLR optimiser
 * step: scripts/WM811k_benchmark.py:242-255).  dx [N][H][W][C] = input gradient of wm_f32_conv2d_fwd for dy [N][P][Q][K];
 * dw_oihw [K][C][R][S] = its weight gradient (pixel ranges summed in a fixed order; workspace from
 * wm_f32_conv2d_wgrad_workspace_bytes); wm_f32_colsum: bias gradients. */
int wm_f32_conv2d_dgrad(const float* dy, const float* w_oihw, float* dx, int N, int H, int W, int C, int K, int R, int S, int P,
                        int Q, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
size_t wm_f32_conv2d_wgrad_workspace_bytes(int N, int P, int Q, int C, int K, int R, int S);
int wm_f32_conv2d_wgrad(const float* dy, const float* x, float* dw_oihw, int N, int H, int W, int C, int K, int R, int S, int P,
                        int Q, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
int wm_f32_colsum(const float* x, long long rows, int C, float* out, void* stream);
/* BatchNorm (training statistics, G groups) backward: gm = dout taken through the ReLU where out_relu (the forward's output)
 * is given; dgamma / dbeta [C] (sums over all groups), dy = gamma * invstd * (gm - mean(gm) - xhat * mean(gm * xhat)), dz (optional)
 * = gm, the gradient of the residual branch.  Workspace: wm_f32_bn_workspace_bytes. */
int wm_f32_bn_bwd(const float* y, const float* dout, const float* out_relu, const float* gamma, const float* save_mean,
                  const float* save_invstd, long long rows, int C, int G, float* dgamma, float* dbeta, float* dy, float* dz,
                  void* workspace, size_t workspace_bytes, void* stream);
int wm_f32_maxpool3x3s2_bwd(const float* x, const float* dy, int N, int H, int W, int C, float* dx, void* stream);
int wm_f32_gap_bwd(const float* dy, int N, int HW, int C, float* dx, void* stream);
/* Backward pieces of the transformer path (the float32 preset can take whole MAE / SimMIM optimiser steps:
 * scripts/WM811k_benchmark.py:876-957, :960-1030).  No float atomics: sums over rows go through per-block slots added in a
 * fixed order, so two runs give the same bits.
 * wm_f32_layernorm_bwd: input gradient dx of wm_f32_layernorm for dy [rows][C] (statistics recomputed as the forward takes
 * them); dgamma / dbeta [C] (either may be NULL) = sum dy * xhat, sum dy.  Workspace: wm_f32_layernorm_bwd_workspace_bytes. */
size_t wm_f32_layernorm_bwd_workspace_bytes(long long rows, int C);
int wm_f32_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, long long rows, int C, float* dx,
                         float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* dx = dy * act'(x + bias) on [rows][C] (bias optional): act 1 exact GELU (Phi(v) + v phi(v)), 2 ReLU, 0 copies dy.  The bias
 * gradient is wm_f32_colsum of dx; a fused-GELU Linear passes its recomputed pre-activation as x. */
int wm_f32_bias_act_bwd(const float* x, const float* bias, const float* dy, int act, long long rows, int C, float* dx,
                        void* stream);
/* Gradient of wm_f32_attention: qkv [B*S][3][H][HD], out [B*S][H*HD] (the forward's output), dout [B*S][H*HD]
 * -> dqkv [B*S][3][H][HD].  One workgroup per (image, head): a query pass (dq) then a key pass (dk, dv); HD 64 or 32, LDS
 * (2 * S * HD + 3 * S) floats (WM_EUNSUPPORTED beyond 160 KiB). */
int wm_f32_attention_bwd(const float* qkv, const float* out, const float* dout, int B, int S, int H, int HD, float scale,
                         float* dqkv, void* stream);
/* Gradient of wm_f32_reduce's losses: dpred = f'(pred - target) * scale * g, mode 1 (squared difference) f' = 2 (pred - target),
 * mode 2 (absolute difference) f' = sign(pred - target); g = *grad_out (device scalar) or 1 when grad_out is NULL. */
int wm_f32_loss_bwd(const float* pred, const float* target, long long n, int mode, double scale, const float* grad_out,
                    float* dpred, void* stream);
/* center = center * momentum + (1 - momentum) * column mean of teacher [rows][D]. */
int wm_f32_center_update(float* center, const float* teacher, int rows, int D, float momentum, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Downstream evaluation (scripts/MixedWM38_evals.py, src/ssl_wafermap/models/evals.py:80-165).
 *
 * Per-label AUROC of multi-label scores: torchmetrics MultilabelAUROC(num_labels, average=None, thresholds=None), the
 * metric of the reference's probes (evals.py:88-96, MixedWM38_evals.py:103-111).  scores [rows][L] (WM_F32 / WM_BF16,
 * row-major), targets [rows][L] int8 (non-zero = positive).  When any score lies outside [0, 1] every score is replaced
 * by its float32 sigmoid first (torchmetrics' rule).  auc[l] = U / (P Q), U = #{(pos, neg): s_pos > s_neg} + #ties / 2,
 * counted exactly in 64-bit integers (same bits on every call); a label without positives or without negatives gets 0.
 * pos_count [L] (may be NULL) receives P per label.  rows * L < 2^31, L <= 1024.
 * Workspace: wm_multilabel_auroc_workspace_bytes(rows, L). */
size_t wm_multilabel_auroc_workspace_bytes(int rows, int L);
int wm_multilabel_auroc(const void* scores, int dtype, const int8_t* targets, int rows, int L, double* auc, int* pos_count,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Inverted dropout (torch.nn.Dropout(p) in training mode, evals.py:162): element i is kept when
 * rand01(seed, i) >= p (the counter RNG of the augmentation kernel's DieNoise) and scaled by 1 / (1 - p); p = 1 gives
 * zeros.  x, y [n] WM_F32 / WM_BF16 (y may equal x), n <= 2^32, 0 <= p <= 1.  The backward pass regenerates the mask
 * from (seed, i): dx = dy * mask / (1 - p), no mask is stored. */
int wm_dropout_fwd(const void* x, int dtype, long long n, float p, uint32_t seed, void* y, void* stream);
int wm_dropout_bwd(const void* dy, int dtype, long long n, float p, uint32_t seed, void* dx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Model inspection (notebooks/2.0-Figures-DINO-attention.ipynb, notebooks/2.0-Figures-GradCAM.ipynb).  No atomics:
 * two calls give the same bits.
 *
 * Attention probabilities softmax(scale q k^T) per head: dino's VisionTransformer.get_last_selfattention, which the
 * attention notebook calls on the last block (with visualize_attention.py's maps of the class-token row).  qkv
 * [B][S][3][H][head_dim] (WM_BF16 or WM_F32, 16-byte aligned), head_dim 64 or 32, S <= 256.  probs float32
 * [B][H][R][S] (16-byte aligned), R = S, or R = 1 when cls_only (the class-token row only; equal to row 0 of the full
 * output bit for bit).  bf16 scores come from the same MFMA products as wm_attention_fwd's. */
int wm_attention_probs(const void* qkv, int dtype, int B, int S, int H, int head_dim, float scale, int cls_only,
                       float* probs, void* stream);
/* visualize_attention.py --threshold: per row of attn [rows][ld] (float32), over entries 0..n-1: keep[row][i] = 1 when
 * sum_{j: a_j < a_i or (a_j = a_i and j <= i)} a_j / sum_j a_j > 1 - threshold (the stable ascending sort + cumsum of
 * the reference, summed in double), else 0.  keep uint8 [rows][n].  n <= 256, ld >= n, 0 <= threshold <= 1. */
int wm_attention_mass_mask(const float* attn, long long rows, int n, long long ld, double threshold, uint8_t* keep,
                           void* stream);
/* pytorch_grad_cam EigenCAM (get_2d_projection + BaseCAM + scale_cam_image) of backbone.layer4[-1] activations, as the
 * GradCAM notebook runs it.  act [N][H][W][C] memory (channels_last [N,C,H,W]; WM_BF16 or WM_F32), H * W <= 64.  Per
 * image: NaN -> 0; A = activations [HW][C] minus the per-channel mean; p = A v1 = sqrt(lambda1) u1 from the leading
 * eigenpair of A A^T (cyclic Jacobi in double); the sign of p chosen so that sum_i p_i r_i >= 0, r_i = the channel
 * sum of the uncentred activations at position i; ReLU; x -= min, x /= 1e-7 + max; bilinear resize to out_h x out_w
 * (half-pixel centres, edges clamped: F.interpolate(mode="bilinear", align_corners=False)); min-max again.  An image
 * with lambda1 = 0 gives zeros.  cam float32 [N][out_h][out_w], out_h, out_w <= 4096. */
int wm_eigencam(const void* act, int dtype, int N, int C, int H, int W, int out_h, int out_w, float* cam, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Embedding clustering (notebooks/3.1-Embeddings-clustering.ipynb, 3.2-Embeddings-SSL-categories.ipynb: HDBSCAN on the
 * dumped embeddings, scored by silhouette).  x float32 [n][d] row-major, 16-byte aligned, d % 4 == 0, d <= 1024.
 * metric 0: Euclidean sqrt(sum (a_k - b_k)^2); 1: Manhattan sum |a_k - b_k| -- accumulated in float32 in index order from
 * the differences themselves, so dist(i, j) and dist(j, i) are the same bits, equal rows are at distance exactly 0 and
 * the relative error is at most (d + 3) * 2^-24 (csrc/cluster.hip).  No floating-point atomics and none on global memory
 * (wm_rank_query adds integers in LDS, nothing else is atomic): two calls give the same bits.
 *
 * wm_core_distance: out[i] = k-th smallest of dist(i, j) over all rows j, i itself included (so k = 1 gives 0:
 * sklearn.cluster.HDBSCAN's min_samples convention).  1 <= k <= 64, k <= n. */
size_t wm_core_distance_workspace_bytes(int n, int d, int k);
int wm_core_distance(const float* x, int n, int d, int metric, int k, float* out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* One Boruvka round on the mutual-reachability graph w_ij = max(core[i], core[j], dist(i, j) * inv_alpha): for every row
 * i the smallest w_ij over the rows j with comp[j] != comp[i] (comp: int32 component id per row) and that j; equal
 * weights resolve to the lowest j.  A row whose component holds every row gets out_j = -1, out_w = +inf. */
size_t wm_mreach_min_edge_workspace_bytes(int n, int d);
int wm_mreach_min_edge(const float* x, const float* core, const int32_t* comp, int n, int d, int metric, float inv_alpha,
                       float* out_w, int32_t* out_j, void* workspace, size_t workspace_bytes, void* stream);
/* out[i][c] = sum over the rows j with labels[j] == c of dist(i, j) (sklearn.metrics.silhouette_samples' reduction):
 * float32 distances added in double in column order.  labels int32 in [-1, n_clusters); rows labelled -1 contribute
 * nowhere and their own output rows are unspecified.  2 <= n_clusters <= n; out double [n][n_clusters].  Fastest when
 * equal labels are adjacent (one running sum per cluster and row). */
int wm_cluster_dist_sums(const float* x, const int32_t* labels, int n, int d, int metric, int n_clusters, double* out,
                         void* stream);

/* The exact k-nearest-neighbour graph under the same distance function: dist float32 [n][k] and idx int32 [n][k], every
 * row ordered by (distance, index) ascending with the row itself among its own candidates (so dist[i][0] = 0).
 * 1 <= k <= 64, k <= n (k > n: WM_EINVAL). */
size_t wm_knn_graph_workspace_bytes(int n, int d, int k);
int wm_knn_graph(const float* x, int n, int d, int metric, int k, float* dist, int32_t* idx, void* workspace,
                 size_t workspace_bytes, void* stream);
/* The rectangular form: for every row of xq float32 [m][d] its k nearest rows of x float32 [n][d] under the same
 * distance function, dist float32 [m][k] and idx int32 [m][k] in [0, n), every row ordered by (distance, index).
 * m >= 1, 1 <= k <= 64, k <= n (k > n: WM_EINVAL); xq, x and the workspace 16-byte aligned.  With xq = x it returns
 * wm_knn_graph's bits. */
size_t wm_knn_query_workspace_bytes(int m, int n, int d, int k);
int wm_knn_query(const float* xq, int m, const float* x, int n, int d, int metric, int k, float* dist, int32_t* idx,
                 void* workspace, size_t workspace_bytes, void* stream);
/* The fitted row nearest to a new row in mutual reachability (HDBSCAN's prediction for new rows): for every row i of
 * xq float32 [m][d] with core distance core_q[i], over all rows c of x float32 [n][d] with core distances core[c],
 * w_ic = max(core_q[i], core[c], dist(i, c) * inv_alpha) under the same distance function; the result is the c that
 * minimises (w_ic, dist(i, c), c) lexicographically: out_w, out_dist float32 [m] and out_j int32 [m] in [0, n).  An exact
 * search over all n rows.  m, n >= 1, inv_alpha > 0; xq, x and the workspace 16-byte aligned.  No atomics: two calls give
 * the same bits. */
size_t wm_mreach_query_workspace_bytes(int m, int n, int d);
int wm_mreach_query(const float* xq, const float* core_q, int m, const float* x, const float* core, int n, int d, int metric,
                    float inv_alpha, float* out_w, float* out_dist, int32_t* out_j, void* workspace, size_t workspace_bytes,
                    void* stream);
/* Per group of columns the nearest one (HDBSCAN's soft clustering: the nearest exemplar of every cluster): for every row
 * i of xq float32 [m][d] and every group c in [0, g), out_dist[i][c] = the smallest dist(xq_i, xe_j) over the rows j of
 * xe float32 [e][d] with group[j] == c under the same distance function (bit-equal to what wm_knn_query returns for the
 * pair; exactly 0 for a row bit-equal to xe_j) and out_j[i][c] = the lowest j that attains it; a group without a column
 * gives +inf / -1.  Precondition: group int32 [e] is non-decreasing with values in [0, g); with a decreasing sequence or
 * a value outside the range the outputs are unspecified (such a column is never used as an index: no access leaves the
 * buffers).  out_dist float32 [m][g], out_j int32 [m][g].  m, e, g >= 1; xq, xe and the workspace 16-byte aligned.  The
 * workspace is one [m][g] plane of (distance, index) per column slice, at most 16 slices (16 * m * g * 8 bytes) and
 * nothing but padding when the rows alone fill the machine (m > 65 472).  No atomics, no memset: two calls give the same
 * bits. */
size_t wm_group_min_dist_workspace_bytes(int m, int e, int d, int g);
int wm_group_min_dist(const float* xq, int m, const float* xe, const int32_t* group, int e, int d, int metric, int g,
                      float* out_dist, int32_t* out_j, void* workspace, size_t workspace_bytes, void* stream);

/* DBCV (density-based cluster validity, Moulavi et al. 2014; DESIGN.md states the definition): its three all-pairs parts
 * under the same distance function.  All take rows SORTED BY GROUP: group int32, non-decreasing, values in [0, g); with
 * another sequence the outputs are unspecified (no access leaves the buffers).  The square ones walk, per row tile, only
 * the column tiles of that tile's own groups: the cost is the sum of n_c^2 over the groups, not n^2.  The workspace-size
 * functions return 0 for sizes that are not supported.  No atomics: two calls give the same bits.
 *
 * wm_allpoints_core: out[i] = ((1 / (n_c - 1)) * sum over the rows j of i's group with dist(i, j) > 0 of
 * dist(i, j)^-p)^(-1 / p), n_c the size of the group; 0 for a row without a positive distance.  The sum is an online
 * log-sum-exp of -p * log(dist) in double, taken in column order, so any p > 0 that a double holds is fine where
 * dist^-p itself would overflow.  out double [n]. */
size_t wm_allpoints_core_workspace_bytes(int n, int d, int g);
int wm_allpoints_core(const float* x, const int32_t* group, int n, int d, int metric, int g, double p, double* out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* wm_mreach_min_edge (at inv_alpha = 1) with the further condition group[j] == group[i]: one Boruvka round of every
 * group's own mutual-reachability tree per call.  A row whose component holds its whole group gets -1 / +inf.  For the
 * rows of one group the weights and (relative to the group's first row) the indices are wm_mreach_min_edge's bits on that
 * group's rows alone. */
size_t wm_mreach_min_edge_grouped_workspace_bytes(int n, int d, int g);
int wm_mreach_min_edge_grouped(const float* x, const float* core, const int32_t* comp, const int32_t* group, int n, int d,
                               int metric, int g, float* out_w, int32_t* out_j, void* workspace, size_t workspace_bytes,
                               void* stream);
/* wm_group_min_dist with the mutual reachability in place of the distance: out_w[i][c] = the smallest
 * max(core_q[i], core[j], dist(xq_i, xe_j)) over the rows j of xe with group[j] == c (wm_mreach_query's out_w bits on
 * those columns alone; wm_group_min_dist's bits when all core distances are 0) and out_j[i][c] the lowest j that attains
 * it; +inf / -1 for a group without a column.  core_q float32 [m], core float32 [e]; everything else, the workspace
 * included, as for wm_group_min_dist (here only the columns are grouped, and all of them are walked). */
size_t wm_group_min_mreach_workspace_bytes(int m, int e, int d, int g);
int wm_group_min_mreach(const float* xq, const float* core_q, int m, const float* xe, const float* core, const int32_t* group,
                        int e, int d, int metric, int g, float* out_w, int32_t* out_j, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Ranks in a row's distance ordering (trustworthiness and continuity of an embedding, manifold.py): the two entry points
 * under the same distance function.  The candidates of a row are ordered by (distance, index).
 *
 * wm_pair_dist: out[i][q] = dist(xq_i, x_j), j = idx[i][q], for idx int32 [m][k]: the bits every all-pairs entry point
 * here gives that pair (wm_knn_graph / wm_knn_query return exactly these for their own lists).  An index outside [0, n)
 * (-1 pads a list) gives +inf and reads nothing.  xq float32 [m][d], x float32 [n][d], both 16-byte aligned; out float32
 * [m][k]; 1 <= k <= 64.  A gather kernel, one thread per pair; no workspace. */
int wm_pair_dist(const float* xq, int m, const float* x, int n, int d, int metric, const int32_t* idx, int k, float* out,
                 void* stream);
/* wm_rank_query: count[i][q] = #{ columns l of x, l != skip[i] : (dist(xq_i, x_l), l) < (t[i][q], tj[i][q]) } in the
 * lexicographic order, for k thresholds per row: t float32 [m][k] with their column indices tj int32 [m][k].  skip int32
 * [m] names a column that is never counted for the row (the row itself when xq is x; -1: none).  A threshold of +inf or an
 * index below 0 counts every column but the skipped one.  With t[i][q] = dist(xq_i, x_j) from wm_pair_dist and tj[i][q] =
 * j, 1 + count is the 1-based rank of j among the candidates of row i, ties resolved by the index.
 * Precondition: every row's thresholds are sorted ascending by (t, tj) (a kNN list is; +inf / negative indices last).
 * With another order the counts are unspecified (no access leaves the buffers).  count int32 [m][k].  m, n >= 1,
 * 1 <= k <= 64; xq, x and the workspace 16-byte aligned.  The workspace is one [m][k] int32 plane per column slice and
 * nothing but padding when the rows alone fill the machine.  The counts are integers: the only atomics are integer adds
 * in LDS, and two calls give the same bits. */
size_t wm_rank_query_workspace_bytes(int m, int n, int d, int k);
int wm_rank_query(const float* xq, int m, const float* x, int n, int d, int metric, const float* t, const int32_t* tj,
                  const int32_t* skip, int k, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * KMeans on embeddings (sklearn.cluster.KMeans(n_clusters=k) of notebooks/1.0-Preprocess-WM811K.ipynb; cluster.KMeans):
 * the update step and the k-means++ seeding (csrc/kmeans.hip).  The assignment step is wm_group_min_dist on the centres
 * of R restarts laid out as R groups of k columns, [R * k][d]: one pass over the rows serves every restart.  x float32
 * [n][d] under the clustering section's rules (16-byte aligned, d % 4 == 0, d <= 1024); n <= 2^24, 1 <= k <= 65536,
 * 1 <= R <= 1024.  The workspace-size functions return 0 for sizes that are not supported.  No floating-point atomics,
 * none on global memory (the member counts are integer adds in LDS), no memset; the order of every floating-point sum
 * depends on (n, d, k) alone: two calls give the same bits, and a restart gives the same bits whether
 * it runs alone or among others.
 *
 * wm_kmeans_update: assign int32 [n][R] and dist float32 [n][R] are what wm_group_min_dist wrote for those centres (the
 * column r * k + c for cluster c of restart r, and the distance to it); a value outside [r * k, (r + 1) * k) puts the row
 * in no cluster of restart r.  prev int32 [n][R] is an earlier assign or NULL.  Per restart r and cluster c:
 * counts[r][c] = the number of members and centres_new[r][c][:] = the float64 sum of the members' rows, divided in double
 * by the count and rounded to float32 once; a cluster without a member keeps centres_old[r][c][:] and reports 0.  The sum
 * runs over fixed slabs of rows, in row order inside a slab, and the slabs are folded in slab order.  Per restart:
 * inertia[r] = the double sum of (double)dist[i][r]^2 (the same slabs: 64 lanes take a slab's rows round-robin, each in
 * order, the lane sums are added in lane order and the slabs' sums in a fixed tree), n_changed[r] = the number of rows with assign[i][r] != prev[i][r] (n when prev is NULL), shift2[r] = the double
 * sum over c and the features of ((double)centres_new - (double)centres_old)^2 (blocks of 256 elements, each and then
 * the blocks' sums in a fixed tree).  centres_old, centres_new
 * float32 [R][k][d] (two buffers), counts int32 [R][k], inertia, shift2 double [R], n_changed int32 [R]. */
size_t wm_kmeans_update_workspace_bytes(int n, int d, int k, int R);
int wm_kmeans_update(const float* x, int n, int d, const int32_t* assign, const float* dist, const int32_t* prev, int R, int k,
                     const float* centres_old, float* centres_new, int32_t* counts, double* inertia, int32_t* n_changed,
                     double* shift2, void* workspace, size_t workspace_bytes, void* stream);
/* wm_kmeans_seed: greedy k-means++ (Arthur & Vassilvitskii 2007 with sklearn's local trials) driven by a table of
 * uniforms u double [k][T] in [0, 1) on the device, so that the device makes no random choice; 1 <= T <= 16, k <= n.
 * Centre 0 is row min(floor(u[0][0] * n), n - 1).  For every later centre c: closest2[i] = the smallest squared distance of
 * row i to the centres chosen so far (the float32 distance of the clustering section, squared in double), pot = its sum,
 * candidate t = the first row i with closest2[i] > 0 whose running sum exceeds u[c][t] * pot (so a row at distance 0 is
 * never drawn; no such row: the last row with closest2 > 0; pot == 0: row min(floor(u[c][t] * n), n - 1)); its potential
 * is the sum over i of min(closest2[i], dist(i, candidate)^2); the candidate of the lowest potential wins, equal potentials
 * resolve to the lowest t, and closest2 becomes its minima.  Sums and running sums: blocks of 256 rows in row order, the
 * blocks folded in block order.  Everything is chained on the stream: no host round trip.  Outputs: centres float32
 * [k][d] (copies of the chosen rows), idx int32 [k], and where not NULL cand int32 [k][T] and pots double [k][T], the
 * candidates and potentials of every step (step 0: one candidate; the unused entries are -1 / +inf). */
size_t wm_kmeans_seed_workspace_bytes(int n, int d, int k, int T);
int wm_kmeans_seed(const float* x, int n, int d, int k, int T, const double* u, float* centres, int32_t* idx, int32_t* cand,
                   double* pots, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * UMAP (umap.UMAP(...).fit_transform of the reference's embedding notebooks) on the graph of wm_knn_graph; the formulas
 * are stated in full in csrc/umap.hip.
 *
 * wm_umap_smooth_knn: per row of dist / idx [n][k] (as wm_knn_graph returns them) rho[i] = the first positive distance
 * (0 if none), sigma[i] by at most 64 bisection steps so that sum_{j >= 1} exp(-max(d_j - rho, 0) / sigma) = log2(k) to
 * 1e-5, floored at 1e-3 * the row's mean distance (rho > 0) or 1e-3 * *mean_dist (rho = 0; mean_dist: device pointer to
 * the mean of all n * k distances), and weights[i][j] = exp(-max(d_j - rho, 0) / sigma), 0 where idx[i][j] = i
 * (umap-learn with local_connectivity = 1).  Double precision inside; rho, sigma [n], weights [n][k] float32. */
int wm_umap_smooth_knn(const float* dist, const int32_t* idx, int n, int k, const double* mean_dist, float* rho, float* sigma,
                       float* weights, void* stream);
/* Layout epochs [epoch_begin, epoch_end) of n_epochs over the symmetric graph in CSR form (indptr int32 [n + 1], indices
 * int32 [nnz] in [0, n), q uint32 [nnz] = rint(65536 * weight / max weight)), one launch per epoch, reading one of
 * y_a / y_b float32 [n][dim] and writing the other, starting from y_a; *result_buffer (host) = 0 when the result is in
 * y_a, 1 when in y_b.  Deterministic gather, no atomics: splitting the epoch range over several calls, or calling
 * twice, gives the same bits.  1 <= dim <= 64, 0 <= neg_rate <= 64; a, b > 0.  No allocation, no synchronisation. */
int wm_umap_layout(float* y_a, float* y_b, const int32_t* indptr, const int32_t* indices, const uint32_t* q, int n, int dim,
                   double a, double b, double gamma, double learning_rate, uint32_t seed, int epoch_begin, int epoch_end,
                   int n_epochs, int neg_rate, int* result_buffer, void* stream);

/* Semi-supervised fits and the transform of new rows (umap-learn's discrete_metric_simplicial_set_intersection +
 * reset_local_connectivity, and UMAP.transform); formulas in csrc/umap.hip.
 *
 * wm_umap_label_intersect: the categorical-target intersection of the symmetric-pattern CSR graph (indptr, indices,
 * data float32 [nnz]) with labels int32 [n] (-1: unknown): every entry times f_unk (a label unknown), f_far (labels
 * differ) or 1, rows divided by their maximum, then G + G^T - G o G^T, in double, rounded once into out float32 [nnz]
 * (the pattern is kept; out may not alias data).  Symmetric in bits; a zero row stays zero.  workspace: n doubles,
 * owned by the caller.  No atomics. */
int wm_umap_label_intersect(const int32_t* indptr, const int32_t* indices, const float* data, const int32_t* labels, int n,
                            double f_far, double f_unk, float* out, double* workspace, void* stream);
/* wm_umap_smooth_knn for the rows of a rectangular kNN result dist float32 [m][k] (wm_knn_query): rho = 0 for every
 * row (umap-learn's local_connectivity - 1 = 0), sigma[i] by the same bisection over j >= 1, floored at
 * 1e-3 * *mean_dist, weights[i][j] = exp(-d_j / sigma) (1 where d_j <= 0; no self test).  1 <= k <= 64. */
int wm_umap_smooth_knn_query(const float* dist, int m, int k, const double* mean_dist, float* sigma, float* weights,
                             void* stream);
/* Layout epochs [epoch_begin, epoch_end) of n_epochs for m new points among n fixed ones, ONE launch for all of them:
 * y_in float32 [m][dim] -> y_out [m][dim] (may be the same buffer), y_train float32 [n][dim] read only, idx int32
 * [m][k] in [0, n), q uint32 [m][k] = rint(65536 * weight / max weight).  Only the new points move, none reads another;
 * the step of epoch ep is float32((learning_rate / 4) (1 - ep / n_epochs)).  Deterministic: splitting the epoch range
 * over several calls, or calling twice, gives the same bits.  1 <= k <= 64, 1 <= dim <= 64, 0 <= neg_rate <= 64. */
int wm_umap_transform_layout(const float* y_in, float* y_out, const float* y_train, const int32_t* idx, const uint32_t* q,
                             int m, int n, int k, int dim, double a, double b, double gamma, double learning_rate,
                             uint32_t seed, int epoch_begin, int epoch_end, int n_epochs, int neg_rate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DensMAP (umap.UMAP(densmap=True, ...): the density-preserving term added to the last dens_frac of the layout epochs);
 * formulas, the live rule and the workspace layout are stated in csrc/umap.hip.
 *
 * wm_densmap_graph_radii: ro[i] = log(1e-8 + sum w_e dist_e^2 / sum w_e) over the live entries of row i of the graph
 * (data = w, dists = max(d_ij, d_ji), both float32 [nnz]; live: (uint64)q_e * n_epochs >= 65536), log 1e-8 for a row
 * without live entries.  Double inside, float32 [n] out. */
int wm_densmap_graph_radii(const int32_t* indptr, const float* data, const float* dists, const uint32_t* q, int n, int n_epochs,
                           float* ro, void* stream);
/* The embedding's radii at the positions y float32 [n][dim]: d[i] = D_i = 2 sum_live 1 / (1 + a r^b) and
 * re[i] = log(1e-8 + N_i / D_i), N_i = 2 sum_live r / (1 + a r^b), r = |y_i - y_j|^2 (log 1e-8 when D_i = 0).  One wave
 * per vertex, double inside in a fixed order, float32 [n] out. */
int wm_densmap_embedding_radii(const float* y, const int32_t* indptr, const int32_t* indices, const uint32_t* q, int n, int dim,
                               double a, double b, int n_epochs, float* re, float* d, void* stream);
/* wm_umap_layout with the density term: epochs ep of [epoch_begin, epoch_end) with dens_lambda > 0 and
 * (ep + 1) / n_epochs > 1 - dens_frac first compute the embedding's radii, their mean, variance and covariance with
 * rad (the standardised graph radii, float32 [n]) and the per-vertex terms into the workspace -- further launches on the
 * stream, no atomics, no synchronisation -- and then run the layout kernel with the density term; every other epoch is
 * wm_umap_layout's, bit for bit.  data float32 [nnz] > 0: the graph's weights; n >= 2; workspace: 16-byte aligned,
 * wm_densmap_layout_workspace_bytes(n) bytes (0: unsupported n), owned by the caller; after a call that ran a phase
 * epoch it holds the values the last phase epoch used. */
size_t wm_densmap_layout_workspace_bytes(int n);
int wm_densmap_layout(float* y_a, float* y_b, const int32_t* indptr, const int32_t* indices, const uint32_t* q, const float* data,
                      const float* rad, int n, int nnz, int dim, double a, double b, double gamma, double learning_rate,
                      double dens_lambda, double dens_frac, double dens_var_shift, uint32_t seed, int epoch_begin, int epoch_end,
                      int n_epochs, int neg_rate, void* workspace, size_t workspace_bytes, int* result_buffer, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PCA of an embedding matrix (sklearn.decomposition.PCA): the passes over the rows, on float64 MFMA tiles
 * (v_mfma_f64_16x16x4_f64); tile sizes, the slice rule and the summation orders are stated in csrc/pca.hip.  The
 * eigendecomposition of the d x d covariance is host code (decomposition.py).
 *
 * Common to the four: x float32 [n][d] row-major; 1 <= n <= 2^24; d % 4 == 0, d <= 4096 (pad with zero columns);
 * 1 <= m <= d; mean: float64 [d] or NULL (nothing subtracted / added); every pointer aligned to its element, the
 * workspace and the x of wm_pca_gram to 16 bytes; the workspace is owned by the caller and holds at least the companion's byte count (0:
 * unsupported sizes; the companions launch nothing; project and reconstruct report a fixed token size and store nothing
 * there).  No atomics, no allocation, no synchronisation: two calls give the same bits.
 *
 * wm_pca_mean: mean_out[f] = (sum_i x[i][f]) / n in double: slabs of rows summed sequentially in row order, the slabs'
 * sums added in slab order.  Slab size: 256 rows while that gives at most 1024 slabs, above that ceil(n / 1024)
 * rounded up to a multiple of 256. */
size_t wm_pca_mean_workspace_bytes(int n, int d);
int wm_pca_mean(const float* x, int n, int d, double* mean_out, void* workspace, size_t workspace_bytes, void* stream);
/* out[d][d] float64 = sum_i (x_i - mean)(x_i - mean)^T, centred before it is multiplied; exactly symmetric (tiles on
 * and below the diagonal are computed, the merge mirrors them).  Rows are cut into slices, each slice's partial plane
 * owned by one workgroup per tile, the planes added in slice order. */
size_t wm_pca_gram_workspace_bytes(int n, int d);
int wm_pca_gram(const float* x, int n, int d, const double* mean, double* out, void* workspace, size_t workspace_bytes,
                void* stream);
/* out[n][m] float32 = (x - mean) W^T, W float64 [m][d]; accumulated in double in feature order, rounded once. */
size_t wm_pca_project_workspace_bytes(int n, int d, int m);
int wm_pca_project(const float* x, int n, int d, const double* mean, const double* w, int m, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
/* out[n][d] float32 = y W + mean, y float32 [n][m], W float64 [m][d]; accumulated in double in component order, the
 * mean added last, rounded once. */
size_t wm_pca_reconstruct_workspace_bytes(int n, int m, int d);
int wm_pca_reconstruct(const float* y, int n, int m, const double* w, int d, const double* mean, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian mixture on an embedding matrix (sklearn.mixture.GaussianMixture; mixture.py): the passes over the rows of
 * the E-step and the M-step in float64.  The Cholesky factors of the k covariance matrices are host code.  Tile
 * sizes, slab / slice rules and summation orders are stated in csrc/gmm.hip.
 *
 * Common to all: x float32 [n][ld] row-major with the true feature count d and the row pitch ld, d <= ld, ld % 4 == 0
 * and x 16-byte aligned; whatever columns d .. ld-1 hold is never used.  Parameters are float64 with pitch d:
 * mean [k][d], inv_var [k][d], pchol [k][d][d], resp / out of the E-step [n][k].  1 <= n <= 2^24, 1 <= k <= 1024,
 * d <= 1024 (logprob_diag, weighted_sums, scatter_diag) or d <= 256 (logprob_full, scatter_full).  Every pointer is
 * aligned to its element, the workspace to 16 bytes; the workspace is owned by the caller and holds at least the
 * companion's byte count (0: unsupported sizes; the companions launch nothing; the log-probability kernels report a
 * fixed token size and store nothing there).  No atomics, no allocation, no synchronisation; every sum has an order
 * that depends on the sizes alone: two calls give the same bits.
 *
 * wm_gmm_logprob_diag: out[i][c] = cst[c] - 0.5 * sum_f (double(x[i][f]) - mean[c][f])^2 * inv_var[c][f], one double
 * accumulator, f ascending. */
size_t wm_gmm_logprob_diag_workspace_bytes(int n, int d, int ld, int k);
int wm_gmm_logprob_diag(const float* x, int n, int d, int ld, const double* mean, const double* inv_var, const double* cst,
                        int k, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* out[i][c] = cst[c] - 0.5 * || (x_i - mean_c) P_c ||^2 with P_c = pchol[c] upper triangular: only pchol[c][f][j] with
 * f <= j is read.  The row is centred before it is multiplied. */
size_t wm_gmm_logprob_full_workspace_bytes(int n, int d, int ld, int k);
int wm_gmm_logprob_full(const float* x, int n, int d, int ld, const double* mean, const double* pchol, const double* cst,
                        int k, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* Per row of wlp [n][k]: m = max_c, lpn[i] = m + log(sum_c exp(wlp - m)) with the sum in component order, the row
 * overwritten with exp(wlp - lpn[i]), label[i] = the argmax (the lowest index wins a tie); *lpn_sum = the sum of lpn
 * over slabs of 256 rows (a fixed tree inside a slab), the slabs added in slab order.  k == 1: resp == 1, lpn == wlp. */
size_t wm_gmm_normalize_workspace_bytes(int n, int k);
int wm_gmm_normalize(double* wlp_inout, int n, int k, double* lpn, int32_t* label, double* lpn_sum, void* workspace,
                     size_t workspace_bytes, void* stream);
/* nk[c] = sum_i resp[i][c], sx[c][f] = sum_i resp[i][c] * x[i][f] (sx [k][d]); nk is column d of the same product (a
 * column of exact ones).  Rows are cut into slices, the slices' partial planes added in slice order. */
size_t wm_gmm_weighted_sums_workspace_bytes(int n, int d, int ld, int k);
int wm_gmm_weighted_sums(const float* x, int n, int d, int ld, const double* resp, int k, double* nk, double* sx,
                         void* workspace, size_t workspace_bytes, void* stream);
/* out[c][f] = sum_i resp[i][c] * (x[i][f] - mean[c][f])^2: slabs of rows in row order, the slabs added in slab order. */
size_t wm_gmm_scatter_diag_workspace_bytes(int n, int d, int ld, int k);
int wm_gmm_scatter_diag(const float* x, int n, int d, int ld, const double* resp, int k, const double* mean, double* out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* out[c][d][d] = sum_i resp[i][c] (x_i - mean_c)(x_i - mean_c)^T; exactly symmetric (tiles on and below the diagonal
 * are computed, the merge mirrors them). */
size_t wm_gmm_scatter_full_workspace_bytes(int n, int d, int ld, int k);
int wm_gmm_scatter_full(const float* x, int n, int d, int ld, const double* resp, int k, const double* mean, double* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Logistic regression on an embedding matrix (linear_model.py: LogisticRegression, MultilabelLogisticRegression): one
 * loss / gradient evaluation of `cols` independent columns in float64, as two passes over the rows.  The penalty, the
 * division by the weight sum and the L-BFGS steps are host code.  Tile sizes and summation orders are stated in
 * csrc/logreg.hip.
 *
 * Common to both: x as in the Gaussian-mixture section (float32 [n][ld], true feature count d, ld % 4 == 0, 16-byte
 * aligned, columns d .. ld-1 never read), 1 <= n <= 2^24, d <= 1024, 1 <= cols <= 256.  Pointers aligned to their
 * element, the workspace to 16 bytes and at least the companion's byte count (0: unsupported sizes; the companions
 * launch nothing).  No atomics, no allocation, no synchronisation; every sum has an order that depends on (n, d) alone:
 * two calls give the same bits, and a problem's loss, residual columns and gradient rows are the same bits whichever
 * other problems share the call.
 *
 * wm_logreg_residual.  w float64 [cols][d + 1], column d the intercept.  z[i][q] = sum_f x[i][f] w[q][f] (f ascending,
 * float64 MFMA tiles) + w[q][d], added last.  z_out (optional) float64 [n][cols] receives z.
 *   mode 0 (softmax)  cols = groups * classes, group g owns columns g * classes .. g * classes + classes - 1.  y int32
 *                     [n] in [-1, classes).  Per (row, group): m = max z, lse = m + log(sum exp(z - m)) in class order,
 *                     p = exp(z - lse); with s_i = sw[i] (1 if sw == NULL): loss_i = s_i (lse - z_y),
 *                     resid = s_i (p - onehot(y)).  A row with y == -1 has weight 0: its resid row is exact zeros and
 *                     it adds an exact 0 to the loss.  loss float64 [groups].
 *   mode 1 (sigmoid)  cols = groups * classes, column g * classes + l reads label l of y int8 [n][classes] (0 / 1).
 *                     a = pos_weight[l] if y == 1 (1 if pos_weight == NULL or y == 0); with e = exp(-|z|):
 *                     loss_i = s_i a (max(-z, 0) + log1p(e)) if y == 1, else s_i (max(z, 0) + log1p(e));
 *                     resid = -s_i a sigma(-z) if y == 1, else s_i sigma(z), sigma from e alone (no exp of a positive
 *                     argument).  loss float64 [cols].
 *   y == NULL         prediction: resid receives p (mode 0) or sigma(z) (mode 1); loss, sw, pos_weight are not used.
 * loss[p] = the sum of loss_i: over a tile of 64 rows the butterfly tree (partners 32, 16, .. 1 rows away), the four
 * tiles of a slab of 256 rows as (t0 + t1) + (t2 + t3), the slabs in slab order (runs of ceil(slabs / 256) consecutive
 * slabs, then the 256 run sums in order: wm_gmm_normalize's rule for lpn_sum).  z never goes through memory between
 * the product and the softmax. */
size_t wm_logreg_residual_workspace_bytes(int n, int d, int ld, int cols, int mode, int classes);
int wm_logreg_residual(const float* x, int n, int d, int ld, const double* w, int cols, int mode, int classes,
                       const void* y, const double* sw, const double* pos_weight, double* resid, double* loss,
                       double* z_out, void* workspace, size_t workspace_bytes, void* stream);
/* grad float64 [cols][d + 1] = resid^T [x | 1], resid float64 [n][cols]: wm_gmm_weighted_sums' launch path (the same
 * tile kernel, the same cut of the rows, the planes added in slice order) with sx and nk stored at pitch d + 1, so
 * grad[q][:d] and grad[q][d] are the bits wm_gmm_weighted_sums returns as sx[q] and nk[q]. */
size_t wm_logreg_gradient_workspace_bytes(int n, int d, int ld, int cols);
int wm_logreg_gradient(const float* x, int n, int d, int ld, const double* resid, int cols, double* grad, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Laplacian eigenmaps (manifold.py: laplacian_eigenpairs, spectral_layout, SpectralEmbedding): the device side of a
 * thick-restart Lanczos iteration with full reorthogonalisation on N = D^-1/2 G D^-1/2 in float64.  The small
 * eigenproblem of T and the component search are host code.  Every summation order is stated in csrc/spectral.hip.
 *
 * Common to the four: G is a symmetric CSR graph, indptr int32 [n + 1] rising from 0 to nnz, indices int32 [nnz] in
 * [0, n), data float32 [nnz] (the kernels trust them: manifold.py checks them once); 1 <= n <= 2^24; a basis is
 * row-major [n][ld] float64 with ld <= 256; every pointer aligned to its element, the workspace to 16 bytes; the
 * workspace is owned by the caller and holds at least the companion's byte count (0: unsupported sizes; the companions
 * launch nothing; degree, matvec and rotate report a fixed token size and store nothing there).  No atomics, no
 * allocation, no synchronisation: two calls give the same bits.
 *
 * wm_spec_degree: deg[i] = the double sum of row i in column order; dinv[i] = 1 / sqrt(deg[i]), 0 for an empty row. */
size_t wm_spec_degree_workspace_bytes(int n);
int wm_spec_degree(const int32_t* indptr, const float* data, int n, double* deg, double* dinv, void* workspace,
                   size_t workspace_bytes, void* stream);
/* w[i] = dinv[i] * sum_p data[p] * (dinv[col[p]] * v[col[p] * ldv]): v is a column of a basis of pitch ldv (1: a plain
 * vector), w a plain vector; v and w must not overlap. */
size_t wm_spec_matvec_workspace_bytes(int n);
int wm_spec_matvec(const int32_t* indptr, const int32_t* indices, const float* data, const double* dinv, const double* v,
                   int ldv, int n, double* w, void* workspace, size_t workspace_bytes, void* stream);
/* The tail of Lanczos step j (0 <= j < m < ldv).  comp int32 [n]: the component label of every row in [0, ncomp),
 * 1 <= ncomp <= 256; u float64 [n]: the unit trivial vectors of the components (disjoint supports) in one array.  Twice:
 * w -= u (u . w) per component, then w -= V[:, 0..j] (V[:, 0..j]^T w).  The coefficients of the two passes are added
 * into T[0..j][j], beta = |w| goes to T[j + 1][j] (if j + 1 < m) and to the double behind T's m x m cells, and
 * V[:, j + 1] = w / beta.  beta < n 2^-53: the int64 behind that double is set to j + 1 if it was 0 and the new column
 * is exact zeros.  w is overwritten with the unnormalised residual.  T: row-major [m][m] + 2 cells of 8 bytes. */
size_t wm_spec_orthonormalise_workspace_bytes(int n, int ldv, int ncomp);
int wm_spec_orthonormalise(double* w, double* V, int n, int ldv, int j, const int32_t* comp, int ncomp, const double* u,
                           double* T, int m, void* workspace, size_t workspace_bytes, void* stream);
/* out[n][q] (pitch ldo) = V[n][m] (pitch ldv) @ S[m][q] (pitch lds) on float64 MFMA tiles, k ascending; out is a second
 * buffer (V == out: WM_EINVAL); m, q <= 256. */
size_t wm_spec_rotate_workspace_bytes(int n, int m, int q);
int wm_spec_rotate(const double* V, int ldv, const double* S, int lds, int n, int m, int q, double* out, int ldo,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Label spreading and propagation over a graph (semi_supervised.py: LabelSpreading, LabelPropagation) in float64.
 * Every summation order is stated in csrc/propagate.hip.
 *
 * Common to the four: the graph is as above (symmetric CSR, int32 / float32, trusted, 1 <= n <= 2^24) and dinv comes
 * from wm_spec_degree.  F is row-major [n][ldf] float64 with cols = groups * classes <= 256 and ldf >= cols; column
 * q = g * classes + c belongs to alpha group g and class c; columns behind cols are never read or written.  labels int32
 * [n] in -1 .. classes - 1 (trusted), -1: unknown.  Pointers aligned to their element, the workspace to 16 bytes and at
 * least the companion's byte count (0: unsupported sizes; init, finalize and neighbor_mean report a fixed token size
 * and store nothing there).  No atomics, no allocation, no synchronisation: two calls give the same bits.
 *
 * wm_lp_init: F[i][g * classes + c] = 1.0 if labels[i] == c, else 0.0, for every group. */
size_t wm_lp_init_workspace_bytes(int n, int classes, int groups);
int wm_lp_init(const int32_t* labels, int n, int classes, int groups, double* F, int ldf, void* workspace,
               size_t workspace_bytes, void* stream);
/* iters >= 1 steps Fa -> Fb -> Fa -> ... (the result is in Fb when iters is odd).  With s = sum_p data[p] * (cs[col[p]] *
 * Fin[col[p]][q]) over the row's entries in storage order and y the one-hot of labels[i] (0 for an unknown row):
 *   hard == 0 (spreading)    cs = dinv, Fout = alpha[g] * (dinv[i] * s) + (1 - alpha[g]) * y;
 *   hard != 0 (propagation)  a labelled row gets y; an unlabelled one cs = 1, t = (dinv[i] * dinv[i]) * s and
 *                            Fout = t / (the sum of t over the group's classes, class order; 1 if that is 0), as
 *                            sklearn's LabelPropagation renormalises every row at every step;
 *   active[g] == 0           the group's columns are copied from Fin bit for bit.
 * alpha float64 [groups] and active int32 [groups] are device arrays.  resid float64 [iters][groups] receives, per step,
 * the sum over the rows and the group's classes of |Fout - Fin| (exactly 0 for a frozen group); its order depends on n
 * and classes alone, not on the number of groups.  Fa and Fb must not overlap. */
size_t wm_lp_iterate_workspace_bytes(int n, int classes, int groups);
int wm_lp_iterate(const int32_t* indptr, const int32_t* indices, const float* data, const double* dinv,
                  const int32_t* labels, int n, int classes, int groups, const double* alpha, const int32_t* active,
                  int hard, int iters, double* Fa, double* Fb, int ldf, double* resid, void* workspace,
                  size_t workspace_bytes, void* stream);
/* One group's columns (F points at the group's first column, pitch ldf): rowsum[i] = the sum of the classes in column
 * order; dist[i][c] (pitch classes) = F / rowsum, zeros where rowsum == 0; pred[i] = the first maximum (0 for an all-zero
 * row); unreached[i] (one byte) = (rowsum == 0). */
size_t wm_lp_finalize_workspace_bytes(int n, int classes);
int wm_lp_finalize(const double* F, int ldf, int n, int classes, double* dist, double* rowsum, int32_t* pred,
                   uint8_t* unreached, void* workspace, size_t workspace_bytes, void* stream);
/* out[r][c] = (sum_t dist[idx[r][t]][c], t ascending) / (its sum over c, c ascending); rows whose sum is 0 stay 0.
 * idx int32 [m][k] in [0, n) (trusted), 1 <= m <= 2^24, 1 <= k <= 64; dist float64 [n][classes], out [m][classes]. */
size_t wm_lp_neighbor_mean_workspace_bytes(int m, int k, int classes);
int wm_lp_neighbor_mean(const int32_t* idx, int m, int k, const double* dist, int n, int classes, double* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Local outlier factor over neighbour lists (neighbors.py: LocalOutlierFactor, outlier_scores, hubness) in float64.
 * The mapping and every summation order are stated in csrc/lof.hip.
 *
 * Common to the three: a list is a row of `ld` columns, 1 <= ld <= 63, of float32 distances and int32 indices as
 * wm_knn_graph / wm_knn_query order them (by (distance, index)); for the fitted set the row itself has been removed.
 * 1 <= rows, n_fit <= 2^24.  ks is a HOST array of `groups` neighbour counts, 1 <= groups <= WM_LOF_MAX_GROUPS, every
 * 1 <= ks[r] <= ld (WM_EINVAL otherwise, before any launch; a caller with a longer list calls once per chunk): group r
 * reads the first ks[r] columns of every row and no other, and all groups are served by one launch.  Outputs are
 * row-major [groups][rows].  An index outside [0, n_fit) gathers nothing (its term counts as 0).  Pointers aligned to
 * their element; the workspace is a token (the companions report a fixed size, 0 for unsupported sizes) and nothing is
 * stored there.  Distances are widened to float64 once; every sum is the balanced tree over the columns t = 0 .. 63
 * (zeros behind ks[r]), pairs (t, t ^ 1) first, then (t, t ^ 2), ... (t, t ^ 32).  No float atomics: two calls give the
 * same bits, and a ks[r] gives the same bits alone as inside any list. */
#define WM_LOF_MAX_GROUPS 64
/* Local reachability density of the query rows against the fitted lists dist_fit [n_fit][ld_fit] (ks[r] <= ld_fit too):
 *   lrd[r][i] = 1 / ((sum_{t < ks[r]} max(dist_q[i][t], dist_fit[idx_q[i][t]][ks[r] - 1])) / ks[r] + 1e-10).
 * For the fit itself the query lists ARE the fitted lists (dist_q == dist_fit is allowed). */
size_t wm_lof_lrd_workspace_bytes(int rows, int ld, int groups);
int wm_lof_lrd(const float* dist_q, const int32_t* idx_q, int rows, int ld, const float* dist_fit, int n_fit, int ld_fit,
               const int32_t* ks, int groups, double* lrd, void* workspace, size_t workspace_bytes, void* stream);
/* lof[r][i] = ((sum_{t < ks[r]} lrd_fit[r][idx_q[i][t]]) / ks[r]) / lrd_q[r][i]; lrd_q [groups][rows] and lrd_fit
 * [groups][n_fit] as wm_lof_lrd wrote them (the same array for the fit itself); lof is a third buffer. */
size_t wm_lof_factor_workspace_bytes(int rows, int ld, int groups);
int wm_lof_factor(const int32_t* idx_q, int rows, int ld, const double* lrd_q, const double* lrd_fit, int n_fit,
                  const int32_t* ks, int groups, double* lof, void* workspace, size_t workspace_bytes, void* stream);
/* indeg[r][j] = #{ (i, t) : t < ks[r], idx[i][t] == j } for j in [0, n), int32 [groups][n]: cleared by a kernel, then one
 * integer atomic add per list entry into the group with the smallest ks[r] > t (max(ks) per row, order-independent), then
 * the groups are added up in the order of their ks[r]. */
size_t wm_lof_indegree_workspace_bytes(int rows, int ld, int groups);
int wm_lof_indegree(const int32_t* idx, int rows, int ld, int n, const int32_t* ks, int groups, int32_t* indeg,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian log-sums over all pairs (density.py: KernelDensity, KDEClassifier, uniformity) in float64.  The mapping and
 * every summation order are stated in csrc/kde.hip.
 *   out[q][i] = log sum_j exp(-inv_two_h2[q] * s_ij),   out row-major [b][m],
 * over the columns j of x [n][d] that are not excluded, for the rows i of xr [m][d].  s_ij is the SQUARED Euclidean
 * distance as the all-pairs kernels build it before the root: float32 fused multiply-adds over the features in index
 * order in one accumulator, widened exactly to double (s_ij and s_ji are the same bits; equal rows give exactly 0;
 * relative error at most (d + 2) 2^-24, first order).  Column j is excluded for row i when self_offset >= 0 and
 * j + self_offset == i: 0 with xr == x is the leave-one-out sum, `lo` with x = xr + lo * d the leave-one-out sum against
 * the rows lo .. lo + n - 1 of xr, -1 excludes nothing.  A duplicate of a row is another column and counts.  A row
 * without an included column gives -inf; a pair whose s is not finite contributes nothing.  inv_two_h2 is a HOST array
 * of b values, 1 <= b <= WM_KDE_MAX_BANDWIDTHS, every one finite and > 0 (WM_EINVAL otherwise, and for self_offset < -1,
 * before any launch; a caller with a longer list calls once per chunk).  d % 4 == 0, d <= 1024, 1 <= m, n <= 2^24; xr, x
 * and the workspace aligned to 16 bytes, out to 8.  Exponent arithmetic and sums in float64; one running minimum of s per
 * row is the shift of every bandwidth, so a bandwidth gives the same bits alone as inside any list; no atomics: two calls
 * give the same bits.  The size function answers 0 for sizes outside these limits. */
#define WM_KDE_MAX_BANDWIDTHS 4
size_t wm_kde_logsum_workspace_bytes(int m, int n, int d, int b);
int wm_kde_logsum(const float* xr, int m, const float* x, int n, int d, const double* inv_two_h2, int b, int self_offset,
                  double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Debugging probe (no reference counterpart): *slot = max(*slot, max_i |x[i]|), NaN if any x[i] is NaN
 * (+inf stays +inf).  x: n elements of WM_F32 / WM_BF16; *slot must hold a non-negative float (zero it
 * first).  Allocates nothing, so it can sit between the launches of a captured hipGraph
 * (tools/nan_hunt.py; DESIGN.md "NaN at cfg 2"). */
int wm_debug_absmax(const void* x, int dtype, long long n, float* slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAFER_HIP_H */
