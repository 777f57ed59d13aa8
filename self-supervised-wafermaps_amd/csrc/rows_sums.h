// The launch path of "out = resp^T [x | 1]" (gmm.hip: gm_rows_tile<GM_WSUM> and gm_wsum_merge), shared by
// wm_gmm_weighted_sums and wm_logreg_gradient (logreg.hip): one tile kernel, one cut of the rows (a function of (n, d)
// alone), the planes added in slice order.  Not part of the C ABI.
#pragma once
#include "common.h"

// 0 for sizes the path does not take (1 <= n <= 2^24, 1 <= k <= 1024, 1 <= d <= 1024, ld % 4 == 0).
__attribute__((visibility("hidden"))) size_t wm_rows_sums_workspace_bytes(int n, int d, int ld, int k);
// sx[c * sx_ld + f] = sum_i resp[i][c] x[i][f] for f < d, nk[c * nk_ld] = sum_i resp[i][c] (column d of the same
// product).  The caller has checked the sizes, the pointers and the workspace.
__attribute__((visibility("hidden"))) int wm_rows_sums_launch(const float* x, int n, int d, int ld, const double* resp, int k,
                                                              double* nk, int nk_ld, double* sx, int sx_ld, void* workspace,
                                                              hipStream_t st);
