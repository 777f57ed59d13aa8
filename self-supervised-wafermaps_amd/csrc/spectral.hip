// Laplacian eigenmaps (manifold.py: laplacian_eigenpairs): the device side of a thick-restart Lanczos iteration with
// full reorthogonalisation on N = D^-1/2 G D^-1/2, G a symmetric CSR graph with float32 weights, everything else float64.
//   wm_spec_degree          deg[i] = the row sum, dinv[i] = 1 / sqrt(deg[i]) (0 for an empty row);
//   wm_spec_matvec          w = N v;
//   wm_spec_orthonormalise  the tail of one Lanczos step: project the trivial vectors and the basis out of w twice
//                           (classical Gram-Schmidt, two passes), write the summed coefficients and beta = |w| into
//                           column j of T, and w / beta into column j + 1 of V;
//   wm_spec_rotate          out = V S on v_mfma_f64_16x16x4_f64 (thick restart, final Ritz vectors).
// No atomics, no allocation, no synchronisation with the host; the order of every sum depends on the sizes alone, so
// two calls give the same bits.
//
// ---- sums and their orders.
//   degree   one thread per row, the row's entries in column (= storage) order, one double accumulator.
//   matvec   16 lanes per row.  Lane l adds the terms data[p] * (dinv[col[p]] * v[col[p]]) of the entries
//            p = begin + l, begin + l + 16, ... in that order into one double; the 16 sums are then added as a xor
//            butterfly over lane distances 8, 4, 2, 1; one multiplication by dinv[i] at the end.  Rows of 0 .. several
//            hundred entries: at most ceil(len / 16) dependent loads per lane, and a wave's 4 rows gather 4 x 16
//            consecutive entries per step.
//   slabs    the reductions over the rows (u . w per component, V^T w, |w|^2) go over slabs of SPEC_SLAB = 256
//            consecutive rows, one workgroup of 4 waves each, in the style of wm_pca_mean: a slab's partial is stored
//            with a plain store into the slab's slot, and a merge kernel adds the slots in slab order, one thread per
//            result.  (Measured, profiles/spectral.md: a step's tail costs the same at j = 32 and j = 63 -- 0.08 ms at
//            12 449 rows, 0.8 ms at 172 950 -- which points at these serial merges, a dependent load per slab, and not at
//            the basis reads; no per-kernel trace was taken.  A merge by one wave per result is the next step.)
//     u . w    per wave and component c: the products u[i] w[i] of the wave's 64 rows whose label is c (0.0 elsewhere)
//              are added as a xor butterfly over lane distances 32, 16, 8, 4, 2, 1; the slab's value is
//              ((wave 0 + wave 1) + wave 2) + wave 3.  A component none of the wave's rows belongs to contributes an
//              exact 0.0 (the butterfly is skipped).
//     V^T w    wave v of the slab owns the rows r = v, v + 4, v + 8, ... of the slab; lane l owns column 64 t + l and
//              adds V[r][c] * w[r] in row order; the slab's value is ((wave 0 + wave 1) + wave 2) + wave 3.
//     |w|^2    thread t squares row t of the slab; xor butterfly 32 .. 1 inside the wave, then ((0 + 1) + 2) + 3.
//   update   w[i] -= sum_c V[i][c] h[c]: 16 lanes per row, lane l adds columns l, l + 16, ... in order, butterfly 8, 4,
//            2, 1 as in the matvec.
//   rotate   one wave per 16 x 16 tile of out, k ascending in steps of 4 (one MFMA each), operands straight from global
//            memory (V is read once per 16 columns of S; S is small and stays in cache), exact zeros outside.
//
// ---- one call of wm_spec_orthonormalise (w in place, 13 launches on the stream):
//   twice:  s_c = u . w per component;  w -= u s_c (fused into the next kernel, which stores the new w);
//           h = V[:, 0..j]^T w;  T[0..j][j] (+)= h;  w -= V[:, 0..j] h
//   then    beta = sqrt(|w|^2) -> T[j + 1][j] (if j + 1 < m) and the slot behind T; beta < n 2^-53 sets the flag word
//           behind that slot to j + 1 (if it is still 0) and the new column is written as exact zeros, never NaN;
//           otherwise V[:, j + 1] = w / beta, beta read from device memory by the dividing kernel.
// T is row-major [m][m] doubles followed by one double (the last beta) and one int64 (the breakdown flag).
//
// Fragment maps of v_mfma_f64_16x16x4_f64 (spec_rotate: fk, fc, the store walk): as stated in f64.h.
#include "f64.h"

namespace {

constexpr int SPEC_MAX_N = 1 << 24;
constexpr int SPEC_MAX_LDV = 256;    // columns of a basis (the LDS partials of a slab are [4][SPEC_MAX_LDV])
constexpr int SPEC_MAX_COMP = 256;   // connected components whose trivial vectors one call projects out
constexpr int SPEC_SLAB = 256;       // rows per slab = threads per workgroup
constexpr int SPEC_THREADS = 256;

inline int spec_slabs(int n) { return (n + SPEC_SLAB - 1) / SPEC_SLAB; }

__device__ __forceinline__ double spec_group16_sum(double v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}
__device__ __forceinline__ double spec_wave_sum(double v) {
  v += __shfl_xor(v, 32, 64);
  v += __shfl_xor(v, 16, 64);
  return spec_group16_sum(v);
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_degree(const int32_t* __restrict__ indptr, const float* __restrict__ data,
                                                            int n, double* __restrict__ deg, double* __restrict__ dinv) {
  const int i = blockIdx.x * SPEC_THREADS + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int p = indptr[i], e = indptr[i + 1]; p < e; ++p) acc += (double)data[p];
  deg[i] = acc;
  dinv[i] = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_matvec(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, const double* __restrict__ dinv,
                                                            const double* __restrict__ v, int ldv, int n, double* __restrict__ w) {
  const int i = blockIdx.x * (SPEC_THREADS / 16) + (threadIdx.x >> 4), l = threadIdx.x & 15;
  double acc = 0.0;
  if (i < n) {
    for (int p = indptr[i] + l, e = indptr[i + 1]; p < e; p += 16) {
      const int c = indices[p];
      acc += (double)data[p] * (dinv[c] * v[(size_t)c * ldv]);
    }
  }
  acc = spec_group16_sum(acc);
  if (i < n && l == 0) w[i] = dinv[i] * acc;
}

// upart[slab][c] = the slab's share of u . w for component c
__global__ __launch_bounds__(SPEC_THREADS) void spec_udot_partial(const double* __restrict__ w, const double* __restrict__ u,
                                                                  const int32_t* __restrict__ comp, int n, int ncomp,
                                                                  double* __restrict__ upart) {
  __shared__ double part[4][SPEC_MAX_COMP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = blockIdx.x * SPEC_SLAB + t;
  const bool live = i < n;
  const int label = live ? comp[i] : -1;
  const double prod = live ? u[i] * w[i] : 0.0;
  for (int c = 0; c < ncomp; ++c) {
    double s = 0.0;
    if (__any(label == c)) s = spec_wave_sum(label == c ? prod : 0.0);
    if (lane == 0) part[wave][c] = s;
  }
  __syncthreads();
  for (int c = t; c < ncomp; c += SPEC_THREADS)
    upart[(size_t)blockIdx.x * ncomp + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// plain[c] = the slots' sum in slab order, out[c stride] (+)= it; `stride` doubles between the cells of out (T's column: m)
__global__ __launch_bounds__(64) void spec_merge(const double* __restrict__ part, int slabs, int width, int count,
                                                 double* __restrict__ plain, double* __restrict__ out, int stride, int add) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= count) return;
  double sum = 0.0;
  for (int s = 0; s < slabs; ++s) sum += part[(size_t)s * width + c];
  plain[c] = sum;
  if (out) out[(size_t)c * stride] = add ? out[(size_t)c * stride] + sum : sum;
}

// w -= u s (stored), then vpart[slab][c] = the slab's share of V[:, c] . w for c < m1
__global__ __launch_bounds__(SPEC_THREADS) void spec_vdot_partial(double* __restrict__ w, const double* __restrict__ u,
                                                                  const int32_t* __restrict__ comp, const double* __restrict__ s,
                                                                  const double* __restrict__ V, int n, int ldv, int m1,
                                                                  double* __restrict__ vpart) {
  __shared__ double wl[SPEC_SLAB];
  __shared__ double part[4][SPEC_MAX_LDV];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i0 = blockIdx.x * SPEC_SLAB, rows = min(SPEC_SLAB, n - i0);
  if (t < rows) {
    const double x = w[i0 + t] - u[i0 + t] * s[comp[i0 + t]];
    w[i0 + t] = x;
    wl[t] = x;
  }
  __syncthreads();
  for (int c = lane; c < m1; c += 64) {
    double acc = 0.0;
    for (int r = wave; r < rows; r += 4) acc += V[(size_t)(i0 + r) * ldv + c] * wl[r];
    part[wave][c] = acc;
  }
  __syncthreads();
  for (int c = t; c < m1; c += SPEC_THREADS)
    vpart[(size_t)blockIdx.x * ldv + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_update(double* __restrict__ w, const double* __restrict__ V,
                                                            const double* __restrict__ h, int n, int ldv, int m1) {
  const int i = blockIdx.x * (SPEC_THREADS / 16) + (threadIdx.x >> 4), l = threadIdx.x & 15;
  double acc = 0.0;
  if (i < n)
    for (int c = l; c < m1; c += 16) acc += V[(size_t)i * ldv + c] * h[c];
  acc = spec_group16_sum(acc);
  if (i < n && l == 0) w[i] -= acc;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_norm_partial(const double* __restrict__ w, int n, double* __restrict__ npart) {
  __shared__ double part[4];
  const int t = threadIdx.x, i = blockIdx.x * SPEC_SLAB + t;
  const double x = i < n ? w[i] : 0.0;
  const double s = spec_wave_sum(x * x);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) npart[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ void spec_norm_merge(const double* __restrict__ npart, int slabs, int n, int j, int m, double* __restrict__ T) {
  double sum = 0.0;
  for (int s = 0; s < slabs; ++s) sum += npart[s];
  const double beta = sqrt(sum);
  if (j + 1 < m) T[(size_t)(j + 1) * m + j] = beta;
  T[(size_t)m * m] = beta;
  long long* flag = reinterpret_cast<long long*>(T + (size_t)m * m + 1);
  if (!(beta >= (double)n * 0x1p-53) && *flag == 0) *flag = j + 1;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_scale(const double* __restrict__ w, const double* __restrict__ beta_at, int n,
                                                           int ldv, int col, double* __restrict__ V) {
  const int i = blockIdx.x * SPEC_THREADS + threadIdx.x;
  if (i >= n) return;
  const double beta = *beta_at;
  V[(size_t)i * ldv + col] = beta >= (double)n * 0x1p-53 ? w[i] / beta : 0.0;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_rotate(const double* __restrict__ V, int ldv, const double* __restrict__ S,
                                                            int lds, int n, int m, int q, double* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = (blockIdx.x * 4 + wave) * 16, c0 = blockIdx.y * 16;
  if (r0 >= n) return;  // (no barrier below)
  const int fk = lane >> 4, fc = lane & 15;
  const int ar = r0 + fc, bc = c0 + fc;
  f64x4_t acc = f64x4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < m; k0 += 4) {
    const int k = k0 + fk;
    const double a = ar < n && k < m ? V[(size_t)ar * ldv + k] : 0.0;
    const double b = bc < q && k < m ? S[(size_t)k * lds + bc] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + fk + 4 * r, col = c0 + fc;
    if (row < n && col < q) out[(size_t)row * ldo + col] = acc[r];
  }
}

inline bool spec_ortho_ok(int n, int ldv, int j, int ncomp, int m) {
  return n <= SPEC_MAX_N && ldv <= SPEC_MAX_LDV && ncomp <= SPEC_MAX_COMP && j + 1 < ldv && j < m && m < ldv;
}

}  // namespace

extern "C" size_t wm_spec_degree_workspace_bytes(int n) { return n >= 1 && n <= SPEC_MAX_N ? WM_TOKEN_WS : 0; }

extern "C" int wm_spec_degree(const int32_t* indptr, const float* data, int n, double* deg, double* dinv, void* workspace,
                              size_t workspace_bytes, void* stream) {
  WM_REQUIRE(indptr && data && deg && dinv && workspace && n > 0, WM_EINVAL);
  WM_REQUIRE(n <= SPEC_MAX_N, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(indptr, 3) && wm_aligned(data, 3) && wm_aligned(deg, 7) && wm_aligned(dinv, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  spec_degree<<<wm_cdiv(n, SPEC_THREADS), SPEC_THREADS, 0, static_cast<hipStream_t>(stream)>>>(indptr, data, n, deg, dinv);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_spec_matvec_workspace_bytes(int n) { return n >= 1 && n <= SPEC_MAX_N ? WM_TOKEN_WS : 0; }

extern "C" int wm_spec_matvec(const int32_t* indptr, const int32_t* indices, const float* data, const double* dinv,
                              const double* v, int ldv, int n, double* w, void* workspace, size_t workspace_bytes,
                              void* stream) {
  WM_REQUIRE(indptr && indices && data && dinv && v && w && workspace && n > 0 && ldv > 0, WM_EINVAL);
  WM_REQUIRE(n <= SPEC_MAX_N && ldv <= SPEC_MAX_LDV, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(indptr, 3) && wm_aligned(indices, 3) && wm_aligned(data, 3) && wm_aligned(dinv, 7) &&
                 wm_aligned(v, 7) && wm_aligned(w, 7),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  spec_matvec<<<wm_cdiv(n, SPEC_THREADS / 16), SPEC_THREADS, 0, static_cast<hipStream_t>(stream)>>>(indptr, indices, data, dinv, v,
                                                                                                   ldv, n, w);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

// workspace: upart [slabs][ncomp] | s [ncomp] | vpart [slabs][ldv] | h [ldv] | npart [slabs], doubles
extern "C" size_t wm_spec_orthonormalise_workspace_bytes(int n, int ldv, int ncomp) {
  if (n < 1 || n > SPEC_MAX_N || ldv < 2 || ldv > SPEC_MAX_LDV || ncomp < 1 || ncomp > SPEC_MAX_COMP) return 0;
  const size_t slabs = (size_t)spec_slabs(n);
  return (slabs * ncomp + ncomp + slabs * ldv + ldv + slabs) * sizeof(double);
}

extern "C" int wm_spec_orthonormalise(double* w, double* V, int n, int ldv, int j, const int32_t* comp, int ncomp,
                                      const double* u, double* T, int m, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  WM_REQUIRE(w && V && comp && u && T && workspace && n > 0 && ldv > 0 && j >= 0 && ncomp > 0 && m > 0, WM_EINVAL);
  WM_REQUIRE(spec_ortho_ok(n, ldv, j, ncomp, m), WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(w, 7) && wm_aligned(V, 7) && wm_aligned(comp, 3) && wm_aligned(u, 7) && wm_aligned(T, 7) &&
                 wm_aligned(workspace, 15),
             WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= wm_spec_orthonormalise_workspace_bytes(n, ldv, ncomp), WM_EWORKSPACE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = spec_slabs(n), m1 = j + 1;
  double* upart = static_cast<double*>(workspace);
  double* s = upart + (size_t)slabs * ncomp;
  double* vpart = s + ncomp;
  double* h = vpart + (size_t)slabs * ldv;
  double* npart = h + ldv;
  for (int pass = 0; pass < 2; ++pass) {
    spec_udot_partial<<<slabs, SPEC_THREADS, 0, st>>>(w, u, comp, n, ncomp, upart);
    WM_LAUNCH_CHECK();
    spec_merge<<<wm_cdiv(ncomp, 64), 64, 0, st>>>(upart, slabs, ncomp, ncomp, s, nullptr, 0, 0);
    WM_LAUNCH_CHECK();
    spec_vdot_partial<<<slabs, SPEC_THREADS, 0, st>>>(w, u, comp, s, V, n, ldv, m1, vpart);
    WM_LAUNCH_CHECK();
    spec_merge<<<wm_cdiv(m1, 64), 64, 0, st>>>(vpart, slabs, ldv, m1, h, T + j, m, pass);
    WM_LAUNCH_CHECK();
    spec_update<<<wm_cdiv(n, SPEC_THREADS / 16), SPEC_THREADS, 0, st>>>(w, V, h, n, ldv, m1);
    WM_LAUNCH_CHECK();
  }
  spec_norm_partial<<<slabs, SPEC_THREADS, 0, st>>>(w, n, npart);
  WM_LAUNCH_CHECK();
  spec_norm_merge<<<1, 1, 0, st>>>(npart, slabs, n, j, m, T);
  WM_LAUNCH_CHECK();
  spec_scale<<<wm_cdiv(n, SPEC_THREADS), SPEC_THREADS, 0, st>>>(w, T + (size_t)m * m, n, ldv, j + 1, V);
  WM_LAUNCH_CHECK();
  return WM_OK;
}

extern "C" size_t wm_spec_rotate_workspace_bytes(int n, int m, int q) {
  return n >= 1 && n <= SPEC_MAX_N && m >= 1 && m <= SPEC_MAX_LDV && q >= 1 && q <= SPEC_MAX_LDV ? WM_TOKEN_WS : 0;
}

extern "C" int wm_spec_rotate(const double* V, int ldv, const double* S, int lds, int n, int m, int q, double* out, int ldo,
                              void* workspace, size_t workspace_bytes, void* stream) {
  WM_REQUIRE(V && S && out && workspace && n > 0 && m > 0 && q > 0, WM_EINVAL);
  WM_REQUIRE(ldv >= m && lds >= q && ldo >= q && V != out, WM_EINVAL);
  WM_REQUIRE(wm_spec_rotate_workspace_bytes(n, m, q) != 0, WM_EUNSUPPORTED);
  WM_REQUIRE(wm_aligned(V, 7) && wm_aligned(S, 7) && wm_aligned(out, 7), WM_EALIGN);
  WM_REQUIRE(workspace_bytes >= WM_TOKEN_WS, WM_EWORKSPACE);
  spec_rotate<<<dim3(wm_cdiv(n, 64), wm_cdiv(q, 16)), SPEC_THREADS, 0, static_cast<hipStream_t>(stream)>>>(V, ldv, S, lds, n, m, q,
                                                                                                          out, ldo);
  WM_LAUNCH_CHECK();
  return WM_OK;
}
