// The ONE distance function of the embedding kernels (cluster.hip states its two properties; kmeans.hip's seeding calls
// it too): the float32 differences accumulated in float32 in index order in a single accumulator, then the root.
#pragma once
#include "common.h"

template <int METRIC>
__device__ __forceinline__ float cl_accum(float a, float b, float acc) {
  const float t = a - b;
  if constexpr (METRIC == 0) return fmaf(t, t, acc);
  return acc + fabsf(t);
}
template <int METRIC>
__device__ __forceinline__ float cl_finish(float acc) {
  if constexpr (METRIC == 0) return sqrtf(acc);  // (the correctly rounded root; __fsqrt_rn is the ~1 ulp native one here)
  return acc;
}
