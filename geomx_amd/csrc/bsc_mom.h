// Bi-Sparse momentum term, shared by the momentum / fused compress kernels
// (kernels.hip) and the boundary select (bscselect.hip): one definition, so
// the sampled boundary and the kernels that compare against it round alike.
#pragma once

#include <hip/hip_runtime.h>

// u*mu and + g are rounded SEPARATELY (no FMA contraction), exactly as
// the golden model (two torch ops) and the sampled boundary prediction
// do: the boundary is the |v| of one sampled element, so a fused
// multiply-add that lands one ulp below it would drop that element, and
// a mixed CPU/GPU party would drift apart in u and v.
__device__ __forceinline__ float bsc_mom(float u, float mu, float g) {
#pragma clang fp contract(off)
  const float p = u * mu;
  return p + g;
}
