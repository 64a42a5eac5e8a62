// Max-pool backward select shared by the kernels that stage a pooled
// gradient straight into LDS (convwrw2.hip, conv.hip): 8 bf16 gradient
// values + their 8 argmax codes (0..3 = quadrant dy*2+dx, 255 = relu
// clamped) -> the 8 values of full-resolution position `quad`. Same
// select as k_relu_maxpool2_bwd_nhwc: code == quad ? g : 0, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ uint4 unpool_select(uint4 g, uint2 code,
                                               unsigned quad) {
  const unsigned gw[4] = {g.x, g.y, g.z, g.w};
  const unsigned cw[2] = {code.x, code.y};
  unsigned r[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned c2 = cw[w >> 1] >> ((w & 1) * 16);
    const unsigned lo = ((c2 & 0xFFu) == quad) ? 0x0000FFFFu : 0u;
    const unsigned hi = (((c2 >> 8) & 0xFFu) == quad) ? 0xFFFF0000u : 0u;
    r[w] = gw[w] & (lo | hi);
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}
