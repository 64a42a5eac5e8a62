// Wire codecs shared by the single-party kernels (kernels.hip), the fused
// wire reduce (wirereduce.hip) and the fused DGT encode (dgtencode.hip): one
// definition of each encode and decode, so all of them produce the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// ---------------------------------------------------------------------------
// 2bit (gradient_compression-inl.h:40-139 semantics)
// code: 0b11 -> +thr, 0b10 -> -thr, 0b00 -> 0; 16 codes per uint32 word,
// slot s occupies bits [2s, 2s+1].
// ---------------------------------------------------------------------------

// spread 16 bits of x to even bit positions of a 32-bit word
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
  x &= 0x0000FFFFu;
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

__device__ __forceinline__ float decode2(uint32_t c, float thr) {
  return (c == 3u) ? thr : ((c == 2u) ? -thr : 0.0f);
}

// ---------------------------------------------------------------------------
// 4-bit linear codes on a chunk's [lo, hi] (van.cc:750-824 semantics): code
// k is the midpoint of the k-th of 16 equal bins. The product and the sum
// contract into one fma.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float step4(float lo, float hi) {
  return fmaxf(hi - lo, 1e-30f) / 16.0f;
}

__device__ __forceinline__ float decode4(uint32_t code, float lo, float step) {
  return lo + ((float)code + 0.5f) * step;
}

// code of f on a chunk with minimum lo; inv = 1.0f / step4(lo, hi)
__device__ __forceinline__ uint32_t encode4(float f, float lo, float inv) {
  const int code = (int)floorf((f - lo) * inv);
  return (uint32_t)(code < 0 ? 0 : (code > 15 ? 15 : code));
}
