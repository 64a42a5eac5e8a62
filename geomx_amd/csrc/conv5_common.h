// Device helpers shared by the conv5 kernels of conv.hip and
// convwrw2.hip: vector types, the zero page and the LDS-DMA pieces, the
// pool / unpool selects, the quad transpose of the packed epilogues, the
// row-image geometry with its staging loop, and the fragment helpers of
// the direct and the wrw kernels. Everything is __forceinline__ (or
// static), so each translation unit gets its own copy; nothing here
// needs relocatable device code.
//
// The larger helpers (stage_rows, direct_a_chunk, pooled_load,
// pooled_write) replace lambdas that captured the kernel's variables by
// reference, and take those variables BY REFERENCE: hipcc simplifies a
// helper on its own before it inlines it, and from references it ends at
// the instruction stream the lambda gave. By value, the same source text
// cost or saved the direct kernels 8-24 VGPRs and moved scalar
// instructions in every staging loop (scripts/kernel_isa_diff.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

typedef unsigned short bf16_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ bf16_t cf2bf(float f) {
  union { float f; unsigned int u; } cv;
  cv.f = f;
  unsigned int lsb = (cv.u >> 16) & 1;  // round-to-nearest-even
  return (bf16_t)((cv.u + 0x7FFFu + lsb) >> 16);
}

// LDS byte address of a pointer into a __shared__ array
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3)))
                               void*)p;
}

// lo/hi halves (k-pixels 0..15 / 16..31 of a transpose read, or two
// ds_read_b64 of an 8 B aligned fragment) -> one MFMA operand
__device__ __forceinline__ bf16x8 join_bf16x4(bf16x4 lo, bf16x4 hi) {
  union { struct { bf16x4 lo, hi; } p; bf16x8 v; } c;
  c.p.lo = lo;
  c.p.hi = hi;
  return c.v;
}

// ---- LDS-DMA staging

// Zero page: staging lanes whose granule falls outside the row read
// here, so padding is zero-filled in the same pass as the data.
static __device__ __attribute__((aligned(64))) bf16_t g_conv5_zeros[1024];
// (through a __device__ function: a kernel's lambda is also host code to
// the compiler, and naming the page there makes it an external symbol
// that device code then reaches through the GOT)
__device__ __forceinline__ const bf16_t* conv5_zeros() {
  return g_conv5_zeros;
}

// One 1 KiB LDS-DMA piece (16 B per lane), the compiler's form: hipcc
// keeps track of it and waits (vmcnt(0)) ahead of the next LDS read it
// cannot prove disjoint. `lds_dst` is the wave-uniform destination.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// One 1 KiB LDS-DMA piece (16 B per lane) that the compiler does not
// see: for a __builtin_amdgcn_global_load_lds in flight hipcc puts
// s_waitcnt vmcnt(0) ahead of the next LDS read it cannot prove
// disjoint, which would end the prefetch of the NEXT block's image at
// the first fragment read of this one. The kernels wait for their pieces
// themselves (vmcnt(0) ahead of the barrier that opens each MFMA phase).
// `lds_dst` is the wave-uniform LDS byte address of the piece.
__device__ __forceinline__ void glds16_unseen(const void* gsrc,
                                              unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
      : "memory");
}

// Row image: rows of PIX pixels x CI bf16 channels in their NHWC order,
// each padded to whole 1 KiB LDS-DMA chunks so every piece writes full
// 64-lane spans (no partial EXEC). SKEW adds 64 B to the pitch, which
// puts the rows one fragment read touches on distinct LDS banks.
template <int PIX, int CI, bool SKEW>
struct RowImage {
  static constexpr int ROW_BYTES = PIX * CI * 2;
  static constexpr int NCH = (ROW_BYTES + 1023) / 1024;  // chunks per row
  static constexpr int PITCH = NCH * 1024 + (SKEW ? 64 : 0);
  // of a full row: 16-pixel tiles per wave (4 waves), 32-pixel K windows
  static constexpr int MAXU = ((PIX - 4) / 16 + 3) / 4;
  static constexpr int WMAX = (PIX - 4) / 32;
};

// Copies rows ho0 .. of image n of the NHWC tensor `in` ([N][Hi][Wi][CI])
// into the row image dst_off bytes into `dst` (pitch PITCH, NCH chunks
// per row, nst = rows * NCH chunks in all): 1 KiB pieces round-robin
// over the block's 4 waves, 16 B granules, a granule that is not wholly
// inside the row from the zero page. With 4 channels a granule is 2
// pixels (Wi even keeps every granule wholly in or out), with 16 half a
// pixel. `dst` is the __shared__ array itself for the compiler's DMA
// form and its LDS byte address for the UNSEEN one.
template <int CI, int NCH, int PITCH, bool UNSEEN, typename Dst>
__device__ __forceinline__ void stage_rows(
    const bf16_t* __restrict__ const& in, long long n, const int& Hi,
    const int& Wi, int ho0, int nst, const int& wid, const int& lane,
    const Dst& dst, int dst_off) {
  static_assert(CI == 4 || CI == 16, "granule <-> pixel mapping");
  for (int t = wid; t < nst; t += 4) {
    const int ir = t / NCH;
    const int c = t - ir * NCH;
    const int slot = c * 64 + lane;              // 16B granule index
    bool in_row;
    long long col;                               // element offset in the row
    if constexpr (CI == 4) {
      const int pix = slot * 2;
      in_row = pix + 1 < Wi;
      col = (long long)pix * CI;
    } else {
      in_row = (slot >> 1) < Wi;
      col = (long long)slot * 8;
    }
    const bf16_t* src =
        in_row ? in + ((n * Hi + (ho0 + ir)) * (long long)Wi * CI + col)
               : conv5_zeros();
    if constexpr (UNSEEN)
      glds16_unseen(src, dst + dst_off + ir * PITCH + c * 1024);
    else
      glds16(src, const_cast<char*>(dst + dst_off + ir * PITCH + c * 1024));
  }
}

// ---- Fused max-pool: forward window, backward select

// bias-added 2x2 window (q0..q3 = (dy,dx) (0,0) (0,1) (1,0) (1,1)) ->
// pooled bf16 and argmax code; the first maximum wins, <= 0 clamps
__device__ __forceinline__ void pool_relu4(float q0, float q1, float q2,
                                           float q3, unsigned& ov,
                                           unsigned& code) {
  float mx = q0;
  unsigned arg = 0;
  if (q1 > mx) { mx = q1; arg = 1; }
  if (q2 > mx) { mx = q2; arg = 2; }
  if (q3 > mx) { mx = q3; arg = 3; }
  if (mx <= 0.0f) {
    ov = 0u;
    code = 255u;
  } else {
    ov = cf2bf(mx);
    code = arg;
  }
}

// Max-pool backward select shared by the kernels that stage a pooled
// gradient straight into LDS: 8 bf16 gradient values + their 8 argmax
// codes (0..3 = quadrant dy*2+dx, 255 = relu clamped) -> the 8 values of
// full-resolution position `quad`. Same select as
// k_relu_maxpool2_bwd_nhwc: code == quad ? g : 0, bit for bit.
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

// The wrw kernels' gout rows from the POOLED gradient + argmax mask
// (Ho, Wo even, so a block's 2 rows are pooled row bh of image n). Item
// `it` = threadIdx.x + i * THREADS is one 16 B granule (8 channels) of
// pooled pixel it / GV, GV = CO / 8 granules per pixel, contiguous in
// global memory along the row. The loads of the NEXT block wait in
// registers through this block's MFMA phase.
template <int NIT, int THREADS, int GV>
__device__ __forceinline__ void pooled_load(
    const bf16_t* __restrict__ const& gp,
    const uint8_t* __restrict__ const& mask, long long n, int bh,
    const int& Ho, const int& Wo, uint4 (&gq)[NIT], uint2 (&mq)[NIT]) {
  const int nreal = (Wo >> 1) * GV;
  const long long rowv = (n * (Ho >> 1) + bh) * (long long)(Wo >> 1) * GV;
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int it = threadIdx.x + i * THREADS;
    gq[i] = make_uint4(0u, 0u, 0u, 0u);
    mq[i] = make_uint2(~0u, ~0u);
    if (it < nreal) {
      gq[i] = reinterpret_cast<const uint4*>(gp)[rowv + it];
      mq[i] = reinterpret_cast<const uint2*>(mask)[rowv + it];
    }
  }
}

// The selects and ds_writes of those items: each expands to its 4 full-
// resolution positions in the per-o-tile [pix][16] gout image, whose
// row (dy, o-tile ot) is region ROW0 + dy * COT + ot of pitch PITCH,
// counted from BOFF bytes into `lds`. Items past the row (pooled pixel
// >= Wo/2) write the zero tail [Wo, 32*W) the K windows read.
template <int NIT, int THREADS, int COT, int BOFF, int ROW0, int PITCH,
          typename Lds>
__device__ __forceinline__ void pooled_write(Lds& lds, const int& W,
                                             const uint4 (&gq)[NIT],
                                             const uint2 (&mq)[NIT]) {
  constexpr int GV = COT * 2;
  const int nit = 16 * W * GV;
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int it = threadIdx.x + i * THREADS;
    if (it < nit) {
      const int wp = it / GV;
      const int rem = it - wp * GV;
      const int ot = rem >> 1;
      const int half = rem & 1;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          *reinterpret_cast<uint4*>(lds + BOFF +
                                    (ROW0 + dy * COT + ot) * PITCH +
                                    (2 * wp + dx) * 32 + half * 16) =
              unpool_select(gq[i], mq[i], dy * 2 + dx);
    }
  }
}

// ---- Packed epilogues

// 4x4 transpose of 16-bit values inside each lane quad (two DPP
// exchanges on packed pairs): every lane passes v0..v3 for ITS channel
// m; lane j = m & 3 of the quad returns v_j of channels (m & ~3) .. +3,
// packed low to high. All 64 lanes must be active.
__device__ __forceinline__ uint2 quad_tr4(unsigned v0, unsigned v1,
                                          unsigned v2, unsigned v3, int m) {
  const unsigned sel1 = (m & 1) ? 0x03020706u : 0x05040100u;
  const bool lo2 = (m & 3) < 2;
  const unsigned a = v0 | (v1 << 16);
  const unsigned b = v2 | (v3 << 16);
  // lane^1: a1 / b1 pair element (m&1) / 2+(m&1) of both lanes
  const unsigned a1 = __builtin_amdgcn_perm(
      (unsigned)__builtin_amdgcn_mov_dpp((int)a, 0xB1, 0xF, 0xF, true), a,
      sel1);
  const unsigned b1 = __builtin_amdgcn_perm(
      (unsigned)__builtin_amdgcn_mov_dpp((int)b, 0xB1, 0xF, 0xF, true), b,
      sel1);
  // lane^2: the lower lane pair keeps a1 and takes the upper pair's a1
  // as its channels 2..3; the upper pair mirrors it
  const unsigned snd = lo2 ? b1 : a1;
  const unsigned rcv =
      (unsigned)__builtin_amdgcn_mov_dpp((int)snd, 0x4E, 0xF, 0xF, true);
  return make_uint2(lo2 ? a1 : rcv, lo2 ? rcv : b1);
}

// four 16-bit codes (quad_tr4 of codes) -> four bytes
__device__ __forceinline__ unsigned pack_codes(uint2 c) {
  return __builtin_amdgcn_perm(c.y, c.x, 0x06040200u);
}

// ---- A fragments of the direct (register-only) kernels

// Chunks km = c*CH .. c*CH + CH - 1 of tile tw for the lane (pixel slot
// p, k-run q) of input row `row` of the image at element `in_n`, straight
// from global memory: one 16-byte load per chunk, zero past K and past
// the real row span S = 5 * CI. The kernels are interior-only: loads are
// always in-bounds once the lane's pixel is clamped to Wo-1, because
// (Wo-1) + 5 taps == Wi exactly.
template <int CI, int CH>
__device__ __forceinline__ void direct_a_chunk(
    const bf16_t* __restrict__ const& in, const long long& in_n, int tw,
    int c, const int& p, const int& q, const int& row, const int& Wi,
    const int& Wo, bf16x8 (&dst)[CH]) {
  constexpr int S = 5 * CI;             // real row span (elements)
  constexpr int Sp = (S + 7) & ~7;      // padded row span
  constexpr int K = 5 * Sp;
  constexpr int nK = (K + 31) / 32;
  const int wo_raw = (tw << 4) + p;
  const int wo = wo_raw < Wo ? wo_raw : (Wo - 1);
  const long long e_base = in_n + (long long)wo * CI +
                           (long long)row * (Wi * CI);
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int km = c * CH + j;
    const int k0 = km * 32 + q * 8;
    const int kh = k0 / Sp;
    const int j0 = k0 % Sp;
    dst[j] = (bf16x8)0;
    if (km < nK && k0 < K && j0 < S) {
      const long long e = e_base + (long long)kh * (Wi * CI) + j0;
      if (S - j0 >= 8) {
        dst[j] = *reinterpret_cast<const bf16x8*>(in + e);
      } else {  // 4 real + 4 zero-pad (conv1's Sp > S)
        const uint2 v = *reinterpret_cast<const uint2*>(in + e);
        union { uint4 u; bf16x8 h; } cv;
        cv.u = make_uint4(v.x, v.y, 0u, 0u);
        dst[j] = cv.h;
      }
    }
  }
}

// ---- Host: the row width a variant must stage

// A kernel that walks `tile`-pixel steps over Wo outputs reads 4 tap
// pixels past its last step and stages every pixel of the Wi-wide row.
static inline int conv5_stage_width(int Wo, int tile, int Wi) {
  const int walked = (Wo + tile - 1) / tile * tile + 4;
  return walked > Wi ? walked : Wi;
}
