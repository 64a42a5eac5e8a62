// k_conv5_pool2_nhwc, the LDS-staged conv1 form of the fused conv + bias
// + ReLU + max-pool stage (the block pipeline is described in conv.hip,
// with its conv2 sibling k_conv5_pool16_nhwc). In a header because its
// three input forms are built in three translation units: the bf16 form
// in conv.hip, the fp32 form in conv1x32.hip and the uint8 form in
// conv1u8.hip, which are compiled without packed fp32 instructions like
// the other newer kernel files.
#pragma once

#include <hip/hip_runtime.h>

#include "conv5_common.h"

#define CONV_THREADS 256  // 4 waves

// conv1 stage. A tile's chunk km reads, per conv row, 16 B at pixel wo
// of staged row r + kh (two ds_read_b64: odd wo is only 8 B aligned);
// slots past S hit the next pixel's data, zeroed by the Sp padding in
// w_frags. The walk is flattened over (tile, km): the reads of the next
// step are issued before the 4 MFMAs (one per conv row) of this one,
// across tiles too. A lane pools to 2 pixels x 2 pooled rows of channel
// m; quad_tr4 turns them into 4 channels of one (pooled row, pixel):
// one 8-byte out store and one 4-byte mask store per lane and tile.
//
// TIN = float is the form that reads the caller's fp32 3-channel image
// [N][Hi][Wi][3] itself (Wi % 4 == 0, 16 B aligned), so that no padded
// bf16 copy has to exist before the forward. A staging item is 4 pixels
// of one staged row: three 16 B loads (12 floats), cf2bf as the pad
// kernel, the zero 4th channel, two ds_write_b128. The loads of the NEXT
// block are issued after the barrier that opens the MFMA phase and wait
// in registers through it; the conversion and the ds_writes into the
// other image follow the phase. The bytes past pixel Wi of every row are
// zeroed once (nothing else writes them), so a staged row is byte for
// byte what the LDS-DMA of the padded copy gives, and the walk, the
// epilogue and out / mask are those of the bf16 form. With `xb` set,
// every block also stores the converted pixels of the input rows it
// owns (its first 4, and every staged row for the last block of an
// image: each row once) to xb [N][Hi][Wi][4], the padded bf16 copy the
// backward kernels read, from the registers that fed the ds_writes and
// behind the next block's loads, like the packed results.
//
// TIN = uint8_t is the same form for a uint8 image [N][Hi][Wi][3] (Wi % 4
// == 0, 4 B aligned) and a value table `tab`, bf16 [3][256]: pixel value
// v of channel c stands for tab[c][v], which is what cf2bf gives for the
// fp32 image x32 = table[c][x] when the host rounded the fp32 table to
// bf16. An item is the same 4 pixels, here 12 bytes in one 3-dword load
// (3 VGPRs in flight per item, not 12), and the conversion is 12
// ds_read_u16 from the table, which lies behind the two row images and
// is loaded once per workgroup ahead of the persistent loop. One lookup
// instruction reads one channel for all 64 lanes, so which banks the
// three channel tables start on does not matter to it. A channel's 512 B
// are 128 dwords: lanes whose values share a dword (v >> 1) are served
// together, lanes on different dwords of one bank serialise, so bytes
// that vary widely across a wave cost several passes per lookup. For
// values spread evenly the bank of a lookup is spread evenly whatever
// offset or copy a lane reads, so replicas would not lower that; the
// conflicts have not been counted. Everything
// from the ds_write_b128 on, xb included, is the fp32 form's.
template <int PIX, typename TIN = bf16_t>
__global__ __launch_bounds__(CONV_THREADS) void k_conv5_pool2_nhwc(
    const TIN* __restrict__ in,          // [N][Hi][Wi][4], fp32: ..[3]
    const bf16_t* __restrict__ w_frags,  // [1][nK][64][8]
    const float* __restrict__ bias,      // [16] or nullptr
    bf16_t* __restrict__ out,            // [N][Hop][Wop][16]
    uint8_t* __restrict__ mask,          // [N*Hop*Wop*16]
    int Nn, int Hi, int Wi, int Ho, int Wo,
    bf16_t* __restrict__ xb,             // fp32 / uint8 forms, or nullptr
    const bf16_t* __restrict__ tab = nullptr) {  // uint8 form: [3][256]
  constexpr bool X32 = sizeof(TIN) == 4;
  constexpr bool U8 = sizeof(TIN) == 1;
  constexpr bool XIN = X32 || U8;         // stages the caller's image
  constexpr int CI = 4;
  constexpr int S = 5 * CI;             // 20
  constexpr int Sp = (S + 7) & ~7;      // 24
  constexpr int K = 5 * Sp;             // 120
  constexpr int nK = (K + 31) / 32;     // 4
  constexpr int CO = 16;
  using Rows = RowImage<PIX, CI, true>;   // bank skew per row
  constexpr int NCHA = Rows::NCH;
  constexpr int ARPB = Rows::PITCH;
  constexpr int ROWS = 4;                 // conv rows per block
  constexpr int NROW = ROWS + 4;
  constexpr int IMG = NROW * ARPB;
  constexpr int MAXU = Rows::MAXU;        // tiles per wave
  constexpr int NS = MAXU * nK;           // steps of the walk
  constexpr int TAB = U8 ? 3 * 512 : 0;   // the value table's bytes
  __shared__ __attribute__((aligned(128))) char lds_rows[2 * IMG + TAB];

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  bf16x8 breg[nK];
#pragma unroll
  for (int i = 0; i < nK; ++i)
    breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  const float bias_v = bias ? bias[m] : 0.0f;

  const int Hop = Ho >> 1, Wop = Wo >> 1;
  const int tiles_w = (Wo + 15) >> 4;
  const int hblocks = (Hop + 1) >> 1;
  const long long n_blocks = (long long)Nn * hblocks;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const unsigned lds0 = lds_addr(lds_rows);

  // per-lane read address of (tile u, chunk km) in image 0, conv row 0.
  // A tile past the row clamps to the last pixel: in-bounds, never
  // stored. The one k-run past K (km 3, q 3) must be ZERO: those lanes
  // read the last 16 bytes of the row's staged kilobytes instead, which
  // lie past pixel PIX and are zero-filled in every staged row (a select
  // after the read cost 16 VALU per tile, 0.007 ms at the flagship).
  static_assert((nK - 1) * 32 + 2 * 8 < K && (nK - 1) * 32 + 3 * 8 >= K, "");
  static_assert(Rows::ROW_BYTES + 16 <= NCHA * 1024, "zero tail behind row");
  unsigned aofs[MAXU][nK];
#pragma unroll
  for (int u = 0; u < MAXU; ++u) {
    const int wo_raw = ((wid + 4 * u) << 4) + p;
    const int wo = wo_raw < Wo ? wo_raw : (Wo - 1);
#pragma unroll
    for (int km = 0; km < nK; ++km) {
      const int k0 = km * 32 + q * 8;
      aofs[u][km] = lds0 + (k0 < K ? (unsigned)(wo * (CI * 2) +
                                                (k0 / Sp) * ARPB +
                                                (k0 % Sp) * 2)
                                   : (unsigned)(NCHA * 1024 - 16));
    }
  }

  auto stage = [&](long long b, int img) {
    if constexpr (!XIN) {
      const long long n = b / hblocks;
      const int ho0 = (int)(b - n * hblocks) * ROWS;
      const int nrows = (Ho - ho0) < ROWS ? (Ho - ho0) : ROWS;
      stage_rows<CI, NCHA, ARPB, true>(in, n, Hi, Wi, ho0,
                                       (nrows + 4) * NCHA, wid, lane, lds0,
                                       img * IMG);
    }
  };

  // fp32 and uint8 forms. Item i of a thread is 4 pixels of staged row x_ir[i],
  // x_pix[i] pixels from the block's first one (rows are contiguous in
  // the image, so the same offset serves x and xb) and x_lds[i] bytes
  // into the row image; a row past the block's (x_ir >= staged rows,
  // always so for x_ir = NROW) is skipped.
  constexpr int XIT = XIN ? 2 : 0;
  static_assert(NROW * (PIX / 4) <= 2 * CONV_THREADS, "2 items per thread");
  struct U8x12 { unsigned a, b, c; };
  int x_ir[XIT + 1], x_pix[XIT + 1], x_lds[XIT + 1];
  float4 xq[(X32 ? XIT : 0) + 1][3];   // the next block's pixels, as loaded
  U8x12 xu[(U8 ? XIT : 0) + 1];        // the same, uint8 form
  uint4 xc[XIT + 1][2];    // the staged block's pixels, converted
  if constexpr (XIN) {
    const int ipr = Wi >> 2;
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
      const int it = threadIdx.x + i * CONV_THREADS;
      const int ir = it / ipr;
      const int j = it - ir * ipr;
      x_ir[i] = ir < NROW ? ir : NROW;
      x_pix[i] = ir * Wi + 4 * j;
      x_lds[i] = ir * ARPB + j * 32;
    }
    // the zero tail of all 2 * NROW rows, in 16 B granules
    for (int t = threadIdx.x; t < 2 * NROW * (NCHA * 64); t += CONV_THREADS) {
      const int g = t % (NCHA * 64);
      if (g * 16 >= Wi * (CI * 2))
        *reinterpret_cast<uint4*>(lds_rows + (t / (NCHA * 64)) * ARPB +
                                  g * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  if constexpr (U8) {
    // the table, once per workgroup; the barrier puts it ahead of the
    // first block's lookups
    for (int t = threadIdx.x; t < TAB / 4; t += CONV_THREADS)
      reinterpret_cast<unsigned*>(lds_rows + 2 * IMG)[t] =
          reinterpret_cast<const unsigned*>(tab)[t];
    __syncthreads();
  }
  // tab[c][v] from LDS
  auto lut = [&](int c, unsigned v) __attribute__((always_inline)) {
    return (unsigned)*(const __attribute__((address_space(3)))
                       unsigned short*)(uintptr_t)(lds0 + 2 * IMG + c * 512 +
                                                   v * 2);
  };
  // a block is (image n, first conv row ho0); the rows it stages
  auto x32_rows = [&](int ho0) {
    return ((Ho - ho0) < ROWS ? (Ho - ho0) : ROWS) + 4;
  };
  // nst: the block's staged rows, 0 for no block (behind a workgroup's
  // last one). Branch-free, in the loop too: an item past the rows loads
  // the first pixels of the block (of x, for no block) again. Loads under
  // a branch are waited for where its paths join.
  auto x32_load = [&](long long n, int ho0, int nst)
                      __attribute__((always_inline)) {
    if constexpr (U8) {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(in) +
                           (n * Hi + ho0) * (long long)Wi * 3;
#pragma unroll
      for (int i = 0; i < XIT; ++i) {
        const int pix = x_ir[i] < nst ? x_pix[i] : 0;
        xu[i] = *reinterpret_cast<const U8x12*>(src + (long long)pix * 3);
      }
    } else {
      const float* src = reinterpret_cast<const float*>(in) +
                         (n * Hi + ho0) * (long long)Wi * 3;
#pragma unroll
      for (int i = 0; i < XIT; ++i) {
        const int pix = x_ir[i] < nst ? x_pix[i] : 0;
        const float4* v =
            reinterpret_cast<const float4*>(src + (long long)pix * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) xq[i][k] = v[k];
      }
    }
  };
  auto x32_write = [&](int nst, int img) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
      unsigned w[8];
      if constexpr (U8) {
        // byte 3k + c of the item is channel c of its pixel k
        const unsigned d[3] = {xu[i].a, xu[i].b, xu[i].c};
        unsigned t[12];
#pragma unroll
        for (int j = 0; j < 12; ++j)
          t[j] = lut(j % 3, (d[j >> 2] >> ((j & 3) * 8)) & 0xFFu);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[2 * k] = t[3 * k] | (t[3 * k + 1] << 16);
          w[2 * k + 1] = t[3 * k + 2];
        }
      } else {
        const float f[12] = {xq[i][0].x, xq[i][0].y, xq[i][0].z, xq[i][0].w,
                             xq[i][1].x, xq[i][1].y, xq[i][1].z, xq[i][1].w,
                             xq[i][2].x, xq[i][2].y, xq[i][2].z, xq[i][2].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[2 * k] = (unsigned)cf2bf(f[3 * k]) |
                     ((unsigned)cf2bf(f[3 * k + 1]) << 16);
          w[2 * k + 1] = (unsigned)cf2bf(f[3 * k + 2]);
        }
      }
      xc[i][0] = make_uint4(w[0], w[1], w[2], w[3]);
      xc[i][1] = make_uint4(w[4], w[5], w[6], w[7]);
      if (x_ir[i] < nst) {
        uint4* d =
            reinterpret_cast<uint4*>(lds_rows + img * IMG + x_lds[i]);
        d[0] = xc[i][0];
        d[1] = xc[i][1];
      }
    }
  };
  // the rows of a block that no other block of its image stages first
  auto x32_store = [&](long long n, int ho0) __attribute__((always_inline)) {
    if (!xb) return;
    const int own = ho0 + ROWS < Ho ? ROWS : x32_rows(ho0);
    bf16_t* dst = xb + (n * Hi + ho0) * (long long)Wi * CI;
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
      if (x_ir[i] < own) {
        uint4* d = reinterpret_cast<uint4*>(dst + (long long)x_pix[i] * CI);
        d[0] = xc[i][0];
        d[1] = xc[i][1];
      }
    }
  };

  // packed results of one block: lane j = m & 3 holds channels
  // (m & ~3)..+3 of pooled row j >> 1, pooled pixel 2q + (j & 1) of tile u
  uint2 pko[MAXU];
  unsigned pkm[MAXU];
  auto flush = [&](long long n, int hb, int npr) {
    const int pr = (m & 3) >> 1;
    if (pr >= npr) return;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int wp = ((wid + 4 * u) << 3) + q * 2 + (m & 1);
      if (wp < Wop) {
        const long long off =
            ((n * Hop + (hb * 2 + pr)) * (long long)Wop + wp) * CO + (m & ~3);
        *reinterpret_cast<uint2*>(out + off) = pko[u];
        *reinterpret_cast<unsigned*>(mask + off) = pkm[u];
      }
    }
  };

  long long blk = wg;
  int img = 0;
  if (blk < n_blocks) stage(blk, 0);
  // fp32 / uint8 forms: the block whose pixels xc holds, and the one in
  // flight
  long long xn = 0;
  int xho0 = 0;
  if constexpr (XIN) {
    if (blk < n_blocks) {
      xn = blk / hblocks;
      xho0 = (int)(blk - xn * hblocks) * ROWS;
      x32_load(xn, xho0, x32_rows(xho0));
      x32_write(x32_rows(xho0), 0);
    }
  }
  long long pn = 0;
  int phb = 0, pnpr = 0;
  for (; blk < n_blocks; blk += n_wg, img ^= 1) {
    // (the fp32 and uint8 forms have no LDS-DMA in flight, and waiting
    // here would also wait for the previous block's stores)
    if constexpr (!XIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (blk + n_wg < n_blocks) stage(blk + n_wg, img ^ 1);
    long long xn_next = 0;
    int xho0_next = 0, xnst_next = 0;
    if constexpr (XIN) {
      if (blk + n_wg < n_blocks) {
        xn_next = (blk + n_wg) / hblocks;
        xho0_next = (int)(blk + n_wg - xn_next * hblocks) * ROWS;
        xnst_next = x32_rows(xho0_next);
      }
      x32_load(xn_next, xho0_next, xnst_next);
    }
    flush(pn, phb, pnpr);
    if constexpr (XIN) x32_store(xn, xho0);

    const long long n = blk / hblocks;
    const int hb = (int)(blk - n * hblocks);
    const unsigned ib = (unsigned)(img * IMG);
    auto ldk = [&](bf16x8(&d)[ROWS], int u, int km) {
      const unsigned a = aofs[u][km] + ib;
      typedef __attribute__((ext_vector_type(2))) unsigned uu2;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        union { struct { uu2 lo, hi; } p; bf16x8 h; } c;
        c.p.lo = *(const __attribute__((address_space(3)))
                   uu2*)(uintptr_t)(a + r * ARPB);
        c.p.hi = *(const __attribute__((address_space(3)))
                   uu2*)(uintptr_t)(a + r * ARPB + 8);
        d[r] = c.h;
      }
    };
    bf16x8 f[2][ROWS];
    ldk(f[0], 0, 0);
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      if (wid + 4 * u >= tiles_w) break;
      f32x4 acc[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) acc[r] = (f32x4)0.0f;
#pragma unroll
      for (int km = 0; km < nK; ++km) {
        const int s = u * nK + km;
        if (s + 1 < NS) ldk(f[(s + 1) & 1], (s + 1) / nK, (s + 1) % nK);
        // (fenced: left alone, the scheduler sinks the reads to their
        // MFMAs; 0.003-0.005 ms at the flagship)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              f[s & 1][r], breg[km], acc[r], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // conv pixel = tile*16 + q*4 + i: horizontal pairs are (i, i+1) of
      // one lane, vertical pairs two accumulators
      unsigned ov[2][2], cd[2][2];
#pragma unroll
      for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
          pool_relu4(acc[2 * pr][2 * pi] + bias_v,
                     acc[2 * pr][2 * pi + 1] + bias_v,
                     acc[2 * pr + 1][2 * pi] + bias_v,
                     acc[2 * pr + 1][2 * pi + 1] + bias_v, ov[pr][pi],
                     cd[pr][pi]);
      pko[u] = quad_tr4(ov[0][0], ov[0][1], ov[1][0], ov[1][1], m);
      pkm[u] = pack_codes(quad_tr4(cd[0][0], cd[0][1], cd[1][0], cd[1][1], m));
    }
    if constexpr (XIN) {
      // the other image was last read before this block's barrier
      x32_write(xnst_next, img ^ 1);
      xn = xn_next;
      xho0 = xho0_next;
    }
    pn = n;
    phb = hb;
    pnpr = (Ho - hb * ROWS) < ROWS ? 1 : 2;
  }
  flush(pn, phb, pnpr);
}
