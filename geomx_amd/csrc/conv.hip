// Direct 5x5 stride-1 convolution on MFMA for gfx950 — the flagship
// CNN's conv shapes (3->16 and 16->32 on 224/110 px, plus the padded
// transpose form for the data gradient), where MIOpen's igemm kernels
// run far from the memory floor.
//
// Formulation: implicit-GEMM. M = N*Ho*Wo output pixels, N = CO,
// K = 5 rows x Sp, Sp = round_up(5*CI, 8) elements per tap row
// ("row span"; NHWC makes (kw, ci) contiguous in memory, so every
// 8-element K-run of an MFMA A-fragment is ONE 16-byte load).
//
//   mfma_f32_16x16x32_bf16 per tile: 16 pixels x 16 outputs, K = 32.
//   A fragment: lane l = (q<<4)|p holds in[pixel p][k = km*32+q*8 .. +8]
//   B fragment: weights, PRE-PACKED on the host in exact per-lane
//     fragment order (w_frags[co_t][km][lane][8 bf16]), staged once per
//     block into LDS and read back with one ds_read_b128 per MFMA —
//     keeping them out of VGPRs preserves occupancy (the first version
//     held them in registers: 228 VGPRs -> 2 waves/SIMD, 2x slower
//     than MIOpen; this version: ~100 VGPRs -> 4-5 waves/SIMD).
//     The LDS-staged data-gradient kernel (k_conv5_lds_nhwc) is the
//     exception: its occupancy is set by the LDS row image, so it holds
//     all 25 fragments in registers and keeps B out of LDS.
//   C/D: lane l holds out[pixel (l>>4)*4+i][o = l&15], i = 0..3.
//
// Each wave owns whole (n, ho) output rows (row-walk: no per-tile
// 64-bit div/mod) and slides across the row's tiles with incremental
// addresses. The direct kernel is interior-only: the data-grad pass
// either zero-pads its input physically or runs the LDS-staged kernel,
// which materialises the border while staging.
//
// Requirements: CI % 4 == 0 (conv1's 3 channels are zero-padded to 4
// by the Python wrapper), CO % 16 == 0, kernel 5x5, stride 1.

#include <hip/hip_runtime.h>

#include "conv5_common.h"

#define CONV_THREADS 256  // 4 waves

template <int CI, int COT>
__global__ __launch_bounds__(CONV_THREADS) void k_conv5_nhwc(
    const bf16_t* __restrict__ in,       // [N][Hi][Wi][CI]
    const bf16_t* __restrict__ w_frags,  // [COT][nK][64][8]
    const float* __restrict__ bias,      // [CO] or nullptr
    bf16_t* __restrict__ out,            // [N][Ho][Wo][CO]
    int Nn, int Hi, int Wi, int Ho, int Wo) {
  constexpr int S = 5 * CI;             // real row span (elements)
  constexpr int Sp = (S + 7) & ~7;      // padded row span
  constexpr int K = 5 * Sp;
  constexpr int nK = (K + 31) / 32;
  constexpr int CO = COT * 16;

  // small variants (nK < 8, i.e. conv1) keep B fragments in REGISTERS
  // (<= 32 VGPRs) so the inner loop has no per-MFMA ds_read dependency;
  // large variants stage B into LDS shared by the block's 4 waves
  constexpr bool BREG = (nK < 8);
  __shared__ __attribute__((aligned(16))) short
      lds_b[BREG ? 8 : COT * nK * 64 * 8];
  if (!BREG) {
    for (int i = threadIdx.x; i < COT * nK * 64; i += blockDim.x) {
      reinterpret_cast<uint4*>(lds_b)[i] =
          reinterpret_cast<const uint4*>(w_frags)[i];
    }
    __syncthreads();
  }

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;        // pixel slot within a tile
  const int q = lane >> 4;        // k-run selector
  // this lane's B read base: ds_read_b128 at [(ct*nK+km)*64+lane]*16B
  const bf16x8* lds_bv = reinterpret_cast<const bf16x8*>(lds_b) + lane;

  bf16x8 breg[BREG ? COT * nK : 1];
  if (BREG) {
#pragma unroll
    for (int i = 0; i < COT * nK; ++i)
      breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  }

  float bias_v[COT];
#pragma unroll
  for (int ct = 0; ct < COT; ++ct)
    bias_v[ct] = bias ? bias[ct * 16 + (lane & 15)] : 0.0f;

  // per-(km,q) constants
  const int tiles_w = (Wo + 15) >> 4;
  const long long n_rows = (long long)Nn * Ho;
  const long long wave_id =
      ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;

  // per-lane k-run constants (kh, j0 depend only on q and km)
  for (long long row = wave_id; row < n_rows; row += n_waves) {
    const int ho = (int)(row % Ho);
    const long long n = row / Ho;
    const long long in_n = (long long)n * Hi * Wi * CI;
    const long long out_row = ((long long)n * Ho + ho) * (long long)Wo * CO;

    // chunked fragment loader (direct_a_chunk). CH frags per chunk keeps
    // the double-buffer register cost at 2*CH*4 VGPRs regardless of nK.
    constexpr int CH = (nK >= 8) ? 4 : nK;
    constexpr int nCH = (nK + CH - 1) / CH;
    auto load_chunk = [&](int tw, int c, bf16x8(&dst)[CH]) {
      direct_a_chunk<CI, CH>(in, in_n, tw, c, p, q, ho, Wi, Wo, dst);
    };

    // software pipeline: the NEXT chunk's loads are issued before this
    // chunk's MFMAs, so global-memory latency hides under matrix work
    // (without this the per-tile load->mfma chain parks waves 89% of
    // the time: SQ_WAIT_ANY/SQ_WAVE_CYCLES = 0.89 measured)
    bf16x8 af[CH];
    load_chunk(0, 0, af);

    for (int tw = 0; tw < tiles_w; ++tw) {
      f32x4 acc[COT];
#pragma unroll
      for (int ct = 0; ct < COT; ++ct) acc[ct] = (f32x4)0.0f;

#pragma unroll 1
      for (int c = 0; c < nCH; ++c) {
        bf16x8 afn[CH];
        if (c + 1 < nCH)
          load_chunk(tw, c + 1, afn);
        else if (tw + 1 < tiles_w)
          load_chunk(tw + 1, 0, afn);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int km = c * CH + j;
          if (km < nK) {
#pragma unroll
            for (int ct = 0; ct < COT; ++ct) {
              if constexpr (BREG)  // nCH==1 here, so km == j statically
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[j], breg[ct * nK + j], acc[ct], 0, 0, 0);
              else
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[j], lds_bv[(ct * nK + km) * 64], acc[ct], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) af[j] = afn[j];
      }

      // store: lane l covers pixels (l>>4)*4+i at channel l&15
      const int wo0 = tw << 4;
      const bool full = (wo0 + 16 <= Wo);
      const int o = lane & 15;
      const long long s_base = out_row + (long long)wo0 * CO + o;
      if (full) {
#pragma unroll
        for (int ct = 0; ct < COT; ++ct) {
          const long long sb = s_base + ct * 16;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            out[sb + (long long)(q * 4 + i) * CO] =
                cf2bf(acc[ct][i] + bias_v[ct]);
        }
      } else {
#pragma unroll
        for (int ct = 0; ct < COT; ++ct) {
          const long long sb = s_base + ct * 16;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int prow = q * 4 + i;
            if (wo0 + prow < Wo)
              out[sb + (long long)prow * CO] =
                  cf2bf(acc[ct][i] + bias_v[ct]);
          }
        }
      }
    }
  }
}


// ---------------------------------------------------------------------
// Fused conv(5x5, CI<=4 padded, CO=16) + bias + ReLU + 2x2 maxpool for
// the flagship conv1 stage: computes TWO conv rows per wave, pools them
// in-register and writes only the pooled row + the argmax-quadrant mask
// (the same uint8 code format k_relu_maxpool2_bwd consumes: 0..3 =
// quadrant (dy,dx), 255 = relu-clamped). Eliminates the full-resolution
// conv output round trip (1.55 GB write + read + 0.19 GB mask at the
// bench shape) and the separate pool kernel.
// ---------------------------------------------------------------------

template <int CI>
__global__ __launch_bounds__(CONV_THREADS) void k_conv5_pool_nhwc(
    const bf16_t* __restrict__ in,       // [N][Hi][Wi][CI]
    const bf16_t* __restrict__ w_frags,  // [1][nK][64][8]
    const float* __restrict__ bias,      // [16] or nullptr
    bf16_t* __restrict__ out,            // [N][Hop][Wop][16]
    uint8_t* __restrict__ mask,          // [N*Hop*Wop*16]
    int Nn, int Hi, int Wi, int Ho, int Wo) {
  constexpr int S = 5 * CI;
  constexpr int Sp = (S + 7) & ~7;
  constexpr int K = 5 * Sp;
  constexpr int nK = (K + 31) / 32;
  constexpr int CO = 16;
  static_assert(nK < 8, "register-B variant only");

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;
  const int q = lane >> 4;
  const int m = lane & 15;

  bf16x8 breg[nK];
#pragma unroll
  for (int i = 0; i < nK; ++i)
    breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  const float bias_v = bias ? bias[m] : 0.0f;

  const int Hop = Ho >> 1, Wop = Wo >> 1;
  const int tiles_w = (Wo + 15) >> 4;
  const long long n_rows = (long long)Nn * Hop;
  const long long wave_id =
      ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;

  for (long long row = wave_id; row < n_rows; row += n_waves) {
    const int hp = (int)(row % Hop);
    const long long n = row / Hop;
    const int ho0 = hp * 2;
    const long long in_n = (long long)n * Hi * Wi * CI;
    const long long out_row =
        ((long long)n * Hop + hp) * (long long)Wop * CO;

    auto load_row = [&](int tw, int r, bf16x8(&dst)[nK]) {
      direct_a_chunk<CI, nK>(in, in_n, tw, 0, p, q, ho0 + r, Wi, Wo, dst);
    };

    bf16x8 af0[nK], af1[nK];
    load_row(0, 0, af0);
    load_row(0, 1, af1);
    for (int tw = 0; tw < tiles_w; ++tw) {
      f32x4 a0 = (f32x4)0.0f, a1 = (f32x4)0.0f;
      bf16x8 nf0[nK], nf1[nK];
      if (tw + 1 < tiles_w) {
        load_row(tw + 1, 0, nf0);
        load_row(tw + 1, 1, nf1);
      }
#pragma unroll
      for (int km = 0; km < nK; ++km) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0[km], breg[km], a0,
                                                     0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1[km], breg[km], a1,
                                                     0, 0, 0);
      }
#pragma unroll
      for (int km = 0; km < nK; ++km) { af0[km] = nf0[km]; af1[km] = nf1[km]; }

      // pool: conv pixel = tw*16 + q*4 + i; horizontal pairs live in
      // (i, i+1) of the SAME lane, vertical in (a0, a1)
      const int wo0 = tw << 4;
#pragma unroll
      for (int pi = 0; pi < 2; ++pi) {
        const int i0 = pi * 2;
        const int wp = (wo0 + q * 4 + i0) >> 1;
        if (wp >= Wop) continue;
        // (pool_relu4 written out: through the helper this kernel
        // measured 0.35 % slower, docs/kernels.md)
        const float q0 = a0[i0] + bias_v;      // (dy,dx)=(0,0)
        const float q1 = a0[i0 + 1] + bias_v;  // (0,1)
        const float q2 = a1[i0] + bias_v;      // (1,0)
        const float q3 = a1[i0 + 1] + bias_v;  // (1,1)
        float mx = q0;
        int arg = 0;
        if (q1 > mx) { mx = q1; arg = 1; }
        if (q2 > mx) { mx = q2; arg = 2; }
        if (q3 > mx) { mx = q3; arg = 3; }
        bf16_t ov;
        uint8_t code;
        if (mx <= 0.0f) {
          ov = (bf16_t)0;
          code = 255;
        } else {
          ov = cf2bf(mx);
          code = (uint8_t)arg;
        }
        const long long o_off = out_row + (long long)wp * CO + m;
        out[o_off] = ov;
        mask[o_off] = code;
      }
    }
  }
}


// ---------------------------------------------------------------------
// LDS-staged forms of the fused conv + bias + ReLU + max-pool stage:
// k_conv5_pool2_nhwc (conv1, CI = 4 padded, CO = 16) and
// k_conv5_pool16_nhwc (conv2, CI = 16, CO = 16 / 32). Both are
// persistent: a block is FOUR conv rows (two pooled rows) of one image,
// staged once as 8 input rows by LDS-DMA (16 B granules, straight NHWC
// copy) into one of two row images. The 4 waves split the 16-pixel
// tiles and read A fragments from LDS; the weight fragments stay in
// registers for the whole loop.
//
//   top of a block:   wait for this block's image, barrier
//                     issue the NEXT block's DMA into the other image
//                     store the PREVIOUS block's packed results
//                     MFMA phase, pool, pack into registers
//
// so neither the staging round trip nor the stores sit in front of an
// MFMA phase, and there is one barrier per block (it also orders the
// previous phase's reads of the other image before the DMA that
// overwrites it). With an odd number of pooled rows the last block of
// an image stages 6 rows and stores one pooled row; its lower two conv
// rows read older LDS data into accumulators that are never stored.
//
// Every accumulator (conv row, tile, co-tile) receives chunks km =
// 0..nK-1 in ascending order with the fragment contents of the 2-row
// kernels these replace (and of k_conv5_pool_nhwc), so out and mask are
// bit-identical to theirs.
// ---------------------------------------------------------------------

// conv1 stage. A tile's chunk km reads, per conv row, 16 B at pixel wo
// of staged row r + kh (two ds_read_b64: odd wo is only 8 B aligned);
// slots past S hit the next pixel's data, zeroed by the Sp padding in
// w_frags. The walk is flattened over (tile, km): the reads of the next
// step are issued before the 4 MFMAs (one per conv row) of this one,
// across tiles too. A lane pools to 2 pixels x 2 pooled rows of channel
// m; quad_tr4 turns them into 4 channels of one (pooled row, pixel):
// one 8-byte out store and one 4-byte mask store per lane and tile.
template <int PIX>
__global__ __launch_bounds__(CONV_THREADS) void k_conv5_pool2_nhwc(
    const bf16_t* __restrict__ in,       // [N][Hi][Wi][4]
    const bf16_t* __restrict__ w_frags,  // [1][nK][64][8]
    const float* __restrict__ bias,      // [16] or nullptr
    bf16_t* __restrict__ out,            // [N][Hop][Wop][16]
    uint8_t* __restrict__ mask,          // [N*Hop*Wop*16]
    int Nn, int Hi, int Wi, int Ho, int Wo) {
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
  __shared__ __attribute__((aligned(128))) char lds_rows[2 * IMG];

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
    const long long n = b / hblocks;
    const int ho0 = (int)(b - n * hblocks) * ROWS;
    const int nrows = (Ho - ho0) < ROWS ? (Ho - ho0) : ROWS;
    stage_rows<CI, NCHA, ARPB, true>(in, n, Hi, Wi, ho0, (nrows + 4) * NCHA,
                                     wid, lane, lds0, img * IMG);
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
  long long pn = 0;
  int phb = 0, pnpr = 0;
  for (; blk < n_blocks; blk += n_wg, img ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (blk + n_wg < n_blocks) stage(blk + n_wg, img ^ 1);
    flush(pn, phb, pnpr);

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
    pn = n;
    phb = hb;
    pnpr = (Ho - hb * ROWS) < ROWS ? 1 : 2;
  }
  flush(pn, phb, pnpr);
}


// conv2 stage (CO = COT*16). With CI = 16 a tap row is 80 K-slots = 2.5
// chunks, so along K a conv row's operand is the row image read linearly
// from its first staged row: "linear fragment" t of row parity par is
// k-run t*32 + q*8 counted from staged row par, and
//
//     A(row par,     chunk km) = F(par, km)
//     A(row par + 2, chunk km) = F(par, km + 5)
//
// Rows par and par + 2 share one walk over t = 0..17 (18 ds_read_b128
// for 26*COT MFMAs; the 2-row kernel read 26 A and 26*COT B fragments
// for them). Chunk 12 is the exception: its k-runs q >= 2 lie past K
// and must be ZERO (the staged data there is finite only by luck), but
// F(par, 12) is also chunk 7 of row par + 2, which needs the real data.
// The walk therefore feeds chunk 12 a copy with lanes q >= 2 zeroed
// (t = 12 for row par, t = 17 for row par + 2). F(1, 17) of those lanes
// would lie one row past the image: the image pair is followed by one
// spare row, so the read stays inside the allocation.
// The COT*13 weight fragments live in registers (104 VGPRs at COT = 2);
// two 8-row images of 4160 B rows + the spare row are 70.7 KB, 2
// workgroups per CU. Reads run two steps ahead of their MFMAs through
// both parities and into the wave's next tile.
template <int COT, int PIX>
__global__ __launch_bounds__(CONV_THREADS, 2) void k_conv5_pool16_nhwc(
    const bf16_t* __restrict__ in,       // [N][Hi][Wi][16]
    const bf16_t* __restrict__ w_frags,  // [COT][nK][64][8]
    const float* __restrict__ bias,      // [CO] or nullptr
    bf16_t* __restrict__ out,            // [N][Hop][Wop][CO]
    uint8_t* __restrict__ mask,          // [N*Hop*Wop*CO]
    int Nn, int Hi, int Wi, int Ho, int Wo) {
  constexpr int CI = 16;
  constexpr int S = 5 * CI;             // 80, already a multiple of 8
  constexpr int K = 5 * S;              // 400
  constexpr int nK = (K + 31) / 32;     // 13
  constexpr int CO = COT * 16;
  using Rows = RowImage<PIX, CI, true>;
  constexpr int NCHA = Rows::NCH;
  constexpr int ARPB = Rows::PITCH;
  constexpr int ROWS = 4;
  constexpr int NROW = ROWS + 4;
  constexpr int IMG = NROW * ARPB;
  constexpr int NT = nK + 5;            // linear fragments per parity
  constexpr int MAXU = Rows::MAXU;
  constexpr int NS = MAXU * 2 * NT;     // steps of the walk
  static_assert(NT % 3 == 0, "three fragment sets rotate per parity");
  __shared__ __attribute__((aligned(128))) char lds_all[2 * IMG + ARPB];

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  bf16x8 breg[COT * nK];
#pragma unroll
  for (int i = 0; i < COT * nK; ++i)
    breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  float bias_v[COT];
#pragma unroll
  for (int ct = 0; ct < COT; ++ct)
    bias_v[ct] = bias ? bias[ct * 16 + m] : 0.0f;

  const int Hop = Ho >> 1, Wop = Wo >> 1;
  const int tiles_w = (Wo + 15) >> 4;
  const int hblocks = (Hop + 1) >> 1;
  const long long n_blocks = (long long)Nn * hblocks;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const unsigned lds0 = lds_addr(lds_all);

  // linear fragment t sits at foff[t % 5] + 2 * (t / 5) rows
  unsigned foff[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int k0 = t * 32 + q * 8;
    foff[t] = (unsigned)((k0 / S) * ARPB + (k0 % S) * 2);
  }
  const bool qlo = q < 2;
  unsigned wofs[MAXU];
#pragma unroll
  for (int u = 0; u < MAXU; ++u) {
    const int wo_raw = ((wid + 4 * u) << 4) + p;
    wofs[u] = lds0 + (unsigned)((wo_raw < Wo ? wo_raw : (Wo - 1)) * (CI * 2));
  }

  auto stage = [&](long long b, int img) {
    const long long n = b / hblocks;
    const int ho0 = (int)(b - n * hblocks) * ROWS;
    const int nrows = (Ho - ho0) < ROWS ? (Ho - ho0) : ROWS;
    stage_rows<CI, NCHA, ARPB, true>(in, n, Hi, Wi, ho0, (nrows + 4) * NCHA,
                                     wid, lane, lds0, img * IMG);
  };

  // packed results of one block, lane j = m & 3 of a quad, channels
  // (m & ~3)..+3. COT = 2: [u][pooled row], pixel 2q + (j >> 1) of
  // co-tile j & 1. COT = 1: [u][0], pooled row j >> 1, pixel 2q + (j & 1).
  uint2 pko[MAXU][COT];
  unsigned pkm[MAXU][COT];
  auto flush = [&](long long n, int hb, int npr) {
    const int j = m & 3;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
#pragma unroll
      for (int e = 0; e < COT; ++e) {
        const int pr = COT == 2 ? e : (j >> 1);
        const int pi = COT == 2 ? (j >> 1) : (j & 1);
        const int ch = (COT == 2 ? (j & 1) * 16 : 0) + (m & ~3);
        const int wp = ((wid + 4 * u) << 3) + q * 2 + pi;
        if (pr < npr && wp < Wop) {
          const long long off =
              ((n * Hop + (hb * 2 + pr)) * (long long)Wop + wp) * CO + ch;
          *reinterpret_cast<uint2*>(out + off) = pko[u][e];
          *reinterpret_cast<unsigned*>(mask + off) = pkm[u][e];
        }
      }
    }
  };

  long long blk = wg;
  int img = 0;
  if (blk < n_blocks) stage(blk, 0);
  long long pn = 0;
  int phb = 0, pnpr = 0;
  for (; blk < n_blocks; blk += n_wg, img ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (blk + n_wg < n_blocks) stage(blk + n_wg, img ^ 1);
    flush(pn, phb, pnpr);

    const long long n = blk / hblocks;
    const int hb = (int)(blk - n * hblocks);
    const unsigned ib = (unsigned)(img * IMG);
    // 5 read bases per tile; every other address is an immediate offset
    // from one of them. (Opaque to the compiler, which otherwise keeps
    // one loop-invariant address register per read of the walk: 72.)
    unsigned fb[MAXU][5];
#pragma unroll
    for (int u = 0; u < MAXU; ++u)
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        fb[u][j] = wofs[u] + ib + foff[j];
        asm volatile("" : "+v"(fb[u][j]));
      }
    // step s = (tile u, parity, t)
    auto ldf = [&](int s) {
      const int u = s / (2 * NT);
      const int par = (s / NT) & 1;
      const int t = s % NT;
      return *(const __attribute__((address_space(3))) bf16x8*)(uintptr_t)(
          fb[u][t % 5] + (par + 2 * (t / 5)) * ARPB);
    };
    bf16x8 f[3];
    f[0] = ldf(0);
    f[1] = ldf(1);
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      if (wid + 4 * u >= tiles_w) break;
      f32x4 acc[ROWS][COT];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int ct = 0; ct < COT; ++ct) acc[r][ct] = (f32x4)0.0f;
#pragma unroll
      for (int par = 0; par < 2; ++par) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int s = (u * 2 + par) * NT + t;
          if (s + 2 < NS) f[(s + 2) % 3] = ldf(s + 2);
          // keeps the read two steps ahead (and not twenty: unfenced,
          // the scheduler hoists reads until the registers run out)
          __builtin_amdgcn_sched_barrier(0);
          const bf16x8 cur = f[s % 3];
          const bf16x8 curz = qlo ? cur : (bf16x8)0;
          if (t < nK) {         // chunk t of conv row par
#pragma unroll
            for (int ct = 0; ct < COT; ++ct)
              acc[par][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  t == nK - 1 ? curz : cur, breg[ct * nK + t], acc[par][ct],
                  0, 0, 0);
          }
          if (t >= 5) {         // chunk t - 5 of conv row par + 2
#pragma unroll
            for (int ct = 0; ct < COT; ++ct)
              acc[par + 2][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  t == NT - 1 ? curz : cur, breg[ct * nK + t - 5],
                  acc[par + 2][ct], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      unsigned ov[2][COT][2], cd[2][COT][2];
#pragma unroll
      for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int ct = 0; ct < COT; ++ct)
#pragma unroll
          for (int pi = 0; pi < 2; ++pi)
            pool_relu4(acc[2 * pr][ct][2 * pi] + bias_v[ct],
                       acc[2 * pr][ct][2 * pi + 1] + bias_v[ct],
                       acc[2 * pr + 1][ct][2 * pi] + bias_v[ct],
                       acc[2 * pr + 1][ct][2 * pi + 1] + bias_v[ct],
                       ov[pr][ct][pi], cd[pr][ct][pi]);
      if constexpr (COT == 2) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          pko[u][pr] = quad_tr4(ov[pr][0][0], ov[pr][1][0], ov[pr][0][1],
                                ov[pr][1][1], m);
          pkm[u][pr] = pack_codes(quad_tr4(cd[pr][0][0], cd[pr][1][0],
                                           cd[pr][0][1], cd[pr][1][1], m));
        }
      } else {
        pko[u][0] = quad_tr4(ov[0][0][0], ov[0][0][1], ov[1][0][0],
                             ov[1][0][1], m);
        pkm[u][0] = pack_codes(quad_tr4(cd[0][0][0], cd[0][0][1],
                                        cd[1][0][0], cd[1][0][1], m));
      }
    }
    pn = n;
    phb = hb;
    pnpr = (Ho - hb * ROWS) < ROWS ? 1 : 2;
  }
  flush(pn, phb, pnpr);
}


// LDS-staged DENSE conv for the conv2 data-gradient: CI=32 (the padded
// grad-out), CO=16 (the dgrad output channels), full-resolution output.
//
// With CI=32 the row span is S = Sp = 160 = 5 chunks of 32, so chunk km
// is exactly (kh = km/5, j = km%5) and its A fragment is pixel wo+j of
// staged row (output row + kh): lane (p, q) holds channels q*8..+8. The
// fragment (staged row r, j) is therefore the A operand of output row
// r-kh with weight fragment kh*5+j for EVERY kh in 0..4. A wave's work
// unit is (16-pixel tile, ROWS=4 output rows): it walks the ROWS+4
// staged rows top to bottom, reads each row's 5 fragments ONCE and
// issues up to 5 MFMAs per fragment into the per-output-row
// accumulators (40 ds_read_b128 per 100 MFMAs; the 2-row kernel before
// it read one A and one B fragment per MFMA). Each accumulator still
// receives its 25 MFMAs in ascending km with the fragments of the
// direct kernel, so the output is bit-identical to k_conv5_nhwc<32,1>.
//
// The 25 weight fragments live in REGISTERS (100 VGPRs) for the whole
// persistent loop: occupancy here is set by the LDS row image, not by
// registers, and the B panel leaves LDS. The next staged row's
// fragments are loaded before this row's MFMAs are issued (the walk is
// fully unrolled, so the compiler places counted lgkmcnt waits). The
// UNPOOL variants also issue the NEXT block's global loads before the
// MFMA phase and do the selects + ds_writes after the barrier that
// ends it, which takes global latency off the critical path.
template <int CIT, int COT, int PIX, int PAD = 0, bool UNPOOL = false>
__global__ __launch_bounds__(CONV_THREADS, (PIX <= 120 ? 2 : 1))
void k_conv5_lds_nhwc(
    const bf16_t* __restrict__ in,   // [N][Hi-2P][Wi-2P][CI] (P virtual)
    const bf16_t* __restrict__ w_frags,  // [COT][nK][64][8]
    const float* __restrict__ bias,      // [CO] or nullptr
    bf16_t* __restrict__ out,            // [N][Ho][Wo][CO]
    int Nn, int Hi, int Wi, int Ho, int Wo,
    const uint8_t* __restrict__ mask) {  // UNPOOL: argmax codes, as `in`
  // PAD>0: `in` is the UNPADDED tensor; the staging pass materialises
  // the zero border directly in LDS (granules map within one pixel for
  // CI>=8, so the border test is per-granule)
  // UNPOOL (CI=32, PAD=4, Ho and Wo even): `in` is the max-POOLED
  // tensor [N][(Hi-8)/2][(Wi-8)/2][CI] and `mask` its argmax codes; the
  // staging pass expands each pooled pixel to its 4 full-resolution
  // positions, so LDS holds what the PAD=4 staging of the scattered
  // gradient would
  static_assert(CIT == 32 && COT == 1, "conv2 dgrad only");
  static_assert(!UNPOOL || PAD == 4, "the pooled form has a virtual border");
  constexpr int CI = CIT;
  constexpr int nK = 25;                 // (kh, j), 5 chunks per tap row
  constexpr int CO = 16;
  using Rows = RowImage<PIX, CI, true>;
  constexpr int NCHA = Rows::NCH;
  constexpr int ARPB = Rows::PITCH;
  constexpr int ROWS = 4;                // output rows per block
  constexpr int NROW = ROWS + 4;         // staged input rows
  constexpr int MAXU = Rows::MAXU;       // units per wave
  __shared__ __attribute__((aligned(128))) char lds_all[NROW * ARPB];

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = threadIdx.x >> 6;

  // weight fragments: one bf16x8 per (km, lane), held for every block
  bf16x8 breg[nK];
#pragma unroll
  for (int i = 0; i < nK; ++i)
    breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  const float bias_v = bias ? bias[m] : 0.0f;

  const int tiles_w = (Wo + 15) >> 4;
  const int hblocks = (Ho + ROWS - 1) / ROWS;
  const long long n_blocks = (long long)Nn * hblocks;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const unsigned lds0 = lds_addr(lds_all);

  // UNPOOL staging. Staged row ir is real row ho0 + ir - 4 and staged
  // pixel pix is real pixel pix - 4, both even-aligned: the 8 rows are
  // pooled rows (ho0>>1) - 2 + k, k = 0..3, and pixels (2pp, 2pp+1) are
  // pooled pixel pp - 2. Item `it` = (k, pp, s): channel granule s
  // (8 channels, 16 B + 8 mask bytes, contiguous in global memory
  // along (pp, s)) of one pooled pixel, written to its 4 full-
  // resolution positions under the same XOR swizzle as the LDS-DMA
  // staging (granule s sits at sub-slot s ^ ((pix>>2)&3), and pix>>2 ==
  // pp>>1 for both pixels). Items outside the image write the zero
  // border / tail. unp_load issues the global loads of one block into
  // registers; unp_write does the selects and ds_writes.
  constexpr int PPR = NCHA * 8;          // pooled pixels per LDS row
  constexpr int IPR = PPR * 4;           // items per pooled row
  constexpr int NPR = NROW / 2;          // pooled rows per block
  constexpr int NIT =
      UNPOOL ? (NPR * IPR + CONV_THREADS - 1) / CONV_THREADS : 1;
  uint4 gq[NIT];
  uint2 mq[NIT];
  auto unp_load = [&](long long b) __attribute__((always_inline)) {
    const int ho0 = (int)(b % hblocks) * ROWS;
    const long long n = b / hblocks;
    const int Hp = (Hi - 8) >> 1, Wp = (Wi - 8) >> 1;
    const int pr0 = (ho0 >> 1) - 2;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = threadIdx.x + i * CONV_THREADS;
      const int k = it / IPR;
      const int rem = it - k * IPR;
      const int pr = pr0 + k;
      const int wp = (rem >> 2) - 2;
      // (predicated loads: a branch-free form that loads a clamped
      // address for border items measured 0.01 ms/step slower)
      gq[i] = make_uint4(0u, 0u, 0u, 0u);
      mq[i] = make_uint2(~0u, ~0u);
      if (k < NPR && pr >= 0 && pr < Hp && wp >= 0 && wp < Wp) {
        const long long v =
            ((n * Hp + pr) * (long long)Wp + wp) * 4 + (rem & 3);
        gq[i] = reinterpret_cast<const uint4*>(in)[v];
        mq[i] = reinterpret_cast<const uint2*>(mask)[v];
      }
    }
  };
  auto unp_write = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = threadIdx.x + i * CONV_THREADS;
      const int k = it / IPR;
      const int rem = it - k * IPR;
      const int pp = rem >> 2;
      const int sub = (rem & 3) ^ ((pp >> 1) & 3);
      if (k < NPR) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx)
            *reinterpret_cast<uint4*>(lds_all + (2 * k + dy) * ARPB +
                                      (2 * pp + dx) * 64 + sub * 16) =
                unpool_select(gq[i], mq[i], dy * 2 + dx);
      }
    }
  };
  if constexpr (UNPOOL) {
    if (wg < n_blocks) {
      unp_load(wg);
      unp_write();
    }
  }

  for (long long blk = wg; blk < n_blocks; blk += n_wg) {
    const int hb = (int)(blk % hblocks);
    const long long n = blk / hblocks;
    const int ho0 = hb * ROWS;
    const int nrows = (Ho - ho0) < ROWS ? (Ho - ho0) : ROWS;
    // LDS-DMA staging of the rows this block's outputs read; with
    // nrows < ROWS the rows below keep older data, which only reaches
    // accumulators that are never stored
    const int nstage = UNPOOL ? 0 : (nrows + 4) * NCHA;
    for (int t = wid; t < nstage; t += 4) {
      const int ir = t / NCHA;
      const int c = t - ir * NCHA;
      const int slot = c * 64 + lane;
      const int pix = (slot * 16) / (CI * 2);      // 16B granule -> pixel
      // CI=32: a pixel is exactly one 64-dword bank row, so un-swizzled
      // fragment reads are 4-way bank conflicted; XOR the granule index
      // with (pix>>2)&3 on the SOURCE (dest stays lane-linear, guide
      // rule 21) and apply the same XOR at the read
      long long sslot = slot;
      if (CI == 32) {
        const int sub = slot & 3;
        sslot = (slot & ~3LL) | (sub ^ ((pix >> 2) & 3));
      }
      const bf16_t* src;
      if (PAD == 0) {
        src = (pix < Wi) ? in + ((n * Hi + (ho0 + ir)) * (long long)Wi * CI +
                               sslot * 8)
                         : conv5_zeros();
      } else {
        const int rrow = ho0 + ir - PAD;
        const int rpix = pix - PAD;
        const int rWi = Wi - 2 * PAD;
        const bool ok = rrow >= 0 && rrow < (Hi - 2 * PAD) && rpix >= 0 &&
                        rpix < rWi;
        // sslot relative to the real pixel: subtract the border columns
        src = ok ? in + ((n * (Hi - 2 * PAD) + rrow) * (long long)rWi * CI +
                         (sslot - (long long)PAD * (CI / 8)) * 8)
                 : conv5_zeros();
      }
      glds16(src, lds_all + ir * ARPB + c * 1024);
    }
    // (the pooled form has no LDS-DMA in flight here, and waiting would
    // also wait for the previous block's output stores)
    if constexpr (!UNPOOL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the next block's pooled rows travel while this block computes
    const bool has_next = UNPOOL && blk + n_wg < n_blocks;
    if constexpr (UNPOOL) {
      if (has_next) unp_load(blk + n_wg);
    }

    // a wave's units are tiles wid, wid+4, ...; their packed outputs
    // wait in registers (2 per row) until the staging of the next block
    // is done, so that the wait for the prefetched loads above never
    // covers a store that was issued after them
    uint2 pk[MAXU][ROWS] = {};
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int tw = wid + 4 * u;
      if (tw >= tiles_w) break;
      const int wo_raw = (tw << 4) + p;
      const int wo = wo_raw < Wo ? wo_raw : (Wo - 1);
      // chunk j of a staged row is pixel wo+j: granule q under the
      // staging XOR ((pixel>>2)&3)
      unsigned aoff[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int Pp = wo + j;
        aoff[j] = lds0 + (unsigned)((Pp * 4 + (q ^ ((Pp >> 2) & 3))) * 16);
      }
      auto load_row = [&](int r, bf16x8(&dst)[5]) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
          dst[j] = *(const __attribute__((address_space(3)))
                     bf16x8*)(uintptr_t)(aoff[j] + r * ARPB);
      };
      f32x4 acc[ROWS];
#pragma unroll
      for (int o = 0; o < ROWS; ++o) acc[o] = (f32x4)0.0f;
      bf16x8 af[5];
      load_row(0, af);
#pragma unroll
      for (int r = 0; r < NROW; ++r) {
        bf16x8 afn[5];
        if (r + 1 < NROW) load_row(r + 1, afn);
        // staged row r is tap row kh = r - o of output row o; per
        // accumulator the MFMAs arrive in ascending km = kh*5 + j
#pragma unroll
        for (int j = 0; j < 5; ++j) {
#pragma unroll
          for (int o = 0; o < ROWS; ++o) {
            const int kh = r - o;
            if (kh >= 0 && kh < 5)
              acc[o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[j], breg[kh * 5 + j], acc[o], 0, 0, 0);
          }
        }
        if (r + 1 < NROW) {
#pragma unroll
          for (int j = 0; j < 5; ++j) af[j] = afn[j];
        }
      }
      // Lane (q, m) holds pixels q*4+i of channel m. quad_tr4 gives it
      // channels (m&~3)..+3 of pixel q*4+(m&3): one 8-byte store, 512
      // contiguous bytes per wave and row, in place of four 2-byte
      // stores.
#pragma unroll
      for (int o = 0; o < ROWS; ++o) {
        unsigned v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = cf2bf(acc[o][i] + bias_v);
        pk[u][o] = quad_tr4(v[0], v[1], v[2], v[3], m);
      }
    }
    __syncthreads();
    if constexpr (UNPOOL) {
      if (has_next) unp_write();
    }
    const long long out_row0 =
        ((long long)n * Ho + ho0) * (long long)Wo * CO;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int spix = ((wid + 4 * u) << 4) + q * 4 + (m & 3);
      if (spix < Wo) {
        const long long sb = out_row0 + (long long)spix * CO + (m & ~3);
#pragma unroll
        for (int o = 0; o < ROWS; ++o)
          if (o < nrows)
            *reinterpret_cast<uint2*>(out + sb + (long long)o * Wo * CO) =
                pk[u][o];
      }
    }
  }
}

// NHWC channel pad: [N,H,W,3] (fp32 or bf16) -> [N,H,W,4] bf16 with a
// zero 4th channel. One thread per OUTPUT pixel: reads 3 elems, writes
// one 8-byte bf16x4.
template <typename TIN>
__global__ void k_pad_ch3to4_nhwc(const TIN* __restrict__ in,
                                  bf16_t* __restrict__ out,
                                  long long npix) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = tid; i < npix; i += stride) {
    bf16_t v[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const TIN x = in[i * 3 + c];
      if constexpr (sizeof(TIN) == 4) {
        v[c] = cf2bf((float)x);
      } else {
        v[c] = (bf16_t)x;
      }
    }
    v[3] = 0;
    *reinterpret_cast<uint2*>(out + i * 4) = *reinterpret_cast<uint2*>(v);
  }
}

// Weight packing: the OIHW fp32 weight to per-lane MFMA B-fragment order
// in bf16, out[i] = idx[i] == numel ? 0 : bf16(w[idx[i]]) (round to
// nearest even, as Tensor.to(bfloat16) for finite values), for up to two
// gather tables (ops/conv.py _frag_index) in one launch: the forward
// and the data-gradient fragments of a layer come from one read of its
// weight. One thread per 8 elements (a fragment lane's 16 B); an index
// outside [0, numel) reads nothing and gives zero.
__global__ __launch_bounds__(256) void k_conv5_pack_frags(
    const float* __restrict__ w, long long numel,
    const long long* __restrict__ idx0, bf16_t* __restrict__ out0,
    long long n0, const long long* __restrict__ idx1,
    bf16_t* __restrict__ out1, long long n1) {
  long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long* idx = idx0;
  bf16_t* out = out0;
  if (g >= n0 / 8) {
    g -= n0 / 8;
    if (g >= n1 / 8) return;
    idx = idx1;
    out = out1;
  }
  __attribute__((aligned(16))) bf16_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long e = idx[g * 8 + j];
    v[j] = (unsigned long long)e < (unsigned long long)numel ? cf2bf(w[e])
                                                             : (bf16_t)0;
  }
  *reinterpret_cast<uint4*>(out + g * 8) = *reinterpret_cast<uint4*>(v);
}

static inline int conv_blocks(long long rows) {
  long long blocks = (rows + 3) / 4;  // 4 waves per block, 1 row per wave
  if (blocks < 1) blocks = 1;
  if (blocks > 32768) blocks = 32768;  // block turnover = extra latency TLP
  return (int)blocks;
}

// Launch table of k_conv5_lds_nhwc<32, 1, ...> (CI=32, CO=16): staging
// rows of 120 and 232 pixels, pad 0 / pad 4, and with `mask` the pooled
// (UNPOOL) form of pad 4. n_wg <= 0 picks the default grid: one
// workgroup per 4-row block up to 4 resident rounds of 2 (120) or 1
// (232) workgroups per CU on 256 CUs, so the weight fragments are
// fetched by few workgroups and the cross-block prefetch has blocks to
// run ahead of. Returns 0, or -1 when no variant serves the geometry.
static int conv5_lds_launch(const bf16_t* in, const uint8_t* mask,
                            const bf16_t* w_frags, const float* bias,
                            bf16_t* out, int Nn, int Hi, int Wi, int Ho,
                            int Wo, int pad, int n_wg, hipStream_t s) {
  const int need = conv5_stage_width(Wo, 16, Wi);
  if (need > 232 || (pad != 0 && pad != 4) || (mask && pad != 4)) return -1;
  const long long blocks = (long long)Nn * ((Ho + 3) / 4);
  if (n_wg <= 0) {
    const long long cap = need <= 120 ? 2048 : 1024;
    n_wg = (int)(blocks < cap ? blocks : cap);
  }
  if (n_wg < 1) n_wg = 1;
#define LDSLAUNCH(PIX_, PAD_, UNP_)                                        \
  if (pad == PAD_ && need <= PIX_ && (mask != nullptr) == UNP_) {          \
    hipLaunchKernelGGL((k_conv5_lds_nhwc<32, 1, PIX_, PAD_, UNP_>),        \
                       dim3(n_wg), dim3(CONV_THREADS), 0, s, in, w_frags,  \
                       bias, out, Nn, Hi, Wi, Ho, Wo, mask);               \
    return 0;                                                              \
  }
  LDSLAUNCH(120, 4, true) LDSLAUNCH(232, 4, true)
  LDSLAUNCH(120, 4, false) LDSLAUNCH(232, 4, false)
  LDSLAUNCH(120, 0, false) LDSLAUNCH(232, 0, false)
#undef LDSLAUNCH
  return -1;
}

// geometry the pooled (UNPOOL) dgrad form accepts
static bool conv5_unpool_geometry_ok(const uint8_t* mask, int Hi, int Wi,
                                     int Ho, int Wo, int CI, int CO) {
  if (CI != 32 || CO != 16 || !mask) return false;
  return Hi >= 10 && Wi >= 10 && Ho == Hi - 4 && Wo == Wi - 4 &&
         !((Hi | Wi) & 1);
}

// Launch table of the fused conv + bias + ReLU + max-pool forward:
// k_conv5_pool16_nhwc (CI=16, 120-pixel rows), k_conv5_pool2_nhwc (CI=4,
// even Wi, 232-pixel rows) and the register-only k_conv5_pool_nhwc<4>
// beyond. n_wg <= 0 picks the default grid. The LDS kernels work in
// blocks of 2 pooled rows. pool16 is capped at the 512 workgroups that
// are resident on 256 CUs (2 per CU, LDS-bound): each fetches its
// weights once and walks a run of blocks with the next block's staging
// in flight (the flagship's 13824 blocks are 27 per workgroup; 1024 and
// 2048 measured 1-4 % slower). pool2 (4 per CU) measured best at two
// resident rounds, 2048. Returns 0, or -1 when nothing serves the
// geometry.
static int conv5_pool_launch(const bf16_t* in, const bf16_t* w_frags,
                             const float* bias, bf16_t* out, uint8_t* mask,
                             int Nn, int Hi, int Wi, int Ho, int Wo, int CI,
                             int CO, int n_wg, hipStream_t s) {
  if ((CO != 16 && CO != 32) || (Ho & 1) || (Wo & 1)) return -1;
  const long long rows = (long long)Nn * (Ho >> 1);
  const long long blocks = (long long)Nn * (((Ho >> 1) + 1) >> 1);
  const dim3 block(CONV_THREADS);
  const int need = conv5_stage_width(Wo, 16, Wi);
  auto grid_of = [&](long long cap) {
    long long g = n_wg > 0 ? n_wg : (blocks < cap ? blocks : cap);
    return dim3((unsigned)(g < 1 ? 1 : g));
  };
  if (CI == 16) {
    if (CO == 32 && need <= 120) {
      hipLaunchKernelGGL((k_conv5_pool16_nhwc<2, 120>), grid_of(512), block,
                         0, s, in, w_frags, bias, out, mask, Nn, Hi, Wi,
                         Ho, Wo);
      return 0;
    }
    if (CO == 16 && need <= 120) {
      hipLaunchKernelGGL((k_conv5_pool16_nhwc<1, 120>), grid_of(512), block,
                         0, s, in, w_frags, bias, out, mask, Nn, Hi, Wi,
                         Ho, Wo);
      return 0;
    }
    return -1;
  }
  if (CI == 4 && !(Wi & 1) && need <= 232) {
    hipLaunchKernelGGL((k_conv5_pool2_nhwc<232>), grid_of(2048), block, 0, s,
                       in, w_frags, bias, out, mask, Nn, Hi, Wi, Ho, Wo);
    return 0;
  }
  if (CI == 4) {
    const dim3 grid(n_wg > 0 ? n_wg : conv_blocks(rows));
    hipLaunchKernelGGL((k_conv5_pool_nhwc<4>), grid, block, 0, s, in,
                       w_frags, bias, out, mask, Nn, Hi, Wi, Ho, Wo);
    return 0;
  }
  return -1;
}

extern "C" {

// Test hook: ALWAYS the direct kernel k_conv5_nhwc<32, 1> on a
// physically padded input (Hi = Ho + 4, Wi = Wo + 4). It issues the same
// MFMA sequence per output as the LDS dgrad kernel, which geops_conv5_nhwc
// prefers below 236-pixel rows. Returns 0, or -1 for other geometry.
int geops_conv5_direct_nhwc(const bf16_t* in, const bf16_t* w_frags,
                            const float* bias, bf16_t* out, int Nn, int Hi,
                            int Wi, int Ho, int Wo, int CI, int CO,
                            hipStream_t s) {
  if (CI != 32 || CO != 16 || Ho < 1 || Wo < 1 || Hi != Ho + 4 ||
      Wi != Wo + 4)
    return -1;
  const dim3 grid(conv_blocks((long long)Nn * Ho)), block(CONV_THREADS);
  hipLaunchKernelGGL((k_conv5_nhwc<32, 1>), grid, block, 0, s, in, w_frags,
                     bias, out, Nn, Hi, Wi, Ho, Wo);
  return 0;
}

// Test hook: the pad == 4 LDS dgrad (`mask` null: `in` is the full-
// resolution grad_out) or its pooled form (`mask` set: `in` is the
// pooled grad_out) on a grid of n_wg workgroups, so that small inputs
// reach the persistent loop. Same geometry table as the default calls.
int geops_conv5_dgrad_nwg_nhwc(const bf16_t* in, const uint8_t* mask,
                               const bf16_t* w_frags, bf16_t* out, int Nn,
                               int Hi, int Wi, int Ho, int Wo, int CI,
                               int CO, int n_wg, hipStream_t s) {
  if (CI != 32 || CO != 16 || n_wg < 1 || Ho != Hi - 4 || Wo != Wi - 4 ||
      Hi < 10 || Wi < 10)
    return -1;
  if (mask && !conv5_unpool_geometry_ok(mask, Hi, Wi, Ho, Wo, CI, CO))
    return -1;
  return conv5_lds_launch(in, mask, w_frags, nullptr, out, Nn, Hi, Wi, Ho,
                          Wo, 4, n_wg, s);
}

// returns 0 on success, -1 for unsupported geometry
int geops_conv5_nhwc(const bf16_t* in, const bf16_t* w_frags,
                     const float* bias, bf16_t* out, int Nn, int Hi, int Wi,
                     int Ho, int Wo, int CI, int CO, int pad,
                     hipStream_t s) {
  const long long rows = (long long)Nn * Ho;
  const dim3 grid(conv_blocks(rows)), block(CONV_THREADS);
  // pad == 0: `in` carries every pixel the taps touch (the data-grad
  // caller zero-pads grad_out physically). pad == 4: `in` is the
  // UNPADDED tensor, Hi/Wi still count the virtual 4-pixel border, and
  // the LDS kernel materialises it while staging -- CI=32, CO=16 only
  // (the conv2 data gradient). The LDS variants are compiled for 120-
  // and 232-pixel staging rows; wider pad-0 rows fall through to the
  // direct kernel, which has no width limit.
  if (CI == 32 && CO == 16 &&
      conv5_lds_launch(in, nullptr, w_frags, bias, out, Nn, Hi, Wi, Ho, Wo,
                       pad, 0, s) == 0)
    return 0;
  if (pad != 0) return -1;
#define LAUNCH(CI_, COT_)                                                 \
  if (CI == CI_ && CO == COT_ * 16) {                                     \
    hipLaunchKernelGGL((k_conv5_nhwc<CI_, COT_>), grid, block, 0, s, in,  \
                       w_frags, bias, out, Nn, Hi, Wi, Ho, Wo);           \
    return 0;                                                             \
  }
  LAUNCH(4, 1) LAUNCH(16, 2) LAUNCH(16, 1) LAUNCH(32, 1) LAUNCH(32, 2)
#undef LAUNCH
  return -1;
}

// conv2 data gradient straight from the POOLED grad_out + argmax mask:
// the pad == 4 LDS route of geops_conv5_nhwc (CI=32, CO=16, same width
// table) with the max-pool backward done while staging. Hi/Wi count the
// full-resolution grad_out plus the virtual 4-pixel border, Ho/Wo are
// the output; gp/mask are [N][(Hi-8)/2][(Wi-8)/2][32]. Returns 0, or -1
// for unsupported geometry (odd full-resolution sizes included).
int geops_conv5_dgrad_unpool_nhwc(const bf16_t* gp, const uint8_t* mask,
                                  const bf16_t* w_frags, bf16_t* out,
                                  int Nn, int Hi, int Wi, int Ho, int Wo,
                                  int CI, int CO, hipStream_t s) {
  if (!conv5_unpool_geometry_ok(mask, Hi, Wi, Ho, Wo, CI, CO)) return -1;
  return conv5_lds_launch(gp, mask, w_frags, nullptr, out, Nn, Hi, Wi, Ho,
                          Wo, 4, 0, s);
}

int geops_conv5_pool_nhwc(const bf16_t* in, const bf16_t* w_frags,
                          const float* bias, bf16_t* out, uint8_t* mask,
                          int Nn, int Hi, int Wi, int Ho, int Wo, int CI,
                          int CO, hipStream_t s) {
  return conv5_pool_launch(in, w_frags, bias, out, mask, Nn, Hi, Wi, Ho, Wo,
                           CI, CO, 0, s);
}

// Test hook: the launch table of geops_conv5_pool_nhwc on a grid of n_wg
// workgroups, so that small inputs reach the persistent loop, the
// cross-block prefetch and the one-pooled-row tail block.
int geops_conv5_pool_nwg_nhwc(const bf16_t* in, const bf16_t* w_frags,
                              const float* bias, bf16_t* out, uint8_t* mask,
                              int Nn, int Hi, int Wi, int Ho, int Wo, int CI,
                              int CO, int n_wg, hipStream_t s) {
  if (n_wg < 1) return -1;
  return conv5_pool_launch(in, w_frags, bias, out, mask, Nn, Hi, Wi, Ho, Wo,
                           CI, CO, n_wg, s);
}

// n0, n1: element counts of the two tables, multiples of 8; n1 == 0 (and
// null idx1/out1) packs one table.
int geops_conv5_pack_frags(const float* w, long long numel,
                           const long long* idx0, bf16_t* out0, long long n0,
                           const long long* idx1, bf16_t* out1, long long n1,
                           hipStream_t s) {
  if (n0 <= 0 || n1 < 0 || (n0 & 7) || (n1 & 7)) return -1;
  const long long blocks = ((n0 + n1) / 8 + 255) / 256;
  if (blocks > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(k_conv5_pack_frags, dim3((int)blocks), dim3(256), 0, s,
                     w, numel, idx0, out0, n0, idx1, out1, n1);
  return 0;
}

void geops_pad_ch3to4_nhwc(const void* in, bf16_t* out, long long npix,
                           int in_is_fp32, hipStream_t s) {
  long long blocks = (npix + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (in_is_fp32)
    hipLaunchKernelGGL((k_pad_ch3to4_nhwc<float>), dim3((int)blocks),
                       dim3(256), 0, s, (const float*)in, out, npix);
  else
    hipLaunchKernelGGL((k_pad_ch3to4_nhwc<bf16_t>), dim3((int)blocks),
                       dim3(256), 0, s, (const bf16_t*)in, out, npix);
}

}  // extern "C"
