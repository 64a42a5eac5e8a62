// Weight-gradient (wrw) v2 for 5x5 stride-1 NHWC conv, CI=16, on gfx950.
//
// dW[kh,kw,ci][o] = sum_{n,ho,wo} in[n,ho+kh,wo+kw,ci] * gout[n,ho,wo,o]
//
// v1 (removed; see git history) staged TRANSPOSED images with
// per-element ds writes and gathered the shifted A fragment with an
// alignbyte funnel; it was LDS-gather bound (1.10 ms standalone on the
// conv2 shape vs MIOpen's 1.60 in-step). v2 removes both costs:
//
//   * LDS images keep the NATURAL pixel-major layout ([pix][ci] for the
//     input — identical to global NHWC — and per-o-tile [pix][16] for
//     gout), so staging is pure LDS-DMA (__builtin_amdgcn_global_load_lds,
//     16 B/lane): zero VALU work, zero ds_write instructions. Lanes whose
//     pixel falls in the zero-padding read a device zero page, so padding
//     is zero-filled in the same pass. The UNPOOL variants (backward of
//     a fused conv+pool stage) instead build the gout image from the
//     POOLED gradient and the argmax mask: one 16 B + 8 B load per
//     8 channels of a pooled pixel, four select + ds_write_b128 — the
//     full-resolution gradient never exists in HBM.
//   * MFMA fragments come from ds_read_b64_tr_b16 (gfx950's LDS
//     transpose read, cdna_hip_programming.md T10): each 16-lane group
//     reads one 4(pix)x16(chan) row-major tile — lane g supplies
//     tile_base + g*8 (8B-aligned) and receives CHANNEL COLUMN g across
//     the 4 pixels. Both A and B fragments use the SAME k-slot->pixel
//     permutation (slot q*8+j <-> pixel 4q+j / 16+4q+j), so the MFMA
//     contraction pairs matched pixels. The kw shift of A is a whole-
//     pixel base offset — no misaligned gathers, no funnel shifts.
//
// Work layout: grid-persistent workgroups own row-blocks of WRW2_R gout
// rows; 4 waves split the 25 (kh,kw) tap tiles round-robin and each
// wave computes BOTH o-tiles for its taps (A-fragment reuse), keeping
// all accumulators in VGPRs until one final per-workgroup slab flush
// (partials summed in torch). Fragment reads are compiler-counted
// builtins issued a few tap tiles ahead of their MFMAs, across (row,
// window) steps; the bias tile reads a constant LDS image of ones; the
// pooled form fetches the next block's gradient and codes during the
// MFMA phase; the launcher picks a straight-line walk (STRAIGHT) where
// every block is full-width and two rows high. Every slab row is
// written, so the caller need not clear the slabs. The CI=4 kernel
// (conv1) packs its taps differently and double-buffers its A image; it
// is described at k_conv5_wrw4_nhwc below.

#include <hip/hip_runtime.h>

#include "conv5_common.h"

#define WRW2_THREADS 256  // 4 waves
#define WRW2_R 2          // gout rows per block

// ds_read_b64_tr_b16: the 16-lane group covers one 4x16 bf16 row-major
// tile (lane g supplies tile_base + g*8); lane g receives column g
// (4 bf16, one per tile row). As a builtin its result lands in MFMA
// operand registers without a repack and the compiler counts its lgkmcnt
// wait, so reads can stay in flight across MFMAs (both wrw kernels
// pipeline them this way). `p` is this lane's LDS address.
__device__ __forceinline__ bf16x4 tr16_ld(
    const __attribute__((address_space(3))) char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

// STRAIGHT: every block is a full-width two-row block (Wo > 32 * (WMAX -
// 1), Ho even), the launcher's choice; the walk is then straight-line
// code. A kernel holds ONE form of the walk: with both behind a branch
// the accumulators get two register sets and copies between them.
template <int COT, int PIX, bool UNPOOL = false, bool STRAIGHT = false>
__global__ __launch_bounds__(WRW2_THREADS) void k_conv5_wrw16_nhwc(
    const bf16_t* __restrict__ in,    // [N][Hi][Wi][16]
    const bf16_t* __restrict__ gout,  // [N][Ho][Wo][CO]; UNPOOL: the
                                      // pooled [N][Ho/2][Wo/2][CO]
    float* __restrict__ part,         // [nWG][T16][CO]
    int Nn, int Hi, int Wi, int Ho, int Wo,
    const uint8_t* __restrict__ mask) {  // UNPOOL: argmax codes, as gout
  constexpr int CI = 16;
  constexpr int CO = COT * 16;
  constexpr int NT = 25;                 // tap tiles = (kh,kw) pairs
  // +1 slab tile: the spare (wid 1, j 6) slot computes the BIAS grad
  // with an all-ones A row (D[0][o] = sum_k B[k][o] accumulated over
  // every pixel window) — kills the separate at::native bias reduce
  constexpr int T16 = (NT + 1) * 16;
  // row region: one 16-wide subimage row (input row, or one o-tile of a
  // gout row), unskewed
  using Rows = RowImage<PIX, CI, false>;
  constexpr int NCH = Rows::NCH;                       // glds chunks/row
  constexpr int RPB = Rows::PITCH;                     // region bytes
  constexpr int NROW_IN = WRW2_R + 4;
  constexpr int NROW_GO = WRW2_R * COT;
  // a gout row holds the WMAX * 32 pixels the K windows read, so the
  // last 1 KiB of its region is free; that of the last region holds the
  // bias tile's A image, 4 pixel rows of [1.0, 0 x 15] at +0 (k-pixels
  // 0..15) and at +512 (k-pixels 16..31)
  constexpr int WMAX = Rows::WMAX;       // K windows of a full row
  constexpr int ONES = (NROW_IN + NROW_GO) * RPB - 1024;
  constexpr int ONES_BYTES = 512 + 128;
  static_assert(WMAX * 1024 + 1024 <= RPB, "room for the ones image");
  __shared__ __attribute__((aligned(128))) char lds_all[(NROW_IN + NROW_GO) *
                                                        RPB];

  typedef const __attribute__((address_space(3))) char* lds_cptr;

  const int lane = threadIdx.x & 63;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int W = (Wo + 31) >> 5;          // 32-pixel K windows per row
  const int blocks_h = (Ho + WRW2_R - 1) / WRW2_R;
  const long long n_blocks = (long long)Nn * blocks_h;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;

  const lds_cptr lds3 = (lds_cptr)lds_all;

  // wave-owned tap tiles: tt = wid + 4*j, accumulators for BOTH o-tiles.
  // Wave 0 owns 7 taps, waves 1..3 own 6. Slot j = 6 of wave 1 (tt = 25)
  // is the bias tile: its A fragment, row 0 all ones and rows 1..15 zero
  // (D[0][o] = sum_k B[k][o]), is read from the ONES image like any tap,
  // at a fixed address. Waves 2 and 3 run the same slot into accumulators
  // that are never flushed: with the slot behind a wave-dependent branch
  // the compiler splits the accumulators over two register sets (112
  // AGPRs, copies in the walk, 2 workgroups per CU).
  constexpr int MAXT = (NT + 3) / 4;     // 7
  f32x4 acc[MAXT][COT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j)
#pragma unroll
    for (int t = 0; t < COT; ++t) acc[j][t] = (f32x4)0.0f;

  // per-lane fragment bases at (gout row 0, window 0): step (r, w) is a
  // constant offset from them, except for slot 6 of waves 1..3, which
  // stays on the ONES image (step6 = 0)
  lds_cptr ab[MAXT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    const int tt = wid + 4 * j;
    const int kh = tt / 5;
    const int kw = tt - kh * 5;
    ab[j] = tt < NT ? lds3 + kh * RPB + (kw + 4 * q) * 32 + m * 8
                    : lds3 + ONES + m * 8;
  }
  const int step6 = wid == 0 ? 1 : 0;
  const lds_cptr bb = lds3 + NROW_IN * RPB + (4 * q) * 32 + m * 8;
  if (threadIdx.x < ONES_BYTES / 16)     // visible after the first barrier
    reinterpret_cast<uint4*>(lds_all + ONES)[threadIdx.x] =
        make_uint4((threadIdx.x & 1) ? 0u : 0x3F80u, 0u, 0u, 0u);

  // ---- staging pieces, chunks round-robin over the 4 waves.
  // A rows by LDS-DMA: a global NHWC row IS the LDS [pix][16] row.
  auto stage_a = [&](long long n, int bh) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;
    stage_rows<CI, NCH, RPB, false>(in, n, Hi, Wi, ho0, (nrows + 4) * NCH,
                                    wid, lane, lds_all, 0);
  };
  // gout rows (full-resolution form): global [pix][CO] -> per-o-tile LDS
  // [pix][16], by LDS-DMA
  auto stage_b = [&](long long n, int bh) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;
    const int nchunks_b = nrows * COT * WMAX;
    for (int t = wid; t < nchunks_b; t += 4) {
      const int rr = t / (COT * WMAX);
      const int rem = t - rr * (COT * WMAX);
      const int ot = rem / WMAX;
      const int c = rem - ot * WMAX;
      const int slot = c * 64 + lane;
      const int pix = slot >> 1;
      const int half = slot & 1;
      const bf16_t* src =
          (pix < Wo)
              ? gout + ((n * Ho + (ho0 + rr)) * (long long)Wo * CO +
                        (long long)pix * CO + ot * 16 + half * 8)
              : conv5_zeros();
      glds16(src, lds_all + (NROW_IN + rr * COT + ot) * RPB + c * 1024);
    }
  };
  // UNPOOL: gout rows from pooled row bh and its argmax codes
  // (pooled_load / pooled_write of conv5_common.h; the selects and
  // ds_writes run after the MFMA phase the loads fly through)
  constexpr int GV = CO / 8;
  constexpr int NIT = (16 * WMAX * GV + WRW2_THREADS - 1) / WRW2_THREADS;
  uint4 gq[NIT];
  uint2 mq[NIT];
  auto load_pooled = [&](long long n, int bh) {
    pooled_load<NIT, WRW2_THREADS, GV>(gout, mask, n, bh, Ho, Wo, gq, mq);
  };
  auto write_pooled = [&]() {
    pooled_write<NIT, WRW2_THREADS, COT, 0, NROW_IN, RPB>(lds_all, W, gq, mq);
  };

  // ---- the (row, window) walk of one block. Fragment reads are
  // compiler-counted builtins, issued DEPTH tap tiles ahead of the MFMAs
  // that use them, across step boundaries: tile j of a step lives in
  // afr[j], which is free for the next step's tile j once this step's
  // MFMA j is issued. The window's B fragments are held in `bcur` for
  // the whole step; the next step's arrive in `bnxt` ahead of its first
  // tile. The walk has no wave-dependent branch (slot 6 differs between
  // the waves by its address alone), so it is straight-line code.
  // Every accumulator still receives its MFMAs in (row, window) order;
  // only the interleaving of different accumulators with the reads
  // changed. The sched_barriers pin that program order; the compiler
  // places the counted lgkmcnt waits.
  constexpr int DEPTH = 3;
  static_assert(DEPTH < MAXT, "a slot is refilled after its MFMA");
  bf16x4 afr[MAXT][2];
  bf16x4 bcur[COT][2], bnxt[COT][2];
  auto ld_a = [&](int j, int oa) __attribute__((always_inline)) {
    const lds_cptr p = j < MAXT - 1 ? ab[j] + oa : ab[j] + oa * step6;
    afr[j][0] = tr16_ld(p);
    afr[j][1] = tr16_ld(p + 512);            // k-pixels 16..31
  };
  auto ld_b = [&](bf16x4 (&b)[COT][2], int ob) __attribute__((always_inline)) {
#pragma unroll
    for (int ot = 0; ot < COT; ++ot) {
      b[ot][0] = tr16_ld(bb + ob + ot * RPB);
      b[ot][1] = tr16_ld(bb + ob + ot * RPB + 512);
    }
  };
  auto mma = [&](int j) __attribute__((always_inline)) {
    const bf16x8 a = join_bf16x4(afr[j][0], afr[j][1]);
#pragma unroll
    for (int ot = 0; ot < COT; ++ot)
      acc[j][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a, join_bf16x4(bcur[ot][0], bcur[ot][1]), acc[j][ot], 0, 0, 0);
  };
  // one step at offsets (oa, ob); (oa_n, ob_n) is the step after it
  auto step = [&](int oa, int ob, int oa_n, int ob_n, bool has_next)
                  __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      const int jn = j + DEPTH;
      if (jn < MAXT) {
        ld_a(jn, oa);
      } else if (has_next) {
        if (jn == MAXT) ld_b(bnxt, ob_n);
        ld_a(jn - MAXT, oa_n);
      }
      __builtin_amdgcn_sched_barrier(0);
      mma(j);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (has_next) {
#pragma unroll
      for (int ot = 0; ot < COT; ++ot) {
        bcur[ot][0] = bnxt[ot][0];
        bcur[ot][1] = bnxt[ot][1];
      }
    }
  };
  // (row r, window w) -> byte offsets in the A and the gout image
  auto off_a = [&](int r, int w) { return r * RPB + w * 1024; };
  auto off_b = [&](int r, int w) { return r * COT * RPB + w * 1024; };
  auto walk = [&](int nrows) __attribute__((always_inline)) {
    ld_b(bcur, 0);
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) ld_a(j, 0);
    if constexpr (STRAIGHT) {
      // full-width two-row blocks (the flagship): every offset is an
      // immediate, the walk is straight-line code
      constexpr int NS = WRW2_R * WMAX;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int s1 = s + 1 < NS ? s + 1 : s;
        step(off_a(s / WMAX, s % WMAX), off_b(s / WMAX, s % WMAX),
             off_a(s1 / WMAX, s1 % WMAX), off_b(s1 / WMAX, s1 % WMAX),
             s + 1 < NS);
      }
    } else {
      // any other width, and one-row tail blocks: the same pipeline in a
      // loop. The step after the last re-reads the last one (in bounds,
      // unused), so a trip has no branch of its own.
      const int nsteps = nrows * W;
      int r = 0, w = 0;
      for (int s = 0; s < nsteps; ++s) {
        int rn = r, wn = w;
        if (s + 1 < nsteps) {
          wn = w + 1;
          if (wn == W) { wn = 0; rn = r + 1; }
        }
        step(off_a(r, w), off_b(r, w), off_a(rn, wn), off_b(rn, wn), true);
        r = rn;
        w = wn;
      }
    }
  };

  // block = (image n, row pair bh), decoded once, one block ahead
  long long blk = wg;
  long long n = 0;
  int bh = 0;
  if (blk < n_blocks) {
    n = blk / blocks_h;
    bh = (int)(blk - n * blocks_h);
    if constexpr (UNPOOL) load_pooled(n, bh);
  }
  for (; blk < n_blocks; blk += n_wg) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;

    // ---- stage this block's images
    stage_a(n, bh);
    if constexpr (UNPOOL) {
      write_pooled();
    } else {
      stage_b(n, bh);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the LDS-DMA pieces
    __syncthreads();

    // ---- the next block's pooled gradient and codes fly during this
    // block's MFMA phase
    if (blk + n_wg < n_blocks) {
      n = (blk + n_wg) / blocks_h;
      bh = (int)(blk + n_wg - n * blocks_h);
      if constexpr (UNPOOL) load_pooled(n, bh);
    }

    walk(nrows);
    __syncthreads();  // before the next block restages LDS
  }

  // ---- flush accumulators: part[wg][tap][o]
  // C/D layout of mfma_f32_16x16x32_bf16: lane (q,m), reg i ->
  // row = q*4 + i (the A row = tap-within-tile), col = m (the B col = o)
  float* base = part + (long long)wg * T16 * CO;
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    const int tt = wid + 4 * j;
    if (tt > NT) continue;               // NT itself = the bias tile
#pragma unroll
    for (int ot = 0; ot < COT; ++ot) {
      const int o = ot * 16 + m;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tap = tt * 16 + q * 4 + i;
        base[(long long)tap * CO + o] = acc[j][ot][i];
      }
    }
  }
}

// ---------------------------------------------------------------------
// probe: verify the tr16 lane mapping numerically (test_kernels_gpu).
// in : 64 bf16 = one 4x16 row-major tile. out[lane][j] = element j of
// lane `lane`'s tr read — expected out[l][j] == tile[j][l&15] for the
// first 16-lane group (all groups read the same tile here).
// ---------------------------------------------------------------------
__global__ void k_tr16_probe(const bf16_t* __restrict__ in,
                             bf16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(128))) bf16_t tile[64];
  const int lane = threadIdx.x & 63;
  tile[lane] = in[lane];
  __syncthreads();
  const unsigned a = lds_addr(tile) + (lane & 15) * 8;
  bf16x4 d;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(d) : "v"(a) : "memory");
#pragma unroll
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = d[j];
}

// ---------------------------------------------------------------------
// CI=4 variant (conv1: 4 padded channels -> 16 outputs).
//
// With 4 channels an image row is 8 B per pixel, so one tr-read quarter
// (4 bf16) is one pixel's channels. The transpose read gathers PER-LANE
// 8 B quarters (test_tr16_per_lane_gather: out[m][j] = mem[addr[4j +
// (m>>2)] + (m&3) elems]), so a fragment's A row m = 4p + ci comes from
// whatever (row, pixel) lane quarter p of the group points at, straight
// from the raw [pix][4] input rows. The 100 taps and the bias sit in
// SEVEN tiles (112 A rows, 101 live):
//   T0..T4 (kw = T): quarter p -> row r+p, pixel kw + 4q + j
//                    A row m = (kh = m>>2, ci = m&3)
//   T5 (kh = 4):     quarter p -> row r+4, pixel p + 4q + j
//                    A row m = (kw = m>>2, ci = m&3), kw = 0..3
//   T6:              quarters 0, 2, 3 -> row r+4, pixel 4 + 4q + j
//                    A rows 0..3 = (kh 4, kw 4, ci); quarter 1 points
//                    into an LDS region of bf16 ones, so A row 4 is the
//                    BIAS row (D[4][o] = sum_k B[k][o]) without a select
//                    in the loop; rows 5..15 are dead
// (j = (lane&15)>>2 is the k-pixel, p = lane&3; the read needs EXEC all
// ones, so dead quarters get an in-bounds address and are dropped at the
// flush). Row regions are skewed by 64 B so the 4 rows a T0..T4 group
// touches land on distinct LDS banks; T5/T6 touch 11 consecutive pixels
// of one row per 32-lane half. Waves own tiles {0,1} {2,3} {4,5} {6}:
// 24 tr reads and 8 MFMAs per (row, window), one of each pair spare
// (the 10-tile kernel: 32 and 11). One tile per wave on 8 waves measured
// slower (docs/kernels.md).
//
// A D row depends on its own A row only, and every tile keeps the
// k-slot -> pixel permutation and the (block, row, window) order of its
// MFMAs, so each (tap, o) and bias sum is the sum the 10-tile kernel
// (tiles t = kw*2 + kh/4, before) computed, bit for bit; the flush
// scatters the live rows to that kernel's slab rows
// (kw*2 + kh/4)*16 + (kh%4)*4 + ci, bias in row 160, and writes zeros
// to the other rows.
//
// Schedule: fragment reads are compiler-counted builtins
// (__builtin_amdgcn_ds_read_tr16_b64_v4i16), software-pipelined two
// (row, window) steps ahead in three register sets, so a wave's reads
// are in flight while its MFMAs run and no lgkmcnt(0) drain sits in the
// walk (the builtin's result needs no repack ahead of a hand-placed
// wait, which is what tied the 10-tile kernel to one asm block per
// step). A full-width two-row block walks straight-line code whose
// offsets are all immediates; other widths and one-row tails take a
// loop with the same pipeline.
// The A image is double-buffered: the next block's rows go by LDS-DMA
// into the other image, and (UNPOOL) its pooled gradient and codes into
// registers, right after the barrier that opens the MFMA phase; the
// selects and ds_write_b128 that build the gout image run after the
// barrier that ends it. The full-resolution form stages gout by LDS-DMA
// into its single image between the two barriers.
// ---------------------------------------------------------------------
template <int PIX, bool UNPOOL = false>
__global__ __launch_bounds__(WRW2_THREADS) void k_conv5_wrw4_nhwc(
    const bf16_t* __restrict__ in,    // [N][Hi][Wi][4]
    const bf16_t* __restrict__ gout,  // [N][Ho][Wo][16]; UNPOOL: the
                                      // pooled [N][Ho/2][Wo/2][16]
    float* __restrict__ part,         // [nWG][176][16]
    int Nn, int Hi, int Wi, int Ho, int Wo,
    const uint8_t* __restrict__ mask) {  // UNPOOL: argmax codes, as gout
  constexpr int CI = 4;
  constexpr int CO = 16;
  constexpr int NT = 7;                   // packed tap tiles, bias in T6
  constexpr int T16 = 176;                // slab rows (10 + 1 tiles)
  using RowsA = RowImage<PIX, CI, true>;  // 64B skew: distinct banks/row
  using RowsB = RowImage<PIX, CO, false>;
  constexpr int NCHA = RowsA::NCH;
  constexpr int ARPB = RowsA::PITCH;
  constexpr int NCHB = RowsB::NCH;
  constexpr int BRPB = RowsB::PITCH;
  constexpr int NROW_A = WRW2_R + 4;      // rows ho0 .. ho0+5
  constexpr int AIMG = NROW_A * ARPB;     // one A image; two of them
  constexpr int BOFF = 2 * AIMG;
  constexpr int WMAX = RowsA::WMAX;       // K windows of a full row
  constexpr int ONES = BOFF + WRW2_R * BRPB;  // bf16 1.0, see ones_q
  constexpr int ONES_BYTES = WRW2_THREADS * 16;
  static_assert(AIMG % 128 == 0, "");
  static_assert(ARPB + (WMAX - 1) * 256 + 128 + 8 <= ONES_BYTES,
                "the bias quarter walks the same offsets as a pixel row");
  __shared__ __attribute__((aligned(128))) char lds_all[ONES + ONES_BYTES];

  const int lane = threadIdx.x & 63;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int W = (Wo + 31) >> 5;
  const int blocks_h = (Ho + WRW2_R - 1) / WRW2_R;
  const long long n_blocks = (long long)Nn * blocks_h;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const __attribute__((address_space(3))) char* lds3 =
      (const __attribute__((address_space(3))) char*)lds_all;
  const unsigned lds0 = lds_addr(lds_all);

  // wave-owned tiles t = 2*wid + j. The spare slot (wid 3, j 1) repeats
  // T6 into an accumulator that is never flushed: the walk then has no
  // wave-dependent branch, so the compiler can count its lgkmcnt waits.
  constexpr int TPW = 2;
  f32x4 acc[TPW];
  // per-lane fragment bases at (r 0, window 0) of A image 0
  const __attribute__((address_space(3))) char* abase[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    acc[j] = (f32x4)0.0f;
    const int t = (2 * wid + j) < NT ? 2 * wid + j : NT - 1;
    const int p = lane & 3;
    const int kpix = 4 * q + (m >> 2);
    const int row = t < 5 ? p : 4;
    const int pix = (t < 5 ? t : (t == 5 ? p : 4)) + kpix;
    abase[j] = lds3 + row * ARPB + pix * 8;
  }
  // T6's quarter 1 (A rows 4..7; row 4 is the bias row) reads constant
  // bf16 ones instead of pixels: its lanes walk the ONES region, filled
  // once here and made visible by the first block's barrier, with the
  // offsets the other quarters walk a pixel row with. Rows 5..7 are dead.
  const bool ones_q = (wid == 3) && ((lane & 3) == 1);
  const __attribute__((address_space(3))) char* ones_p = lds3 + ONES;
  reinterpret_cast<uint4*>(lds_all + ONES)[threadIdx.x] =
      make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
  const __attribute__((address_space(3))) char* bbase =
      lds3 + BOFF + (4 * q) * 32 + m * 8;

  // ---- staging pieces. A rows by LDS-DMA (16 B = 2 pixels per lane),
  // chunks round-robin over the 4 waves; only the nrows + 4 rows the
  // block's taps read are fetched.
  auto stage_a = [&](long long n, int bh, int img) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;
    stage_rows<CI, NCHA, ARPB, true>(in, n, Hi, Wi, ho0, (nrows + 4) * NCHA,
                                     wid, lane, lds0, img * AIMG);
  };
  // UNPOOL: both gout rows of a block come from pooled row bh and its
  // argmax codes (pooled_write, GV = 2). At most one item per thread:
  // 16 * 7 windows * 2 granules = 224. The load stays here: it is
  // pooled_load<1, .., 2> without the per-block reset of items past the
  // row, and with the reset the kernel's registers change (96 -> 92
  // VGPRs, 83 -> 87 SGPRs), so it would no longer be the measured kernel.
  static_assert(16 * WMAX * 2 <= WRW2_THREADS, "");
  uint4 gq[1] = {make_uint4(0u, 0u, 0u, 0u)};
  uint2 mq[1] = {make_uint2(~0u, ~0u)};
  auto load_pooled = [&](long long n, int bh) {
    const long long rowv = (n * (Ho >> 1) + bh) * (long long)(Wo >> 1) * 2;
    if ((int)threadIdx.x < (Wo >> 1) * 2) {
      gq[0] = reinterpret_cast<const uint4*>(gout)[rowv + threadIdx.x];
      mq[0] = reinterpret_cast<const uint2*>(mask)[rowv + threadIdx.x];
    }
  };
  auto write_pooled = [&]() {
    pooled_write<1, WRW2_THREADS, 1, BOFF, 0, BRPB>(lds_all, W, gq, mq);
  };
  auto stage_b = [&](long long n, int bh) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;
    const int nchunks_b = nrows * NCHB;
    for (int t = wid; t < nchunks_b; t += 4) {
      const int rr = t / NCHB;
      const int c = t - rr * NCHB;
      const int slot = c * 64 + lane;
      const int pix = slot >> 1;
      const bf16_t* src =
          (pix < Wo) ? gout + ((n * Ho + (ho0 + rr)) * (long long)Wo * CO +
                               (long long)slot * 8)
                     : conv5_zeros();
      glds16_unseen(src, lds0 + BOFF + rr * BRPB + c * 1024);
    }
  };

  // one (row, window) step's fragments: B lo/hi and per tile A lo/hi
  // (hi = k-pixels 16..31: +512 B in the gout image, +128 B in a row)
  struct Frag {
    bf16x4 b[2];
    bf16x4 a[TPW][2];
  };

  // block = (image n, row pair bh), decoded once, one block ahead
  long long blk = wg;
  int img = 0;
  long long n = 0;
  int bh = 0;
  if (blk < n_blocks) {
    n = blk / blocks_h;
    bh = (int)(blk - n * blocks_h);
    stage_a(n, bh, 0);
    if constexpr (UNPOOL) load_pooled(n, bh);
  }
  for (; blk < n_blocks; blk += n_wg, img ^= 1) {
    const int ho0 = bh * WRW2_R;
    const int nrows = (Ho - ho0) < WRW2_R ? (Ho - ho0) : WRW2_R;

    // ---- the gout image of this block (the A image was prefetched)
    if constexpr (UNPOOL) {
      write_pooled();
    } else {
      stage_b(n, bh);
    }
    // vmcnt(0), as a builtin so that the compiler's own bookkeeping of
    // the pooled loads sees it (an asm wait would leave it re-waiting,
    // on the DMA pieces just issued, before the next load_pooled)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

    // ---- the next block's fetches fly during this block's MFMA phase
    if (blk + n_wg < n_blocks) {
      n = (blk + n_wg) / blocks_h;
      bh = (int)(blk + n_wg - n * blocks_h);
      stage_a(n, bh, img ^ 1);
      if constexpr (UNPOOL) load_pooled(n, bh);
    }

    // ---- walk the (row, window) steps s = r*W + w in order, fragment
    // reads two steps ahead of their MFMAs in three register sets.
    // Step (r, w) is a constant offset from the block's per-lane bases.
    const __attribute__((address_space(3))) char* ab0 =
        ones_q ? ones_p : abase[0] + img * AIMG;   // T6 is (wid 3, j 0)
    const __attribute__((address_space(3))) char* ab1 =
        abase[1] + img * AIMG;
    auto load = [&](Frag& f, int r, int w) {
      const int oa = r * ARPB + w * (32 * 8);
      const int ob = r * BRPB + w * (32 * 32);
      f.b[0] = tr16_ld(bbase + ob);
      f.b[1] = tr16_ld(bbase + ob + 512);
      f.a[0][0] = tr16_ld(ab0 + oa);
      f.a[0][1] = tr16_ld(ab0 + oa + 128);
      f.a[1][0] = tr16_ld(ab1 + oa);
      f.a[1][1] = tr16_ld(ab1 + oa + 128);
    };
    auto mma = [&](const Frag& f) {
      const bf16x8 b = join_bf16x4(f.b[0], f.b[1]);
#pragma unroll
      for (int j = 0; j < TPW; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            join_bf16x4(f.a[j][0], f.a[j][1]), b, acc[j], 0, 0, 0);
    };
    // The sched_barriers keep each step's reads ahead of the MFMAs they
    // overlap; the compiler places the counted lgkmcnt waits.
    Frag f[3];
    if (W == WMAX && nrows == WRW2_R) {
      // full-width two-row block (the flagship): every offset is an
      // immediate, the walk is straight-line code
      constexpr int NS = WRW2_R * WMAX;
      load(f[0], 0, 0);
      load(f[1], 1 / WMAX, 1 % WMAX);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s + 2 < NS) load(f[(s + 2) % 3], (s + 2) / WMAX, (s + 2) % WMAX);
        __builtin_amdgcn_sched_barrier(0);
        mma(f[s % 3]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // any other width, and one-row tail blocks. A step past the last
      // re-reads the last one (in bounds, unused); no branch in a trip.
      const int nsteps = nrows * W;
      static_assert(WRW2_R == 2, "ld() decodes r from one compare");
      auto ld = [&](Frag& fr, int s) {
        if (s > nsteps - 1) s = nsteps - 1;
        const int r = s >= W ? 1 : 0;
        load(fr, r, s - (r ? W : 0));
      };
      ld(f[0], 0);
      ld(f[1], 1);
      int s = 0;
      for (; s + 2 < nsteps; s += 3) {
        ld(f[2], s + 2);
        __builtin_amdgcn_sched_barrier(0);
        mma(f[0]);
        __builtin_amdgcn_sched_barrier(0);
        ld(f[0], s + 3);
        __builtin_amdgcn_sched_barrier(0);
        mma(f[1]);
        __builtin_amdgcn_sched_barrier(0);
        ld(f[1], s + 4);
        __builtin_amdgcn_sched_barrier(0);
        mma(f[2]);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the last nsteps % 3 steps; their reads are already in flight
      if (s < nsteps) mma(f[0]);
      if (s + 1 < nsteps) mma(f[1]);
    }
    __syncthreads();  // before the next block rebuilds the gout image
  }

  // ---- flush the live D rows (row = q*4 + i, col = m = o) to the slab
  // rows of the 10-tile layout; the dead rows get zeros below, so the
  // caller need not clear the slab
  float* base = part + (long long)wg * T16 * CO;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int t = 2 * wid + j;
    if (t >= NT) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int slot;
      if (t < 5)                          // kw = t, kh = q, ci = i
        slot = t * 32 + q * 4 + i;
      else if (t == 5)                    // kh = 4, kw = q, ci = i
        slot = (q * 2 + 1) * 16 + i;
      else                                // kh 4, kw 4 | bias | dead
        slot = q == 0 ? 9 * 16 + i : ((q == 1 && i == 0) ? 160 : -1);
      if (slot >= 0) base[(long long)slot * CO + m] = acc[j][i];
    }
  }
  // the dead rows: 4..15 of the five kh = 4 tiles (12 rows = 48 float4
  // each) and the 15 rows behind the bias row (60 float4)
  static_assert(WRW2_THREADS >= 5 * 48, "");
  {
    const int t = threadIdx.x;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < 5 * 48) {
      const int kw = t / 48;
      const int off = t - kw * 48;
      reinterpret_cast<float4*>(base + ((2 * kw + 1) * 16 + 4) * CO)[off] = z;
    }
    if (t < 15 * CO / 4)
      reinterpret_cast<float4*>(base + 161 * CO)[t] = z;
  }
}

// probe 2: SCATTERED per-lane addresses. If the transpose read gathers
// each lane's own 8B quarter (out[g][j] = mem[addr[4j+(g>>2)] + 2*(g&3)])
// the wrw4 staging can drop its interleaved-image duplication. in: 512
// bf16 of content; addr_off[l] (elements) programs lane l's address.
__global__ void k_tr16_probe2(const bf16_t* __restrict__ in,
                              const int* __restrict__ addr_off,
                              bf16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(128))) bf16_t buf[512];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 512; i += blockDim.x) buf[i] = in[i];
  __syncthreads();
  const unsigned a = lds_addr(buf) + (unsigned)addr_off[lane] * 2;
  bf16x4 d;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(d) : "v"(a) : "memory");
#pragma unroll
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = d[j];
}

extern "C" {

// Launch tables. `mask` == nullptr: gout is the full-resolution
// gradient. Otherwise gout is the POOLED gradient [N][Ho/2][Wo/2][CO]
// and mask its argmax codes; the kernels unpool while staging (Ho, Wo
// are still the full-resolution sizes and must be even).
static int wrw16_launch(const bf16_t* in, const bf16_t* gout,
                        const uint8_t* mask, float* part, int Nn, int Hi,
                        int Wi, int Ho, int Wo, int CI, int CO, int n_wg,
                        hipStream_t s) {
  if (CI != 16) return -1;
  if (mask && ((Ho | Wo) & 1)) return -1;
  const int W = (Wo + 31) >> 5;
  const int need = conv5_stage_width(Wo, 32, Wi);
#define W2KERNEL(COT_, PIX_, UNPOOL_, STRAIGHT_)                          \
  hipLaunchKernelGGL((k_conv5_wrw16_nhwc<COT_, PIX_, UNPOOL_, STRAIGHT_>), \
                     dim3(n_wg), dim3(WRW2_THREADS), 0, s, in, gout, part, \
                     Nn, Hi, Wi, Ho, Wo, mask)
  // straight-line walk: every row has the variant's full window count
  // and no block is a one-row tail
#define W2LAUNCH(COT_, PIX_)                                              \
  if (need <= PIX_) {                                                     \
    const bool straight = W == (PIX_ - 4) / 32 && !(Ho & 1);              \
    if (mask && straight)                                                 \
      W2KERNEL(COT_, PIX_, true, true);                                   \
    else if (mask)                                                        \
      W2KERNEL(COT_, PIX_, true, false);                                  \
    else if (straight)                                                    \
      W2KERNEL(COT_, PIX_, false, true);                                  \
    else                                                                  \
      W2KERNEL(COT_, PIX_, false, false);                                 \
    return n_wg;                                                          \
  }
  if (CO == 32) { W2LAUNCH(2, 136) W2LAUNCH(2, 232) }
  if (CO == 16) { W2LAUNCH(1, 136) W2LAUNCH(1, 232) }
#undef W2LAUNCH
#undef W2KERNEL
  return -1;
}

static int wrw4_launch(const bf16_t* in, const bf16_t* gout,
                       const uint8_t* mask, float* part, int Nn, int Hi,
                       int Wi, int Ho, int Wo, int CI, int CO, int n_wg,
                       hipStream_t s) {
  // Wi must be even: the A staging copies 2-pixel (16B) granules
  if (CI != 4 || CO != 16 || (Wi & 1)) return -1;
  if (mask && ((Ho | Wo) & 1)) return -1;
  const int need = conv5_stage_width(Wo, 32, Wi);
#define W4LAUNCH(PIX_)                                                    \
  if (need <= PIX_) {                                                     \
    if (mask)                                                             \
      hipLaunchKernelGGL((k_conv5_wrw4_nhwc<PIX_, true>), dim3(n_wg),     \
                         dim3(WRW2_THREADS), 0, s, in, gout, part, Nn,    \
                         Hi, Wi, Ho, Wo, mask);                           \
    else                                                                  \
      hipLaunchKernelGGL((k_conv5_wrw4_nhwc<PIX_, false>), dim3(n_wg),    \
                         dim3(WRW2_THREADS), 0, s, in, gout, part, Nn,    \
                         Hi, Wi, Ho, Wo, mask);                           \
    return n_wg;                                                          \
  }
  W4LAUNCH(136) W4LAUNCH(232)
#undef W4LAUNCH
  return -1;
}

int geops_conv5_wrw16_nhwc(const bf16_t* in, const bf16_t* gout, float* part,
                           int Nn, int Hi, int Wi, int Ho, int Wo, int CI,
                           int CO, int n_wg, hipStream_t s) {
  return wrw16_launch(in, gout, nullptr, part, Nn, Hi, Wi, Ho, Wo, CI, CO,
                      n_wg, s);
}

int geops_conv5_wrw4_nhwc(const bf16_t* in, const bf16_t* gout, float* part,
                          int Nn, int Hi, int Wi, int Ho, int Wo, int CI,
                          int CO, int n_wg, hipStream_t s) {
  return wrw4_launch(in, gout, nullptr, part, Nn, Hi, Wi, Ho, Wo, CI, CO,
                     n_wg, s);
}

// gp/mask: pooled gradient + argmax codes; Ho, Wo full resolution (even)
int geops_conv5_wrw_unpool_nhwc(const bf16_t* in, const bf16_t* gp,
                                const uint8_t* mask, float* part, int Nn,
                                int Hi, int Wi, int Ho, int Wo, int CI,
                                int CO, int n_wg, hipStream_t s) {
  if (!mask) return -1;
  return (CI == 4 ? wrw4_launch : wrw16_launch)(in, gp, mask, part, Nn, Hi,
                                                Wi, Ho, Wo, CI, CO, n_wg, s);
}

void geops_tr16_probe(const bf16_t* in, bf16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_tr16_probe, dim3(1), dim3(64), 0, s, in, out);
}

void geops_tr16_probe2(const bf16_t* in, const int* addr_off, bf16_t* out,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_tr16_probe2, dim3(1), dim3(64), 0, s, in, addr_off,
                     out);
}

}  // extern "C"
