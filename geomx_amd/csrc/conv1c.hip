// Grayscale conv1 stage (CI = 1, CO = 16, 5x5, stride 1, pad 0) on gfx950:
// the fused forward k_conv5c1_pool and the weight + bias gradient
// k_conv5c1_wrw.
//
// A one-channel image has a shape of its own. NCHW and NHWC are the same
// memory, the whole im2col depth is 25, and eight consecutive K-slots of
// a tap row are eight consecutive pixels of an image row. Both kernels
// therefore keep the input as a plain ROW IMAGE in LDS (bf16 pixels, two
// per dword, rows PITCH bytes apart) and read every A fragment as a
// contiguous 16-byte run of it:
//
//   forward   M = 16 conv pixels, K = kh*8 + kw (kw 5..7 dead, K = 40 in
//             two chunks): lane (q, p) of chunk 0 holds pixels wo..wo+7
//             of staged row r + q, chunk 1 row r + 4 (its q >= 1 k-runs
//             are dead; those lanes read row r + 4 too). Dead slots meet
//             zero weights (build_c1_fwd_index), so the data side only
//             has to be FINITE there: staged pixels or the zero tail.
//   wrw       M = taps (two 16-row tiles: 0..24 taps, 25 bias, 26..31
//             dead), N = 16, K = 32 gout pixels: lane (q, m) holds pixels
//             x0 + 8q + kw_m .. +7 of staged row y + kh_m. No transpose
//             read on the input side; the gout side is the [pix][16]
//             image of the wrw16 kernel, read with ds_read_b64_tr_b16 at
//             pixel base 8q so both operands pair the same pixels.
//
// Alignment. A run starts at any pixel, i.e. on a 2-byte boundary, and
// its parity is a per-lane constant (wo = 16*tile + p; kw_m). The scheme
// chosen is the FUNNEL SHIFT: five aligned ds_read_b32 from dword s >> 1
// and four v_alignbyte_b32 by (s & 1) * 2 bytes (c1_frag). The other
// candidate, a second row image shifted by one pixel, saves the four
// VALU but doubles the ds_writes of staging and needs the odd pixel pairs
// from a second, misaligned global load; both kernels are bound by their
// global traffic and their staging round trip, not by the fragment reads.
//
// Staging. Global rows are only 4 B (bf16) or 8 B (fp32) aligned, so
// rows are staged with plain vector loads of one pixel pair and one
// ds_write_b32 each, no LDS-DMA. An fp32 input is rounded to bf16 with
// cf2bf on the way (PixPair); no bf16 copy of the input ever exists. The
// loads of the NEXT block are issued before this block's MFMA phase and
// wait in registers through it. Each staged row ends in zero pairs that
// cover everything a clamped or last tile reads past the row; rows past
// the image are zero.
//
// A uint8 input comes with a value table, bf16 [256], that the workgroup
// copies into LDS once: byte v stands for tab[v], the bits cf2bf gives
// for the fp32 image table[x] when the host rounded the fp32 table to
// bf16. A pixel pair is then 2 bytes of global traffic (one ushort load)
// and two ds_read_u16 on the way into the row image; everything behind
// the row image is the same for the three input types.

#include <hip/hip_runtime.h>

#include "conv5_common.h"

#define C1_THREADS 256   // 4 waves
#define C1_MAXW 228      // widest served row (14 tiles / 7 K windows + 4)
#define C1_PITCH 576     // row image pitch: 144 dwords = 16 mod 64 banks,
                         // so the rows one read touches sit 16 banks apart

// One pair of adjacent pixels as the input holds it, and as bf16 x 2 (the
// left pixel in the low half). `tab` is the LDS byte address of the value
// table, read by the uint8 form only.
template <typename TIN> struct PixPair;
template <> struct PixPair<float> {
  typedef float2 raw;
  static __device__ __forceinline__ raw zero() { return make_float2(0, 0); }
  static __device__ __forceinline__ raw ld(const float* p) {
    return *reinterpret_cast<const raw*>(p);
  }
  static __device__ __forceinline__ unsigned pack(raw v, unsigned) {
    return (unsigned)cf2bf(v.x) | ((unsigned)cf2bf(v.y) << 16);
  }
};
template <> struct PixPair<bf16_t> {
  typedef unsigned raw;
  static __device__ __forceinline__ raw zero() { return 0u; }
  static __device__ __forceinline__ raw ld(const bf16_t* p) {
    return *reinterpret_cast<const raw*>(p);
  }
  static __device__ __forceinline__ unsigned pack(raw v, unsigned) {
    return v;
  }
};
// A pair past the image stages as zero bits, which tab[0] need not be: a
// loaded pair carries bit 16 and zero() does not.
template <> struct PixPair<uint8_t> {
  typedef unsigned raw;
  static __device__ __forceinline__ raw zero() { return 0u; }
  static __device__ __forceinline__ raw ld(const uint8_t* p) {
    return 0x10000u | *reinterpret_cast<const unsigned short*>(p);
  }
  static __device__ __forceinline__ unsigned pack(raw v, unsigned tab) {
    typedef const __attribute__((address_space(3))) unsigned short* lds_u16;
    const unsigned lo = *(lds_u16)(uintptr_t)(tab + (v & 0xFFu) * 2);
    const unsigned hi = *(lds_u16)(uintptr_t)(tab + ((v >> 8) & 0xFFu) * 2);
    return (v >> 16) ? (lo | (hi << 16)) : 0u;
  }
};
constexpr int C1_TAB = 256;   // table entries

// The uint8 forms' table into LDS, once per workgroup; the barrier puts
// it ahead of the first lookups. Nothing for the other input types.
template <typename TIN>
__device__ __forceinline__ void c1_tab_load(bf16_t* lds_tab,
                                            const bf16_t* __restrict__ tab) {
  if constexpr (sizeof(TIN) == 1) {
    for (int t = threadIdx.x; t < C1_TAB / 2; t += C1_THREADS)
      reinterpret_cast<unsigned*>(lds_tab)[t] =
          reinterpret_cast<const unsigned*>(tab)[t];
    __syncthreads();
  }
}

// Eight pixels from pixel s of a row image as one MFMA operand: `a` is
// the LDS byte address of dword s >> 1, `sh` = (s & 1) * 2.
__device__ __forceinline__ bf16x8 c1_frag(unsigned a, unsigned sh) {
  typedef const __attribute__((address_space(3))) unsigned* lds_u32;
  unsigned d[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) d[i] = *(lds_u32)(uintptr_t)(a + 4 * i);
  union { unsigned u[4]; bf16x8 h; } c;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    c.u[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
  return c.h;
}

// Row-image staging shared by both kernels: item i of a thread is pixel
// pair `col` of staged row `row` (fixed for the kernel's life, so the
// divisions run once); pairs past the image row and rows past the image
// are zero.
template <typename TIN, int NIT>
struct C1Stage {
  typedef typename PixPair<TIN>::raw raw;
  int row[NIT], col[NIT];
  raw v[NIT];

  // nrow rows of rw pairs each
  __device__ __forceinline__ void init(int nrow, int rw) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = threadIdx.x + i * C1_THREADS;
      row[i] = it / rw;
      col[i] = it - row[i] * rw;
      if (row[i] >= nrow) row[i] = -1;   // no item
    }
  }
  // rows h0 .. of image n
  __device__ __forceinline__ void load(const TIN* __restrict__ x,
                                       long long n, int h0, int H, int W) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      v[i] = PixPair<TIN>::zero();
      if (row[i] >= 0 && h0 + row[i] < H && 2 * col[i] < W)
        v[i] = PixPair<TIN>::ld(
            x + ((n * H + (h0 + row[i])) * (long long)W + 2 * col[i]));
    }
  }
  __device__ __forceinline__ void write(char* img, unsigned tab) const {
#pragma unroll
    for (int i = 0; i < NIT; ++i)
      if (row[i] >= 0)
        *reinterpret_cast<unsigned*>(img + row[i] * C1_PITCH + col[i] * 4) =
            PixPair<TIN>::pack(v[i], tab);
  }
};

// ---------------------------------------------------------------------
// Forward: conv(1 -> 16) + bias + ReLU + 2x2 max-pool. out / mask are
// what k_conv5_pool2_nhwc writes: [N][Ho/2][Wo/2][16] bf16 and the uint8
// argmax codes at the same flat index.
//
// Persistent. A block is 4 conv rows (2 pooled rows) of one image: 8
// input rows in one of two row images. Per block
//
//     write the pairs loaded during the previous phase into image i
//     barrier
//     store the PREVIOUS block's packed results
//     load the next block's pairs into registers
//     MFMA phase on image i, pool, pack into registers
//
// so there is one barrier per block: image i ^ 1 is written while slower
// waves still read image i, and is not written again before every wave
// has passed the next barrier. The four waves split the 16-pixel tiles
// (tile = wave + 4u); a wave's tile is 4 conv rows x 2 chunks = 8 MFMAs.
// Pooling and the packed epilogue are those of k_conv5_pool2_nhwc:
// horizontal pairs in one lane, vertical pairs in two accumulators,
// quad_tr4 / pack_codes to one 8-byte out store and one 4-byte mask store
// per lane and tile. With an odd number of pooled rows the last block of
// an image stages zero rows below the image and stores one pooled row.
// ---------------------------------------------------------------------
template <typename TIN>
__global__ __launch_bounds__(C1_THREADS) void k_conv5c1_pool(
    const TIN* __restrict__ x,           // [N][H][W]
    const bf16_t* __restrict__ w_frags,  // [2][64][8]
    const float* __restrict__ bias,      // [16] or nullptr
    bf16_t* __restrict__ out,            // [N][Hop][Wop][16]
    uint8_t* __restrict__ mask,          // [N*Hop*Wop*16]
    int Nn, int H, int W,
    const bf16_t* __restrict__ tab) {    // uint8 form: [256]
  constexpr int CO = 16;
  constexpr int ROWS = 4;                 // conv rows per block
  constexpr int NROW = ROWS + 4;
  constexpr int IMG = NROW * C1_PITCH;
  constexpr int MAXU = (C1_MAXW - 4) / 16 / 4 + 1;        // tiles per wave
  constexpr int MAXRW = C1_MAXW / 2 + 2;  // pairs per staged row
  constexpr int NIT = (NROW * MAXRW + C1_THREADS - 1) / C1_THREADS;
  static_assert(MAXRW * 4 <= C1_PITCH, "row and zero tail fit the pitch");
  static_assert(MAXU * 4 * 16 >= C1_MAXW - 4, "tiles cover the row");
  __shared__ __attribute__((aligned(16))) char lds_rows[2 * IMG];
  __shared__ __attribute__((aligned(16))) bf16_t
      lds_tab[sizeof(TIN) == 1 ? C1_TAB : 2];
  c1_tab_load<TIN>(lds_tab, tab);
  const unsigned tab0 = lds_addr(lds_tab);

  const int lane = threadIdx.x & 63;
  const int p = lane & 15;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  bf16x8 breg[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    breg[i] = *reinterpret_cast<const bf16x8*>(w_frags + (i * 64 + lane) * 8);
  const float bias_v = bias ? bias[m] : 0.0f;

  const int Ho = H - 4, Wo = W - 4;
  const int Hop = Ho >> 1, Wop = Wo >> 1;
  const int tiles_w = (Wo + 15) >> 4;
  const int hblocks = (Hop + 1) >> 1;
  const long long n_blocks = (long long)Nn * hblocks;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const unsigned lds0 = lds_addr(lds_rows);

  // per-lane read position of tile u in image 0, staged row 0. A pixel
  // past the row clamps to the last one: in bounds, never stored. The
  // clamped run ends at pixel Wo + 7 and its fifth dword at W + 3: the
  // two zero pairs behind every staged row.
  unsigned aofs[MAXU], ash[MAXU];
#pragma unroll
  for (int u = 0; u < MAXU; ++u) {
    const int wo_raw = ((wid + 4 * u) << 4) + p;
    const int wo = wo_raw < Wo ? wo_raw : (Wo - 1);
    aofs[u] = lds0 + (unsigned)((wo >> 1) * 4);
    ash[u] = (unsigned)((wo & 1) * 2);
  }

  C1Stage<TIN, NIT> st;
  st.init(NROW, (W >> 1) + 2);
  auto load = [&](long long b) {
    const long long n = b / hblocks;
    st.load(x, n, (int)(b - n * hblocks) * ROWS, H, W);
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
  if (blk < n_blocks) load(blk);
  long long pn = 0;
  int phb = 0, pnpr = 0;
  for (; blk < n_blocks; blk += n_wg, img ^= 1) {
    st.write(lds_rows + img * IMG, tab0);
    __syncthreads();
    flush(pn, phb, pnpr);
    if (blk + n_wg < n_blocks) load(blk + n_wg);

    const long long n = blk / hblocks;
    const int hb = (int)(blk - n * hblocks);
    const unsigned ib = (unsigned)(img * IMG);
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      if (wid + 4 * u >= tiles_w) break;
      const unsigned a = aofs[u] + ib;
      bf16x8 f0[ROWS], f1[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        f0[r] = c1_frag(a + (r + q) * C1_PITCH, ash[u]);
        f1[r] = c1_frag(a + (r + 4) * C1_PITCH, ash[u]);
      }
      f32x4 acc[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            f0[r], breg[0], (f32x4)0.0f, 0, 0, 0);
        acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            f1[r], breg[1], acc[r], 0, 0, 0);
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

// ---------------------------------------------------------------------
// Weight + bias gradient:
//   dW[kh*5+kw][o] = sum x[n][y+kh][x+kw] * g[n][y][x][o],  db[o] = sum g
// as per-workgroup slabs part[wg][32][16] (rows 0..24 taps, 25 bias,
// 26..31 zero; every row written), summed by the host.
//
// Persistent. A block is 2 conv rows of one image (one pooled row): 6
// input rows in the row image and 2 gout rows in the [pix][16] image of
// Wn = ceil(Wo / 32) K windows, zero from Wo to 32 * Wn. UNPOOL builds
// the gout image from the pooled gradient and its argmax codes
// (pooled_load / pooled_write); the plain form copies the full-
// resolution gradient, rows past the image as zeros, so a block always
// walks 2 * Wn (row, window) steps. Per block
//
//     write the staged registers to LDS; barrier
//     load the next block's pixels and gradient into registers
//     walk; barrier
//
// A step is two MFMAs (the two tap tiles) on one B fragment. The steps
// go round-robin over the four waves, each wave accumulating the whole
// 32 x 16 slab; the reads of a wave's next step are issued ahead of the
// MFMAs of this one. The bias row reads an LDS run of bf16 ones and the
// dead rows a run of zeros, both at fixed addresses (step multiplier 0).
// At the end the four waves' accumulators are summed through LDS in wave
// order 0..3, so a slab is a function of (inputs, n_wg) alone.
// ---------------------------------------------------------------------
__device__ __forceinline__ bf16x4 c1_tr16_ld(unsigned a) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)(uintptr_t)a);
}

template <typename TIN, bool UNPOOL>
__global__ __launch_bounds__(C1_THREADS) void k_conv5c1_wrw(
    const TIN* __restrict__ x,         // [N][H][W]
    const bf16_t* __restrict__ g,      // [N][Ho][Wo][16]; UNPOOL: the
                                       // pooled [N][Ho/2][Wo/2][16]
    const uint8_t* __restrict__ mask,  // UNPOOL: argmax codes, as g
    float* __restrict__ part,          // [n_wg][32][16]
    int Nn, int H, int W,
    const bf16_t* __restrict__ tab) {  // uint8 form: [256]
  constexpr int NROW_A = 2 + 4;
  constexpr int WMAX = (C1_MAXW - 4) / 32;         // 7 K windows
  constexpr int PB = WMAX * 1024;                  // gout row: 32 B / pixel
  constexpr int B_OFF = NROW_A * C1_PITCH;
  constexpr int ONES = B_OFF + 2 * PB;             // 32 B of ones, 32 of 0
  constexpr int MAXRW = 16 * WMAX + 3;
  constexpr int NIT_A = (NROW_A * MAXRW + C1_THREADS - 1) / C1_THREADS;
  constexpr int NIT_B = (2 * WMAX * 64 + C1_THREADS - 1) / C1_THREADS;
  constexpr int NIT_P = (16 * WMAX * 2 + C1_THREADS - 1) / C1_THREADS;
  static_assert(MAXRW * 4 <= C1_PITCH, "row and zero tail fit the pitch");
  static_assert(B_OFF % 16 == 0 && 4 * 512 * 4 <= 2 * PB,
                "gout image aligned; the slab reduction fits in it");
  __shared__ __attribute__((aligned(16))) char lds_all[ONES + 64];
  __shared__ __attribute__((aligned(16))) bf16_t
      lds_tab[sizeof(TIN) == 1 ? C1_TAB : 2];
  c1_tab_load<TIN>(lds_tab, tab);
  const unsigned tab0 = lds_addr(lds_tab);

  const int lane = threadIdx.x & 63;
  const int q = lane >> 4;
  const int m = lane & 15;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int Ho = H - 4, Wo = W - 4;
  const int Wn = (Wo + 31) >> 5;
  const int blocks_h = (Ho + 1) >> 1;
  const long long n_blocks = (long long)Nn * blocks_h;
  const int wg = blockIdx.x;
  const int n_wg = gridDim.x;
  const unsigned lds0 = lds_addr(lds_all);

  if (threadIdx.x < 16)                    // visible after the first barrier
    reinterpret_cast<unsigned*>(lds_all + ONES)[threadIdx.x] =
        threadIdx.x < 8 ? 0x3F803F80u : 0u;

  // per-lane fragment bases at (row 0, window 0). Tap m of tile 0 and
  // taps 16..24 of tile 1 move with the step; the bias row and the dead
  // rows of tile 1 stay where they are (amul1 = 0).
  unsigned abase[2], ashv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int tap = 16 * t + m;
    const int kh = tap / 5, kw = tap - kh * 5;
    abase[t] = lds0 + (unsigned)(kh * C1_PITCH + (4 * q + (kw >> 1)) * 4);
    ashv[t] = (unsigned)((kw & 1) * 2);
  }
  const unsigned amul1 = m < 9 ? 1u : 0u;
  if (m >= 9) {
    abase[1] = lds0 + ONES + (m == 9 ? 0 : 32);
    ashv[1] = 0u;
  }
  const unsigned bbase = lds0 + B_OFF + (8 * q) * 32 + m * 8;

  // ---- staging
  C1Stage<TIN, NIT_A> st;
  st.init(NROW_A, 16 * Wn + 3);   // the last window's run ends in dword
                                  // 16 * Wn + 2
  uint4 gq[UNPOOL ? NIT_P : NIT_B];
  uint2 mq[NIT_P];
  auto load = [&](long long n, int bh) {
    st.load(x, n, bh * 2, H, W);
    if constexpr (UNPOOL) {
      pooled_load<NIT_P, C1_THREADS, 2>(g, mask, n, bh, Ho, Wo, gq, mq);
    } else {
#pragma unroll
      for (int i = 0; i < NIT_B; ++i) {
        const int it = threadIdx.x + i * C1_THREADS;
        const int r = it >= 64 * Wn ? 1 : 0;
        const int rem = it - r * 64 * Wn;          // 2 granules per pixel
        gq[i] = make_uint4(0u, 0u, 0u, 0u);
        if (it < 128 * Wn && (rem >> 1) < Wo && bh * 2 + r < Ho)
          gq[i] = reinterpret_cast<const uint4*>(
              g)[((n * Ho + (bh * 2 + r)) * (long long)Wo) * 2 + rem];
      }
    }
  };
  auto write = [&]() {
    st.write(lds_all, tab0);
    if constexpr (UNPOOL) {
      pooled_write<NIT_P, C1_THREADS, 1, B_OFF, 0, PB>(lds_all, Wn, gq, mq);
    } else {
#pragma unroll
      for (int i = 0; i < NIT_B; ++i) {
        const int it = threadIdx.x + i * C1_THREADS;
        const int r = it >= 64 * Wn ? 1 : 0;
        const int rem = it - r * 64 * Wn;
        if (it < 128 * Wn)
          *reinterpret_cast<uint4*>(lds_all + B_OFF + r * PB + rem * 16) =
              gq[i];
      }
    }
  };

  // ---- the walk
  f32x4 acc[2] = {(f32x4)0.0f, (f32x4)0.0f};
  struct Frags { bf16x8 a0, a1, b; };
  auto ld = [&](int s) {
    const int r = s >= Wn ? 1 : 0;
    const int w = s - r * Wn;
    const unsigned oa = (unsigned)(r * C1_PITCH + w * 64);
    const unsigned ob = bbase + (unsigned)(r * PB + w * 1024);
    Frags f;
    f.a0 = c1_frag(abase[0] + oa, ashv[0]);
    f.a1 = c1_frag(abase[1] + oa * amul1, ashv[1]);
    f.b = join_bf16x4(c1_tr16_ld(ob), c1_tr16_ld(ob + 128));
    return f;
  };
  auto walk = [&]() {
    const int nsteps = 2 * Wn;
    int s = wid;
    if (s >= nsteps) return;
    Frags cur = ld(s);
    for (; s < nsteps; s += 4) {
      // the step after the last re-reads the last one (unused)
      const Frags nxt = ld(s + 4 < nsteps ? s + 4 : s);
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.a0, cur.b, acc[0],
                                                       0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.a1, cur.b, acc[1],
                                                       0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      cur = nxt;
    }
  };

  // block = (image n, row pair bh), decoded once, one block ahead
  long long blk = wg;
  long long n = 0;
  int bh = 0;
  if (blk < n_blocks) {
    n = blk / blocks_h;
    bh = (int)(blk - n * blocks_h);
    load(n, bh);
  }
  for (; blk < n_blocks; blk += n_wg) {
    write();
    __syncthreads();
    if (blk + n_wg < n_blocks) {
      n = (blk + n_wg) / blocks_h;
      bh = (int)(blk + n_wg - n * blocks_h);
      load(n, bh);
    }
    walk();
    __syncthreads();  // before the next block restages LDS
  }

  // ---- the four waves' slabs summed in wave order; C/D layout: lane
  // (q, m), reg i -> row q*4 + i (tap within the tile), col m (o)
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds_all + B_OFF);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[wid * 512 + (16 * t + 4 * q + i) * 16 + m] = acc[t][i];
  __syncthreads();
  float* base = part + (long long)wg * 512;
#pragma unroll
  for (int e = threadIdx.x; e < 512; e += C1_THREADS)
    base[e] = ((red[e] + red[512 + e]) + red[1024 + e]) + red[1536 + e];
}

// ---------------------------------------------------------------------
// Launchers. Both kernels serve even W from 6 to C1_MAXW; the forward
// and the pooled wrw also need an even Ho. x_kind says what x holds: 0
// bf16, 1 fp32, 2 uint8 with its table `tab` (bf16 [256], 4 B aligned;
// null for the other kinds). n_wg >= 1 is the grid. Return 0, or -1
// outside the served table.
// ---------------------------------------------------------------------
static bool c1_kind_ok(int x_kind, const bf16_t* tab) {
  if (x_kind == 2) return tab && ((uintptr_t)tab & 3) == 0;
  return (x_kind == 0 || x_kind == 1) && !tab;
}

extern "C" {

int geops_conv5c1_pool(const void* x, int x_kind, const bf16_t* tab,
                       const bf16_t* w_frags, const float* bias, bf16_t* out,
                       uint8_t* mask, int Nn, int H, int W, int n_wg,
                       hipStream_t s) {
  if (Nn < 1 || H < 6 || W < 6 || W > C1_MAXW || (W & 1) || (H & 1) ||
      n_wg < 1 || !c1_kind_ok(x_kind, tab))
    return -1;
#define C1POOL(TIN_)                                                       \
  hipLaunchKernelGGL((k_conv5c1_pool<TIN_>), dim3(n_wg), dim3(C1_THREADS), \
                     0, s, (const TIN_*)x, w_frags, bias, out, mask, Nn, H, \
                     W, tab)
  if (x_kind == 2) C1POOL(uint8_t);
  else if (x_kind == 1) C1POOL(float);
  else C1POOL(bf16_t);
#undef C1POOL
  return 0;
}

// mask == nullptr: g is the full-resolution gradient; otherwise the
// pooled gradient and its argmax codes.
int geops_conv5c1_wrw(const void* x, int x_kind, const bf16_t* tab,
                      const bf16_t* g, const uint8_t* mask, float* part,
                      int Nn, int H, int W, int n_wg, hipStream_t s) {
  if (Nn < 1 || H < 5 || W < 6 || W > C1_MAXW || (W & 1) || n_wg < 1 ||
      (mask && (H & 1)) || !c1_kind_ok(x_kind, tab))
    return -1;
#define C1WRW(TIN_)                                                         \
  do {                                                                      \
    if (mask)                                                               \
      hipLaunchKernelGGL((k_conv5c1_wrw<TIN_, true>), dim3(n_wg),           \
                         dim3(C1_THREADS), 0, s, (const TIN_*)x, g, mask,   \
                         part, Nn, H, W, tab);                              \
    else                                                                    \
      hipLaunchKernelGGL((k_conv5c1_wrw<TIN_, false>), dim3(n_wg),          \
                         dim3(C1_THREADS), 0, s, (const TIN_*)x, g, mask,   \
                         part, Nn, H, W, tab);                              \
  } while (0)
  if (x_kind == 2) C1WRW(uint8_t);
  else if (x_kind == 1) C1WRW(float);
  else C1WRW(bf16_t);
#undef C1WRW
  return 0;
}

}  // extern "C"
