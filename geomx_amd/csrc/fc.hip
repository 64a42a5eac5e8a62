// NHWC-native backward of the first dense layer (classifier head) for
// gfx950.
//
// The conv stack hands the head a channels_last feature map, so the
// flattened K axis the data already has is (h, w, c). nn.Linear keeps
// its weight in (c, h, w) order. The head's backward runs its two GEMMs
// in the data's order instead of copying the 92 MB activation gradient
// back to channels_last; the permutation is paid on the weight side,
// inside casts of the weight's size:
//
//   k_fc_w_permute_bf16    fp32 [O][C][HW] -> bf16 [O][HW][C]
//                          (the data-gradient GEMM's weight operand)
//   k_fc_w_unpermute_f32   bf16 [O][HW][C] -> fp32 [O][C][HW]
//                          (replaces the weight gradient's bf16 -> fp32)
//   k_fc_w_pack2_bf16      the permute kernel plus the forward GEMM's
//                          plain bf16 cast, from one read of the weight
//   k_fc_w_unpermute_into  the un-permute, written into a caller-given
//                          span (the trainer's gradient bucket)
//
// The forward GEMM reduces over K, so it keeps the (c, h, w) order and
// its rounding; its activation copy is k_fc_flatten_nchw, an LDS-tiled
// transpose in place of the strided elementwise copy.
//
// C is fixed at 32: a weight row of the permuted layout is a sequence
// of 64 B pixel records, one 16 B store per lane.

#include <hip/hip_runtime.h>

#include <cstdint>

typedef unsigned short bf16_t;
typedef __attribute__((ext_vector_type(8))) short bf16x8;

#define FC_C 32           // channels per pixel
#define FC_THREADS 256    // 4 waves
#define FC_PERM_HW 128    // pixels per permute tile
#define FC_PERM_LD 129    // LDS row stride (floats): +1 keeps both the
                          // [c][hw] writes and the 8-channel column
                          // reads conflict-free

__device__ __forceinline__ bf16_t fc_f2bf(float f) {
  union { float f; unsigned int u; } cv;
  cv.f = f;
  if ((cv.u & 0x7FFFFFFFu) > 0x7F800000u)  // NaN: quiet, keep the sign
    return (bf16_t)((cv.u >> 16) | 0x0040u);
  const unsigned int lsb = (cv.u >> 16) & 1;  // round-to-nearest-even
  return (bf16_t)((cv.u + 0x7FFFu + lsb) >> 16);
}

// fp32 [O][32][HW] -> bf16 [O][HW][32]. grid (ceil(HW/128), O).
// Reads are dword-coalesced along hw (HW may be odd: a channel row is
// only 4 B aligned); writes are 16 B per lane, 64 B per pixel.
__global__ __launch_bounds__(FC_THREADS) void k_fc_w_permute_bf16(
    const float* __restrict__ w, bf16_t* __restrict__ wp, int HW) {
  __shared__ float tile[FC_C * FC_PERM_LD];
  const int t = threadIdx.x;
  const int hw0 = blockIdx.x * FC_PERM_HW;
  const long long o = blockIdx.y;
  const float* src = w + o * FC_C * HW;
  {
    // all 16 loads of a lane are issued before the first LDS write
    const int hw = t & (FC_PERM_HW - 1), c0 = t >> 7;
    if (hw0 + hw < HW) {
      float v[FC_C / 2];
#pragma unroll
      for (int i = 0; i < FC_C / 2; ++i)
        v[i] = src[(long long)(c0 + 2 * i) * HW + hw0 + hw];
#pragma unroll
      for (int i = 0; i < FC_C / 2; ++i)
        tile[(c0 + 2 * i) * FC_PERM_LD + hw] = v[i];
    }
  }
  __syncthreads();
  bf16_t* dst = wp + o * HW * FC_C;
  const int cg = t & 3;  // channel group of 8
#pragma unroll
  for (int p = 0; p < FC_PERM_HW / (FC_THREADS / 4); ++p) {
    const int hw = p * (FC_THREADS / 4) + (t >> 2);
    if (hw0 + hw < HW) {
      union { bf16x8 v; bf16_t e[8]; } pk;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        pk.e[j] = fc_f2bf(tile[(cg * 8 + j) * FC_PERM_LD + hw]);
      *reinterpret_cast<bf16x8*>(dst + (long long)(hw0 + hw) * FC_C +
                                 cg * 8) = pk.v;
    }
  }
}

// Both bf16 layouts of the weight from ONE read of the fp32 master:
//   wb  bf16 [O][32][HW]  the forward GEMM's operand (weight order)
//   wp  bf16 [O][HW][32]  the data-gradient operand, as the permute
//                         kernel writes it; wp == nullptr skips it
// Same block as k_fc_w_permute_bf16 (one per (o, 128-pixel tile), the
// [32][129] fp32 tile, fc_f2bf); the wp half is that kernel's code. The
// wb half walks along hw the way k_fc_flatten_nchw does: HW may be odd,
// so a channel row is only 2 B aligned; pairs are taken on even GLOBAL
// element indices (4 B stores), and the one or two elements a tile has
// left over at its ends go out as 2 B stores. wb itself is 4 B aligned.
__global__ __launch_bounds__(FC_THREADS) void k_fc_w_pack2_bf16(
    const float* __restrict__ w, bf16_t* __restrict__ wb,
    bf16_t* __restrict__ wp, int HW) {
  __shared__ float tile[FC_C * FC_PERM_LD];
  const int t = threadIdx.x;
  const int hw0 = blockIdx.x * FC_PERM_HW;  // even
  const long long o = blockIdx.y;
  const float* src = w + o * FC_C * HW;
  {
    const int hw = t & (FC_PERM_HW - 1), c0 = t >> 7;
    if (hw0 + hw < HW) {
      float v[FC_C / 2];
#pragma unroll
      for (int i = 0; i < FC_C / 2; ++i)
        v[i] = src[(long long)(c0 + 2 * i) * HW + hw0 + hw];
#pragma unroll
      for (int i = 0; i < FC_C / 2; ++i)
        tile[(c0 + 2 * i) * FC_PERM_LD + hw] = v[i];
    }
  }
  __syncthreads();
  if (wp != nullptr) {
    bf16_t* dst = wp + o * HW * FC_C;
    const int cg = t & 3;  // channel group of 8
#pragma unroll
    for (int p = 0; p < FC_PERM_HW / (FC_THREADS / 4); ++p) {
      const int hw = p * (FC_THREADS / 4) + (t >> 2);
      if (hw0 + hw < HW) {
        union { bf16x8 v; bf16_t e[8]; } pk;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          pk.e[j] = fc_f2bf(tile[(cg * 8 + j) * FC_PERM_LD + hw]);
        *reinterpret_cast<bf16x8*>(dst + (long long)(hw0 + hw) * FC_C +
                                   cg * 8) = pk.v;
      }
    }
  }
  const int wave = t >> 6, lane = t & 63;
#pragma unroll
  for (int i = 0; i < FC_C / 4; ++i) {
    const int c = wave * (FC_C / 4) + i;
    const long long row = (o * FC_C + c) * HW + hw0;  // first element
    const int par = (int)(row & 1);
    const float* trow = tile + c * FC_PERM_LD;
    bf16_t* dst = wb + row;
    const int e0 = 2 * lane - par, e1 = e0 + 1;  // row + e0 is even
    const bool ok0 = e0 >= 0 && hw0 + e0 < HW;
    const bool ok1 = hw0 + e1 < HW;
    if (ok0 && ok1) {
      const unsigned v = (unsigned)fc_f2bf(trow[e0]) |
                         ((unsigned)fc_f2bf(trow[e1]) << 16);
      *reinterpret_cast<unsigned*>(dst + e0) = v;
    } else if (ok0) {
      dst[e0] = fc_f2bf(trow[e0]);
    } else if (ok1) {
      dst[e1] = fc_f2bf(trow[e1]);
    }
    // an odd row leaves the tile's last element unpaired
    if (par && lane == 0 && hw0 + FC_PERM_HW - 1 < HW)
      dst[FC_PERM_HW - 1] = fc_f2bf(trow[FC_PERM_HW - 1]);
  }
}

// bf16 [O][HW][32] -> fp32 [O][32][HW]: the mirror image. kPosZero
// stores x + 0.0f, the value `0 + x` of an accumulation into a cleared
// buffer: a -0 becomes +0, everything else keeps its bits.
template <bool kPosZero>
__device__ __forceinline__ void fc_w_unpermute_body(
    const bf16_t* __restrict__ gp, float* __restrict__ g, int HW) {
  __shared__ float tile[FC_C * FC_PERM_LD];
  const int t = threadIdx.x;
  const int hw0 = blockIdx.x * FC_PERM_HW;
  const long long o = blockIdx.y;
  const bf16_t* src = gp + o * HW * FC_C;
  const int cg = t & 3;
#pragma unroll
  for (int p = 0; p < FC_PERM_HW / (FC_THREADS / 4); ++p) {
    const int hw = p * (FC_THREADS / 4) + (t >> 2);
    if (hw0 + hw < HW) {
      union { bf16x8 v; bf16_t e[8]; } pk;
      pk.v = *reinterpret_cast<const bf16x8*>(
          src + (long long)(hw0 + hw) * FC_C + cg * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        union { unsigned int u; float f; } cv;
        cv.u = (unsigned int)pk.e[j] << 16;
        tile[(cg * 8 + j) * FC_PERM_LD + hw] = cv.f;
      }
    }
  }
  __syncthreads();
  float* dst = g + o * FC_C * HW;
  const int hw = t & (FC_PERM_HW - 1), c0 = t >> 7;
  if (hw0 + hw < HW) {
#pragma unroll
    for (int i = 0; i < FC_C / 2; ++i) {
      const float v = tile[(c0 + 2 * i) * FC_PERM_LD + hw];
      dst[(long long)(c0 + 2 * i) * HW + hw0 + hw] = kPosZero ? v + 0.0f : v;
    }
  }
}

__global__ __launch_bounds__(FC_THREADS) void k_fc_w_unpermute_f32(
    const bf16_t* __restrict__ gp, float* __restrict__ g, int HW) {
  fc_w_unpermute_body<false>(gp, g, HW);
}

// The same into a caller-given dense [O][32*HW] destination that may
// start at any 4 B-aligned address inside a larger buffer (the stores
// are dword-wise): the weight gradient written where it is consumed.
__global__ __launch_bounds__(FC_THREADS) void k_fc_w_unpermute_into(
    const bf16_t* __restrict__ gp, float* __restrict__ g, int HW) {
  fc_w_unpermute_body<true>(gp, g, HW);
}

// Flatten of a channels_last activation: bf16 [N][HW][32] -> bf16
// [N][32][HW], the NCHW-flatten order nn.Linear's weight is in. Pure
// data movement (bit-exact with torch.flatten's strided copy), through
// a [32][HW tile] LDS tile so that both sides are coalesced: 16 B loads
// (a pixel is 64 contiguous bytes), 4 B stores of two pixels along hw.
// HW may be odd, so an output row starts on either 2 B parity; pairs
// are taken on even GLOBAL element indices and the one or two elements
// a tile has left over at its ends go out as 2 B stores.
// grid (ceil(HW/128), N), one wave per 8 channel rows.
#define FC_FLAT_LD 130  // LDS row stride (bf16): 65 dwords, odd
__global__ __launch_bounds__(FC_THREADS) void k_fc_flatten_nchw(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int HW) {
  __shared__ bf16_t tile[FC_C * FC_FLAT_LD];
  const int t = threadIdx.x;
  const int hw0 = blockIdx.x * FC_PERM_HW;  // even
  const long long n = blockIdx.y;
  const bf16_t* src = x + n * HW * FC_C;
  const int cg = t & 3;
#pragma unroll
  for (int p = 0; p < FC_PERM_HW / (FC_THREADS / 4); ++p) {
    const int hw = p * (FC_THREADS / 4) + (t >> 2);
    if (hw0 + hw < HW) {
      union { bf16x8 v; bf16_t e[8]; } pk;
      pk.v = *reinterpret_cast<const bf16x8*>(
          src + (long long)(hw0 + hw) * FC_C + cg * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        tile[(cg * 8 + j) * FC_FLAT_LD + hw] = pk.e[j];
    }
  }
  __syncthreads();
  const int wave = t >> 6, lane = t & 63;
#pragma unroll
  for (int i = 0; i < FC_C / 4; ++i) {
    const int c = wave * (FC_C / 4) + i;
    const long long row = (n * FC_C + c) * HW + hw0;  // first element
    const int par = (int)(row & 1);
    const bf16_t* trow = tile + c * FC_FLAT_LD;
    bf16_t* dst = y + row;
    const int e0 = 2 * lane - par, e1 = e0 + 1;  // row + e0 is even
    const bool ok0 = e0 >= 0 && hw0 + e0 < HW;
    const bool ok1 = hw0 + e1 < HW;
    if (ok0 && ok1) {
      const unsigned v = (unsigned)trow[e0] | ((unsigned)trow[e1] << 16);
      *reinterpret_cast<unsigned*>(dst + e0) = v;
    } else if (ok0) {
      dst[e0] = trow[e0];
    } else if (ok1) {
      dst[e1] = trow[e1];
    }
    // an odd row leaves the tile's last element unpaired
    if (par && lane == 0 && hw0 + FC_PERM_HW - 1 < HW)
      dst[FC_PERM_HW - 1] = trow[FC_PERM_HW - 1];
  }
}

extern "C" {

// Launch table of the head kernels: C == 32, every extent positive and
// inside the grid limits. Returns 0 on launch, -1 for a geometry
// outside the table (nothing is launched).
static bool fc_geometry_ok(long long rows, int C, int HW) {
  return C == FC_C && rows > 0 && rows <= 65535 && HW > 0 &&
         HW <= (1 << 24);
}

int geops_fc_w_permute_bf16(const float* w, bf16_t* wp, int O, int C, int HW,
                            hipStream_t s) {
  if (!fc_geometry_ok(O, C, HW)) return -1;
  hipLaunchKernelGGL(k_fc_w_permute_bf16,
                     dim3((HW + FC_PERM_HW - 1) / FC_PERM_HW, O),
                     dim3(FC_THREADS), 0, s, w, wp, HW);
  return 0;
}

int geops_fc_w_unpermute_f32(const bf16_t* gp, float* g, int O, int C, int HW,
                             hipStream_t s) {
  if (!fc_geometry_ok(O, C, HW)) return -1;
  hipLaunchKernelGGL(k_fc_w_unpermute_f32,
                     dim3((HW + FC_PERM_HW - 1) / FC_PERM_HW, O),
                     dim3(FC_THREADS), 0, s, gp, g, HW);
  return 0;
}

int geops_fc_w_pack2_bf16(const float* w, bf16_t* wb, bf16_t* wp, int O,
                          int C, int HW, hipStream_t s) {
  if (!fc_geometry_ok(O, C, HW)) return -1;
  hipLaunchKernelGGL(k_fc_w_pack2_bf16,
                     dim3((HW + FC_PERM_HW - 1) / FC_PERM_HW, O),
                     dim3(FC_THREADS), 0, s, w, wb, wp, HW);
  return 0;
}

int geops_fc_w_unpermute_into(const bf16_t* gp, float* g, int O, int C,
                              int HW, hipStream_t s) {
  if (!fc_geometry_ok(O, C, HW)) return -1;
  hipLaunchKernelGGL(k_fc_w_unpermute_into,
                     dim3((HW + FC_PERM_HW - 1) / FC_PERM_HW, O),
                     dim3(FC_THREADS), 0, s, gp, g, HW);
  return 0;
}

int geops_fc_flatten_nchw(const bf16_t* x, bf16_t* y, int N, int C, int HW,
                          hipStream_t s) {
  if (!fc_geometry_ok(N, C, HW)) return -1;
  hipLaunchKernelGGL(k_fc_flatten_nchw,
                     dim3((HW + FC_PERM_HW - 1) / FC_PERM_HW, N),
                     dim3(FC_THREADS), 0, s, x, y, HW);
  return 0;
}

}  // extern "C"
