// gfx950 (MI355X / CDNA4) fused DGT encode: the send side of DGT mode 3.
// One kernel turns a gradient bucket and its residual into the wire payload
// of DGTState.compress,
//
//   exact  f32 [n_keep][chunk]     the kept chunks, raw x
//   packed u8  [n_lossy][chunk/2]  4-bit codes of x + residual of the rest
//   minmax f32 [n_lossy][2]        their codebooks (lo, hi)
//
// and updates the residual in place (0 for a kept chunk, the quantization
// error for a lossy one). It is the mirror of k_wire_sum_dgt: the sorted
// keep_idx alone says which row a chunk is, so there is no mask, no nonzero
// and no gather. The bits are those of the chain it replaces (zero-padded
// copies, k_minmax_chunk, k_quantize_4bit, row gathers, dead-chunk masks,
// ops.reference.dgt_encode): the codec expressions are the functions of
// wire_codec.h that k_quantize_4bit calls, and min/max do not depend on the
// order of the reduction.
//
// Work split (DgtShape). A lane owns float4 granules, a chunk is owned by a
// group of LPC lanes:
//   chunk   64 ..  512: LPC = chunk / 4 = 16 .. 128 lanes, one granule per
//                       lane, 16 .. 2 chunks per 256-thread workgroup;
//   chunk 1024 .. 8192: the whole workgroup, G = 1 .. 8 granules per lane,
//                       granule g = lane + j * 256 (coalesced per load).
// A chunk lives in registers from its loads to its stores: x and the
// residual are read once, 16 B per lane, and never staged in LDS.
//
// Order inside one trip of the grid-stride loop:
//   1. issue all loads of x and the residual (2 G float4 per lane);
//   2. locate the chunk in keep_idx. The loads come first because they do
//      not need the row. The compiler waits for them before the first probe
//      all the same (the join of the whole/partial load paths and the zero
//      test of contrib drain the load counter), so a trip is loads, then 3
//      probes; other waves hide that. A variant with no wait before the
//      first probe measured 4 % slower at chunk 1024 (docs/kernels.md);
//   3. min/max of f = x + residual: xor butterfly inside the group, every
//      lane ends with the result; where a chunk spans 2 or 4 waves the wave
//      results meet in LDS (8 B per wave, double-buffered by trip parity, so
//      one barrier per trip is enough);
//   4. kept: exact row and zero residual as float4; lossy: codes, residual,
//      codebook.
//
// Locate. r = lower_bound(keep_idx, c): kept iff keep_idx[r] == c (row r of
// `exact`), else lossy row c - r. The search is W-ary across the lanes of
// the group (W = min(LPC, 64)): per step lane j probes the last element of
// the j-th of W equal slices of the remaining range and the group counts,
// by ballot, how many probes are < c. n_keep = 32768 takes 3 dependent loads
// instead of 16. The remaining range is always closed by a probed element
// that is >= c (or by n_keep), so "some probe was == c" is the kept test and
// no further load follows the search. Rows are range-checked before they
// become addresses: a keep_idx that is not sorted and unique cannot send a
// store out of bounds, and with n_lossy == 0 no address is formed from the
// null `packed` and `minmax`.
//
// Code stores. A lane's granule is one 16-bit word of codes. Lanes 4i..4i+3
// pass their words to lane 4i with two quad-local DPP moves and that lane
// stores 8 B. Residual and exact rows go out as float4. The last chunk may
// be partial: positions at or past numel read as x = residual = 0 (they enter
// min/max and their codes are written, as the padded chain does) and no
// residual is written there.
//
// Conventions follow kernels.hip: wave64, <= GEOPS_MAX_BLOCKS workgroups of
// 256 threads, grid-stride, 64-bit element offsets, no atomics, no
// workspace, no host synchronisation. Built with the packed-fp32 feature off,
// as wirereduce.hip is (see setup.py and docs/kernels.md for what that
// changes: registers, not results).

#include <hip/hip_runtime.h>

#include <cstdint>
#include "wire_codec.h"

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048

template <int LOG2C>
struct DgtShape {
  static constexpr int CHUNK = 1 << LOG2C;
  static constexpr int GPC = CHUNK / 4;  // float4 granules per chunk
  static constexpr int LPC = GPC < GEOPS_THREADS ? GPC : GEOPS_THREADS;
  static constexpr int G = GPC / LPC;            // granules per lane
  static constexpr int CPW = GEOPS_THREADS / LPC;  // chunks per workgroup
  static constexpr int W = LPC < 64 ? LPC : 64;  // lanes of a group per wave
  static constexpr int WPC = LPC / W;            // waves per chunk
};

// DPP controls: quad_perm [1,0,3,2] and [2,3,0,1] are lane ^ 1 and lane ^ 2;
// the mirrors reverse 8 and 16 lanes, which pairs each lane with one of the
// other quad / the other half row, all a symmetric reduction needs.
#define DPP_XOR1 0xB1
#define DPP_XOR2 0x4E
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_ROW_MIRROR 0x140

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF,
                                               false);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v)));
}

// min and max over aligned groups of W lanes (16, 32 or 64) of a wave; every
// lane ends with the group's result. All lanes of the wave must be active.
template <int W>
__device__ __forceinline__ void group_minmax(float& mn, float& mx) {
  mn = fminf(mn, dpp_f32<DPP_XOR1>(mn));
  mx = fmaxf(mx, dpp_f32<DPP_XOR1>(mx));
  mn = fminf(mn, dpp_f32<DPP_XOR2>(mn));
  mx = fmaxf(mx, dpp_f32<DPP_XOR2>(mx));
  mn = fminf(mn, dpp_f32<DPP_ROW_HALF_MIRROR>(mn));
  mx = fmaxf(mx, dpp_f32<DPP_ROW_HALF_MIRROR>(mx));
  mn = fminf(mn, dpp_f32<DPP_ROW_MIRROR>(mn));
  mx = fmaxf(mx, dpp_f32<DPP_ROW_MIRROR>(mx));
  if constexpr (W >= 32) {
    mn = fminf(mn, __shfl_xor(mn, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  }
  if constexpr (W >= 64) {
    mn = fminf(mn, __shfl_xor(mn, 32, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  }
}

// 4 elements from e on; those at or past numel read as 0
__device__ __forceinline__ float4 load4_below(const float* __restrict__ p,
                                              long long e, long long numel) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (e < numel) v.x = p[e];
  if (e + 1 < numel) v.y = p[e + 1];
  if (e + 2 < numel) v.z = p[e + 2];
  if (e + 3 < numel) v.w = p[e + 3];
  return v;
}

__device__ __forceinline__ void store4_below(float* __restrict__ p,
                                             long long e, long long numel,
                                             const float4& v) {
  if (e < numel) p[e] = v.x;
  if (e + 1 < numel) p[e + 1] = v.y;
  if (e + 2 < numel) p[e + 2] = v.z;
  if (e + 3 < numel) p[e + 3] = v.w;
}

template <int LOG2C>
__global__ __launch_bounds__(GEOPS_THREADS) void k_dgt_encode(
    const float* __restrict__ x, float* __restrict__ residual,
    const float* __restrict__ contrib, const int* __restrict__ keep_idx,
    float* __restrict__ exact, uint8_t* __restrict__ packed,
    float* __restrict__ minmax, long long numel, int nchunks, int n_keep,
    int search_steps) {
  using S = DgtShape<LOG2C>;
  constexpr int G = S::G, LPC = S::LPC, W = S::W;
  __shared__ float2 wave_mm[2][GEOPS_THREADS / 64];

  const int lic = threadIdx.x & (LPC - 1);  // lane in chunk
  const int grp = threadIdx.x / LPC;        // chunk of this trip
  const int sub = threadIdx.x & (W - 1);    // lane in the group's wave part
  // the group's lanes within the wave's ballot
  const uint64_t gmask =
      W == 64 ? ~0ull : (((1ull << (W & 63)) - 1) << ((threadIdx.x & 63) - sub));
  const int n_lossy = nchunks - n_keep;
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

  // every lane of the workgroup runs every trip (the DPP moves, the ballots
  // and the barrier need all of them); a group past the last chunk loads
  // zeros, finds nothing and stores nothing
  int trip = 0;
  for (long long base = (long long)blockIdx.x * S::CPW; base < nchunks;
       base += (long long)gridDim.x * S::CPW, ++trip) {
    const long long cl = base + grp;
    const bool live = cl < nchunks;
    const int c = (int)cl;
    const long long e0 = cl << LOG2C;            // first element
    const bool whole = e0 + S::CHUNK <= numel;   // no position past numel

    // 1. all loads of the chunk
    float4 xv[G], rv[G];
    if (whole) {
      const float4* x4 = reinterpret_cast<const float4*>(x + e0);
      const float4* r4 = reinterpret_cast<const float4*>(residual + e0);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        xv[j] = x4[lic + j * LPC];
        rv[j] = r4[lic + j * LPC];
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const long long e = e0 + 4 * (lic + j * LPC);
        xv[j] = load4_below(x, e, numel);
        rv[j] = load4_below(residual, e, numel);
      }
    }
    const float cb = live ? contrib[c] : 1.0f;

    // 2. W-ary lower_bound of c in keep_idx, answer in [lb, lb + len]
    int lb = 0, len = live ? n_keep : 0;
    bool hit = false;
    for (int s = 0; s < search_steps; ++s) {
      const int span = (len + W - 1) / W;
      const int end = lb + len;
      const int p = lb + (sub + 1) * span - 1;
      int v = INT32_MAX;  // no chunk has this index
      if (len > 0 && p < end) v = keep_idx[p];  // lb <= p < lb + len
      const int below = __popcll(__ballot(v < c) & gmask);
      hit = hit || (__ballot(v == c) & gmask) != 0;
      lb += below * span;
      len = min(span - 1, end - lb);
      len = len < 0 ? 0 : len;
    }

    // 3. min/max of f = x + residual over the chunk
    float mn = 3.4e38f, mx = -3.4e38f;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float f0 = xv[j].x + rv[j].x, f1 = xv[j].y + rv[j].y;
      const float f2 = xv[j].z + rv[j].z, f3 = xv[j].w + rv[j].w;
      mn = fminf(fminf(fminf(mn, f0), f1), fminf(f2, f3));
      mx = fmaxf(fmaxf(fmaxf(mx, f0), f1), fmaxf(f2, f3));
    }
    group_minmax<W>(mn, mx);
    if constexpr (S::WPC > 1) {
      const int wave = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) wave_mm[trip & 1][wave] = make_float2(mn, mx);
      __syncthreads();
      const int first = wave & ~(S::WPC - 1);
#pragma unroll
      for (int w = 0; w < S::WPC; ++w) {
        const float2 m = wave_mm[trip & 1][first + w];
        mn = fminf(mn, m.x);
        mx = fmaxf(mx, m.y);
      }
    }
    if (!live) continue;

    // 4. stores
    const int r = lb;
    const bool dead = cb == 0.0f;
    if (hit) {
      if (r >= n_keep) continue;
      float4* ex4 = reinterpret_cast<float4*>(exact) + (long long)r * S::GPC;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int g = lic + j * LPC;
        // (a select of the two float4 lvalues would pin xv in scratch)
        ex4[g] = make_float4(dead ? 0.0f : xv[j].x, dead ? 0.0f : xv[j].y,
                             dead ? 0.0f : xv[j].z, dead ? 0.0f : xv[j].w);
        if (whole)
          reinterpret_cast<float4*>(residual + e0)[g] = zero4;
        else
          store4_below(residual, e0 + 4 * g, numel, zero4);
      }
    } else {
      const int l = c - r;
      if (l < 0 || l >= n_lossy) continue;
      const float lo = mn, hi = mx;
      const float step = step4(lo, hi);
      const float inv = 1.0f / step;
      uint2* pk8 = reinterpret_cast<uint2*>(packed + (long long)l * (S::CHUNK / 2));
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int g = lic + j * LPC;
        const float f[4] = {xv[j].x + rv[j].x, xv[j].y + rv[j].y,
                            xv[j].z + rv[j].z, xv[j].w + rv[j].w};
        float rout[4];
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t code = encode4(f[i], lo, inv);
          rout[i] = f[i] - decode4(code, lo, step);
          word |= code << (4 * i);
        }
        const float4 rn = make_float4(rout[0], rout[1], rout[2], rout[3]);
        if (whole)
          reinterpret_cast<float4*>(residual + e0)[g] = rn;
        else
          store4_below(residual, e0 + 4 * g, numel, rn);
        // the quad's four 16-bit words meet in its first lane
        const uint32_t pair = word | (dpp_u32<DPP_XOR1>(word) << 16);
        const uint32_t pair2 = dpp_u32<DPP_XOR2>(pair);
        if ((lic & 3) == 0) pk8[g >> 2] = make_uint2(pair, pair2);
      }
      if (lic == 0)
        reinterpret_cast<float2*>(minmax)[l] =
            dead ? make_float2(0.0f, 0.0f) : make_float2(lo, hi);
    }
  }
}

template <int LOG2C>
static void launch_dgt_encode(const float* x, float* residual,
                              const float* contrib, const int* keep_idx,
                              float* exact, uint8_t* packed, float* minmax,
                              long long numel, int nchunks, int n_keep,
                              hipStream_t s) {
  using S = DgtShape<LOG2C>;
  // trips of the W-ary search: a range of len shrinks to ceil(len / W) - 1
  int steps = 0;
  for (int len = n_keep; len > 0; len = (len + S::W - 1) / S::W - 1) ++steps;
  long long nb = ((long long)nchunks + S::CPW - 1) / S::CPW;
  if (nb > GEOPS_MAX_BLOCKS) nb = GEOPS_MAX_BLOCKS;
  hipLaunchKernelGGL((k_dgt_encode<LOG2C>), dim3((int)nb),
                     dim3(GEOPS_THREADS), 0, s, x, residual, contrib, keep_idx,
                     exact, packed, minmax, numel, nchunks, n_keep, steps);
}

extern "C" {

// chunk: a power of two in [64, 8192]; nchunks = ceil(numel / chunk) >= 1;
// keep_idx sorted ascending and unique. Returns -1 for a chunk outside the
// served range (the binding checks it first).
int geops_dgt_encode(const float* x, float* residual, const float* contrib,
                     const int* keep_idx, float* exact, uint8_t* packed,
                     float* minmax, long long numel, int chunk, int nchunks,
                     int n_keep, hipStream_t s) {
#define DGT_ENCODE_CASE(L)                                                   \
  case 1 << L:                                                               \
    launch_dgt_encode<L>(x, residual, contrib, keep_idx, exact, packed,      \
                         minmax, numel, nchunks, n_keep, s);                 \
    return 0;
  switch (chunk) {
    DGT_ENCODE_CASE(6)
    DGT_ENCODE_CASE(7)
    DGT_ENCODE_CASE(8)
    DGT_ENCODE_CASE(9)
    DGT_ENCODE_CASE(10)
    DGT_ENCODE_CASE(11)
    DGT_ENCODE_CASE(12)
    DGT_ENCODE_CASE(13)
  }
#undef DGT_ENCODE_CASE
  return -1;
}

}  // extern "C"
