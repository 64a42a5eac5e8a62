// Layer-wise LARS server update (LBSGD, warmup_strategy='lars') over a flat
// fp32 bucket cut into S segments (one per layer) by the device table
// seg_off[S+1]. Three launches, no host wait between them:
//
//   k_lars_sumsq   one pass over w and g: the pair (sum w^2, sum g^2) of
//                  every tile
//   k_lars_ratio   one small block per segment: the tiles' pairs summed in
//                  double, ratio[s] = clamp(sqrt(W2 / (G2 + wd W2 + 1e-18)),
//                  0.01, 100)
//   k_lars_update  the sgd / sgd-momentum rule of optim_rules.h with
//                  lr * ratio[segment] * lbmult as its rate
//
// Work split. The unit is a TILE of 4096 consecutive elements of ONE segment
// (256 threads x 16 elements: 4 granules of 16 B per thread and operand at
// VEC = 4, 16 single floats at VEC = 1); a tile never crosses a segment
// boundary, segment s has ceil(len_s / TILE) tiles, and tile_start[S+1] is
// their prefix sum (built on the host, cached on the device by ops). A block
// walks the tiles grid-stride and finds a tile's segment with a block-uniform
// binary search over tile_start, started at the segment of its previous tile.
// Within a tile granule j of thread t is elements (j * 256 + t) * VEC ..., so
// a wave reads 1 KiB (VEC = 4) of consecutive memory per access.
//
// The sums are reproducible: there is no floating-point atomic, and every
// addition happens in an order fixed by (seg_off, TILE) alone.
//   1. a thread folds its 16 squares into one fp32 accumulator with fmaf, in
//      element order (elements past the end of a partial tile enter as 0);
//   2. a wave sums its 64 accumulators with a 6-step xor butterfly (a + b is
//      commutative bit for bit, so every lane holds the same sum);
//   3. thread 0 adds the four waves' sums in wave order and writes the pair
//      (sum w^2, sum g^2) to partials[tile];
//   4. k_lars_ratio sums a segment's partials in double: thread t takes
//      tiles t, t + 256, ... in ascending order, then a fixed 256 -> 1 tree
//      in LDS.
// The longest chain of fp32 roundings an element passes through is
// 1 (square) + 15 (thread) + 6 (butterfly) + 3 (waves) = 25.
//
// The ratio has a launch of its own. The form in which the block that
// finishes a segment's last outstanding tile computes the ratio (a fence
// and one integer atomicAdd on a per-segment counter per tile) was built
// first and gave the same bits, but ran the pass at 0.59 TB/s at 64M
// elements: the agent-scope release fence after each tile's partial is an
// L2 write-back on this part, whose XCDs have an L2 each (docs/kernels.md).
//
// Empty segments have no tile: their sums are 0 and their ratio 0.01.
//
// Built without packed fp32 instructions (setup.py), like every file here
// whose sums are specified one rounded operation at a time.

#include <hip/hip_runtime.h>

#include "geops_grid.h"
#include "optim_rules.h"

#define LARS_TILE 4096
#define LARS_PER_THREAD (LARS_TILE / GEOPS_THREADS)
#define LARS_WAVES (GEOPS_THREADS / 64)

namespace {

// One tile of the walk: elements [base, base + len) of segment seg.
struct LarsTile {
  long long base;
  int len;
};

// Segment of tile t: the s with tile_start[s] <= t < tile_start[s+1] (empty
// segments repeat a value and are never the answer). `seg` is the segment
// of the block's previous tile, or 0; tiles only move forward. Everything
// here is block-uniform, so the table reads are scalar loads. `n` bounds
// the tile once more: no address leaves the operands whatever the tables say.
__device__ __forceinline__ LarsTile lars_tile(
    const long long* __restrict__ seg_off,
    const long long* __restrict__ tile_start, int S, long long n, long long t,
    int& seg) {
  if (t >= tile_start[seg + 1]) {
    int lo = seg + 1, hi = S;  // tile_start[lo] <= t < tile_start[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= t) lo = mid; else hi = mid;
    }
    seg = lo;
  }
  LarsTile tl;
  tl.base = seg_off[seg] + (t - tile_start[seg]) * LARS_TILE;
  long long end = seg_off[seg + 1];
  if (end > n) end = n;
  long long len = end - tl.base;
  if (tl.base < 0 || len < 0) len = 0;
  tl.len = len < LARS_TILE ? (int)len : LARS_TILE;
  return tl;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

template <int VEC>
__global__ __launch_bounds__(GEOPS_THREADS) void k_lars_sumsq(
    const float* __restrict__ w, const float* __restrict__ g,
    const long long* __restrict__ seg_off,
    const long long* __restrict__ tile_start,
    float2* __restrict__ partials, int S, long long total, long long n) {
  __shared__ float s_wave[2][LARS_WAVES];
  const int tid = threadIdx.x;
  constexpr int NG = LARS_PER_THREAD / VEC;
  int seg = 0;
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const LarsTile tl = lars_tile(seg_off, tile_start, S, n, t, seg);
    // all loads first, so that they are in flight together
    Granule<VEC> wv[NG], gv[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int off = (j * GEOPS_THREADS + tid) * VEC;
      if (off < tl.len) {   // len is a multiple of VEC: whole granules
        wv[j].load(w + tl.base + off);
        gv[j].load(g + tl.base + off);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) wv[j].v[v] = gv[j].v[v] = 0.0f;
      }
    }
    float sw = 0.0f, sg = 0.0f;
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        sw = fmaf(wv[j].v[v], wv[j].v[v], sw);
        sg = fmaf(gv[j].v[v], gv[j].v[v], sg);
      }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    if ((tid & 63) == 0) {
      s_wave[0][tid >> 6] = sw;
      s_wave[1][tid >> 6] = sg;
    }
    __syncthreads();
    if (tid == 0) {
      float a = s_wave[0][0], b = s_wave[1][0];
#pragma unroll
      for (int k = 1; k < LARS_WAVES; ++k) {
        a += s_wave[0][k];
        b += s_wave[1][k];
      }
      partials[t] = make_float2(a, b);
    }
    __syncthreads();   // s_wave is free for the next tile
  }
}

// block s: segment s
__global__ __launch_bounds__(GEOPS_THREADS) void k_lars_ratio(
    const float2* __restrict__ partials,
    const long long* __restrict__ tile_start, float* __restrict__ ratio,
    double wd) {
  __shared__ double s_red[2][GEOPS_THREADS];
  const int tid = threadIdx.x, seg = blockIdx.x;
  const long long t0 = tile_start[seg];
  const int ntiles = (int)(tile_start[seg + 1] - t0);
  double dw = 0.0, dg = 0.0;
#pragma unroll 4
  for (int i = tid; i < ntiles; i += GEOPS_THREADS) {
    const float2 p = partials[t0 + i];
    dw += (double)p.x;
    dg += (double)p.y;
  }
  s_red[0][tid] = dw;
  s_red[1][tid] = dg;
  __syncthreads();
  for (int h = GEOPS_THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      s_red[0][tid] += s_red[0][tid + h];
      s_red[1][tid] += s_red[1][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double W2 = s_red[0][0], G2 = s_red[1][0];
    double r = sqrt(W2 / (G2 + wd * W2 + 1e-18));
    if (r < 0.01) r = 0.01; else if (r > 100.0) r = 100.0;
    ratio[seg] = (float)r;
  }
}

template <typename RULE>
OPTIM_FN RULE lars_rule(float lr, float momentum, float wd, float rescale);
template <>
OPTIM_FN SgdRule lars_rule<SgdRule>(float lr, float, float wd,
                                    float rescale) {
  return SgdRule{lr, wd, rescale};
}
template <>
OPTIM_FN SgdMomRule lars_rule<SgdMomRule>(float lr, float momentum, float wd,
                                          float rescale) {
  return SgdMomRule{lr, momentum, wd, rescale};
}

template <int VEC, typename RULE>
__global__ __launch_bounds__(GEOPS_THREADS) void k_lars_update(
    float* __restrict__ w, const float* __restrict__ g,
    float* __restrict__ mom, const long long* __restrict__ seg_off,
    const long long* __restrict__ tile_start,
    const float* __restrict__ ratio, int S, long long total, long long n,
    double lr, double lbmult, float momentum, float wd, float rescale) {
  constexpr int NG = LARS_PER_THREAD / VEC;
  const int tid = threadIdx.x;
  int seg = 0;
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const LarsTile tl = lars_tile(seg_off, tile_start, S, n, t, seg);
    const RULE op = lars_rule<RULE>(
        (float)(lr * (double)ratio[seg] * lbmult), momentum, wd, rescale);
    // all loads, then the rule, then all stores: a thread keeps its 4
    // granules per operand in flight together. w is loaded before g, as
    // in optim_apply.
    Granule<VEC> wv[NG], mv[NG], gv[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const long long off = tl.base + (j * GEOPS_THREADS + tid) * VEC;
      if (off < tl.base + tl.len) {
        wv[j].load(w + off);
        if (RULE::NSTATE >= 1) mv[j].load(mom + off);
        gv[j].load(g + off);
      }
    }
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        op.apply(wv[j].v[v], gv[j].v[v], mv[j].v[v], mv[j].v[v]);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const long long off = tl.base + (j * GEOPS_THREADS + tid) * VEC;
      if (off < tl.base + tl.len) {
        wv[j].store(w + off);
        if (RULE::NSTATE >= 1) mv[j].store(mom + off);
      }
    }
  }
}

// n_wg > 0 is the test hook; 0 is one block per tile up to the cap
inline int lars_grid(long long total, int n_wg) {
  return n_wg > 0 ? n_wg : geops_blocks(total * GEOPS_THREADS);
}

}  // namespace

extern "C" {

int geops_lars_tile() { return LARS_TILE; }

// vec: 4 when every seg_off entry is a multiple of 4 and w, g (and mom) are
// 16 B aligned, else 1. partials holds 2 * total floats. S >= 1.
void geops_lars_sumsq(const float* w, const float* g,
                      const long long* seg_off, const long long* tile_start,
                      float* partials, float* ratio, int S, long long total,
                      long long n, double wd, int vec, int n_wg,
                      hipStream_t s) {
  const dim3 grid(lars_grid(total, n_wg)), block(GEOPS_THREADS);
  float2* part = reinterpret_cast<float2*>(partials);
  if (total > 0) {
    if (vec == 4)
      hipLaunchKernelGGL(k_lars_sumsq<4>, grid, block, 0, s, w, g, seg_off,
                         tile_start, part, S, total, n);
    else
      hipLaunchKernelGGL(k_lars_sumsq<1>, grid, block, 0, s, w, g, seg_off,
                         tile_start, part, S, total, n);
  }
  hipLaunchKernelGGL(k_lars_ratio, dim3(S), block, 0, s, part, tile_start,
                     ratio, wd);
}

// mom == nullptr is plain sgd (SgdRule), else sgd with momentum (SgdMomRule)
void geops_lars_update(float* w, const float* g, float* mom,
                       const long long* seg_off, const long long* tile_start,
                       const float* ratio, int S, long long total,
                       long long n, double lr, double lbmult, float momentum,
                       float wd, float rescale, int vec, int n_wg,
                       hipStream_t s) {
  const dim3 grid(lars_grid(total, n_wg)), block(GEOPS_THREADS);
#define LARS_UPDATE(VEC_, RULE_)                                            \
  hipLaunchKernelGGL((k_lars_update<VEC_, RULE_>), grid, block, 0, s, w, g, \
                     mom, seg_off, tile_start, ratio, S, total, n, lr,      \
                     lbmult, momentum, wd, rescale)
  if (mom != nullptr) {
    if (vec == 4) LARS_UPDATE(4, SgdMomRule); else LARS_UPDATE(1, SgdMomRule);
  } else {
    if (vec == 4) LARS_UPDATE(4, SgdRule); else LARS_UPDATE(1, SgdRule);
  }
#undef LARS_UPDATE
}

}  // extern "C"
