// gfx950 (MI355X / CDNA4) fused wire reduce: the receive side of the
// compressed tiers. A leader or global server holds the all_gathered
// payloads of P parties; one kernel decodes all of them and writes
//
//   out[i] = (accumulate ? out[i] : +0.0f) + c_0[i] + c_1[i] + ... + c_{P-1}[i]
//
// in fp32, left to right in party order, every addition rounded. c_p[i] is
// party p's decoded value, decoded by the functions of wire_codec.h that the
// single-party kernels of kernels.hip use. Order and starting value are the
// interface: they make the result bit-equal to the chain
// `acc = zeros; for p: acc += decode(p)` that the call sites used to run.
//
// Party table. The payload base pointers travel BY VALUE in the kernel
// arguments (WireTab, at most WIRE_MAX_PARTIES = 16 pointers), so there is
// no table upload and nothing to keep alive. The kernels are templates on
// the number of parties NP of one launch: every table access is a constant
// index into the kernel-argument segment (a dynamic index would copy the
// table to scratch), and the per-party registers are plain arrays the
// compiler unrolls. The launcher serves P > 16 in groups of 16; every group
// after the first runs with accumulate = true. The fold is a left fold that
// starts from `out`, so the bits do not depend on the grouping.
//
// Memory-level parallelism is the design: a lane issues the loads of ALL
// parties of its group before it decodes the first one, so NP independent
// loads are in flight per lane (2 NP in the 2bit kernel, which works
// through two granules per trip). Nothing else is needed to stream: no
// atomics, no workspace, no LDS, no host synchronisation.
//
// Conventions follow kernels.hip: wave64, <= GEOPS_MAX_BLOCKS workgroups of
// 256 threads, grid-stride loops, 64-bit element offsets, float4 stores.
//
// This file is built without packed fp32 instructions (see setup.py).

#include <hip/hip_runtime.h>

#include <cstdint>
#include "wire_codec.h"

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048
#define WIRE_MAX_PARTIES 16

struct WireTab {
  const void* p[WIRE_MAX_PARTIES];
};

// the four tensors of a DGT mode-3 payload, per party
struct WireTabDgt {
  const float* exact[WIRE_MAX_PARTIES];
  const int* keep[WIRE_MAX_PARTIES];
  const uint16_t* packed[WIRE_MAX_PARTIES];
  const float* minmax[WIRE_MAX_PARTIES];
};

static inline int wire_blocks(long long work, int per_thread) {
  long long b = (work + (long long)GEOPS_THREADS * per_thread - 1) /
                ((long long)GEOPS_THREADS * per_thread);
  if (b < 1) b = 1;
  if (b > GEOPS_MAX_BLOCKS) b = GEOPS_MAX_BLOCKS;
  return (int)b;
}

__device__ __forceinline__ void add4(float4& a, const float4& c) {
  a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
}

// ---------------------------------------------------------------------------
// 2bit. Element mapping of k_dequantize_2bit: a lane owns the 4 consecutive
// elements of granule q, byte q & 3 of word q >> 2; the four lanes of a quad
// read the same word (one request) and the lane stores one float4. Two
// granules (q and q + stride) per trip: 2 NP word loads are issued before
// the first decode.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float4 decode2x4(uint32_t word, long long q,
                                            float thr) {
  const uint32_t byte = (word >> ((q & 3) * 8)) & 0xFFu;
  float4 o;
  o.x = decode2(byte & 3u, thr);
  o.y = decode2((byte >> 2) & 3u, thr);
  o.z = decode2((byte >> 4) & 3u, thr);
  o.w = decode2((byte >> 6) & 3u, thr);
  return o;
}

template <int NP>
__global__ __launch_bounds__(GEOPS_THREADS) void k_wire_sum_2bit(
    WireTab tab, float* __restrict__ out, long long n, float thr,
    bool accumulate) {
  const long long tid = (long long)blockIdx.x * GEOPS_THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * GEOPS_THREADS;
  const long long n4 = n >> 2;  // float4 granules fully inside n
  float4* out4 = reinterpret_cast<float4*>(out);
  for (long long q0 = tid; q0 < n4; q0 += 2 * stride) {
    // past the end the second granule repeats the first: the loads stay
    // unconditional and only its store is dropped
    const bool two = q0 + stride < n4;
    const long long q1 = two ? q0 + stride : q0;
    uint32_t w0[NP], w1[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const uint32_t* in = static_cast<const uint32_t*>(tab.p[p]);
      w0[p] = in[q0 >> 2];
      w1[p] = in[q1 >> 2];
    }
    float4 a0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a1 = a0;
    if (accumulate) {
      a0 = out4[q0];
      a1 = out4[q1];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      add4(a0, decode2x4(w0[p], q0, thr));
      add4(a1, decode2x4(w1[p], q1, thr));
    }
    out4[q0] = a0;
    if (two) out4[q1] = a1;
  }
  // scalar tail (n % 4 elements); unused slots of the last word hold code 0
  for (long long i = (n4 << 2) + tid; i < n; i += stride) {
    float a = accumulate ? out[i] : 0.0f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const uint32_t word = static_cast<const uint32_t*>(tab.p[p])[i >> 4];
      a += decode2((word >> ((i & 15) * 2)) & 3u, thr);
    }
    out[i] = a;
  }
}

// ---------------------------------------------------------------------------
// fp16 wire. A lane owns 8 elements: one 16 B granule per party, two float4
// stores. half -> float is exact (subnormal halves are normal floats). A
// payload that is a slice view need not start on a 16 B boundary; `vec` is
// false then and the whole call takes the scalar loop.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

template <int NP>
__global__ __launch_bounds__(GEOPS_THREADS) void k_wire_sum_f16(
    WireTab tab, float* __restrict__ out, long long n, bool vec,
    bool accumulate) {
  const long long tid = (long long)blockIdx.x * GEOPS_THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * GEOPS_THREADS;
  const long long n8 = vec ? (n >> 3) : 0;
  float4* out4 = reinterpret_cast<float4*>(out);
  for (long long q = tid; q < n8; q += stride) {
    uint4 h[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p)
      h[p] = static_cast<const uint4*>(tab.p[p])[q];
    float4 a0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a1 = a0;
    if (accumulate) {
      a0 = out4[2 * q];
      a1 = out4[2 * q + 1];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      a0.x += half_bits_to_float(h[p].x & 0xFFFFu);
      a0.y += half_bits_to_float(h[p].x >> 16);
      a0.z += half_bits_to_float(h[p].y & 0xFFFFu);
      a0.w += half_bits_to_float(h[p].y >> 16);
      a1.x += half_bits_to_float(h[p].z & 0xFFFFu);
      a1.y += half_bits_to_float(h[p].z >> 16);
      a1.z += half_bits_to_float(h[p].w & 0xFFFFu);
      a1.w += half_bits_to_float(h[p].w >> 16);
    }
    out4[2 * q] = a0;
    out4[2 * q + 1] = a1;
  }
  // scalar tail (n % 8 elements), or everything when !vec
  for (long long i = (n8 << 3) + tid; i < n; i += stride) {
    float a = accumulate ? out[i] : 0.0f;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      a += half_bits_to_float(static_cast<const uint16_t*>(tab.p[p])[i]);
    out[i] = a;
  }
}

// ---------------------------------------------------------------------------
// DGT mode 3. Per party the payload of DGTState.compress:
//   exact  f32 [n_keep][chunk]     keep_idx i32 [n_keep], sorted ascending
//   packed u8  [n_lossy][chunk/2]  minmax   f32 [n_lossy][2]
// One workgroup per chunk, grid-stride over chunks; chunk is a power of two
// >= 64 (the launcher passes log2(chunk / 4), the granules per chunk).
//
// Locate. keep_idx is sorted, so r = lower_bound(keep_idx, c) answers both
// questions at once: keep_idx[r] == c means chunk c is row r of `exact`;
// otherwise r kept chunks precede c, and c is lossy row c - r of `packed`
// and `minmax`. Every lane runs the same search (the addresses are uniform);
// the NP searches advance in lockstep, one probe per party per step, so a
// step costs one load latency, not NP. This replaces the receiver's mask,
// nonzero and row scatter: no index tensor is built and the host never
// waits. A keep_idx that is not sorted and unique can yield a lossy row
// outside [0, n_lossy); such a party contributes nothing to that chunk and
// the row is never turned into an address. With n_lossy == 0 no row is in
// range, so the null `packed` and `minmax` are never dereferenced.
//
// Sum. A lane owns granule g of the chunk: one float4 of `exact` for a
// party that kept it, one uint16 of codes for a party that did not. All NP
// loads are issued before the first decode. A dead chunk (minmax == (0, 0))
// decodes like any other, to ~1e-32. The last chunk may be partial: the
// payload rows are whole, `out` is written only below numel.
// ---------------------------------------------------------------------------

// where a party holds chunk c: row r of `exact` as r >= 0, lossy row l as
// -1 - l, nowhere as WIRE_SKIP
#define WIRE_SKIP INT32_MIN

template <int NP>
__global__ __launch_bounds__(GEOPS_THREADS) void k_wire_sum_dgt(
    WireTabDgt tab, float* __restrict__ out, long long numel, int nchunks,
    int n_keep, int log2g, int search_steps, bool accumulate) {
  const int gpc = 1 << log2g;  // float4 granules per chunk
  const int n_lossy = nchunks - n_keep;
  float4* out4 = reinterpret_cast<float4*>(out);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int lb[NP], ub[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) { lb[p] = 0; ub[p] = n_keep; }
    // search_steps = bit width of n_keep: enough to empty [lb, ub)
    for (int s = 0; s < search_steps; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (lb[p] < ub[p]) {
          const int mid = (lb[p] + ub[p]) >> 1;
          if (tab.keep[p][mid] < c) lb[p] = mid + 1; else ub[p] = mid;
        }
      }
    }
    int row[NP];
    float lo[NP], step[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = lb[p];
      const int l = c - r;
      row[p] = WIRE_SKIP;
      lo[p] = 0.0f; step[p] = 0.0f;
      if (r < n_keep && tab.keep[p][r] == c) {
        row[p] = r;
      } else if (l >= 0 && l < n_lossy) {
        row[p] = -1 - l;
        lo[p] = tab.minmax[p][2 * l];
        step[p] = step4(lo[p], tab.minmax[p][2 * l + 1]);
      }
    }
    for (int g = threadIdx.x; g < gpc; g += GEOPS_THREADS) {
      float4 raw[NP];  // kept: the values; lossy: .x holds the 4 codes
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        raw[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row[p] >= 0)
          raw[p] = reinterpret_cast<const float4*>(
              tab.exact[p])[((long long)row[p] << log2g) + g];
        else if (row[p] != WIRE_SKIP)
          raw[p].x = __uint_as_float(
              tab.packed[p][((long long)(-1 - row[p]) << log2g) + g]);
      }
      const long long q = ((long long)c << log2g) + g;
      const long long e = q << 2;
      const bool whole = e + 3 < numel;
      float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (accumulate) {
        if (whole) {
          a = out4[q];
        } else {
          if (e < numel) a.x = out[e];
          if (e + 1 < numel) a.y = out[e + 1];
          if (e + 2 < numel) a.z = out[e + 2];
        }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (row[p] >= 0) {
          add4(a, raw[p]);
        } else if (row[p] != WIRE_SKIP) {
          const uint32_t w = __float_as_uint(raw[p].x);
          float4 d;
          d.x = decode4(w & 0xFu, lo[p], step[p]);
          d.y = decode4((w >> 4) & 0xFu, lo[p], step[p]);
          d.z = decode4((w >> 8) & 0xFu, lo[p], step[p]);
          d.w = decode4((w >> 12) & 0xFu, lo[p], step[p]);
          add4(a, d);
        }
      }
      if (whole) {
        out4[q] = a;
      } else {
        if (e < numel) out[e] = a.x;
        if (e + 1 < numel) out[e + 1] = a.y;
        if (e + 2 < numel) out[e + 2] = a.z;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launchers: pick the instantiation for the group's party count.
// ---------------------------------------------------------------------------

template <int NP>
static void launch_2bit(int np, const WireTab& tab, float* out, long long n,
                        float thr, bool acc, hipStream_t s) {
  if (np == NP) {
    hipLaunchKernelGGL((k_wire_sum_2bit<NP>), dim3(wire_blocks(n >> 2, 2)),
                       dim3(GEOPS_THREADS), 0, s, tab, out, n, thr, acc);
  } else if constexpr (NP > 1) {
    launch_2bit<NP - 1>(np, tab, out, n, thr, acc, s);
  }
}

template <int NP>
static void launch_f16(int np, const WireTab& tab, float* out, long long n,
                       bool vec, bool acc, hipStream_t s) {
  if (np == NP) {
    hipLaunchKernelGGL((k_wire_sum_f16<NP>),
                       dim3(wire_blocks(vec ? (n >> 3) : n, 1)),
                       dim3(GEOPS_THREADS), 0, s, tab, out, n, vec, acc);
  } else if constexpr (NP > 1) {
    launch_f16<NP - 1>(np, tab, out, n, vec, acc, s);
  }
}

template <int NP>
static void launch_dgt(int np, const WireTabDgt& tab, float* out,
                       long long numel, int nchunks, int n_keep, int log2g,
                       int steps, bool acc, hipStream_t s) {
  if (np == NP) {
    const int nb = nchunks < GEOPS_MAX_BLOCKS ? nchunks : GEOPS_MAX_BLOCKS;
    hipLaunchKernelGGL((k_wire_sum_dgt<NP>), dim3(nb), dim3(GEOPS_THREADS), 0,
                       s, tab, out, numel, nchunks, n_keep, log2g, steps, acc);
  } else if constexpr (NP > 1) {
    launch_dgt<NP - 1>(np, tab, out, numel, nchunks, n_keep, log2g, steps,
                       acc, s);
  }
}

extern "C" {

// payloads: P device pointers (host array). Groups of WIRE_MAX_PARTIES.
void geops_wire_sum_2bit(const void* const* payloads, int P, float* out,
                         long long n, float thr, bool accumulate,
                         hipStream_t s) {
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    WireTab tab = {};
    for (int j = 0; j < np; ++j) tab.p[j] = payloads[p0 + j];
    launch_2bit<WIRE_MAX_PARTIES>(np, tab, out, n, thr,
                                  accumulate || p0 > 0, s);
  }
}

void geops_wire_sum_f16(const void* const* payloads, int P, float* out,
                        long long n, bool accumulate, hipStream_t s) {
  bool vec = true;
  for (int p = 0; p < P; ++p) vec = vec && ((uintptr_t)payloads[p] & 15) == 0;
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    WireTab tab = {};
    for (int j = 0; j < np; ++j) tab.p[j] = payloads[p0 + j];
    launch_f16<WIRE_MAX_PARTIES>(np, tab, out, n, vec, accumulate || p0 > 0,
                                 s);
  }
}

// chunk: a power of two >= 64 (checked by the binding)
void geops_wire_sum_dgt(const float* const* exacts, const int* const* keeps,
                        const uint8_t* const* packeds,
                        const float* const* minmaxs, int P, float* out,
                        long long numel, int chunk, int nchunks, int n_keep,
                        bool accumulate, hipStream_t s) {
  int log2g = 0;
  while ((4 << log2g) < chunk) ++log2g;
  int steps = 0;
  while ((n_keep >> steps) != 0) ++steps;
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    WireTabDgt tab = {};
    for (int j = 0; j < np; ++j) {
      tab.exact[j] = exacts[p0 + j];
      tab.keep[j] = keeps[p0 + j];
      tab.packed[j] = reinterpret_cast<const uint16_t*>(packeds[p0 + j]);
      tab.minmax[j] = minmaxs[p0 + j];
    }
    launch_dgt<WIRE_MAX_PARTIES>(np, tab, out, numel, nchunks, n_keep, log2g,
                                 steps, accumulate || p0 > 0, s);
  }
}

}  // extern "C"
