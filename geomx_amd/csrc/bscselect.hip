// Bi-Sparse boundary select for gfx950: the exact k-th largest of S sampled
// fp32 magnitudes, written as one device float (the boundary k_bsc_fused
// reads). Replaces the gather / multiply / add / abs / topk / slice / clone
// op chain of the sampled boundary prediction.
//
// Key of sample position i = si[j]:
//     c   = v[i] + bsc_mom(u[i], mu, g[i])      (with g and u; v[i] alone
//     key = bits(c) & 0x7fffffff                  without them)
// Keys compare as unsigned integers: the order of |c|, NaN above inf as
// torch.topk has it. The result is the float whose bits are the k-th largest
// key: a value, so ties need no rule.
//
// MSB-first radix select, digits of 11 / 11 / 9 bits (bits 30..20 = exponent
// and 3 mantissa bits, 19..9, 8..0): per digit an LDS histogram (LDS atomics),
// a block-wide suffix scan from the top bin for the bin that holds rank k,
// then only the keys of that bin go on.
//
// Two forms, neither waits on another workgroup:
//   one  (k_bsc_boundary_one, 1 workgroup of 1024): S <= 32768. Keys are
//        gathered straight into 128 KB of LDS, survivors of each digit are
//        compacted in place.
//   many (k_bsc_boundary_many, G workgroups of 1024): each gathers a
//        contiguous slice of si, writes its keys coalesced to a uint32[S]
//        workspace, histograms the top digit in LDS and flushes the non-empty
//        bins with global integer atomics; agent-scope release, then a ticket.
//        The workgroup that draws the last ticket acquires and finishes alone:
//        suffix scan of the global histogram, then the keys of the chosen bin
//        are either compacted from the workspace into LDS (<= 8192 of them)
//        and resolved there, or, when more share the bin (S equal keys all
//        do), resolved by prefix-filtered histogram passes over the
//        workspace. Every other workgroup exits; nothing spins.
//
// Sample positions are clamped into [0, n), so no address leaves the
// operands whatever si holds.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include "bsc_mom.h"

#define BSCSEL_NT 1024       // threads per workgroup, both forms
#define BSCSEL_NB 2048       // bins of the widest digit
#define BSCSEL_U 4           // loads in flight per thread and operand
#define BSCSEL_CAP1 32768    // keys form one holds in LDS (128 KB)
#define BSCSEL_CAND 8192     // candidate keys form many resolves in LDS
#define BSCSEL_WS_HEAD 2052  // uint32 words in front of the workspace keys:
                             // 2048 bins, the ticket, pad to 16 B
#define BSCSEL_SWITCH 4096   // largest S the launcher gives to form one
#define BSCSEL_MAX_WG 128    // most workgroups the launcher gives form many

namespace {

struct SelScratch {
  unsigned wsum[BSCSEL_NT / 64];
  unsigned d, k, c;  // chosen bin, rank inside it, its count
  unsigned cursor;
  unsigned last;
};

__device__ __forceinline__ int digit_shift(int p) {
  return p == 0 ? 20 : p == 1 ? 9 : 0;
}
__device__ __forceinline__ int digit_bits(int p) { return p == 2 ? 9 : 11; }

// Keys of up to U samples per thread, positions [base, hi) of si strided by
// the workgroup. All of a thread's loads are issued before the first use.
template <bool MOM>
__device__ __forceinline__ void gather_keys(
    const float* __restrict__ v, const float* __restrict__ g,
    const float* __restrict__ u, const int* __restrict__ si, float mu,
    unsigned n, unsigned base, unsigned hi, uint32_t (&key)[BSCSEL_U]) {
  unsigned p[BSCSEL_U];
#pragma unroll
  for (int j = 0; j < BSCSEL_U; ++j) {
    const unsigned i = base + j * BSCSEL_NT + threadIdx.x;
    p[j] = i < hi ? min((unsigned)si[i], n - 1) : 0u;
  }
  float vv[BSCSEL_U], gg[BSCSEL_U], uu[BSCSEL_U];
#pragma unroll
  for (int j = 0; j < BSCSEL_U; ++j) {
    vv[j] = v[p[j]];
    if (MOM) {
      gg[j] = g[p[j]];
      uu[j] = u[p[j]];
    }
  }
#pragma unroll
  for (int j = 0; j < BSCSEL_U; ++j) {
    const float c = MOM ? vv[j] + bsc_mom(uu[j], mu, gg[j]) : vv[j];
    key[j] = __float_as_uint(c) & 0x7fffffffu;
  }
}

// One round of a sweep over keys[0, m): U 16 B vectors per thread. Slots at
// or past m come back as 0xffffffff, which no prefix filter accepts (a key
// has bit 31 clear). keys must be 16 B aligned and readable up to the next
// multiple of 4.
__device__ __forceinline__ void load_round(const uint32_t* keys, unsigned m,
                                           unsigned base4,
                                           uint32_t (&q)[BSCSEL_U][4]) {
  const uint4* k4 = reinterpret_cast<const uint4*>(keys);
  const unsigned m4 = (m + 3) >> 2;
#pragma unroll
  for (int j = 0; j < BSCSEL_U; ++j) {
    const unsigned i4 = base4 + j * BSCSEL_NT + threadIdx.x;
    uint4 t = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (i4 < m4) t = k4[i4];
    const unsigned e = i4 * 4;
    q[j][0] = e < m ? t.x : ~0u;
    q[j][1] = e + 1 < m ? t.y : ~0u;
    q[j][2] = e + 2 < m ? t.z : ~0u;
    q[j][3] = e + 3 < m ? t.w : ~0u;
  }
}

// hist[d] += 1 for every lane with `match`, called by whole waves. The lanes
// that share the first matching lane's digit are counted with one ballot and
// added once: LDS atomics of one wave to one address run one after another,
// and a sample of equal keys (a bucket of zeros) would put all 64 there.
__device__ __forceinline__ void hist_add(unsigned* hist, bool match,
                                         unsigned d) {
  const unsigned long long mm = __ballot(match);
  if (mm == 0) return;  // wave-uniform
  const int leader = __ffsll((long long)mm) - 1;
  const unsigned d0 = __shfl(d, leader, 64);
  const unsigned long long same = __ballot(match && d == d0);
  if (match) {
    if (d != d0)
      atomicAdd(&hist[d], 1u);
    else if ((int)(threadIdx.x & 63) == leader)
      atomicAdd(&hist[d0], (unsigned)__popcll(same));
  }
}

// hist[digit] += 1 for every key of keys[0, m) whose bits above the digit
// equal `prefix`. hist must be zero on entry; the caller synchronizes.
__device__ __forceinline__ void block_hist(const uint32_t* keys, unsigned m,
                                           int p, uint32_t prefix,
                                           unsigned* hist) {
  const int shift = digit_shift(p), hi = shift + digit_bits(p);
  const uint32_t dmask = (1u << digit_bits(p)) - 1u;
  const unsigned m4 = (m + 3) >> 2;
  for (unsigned base4 = 0; base4 < m4; base4 += BSCSEL_NT * BSCSEL_U) {
    uint32_t q[BSCSEL_U][4];
    load_round(keys, m, base4, q);
#pragma unroll
    for (int j = 0; j < BSCSEL_U; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        hist_add(hist, (q[j][e] >> hi) == prefix,
                 (q[j][e] >> shift) & dmask);
  }
}

// Suffix scan of hist from the top bin: s.d = the bin that holds rank k
// (counting from the largest key), s.k = the rank inside that bin, s.c = its
// count. Needs 1 <= k <= sum(hist). Leaves hist zero.
__device__ __forceinline__ void block_select(unsigned* hist, unsigned k,
                                             SelScratch& s) {
  constexpr int BPT = BSCSEL_NB / BSCSEL_NT;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned c[BPT], tsum = 0;
#pragma unroll
  for (int b = 0; b < BPT; ++b) {
    c[b] = hist[threadIdx.x * BPT + b];
    hist[threadIdx.x * BPT + b] = 0;
    tsum += c[b];
  }
  unsigned x = tsum;  // inclusive suffix sum over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned y = __shfl_down(x, off, 64);
    if (lane + off < 64) x += y;
  }
  if (lane == 0) s.wsum[wid] = x;
  __syncthreads();
  unsigned above = x - tsum;  // keys in bins above this thread's
  for (int w = wid + 1; w < BSCSEL_NT / 64; ++w) above += s.wsum[w];
#pragma unroll
  for (int b = BPT - 1; b >= 0; --b) {
    if (above < k && k <= above + c[b]) {
      s.d = threadIdx.x * BPT + b;
      s.k = k - above;
      s.c = c[b];
    }
    above += c[b];
  }
  __syncthreads();
}

// dst[0, count) = the keys of src[0, m) with (key >> shift) == want, in any
// order; returns count (at most cap, the room of dst). INPLACE (dst == src,
// in LDS): a round's writes land below the positions the round has read, and
// every thread has read before any writes, so no unread key is overwritten.
template <bool INPLACE>
__device__ __forceinline__ unsigned block_compact(const uint32_t* src,
                                                  unsigned m, int shift,
                                                  uint32_t want, uint32_t* dst,
                                                  unsigned cap,
                                                  SelScratch& s) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s.cursor = 0;
  __syncthreads();
  const unsigned m4 = (m + 3) >> 2;
  for (unsigned base4 = 0; base4 < m4; base4 += BSCSEL_NT * BSCSEL_U) {
    uint32_t q[BSCSEL_U][4];
    load_round(src, m, base4, q);
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < BSCSEL_U; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) cnt += (q[j][e] >> shift) == want;
    if (INPLACE) __syncthreads();
    unsigned incl = cnt;  // inclusive prefix over the wave's lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    unsigned wbase = 0;
    if (lane == 63 && incl) wbase = atomicAdd(&s.cursor, incl);
    unsigned pos = __shfl(wbase, 63, 64) + incl - cnt;
#pragma unroll
    for (int j = 0; j < BSCSEL_U; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((q[j][e] >> shift) == want) {
          if (pos < cap) dst[pos] = q[j][e];
          ++pos;
        }
  }
  __syncthreads();
  const unsigned count = min(s.cursor, cap);
  __syncthreads();
  return count;
}

// Digits p0..2 of the rank-k key among the keys of keys[0, m) that carry
// `prefix` above digit p0. COMPACT: keys is an LDS list that already holds
// only such keys and is compacted in place after each digit; otherwise keys
// is swept whole with the prefix filter. hist must be zero on entry.
template <bool COMPACT>
__device__ __forceinline__ uint32_t radix_finish(uint32_t* keys, unsigned m,
                                                 unsigned k, int p0,
                                                 uint32_t prefix,
                                                 unsigned* hist,
                                                 SelScratch& s) {
  for (int p = p0; p < 3; ++p) {
    block_hist(keys, m, p, prefix, hist);
    __syncthreads();
    block_select(hist, k, s);
    prefix = (prefix << digit_bits(p)) | s.d;
    k = s.k;
    if (COMPACT && p < 2)
      m = block_compact<true>(keys, m, digit_shift(p), prefix, keys, m, s);
  }
  return prefix;
}

}  // namespace

template <bool MOM>
__global__ __launch_bounds__(BSCSEL_NT) void k_bsc_boundary_one(
    const float* __restrict__ v, const float* __restrict__ g,
    const float* __restrict__ u, const int* __restrict__ si, unsigned S,
    unsigned k, unsigned n, float mu, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t keys[BSCSEL_CAP1];
  __shared__ unsigned hist[BSCSEL_NB];
  __shared__ SelScratch s;
  for (int b = threadIdx.x; b < BSCSEL_NB; b += BSCSEL_NT) hist[b] = 0;
  for (unsigned base = 0; base < S; base += BSCSEL_NT * BSCSEL_U) {
    uint32_t key[BSCSEL_U];
    gather_keys<MOM>(v, g, u, si, mu, n, base, S, key);
#pragma unroll
    for (int j = 0; j < BSCSEL_U; ++j) {
      const unsigned i = base + j * BSCSEL_NT + threadIdx.x;
      if (i < S) keys[i] = key[j];
    }
  }
  __syncthreads();
  const uint32_t r = radix_finish<true>(keys, S, k, 0, 0u, hist, s);
  if (threadIdx.x == 0) *out = __uint_as_float(r);
}

template <bool MOM>
__global__ __launch_bounds__(BSCSEL_NT) void k_bsc_boundary_many(
    const float* __restrict__ v, const float* __restrict__ g,
    const float* __restrict__ u, const int* __restrict__ si, unsigned S,
    unsigned k, unsigned n, float mu, float* __restrict__ out,
    uint32_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) uint32_t cand[BSCSEL_CAND];
  __shared__ unsigned hist[BSCSEL_NB];
  __shared__ SelScratch s;
  unsigned* ghist = ws;
  unsigned* ticket = ws + BSCSEL_NB;
  uint32_t* gkeys = ws + BSCSEL_WS_HEAD;
  for (int b = threadIdx.x; b < BSCSEL_NB; b += BSCSEL_NT) hist[b] = 0;
  __syncthreads();

  // ---- every workgroup: gather a slice, keys out, top-digit histogram ----
  const unsigned slice = (S + gridDim.x - 1) / gridDim.x;
  const unsigned lo = min(S, blockIdx.x * slice);
  const unsigned hi = min(S, lo + slice);
  for (unsigned base = lo; base < hi; base += BSCSEL_NT * BSCSEL_U) {
    uint32_t key[BSCSEL_U];
    gather_keys<MOM>(v, g, u, si, mu, n, base, hi, key);
#pragma unroll
    for (int j = 0; j < BSCSEL_U; ++j) {
      const unsigned i = base + j * BSCSEL_NT + threadIdx.x;
      if (i < hi) gkeys[i] = key[j];
      hist_add(hist, i < hi, key[j] >> digit_shift(0));
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BSCSEL_NB; b += BSCSEL_NT) {
    const unsigned c = hist[b];
    hist[b] = 0;
    if (c)
      __hip_atomic_fetch_add(&ghist[b], c, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  // release this thread's keys and bin counts to the agent (another XCD's
  // workgroup may finish), then one ticket per workgroup
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL,
                                              __HIP_MEMORY_SCOPE_AGENT);
    s.last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!s.last) return;

  // ---- last ticket: finish alone ------------------------------------------
  __threadfence();  // acquire what every other workgroup released
  for (int b = threadIdx.x; b < BSCSEL_NB; b += BSCSEL_NT)
    hist[b] = __hip_atomic_load(&ghist[b], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  block_select(hist, k, s);
  const uint32_t d0 = s.d;
  const unsigned k0 = s.k, c0 = s.c;
  uint32_t r;
  if (c0 <= BSCSEL_CAND) {
    const unsigned m =
        block_compact<false>(gkeys, S, digit_shift(0), d0, cand,
                             BSCSEL_CAND, s);
    r = radix_finish<true>(cand, m, k0, 1, d0, hist, s);
  } else {
    r = radix_finish<false>(gkeys, S, k0, 1, d0, hist, s);
  }
  if (threadIdx.x == 0) *out = __uint_as_float(r);
}

extern "C" {

int geops_bsc_boundary_cap() { return BSCSEL_CAP1; }

// Workgroups a call runs on: 1 = form one, >= 2 = form many, -1 = n_wg asks
// for form one and S is over its capacity. n_wg 0 chooses.
int geops_bsc_boundary_grid(long long S, int n_wg) {
  if (n_wg == 1) return S <= BSCSEL_CAP1 ? 1 : -1;
  if (n_wg >= 2) return n_wg;
  if (S <= BSCSEL_SWITCH) return 1;
  // the gather costs S / G per workgroup, the histogram flush G workgroups'
  // atomics on the same few bins: least near G ~ sqrt(S) (measured, /8)
  int G = (int)(sqrt((double)S) / 8.0 + 0.5);
  if (G < 2) G = 2;
  if (G > BSCSEL_MAX_WG) G = BSCSEL_MAX_WG;
  return G;
}

// uint32 words of workspace form many needs (keys rounded up to 16 B)
long long geops_bsc_boundary_ws_words(long long S) {
  return BSCSEL_WS_HEAD + ((S + 3) & ~3LL);
}

// grid: what geops_bsc_boundary_grid returned. g and u are both null for the
// |v|-only key. ws is used by form many only; its head (histogram, ticket)
// is zeroed here on the stream, so calls are independent.
void geops_bsc_boundary(const float* v, const float* g, const float* u,
                        const int* si, long long S, long long k, long long n,
                        float mu, float* out, uint32_t* ws, int grid,
                        hipStream_t s) {
  const unsigned S_ = (unsigned)S, k_ = (unsigned)k, n_ = (unsigned)n;
  if (grid == 1) {
    if (g)
      hipLaunchKernelGGL(k_bsc_boundary_one<true>, dim3(1), dim3(BSCSEL_NT),
                         0, s, v, g, u, si, S_, k_, n_, mu, out);
    else
      hipLaunchKernelGGL(k_bsc_boundary_one<false>, dim3(1), dim3(BSCSEL_NT),
                         0, s, v, g, u, si, S_, k_, n_, mu, out);
    return;
  }
  (void)hipMemsetAsync(ws, 0, BSCSEL_WS_HEAD * sizeof(uint32_t), s);
  if (g)
    hipLaunchKernelGGL(k_bsc_boundary_many<true>, dim3(grid),
                       dim3(BSCSEL_NT), 0, s, v, g, u, si, S_, k_, n_, mu,
                       out, ws);
  else
    hipLaunchKernelGGL(k_bsc_boundary_many<false>, dim3(grid),
                       dim3(BSCSEL_NT), 0, s, v, g, u, si, S_, k_, n_, mu,
                       out, ws);
}

}  // extern "C"
