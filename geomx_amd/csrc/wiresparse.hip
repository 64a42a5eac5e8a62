// gfx950 (MI355X / CDNA4) fused Bi-Sparse wire reduce: the receive side of
// the sparse tiers (bsc, mpq, bsc_dgt). A leader or global server holds the
// all_gathered lists of P parties; one kernel turns them into the dense sum
//
//   out[i] = (accumulate ? out[i] : +0.0f) + c_0[i] + c_1[i] + ... + c_{P-1}[i]
//
// in fp32, left to right in party order, every addition rounded. c_p[i] is
// the value of party p's entry with index i, nothing if p has none. It is the
// contract of the wire_sum_* kernels of wirereduce.hip, and it makes the
// result bit-equal to the chain the call sites used to run: `acc = zeros`,
// then per party a scatter-add of its list (k_bsc_unpack).
//
// A party's list is `k` slots of (value, index i32), in ascending index
// order with the placeholders (index -1) last: every packer writes it so
// (k_bsc_fused, k_bsc_pack, k_bsc_pull_pack). Indices compare as UNSIGNED
// here, so the placeholders and any index >= n sort behind every output
// element and no party needs a separate length. For a list that breaks the
// order the values of the result are unspecified, but every address stays
// inside the operands: search results are clamped to [0, k], an index is
// range-checked against the tile before it becomes an LDS address, and a
// DGT row is range-checked before it becomes a global one.
//
// Work split. A workgroup owns a tile of T = 8192 consecutive output
// elements in LDS (32 KB, plus under 2 KB of search results) and grid-strides
// over the tiles. Four workgroups share a CU's 160 KB: 16 waves, enough to
// overlap one tile's dependent searches with the other tiles' streaming,
// while a tile is still long enough that its per-party searches are a small
// part of its traffic (about 82 entries per party at ratio 0.01). The
// kernels need few registers, so LDS alone sets the occupancy.
//
// One tile, step by step:
//   1. the tile starts as zeros, or as `out` when accumulating (float4 loads;
//      scalar for the last partial tile or an `out` off a 16 B boundary);
//   2. locate: the entries of party p that fall into the tile are
//      [lower_bound(idx_p, tile_lo), lower_bound(idx_p, tile_hi)). Wave w
//      takes parties w, w + 4, ..., so the NP searches run side by side on
//      the four waves. A search is W-ary across the 64 lanes of the wave, the
//      ballot scheme of k_dgt_encode: 4 dependent loads for 16 M entries.
//      The two bounds of a party advance in lockstep, one probe each per
//      step, so the upper bound costs no latency of its own; that is why the
//      bound is not carried from tile to tile (the grid-stride order would
//      have to change for it, to save loads that already overlap);
//   3. the first 256 entries of EVERY party's range are loaded (index and
//      value) before the first add, NP independent loads per lane; at ratio
//      0.01 that is the whole range;
//   4. parties are added in order 0 .. NP-1, a barrier after each. Inside a
//      party the indices are unique, so the order of its adds is free; the
//      add is the LDS float atomic (ds_add_f32), which stays a well-defined
//      sum if a malformed list repeats an index;
//   5. the tile leaves as contiguous float4 stores (scalar as in 1).
// No dense scratch tensor, no global atomic, no workspace, no host
// synchronisation.
//
// Coded form (bsc_dgt). The values travel as a DGT mode-3 payload over the
// list positions: position j belongs to chunk c = j / chunk, which is row r
// of `exact` if keep_idx[r = lower_bound(keep_idx, c)] == c and lossy row
// c - r of `packed` / `minmax` otherwise (k_wire_sum_dgt's rule). The
// positions of one tile span few chunks, so the wave that located party p
// also resolves the first BSC_ROWS chunks of its range, one per lane, and
// parks (row, lo, step) in LDS; an entry then costs one 4 B load from
// `exact` or one byte of `packed` (low nibble = even position, as
// k_dequantize_4bit). The rows are found by a per-lane binary search, not a
// W-ary one: n_keep is k / chunk at most (a few hundred), the lanes search
// different chunks at once, and the same function serves an entry whose
// chunk lies past the parked rows (a party with more than BSC_ROWS chunks
// of entries in one tile), so there is one locate routine for both.
// decode4 and step4 are those of wire_codec.h: a dead chunk's 1e-30 span
// decodes as it does in k_dequantize_4bit.
//
// Party table by value, kernels templated on the party count NP of a launch
// (constant indices into the kernel arguments, no scratch), P > 16 served in
// groups of 16 with accumulate = true: all as in wirereduce.hip.
//
// This file is built without packed fp32 instructions (see setup.py).

#include <hip/hip_runtime.h>

#include <cstdint>
#include "wire_codec.h"

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048
#define WIRE_MAX_PARTIES 16
#define BSC_TILE 8192  // output elements per tile
#define BSC_ROWS 8     // DGT chunks of a party's range resolved ahead
#define BSC_WAVES (GEOPS_THREADS / 64)

struct SparseTab {
  const float* vals[WIRE_MAX_PARTIES];
  const int* idx[WIRE_MAX_PARTIES];
};

// coded form: the DGT mode-3 payload of the values, and the exact indices
struct SparseTabDgt {
  const float* exact[WIRE_MAX_PARTIES];
  const int* keep[WIRE_MAX_PARTIES];
  const uint8_t* packed[WIRE_MAX_PARTIES];
  const float* minmax[WIRE_MAX_PARTIES];
  const int* idx[WIRE_MAX_PARTIES];
};

// where a party holds a DGT chunk: row r of `exact` as r >= 0, lossy row l as
// -1 - l (with its codebook), nowhere as BSC_SKIP
#define BSC_SKIP INT32_MIN

struct DgtRow {
  int row;
  float lo, step;
};

// Every lane on its own: plain binary lower_bound of c in keep_idx, then the
// range checks. At most bit-width-of-n_keep dependent loads.
__device__ __forceinline__ DgtRow dgt_locate(const int* __restrict__ keep,
                                             const float* __restrict__ minmax,
                                             int n_keep, int n_lossy, int c) {
  int lb = 0, ub = n_keep;
  while (lb < ub) {
    const int mid = (lb + ub) >> 1;
    if (keep[mid] < c) lb = mid + 1; else ub = mid;
  }
  DgtRow d = {BSC_SKIP, 0.0f, 0.0f};
  const int l = c - lb;
  if (lb < n_keep && keep[lb] == c) {
    d.row = lb;
  } else if (l >= 0 && l < n_lossy) {
    d.row = -1 - l;
    d.lo = minmax[2 * l];
    d.step = step4(d.lo, minmax[2 * l + 1]);
  }
  return d;
}

// value of list position j (0 <= j < k) given its chunk's row
__device__ __forceinline__ float dgt_value(const float* __restrict__ exact,
                                           const uint8_t* __restrict__ packed,
                                           const DgtRow& d, int j, int log2c) {
  const long long e = j & ((1 << log2c) - 1);
  if (d.row >= 0) return exact[((long long)d.row << log2c) + e];
  const uint32_t byte =
      packed[((long long)(-1 - d.row) << (log2c - 1)) + (e >> 1)];
  return decode4((j & 1) ? (byte >> 4) : (byte & 0xFu), d.lo, d.step);
}

// One step of two W-ary lower_bound searches over the same list a[0, k),
// compared as unsigned: lane j probes the last element of the j-th of 64
// equal slices of each remaining range [lb, lb + len), and the wave counts by
// ballot how many probes are below the key. len shrinks to ceil(len / 64) - 1
// at most. Whatever the list holds, 0 <= lb and lb + len <= k stay true.
__device__ __forceinline__ void search_step2(const int* __restrict__ a,
                                             int lane, uint32_t key0, int& lb0,
                                             int& len0, uint32_t key1,
                                             int& lb1, int& len1) {
  const int span0 = (len0 + 63) >> 6, span1 = (len1 + 63) >> 6;
  const int end0 = lb0 + len0, end1 = lb1 + len1;
  const int p0 = lb0 + (lane + 1) * span0 - 1;
  const int p1 = lb1 + (lane + 1) * span1 - 1;
  uint32_t v0 = UINT32_MAX, v1 = UINT32_MAX;  // never below a key
  if (len0 > 0 && p0 < end0) v0 = (uint32_t)a[p0];
  if (len1 > 0 && p1 < end1) v1 = (uint32_t)a[p1];
  lb0 += __popcll(__ballot(v0 < key0)) * span0;
  lb1 += __popcll(__ballot(v1 < key1)) * span1;
  len0 = max(0, min(span0 - 1, end0 - lb0));
  len1 = max(0, min(span1 - 1, end1 - lb1));
}

template <int NP, bool CODED>
struct TabOf {
  using type = SparseTab;
};
template <int NP>
struct TabOf<NP, true> {
  using type = SparseTabDgt;
};

// k: slots per list (every party's), < 2^30. n < 2^31 (indices are i32).
// vec: out is 16 B aligned. log2c, n_keep, n_lossy: coded form only.
template <int NP, bool CODED>
__global__ __launch_bounds__(GEOPS_THREADS) void k_wire_sum_bsc(
    typename TabOf<NP, CODED>::type tab, float* __restrict__ out, long long n,
    int k, int log2c, int n_keep, int n_lossy, bool vec, bool accumulate) {
  __shared__ float tile[BSC_TILE];
  __shared__ int s_lo[NP], s_hi[NP];
  __shared__ DgtRow s_row[CODED ? NP : 1][BSC_ROWS];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long long ntiles = (n + BSC_TILE - 1) / BSC_TILE;

  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long base = t * BSC_TILE;
    const int tlen = (int)min((long long)BSC_TILE, n - base);
    const bool whole = vec && tlen == BSC_TILE;

    // 1. the tile's starting value
    if (whole) {
      const float4* o4 = reinterpret_cast<const float4*>(out + base);
      float4* t4 = reinterpret_cast<float4*>(tile);
#pragma unroll
      for (int g = 0; g < BSC_TILE / 4 / GEOPS_THREADS; ++g) {
        const int q = tid + g * GEOPS_THREADS;
        t4[q] = accumulate ? o4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    } else {
      for (int e = tid; e < tlen; e += GEOPS_THREADS)
        tile[e] = accumulate ? out[base + e] : 0.0f;
    }

    // 2. locate every party's entries of [base, base + tlen)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if ((p & (BSC_WAVES - 1)) != wave) continue;  // wave-uniform
      int lb0 = 0, len0 = k, lb1 = 0, len1 = k;
      while (len0 > 0 || len1 > 0)
        search_step2(tab.idx[p], lane, (uint32_t)base, lb0, len0,
                     (uint32_t)(base + tlen), lb1, len1);
      if (lane == 0) {
        s_lo[p] = lb0;
        s_hi[p] = lb1 < lb0 ? lb0 : lb1;  // an unsorted list: empty range
      }
      if constexpr (CODED) {
        if (lane < BSC_ROWS && lb0 < lb1)
          s_row[p][lane] = dgt_locate(tab.keep[p], tab.minmax[p], n_keep,
                                      n_lossy, (lb0 >> log2c) + lane);
      }
    }
    __syncthreads();

    // 3. the first GEOPS_THREADS entries of every party's range
    int fi[NP];
    float fv[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int j = s_lo[p] + tid;
      fi[p] = -1;
      fv[p] = 0.0f;
      if (j < s_hi[p]) {
        fi[p] = tab.idx[p][j];
        if constexpr (CODED) {
          const int r = (j >> log2c) - (s_lo[p] >> log2c);
          const DgtRow d = r < BSC_ROWS
              ? s_row[p][r]
              : dgt_locate(tab.keep[p], tab.minmax[p], n_keep, n_lossy,
                           j >> log2c);
          if (d.row == BSC_SKIP)
            fi[p] = -1;
          else
            fv[p] = dgt_value(tab.exact[p], tab.packed[p], d, j, log2c);
        } else {
          fv[p] = tab.vals[p][j];
        }
      }
    }

    // 4. ordered adds: party p is complete before party p + 1 starts
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int lo = s_lo[p], hi = s_hi[p];
      // unsigned: a negative index, or one below the tile, wraps past tlen
      uint32_t off = (uint32_t)fi[p] - (uint32_t)base;
      if (off < (uint32_t)tlen) atomicAdd(&tile[off], fv[p]);
      for (int j = lo + GEOPS_THREADS + tid; j < hi; j += GEOPS_THREADS) {
        off = (uint32_t)tab.idx[p][j] - (uint32_t)base;
        if (off >= (uint32_t)tlen) continue;
        float v;
        if constexpr (CODED) {
          const int r = (j >> log2c) - (lo >> log2c);
          const DgtRow d = r < BSC_ROWS
              ? s_row[p][r]
              : dgt_locate(tab.keep[p], tab.minmax[p], n_keep, n_lossy,
                           j >> log2c);
          if (d.row == BSC_SKIP) continue;
          v = dgt_value(tab.exact[p], tab.packed[p], d, j, log2c);
        } else {
          v = tab.vals[p][j];
        }
        atomicAdd(&tile[off], v);
      }
      __syncthreads();
    }

    // 5. the tile leaves; the barrier keeps the next trip's step 1 and 2
    // from overwriting what a slower wave still reads
    if (whole) {
      float4* o4 = reinterpret_cast<float4*>(out + base);
      const float4* t4 = reinterpret_cast<const float4*>(tile);
#pragma unroll
      for (int g = 0; g < BSC_TILE / 4 / GEOPS_THREADS; ++g)
        o4[tid + g * GEOPS_THREADS] = t4[tid + g * GEOPS_THREADS];
    } else {
      for (int e = tid; e < tlen; e += GEOPS_THREADS) out[base + e] = tile[e];
    }
    __syncthreads();
  }
}

template <int NP, bool CODED>
static void launch_bsc(int np, const typename TabOf<NP, CODED>::type& tab,
                       float* out, long long n, int k, int log2c, int n_keep,
                       int n_lossy, bool acc, hipStream_t s) {
  if (np == NP) {
    long long nb = (n + BSC_TILE - 1) / BSC_TILE;
    if (nb > GEOPS_MAX_BLOCKS) nb = GEOPS_MAX_BLOCKS;
    const bool vec = ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL((k_wire_sum_bsc<NP, CODED>), dim3((int)nb),
                       dim3(GEOPS_THREADS), 0, s, tab, out, n, k, log2c,
                       n_keep, n_lossy, vec, acc);
  } else if constexpr (NP > 1) {
    launch_bsc<NP - 1, CODED>(np, tab, out, n, k, log2c, n_keep, n_lossy, acc,
                              s);
  }
}

extern "C" {

int geops_wire_sum_bsc_tile() { return BSC_TILE; }

// vals, idxs: P device pointers each (host arrays), every list k slots long.
// 1 <= n < 2^31, 0 <= k < 2^30 (checked by the binding).
void geops_wire_sum_bsc(const float* const* vals, const int* const* idxs,
                        int P, int k, float* out, long long n,
                        bool accumulate, hipStream_t s) {
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    SparseTab tab = {};
    for (int j = 0; j < np; ++j) {
      tab.vals[j] = vals[p0 + j];
      tab.idx[j] = idxs[p0 + j];
    }
    launch_bsc<WIRE_MAX_PARTIES, false>(np, tab, out, n, k, 0, 0, 0,
                                        accumulate || p0 > 0, s);
  }
}

// coded form: the values are DGT mode-3 payloads over the k list positions,
// nchunks = ceil(k / chunk), n_keep kept chunks per party; chunk a power of
// two in [64, 8192], k >= 1
void geops_wire_sum_bsc_dgt(const float* const* exacts,
                            const int* const* keeps,
                            const uint8_t* const* packeds,
                            const float* const* minmaxs,
                            const int* const* idxs, int P, int k, int chunk,
                            int n_keep, float* out, long long n,
                            bool accumulate, hipStream_t s) {
  int log2c = 0;
  while ((1 << log2c) < chunk) ++log2c;
  const int n_lossy = (k + chunk - 1) / chunk - n_keep;
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    SparseTabDgt tab = {};
    for (int j = 0; j < np; ++j) {
      tab.exact[j] = exacts[p0 + j];
      tab.keep[j] = keeps[p0 + j];
      tab.packed[j] = packeds[p0 + j];
      tab.minmax[j] = minmaxs[p0 + j];
      tab.idx[j] = idxs[p0 + j];
    }
    launch_bsc<WIRE_MAX_PARTIES, true>(np, tab, out, n, k, log2c, n_keep,
                                       n_lossy, accumulate || p0 > 0, s);
  }
}

}  // extern "C"
