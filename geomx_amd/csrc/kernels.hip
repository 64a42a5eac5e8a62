// gfx950 (MI355X / CDNA4) kernels for the geomx_amd kvstore hot path.
//
// Every kernel here is memory-bound (elementwise / select / pack); the
// design rules applied (from the CDNA4 programming guide):
//   - wave64: ballots are 64-bit, lane masks use (1ull<<lane)-1
//   - vectorized float4 (16B/lane) loads/stores on the streaming paths
//   - grid-stride loops, grid capped at ~2048 blocks of 256 threads
//   - wave-level prefix sums via __ballot/__popcll for the pack paths
//     (replaces the reference's serial CPU scans,
//      gradient_compression.cc:191-336)
//
// Semantics match geomx_amd/ops/reference.py (the golden model used by
// tests/test_kernels_gpu.py).

#include <hip/hip_runtime.h>

#include <cstdint>
#include "optim_rules.h"

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048

static inline int geops_blocks(long long work, int per_thread = 1) {
  long long b = (work + (long long)GEOPS_THREADS * per_thread - 1) /
                ((long long)GEOPS_THREADS * per_thread);
  if (b < 1) b = 1;
  if (b > GEOPS_MAX_BLOCKS) b = GEOPS_MAX_BLOCKS;
  return (int)b;
}

// ---------------------------------------------------------------------------
// 2bit quantization (gradient_compression-inl.h:40-139 semantics)
// code: 0b11 -> +thr, 0b10 -> -thr, 0b00 -> 0; 16 codes per uint32 word,
// slot s occupies bits [2s, 2s+1].
// ---------------------------------------------------------------------------

// spread 16 bits of x to even bit positions of a 32-bit word
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
  x &= 0x0000FFFFu;
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

extern "C" __global__ void k_quantize_2bit(const float* __restrict__ grad,
                                           float* __restrict__ residual,
                                           uint32_t* __restrict__ out,
                                           long long n, float thr) {
  const int lane = threadIdx.x & 63;
  const long long wave_id = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long base = wave_id * 64; base < n; base += n_waves * 64) {
    const long long i = base + lane;
    const bool active = i < n;
    uint32_t b0 = 0, b1 = 0;  // bit0 / bit1 of this lane's code
    if (active) {
      float r = residual[i] + grad[i];
      if (r >= thr) {
        b0 = 1; b1 = 1;       // 0b11
        r -= thr;
      } else if (r <= -thr) {
        b1 = 1;               // 0b10
        r += thr;
      }
      residual[i] = r;
    }
    const uint64_t m0 = __ballot(b0);
    const uint64_t m1 = __ballot(b1);
    if ((lane & 15) == 0) {
      const int j = lane >> 4;  // which 16-lane group
      const uint32_t s0 = (uint32_t)((m0 >> (j * 16)) & 0xFFFFu);
      const uint32_t s1 = (uint32_t)((m1 >> (j * 16)) & 0xFFFFu);
      const long long w = (base >> 4) + j;
      if (w * 16 < n) out[w] = spread16(s0) | (spread16(s1) << 1);
    }
  }
}

__device__ __forceinline__ float decode2(uint32_t c, float thr) {
  return (c == 3u) ? thr : ((c == 2u) ? -thr : 0.0f);
}

// vectorized main body: each thread decodes 4 elements (one byte of a
// word) and stores one float4 — lane-contiguous 16B stores; scalar tail.
extern "C" __global__ void k_dequantize_2bit(const uint32_t* __restrict__ in,
                                             float* __restrict__ out,
                                             long long n, float thr) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = n >> 2;  // float4 groups fully inside n
  float4* out4 = reinterpret_cast<float4*>(out);
  for (long long q = tid; q < n4; q += stride) {
    // elements 4q..4q+3 live in byte (q&3) of word (q>>2)
    const uint32_t word = in[q >> 2];
    const uint32_t byte = (word >> ((q & 3) * 8)) & 0xFFu;
    float4 o;
    o.x = decode2(byte & 3u, thr);
    o.y = decode2((byte >> 2) & 3u, thr);
    o.z = decode2((byte >> 4) & 3u, thr);
    o.w = decode2((byte >> 6) & 3u, thr);
    out4[q] = o;
  }
  for (long long i = (n4 << 2) + tid; i < n; i += stride) {
    const uint32_t word = in[i >> 4];
    out[i] = decode2((word >> ((i & 15) * 2)) & 3u, thr);
  }
}

// ---------------------------------------------------------------------------
// Bi-Sparse: fused momentum correction (u = mu*u + g ; v += u)
// ---------------------------------------------------------------------------

// u*mu and + g are rounded SEPARATELY (no FMA contraction), exactly as
// the golden model (two torch ops) and the sampled boundary prediction
// do: the boundary is the |v| of one sampled element, so a fused
// multiply-add that lands one ulp below it would drop that element, and
// a mixed CPU/GPU party would drift apart in u and v.
__device__ __forceinline__ float bsc_mom(float u, float mu, float g) {
#pragma clang fp contract(off)
  const float p = u * mu;
  return p + g;
}

extern "C" __global__ void k_bsc_momentum(const float* __restrict__ g,
                                          float* __restrict__ u,
                                          float* __restrict__ v,
                                          float mu, long long n) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* u4 = reinterpret_cast<float4*>(u);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (long long i = tid; i < n4; i += stride) {
    float4 gg = g4[i], uu = u4[i], vv = v4[i];
    uu.x = bsc_mom(uu.x, mu, gg.x); vv.x += uu.x;
    uu.y = bsc_mom(uu.y, mu, gg.y); vv.y += uu.y;
    uu.z = bsc_mom(uu.z, mu, gg.z); vv.z += uu.z;
    uu.w = bsc_mom(uu.w, mu, gg.w); vv.w += uu.w;
    u4[i] = uu; v4[i] = vv;
  }
  for (long long i = (n4 << 2) + tid; i < n; i += stride) {
    float uu = bsc_mom(u[i], mu, g[i]);
    u[i] = uu;
    v[i] += uu;
  }
}

// ---------------------------------------------------------------------------
// Bi-Sparse pack: 3-phase parallel replacement of the reference's serial
// capacity-bounded index-order scan (gradient_compression.cc:245-267).
// Blocks own contiguous chunks so the packed output preserves index order.
// ---------------------------------------------------------------------------

__device__ __forceinline__ long long chunk_begin(long long n, int nb, int b) {
  // chunk rounded to a multiple of 4 so every block's slice is
  // 16-byte aligned for float4 loads
  const long long chunk = (((n + nb - 1) / nb) + 3) & ~3LL;
  long long s = (long long)b * chunk;
  return s < n ? s : n;
}

// phase 1: per-block predicate counts (float4 main body + scalar tail;
// chunk boundaries are 4-aligned by construction in chunk_begin)
template <bool NONZERO>
__global__ void k_bsc_count_t(const float* __restrict__ v, float boundary,
                              long long n, int nb,
                              long long* __restrict__ counts) {
  __shared__ long long lds[GEOPS_THREADS / 64];
  const int b = blockIdx.x;
  const long long lo = chunk_begin(n, nb, b), hi = chunk_begin(n, nb, b + 1);
  long long cnt = 0;
  const long long nvec = (hi - lo) >> 2;
  const float4* v4 = reinterpret_cast<const float4*>(v + lo);
  for (long long q = threadIdx.x; q < nvec; q += blockDim.x) {
    const float4 x = v4[q];
    if (NONZERO) {
      cnt += (x.x != 0.0f) + (x.y != 0.0f) + (x.z != 0.0f) + (x.w != 0.0f);
    } else {
      cnt += (fabsf(x.x) >= boundary) + (fabsf(x.y) >= boundary) +
             (fabsf(x.z) >= boundary) + (fabsf(x.w) >= boundary);
    }
  }
  for (long long i = lo + (nvec << 2) + threadIdx.x; i < hi; i += blockDim.x) {
    const float x = v[i];
    const bool pred = NONZERO ? (x != 0.0f) : (fabsf(x) >= boundary);
    cnt += pred ? 1 : 0;
  }
  // wave reduce then LDS reduce
  for (int off = 32; off > 0; off >>= 1)
    cnt += __shfl_down(cnt, off, 64);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wid] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += lds[w];
    counts[b] = total;
  }
}

// phase 2: single-block exclusive scan of per-block counts (+ total at [nb])
extern "C" __global__ void k_bsc_scan(long long* __restrict__ counts, int nb) {
  // nb <= 2048; serial scan by one thread is fine (tiny)
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    long long acc = 0;
    for (int i = 0; i < nb; ++i) {
      const long long c = counts[i];
      counts[i] = acc;
      acc += c;
    }
    counts[nb] = acc;
  }
}

// phase 3: ordered pack with capacity bound; optionally zero u,v at the
// positions actually sent (error feedback, reference :258-260)
// ordered capacity-bounded pack: each thread takes 4 consecutive
// elements per iteration (block covers 1024), per-thread counts are
// scanned wave-wide with __shfl_up, wave totals with one LDS pass —
// index order is preserved across threads, waves, iterations, blocks.
template <bool ZERO_UV>
__global__ void k_bsc_pack_t(const float* __restrict__ v_in,
                             float* __restrict__ v_mut,
                             float* __restrict__ u_mut,
                             float* __restrict__ vals,
                             int* __restrict__ idx,
                             const long long* __restrict__ offsets,
                             float boundary, long long n, int nb,
                             long long capacity) {
  __shared__ long long wave_base[GEOPS_THREADS / 64];
  __shared__ long long carry_s;
  const int b = blockIdx.x;
  const long long lo = chunk_begin(n, nb, b), hi = chunk_begin(n, nb, b + 1);
  if (threadIdx.x == 0) carry_s = offsets[b];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const long long span = (long long)blockDim.x * 4;
  for (long long base = lo; base < hi; base += span) {
    const long long i0 = base + (long long)threadIdx.x * 4;
    float x[4];
    bool p[4];
    int cnt = 0;
    if (i0 + 4 <= hi) {  // aligned float4 fast path (lo is 4-aligned)
      const float4 xx = *reinterpret_cast<const float4*>(v_in + i0);
      x[0] = xx.x; x[1] = xx.y; x[2] = xx.z; x[3] = xx.w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        p[j] = fabsf(x[j]) >= boundary;
        cnt += p[j] ? 1 : 0;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = i0 + j;
        const bool in_range = i < hi;
        x[j] = in_range ? v_in[i] : 0.0f;
        p[j] = in_range && (fabsf(x[j]) >= boundary);
        cnt += p[j] ? 1 : 0;
      }
    }
    // wave-inclusive scan of per-thread counts
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    const int excl = incl - cnt;
    const int wave_total = __shfl(incl, 63, 64);
    if (lane == 63) wave_base[wid] = incl;  // wave total
    __syncthreads();
    if (threadIdx.x == 0) {
      long long acc = carry_s;
      for (int w = 0; w < nwaves; ++w) {
        const long long c = wave_base[w];
        wave_base[w] = acc;
        acc += c;
      }
      carry_s = acc;
    }
    __syncthreads();
    long long pos = wave_base[wid] + excl;
    (void)wave_total;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (p[j]) {
        if (pos < capacity) {
          const long long i = i0 + j;
          vals[pos] = x[j];
          idx[pos] = (int)i;
          if (ZERO_UV) {
            v_mut[i] = 0.0f;
            u_mut[i] = 0.0f;
          }
        }
        ++pos;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Fused single-pass Bi-Sparse compress: momentum + count + ordered pack in
// ONE sweep of (g,u,v) with a decoupled-lookback prefix over blocks
// (replaces the momentum + count + scan + pack 4-launch chain: the extra
// 4n-byte count read disappears; the boundary arrives as a DEVICE scalar
// so the host never synchronizes). Per block: phase 1 streams its
// contiguous chunk (float4), applies u=mu*u+g, v+=u, records the
// |v|>=boundary predicate as an LDS bitmask; phase 2 publishes the block
// aggregate and resolves the exclusive prefix via single-8B agent-scope
// atomics ({status,count} in one granule — the R2 untorn-granule form, no
// fences needed); phase 3 walks the bitmask, wave-scans positions, and
// writes the capacity-bounded ordered pack, zeroing u,v at sent slots.
// Deadlock-free by construction: the grid is capped at 4 blocks/CU x 256
// CUs, so every block is resident and publishes its aggregate with no
// dependence on any other block.
// ---------------------------------------------------------------------------

#define BSC_FUSE_CHUNK_MAX (128 * 1024)  // elements per block (16 KiB mask)
#define BSC_FUSE_MAX_BLOCKS 1024         // 4 blocks/CU x 256 CUs: all resident

extern "C" __global__ __launch_bounds__(GEOPS_THREADS, 4) void k_bsc_fused(
    const float* __restrict__ g, float* __restrict__ u,
    float* __restrict__ v, float* __restrict__ vals, int* __restrict__ idx,
    const float* __restrict__ boundary_p,
    unsigned long long* __restrict__ ws,  // [nb+1] lookback slots
    float mu, long long n, long long capacity, int nb) {
  __shared__ unsigned char mask[BSC_FUSE_CHUNK_MAX / 8];
  __shared__ long long wave_base[GEOPS_THREADS / 64];
  __shared__ long long carry_s;
  const int b = blockIdx.x;
  // 8-aligned contiguous chunks (float4 x2 per thread-iteration)
  const long long chunk = (((n + nb - 1) / nb) + 7) & ~7LL;
  long long lo = (long long)b * chunk;
  if (lo > n) lo = n;
  long long hi = lo + chunk;
  if (hi > n) hi = n;
  const float boundary = *boundary_p;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const long long span = (long long)blockDim.x * 8;

  // ---- phase 1: momentum + predicate bitmask + block count ----------
  long long cnt = 0;
  for (long long base = lo; base < hi; base += span) {
    const long long i0 = base + (long long)threadIdx.x * 8;
    unsigned byte = 0;
    if (i0 + 8 <= hi) {
      const float4 g0 = *reinterpret_cast<const float4*>(g + i0);
      const float4 g1 = *reinterpret_cast<const float4*>(g + i0 + 4);
      float4 u0 = *reinterpret_cast<float4*>(u + i0);
      float4 u1 = *reinterpret_cast<float4*>(u + i0 + 4);
      float4 v0 = *reinterpret_cast<float4*>(v + i0);
      float4 v1 = *reinterpret_cast<float4*>(v + i0 + 4);
      u0.x = bsc_mom(u0.x, mu, g0.x); v0.x += u0.x;
      u0.y = bsc_mom(u0.y, mu, g0.y); v0.y += u0.y;
      u0.z = bsc_mom(u0.z, mu, g0.z); v0.z += u0.z;
      u0.w = bsc_mom(u0.w, mu, g0.w); v0.w += u0.w;
      u1.x = bsc_mom(u1.x, mu, g1.x); v1.x += u1.x;
      u1.y = bsc_mom(u1.y, mu, g1.y); v1.y += u1.y;
      u1.z = bsc_mom(u1.z, mu, g1.z); v1.z += u1.z;
      u1.w = bsc_mom(u1.w, mu, g1.w); v1.w += u1.w;
      *reinterpret_cast<float4*>(u + i0) = u0;
      *reinterpret_cast<float4*>(u + i0 + 4) = u1;
      *reinterpret_cast<float4*>(v + i0) = v0;
      *reinterpret_cast<float4*>(v + i0 + 4) = v1;
      byte |= (fabsf(v0.x) >= boundary) << 0;
      byte |= (fabsf(v0.y) >= boundary) << 1;
      byte |= (fabsf(v0.z) >= boundary) << 2;
      byte |= (fabsf(v0.w) >= boundary) << 3;
      byte |= (fabsf(v1.x) >= boundary) << 4;
      byte |= (fabsf(v1.y) >= boundary) << 5;
      byte |= (fabsf(v1.z) >= boundary) << 6;
      byte |= (fabsf(v1.w) >= boundary) << 7;
    } else {
      for (int j = 0; j < 8; ++j) {
        const long long i = i0 + j;
        if (i < hi) {
          const float uu = bsc_mom(u[i], mu, g[i]);
          u[i] = uu;
          const float vv = v[i] + uu;
          v[i] = vv;
          byte |= (fabsf(vv) >= boundary) << j;
        }
      }
    }
    if (i0 < hi) mask[(i0 - lo) >> 3] = (unsigned char)byte;
    cnt += __popc(byte);
  }
  // block reduce
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) wave_base[wid] = cnt;
  __syncthreads();

  // ---- phase 2: publish aggregate, decoupled lookback ----------------
  if (threadIdx.x == 0) {
    long long agg = 0;
    for (int w = 0; w < nwaves; ++w) agg += wave_base[w];
    // status 1 = aggregate ready (bit 62), 2 = inclusive prefix ready
    __hip_atomic_store(&ws[b], (1ULL << 62) | (unsigned long long)agg,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long excl = 0;
    for (int p = b - 1; p >= 0;) {
      const unsigned long long w64 = __hip_atomic_load(
          &ws[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned st = (unsigned)(w64 >> 62);
      if (st == 0) {
        __builtin_amdgcn_s_sleep(2);
        continue;
      }
      excl += (long long)(w64 & ((1ULL << 62) - 1));
      if (st >= 2) break;
      --p;
    }
    __hip_atomic_store(&ws[b],
                       (2ULL << 62) | (unsigned long long)(excl + agg),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b == nb - 1) ws[nb] = (unsigned long long)(excl + agg);  // total
    carry_s = excl;
  }
  __syncthreads();

  // ---- phase 3: bitmask walk, wave-scan, ordered capacity-bound pack -
  for (long long base = lo; base < hi; base += span) {
    const long long i0 = base + (long long)threadIdx.x * 8;
    const unsigned byte = (i0 < hi) ? mask[(i0 - lo) >> 3] : 0u;
    int c = __popc(byte);
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    const int excl = incl - c;
    if (lane == 63) wave_base[wid] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      long long acc = carry_s;
      for (int w = 0; w < nwaves; ++w) {
        const long long t = wave_base[w];
        wave_base[w] = acc;
        acc += t;
      }
      carry_s = acc;
    }
    __syncthreads();
    long long pos = wave_base[wid] + excl;
    unsigned bits = byte;
    while (bits) {
      const int j = __ffs(bits) - 1;
      bits &= bits - 1;
      if (pos < capacity) {
        const long long i = i0 + j;
        vals[pos] = v[i];
        idx[pos] = (int)i;
        v[i] = 0.0f;
        u[i] = 0.0f;
      }
      ++pos;
    }
    __syncthreads();
  }
}

// placeholder fill for unused capacity (reference :262-266)
extern "C" __global__ void k_bsc_fill_tail(float* __restrict__ vals,
                                           int* __restrict__ idx,
                                           const long long* __restrict__ counts,
                                           int nb, long long capacity,
                                           float placeholder) {
  long long total = counts[nb];
  if (total > capacity) total = capacity;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = total + tid; i < capacity; i += stride) {
    vals[i] = placeholder;
    idx[i] = -1;
  }
}

extern "C" __global__ void k_bsc_unpack(const float* __restrict__ vals,
                                        const int* __restrict__ idx,
                                        float* __restrict__ out,
                                        long long k, long long n,
                                        bool accumulate) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = tid; i < k; i += stride) {
    const int j = idx[i];
    // indices come off the wire: placeholders (-1) and anything outside
    // [0, n) are skipped, as the row-sparse kernels skip out-of-range ids
    if (j >= 0 && j < n) {
      if (accumulate)
        atomicAdd(out + j, vals[i]);
      else
        out[j] = vals[i];
    }
  }
}

// ---------------------------------------------------------------------------
// DGT: per-chunk mean(|g|) contribution (kv_app.h:853-876)
// ---------------------------------------------------------------------------

extern "C" __global__ void k_dgt_contribution(const float* __restrict__ g,
                                              float* __restrict__ out,
                                              long long n, int chunk,
                                              int nchunks) {
  __shared__ float lds[GEOPS_THREADS / 64];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long long lo = (long long)c * chunk;
    const long long hi = min(lo + chunk, n);
    float s = 0.0f;
    // float4 loads need g + c*chunk 16-byte aligned: only when chunk is
    // a multiple of 4 (g itself is); any other chunk takes the scalar loop
    const long long nvec = ((chunk & 3) == 0) ? ((hi - lo) >> 2) : 0;
    const float4* g4 = reinterpret_cast<const float4*>(g + lo);
    for (long long q = threadIdx.x; q < nvec; q += blockDim.x) {
      const float4 v = g4[q];
      s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
    }
    for (long long i = lo + (nvec << 2) + threadIdx.x; i < hi;
         i += blockDim.x)
      s += fabsf(g[i]);
    for (int off = 32; off > 0; off >>= 1)
      s += __shfl_down(s, off, 64);
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      float total = 0.0f;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += lds[w];
      out[c] = total / (float)(hi - lo);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// 4-bit linear quantization per chunk with residual feedback
// (van.cc:750-824 semantics; codes are bin midpoints on [min,max])
// ---------------------------------------------------------------------------

extern "C" __global__ void k_minmax_chunk(const float* __restrict__ x,
                                          const float* __restrict__ residual,
                                          float* __restrict__ minmax,
                                          long long n, int chunk, int nchunks,
                                          bool has_res) {
  __shared__ float lmin[GEOPS_THREADS / 64];
  __shared__ float lmax[GEOPS_THREADS / 64];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long long lo = (long long)c * chunk;
    const long long hi = min(lo + chunk, n);
    float mn = 3.4e38f, mx = -3.4e38f;
    const long long nvec = (hi - lo) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + lo);
    const float4* r4 = reinterpret_cast<const float4*>(residual + lo);
    for (long long q = threadIdx.x; q < nvec; q += blockDim.x) {
      float4 f = x4[q];
      if (has_res) {
        const float4 r = r4[q];
        f.x += r.x; f.y += r.y; f.z += r.z; f.w += r.w;
      }
      mn = fminf(fminf(fminf(mn, f.x), f.y), fminf(f.z, f.w));
      mx = fmaxf(fmaxf(fmaxf(mx, f.x), f.y), fmaxf(f.z, f.w));
    }
    for (long long i = lo + (nvec << 2) + threadIdx.x; i < hi;
         i += blockDim.x) {
      const float f = x[i] + (has_res ? residual[i] : 0.0f);
      mn = fminf(mn, f);
      mx = fmaxf(mx, f);
    }
    for (int off = 32; off > 0; off >>= 1) {
      mn = fminf(mn, __shfl_down(mn, off, 64));
      mx = fmaxf(mx, __shfl_down(mx, off, 64));
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { lmin[wid] = mn; lmax[wid] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
        lmin[0] = fminf(lmin[0], lmin[w]);
        lmax[0] = fmaxf(lmax[0], lmax[w]);
      }
      minmax[2 * c] = lmin[0];
      minmax[2 * c + 1] = lmax[0];
    }
    __syncthreads();
  }
}

// chunk must be a power of two on the GPU path (log2c = log2(chunk));
// each thread packs 4 elements (reads float4, writes one u16).
extern "C" __global__ void k_quantize_4bit(const float* __restrict__ x,
                                           float* __restrict__ residual,
                                           uint8_t* __restrict__ out,
                                           const float* __restrict__ minmax,
                                           long long n, int log2c,
                                           bool has_res) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long nq = n >> 2;
  uint16_t* out16 = reinterpret_cast<uint16_t*>(out);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* r4 = reinterpret_cast<float4*>(residual);
  for (long long q = tid; q < nq; q += stride) {
    // chunk is a power of two >= 4: the 4 elements of q share one chunk
    const int c = (int)((q << 2) >> log2c);
    const float lo = minmax[2 * c];
    const float step = fmaxf(minmax[2 * c + 1] - lo, 1e-30f) / 16.0f;
    const float inv = 1.0f / step;
    const float4 xx = x4[q];
    float f[4] = {xx.x, xx.y, xx.z, xx.w};
    if (has_res) {
      const float4 rr = r4[q];
      f[0] += rr.x; f[1] += rr.y; f[2] += rr.z; f[3] += rr.w;
    }
    uint16_t word = 0;
    float rout[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int code = (int)floorf((f[j] - lo) * inv);
      code = code < 0 ? 0 : (code > 15 ? 15 : code);
      rout[j] = f[j] - (lo + ((float)code + 0.5f) * step);
      word |= (uint16_t)(code << (4 * j));
    }
    if (has_res) r4[q] = make_float4(rout[0], rout[1], rout[2], rout[3]);
    out16[q] = word;
  }
  // scalar tail (< 4 elements): one thread packs the remaining bytes
  if (tid == 0) {
    for (long long i = (nq << 2); i < n; i += 2) {
      uint8_t byte = 0;
      for (int h = 0; h < 2 && i + h < n; ++h) {
        const long long ii = i + h;
        const int c = (int)(ii >> log2c);
        const float lo = minmax[2 * c];
        const float step = fmaxf(minmax[2 * c + 1] - lo, 1e-30f) / 16.0f;
        const float f = x[ii] + (has_res ? residual[ii] : 0.0f);
        int code = (int)floorf((f - lo) / step);
        code = code < 0 ? 0 : (code > 15 ? 15 : code);
        if (has_res) residual[ii] = f - (lo + ((float)code + 0.5f) * step);
        byte |= (uint8_t)(code << (4 * h));
      }
      out[i >> 1] = byte;
    }
  }
}

extern "C" __global__ void k_dequantize_4bit(const uint8_t* __restrict__ in,
                                             const float* __restrict__ minmax,
                                             float* __restrict__ out,
                                             long long n, int log2c) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long nq = n >> 2;
  const uint16_t* in16 = reinterpret_cast<const uint16_t*>(in);
  float4* out4 = reinterpret_cast<float4*>(out);
  for (long long q = tid; q < nq; q += stride) {
    const int c = (int)((q << 2) >> log2c);
    const float lo = minmax[2 * c];
    const float step = fmaxf(minmax[2 * c + 1] - lo, 1e-30f) / 16.0f;
    const uint16_t w = in16[q];
    float4 o;
    o.x = lo + ((float)(w & 0xF) + 0.5f) * step;
    o.y = lo + ((float)((w >> 4) & 0xF) + 0.5f) * step;
    o.z = lo + ((float)((w >> 8) & 0xF) + 0.5f) * step;
    o.w = lo + ((float)((w >> 12) & 0xF) + 0.5f) * step;
    out4[q] = o;
  }
  for (long long i = (nq << 2) + tid; i < n; i += stride) {
    const int c = (int)(i >> log2c);
    const float lo = minmax[2 * c];
    const float step = fmaxf(minmax[2 * c + 1] - lo, 1e-30f) / 16.0f;
    const uint8_t byte = in[i >> 1];
    const int code = (i & 1) ? (byte >> 4) : (byte & 0x0F);
    out[i] = lo + ((float)code + 0.5f) * step;
  }
}

// ---------------------------------------------------------------------------
// Fused optimizer updates (the server ApplyUpdates hot loop,
// optimizer_op.cc:43-651 semantics). fp32. One loop over the rules of
// optim_rules.h: VEC = 4 is float4 granules + scalar tail, VEC = 1 a plain
// loop. blockDim.x in a device function keeps a partial-workgroup path that
// a kernel body folds away, hence the builtin. k_signum_update and
// k_dcasgd_update keep their own loops: through optim_dense they measured
// 2.4 % and 6 % slower than before (docs/kernels.md).
// ---------------------------------------------------------------------------

template <int VEC, typename OP>
__device__ __forceinline__ void optim_dense(
    const OP& op, long long n, float* __restrict__ w,
    const float* __restrict__ g, float* __restrict__ s0 = nullptr,
    float* __restrict__ s1 = nullptr) {
  const unsigned bdim = __builtin_amdgcn_workgroup_size_x();
  const long long tid = (long long)blockIdx.x * bdim + threadIdx.x;
  const long long stride = (long long)gridDim.x * bdim;
  const long long nv = (VEC == 4) ? (n >> 2) : n;
  for (long long i = tid; i < nv; i += stride)
    optim_apply<VEC>(op, g + i * VEC, w, s0, s1, i * VEC);
  if (VEC > 1)
    for (long long i = nv * VEC + tid; i < n; i += stride)
      optim_apply<1>(op, g + i, w, s0, s1, i);
}

extern "C" __global__ void k_sgd_update(float* __restrict__ w,
                                        const float* __restrict__ g,
                                        float lr, float wd, float rescale,
                                        long long n) {
  optim_dense<4>(SgdRule{lr, wd, rescale}, n, w, g);
}

extern "C" __global__ void k_sgd_mom_update(float* __restrict__ w,
                                            const float* __restrict__ g,
                                            float* __restrict__ mom,
                                            float lr, float momentum,
                                            float wd, float rescale,
                                            long long n) {
  optim_dense<4>(SgdMomRule{lr, momentum, wd, rescale}, n, w, g, mom);
}

extern "C" __global__ void k_adam_update(float* __restrict__ w,
                                         const float* __restrict__ g,
                                         float* __restrict__ m,
                                         float* __restrict__ v,
                                         float lr_t, float beta1, float beta2,
                                         float eps, float wd, float rescale,
                                         long long n) {
  optim_dense<4>(AdamRule{lr_t, beta1, beta2, eps, wd, rescale}, n, w, g, m,
                 v);
}

extern "C" __global__ void k_rmsprop_update(float* __restrict__ w,
                                            const float* __restrict__ g,
                                            float* __restrict__ n_st,
                                            float lr, float rho, float eps,
                                            float wd, float rescale,
                                            long long n) {
  optim_dense<4>(RmspropRule{lr, rho, eps, wd, rescale}, n, w, g, n_st);
}

extern "C" __global__ void k_adagrad_update(float* __restrict__ w,
                                            const float* __restrict__ g,
                                            float* __restrict__ h,
                                            float lr, float eps, float wd,
                                            float rescale, long long n) {
  optim_dense<1>(AdagradRule{lr, eps, wd, rescale}, n, w, g, h);
}

extern "C" __global__ void k_signsgd_update(float* __restrict__ w,
                                            const float* __restrict__ g,
                                            float lr, float wd,
                                            float rescale, long long n) {
  optim_dense<1>(SignsgdRule{lr, wd, rescale}, n, w, g);
}

extern "C" __global__ void k_signum_update(float* __restrict__ w,
                                           const float* __restrict__ g,
                                           float* __restrict__ mom,
                                           float lr, float momentum,
                                           float wd, float rescale,
                                           long long n) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = tid; i < n; i += stride) {
    const float gg = g[i] * rescale + wd * w[i];
    const float mv = momentum * mom[i] + (1.0f - momentum) * gg;
    mom[i] = mv;
    w[i] -= lr * ((mv > 0.0f) ? 1.0f : ((mv < 0.0f) ? -1.0f : 0.0f));
  }
}

extern "C" __global__ void k_dcasgd_update(float* __restrict__ w,
                                           const float* __restrict__ g,
                                           float* __restrict__ prev_w,
                                           float* __restrict__ mom,
                                           float lr, float lamda,
                                           float momentum, float wd,
                                           float rescale, long long n,
                                           bool has_mom) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = tid; i < n; i += stride) {
    const float ww = w[i];
    const float gg = g[i] * rescale;
    float upd = -lr * (gg + wd * ww + lamda * gg * gg * (ww - prev_w[i]));
    if (has_mom) {
      upd = mom[i] * momentum + upd;
      mom[i] = upd;
    }
    prev_w[i] = ww;
    w[i] = ww + upd;
  }
}

// ---------------------------------------------------------------------------
// Fused ReLU + MaxPool2x2(stride 2) NHWC bf16 — replaces ATen's separate
// relu elementwise + max_pool_{forward,backward}_nhwc kernels (together
// ~40% of the CNN benchmark step). relu(maxpool(x)) == maxpool(relu(x))
// for max pooling; the fwd records a per-channel 8-bit code: quadrant
// 0..3 of the argmax, or 255 when the max is <= 0 (ReLU clamps, no
// gradient flows). Layout: logical [N,H,W,C] contiguous (torch
// channels_last), C % 8 == 0, H,W even. 8 bf16 = one 16B vector per lane.
// ---------------------------------------------------------------------------

typedef unsigned short bf16raw;

__device__ __forceinline__ float bf2f(bf16raw h) {
  union { unsigned int u; float f; } cv;
  cv.u = ((unsigned int)h) << 16;
  return cv.f;
}

extern "C" __global__ void k_relu_maxpool2_fwd_nhwc(
    const bf16raw* __restrict__ in, bf16raw* __restrict__ out,
    uint8_t* __restrict__ idx, long long n_vec, int Ho, int Wo, int C) {
  // n_vec = N*Ho*Wo*(C/8); vector v covers out[...][cb*8 .. cb*8+7]
  const int cvec = C >> 3;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int Wi = Wo * 2;
  for (long long v = tid; v < n_vec; v += stride) {
    const int cb = (int)(v % cvec);
    long long rest = v / cvec;
    const int wo = (int)(rest % Wo);
    rest /= Wo;
    const int ho = (int)(rest % Ho);
    const long long n = rest / Ho;
    const long long base =
        (((n * (Ho * 2) + ho * 2) * (long long)Wi + wo * 2) * cvec + cb);
    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    // quadrants: 0=(0,0) 1=(0,1) 2=(1,0) 3=(1,1) in (dy,dx)
    const uint4 q0 = in4[base];
    const uint4 q1 = in4[base + cvec];
    const uint4 q2 = in4[base + (long long)Wi * cvec];
    const uint4 q3 = in4[base + (long long)Wi * cvec + cvec];
    const bf16raw* p0 = reinterpret_cast<const bf16raw*>(&q0);
    const bf16raw* p1 = reinterpret_cast<const bf16raw*>(&q1);
    const bf16raw* p2 = reinterpret_cast<const bf16raw*>(&q2);
    const bf16raw* p3 = reinterpret_cast<const bf16raw*>(&q3);
    bf16raw ov[8];
    uint8_t code[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float m = bf2f(p0[c]);
      int arg = 0;
      const float f1 = bf2f(p1[c]);
      if (f1 > m) { m = f1; arg = 1; }
      const float f2 = bf2f(p2[c]);
      if (f2 > m) { m = f2; arg = 2; }
      const float f3 = bf2f(p3[c]);
      if (f3 > m) { m = f3; arg = 3; }
      if (m <= 0.0f) {
        ov[c] = 0;            // relu clamp
        code[c] = 255;        // no gradient
      } else {
        const bf16raw srcs[4] = {p0[c], p1[c], p2[c], p3[c]};
        ov[c] = srcs[arg];
        code[c] = (uint8_t)arg;
      }
    }
    reinterpret_cast<uint4*>(out)[v] = *reinterpret_cast<uint4*>(ov);
    reinterpret_cast<uint2*>(idx)[v] = *reinterpret_cast<uint2*>(code);
  }
}

extern "C" __global__ void k_relu_maxpool2_bwd_nhwc(
    const bf16raw* __restrict__ grad_out, const uint8_t* __restrict__ idx,
    bf16raw* __restrict__ grad_in, long long n_vec_in, int Hi, int Wi,
    int C) {
  // n_vec_in = N*Hi*Wi*(C/8) over the INPUT tensor
  const int cvec = C >> 3;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int Wo = Wi >> 1;
  const int Ho = Hi >> 1;
  for (long long v = tid; v < n_vec_in; v += stride) {
    const int cb = (int)(v % cvec);
    long long rest = v / cvec;
    const int wi = (int)(rest % Wi);
    rest /= Wi;
    const int hi = (int)(rest % Hi);
    const long long n = rest / Hi;
    const int quad = ((hi & 1) << 1) | (wi & 1);
    const long long ov =
        (((n * Ho + (hi >> 1)) * (long long)Wo + (wi >> 1)) * cvec + cb);
    const uint2 ic = reinterpret_cast<const uint2*>(idx)[ov];
    const uint4 gv = reinterpret_cast<const uint4*>(grad_out)[ov];
    const uint8_t* code = reinterpret_cast<const uint8_t*>(&ic);
    const bf16raw* g = reinterpret_cast<const bf16raw*>(&gv);
    bf16raw r[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
      r[c] = (code[c] == (uint8_t)quad) ? g[c] : (bf16raw)0;
    reinterpret_cast<uint4*>(grad_in)[v] = *reinterpret_cast<uint4*>(r);
  }
}

// ---------------------------------------------------------------------------
// C-ABI launchers
// ---------------------------------------------------------------------------

extern "C" {

void geops_quantize_2bit(const float* grad, float* residual, uint32_t* out,
                         long long n, float thr, hipStream_t s) {
  hipLaunchKernelGGL(k_quantize_2bit, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, grad, residual, out, n, thr);
}

void geops_dequantize_2bit(const uint32_t* in, float* out, long long n,
                           float thr, hipStream_t s) {
  hipLaunchKernelGGL(k_dequantize_2bit, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, in, out, n, thr);
}

void geops_bsc_momentum(const float* g, float* u, float* v, float mu,
                        long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_bsc_momentum, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, g, u, v, mu, n);
}

static int bsc_nblocks(long long n) {
  int nb = (int)((n + 16383) / 16384);
  if (nb < 1) nb = 1;
  if (nb > 1024) nb = 1024;
  return nb;
}


// fused single-pass path; returns -1 when the shape needs the multi-pass
// chain (chunk would exceed the LDS bitmask)
int geops_bsc_fused(const float* g, float* u, float* v, float* vals,
                    int* idx, const float* boundary_p,
                    unsigned long long* ws, float mu, long long n,
                    long long capacity, float placeholder, hipStream_t s) {
  int nb = (int)((n + 16383) / 16384);
  if (nb < 1) nb = 1;
  if (nb > BSC_FUSE_MAX_BLOCKS) nb = BSC_FUSE_MAX_BLOCKS;
  const long long chunk = (((n + nb - 1) / nb) + 7) & ~7LL;
  if (chunk > BSC_FUSE_CHUNK_MAX) return -1;
  hipMemsetAsync(ws, 0, (nb + 1) * sizeof(unsigned long long), s);
  hipLaunchKernelGGL(k_bsc_fused, dim3(nb), dim3(GEOPS_THREADS), 0, s, g,
                     u, v, vals, idx, boundary_p, ws, mu, n, capacity, nb);
  hipLaunchKernelGGL(k_bsc_fill_tail, dim3(geops_blocks(capacity)),
                     dim3(GEOPS_THREADS), 0, s, vals, idx, (long long*)ws,
                     nb, capacity, placeholder);
  return 0;
}

// workspace: (nb+1) int64 entries
void geops_bsc_pack(const float* v_in, float* v_mut, float* u_mut,
                    float* vals, int* idx, long long* workspace,
                    float boundary, long long n, long long capacity,
                    float placeholder, bool zero_uv, hipStream_t s) {
  const int nb = bsc_nblocks(n);
  hipLaunchKernelGGL((k_bsc_count_t<false>), dim3(nb), dim3(GEOPS_THREADS),
                     0, s, v_in, boundary, n, nb, workspace);
  hipLaunchKernelGGL(k_bsc_scan, dim3(1), dim3(64), 0, s, workspace, nb);
  if (zero_uv)
    hipLaunchKernelGGL((k_bsc_pack_t<true>), dim3(nb), dim3(GEOPS_THREADS),
                       0, s, v_in, v_mut, u_mut, vals, idx, workspace,
                       boundary, n, nb, capacity);
  else
    hipLaunchKernelGGL((k_bsc_pack_t<false>), dim3(nb), dim3(GEOPS_THREADS),
                       0, s, v_in, v_mut, u_mut, vals, idx, workspace,
                       boundary, n, nb, capacity);
  hipLaunchKernelGGL(k_bsc_fill_tail, dim3(geops_blocks(capacity)),
                     dim3(GEOPS_THREADS), 0, s, vals, idx, workspace, nb,
                     capacity, placeholder);
}

// pull-side pack of nonzeros: reuse the pack machinery with boundary
// semantics pred = (x != 0): count<true> + pack with boundary=0 on |x|>0.
// A dedicated tiny epsilon boundary on |x| >= FLT_MIN would miss true
// zeros only; we use the NONZERO counter and a pack over |x| >= min_sub.
void geops_bsc_pull_pack(const float* x, float* vals, int* idx,
                         long long* workspace, long long n,
                         long long capacity, float placeholder,
                         hipStream_t s) {
  const int nb = bsc_nblocks(n);
  hipLaunchKernelGGL((k_bsc_count_t<true>), dim3(nb), dim3(GEOPS_THREADS),
                     0, s, x, 0.0f, n, nb, workspace);
  hipLaunchKernelGGL(k_bsc_scan, dim3(1), dim3(64), 0, s, workspace, nb);
  // pred |x| >= FLT_TRUE_MIN  <=>  x != 0 for floats (incl. subnormals)
  hipLaunchKernelGGL((k_bsc_pack_t<false>), dim3(nb), dim3(GEOPS_THREADS),
                     0, s, x, nullptr, nullptr, vals, idx, workspace,
                     1.4e-45f, n, nb, capacity);
  hipLaunchKernelGGL(k_bsc_fill_tail, dim3(geops_blocks(capacity)),
                     dim3(GEOPS_THREADS), 0, s, vals, idx, workspace, nb,
                     capacity, placeholder);
}

void geops_bsc_unpack(const float* vals, const int* idx, float* out,
                      long long k, long long n, bool accumulate,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_bsc_unpack, dim3(geops_blocks(k)),
                     dim3(GEOPS_THREADS), 0, s, vals, idx, out, k, n,
                     accumulate);
}

void geops_dgt_contribution(const float* g, float* out, long long n,
                            int chunk, int nchunks, hipStream_t s) {
  int nb = nchunks < GEOPS_MAX_BLOCKS ? nchunks : GEOPS_MAX_BLOCKS;
  hipLaunchKernelGGL(k_dgt_contribution, dim3(nb), dim3(GEOPS_THREADS),
                     0, s, g, out, n, chunk, nchunks);
}

static int ilog2(int x) {
  int l = 0;
  while ((1 << l) < x) ++l;
  return l;
}

// chunk must be a power of two (enforced by the binding)
void geops_quantize_4bit(const float* x, float* residual, uint8_t* out,
                         float* minmax, long long n, int chunk, int nchunks,
                         bool has_res, hipStream_t s) {
  int nb = nchunks < GEOPS_MAX_BLOCKS ? nchunks : GEOPS_MAX_BLOCKS;
  hipLaunchKernelGGL(k_minmax_chunk, dim3(nb), dim3(GEOPS_THREADS), 0, s,
                     x, residual, minmax, n, chunk, nchunks, has_res);
  hipLaunchKernelGGL(k_quantize_4bit, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, x, residual, out, minmax, n,
                     ilog2(chunk), has_res);
}

void geops_dequantize_4bit(const uint8_t* in, const float* minmax, float* out,
                           long long n, int chunk, hipStream_t s) {
  hipLaunchKernelGGL(k_dequantize_4bit, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, in, minmax, out, n,
                     ilog2(chunk));
}

void geops_relu_maxpool2_fwd(const unsigned short* in, unsigned short* out,
                             uint8_t* idx, long long n_vec, int Ho, int Wo,
                             int C, hipStream_t s) {
  hipLaunchKernelGGL(k_relu_maxpool2_fwd_nhwc, dim3(geops_blocks(n_vec)),
                     dim3(GEOPS_THREADS), 0, s, in, out, idx, n_vec, Ho, Wo,
                     C);
}

void geops_relu_maxpool2_bwd(const unsigned short* grad_out,
                             const uint8_t* idx, unsigned short* grad_in,
                             long long n_vec_in, int Hi, int Wi, int C,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_relu_maxpool2_bwd_nhwc, dim3(geops_blocks(n_vec_in)),
                     dim3(GEOPS_THREADS), 0, s, grad_out, idx, grad_in,
                     n_vec_in, Hi, Wi, C);
}

void geops_sgd_update(float* w, const float* g, float lr, float wd,
                      float rescale, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_sgd_update, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, w, g, lr, wd, rescale, n);
}

void geops_sgd_mom_update(float* w, const float* g, float* mom, float lr,
                          float momentum, float wd, float rescale,
                          long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_sgd_mom_update, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, w, g, mom, lr, momentum, wd,
                     rescale, n);
}

void geops_adam_update(float* w, const float* g, float* m, float* v,
                       float lr_t, float beta1, float beta2, float eps,
                       float wd, float rescale, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_adam_update, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, w, g, m, v, lr_t, beta1,
                     beta2, eps, wd, rescale, n);
}

void geops_rmsprop_update(float* w, const float* g, float* n_st, float lr,
                          float rho, float eps, float wd, float rescale,
                          long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_rmsprop_update, dim3(geops_blocks(n, 4)),
                     dim3(GEOPS_THREADS), 0, s, w, g, n_st, lr, rho, eps,
                     wd, rescale, n);
}

void geops_adagrad_update(float* w, const float* g, float* h, float lr,
                          float eps, float wd, float rescale, long long n,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_adagrad_update, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, w, g, h, lr, eps, wd,
                     rescale, n);
}

void geops_signsgd_update(float* w, const float* g, float lr, float wd,
                          float rescale, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_signsgd_update, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, w, g, lr, wd, rescale, n);
}

void geops_signum_update(float* w, const float* g, float* mom, float lr,
                         float momentum, float wd, float rescale,
                         long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_signum_update, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, w, g, mom, lr, momentum, wd,
                     rescale, n);
}

void geops_dcasgd_update(float* w, const float* g, float* prev_w, float* mom,
                         float lr, float lamda, float momentum, float wd,
                         float rescale, long long n, bool has_mom,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_dcasgd_update, dim3(geops_blocks(n)),
                     dim3(GEOPS_THREADS), 0, s, w, g, prev_w, mom, lr, lamda,
                     momentum, wd, rescale, n, has_mom);
}

}  // extern "C"
