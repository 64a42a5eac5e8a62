// gfx950 (MI355X / CDNA4) FP8 wire tier: block-scaled OCP E4M3 with error
// feedback, the tier between the fp16 wire and the 4-bit one. Both sides of
// the wire are here: k_fp8_encode (send) and k_wire_sum_fp8 (fused receive).
//
// Payload of n elements at chunk size C (a power of two in [64, 8192]),
// nchunks = ceil(n / C), one uint8 tensor:
//
//   codes  u8 [nchunks][C]   E4M3 codes, whole rows (positions >= n code 0)
//   scales u8 [nchunks]      e + 127, the chunk's power-of-two exponent
//   zeros up to a multiple of 16 bytes
//
// Encode of one chunk of c = x + r (one rounded add; r is the residual):
//   amax = max |c|;  amax == 0: e = -127;  else amax = m * 2^E, 1 <= m < 2:
//   e = (m <= 1.75 ? E - 8 : E - 7) clamped to [-127, 127]
// so amax * 2^-e <= 448, the largest E4M3 value: no convert saturates and no
// NaN code is produced. code = RNE(c * 2^-e), d = float(code) * 2^e, and the
// new residual is c - d (one rounded subtraction). Both scalings are by
// powers of two and exact: float(code) * 2^e is at least 2^-9 * 2^-127, a
// subnormal fp32, and a c * 2^-e that underflows fp32 is far below half the
// smallest E4M3 subnormal (2^-10) and codes 0 either way. The kernels run
// with fp32 subnormals on (the gfx9 default); 2^-127 itself is one.
//
// k_fp8_encode<LOG2C, HAS_R>. A lane owns granules of 16 consecutive
// elements: four 16 B loads of x (and of r), one 16 B store of codes, four
// 16 B stores of r. A chunk is owned by LPC = min(C / 16, 64) lanes of ONE
// wave, G = C / 16 / LPC granules per lane (granule lic + j * LPC):
//   C    64 ..  512: 4 .. 32 lanes, G = 1, 64 .. 8 chunks per workgroup;
//   C  1024 .. 8192: the whole wave, G = 1 .. 8, 4 chunks per workgroup.
// The chunk lives in registers as c from its loads to its stores; x and r
// are summed as they arrive, so a lane holds 16 G floats, not 32 G. No chunk
// spans waves: there is no LDS, no barrier and no workspace. amax is the
// integer maximum of the |c| bit patterns (ordered like the values), folded
// over the lane's elements and then by an xor butterfly over the LPC lanes
// (DPP inside a row of 16, ds_bpermute across rows); every lane ends with the
// chunk's amax and derives e from its exponent and mantissa fields. Four
// codes fill a dword through two v_cvt_pk_fp8_f32. The lane lic == 0 stores
// the scale byte (a plain byte store), and the lane that owns the last chunk
// also clears the alignment bytes behind the scales.
//
// k_wire_sum_fp8<NP>, under the fold contract of wirereduce.hip:
//   out[i] = (accumulate ? out[i] : +0) + d_0[i] + ... + d_{P-1}[i]
// left to right, every add rounded (d_p[i] is exact, see above), bit-equal
// to `acc = zeros; for p: acc += decode(p)`. Party pointers by value
// (WireTab), groups of 16 with accumulate set after the first. A lane owns
// granule q (elements 16 q .. 16 q + 15): per party one 16 B load of codes and
// one byte load of the scale of chunk 16 q / C (C >= 64, so one scale serves
// the granule; neighbouring lanes read the same byte). All 2 NP loads are
// issued before the first decode. Four float4 stores; a granule that crosses
// n stores its elements below n one by one, so nothing at or past n is
// written.
//
// Conventions follow kernels.hip: wave64, <= GEOPS_MAX_BLOCKS workgroups of
// 256 threads, grid-stride loops, 64-bit element offsets. Built without
// packed fp32 instructions (setup.py) and with contraction off: the add of
// the residual, the subtraction of the decoded value and the adds of the
// fold are single rounded operations.

#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048
#define WIRE_MAX_PARTIES 16

struct WireTab {
  const void* p[WIRE_MAX_PARTIES];
};

// ---------------------------------------------------------------------------
// Codec
// ---------------------------------------------------------------------------

// 2^e for e in [-127, 127]; 2^-127 is the subnormal 0x00400000
__device__ __forceinline__ float pow2f(int e) {
  return __uint_as_float(e > -127 ? (uint32_t)(e + 127) << 23 : 0x00400000u);
}

// the chunk exponent of amax, given as the bits of |amax|
__device__ __forceinline__ int fp8_exponent(uint32_t abits) {
  const int E = (int)(abits >> 23) - 127;
  const int e = E - 8 + ((abits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return e < -127 ? -127 : e;  // zero and subnormal amax land here
}

// four E4M3 codes of a dword, decoded and scaled (exact)
__device__ __forceinline__ float4 fp8_decode4(uint32_t w, float scale) {
  float4 d;
  d.x = __builtin_amdgcn_cvt_f32_fp8((int)w, 0) * scale;
  d.y = __builtin_amdgcn_cvt_f32_fp8((int)w, 1) * scale;
  d.z = __builtin_amdgcn_cvt_f32_fp8((int)w, 2) * scale;
  d.w = __builtin_amdgcn_cvt_f32_fp8((int)w, 3) * scale;
  return d;
}

// ---------------------------------------------------------------------------
// Encode
// ---------------------------------------------------------------------------

template <int LOG2C>
struct Fp8Shape {
  static constexpr int CHUNK = 1 << LOG2C;
  static constexpr int GPC = CHUNK / 16;            // granules per chunk
  static constexpr int LPC = GPC < 64 ? GPC : 64;   // lanes per chunk
  static constexpr int G = GPC / LPC;               // granules per lane
  static constexpr int CPW = GEOPS_THREADS / LPC;   // chunks per workgroup
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

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) {
  return a > b ? a : b;
}

// maximum over aligned groups of W lanes (4 .. 64) of a wave; every lane ends
// with the group's result. All lanes of the wave must be active.
template <int W>
__device__ __forceinline__ uint32_t group_umax(uint32_t m) {
  m = umax(m, dpp_u32<DPP_XOR1>(m));
  m = umax(m, dpp_u32<DPP_XOR2>(m));
  if constexpr (W >= 8) m = umax(m, dpp_u32<DPP_ROW_HALF_MIRROR>(m));
  if constexpr (W >= 16) m = umax(m, dpp_u32<DPP_ROW_MIRROR>(m));
  if constexpr (W >= 32) m = umax(m, (uint32_t)__shfl_xor((int)m, 16, 64));
  if constexpr (W >= 64) m = umax(m, (uint32_t)__shfl_xor((int)m, 32, 64));
  return m;
}

__device__ __forceinline__ uint32_t abs_bits(float f) {
  return __float_as_uint(f) & 0x7FFFFFFFu;
}

template <int LOG2C, bool HAS_R>
__global__ __launch_bounds__(GEOPS_THREADS) void k_fp8_encode(
    const float* __restrict__ x, float* __restrict__ residual,
    uint8_t* __restrict__ payload, long long n, int nchunks,
    long long payload_bytes) {
  using S = Fp8Shape<LOG2C>;
  constexpr int G = S::G, LPC = S::LPC;
  const int lic = threadIdx.x & (LPC - 1);  // lane in chunk
  const int grp = threadIdx.x / LPC;        // chunk of this trip
  uint8_t* scales = payload + ((long long)nchunks << LOG2C);

  // every lane of the workgroup runs every trip (the butterfly needs whole
  // waves); a group past the last chunk loads nothing and stores nothing
  for (long long base = (long long)blockIdx.x * S::CPW; base < nchunks;
       base += (long long)gridDim.x * S::CPW) {
    const long long cl = base + grp;
    const bool live = cl < nchunks;
    const long long e0 = cl << LOG2C;  // first element of the chunk

    // 1. the chunk: c = x + r, 16 elements per granule
    float c[G][16];
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const long long e = e0 + 16ll * (lic + j * LPC);
      if (live && e + 16 <= n) {
        float4 xv[4], rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xv[i] = reinterpret_cast<const float4*>(x + e)[i];
          if (HAS_R) rv[i] = reinterpret_cast<const float4*>(residual + e)[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          c[j][4 * i] = HAS_R ? xv[i].x + rv[i].x : xv[i].x;
          c[j][4 * i + 1] = HAS_R ? xv[i].y + rv[i].y : xv[i].y;
          c[j][4 * i + 2] = HAS_R ? xv[i].z + rv[i].z : xv[i].z;
          c[j][4 * i + 3] = HAS_R ? xv[i].w + rv[i].w : xv[i].w;
        }
      } else {
        // the granule that crosses n, and everything behind it: 0 past n
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const bool in = live && e + i < n;
          const float xi = in ? x[e + i] : 0.0f;
          c[j][i] = (HAS_R && in) ? xi + residual[e + i] : xi;
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) amax = umax(amax, abs_bits(c[j][i]));
    }

    // 2. amax over the chunk's lanes, the exponent from its fields
    amax = group_umax<LPC>(amax);
    if (!live) continue;
    const int ex = fp8_exponent(amax);
    const float inv = pow2f(-ex);  // -ex in [-120, 127]: a normal float
    const float scale = pow2f(ex);

    // 3. codes and residual
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const long long e = e0 + 16ll * (lic + j * LPC);
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(c[j][4 * i] * inv,
                                                 c[j][4 * i + 1] * inv, 0,
                                                 false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(c[j][4 * i + 2] * inv,
                                             c[j][4 * i + 3] * inv, pk, true);
        w[i] = (uint32_t)pk;
      }
      // rows are whole: e + 16 <= nchunks * CHUNK
      *reinterpret_cast<uint4*>(payload + e) =
          make_uint4(w[0], w[1], w[2], w[3]);
      if (HAS_R) {
        if (e + 16 <= n) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 d = fp8_decode4(w[i], scale);
            reinterpret_cast<float4*>(residual + e)[i] =
                make_float4(c[j][4 * i] - d.x, c[j][4 * i + 1] - d.y,
                            c[j][4 * i + 2] - d.z, c[j][4 * i + 3] - d.w);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 d = fp8_decode4(w[i], scale);
            const long long f = e + 4 * i;
            if (f < n) residual[f] = c[j][4 * i] - d.x;
            if (f + 1 < n) residual[f + 1] = c[j][4 * i + 1] - d.y;
            if (f + 2 < n) residual[f + 2] = c[j][4 * i + 2] - d.z;
            if (f + 3 < n) residual[f + 3] = c[j][4 * i + 3] - d.w;
          }
        }
      }
    }
    if (lic == 0) {
      scales[cl] = (uint8_t)(ex + 127);
      if (cl == nchunks - 1) {
        // alignment bytes behind the scales (at most 15)
        for (long long b = ((long long)nchunks << LOG2C) + nchunks;
             b < payload_bytes; ++b)
          payload[b] = 0;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Fused receive: decode and sum all parties
// ---------------------------------------------------------------------------

__device__ __forceinline__ void add4(float4& a, const float4& c) {
  a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
}

template <int NP>
__global__ __launch_bounds__(GEOPS_THREADS) void k_wire_sum_fp8(
    WireTab tab, float* __restrict__ out, long long n, int log2c, int nchunks,
    bool accumulate) {
  const long long tid = (long long)blockIdx.x * GEOPS_THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * GEOPS_THREADS;
  const long long nq = (n + 15) >> 4;  // granules with an element below n
  const long long scale_off = (long long)nchunks << log2c;
  for (long long q = tid; q < nq; q += stride) {
    const long long e = q << 4;
    // e < n <= nchunks * chunk: the granule is inside the code rows and
    // chunk e >> log2c has a scale byte
    const long long ch = e >> log2c;
    uint4 h[NP];
    uint32_t sb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const uint8_t* in = static_cast<const uint8_t*>(tab.p[p]);
      h[p] = reinterpret_cast<const uint4*>(in)[q];
      sb[p] = in[scale_off + ch];
    }
    const bool whole = e + 16 <= n;
    float4 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (accumulate) {
      if (whole) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a[i] = reinterpret_cast<const float4*>(out + e)[i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long f = e + 4 * i;
          if (f < n) a[i].x = out[f];
          if (f + 1 < n) a[i].y = out[f + 1];
          if (f + 2 < n) a[i].z = out[f + 2];
          if (f + 3 < n) a[i].w = out[f + 3];
        }
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float scale = pow2f((int)sb[p] - 127);
      add4(a[0], fp8_decode4(h[p].x, scale));
      add4(a[1], fp8_decode4(h[p].y, scale));
      add4(a[2], fp8_decode4(h[p].z, scale));
      add4(a[3], fp8_decode4(h[p].w, scale));
    }
    if (whole) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        reinterpret_cast<float4*>(out + e)[i] = a[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long f = e + 4 * i;
        if (f < n) out[f] = a[i].x;
        if (f + 1 < n) out[f + 1] = a[i].y;
        if (f + 2 < n) out[f + 2] = a[i].z;
        if (f + 3 < n) out[f + 3] = a[i].w;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------

template <int LOG2C>
static void launch_fp8_encode(const float* x, float* residual,
                              uint8_t* payload, long long n, int nchunks,
                              long long payload_bytes, hipStream_t s) {
  using S = Fp8Shape<LOG2C>;
  long long nb = ((long long)nchunks + S::CPW - 1) / S::CPW;
  if (nb > GEOPS_MAX_BLOCKS) nb = GEOPS_MAX_BLOCKS;
  if (residual)
    hipLaunchKernelGGL((k_fp8_encode<LOG2C, true>), dim3((int)nb),
                       dim3(GEOPS_THREADS), 0, s, x, residual, payload, n,
                       nchunks, payload_bytes);
  else
    hipLaunchKernelGGL((k_fp8_encode<LOG2C, false>), dim3((int)nb),
                       dim3(GEOPS_THREADS), 0, s, x, residual, payload, n,
                       nchunks, payload_bytes);
}

template <int NP>
static void launch_sum_fp8(int np, const WireTab& tab, float* out,
                           long long n, int log2c, int nchunks, bool acc,
                           hipStream_t s) {
  if (np == NP) {
    long long nb = (((n + 15) >> 4) + GEOPS_THREADS - 1) / GEOPS_THREADS;
    if (nb > GEOPS_MAX_BLOCKS) nb = GEOPS_MAX_BLOCKS;
    hipLaunchKernelGGL((k_wire_sum_fp8<NP>), dim3((int)nb),
                       dim3(GEOPS_THREADS), 0, s, tab, out, n, log2c, nchunks,
                       acc);
  } else if constexpr (NP > 1) {
    launch_sum_fp8<NP - 1>(np, tab, out, n, log2c, nchunks, acc, s);
  }
}

static int fp8_log2_chunk(int chunk) {
  for (int l = 6; l <= 13; ++l)
    if (chunk == 1 << l) return l;
  return -1;
}

extern "C" {

// bytes of the payload of n elements: code rows, scales, padded to 16
long long geops_fp8_wire_bytes(long long n, int chunk) {
  const long long nchunks = (n + chunk - 1) / chunk;
  return (nchunks * chunk + nchunks + 15) / 16 * 16;
}

// chunk: a power of two in [64, 8192]; 1 <= n < 2^31; x, residual (may be
// null: no error feedback) and payload on 16 B boundaries; payload holds
// geops_fp8_wire_bytes(n, chunk) bytes. Returns -1 for a chunk outside the
// served range (the binding checks it first).
int geops_fp8_encode(const float* x, float* residual, uint8_t* payload,
                     long long n, int chunk, hipStream_t s) {
  const int nchunks = (int)((n + chunk - 1) / chunk);
  const long long bytes = geops_fp8_wire_bytes(n, chunk);
#define FP8_ENCODE_CASE(L)                                                \
  case L:                                                                 \
    launch_fp8_encode<L>(x, residual, payload, n, nchunks, bytes, s);     \
    return 0;
  switch (fp8_log2_chunk(chunk)) {
    FP8_ENCODE_CASE(6)
    FP8_ENCODE_CASE(7)
    FP8_ENCODE_CASE(8)
    FP8_ENCODE_CASE(9)
    FP8_ENCODE_CASE(10)
    FP8_ENCODE_CASE(11)
    FP8_ENCODE_CASE(12)
    FP8_ENCODE_CASE(13)
  }
#undef FP8_ENCODE_CASE
  return -1;
}

// payloads: P device pointers (host array), each a payload of n elements at
// this chunk on a 16 B boundary. Groups of WIRE_MAX_PARTIES.
int geops_wire_sum_fp8(const void* const* payloads, int P, float* out,
                       long long n, int chunk, bool accumulate,
                       hipStream_t s) {
  const int log2c = fp8_log2_chunk(chunk);
  if (log2c < 0) return -1;
  const int nchunks = (int)((n + chunk - 1) / chunk);
  for (int p0 = 0; p0 < P; p0 += WIRE_MAX_PARTIES) {
    const int np = P - p0 < WIRE_MAX_PARTIES ? P - p0 : WIRE_MAX_PARTIES;
    WireTab tab = {};
    for (int j = 0; j < np; ++j) tab.p[j] = payloads[p0 + j];
    launch_sum_fp8<WIRE_MAX_PARTIES>(np, tab, out, n, log2c, nchunks,
                                     accumulate || p0 > 0, s);
  }
  return 0;
}

}  // extern "C"
