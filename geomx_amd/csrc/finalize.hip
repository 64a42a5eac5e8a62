// Gradient finalize kernels for gfx950: the small parameters' gradients
// written where the trainer consumes them, in one launch per group of
// tensors instead of a cast, a gather or an add per tensor.
//
//   k_conv5_wrw_finalize        summed wrw slab [T16][CO] -> the weight
//                               gradient (OIHW logical order, any strides)
//                               and the bias gradient (slab row T16-16)
//   k_cast_many_f32_bf16        up to 8 fp32 tensors -> their bf16 copies
//                               (the casts autocast makes one at a time)
//   k_cast_many_bf16_f32_into   up to 8 bf16 tensors -> fp32 destinations
//   k_zero_many_f32             up to 8 fp32 ranges cleared
//
// Every store into a gradient destination is x + 0.0f, the value an
// accumulation `0 + x` into a cleared buffer has: a -0 becomes +0, all
// else keeps its bits (as k_fc_w_unpermute_into, fc.hip). Accesses are
// element-wise: a destination may start at any address aligned to its
// element inside a larger buffer. Nothing here sums.

#include <hip/hip_runtime.h>

#include <cstdint>

typedef unsigned short bf16_t;

#define FIN_THREADS 256
#define FIN_MAX_TENSORS 8
#define FIN_MAX_BLOCKS 256   // per tensor; the blocks stride over it

// the rounding of fc_f2bf (fc.hip): nearest even, NaN kept quiet
__device__ __forceinline__ bf16_t fin_f2bf(float f) {
  union { float f; unsigned int u; } cv;
  cv.f = f;
  if ((cv.u & 0x7FFFFFFFu) > 0x7F800000u)
    return (bf16_t)((cv.u >> 16) | 0x0040u);
  const unsigned int lsb = (cv.u >> 16) & 1;
  return (bf16_t)((cv.u + 0x7FFFu + lsb) >> 16);
}

__device__ __forceinline__ float fin_bf2f(bf16_t b) {
  union { unsigned int u; float f; } cv;
  cv.u = (unsigned int)b << 16;
  return cv.f;
}

// One thread per weight element e = ((o*CIr + ci)*5 + kh)*5 + kw, then
// one per output channel for the bias. idx[e] is the element's place in
// the slab (build_wrw_unpack_index); an index outside the slab reads
// nothing and stores NaN.
// dw / db may each be null (that gradient is not wanted).
__global__ __launch_bounds__(FIN_THREADS) void k_conv5_wrw_finalize(
    const float* __restrict__ full, const long long* __restrict__ idx,
    float* __restrict__ dw, float* __restrict__ db, int CO, int CIr, int T16,
    long long s_o, long long s_i, long long s_h, long long s_w) {
  const int numel = CO * CIr * 25;
  const int e = blockIdx.x * FIN_THREADS + threadIdx.x;
  if (e < numel) {
    if (dw == nullptr) return;
    const int kw = e % 5, kh = (e / 5) % 5;
    const int ci = (e / 25) % CIr, o = e / (25 * CIr);
    const long long j = idx[e];
    const bool in = j >= 0 && j < (long long)T16 * CO;
    dw[o * s_o + ci * s_i + kh * s_h + kw * s_w] =
        in ? full[j] + 0.0f : __builtin_nanf("");
  } else if (e < numel + CO) {
    if (db == nullptr) return;
    const int o = e - numel;
    db[o] = full[(long long)(T16 - 16) * CO + o] + 0.0f;
  }
}

struct FinTable {
  const void* src[FIN_MAX_TENSORS];
  void* dst[FIN_MAX_TENSORS];
  long long n[FIN_MAX_TENSORS];
};

// grid (blocks, tensors): blockIdx.y picks the table entry, the blocks
// of a row stride over its n elements.
__global__ __launch_bounds__(FIN_THREADS) void k_cast_many_f32_bf16(
    const FinTable t) {
  const int k = blockIdx.y;
  const float* __restrict__ src = (const float*)t.src[k];
  bf16_t* __restrict__ dst = (bf16_t*)t.dst[k];
  const long long n = t.n[k];
  for (long long i = (long long)blockIdx.x * FIN_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * FIN_THREADS)
    dst[i] = fin_f2bf(src[i]);
}

__global__ __launch_bounds__(FIN_THREADS) void k_cast_many_bf16_f32_into(
    const FinTable t) {
  const int k = blockIdx.y;
  const bf16_t* __restrict__ src = (const bf16_t*)t.src[k];
  float* __restrict__ dst = (float*)t.dst[k];
  const long long n = t.n[k];
  for (long long i = (long long)blockIdx.x * FIN_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * FIN_THREADS)
    dst[i] = fin_bf2f(src[i]) + 0.0f;
}

__global__ __launch_bounds__(FIN_THREADS) void k_zero_many_f32(
    const FinTable t) {
  const int k = blockIdx.y;
  float* __restrict__ dst = (float*)t.dst[k];
  const long long n = t.n[k];
  for (long long i = (long long)blockIdx.x * FIN_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * FIN_THREADS)
    dst[i] = 0.0f;
}

extern "C" {

// Returns 0 on launch, -1 for a geometry outside the table (nothing is
// launched). The wrw kernels serve (CI, CO) in {(4,16), (16,32), (16,16)}
// with T16 = 176 or 416; the finalize only needs positive extents.
int geops_conv5_wrw_finalize(const float* full, const long long* idx,
                             float* dw, float* db, int CO, int CIr, int T16,
                             long long s_o, long long s_i, long long s_h,
                             long long s_w, hipStream_t s) {
  if (CO <= 0 || CIr <= 0 || T16 < 16 || CO > 1024 || CIr > 1024) return -1;
  const int work = CO * CIr * 25 + CO;
  hipLaunchKernelGGL(k_conv5_wrw_finalize,
                     dim3((work + FIN_THREADS - 1) / FIN_THREADS),
                     dim3(FIN_THREADS), 0, s, full, idx, dw, db, CO, CIr, T16,
                     s_o, s_i, s_h, s_w);
  return 0;
}

// kind 0: fp32 -> bf16, 1: bf16 -> fp32 as x + 0.0f, 2: clear fp32 (src
// unused). count in 1..8, every n >= 0 and at least one positive.
int geops_many(int kind, int count, const void* const* src, void* const* dst,
               const long long* n, hipStream_t s) {
  if (count < 1 || count > FIN_MAX_TENSORS || kind < 0 || kind > 2) return -1;
  FinTable t;
  long long most = 0;
  for (int k = 0; k < FIN_MAX_TENSORS; ++k) {
    t.src[k] = k < count && src != nullptr ? src[k] : nullptr;
    t.dst[k] = k < count ? dst[k] : nullptr;
    t.n[k] = k < count ? n[k] : 0;
    if (t.n[k] < 0) return -1;
    if (t.n[k] > most) most = t.n[k];
  }
  if (most == 0) return -1;
  long long blocks = (most + FIN_THREADS - 1) / FIN_THREADS;
  if (blocks > FIN_MAX_BLOCKS) blocks = FIN_MAX_BLOCKS;
  const dim3 grid((unsigned)blocks, (unsigned)count);
  if (kind == 0)
    hipLaunchKernelGGL(k_cast_many_f32_bf16, grid, dim3(FIN_THREADS), 0, s, t);
  else if (kind == 1)
    hipLaunchKernelGGL(k_cast_many_bf16_f32_into, grid, dim3(FIN_THREADS), 0,
                       s, t);
  else
    hipLaunchKernelGGL(k_zero_many_f32, grid, dim3(FIN_THREADS), 0, s, t);
  return 0;
}

}  // extern "C"
