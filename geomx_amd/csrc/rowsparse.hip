// gfx950 (MI355X / CDNA4) row-sparse kernels for the kvstore push path:
// deterministic duplicate merge, row scatter and row-indexed fused
// optimizer updates (the reference's AccumulateRowSparseGrads +
// row_sparse lazy_update optimizer ops, kvstore_dist_server.h:571).
//
// Conventions follow kernels.hip: wave64, <= 2048 blocks of 256 threads,
// grid-stride loops. One thread owns one (row slot, column granule) pair
// with lanes running along `width`, so a row is read and written as
// contiguous granules. VEC = 4 is the 16 B/lane path; the launcher takes
// it only when width % 4 == 0 and every base pointer is 16 B aligned
// (then every row base is too). VEC = 1 is the scalar path for odd widths
// and for views that start at an odd element offset.
//
// Element offsets are 64-bit throughout (row * width exceeds 2^31 on real
// embedding tables). Row ids outside [0, rows) — including the -1 padding
// of unused slots — are skipped and never turned into an address.
//
// Semantics match geomx_amd/ops/reference.py (rsp_* golden models).

#include <hip/hip_runtime.h>

#include <cstdint>
#include "optim_rules.h"

#define RSP_THREADS 256
#define RSP_MAX_BLOCKS 2048

static inline int rsp_blocks(long long work) {
  long long b = (work + RSP_THREADS - 1) / RSP_THREADS;
  if (b < 1) b = 1;
  if (b > RSP_MAX_BLOCKS) b = RSP_MAX_BLOCKS;
  return (int)b;
}

// ---------------------------------------------------------------------------
// rsp_merge: sum duplicate rows, deterministically and without atomics.
//
// Inputs are the STABLY sorted ids, the permutation that sorted them and
// seg[p] = index of the unique id that sorted position p belongs to
// (inclusive scan of the segment-head flags, minus one). The thread that
// lands on a segment head walks the whole segment and adds its rows one
// by one in sorted order, which — the sort being stable — is ascending
// ORIGINAL position: the same sequence the golden model adds in, so the
// fp32 result is bit-identical. Threads on non-head positions do nothing.
//
// Skew: a run of k equal ids is k serial adds in one thread. Accepted:
// splitting the segment would change the summation order.
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(RSP_THREADS) void k_rsp_merge(
    const long long* __restrict__ sorted_ids,
    const long long* __restrict__ perm,
    const long long* __restrict__ seg,
    const float* __restrict__ vals,
    long long* __restrict__ out_ids,
    float* __restrict__ out_vals,
    long long nnz, long long width) {
  const long long G = width / VEC;
  const long long total = nnz * G;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const long long p = t / G;
    const long long c = (t - p * G) * VEC;
    const long long u = seg[p];
    if (p > 0 && seg[p - 1] == u) continue;  // not a segment head
    Granule<VEC> acc;
    acc.load(vals + perm[p] * width + c);
    for (long long q = p + 1; q < nnz && seg[q] == u; ++q) {
      Granule<VEC> x;
      x.load(vals + perm[q] * width + c);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc.v[j] += x.v[j];
    }
    acc.store(out_vals + u * width + c);
    if (c == 0) out_ids[u] = sorted_ids[p];
  }
}

// ---------------------------------------------------------------------------
// rsp_scatter: dense[ids[u]] (+)= merged[u] for UNIQUE ids. Plain stores;
// accumulate is a non-atomic read-modify-write, safe because no two slots
// name the same row.
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(RSP_THREADS) void k_rsp_scatter(
    const long long* __restrict__ ids, const float* __restrict__ merged,
    float* __restrict__ dense, long long n_u, long long rows,
    long long width, bool accumulate) {
  const long long G = width / VEC;
  const long long total = n_u * G;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const long long u = t / G;
    const long long c = (t - u * G) * VEC;
    const long long r = ids[u];
    if (r < 0 || r >= rows) continue;
    Granule<VEC> g;
    g.load(merged + u * width + c);
    float* dst = dense + r * width + c;
    if (accumulate) {
      Granule<VEC> d;
      d.load(dst);
#pragma unroll
      for (int j = 0; j < VEC; ++j) g.v[j] = d.v[j] + g.v[j];
    }
    g.store(dst);
  }
}

// ---------------------------------------------------------------------------
// Row-indexed fused optimizer updates: a rule of optim_rules.h (the functor
// of that optimizer's dense kernel) on row ids[u] of w and of the states with
// gradient row merged[u]; rows no id names are never touched (lazy update).
// Own loads and stores, not optim_apply: through the helper the 16 B Adam
// instantiation fuses the other product of its moments (docs/kernels.md).
// ---------------------------------------------------------------------------
template <typename OP, int VEC>
__global__ __launch_bounds__(RSP_THREADS) void k_rsp_update(
    OP op, const long long* __restrict__ ids,
    const float* __restrict__ merged, float* __restrict__ w,
    float* __restrict__ s0, float* __restrict__ s1, long long n_u,
    long long rows, long long width) {
  const long long G = width / VEC;
  const long long total = n_u * G;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const long long u = t / G;
    const long long c = (t - u * G) * VEC;
    const long long r = ids[u];
    if (r < 0 || r >= rows) continue;
    const long long off = r * width + c;
    Granule<VEC> g, wv, a, b;
    g.load(merged + u * width + c);
    wv.load(w + off);
    if (OP::NSTATE >= 1) a.load(s0 + off);
    if (OP::NSTATE >= 2) b.load(s1 + off);
#pragma unroll
    for (int j = 0; j < VEC; ++j) op.apply(wv.v[j], g.v[j], a.v[j], b.v[j]);
    wv.store(w + off);
    if (OP::NSTATE >= 1) a.store(s0 + off);
    if (OP::NSTATE >= 2) b.store(s1 + off);
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

static inline bool rsp_al16(const void* p) {
  return p == nullptr || ((uintptr_t)p & 15) == 0;
}

template <typename OP>
static void rsp_launch_update(const OP& op, const long long* ids,
                              const float* merged, float* w, float* s0,
                              float* s1, long long n_u, long long rows,
                              long long width, hipStream_t s) {
  if (n_u <= 0 || width <= 0 || rows <= 0) return;  // zero grid is an error
  const bool vec = (width % 4 == 0) && rsp_al16(merged) && rsp_al16(w) &&
                   rsp_al16(s0) && rsp_al16(s1);
  if (vec) {
    hipLaunchKernelGGL((k_rsp_update<OP, 4>), dim3(rsp_blocks(n_u * (width / 4))),
                       dim3(RSP_THREADS), 0, s, op, ids, merged, w, s0, s1,
                       n_u, rows, width);
  } else {
    hipLaunchKernelGGL((k_rsp_update<OP, 1>), dim3(rsp_blocks(n_u * width)),
                       dim3(RSP_THREADS), 0, s, op, ids, merged, w, s0, s1,
                       n_u, rows, width);
  }
}

extern "C" {

void geops_rsp_merge(const long long* sorted_ids, const long long* perm,
                     const long long* seg, const float* vals,
                     long long* out_ids, float* out_vals, long long nnz,
                     long long width, hipStream_t s) {
  if (nnz <= 0 || width <= 0) return;
  if ((width % 4 == 0) && rsp_al16(vals) && rsp_al16(out_vals)) {
    hipLaunchKernelGGL((k_rsp_merge<4>), dim3(rsp_blocks(nnz * (width / 4))),
                       dim3(RSP_THREADS), 0, s, sorted_ids, perm, seg, vals,
                       out_ids, out_vals, nnz, width);
  } else {
    hipLaunchKernelGGL((k_rsp_merge<1>), dim3(rsp_blocks(nnz * width)),
                       dim3(RSP_THREADS), 0, s, sorted_ids, perm, seg, vals,
                       out_ids, out_vals, nnz, width);
  }
}

void geops_rsp_scatter(const long long* ids, const float* merged,
                       float* dense, long long n_u, long long rows,
                       long long width, bool accumulate, hipStream_t s) {
  if (n_u <= 0 || width <= 0 || rows <= 0) return;
  if ((width % 4 == 0) && rsp_al16(merged) && rsp_al16(dense)) {
    hipLaunchKernelGGL((k_rsp_scatter<4>), dim3(rsp_blocks(n_u * (width / 4))),
                       dim3(RSP_THREADS), 0, s, ids, merged, dense, n_u, rows,
                       width, accumulate);
  } else {
    hipLaunchKernelGGL((k_rsp_scatter<1>), dim3(rsp_blocks(n_u * width)),
                       dim3(RSP_THREADS), 0, s, ids, merged, dense, n_u, rows,
                       width, accumulate);
  }
}

void geops_rsp_sgd_update(const long long* ids, const float* merged,
                          float* w, float lr, float wd, float rescale,
                          long long n_u, long long rows, long long width,
                          hipStream_t s) {
  rsp_launch_update(SgdRule{lr, wd, rescale}, ids, merged, w, nullptr,
                    nullptr, n_u, rows, width, s);
}

void geops_rsp_sgd_mom_update(const long long* ids, const float* merged,
                              float* w, float* mom, float lr, float momentum,
                              float wd, float rescale, long long n_u,
                              long long rows, long long width,
                              hipStream_t s) {
  rsp_launch_update(SgdMomRule{lr, momentum, wd, rescale}, ids, merged, w,
                    mom, nullptr, n_u, rows, width, s);
}

void geops_rsp_adam_update(const long long* ids, const float* merged,
                           float* w, float* m, float* v, float lr_t,
                           float beta1, float beta2, float eps, float wd,
                           float rescale, long long n_u, long long rows,
                           long long width, hipStream_t s) {
  rsp_launch_update(AdamRule{lr_t, beta1, beta2, eps, wd, rescale}, ids,
                    merged, w, m, v, n_u, rows, width, s);
}

void geops_rsp_adagrad_update(const long long* ids, const float* merged,
                              float* w, float* h, float lr, float eps,
                              float wd, float rescale, long long n_u,
                              long long rows, long long width,
                              hipStream_t s) {
  rsp_launch_update(AdagradRule{lr, eps, wd, rescale}, ids, merged, w, h,
                    nullptr, n_u, rows, width, s);
}

}  // extern "C"
