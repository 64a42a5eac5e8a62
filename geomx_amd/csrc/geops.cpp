// Torch bindings for the geomx_amd gfx950 kernel library: kernels.hip
// (kvstore compression, optimizer updates, fused ReLU+pool), conv.hip
// (5x5 conv forward / data gradient), wirereduce.hip (fused decode-and-sum
// of all parties' wire payloads), wiresparse.hip (the same for the Bi-Sparse
// lists), dgtencode.hip (fused DGT mode-3 encode), bscselect.hip (Bi-Sparse
// boundary select),
// convwrw2.hip (5x5 conv weight gradient, tr16 probes) and fc.hip
// (NHWC-native first dense layer layout kernels: permuting weight casts,
// transposing flatten), lars.hip (layer-wise LARS: segmented sums of squares
// and the per-segment sgd update).
//
// Thin checked wrappers: dtype/contiguity/device checks, stream plumbing
// (kernels run on the current torch stream so they order correctly with
// autograd/backward and RCCL collectives), and workspace management for
// the Bi-Sparse pack pipeline.

#include <torch/extension.h>

#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

// C-ABI launchers from the .hip files
extern "C" {
void geops_quantize_2bit(const float*, float*, uint32_t*, long long, float,
                         hipStream_t);
void geops_dequantize_2bit(const uint32_t*, float*, long long, float,
                           hipStream_t);
void geops_bsc_momentum(const float*, float*, float*, float, long long,
                        hipStream_t);
void geops_bsc_pack(const float*, float*, float*, float*, int*, long long*,
                    float, long long, long long, float, bool, hipStream_t);
void geops_bsc_pull_pack(const float*, float*, int*, long long*, long long,
                         long long, float, hipStream_t);
int geops_bsc_fused(const float*, float*, float*, float*, int*, const float*,
                    unsigned long long*, float, long long, long long, float,
                    hipStream_t);
void geops_bsc_unpack(const float*, const int*, float*, long long, long long,
                      bool, hipStream_t);
void geops_dgt_contribution(const float*, float*, long long, int, int,
                            hipStream_t);
void geops_quantize_4bit(const float*, float*, uint8_t*, float*, long long,
                         int, int, bool, hipStream_t);
void geops_dequantize_4bit(const uint8_t*, const float*, float*, long long,
                           int, hipStream_t);
void geops_sgd_update(float*, const float*, float, float, float, long long,
                      hipStream_t);
void geops_sgd_mom_update(float*, const float*, float*, float, float, float,
                          float, long long, hipStream_t);
void geops_adam_update(float*, const float*, float*, float*, float, float,
                       float, float, float, float, long long, hipStream_t);
void geops_dcasgd_update(float*, const float*, float*, float*, float, float,
                         float, float, float, long long, bool, hipStream_t);
void geops_rmsprop_update(float*, const float*, float*, float, float, float,
                          float, float, long long, hipStream_t);
void geops_adagrad_update(float*, const float*, float*, float, float, float,
                          float, long long, hipStream_t);
void geops_signsgd_update(float*, const float*, float, float, float,
                          long long, hipStream_t);
void geops_signum_update(float*, const float*, float*, float, float, float,
                         float, long long, hipStream_t);
// lars.hip
int geops_lars_tile();
void geops_lars_sumsq(const float*, const float*, const long long*,
                      const long long*, float*, float*, int, long long,
                      long long, double, int, int, hipStream_t);
void geops_lars_update(float*, const float*, float*, const long long*,
                       const long long*, const float*, int, long long,
                       long long, double, double, float, float, float, int,
                       int, hipStream_t);
// wirereduce.hip
void geops_wire_sum_2bit(const void* const*, int, float*, long long, float,
                         bool, hipStream_t);
void geops_wire_sum_f16(const void* const*, int, float*, long long, bool,
                        hipStream_t);
void geops_wire_sum_dgt(const float* const*, const int* const*,
                        const uint8_t* const*, const float* const*, int,
                        float*, long long, int, int, int, bool, hipStream_t);
// wiresparse.hip
int geops_wire_sum_bsc_tile();
void geops_wire_sum_bsc(const float* const*, const int* const*, int, int,
                        float*, long long, bool, hipStream_t);
void geops_wire_sum_bsc_dgt(const float* const*, const int* const*,
                            const uint8_t* const*, const float* const*,
                            const int* const*, int, int, int, int, float*,
                            long long, bool, hipStream_t);
// dgtencode.hip
int geops_dgt_encode(const float*, float*, const float*, const int*, float*,
                     uint8_t*, float*, long long, int, int, int, hipStream_t);
// wirefp8.hip
long long geops_fp8_wire_bytes(long long, int);
int geops_fp8_encode(const float*, float*, uint8_t*, long long, int,
                     hipStream_t);
int geops_wire_sum_fp8(const void* const*, int, float*, long long, int, bool,
                       hipStream_t);
// bscselect.hip
int geops_bsc_boundary_cap();
int geops_bsc_boundary_grid(long long, int);
long long geops_bsc_boundary_ws_words(long long);
void geops_bsc_boundary(const float*, const float*, const float*, const int*,
                        long long, long long, long long, float, float*,
                        uint32_t*, int, hipStream_t);
// rowsparse.hip
void geops_rsp_merge(const long long*, const long long*, const long long*,
                     const float*, long long*, float*, long long, long long,
                     hipStream_t);
void geops_rsp_scatter(const long long*, const float*, float*, long long,
                       long long, long long, bool, hipStream_t);
void geops_rsp_sgd_update(const long long*, const float*, float*, float,
                          float, float, long long, long long, long long,
                          hipStream_t);
void geops_rsp_sgd_mom_update(const long long*, const float*, float*, float*,
                              float, float, float, float, long long,
                              long long, long long, hipStream_t);
void geops_rsp_adam_update(const long long*, const float*, float*, float*,
                           float*, float, float, float, float, float, float,
                           long long, long long, long long, hipStream_t);
void geops_rsp_adagrad_update(const long long*, const float*, float*, float*,
                              float, float, float, float, long long,
                              long long, long long, hipStream_t);
void geops_relu_maxpool2_fwd(const unsigned short*, unsigned short*, uint8_t*,
                             long long, int, int, int, hipStream_t);
void geops_relu_maxpool2_bwd(const unsigned short*, const uint8_t*,
                             unsigned short*, long long, int, int, int,
                             hipStream_t);
int geops_conv5_nhwc(const unsigned short*, const unsigned short*,
                     const float*, unsigned short*, int, int, int, int, int,
                     int, int, int, hipStream_t);
int geops_conv5_pool_nhwc(const unsigned short*, const unsigned short*,
                          const float*, unsigned short*, uint8_t*, int, int,
                          int, int, int, int, int, hipStream_t);
int geops_conv5_pool_nwg_nhwc(const unsigned short*, const unsigned short*,
                              const float*, unsigned short*, uint8_t*, int,
                              int, int, int, int, int, int, int, hipStream_t);
int geops_conv5_pool_x32_nhwc(const float*, const unsigned short*,
                              const float*, unsigned short*, uint8_t*,
                              unsigned short*, int, int, int, int, int, int,
                              int, hipStream_t);
int geops_conv5_pool_u8_nhwc(const uint8_t*, const unsigned short*,
                             const unsigned short*, const float*,
                             unsigned short*, uint8_t*, unsigned short*, int,
                             int, int, int, int, int, int, hipStream_t);
void geops_pad_ch3to4_nhwc(const void*, unsigned short*, long long, int,
                           hipStream_t);
int geops_conv5_pack_frags(const float*, long long, const long long*,
                           unsigned short*, long long, const long long*,
                           unsigned short*, long long, hipStream_t);
int geops_conv5_wrw16_nhwc(const unsigned short*, const unsigned short*,
                           float*, int, int, int, int, int, int, int, int,
                           hipStream_t);
int geops_conv5_wrw4_nhwc(const unsigned short*, const unsigned short*,
                          float*, int, int, int, int, int, int, int, int,
                          hipStream_t);
int geops_conv5_wrw_unpool_nhwc(const unsigned short*, const unsigned short*,
                                const uint8_t*, float*, int, int, int, int,
                                int, int, int, int, hipStream_t);
int geops_conv5_dgrad_unpool_nhwc(const unsigned short*, const uint8_t*,
                                  const unsigned short*, unsigned short*,
                                  int, int, int, int, int, int, int,
                                  hipStream_t);
int geops_conv5_direct_nhwc(const unsigned short*, const unsigned short*,
                            const float*, unsigned short*, int, int, int, int,
                            int, int, int, hipStream_t);
int geops_conv5_dgrad_nwg_nhwc(const unsigned short*, const uint8_t*,
                               const unsigned short*, unsigned short*, int,
                               int, int, int, int, int, int, int,
                               hipStream_t);
int geops_conv5c1_pool(const void*, int, const unsigned short*,
                       const unsigned short*, const float*, unsigned short*,
                       uint8_t*, int, int, int, int, hipStream_t);
int geops_conv5c1_wrw(const void*, int, const unsigned short*,
                      const unsigned short*, const uint8_t*, float*, int, int,
                      int, int, hipStream_t);
int geops_fc_w_permute_bf16(const float*, unsigned short*, int, int, int,
                            hipStream_t);
int geops_fc_w_unpermute_f32(const unsigned short*, float*, int, int, int,
                             hipStream_t);
int geops_fc_flatten_nchw(const unsigned short*, unsigned short*, int, int,
                          int, hipStream_t);
int geops_fc_w_pack2_bf16(const float*, unsigned short*, unsigned short*,
                          int, int, int, hipStream_t);
int geops_fc_w_unpermute_into(const unsigned short*, float*, int, int, int,
                              hipStream_t);
int geops_conv5_wrw_finalize(const float*, const long long*, float*, float*,
                             int, int, int, long long, long long, long long,
                             long long, hipStream_t);
int geops_many(int, int, const void* const*, void* const*, const long long*,
               hipStream_t);
void geops_tr16_probe(const unsigned short*, unsigned short*, hipStream_t);
void geops_tr16_probe2(const unsigned short*, const int*, unsigned short*,
                       hipStream_t);
}

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

// surface async launch errors at the call site instead of a later,
// unrelated synchronize
void launch_check(const char* what) {
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, what, ": kernel launch failed: ",
              hipGetErrorString(e));
}

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, name,
              " must be 16-byte aligned");
}

// the dense optimizer kernels take their length from w: g and every state
// must hold as many elements, or the kernel reads and writes past them
void check_same_numel(const torch::Tensor& w, const torch::Tensor& t,
                      const char* name) {
  TORCH_CHECK(t.numel() == w.numel(), name, " must have as many elements as w"
              " (", t.numel(), " vs ", w.numel(), ")");
}

// Adam's bias-corrected rate at step t, in double
double adam_lr_t(double lr, double beta1, double beta2, int64_t t) {
  return lr * std::sqrt(1.0 - std::pow(beta2, (double)t)) /
         (1.0 - std::pow(beta1, (double)t));
}

void quantize_2bit(torch::Tensor grad, torch::Tensor residual,
                   torch::Tensor out, double thr) {
  check_f32(grad, "grad");
  check_f32(residual, "residual");
  TORCH_CHECK(out.scalar_type() == torch::kInt32 && out.is_contiguous());
  const long long n = grad.numel();
  TORCH_CHECK(residual.numel() == n);
  TORCH_CHECK(out.numel() == (n + 15) / 16);
  geops_quantize_2bit(grad.data_ptr<float>(), residual.data_ptr<float>(),
                      (uint32_t*)out.data_ptr<int32_t>(), n, (float)thr,
                      cur_stream());
  launch_check("quantize_2bit");
}

void dequantize_2bit(torch::Tensor packed, torch::Tensor out, double thr) {
  check_f32(out, "out");
  TORCH_CHECK(packed.scalar_type() == torch::kInt32 && packed.is_contiguous());
  const long long n = out.numel();
  TORCH_CHECK(packed.numel() >= (n + 15) / 16);
  geops_dequantize_2bit((const uint32_t*)packed.data_ptr<int32_t>(),
                        out.data_ptr<float>(), n, (float)thr, cur_stream());
  launch_check("dequantize_2bit");
}

void bsc_momentum(torch::Tensor g, torch::Tensor u, torch::Tensor v,
                  double mu) {
  check_f32(g, "g"); check_f32(u, "u"); check_f32(v, "v");
  const long long n = g.numel();
  TORCH_CHECK(u.numel() == n && v.numel() == n);
  geops_bsc_momentum(g.data_ptr<float>(), u.data_ptr<float>(),
                     v.data_ptr<float>(), (float)mu, n, cur_stream());
  launch_check("bsc_momentum");
}

torch::Tensor make_workspace(const torch::Tensor& like) {
  return torch::empty({2049}, torch::TensorOptions()
                                  .dtype(torch::kInt64)
                                  .device(like.device()));
}

void bsc_pack(torch::Tensor v, torch::Tensor u, torch::Tensor vals,
              torch::Tensor idx, double boundary, double placeholder) {
  check_f32(v, "v"); check_f32(u, "u"); check_f32(vals, "vals");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous());
  TORCH_CHECK(vals.numel() == idx.numel());
  auto ws = make_workspace(v);
  geops_bsc_pack(v.data_ptr<float>(), v.data_ptr<float>(),
                 u.data_ptr<float>(), vals.data_ptr<float>(),
                 idx.data_ptr<int32_t>(), (long long*)ws.data_ptr<int64_t>(),
                 (float)boundary, v.numel(), vals.numel(),
                 (float)placeholder, /*zero_uv=*/true, cur_stream());
  launch_check("bsc_pack");
}

bool bsc_compress_fused(torch::Tensor g, torch::Tensor u, torch::Tensor v,
                        torch::Tensor vals, torch::Tensor idx,
                        torch::Tensor boundary, double mu,
                        double placeholder) {
  check_f32(g, "g"); check_f32(u, "u"); check_f32(v, "v");
  check_f32(vals, "vals"); check_f32(boundary, "boundary");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous());
  TORCH_CHECK(vals.numel() == idx.numel());
  const long long n = g.numel();
  TORCH_CHECK(u.numel() == n && v.numel() == n && boundary.numel() == 1);
  auto ws = make_workspace(g);
  const int rc = geops_bsc_fused(
      g.data_ptr<float>(), u.data_ptr<float>(), v.data_ptr<float>(),
      vals.data_ptr<float>(), idx.data_ptr<int32_t>(),
      boundary.data_ptr<float>(), (unsigned long long*)ws.data_ptr<int64_t>(),
      (float)mu, n, vals.numel(), (float)placeholder, cur_stream());
  launch_check("bsc_compress_fused");
  return rc == 0;
}

// ---------------------------------------------------------------------------
// Bi-Sparse boundary select (bscselect.hip): out[0] = the k-th largest
// |v[i] + (u[i]*mu + g[i])| (g and u given) or |v[i]| (both empty) over
// the sample positions i = si[0..S). n_wg: 0 lets the launcher choose, 1
// forces the one-workgroup form, >= 2 the ticket form on that many
// workgroups (the hook of the tests and the grid sweep).
// ---------------------------------------------------------------------------

void bsc_boundary(torch::Tensor v, torch::Tensor g, torch::Tensor u,
                  torch::Tensor si, int64_t k, double mu, torch::Tensor out,
                  int64_t n_wg) {
  // not check_f32: the gathers are 4 B reads, v may be a view off a 16 B
  // boundary
  auto check = [&](const torch::Tensor& t, torch::ScalarType dtype,
                   const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == v.device(), "bsc_boundary: ",
                name, " must be a GPU tensor on v's device");
    TORCH_CHECK(t.is_contiguous(), "bsc_boundary: ", name,
                " must be contiguous");
    TORCH_CHECK(t.scalar_type() == dtype, "bsc_boundary: ", name,
                " must be ", dtype, ", got ", t.scalar_type());
  };
  check(v, torch::kFloat32, "v");
  check(si, torch::kInt32, "si");
  check(out, torch::kFloat32, "out");
  // torch.Tensor() from Python is an empty tensor, as for dcasgd's mom
  const bool mom = g.defined() && g.numel() > 0;
  TORCH_CHECK(mom == (u.defined() && u.numel() > 0),
              "bsc_boundary takes g and u together or neither");
  const long long n = v.numel(), S = si.numel();
  if (mom) {
    check(g, torch::kFloat32, "g");
    check(u, torch::kFloat32, "u");
    TORCH_CHECK(g.numel() == n && u.numel() == n,
                "bsc_boundary: g and u must have as many elements as v");
  }
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, "bsc_boundary serves 1 <= n < 2^31, "
              "got ", n);
  TORCH_CHECK(S <= INT32_MAX, "bsc_boundary serves fewer than 2^31 samples");
  TORCH_CHECK(k >= 1 && k <= S, "bsc_boundary needs 1 <= k <= S, got k = ", k,
              ", S = ", S);
  TORCH_CHECK(out.numel() >= 1, "bsc_boundary: out needs one element");
  TORCH_CHECK(n_wg >= 0 && n_wg <= 65535, "bsc_boundary: n_wg out of range");
  const int grid = geops_bsc_boundary_grid(S, (int)n_wg);
  TORCH_CHECK(grid >= 1, "bsc_boundary: the one-workgroup form holds ",
              geops_bsc_boundary_cap(), " samples, got ", S);
  torch::Tensor ws;
  if (grid > 1)
    ws = torch::empty({geops_bsc_boundary_ws_words(S)},
                      torch::TensorOptions().dtype(torch::kInt32)
                          .device(v.device()));
  geops_bsc_boundary(v.data_ptr<float>(),
                     mom ? g.data_ptr<float>() : nullptr,
                     mom ? u.data_ptr<float>() : nullptr,
                     si.data_ptr<int32_t>(), S, k, n, (float)mu,
                     out.data_ptr<float>(),
                     grid > 1 ? (uint32_t*)ws.data_ptr<int32_t>() : nullptr,
                     grid, cur_stream());
  launch_check("bsc_boundary");
}

void bsc_pull_pack(torch::Tensor x, torch::Tensor vals, torch::Tensor idx,
                   double placeholder) {
  check_f32(x, "x"); check_f32(vals, "vals");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous());
  auto ws = make_workspace(x);
  geops_bsc_pull_pack(x.data_ptr<float>(), vals.data_ptr<float>(),
                      idx.data_ptr<int32_t>(), (long long*)ws.data_ptr<int64_t>(),
                      x.numel(), vals.numel(), (float)placeholder,
                      cur_stream());
  launch_check("bsc_pull_pack");
}

void bsc_unpack(torch::Tensor vals, torch::Tensor idx, torch::Tensor out,
                bool accumulate) {
  check_f32(vals, "vals"); check_f32(out, "out");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous());
  TORCH_CHECK(idx.is_cuda() && idx.numel() >= vals.numel(),
              "idx must be a GPU tensor at least as long as vals");
  if (!accumulate) {
    hipMemsetAsync(out.data_ptr<float>(), 0, out.numel() * sizeof(float),
                   cur_stream());
  }
  geops_bsc_unpack(vals.data_ptr<float>(), idx.data_ptr<int32_t>(),
                   out.data_ptr<float>(), vals.numel(), out.numel(),
                   accumulate, cur_stream());
  launch_check("bsc_unpack");
}

void dgt_contribution(torch::Tensor g, torch::Tensor out, int64_t chunk) {
  check_f32(g, "g"); check_f32(out, "out");
  const long long n = g.numel();
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, "chunk must be positive");
  const int nchunks = (int)((n + chunk - 1) / chunk);
  TORCH_CHECK(out.numel() == nchunks);
  geops_dgt_contribution(g.data_ptr<float>(), out.data_ptr<float>(), n,
                         (int)chunk, nchunks, cur_stream());
  launch_check("dgt_contribution");
}

void quantize_4bit(torch::Tensor x, torch::Tensor residual,
                   torch::Tensor packed, torch::Tensor minmax,
                   int64_t chunk) {
  check_f32(x, "x");
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8 && packed.is_contiguous());
  check_f32(minmax, "minmax");
  const long long n = x.numel();
  const int nchunks = (int)((n + chunk - 1) / chunk);
  TORCH_CHECK(packed.numel() == (n + 1) / 2);
  TORCH_CHECK(minmax.numel() == 2 * nchunks);
  TORCH_CHECK((chunk & (chunk - 1)) == 0 && chunk >= 4,
              "GPU quantize_4bit needs power-of-two chunk >= 4");
  const bool has_res = residual.defined() && residual.numel() > 0;
  if (has_res) check_f32(residual, "residual");
  geops_quantize_4bit(x.data_ptr<float>(),
                      has_res ? residual.data_ptr<float>() : nullptr,
                      packed.data_ptr<uint8_t>(), minmax.data_ptr<float>(),
                      n, (int)chunk, nchunks, has_res, cur_stream());
  launch_check("quantize_4bit");
}

void dequantize_4bit(torch::Tensor packed, torch::Tensor minmax,
                     torch::Tensor out, int64_t chunk) {
  check_f32(out, "out"); check_f32(minmax, "minmax");
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8 && packed.is_contiguous());
  TORCH_CHECK((chunk & (chunk - 1)) == 0 && chunk >= 4,
              "GPU dequantize_4bit needs power-of-two chunk >= 4");
  geops_dequantize_4bit(packed.data_ptr<uint8_t>(), minmax.data_ptr<float>(),
                        out.data_ptr<float>(), out.numel(), (int)chunk,
                        cur_stream());
  launch_check("dequantize_4bit");
}

// ---------------------------------------------------------------------------
// Fused wire reduce (wirereduce.hip): out = (accumulate ? out : +0) + the
// decoded payloads of all parties, folded in list order.
// ---------------------------------------------------------------------------

// one party's wire tensor: on out's device, contiguous, dtype and length
// as the format prescribes. An empty tensor may have a null data pointer;
// the kernels never dereference it.
const void* check_payload(const torch::Tensor& t, const torch::Tensor& out,
                          torch::ScalarType dtype, int64_t numel,
                          const char* name, size_t party) {
  TORCH_CHECK(t.is_cuda() && t.device() == out.device(), name, "[", party,
              "] must be a GPU tensor on out's device");
  TORCH_CHECK(t.is_contiguous(), name, "[", party, "] must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, name, "[", party, "] must be ",
              dtype, ", got ", t.scalar_type());
  TORCH_CHECK(t.numel() == numel, name, "[", party, "] must have ", numel,
              " elements, got ", t.numel());
  return t.data_ptr();
}

void wire_sum_2bit(std::vector<torch::Tensor> payloads, torch::Tensor out,
                   double thr, bool accumulate) {
  check_f32(out, "out");
  TORCH_CHECK(!payloads.empty(), "wire_sum_2bit needs at least one party");
  const long long n = out.numel();
  std::vector<const void*> ptrs;
  for (size_t p = 0; p < payloads.size(); ++p)
    ptrs.push_back(check_payload(payloads[p], out, torch::kInt32,
                                 (n + 15) / 16, "payloads", p));
  geops_wire_sum_2bit(ptrs.data(), (int)ptrs.size(), out.data_ptr<float>(), n,
                      (float)thr, accumulate, cur_stream());
  launch_check("wire_sum_2bit");
}

void wire_sum_f16(std::vector<torch::Tensor> payloads, torch::Tensor out,
                  bool accumulate) {
  check_f32(out, "out");
  TORCH_CHECK(!payloads.empty(), "wire_sum_f16 needs at least one party");
  const long long n = out.numel();
  std::vector<const void*> ptrs;
  for (size_t p = 0; p < payloads.size(); ++p)
    ptrs.push_back(check_payload(payloads[p], out, torch::kFloat16, n,
                                 "payloads", p));
  geops_wire_sum_f16(ptrs.data(), (int)ptrs.size(), out.data_ptr<float>(), n,
                     accumulate, cur_stream());
  launch_check("wire_sum_f16");
}

void wire_sum_dgt(std::vector<torch::Tensor> exacts,
                  std::vector<torch::Tensor> keep_idxs,
                  std::vector<torch::Tensor> packeds,
                  std::vector<torch::Tensor> minmaxs, torch::Tensor out,
                  int64_t chunk, bool accumulate) {
  check_f32(out, "out");
  const size_t P = exacts.size();
  TORCH_CHECK(P >= 1, "wire_sum_dgt needs at least one party");
  TORCH_CHECK(keep_idxs.size() == P && packeds.size() == P &&
              minmaxs.size() == P,
              "wire_sum_dgt needs the four payload lists equally long");
  TORCH_CHECK(chunk >= 64 && chunk <= (1 << 30) && (chunk & (chunk - 1)) == 0,
              "wire_sum_dgt needs a power-of-two chunk >= 64, got ", chunk);
  const long long numel = out.numel();
  const long long nchunks = (numel + chunk - 1) / chunk;
  TORCH_CHECK(nchunks <= INT32_MAX, "too many chunks");
  const long long n_keep = keep_idxs[0].numel();
  TORCH_CHECK(n_keep <= nchunks, "keep_idx names ", n_keep, " of ", nchunks,
              " chunks");
  const long long n_lossy = nchunks - n_keep;
  std::vector<const float*> pe, pm;
  std::vector<const int*> pk;
  std::vector<const uint8_t*> pp;
  for (size_t p = 0; p < P; ++p) {
    pe.push_back((const float*)check_payload(
        exacts[p], out, torch::kFloat32, n_keep * chunk, "exact", p));
    pk.push_back((const int*)check_payload(
        keep_idxs[p], out, torch::kInt32, n_keep, "keep_idx", p));
    pp.push_back((const uint8_t*)check_payload(
        packeds[p], out, torch::kUInt8, n_lossy * (chunk / 2), "packed", p));
    pm.push_back((const float*)check_payload(
        minmaxs[p], out, torch::kFloat32, 2 * n_lossy, "minmax", p));
    TORCH_CHECK(((uintptr_t)pe.back() & 15) == 0, "exact[", p,
                "] must be 16-byte aligned");
    TORCH_CHECK(((uintptr_t)pp.back() & 1) == 0, "packed[", p,
                "] must be 2-byte aligned");
  }
  geops_wire_sum_dgt(pe.data(), pk.data(), pp.data(), pm.data(), (int)P,
                     out.data_ptr<float>(), numel, (int)chunk, (int)nchunks,
                     (int)n_keep, accumulate, cur_stream());
  launch_check("wire_sum_dgt");
}

// ---------------------------------------------------------------------------
// Fused Bi-Sparse wire reduce (wiresparse.hip): out = (accumulate ? out : +0)
// + the scattered lists of all parties, folded in list order. Every list has
// the same number of slots; each is in ascending index order with its
// placeholders (index -1) last, which is not checked here.
// ---------------------------------------------------------------------------

// what both forms share: out, and the lists' common length
long long check_bsc_lists(const std::vector<torch::Tensor>& idxs,
                          const torch::Tensor& out, const char* what) {
  // not check_f32: the kernel has a scalar path for an `out` (a slice view)
  // off a 16 B boundary
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
              out.scalar_type() == torch::kFloat32, what,
              ": out must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(!idxs.empty(), what, " needs at least one party");
  TORCH_CHECK(out.numel() >= 1 && out.numel() <= INT32_MAX, what,
              " serves 1 <= n < 2^31, got ", out.numel());
  const long long k = idxs[0].numel();
  TORCH_CHECK(k < (1 << 30), what, " serves lists of fewer than 2^30 slots");
  return k;
}

void wire_sum_bsc(std::vector<torch::Tensor> vals,
                  std::vector<torch::Tensor> idxs, torch::Tensor out,
                  bool accumulate) {
  const long long k = check_bsc_lists(idxs, out, "wire_sum_bsc");
  const size_t P = idxs.size();
  TORCH_CHECK(vals.size() == P,
              "wire_sum_bsc needs as many value lists as index lists");
  std::vector<const float*> pv;
  std::vector<const int*> pi;
  for (size_t p = 0; p < P; ++p) {
    pv.push_back((const float*)check_payload(vals[p], out, torch::kFloat32, k,
                                             "vals", p));
    pi.push_back((const int*)check_payload(idxs[p], out, torch::kInt32, k,
                                           "idx", p));
  }
  geops_wire_sum_bsc(pv.data(), pi.data(), (int)P, (int)k,
                     out.data_ptr<float>(), out.numel(), accumulate,
                     cur_stream());
  launch_check("wire_sum_bsc");
}

void wire_sum_bsc_dgt(std::vector<torch::Tensor> exacts,
                      std::vector<torch::Tensor> keep_idxs,
                      std::vector<torch::Tensor> packeds,
                      std::vector<torch::Tensor> minmaxs,
                      std::vector<torch::Tensor> idxs, torch::Tensor out,
                      int64_t chunk, bool accumulate) {
  const long long k = check_bsc_lists(idxs, out, "wire_sum_bsc_dgt");
  const size_t P = idxs.size();
  TORCH_CHECK(exacts.size() == P && keep_idxs.size() == P &&
              packeds.size() == P && minmaxs.size() == P,
              "wire_sum_bsc_dgt needs the five payload lists equally long");
  TORCH_CHECK(chunk >= 64 && chunk <= 8192 && (chunk & (chunk - 1)) == 0,
              "wire_sum_bsc_dgt serves a power-of-two chunk in [64, 8192], "
              "got ", chunk);
  TORCH_CHECK(k >= 1, "wire_sum_bsc_dgt needs at least one list slot");
  const long long nchunks = (k + chunk - 1) / chunk;
  const long long n_keep = keep_idxs[0].numel();
  TORCH_CHECK(n_keep <= nchunks, "keep_idx names ", n_keep, " of ", nchunks,
              " chunks");
  const long long n_lossy = nchunks - n_keep;
  std::vector<const float*> pe, pm;
  std::vector<const int*> pk, pi;
  std::vector<const uint8_t*> pp;
  for (size_t p = 0; p < P; ++p) {
    pe.push_back((const float*)check_payload(
        exacts[p], out, torch::kFloat32, n_keep * chunk, "exact", p));
    pk.push_back((const int*)check_payload(
        keep_idxs[p], out, torch::kInt32, n_keep, "keep_idx", p));
    pp.push_back((const uint8_t*)check_payload(
        packeds[p], out, torch::kUInt8, n_lossy * (chunk / 2), "packed", p));
    pm.push_back((const float*)check_payload(
        minmaxs[p], out, torch::kFloat32, 2 * n_lossy, "minmax", p));
    pi.push_back((const int*)check_payload(idxs[p], out, torch::kInt32, k,
                                           "idx", p));
  }
  geops_wire_sum_bsc_dgt(pe.data(), pk.data(), pp.data(), pm.data(),
                         pi.data(), (int)P, (int)k, (int)chunk, (int)n_keep,
                         out.data_ptr<float>(), out.numel(), accumulate,
                         cur_stream());
  launch_check("wire_sum_bsc_dgt");
}

// ---------------------------------------------------------------------------
// Fused DGT encode (dgtencode.hip): the mode-3 wire payload of one bucket and
// the residual update in one kernel. The outputs are written whole.
// ---------------------------------------------------------------------------

void dgt_encode(torch::Tensor x, torch::Tensor residual, torch::Tensor contrib,
                torch::Tensor keep_idx, torch::Tensor exact,
                torch::Tensor packed, torch::Tensor minmax, int64_t chunk) {
  check_f32(x, "x"); check_f32(residual, "residual");
  check_f32(exact, "exact");
  TORCH_CHECK(chunk >= 64 && chunk <= 8192 && (chunk & (chunk - 1)) == 0,
              "dgt_encode serves a power-of-two chunk in [64, 8192], got ",
              chunk);
  const long long numel = x.numel();
  TORCH_CHECK(numel >= 1, "dgt_encode needs at least one element");
  TORCH_CHECK(residual.numel() == numel, "residual must have as many "
              "elements as x (", residual.numel(), " vs ", numel, ")");
  const long long nchunks = (numel + chunk - 1) / chunk;
  TORCH_CHECK(nchunks <= INT32_MAX, "too many chunks");
  const long long n_keep = keep_idx.numel();
  TORCH_CHECK(n_keep <= nchunks, "keep_idx names ", n_keep, " of ", nchunks,
              " chunks");
  const long long n_lossy = nchunks - n_keep;
  check_payload(contrib, x, torch::kFloat32, nchunks, "contrib", 0);
  check_payload(keep_idx, x, torch::kInt32, n_keep, "keep_idx", 0);
  TORCH_CHECK(residual.device() == x.device() && exact.device() == x.device(),
              "residual and exact must be on x's device");
  TORCH_CHECK(exact.numel() == n_keep * chunk, "exact must have ",
              n_keep * chunk, " elements, got ", exact.numel());
  // empty when n_lossy == 0: the data pointers may be null, never used
  const void* pk = check_payload(packed, x, torch::kUInt8,
                                 n_lossy * (chunk / 2), "packed", 0);
  const void* mm = check_payload(minmax, x, torch::kFloat32, 2 * n_lossy,
                                 "minmax", 0);
  TORCH_CHECK(((uintptr_t)pk & 15) == 0 && ((uintptr_t)mm & 15) == 0,
              "packed and minmax must be 16-byte aligned");
  const int rc = geops_dgt_encode(
      x.data_ptr<float>(), residual.data_ptr<float>(),
      contrib.data_ptr<float>(), keep_idx.data_ptr<int32_t>(),
      exact.data_ptr<float>(), (uint8_t*)pk, (float*)mm, numel, (int)chunk,
      (int)nchunks, (int)n_keep, cur_stream());
  TORCH_CHECK(rc == 0, "dgt_encode: no kernel for chunk ", chunk);
  launch_check("dgt_encode");
}

// ---------------------------------------------------------------------------
// FP8 wire tier (wirefp8.hip): block-scaled E4M3 payload of one bucket with
// the residual update, and the fused decode-and-sum of all parties.
// ---------------------------------------------------------------------------

// chunk in the kernels' table and 1 <= n < 2^31; returns the payload bytes
long long check_fp8_shape(const char* what, long long n, int64_t chunk) {
  TORCH_CHECK(chunk >= 64 && chunk <= 8192 && (chunk & (chunk - 1)) == 0,
              what, " serves a power-of-two chunk in [64, 8192], got ", chunk);
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, what, " serves 1 <= n < 2^31, got ",
              n);
  return geops_fp8_wire_bytes(n, (int)chunk);
}

void fp8_encode(torch::Tensor x, c10::optional<torch::Tensor> residual,
                torch::Tensor payload, int64_t chunk) {
  check_f32(x, "x");
  const long long n = x.numel();
  const long long bytes = check_fp8_shape("fp8_encode", n, chunk);
  float* res = nullptr;
  if (residual) {
    check_f32(*residual, "residual");
    TORCH_CHECK(residual->device() == x.device(),
                "residual must be on x's device");
    TORCH_CHECK(residual->numel() == n, "residual must have as many "
                "elements as x (", residual->numel(), " vs ", n, ")");
    res = residual->data_ptr<float>();
  }
  const void* pl = check_payload(payload, x, torch::kUInt8, bytes, "payload",
                                 0);
  TORCH_CHECK(((uintptr_t)pl & 15) == 0, "payload must be 16-byte aligned");
  const int rc = geops_fp8_encode(x.data_ptr<float>(), res, (uint8_t*)pl, n,
                                  (int)chunk, cur_stream());
  TORCH_CHECK(rc == 0, "fp8_encode: no kernel for chunk ", chunk);
  launch_check("fp8_encode");
}

void wire_sum_fp8(std::vector<torch::Tensor> payloads, torch::Tensor out,
                  int64_t chunk, bool accumulate) {
  check_f32(out, "out");
  TORCH_CHECK(!payloads.empty(), "wire_sum_fp8 needs at least one party");
  const long long n = out.numel();
  const long long bytes = check_fp8_shape("wire_sum_fp8", n, chunk);
  std::vector<const void*> ptrs;
  for (size_t p = 0; p < payloads.size(); ++p) {
    ptrs.push_back(check_payload(payloads[p], out, torch::kUInt8, bytes,
                                 "payloads", p));
    TORCH_CHECK(((uintptr_t)ptrs.back() & 15) == 0, "payloads[", p,
                "] must be 16-byte aligned");
  }
  const int rc = geops_wire_sum_fp8(ptrs.data(), (int)ptrs.size(),
                                    out.data_ptr<float>(), n, (int)chunk,
                                    accumulate, cur_stream());
  TORCH_CHECK(rc == 0, "wire_sum_fp8: no kernel for chunk ", chunk);
  launch_check("wire_sum_fp8");
}

void relu_maxpool2_fwd(torch::Tensor in, torch::Tensor out, torch::Tensor idx,
                       int64_t N, int64_t C, int64_t Hi, int64_t Wi) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda() && idx.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(idx.scalar_type() == torch::kUInt8);
  TORCH_CHECK(C % 8 == 0 && Hi % 2 == 0 && Wi % 2 == 0,
              "relu_maxpool2 needs C%8==0 and even H,W");
  const int Ho = (int)(Hi / 2), Wo = (int)(Wi / 2);
  const long long n_vec = (long long)N * Ho * Wo * (C / 8);
  geops_relu_maxpool2_fwd((const unsigned short*)in.data_ptr(),
                          (unsigned short*)out.data_ptr(),
                          idx.data_ptr<uint8_t>(), n_vec, Ho, Wo, (int)C,
                          cur_stream());
  launch_check("relu_maxpool2_fwd");
}

void relu_maxpool2_bwd(torch::Tensor grad_out, torch::Tensor idx,
                       torch::Tensor grad_in, int64_t N, int64_t C,
                       int64_t Hi, int64_t Wi) {
  TORCH_CHECK(grad_out.is_cuda() && idx.is_cuda() && grad_in.is_cuda());
  TORCH_CHECK(grad_out.scalar_type() == torch::kBFloat16 &&
              grad_in.scalar_type() == torch::kBFloat16);
  const long long n_vec_in = (long long)N * Hi * Wi * (C / 8);
  geops_relu_maxpool2_bwd((const unsigned short*)grad_out.data_ptr(),
                          idx.data_ptr<uint8_t>(),
                          (unsigned short*)grad_in.data_ptr(), n_vec_in,
                          (int)Hi, (int)Wi, (int)C, cur_stream());
  launch_check("relu_maxpool2_bwd");
}

void conv5_nhwc(torch::Tensor in, torch::Tensor w_frags, torch::Tensor bias,
                torch::Tensor out, int64_t N, int64_t Hi, int64_t Wi,
                int64_t Ho, int64_t Wo, int64_t CI, int64_t CO,
                int64_t pad) {
  TORCH_CHECK(in.is_cuda() && w_frags.is_cuda() && out.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  const bool has_bias = bias.defined() && bias.numel() > 0;
  if (has_bias)
    TORCH_CHECK(bias.scalar_type() == torch::kFloat32 && bias.is_cuda());
  const int rc = geops_conv5_nhwc(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)w_frags.data_ptr(),
      has_bias ? bias.data_ptr<float>() : nullptr,
      (unsigned short*)out.data_ptr(), (int)N, (int)Hi, (int)Wi, (int)Ho,
      (int)Wo, (int)CI, (int)CO, (int)pad, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_nhwc: unsupported geometry CI=", CI,
              " CO=", CO, " pad=", pad);
  launch_check("conv5_nhwc");
}

void conv5_pool_nhwc(torch::Tensor in, torch::Tensor w_frags,
                     torch::Tensor bias, torch::Tensor out,
                     torch::Tensor mask, int64_t N, int64_t Hi, int64_t Wi,
                     int64_t Ho, int64_t Wo, int64_t CI, int64_t CO) {
  TORCH_CHECK(in.is_cuda() && w_frags.is_cuda() && out.is_cuda() &&
              mask.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16 &&
              mask.scalar_type() == torch::kUInt8);
  const bool has_bias = bias.numel() > 0;
  const int rc = geops_conv5_pool_nhwc(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)w_frags.data_ptr(),
      has_bias ? bias.data_ptr<float>() : nullptr,
      (unsigned short*)out.data_ptr(), mask.data_ptr<uint8_t>(), (int)N,
      (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)CI, (int)CO, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_pool_nhwc: unsupported geometry CI=", CI,
              " CO=", CO);
  launch_check("conv5_pool_nhwc");
}

// Test hook: conv5_pool_nhwc on a grid of n_wg workgroups, with the
// tensor sizes checked against the geometry.
void conv5_pool_nwg_nhwc(torch::Tensor in, torch::Tensor w_frags,
                         torch::Tensor bias, torch::Tensor out,
                         torch::Tensor mask, int64_t N, int64_t Hi,
                         int64_t Wi, int64_t Ho, int64_t Wo, int64_t CI,
                         int64_t CO, int64_t n_wg) {
  TORCH_CHECK(in.is_cuda() && w_frags.is_cuda() && out.is_cuda() &&
              mask.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16 &&
              mask.scalar_type() == torch::kUInt8);
  TORCH_CHECK(N >= 1 && Ho >= 2 && Wo >= 2 && Hi == Ho + 4 && Wi == Wo + 4 &&
              n_wg >= 1 && n_wg <= 65536 && (CI == 4 || CI == 16) &&
              (CO == 16 || CO == 32),
              "conv5_pool_nwg_nhwc: bad size or n_wg");
  const int64_t Sp = (5 * CI + 7) & ~7, nK = (5 * Sp + 31) / 32;
  TORCH_CHECK(in.numel() == N * Hi * Wi * CI &&
              out.numel() == N * (Ho / 2) * (Wo / 2) * CO &&
              mask.numel() == out.numel() &&
              w_frags.numel() == (CO / 16) * nK * 64 * 8,
              "conv5_pool_nwg_nhwc: tensor size mismatch");
  const bool has_bias = bias.numel() > 0;
  if (has_bias)
    TORCH_CHECK(bias.scalar_type() == torch::kFloat32 && bias.is_cuda() &&
                bias.numel() == CO);
  const int rc = geops_conv5_pool_nwg_nhwc(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)w_frags.data_ptr(),
      has_bias ? bias.data_ptr<float>() : nullptr,
      (unsigned short*)out.data_ptr(), mask.data_ptr<uint8_t>(), (int)N,
      (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)CI, (int)CO, (int)n_wg,
      cur_stream());
  TORCH_CHECK(rc == 0, "conv5_pool_nwg_nhwc: unsupported geometry CI=", CI,
              " CO=", CO);
  launch_check("conv5_pool_nwg_nhwc");
}

// conv1 stage from the caller's fp32 image: x is [N][3][Hi][Wi] in
// channels_last memory (or [N][Hi][Wi][3] contiguous); out and mask as
// conv5_pool_nhwc gives them for pad_ch3to4_nhwc(x), which is written
// to xb_out unless that is an empty tensor. The kernel addresses every
// operand from the geometry alone, so all sizes are checked here.
// n_wg == 0 is the default grid. With `table` (the uint8 form) x holds
// uint8 pixels and table the bf16 [3][256] values they stand for.
static void check_value_table(const char* what, const torch::Tensor& table,
                              int64_t channels) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kBFloat16 &&
              table.dim() == 2 && table.size(0) == channels &&
              table.size(1) == 256 && table.is_contiguous() &&
              ((uintptr_t)table.data_ptr() & 3) == 0, what,
              ": table must be a contiguous bf16 [", channels,
              "][256] GPU tensor");
}

static void conv5_pool_x32_checked(const char* what, torch::Tensor x,
                                   const torch::Tensor* table,
                                   torch::Tensor w_frags, torch::Tensor bias,
                                   torch::Tensor out, torch::Tensor mask,
                                   torch::Tensor xb_out, int64_t N,
                                   int64_t Hi, int64_t Wi, int64_t Ho,
                                   int64_t Wo, int64_t CO, int64_t n_wg) {
  TORCH_CHECK(x.is_cuda() && w_frags.is_cuda() && out.is_cuda() &&
              mask.is_cuda(), what, ": operands must be GPU tensors");
  TORCH_CHECK(x.scalar_type() == (table ? torch::kUInt8 : torch::kFloat32) &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16 &&
              mask.scalar_type() == torch::kUInt8, what, ": operand dtype");
  if (table) check_value_table(what, *table, 3);
  TORCH_CHECK(N >= 1 && N <= INT32_MAX && Ho >= 2 && Wo >= 2 &&
              Hi == Ho + 4 && Wi == Wo + 4 && Hi <= INT32_MAX && CO == 16 &&
              n_wg >= 0 && n_wg <= 65536, what, ": bad size or n_wg");
  const bool nhwc =
      x.dim() == 4 &&
      ((x.size(0) == N && x.size(1) == 3 && x.size(2) == Hi &&
        x.size(3) == Wi &&
        x.is_contiguous(at::MemoryFormat::ChannelsLast)) ||
       (x.size(0) == N && x.size(1) == Hi && x.size(2) == Wi &&
        x.size(3) == 3 && x.is_contiguous()));
  TORCH_CHECK(nhwc, what, ": x must hold [N][Hi][Wi][3] densely");
  TORCH_CHECK(out.numel() == N * (Ho / 2) * (Wo / 2) * CO &&
              mask.numel() == out.numel() && w_frags.numel() == 4 * 64 * 8,
              what, ": tensor size mismatch");
  const bool has_bias = bias.numel() > 0;
  if (has_bias)
    TORCH_CHECK(bias.scalar_type() == torch::kFloat32 && bias.is_cuda() &&
                bias.numel() == CO, what, ": bias must be 16 fp32 on the GPU");
  const bool has_xb = xb_out.numel() > 0;
  if (has_xb)
    TORCH_CHECK(xb_out.is_cuda() &&
                xb_out.scalar_type() == torch::kBFloat16 &&
                xb_out.is_non_overlapping_and_dense() &&
                xb_out.numel() == N * Hi * Wi * 4, what,
                ": xb_out must hold [N][Hi][Wi][4] bf16");
  const float* b = has_bias ? bias.data_ptr<float>() : nullptr;
  unsigned short* xb = has_xb ? (unsigned short*)xb_out.data_ptr() : nullptr;
  const int rc =
      table ? geops_conv5_pool_u8_nhwc(
                  x.data_ptr<uint8_t>(),
                  (const unsigned short*)table->data_ptr(),
                  (const unsigned short*)w_frags.data_ptr(), b,
                  (unsigned short*)out.data_ptr(), mask.data_ptr<uint8_t>(),
                  xb, (int)N, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)CO,
                  (int)n_wg, cur_stream())
            : geops_conv5_pool_x32_nhwc(
                  x.data_ptr<float>(),
                  (const unsigned short*)w_frags.data_ptr(), b,
                  (unsigned short*)out.data_ptr(), mask.data_ptr<uint8_t>(),
                  xb, (int)N, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)CO,
                  (int)n_wg, cur_stream());
  TORCH_CHECK(rc == 0, what, ": unsupported geometry or alignment Hi=", Hi,
              " Wi=", Wi);
  launch_check(what);
}

void conv5_pool_x32_nhwc(torch::Tensor x, torch::Tensor w_frags,
                         torch::Tensor bias, torch::Tensor out,
                         torch::Tensor mask, torch::Tensor xb_out, int64_t N,
                         int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo,
                         int64_t CO) {
  conv5_pool_x32_checked("conv5_pool_x32_nhwc", x, nullptr, w_frags, bias,
                         out, mask, xb_out, N, Hi, Wi, Ho, Wo, CO, 0);
}

// Test hook: conv5_pool_x32_nhwc on a grid of n_wg workgroups.
void conv5_pool_x32_nwg_nhwc(torch::Tensor x, torch::Tensor w_frags,
                             torch::Tensor bias, torch::Tensor out,
                             torch::Tensor mask, torch::Tensor xb_out,
                             int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                             int64_t Wo, int64_t CO, int64_t n_wg) {
  TORCH_CHECK(n_wg >= 1, "conv5_pool_x32_nwg_nhwc: n_wg must be positive");
  conv5_pool_x32_checked("conv5_pool_x32_nwg_nhwc", x, nullptr, w_frags, bias,
                         out, mask, xb_out, N, Hi, Wi, Ho, Wo, CO, n_wg);
}

// conv1 stage from a uint8 image and its value table: x as for
// conv5_pool_x32_nhwc but uint8, table bf16 [3][256]; out, mask and xb_out
// are what conv5_pool_x32_nhwc gives for the fp32 image table[c][x].
void conv5_pool_u8_nhwc(torch::Tensor x, torch::Tensor table,
                        torch::Tensor w_frags, torch::Tensor bias,
                        torch::Tensor out, torch::Tensor mask,
                        torch::Tensor xb_out, int64_t N, int64_t Hi,
                        int64_t Wi, int64_t Ho, int64_t Wo, int64_t CO) {
  conv5_pool_x32_checked("conv5_pool_u8_nhwc", x, &table, w_frags, bias, out,
                         mask, xb_out, N, Hi, Wi, Ho, Wo, CO, 0);
}

// Test hook: conv5_pool_u8_nhwc on a grid of n_wg workgroups.
void conv5_pool_u8_nwg_nhwc(torch::Tensor x, torch::Tensor table,
                            torch::Tensor w_frags, torch::Tensor bias,
                            torch::Tensor out, torch::Tensor mask,
                            torch::Tensor xb_out, int64_t N, int64_t Hi,
                            int64_t Wi, int64_t Ho, int64_t Wo, int64_t CO,
                            int64_t n_wg) {
  TORCH_CHECK(n_wg >= 1, "conv5_pool_u8_nwg_nhwc: n_wg must be positive");
  conv5_pool_x32_checked("conv5_pool_u8_nwg_nhwc", x, &table, w_frags, bias,
                         out, mask, xb_out, N, Hi, Wi, Ho, Wo, CO, n_wg);
}

void conv5_wrw_nhwc(torch::Tensor in, torch::Tensor gout, torch::Tensor part,
                    int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                    int64_t Wo, int64_t CI, int64_t CO, int64_t n_wg) {
  TORCH_CHECK(in.is_cuda() && gout.is_cuda() && part.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              gout.scalar_type() == torch::kBFloat16 &&
              part.scalar_type() == torch::kFloat32);
  // The two kernels write different slab layouts (ops/conv.py
  // build_wrw_unpack_index), so there is no fallback between them: a
  // geometry neither launcher accepts is an error.
  const auto launch =
      CI == 4 ? geops_conv5_wrw4_nhwc : geops_conv5_wrw16_nhwc;
  const int rc = launch(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)gout.data_ptr(), part.data_ptr<float>(),
      (int)N, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)CI, (int)CO,
      (int)n_wg, cur_stream());
  TORCH_CHECK(rc > 0, "conv5_wrw_nhwc: unsupported geometry CI=", CI,
              " CO=", CO, " Wi=", Wi, " Wo=", Wo);
  launch_check("conv5_wrw_nhwc");
}

// Weight gradient from the POOLED grad_out `gp` [N][Ho/2][Wo/2][CO] and
// its argmax codes `mask`: the kernel does the max-pool backward while
// staging. Ho, Wo are the full-resolution sizes (even); slab layout and
// n_wg as conv5_wrw_nhwc.
void conv5_wrw_unpool_nhwc(torch::Tensor in, torch::Tensor gp,
                           torch::Tensor mask, torch::Tensor part, int64_t N,
                           int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo,
                           int64_t CI, int64_t CO, int64_t n_wg) {
  TORCH_CHECK(in.is_cuda() && gp.is_cuda() && mask.is_cuda() &&
              part.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              gp.scalar_type() == torch::kBFloat16 &&
              mask.scalar_type() == torch::kUInt8 &&
              part.scalar_type() == torch::kFloat32);
  TORCH_CHECK(Ho == Hi - 4 && Wo == Wi - 4 && in.numel() == N * Hi * Wi * CI,
              "conv5_wrw_unpool_nhwc: input size mismatch");
  TORCH_CHECK(gp.numel() == N * (Ho / 2) * (Wo / 2) * CO &&
                  mask.numel() == gp.numel(),
              "conv5_wrw_unpool_nhwc: pooled gradient / mask size mismatch");
  TORCH_CHECK(n_wg > 0 && part.numel() >= n_wg * (CI == 4 ? 176 : 416) * CO,
              "conv5_wrw_unpool_nhwc: partial slab too small");
  const int rc = geops_conv5_wrw_unpool_nhwc(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)gp.data_ptr(), mask.data_ptr<uint8_t>(),
      part.data_ptr<float>(), (int)N, (int)Hi, (int)Wi, (int)Ho, (int)Wo,
      (int)CI, (int)CO, (int)n_wg, cur_stream());
  TORCH_CHECK(rc > 0, "conv5_wrw_unpool_nhwc: unsupported geometry CI=", CI,
              " CO=", CO, " Wi=", Wi, " Ho=", Ho, " Wo=", Wo);
  launch_check("conv5_wrw_unpool_nhwc");
}

// conv2 data gradient from the POOLED grad_out + argmax codes; sizes as
// conv5_nhwc with pad=4 (Hi, Wi = full-resolution grad_out + 8).
void conv5_dgrad_unpool_nhwc(torch::Tensor gp, torch::Tensor mask,
                             torch::Tensor w_frags, torch::Tensor out,
                             int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                             int64_t Wo, int64_t CI, int64_t CO) {
  TORCH_CHECK(gp.is_cuda() && mask.is_cuda() && w_frags.is_cuda() &&
              out.is_cuda());
  TORCH_CHECK(gp.scalar_type() == torch::kBFloat16 &&
              mask.scalar_type() == torch::kUInt8 &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(Hi >= 10 && Wi >= 10 &&
                  gp.numel() == N * ((Hi - 8) / 2) * ((Wi - 8) / 2) * CI &&
                  mask.numel() == gp.numel(),
              "conv5_dgrad_unpool_nhwc: pooled gradient / mask size mismatch");
  TORCH_CHECK(out.numel() == N * Ho * Wo * CO,
              "conv5_dgrad_unpool_nhwc: output size mismatch");
  const int rc = geops_conv5_dgrad_unpool_nhwc(
      (const unsigned short*)gp.data_ptr(), mask.data_ptr<uint8_t>(),
      (const unsigned short*)w_frags.data_ptr(),
      (unsigned short*)out.data_ptr(), (int)N, (int)Hi, (int)Wi, (int)Ho,
      (int)Wo, (int)CI, (int)CO, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_dgrad_unpool_nhwc: unsupported geometry CI=",
              CI, " CO=", CO, " Hi=", Hi, " Wi=", Wi);
  launch_check("conv5_dgrad_unpool_nhwc");
}

// Test hook: the direct kernel k_conv5_nhwc<32, 1> on a physically
// padded input [N][Ho+4][Wo+4][32], whatever the row width. conv5_nhwc
// routes such rows to the LDS kernel below 236 pixels; this entry is the
// bit-exact oracle that kernel is tested against.
void conv5_direct_nhwc(torch::Tensor in, torch::Tensor w_frags,
                       torch::Tensor out, int64_t N, int64_t Hi, int64_t Wi,
                       int64_t Ho, int64_t Wo, int64_t CI, int64_t CO) {
  TORCH_CHECK(in.is_cuda() && w_frags.is_cuda() && out.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(in.numel() == N * Hi * Wi * CI &&
                  out.numel() == N * Ho * Wo * CO &&
                  w_frags.numel() == 25 * 64 * 8,
              "conv5_direct_nhwc: tensor size mismatch");
  const int rc = geops_conv5_direct_nhwc(
      (const unsigned short*)in.data_ptr(),
      (const unsigned short*)w_frags.data_ptr(), nullptr,
      (unsigned short*)out.data_ptr(), (int)N, (int)Hi, (int)Wi, (int)Ho,
      (int)Wo, (int)CI, (int)CO, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_direct_nhwc: unsupported geometry CI=", CI,
              " CO=", CO, " Hi=", Hi, " Wi=", Wi);
  launch_check("conv5_direct_nhwc");
}

// Test hook: the conv2 data gradient on a grid of n_wg workgroups, so
// that a small input runs several blocks per workgroup. With an empty
// `mask`, `in` is the full-resolution grad_out (conv5_nhwc with pad=4);
// otherwise `in` is the pooled grad_out (conv5_dgrad_unpool_nhwc).
void conv5_dgrad_nwg_nhwc(torch::Tensor in, torch::Tensor mask,
                          torch::Tensor w_frags, torch::Tensor out,
                          int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                          int64_t Wo, int64_t CI, int64_t CO, int64_t n_wg) {
  const bool pooled = mask.defined() && mask.numel() > 0;
  TORCH_CHECK(in.is_cuda() && w_frags.is_cuda() && out.is_cuda());
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 &&
              w_frags.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(Hi >= 10 && Wi >= 10 && n_wg >= 1 && n_wg <= 65536,
              "conv5_dgrad_nwg_nhwc: bad size or n_wg");
  if (pooled) {
    TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8);
    TORCH_CHECK(in.numel() == N * ((Hi - 8) / 2) * ((Wi - 8) / 2) * CI &&
                    mask.numel() == in.numel(),
                "conv5_dgrad_nwg_nhwc: pooled gradient / mask size mismatch");
  } else {
    TORCH_CHECK(in.numel() == N * (Hi - 8) * (Wi - 8) * CI,
                "conv5_dgrad_nwg_nhwc: gradient size mismatch");
  }
  TORCH_CHECK(out.numel() == N * Ho * Wo * CO &&
                  w_frags.numel() == 25 * 64 * 8,
              "conv5_dgrad_nwg_nhwc: output / weight size mismatch");
  const int rc = geops_conv5_dgrad_nwg_nhwc(
      (const unsigned short*)in.data_ptr(),
      pooled ? mask.data_ptr<uint8_t>() : nullptr,
      (const unsigned short*)w_frags.data_ptr(),
      (unsigned short*)out.data_ptr(), (int)N, (int)Hi, (int)Wi, (int)Ho,
      (int)Wo, (int)CI, (int)CO, (int)n_wg, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_dgrad_nwg_nhwc: unsupported geometry CI=", CI,
              " CO=", CO, " Hi=", Hi, " Wi=", Wi);
  launch_check("conv5_dgrad_nwg_nhwc");
}

// ---- grayscale conv1 stage (conv1c.hip): CI = 1, CO = 16 ----

// x is the [N][1][H][W] tensor as it is, fp32 or bf16 (the kernels round
// fp32 while staging), or uint8 with `table`, the bf16 [1][256] values
// its bytes stand for (undefined or empty for the other two). Returns the
// launchers' x_kind: 1 for fp32, 0 for bf16, 2 for uint8.
int check_c1_input(const torch::Tensor& x, const torch::Tensor& table,
                   int64_t N, int64_t H, int64_t W, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), what,
              ": x must be a contiguous GPU tensor");
  const bool has_table = table.defined() && table.numel() > 0;
  const bool f32 = x.scalar_type() == torch::kFloat32;
  const bool u8 = x.scalar_type() == torch::kUInt8;
  if (has_table) {
    TORCH_CHECK(u8, what, ": a table goes with a uint8 x");
    check_value_table(what, table, 1);
  } else {
    TORCH_CHECK(f32 || x.scalar_type() == torch::kBFloat16, what,
                ": x must be fp32 or bf16, or uint8 with a table");
  }
  TORCH_CHECK(N >= 1 && H >= 5 && W >= 5 && x.numel() == N * H * W, what,
              ": x does not hold N*H*W elements");
  TORCH_CHECK(((uintptr_t)x.data_ptr() & (f32 ? 7 : u8 ? 1 : 3)) == 0, what,
              ": x must be aligned to a pixel pair");
  return u8 ? 2 : f32 ? 1 : 0;
}

const unsigned short* c1_table_ptr(const torch::Tensor& table, int kind) {
  return kind == 2 ? (const unsigned short*)table.data_ptr() : nullptr;
}

// a dense NHWC operand: plain contiguous, or an NCHW-shaped channels_last
void check_c1_nhwc(const torch::Tensor& t, torch::ScalarType dtype,
                   int64_t numel, const char* what, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dtype, what, ": ", name,
              " has the wrong device or dtype");
  TORCH_CHECK(t.is_contiguous() ||
                  (t.dim() == 4 &&
                   t.is_contiguous(at::MemoryFormat::ChannelsLast)),
              what, ": ", name, " must be dense");
  TORCH_CHECK(t.numel() == numel, what, ": ", name, " holds ", t.numel(),
              " elements, expected ", numel);
  TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, what, ": ", name,
              " must be 16-byte aligned");
}

// the grid: n_wg > 0 as given (test hook), 0 = min(cap, blocks)
int64_t c1_grid(int64_t n_wg, int64_t blocks, int64_t cap, const char* what) {
  TORCH_CHECK(n_wg >= 0 && n_wg <= 65536, what, ": bad n_wg");
  if (n_wg > 0) return n_wg;
  return blocks < cap ? (blocks < 1 ? 1 : blocks) : cap;
}

// conv(1 -> 16, 5x5) + bias + ReLU + 2x2 max-pool; out / mask as
// conv5_pool_nhwc. Blocks are 4 conv rows; the default grid is two
// resident rounds, as for the CI = 4 kernel.
void conv5c1_pool(torch::Tensor x, torch::Tensor w_frags, torch::Tensor bias,
                  torch::Tensor out, torch::Tensor mask, int64_t N, int64_t H,
                  int64_t W, int64_t n_wg,
                  c10::optional<torch::Tensor> table_) {
  const char* what = "conv5c1_pool";
  const torch::Tensor table = table_.value_or(torch::Tensor());
  const int kind = check_c1_input(x, table, N, H, W, what);
  const int64_t Hop = (H - 4) / 2, Wop = (W - 4) / 2;
  check_c1_nhwc(w_frags, torch::kBFloat16, 2 * 64 * 8, what, "w_frags");
  check_c1_nhwc(out, torch::kBFloat16, N * Hop * Wop * 16, what, "out");
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 &&
                  mask.is_contiguous() && mask.numel() == out.numel() &&
                  ((uintptr_t)mask.data_ptr() & 3) == 0,
              what, ": mask must be uint8, dense, as large as out");
  const bool has_bias = bias.defined() && bias.numel() > 0;
  if (has_bias)
    TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == torch::kFloat32 &&
                    bias.is_contiguous() && bias.numel() == 16,
                what, ": bias must be 16 fp32 values");
  const int64_t grid = c1_grid(n_wg, N * ((Hop + 1) / 2), 2048, what);
  const int rc = geops_conv5c1_pool(
      x.data_ptr(), kind, c1_table_ptr(table, kind),
      (const unsigned short*)w_frags.data_ptr(),
      has_bias ? bias.data_ptr<float>() : nullptr,
      (unsigned short*)out.data_ptr(), mask.data_ptr<uint8_t>(), (int)N,
      (int)H, (int)W, (int)grid, cur_stream());
  TORCH_CHECK(rc == 0, what, ": unsupported geometry H=", H, " W=", W,
              " (even H, even W in 6..228)");
  launch_check(what);
}

void c1_wrw(const char* what, torch::Tensor x, torch::Tensor g,
            const torch::Tensor* mask, torch::Tensor part, int64_t N,
            int64_t H, int64_t W, int64_t n_wg, const torch::Tensor& table) {
  const int kind = check_c1_input(x, table, N, H, W, what);
  const int64_t Ho = H - 4, Wo = W - 4;
  if (mask) {
    check_c1_nhwc(g, torch::kBFloat16, N * (Ho / 2) * (Wo / 2) * 16, what,
                  "gp");
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == torch::kUInt8 &&
                    mask->is_contiguous() && mask->numel() == g.numel() &&
                    ((uintptr_t)mask->data_ptr() & 7) == 0,
                what, ": mask must be uint8, dense, as large as gp");
  } else {
    check_c1_nhwc(g, torch::kBFloat16, N * Ho * Wo * 16, what, "go");
  }
  const int64_t grid = c1_grid(n_wg, N * ((Ho + 1) / 2), 768, what);
  check_f32(part, "part");
  TORCH_CHECK(part.numel() == grid * 32 * 16, what, ": part must be [", grid,
              "][32][16]");
  const int rc = geops_conv5c1_wrw(
      x.data_ptr(), kind, c1_table_ptr(table, kind),
      (const unsigned short*)g.data_ptr(),
      mask ? mask->data_ptr<uint8_t>() : nullptr, part.data_ptr<float>(),
      (int)N, (int)H, (int)W, (int)grid, cur_stream());
  TORCH_CHECK(rc == 0, what, ": unsupported geometry H=", H, " W=", W,
              " (even W in 6..228; even H for the pooled form)");
  launch_check(what);
}

// Weight + bias gradient slabs part[n_wg][32][16] (rows 0..24 the taps
// kh*5+kw, row 25 the bias, rows 26..31 zero) from the full-resolution
// gradient go [N][Ho][Wo][16]; the default grid is min(768, N*ceil(Ho/2)).
void conv5c1_wrw(torch::Tensor x, torch::Tensor go, torch::Tensor part,
                 int64_t N, int64_t H, int64_t W, int64_t n_wg,
                 c10::optional<torch::Tensor> table) {
  c1_wrw("conv5c1_wrw", x, go, nullptr, part, N, H, W, n_wg,
         table.value_or(torch::Tensor()));
}

// The same from the POOLED gradient gp [N][Ho/2][Wo/2][16] and its
// argmax codes: the kernel unpools while staging.
void conv5c1_wrw_unpool(torch::Tensor x, torch::Tensor gp, torch::Tensor mask,
                        torch::Tensor part, int64_t N, int64_t H, int64_t W,
                        int64_t n_wg, c10::optional<torch::Tensor> table) {
  c1_wrw("conv5c1_wrw_unpool", x, gp, &mask, part, N, H, W, n_wg,
         table.value_or(torch::Tensor()));
}

// ---- first dense layer layout kernels (fc.hip) ----

void check_fc_operand(const torch::Tensor& t, torch::ScalarType dtype,
                      int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, name, " has the wrong dtype");
  TORCH_CHECK(t.numel() == numel, name, " has ", t.numel(),
              " elements, expected ", numel);
  // bf16 operands move as 16-byte vectors; the fp32 weight side is
  // accessed dword-wise (HW may be odd) and needs no more than that
  if (dtype != torch::kFloat32)
    TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, name,
                " must be 16-byte aligned");
}

// fp32 master weight [O][C*HW] (NCHW-flatten order) -> bf16 [O][HW*C],
// the data-gradient GEMM's weight operand.
torch::Tensor fc_w_permute_bf16(torch::Tensor w, int64_t O, int64_t C,
                                int64_t HW) {
  check_fc_operand(w, torch::kFloat32, O * C * HW, "weight");
  auto wp = torch::empty({O, HW * C}, w.options().dtype(torch::kBFloat16));
  const int rc = geops_fc_w_permute_bf16(
      w.data_ptr<float>(), (unsigned short*)wp.data_ptr(), (int)O, (int)C,
      (int)HW, cur_stream());
  TORCH_CHECK(rc == 0, "fc_w_permute_bf16: unsupported geometry O=", O,
              " C=", C, " HW=", HW);
  launch_check("fc_w_permute_bf16");
  return wp;
}

// bf16 [O][HW*C] -> fp32 [O][C*HW]: the inverse, for the weight gradient.
torch::Tensor fc_w_unpermute_f32(torch::Tensor gp, int64_t O, int64_t C,
                                 int64_t HW) {
  check_fc_operand(gp, torch::kBFloat16, O * C * HW, "permuted gradient");
  auto g = torch::empty({O, C * HW}, gp.options().dtype(torch::kFloat32));
  const int rc = geops_fc_w_unpermute_f32(
      (const unsigned short*)gp.data_ptr(), g.data_ptr<float>(), (int)O,
      (int)C, (int)HW, cur_stream());
  TORCH_CHECK(rc == 0, "fc_w_unpermute_f32: unsupported geometry O=", O,
              " C=", C, " HW=", HW);
  launch_check("fc_w_unpermute_f32");
  return g;
}

// The kernels are launched on the current stream, which belongs to the
// current device: an operand from another device would be written by a
// queue that does not own it.
void check_on_current_device(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.get_device() == at::cuda::current_device(), name,
              " is on device ", t.get_device(),
              ", the current device is ", (int)at::cuda::current_device());
}

// fp32 master weight [O][C*HW] -> (wb, wp): wb bf16 [O][C*HW], the bits
// of w.to(bfloat16) (the forward GEMM's operand), and, with want_perm,
// wp bf16 [O][HW*C], the bits of fc_w_permute_bf16(w); otherwise wp is
// None and that half is skipped. One read of the weight serves both.
// wb_out / wp_out place the outputs in caller-given storage (wb needs
// 4 B alignment, wp 16 B); by default both are freshly allocated.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> fc_w_pack2_bf16(
    torch::Tensor w, int64_t O, int64_t C, int64_t HW, bool want_perm,
    c10::optional<torch::Tensor> wb_out,
    c10::optional<torch::Tensor> wp_out) {
  check_fc_operand(w, torch::kFloat32, O * C * HW, "weight");
  check_on_current_device(w, "weight");
  const auto opts = w.options().dtype(torch::kBFloat16);
  torch::Tensor wb;
  if (wb_out.has_value()) {
    wb = *wb_out;
    TORCH_CHECK(wb.is_cuda() && wb.is_contiguous() &&
                    wb.scalar_type() == torch::kBFloat16 &&
                    wb.numel() == O * C * HW,
                "wb_out must be a contiguous GPU bf16 tensor of ",
                O * C * HW, " elements");
    TORCH_CHECK(((uintptr_t)wb.data_ptr() & 3) == 0,
                "wb_out must be 4-byte aligned");
    TORCH_CHECK(wb.device() == w.device(),
                "wb_out must be on the weight's device");
  } else {
    wb = torch::empty({O, C * HW}, opts);
  }
  c10::optional<torch::Tensor> wp;
  if (want_perm) {
    if (wp_out.has_value()) {
      check_fc_operand(*wp_out, torch::kBFloat16, O * C * HW, "wp_out");
      TORCH_CHECK(wp_out->device() == w.device(),
                  "wp_out must be on the weight's device");
      wp = *wp_out;
    } else {
      wp = torch::empty({O, HW * C}, opts);
    }
  }
  const int rc = geops_fc_w_pack2_bf16(
      w.data_ptr<float>(), (unsigned short*)wb.data_ptr(),
      wp.has_value() ? (unsigned short*)wp->data_ptr() : nullptr, (int)O,
      (int)C, (int)HW, cur_stream());
  TORCH_CHECK(rc == 0, "fc_w_pack2_bf16: unsupported geometry O=", O,
              " C=", C, " HW=", HW);
  launch_check("fc_w_pack2_bf16");
  return {wb, wp};
}

// fc_w_unpermute_f32 into a caller-given dense fp32 destination of
// O*C*HW elements (any 4 B-aligned offset of a larger buffer), with a
// -0 stored as +0: the bytes `zeros + fc_w_unpermute_f32(gp)` has.
void fc_w_unpermute_into(torch::Tensor gp, torch::Tensor dst, int64_t O,
                         int64_t C, int64_t HW) {
  check_fc_operand(gp, torch::kBFloat16, O * C * HW, "permuted gradient");
  check_fc_operand(dst, torch::kFloat32, O * C * HW, "destination");
  TORCH_CHECK(dst.device() == gp.device(),
              "destination must be on the permuted gradient's device");
  check_on_current_device(gp, "permuted gradient");
  const int rc = geops_fc_w_unpermute_into(
      (const unsigned short*)gp.data_ptr(), dst.data_ptr<float>(), (int)O,
      (int)C, (int)HW, cur_stream());
  TORCH_CHECK(rc == 0, "fc_w_unpermute_into: unsupported geometry O=", O,
              " C=", C, " HW=", HW);
  launch_check("fc_w_unpermute_into");
}

// channels_last activation [N][HW*C] -> NCHW-flatten order [N][C*HW],
// bit-exact with torch.flatten(x, 1) of the channels_last tensor.
torch::Tensor fc_flatten_nchw(torch::Tensor x, int64_t N, int64_t C,
                              int64_t HW) {
  check_fc_operand(x, torch::kBFloat16, N * C * HW, "x");
  auto y = torch::empty({N, C * HW}, x.options());
  const int rc = geops_fc_flatten_nchw(
      (const unsigned short*)x.data_ptr(), (unsigned short*)y.data_ptr(),
      (int)N, (int)C, (int)HW, cur_stream());
  TORCH_CHECK(rc == 0, "fc_flatten_nchw: unsupported geometry N=", N,
              " C=", C, " HW=", HW);
  launch_check("fc_flatten_nchw");
  return y;
}

// The summed wrw slab `full` fp32 [T16][CO] -> the gradients of a conv
// weight [CO][CIr][5][5] and its bias [CO], written as x + 0.0f into
// caller-given fp32 destinations (finalize.hip): dw with the weight's
// shape and any dense strides (OIHW or channels_last), db contiguous;
// either may be None. idx is the int64 unpack table of the weight shape.
void conv5_wrw_finalize(torch::Tensor full, torch::Tensor idx,
                        c10::optional<torch::Tensor> dw,
                        c10::optional<torch::Tensor> db, int64_t CO,
                        int64_t CIr, int64_t T16) {
  TORCH_CHECK(full.is_cuda() && full.is_contiguous() &&
                  full.scalar_type() == torch::kFloat32 &&
                  full.numel() == T16 * CO,
              "full must be a contiguous GPU fp32 tensor of ", T16 * CO,
              " elements");
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() &&
                  idx.scalar_type() == torch::kInt64 &&
                  idx.numel() == CO * CIr * 25,
              "idx must be a contiguous GPU int64 tensor of ", CO * CIr * 25,
              " elements");
  TORCH_CHECK(idx.device() == full.device(), "idx must be on full's device");
  check_on_current_device(full, "full");
  TORCH_CHECK(dw.has_value() || db.has_value(), "no destination given");
  float *pw = nullptr, *pb = nullptr;
  long long st[4] = {0, 0, 0, 0};
  if (dw.has_value()) {
    const auto& t = *dw;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                    t.dim() == 4 && t.size(0) == CO && t.size(1) == CIr &&
                    t.size(2) == 5 && t.size(3) == 5 &&
                    t.is_non_overlapping_and_dense(),
                "dw must be a dense GPU fp32 tensor of shape [", CO, "][",
                CIr, "][5][5]");
    TORCH_CHECK(t.device() == full.device(), "dw must be on full's device");
    for (int d = 0; d < 4; ++d) st[d] = t.stride(d);
    pw = t.data_ptr<float>();
  }
  if (db.has_value()) {
    const auto& t = *db;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                    t.is_contiguous() && t.numel() == CO,
                "db must be a contiguous GPU fp32 tensor of ", CO,
                " elements");
    TORCH_CHECK(t.device() == full.device(), "db must be on full's device");
    pb = t.data_ptr<float>();
  }
  const int rc = geops_conv5_wrw_finalize(
      full.data_ptr<float>(), (const long long*)idx.data_ptr<int64_t>(), pw,
      pb, (int)CO, (int)CIr, (int)T16, st[0], st[1], st[2], st[3],
      cur_stream());
  TORCH_CHECK(rc == 0, "conv5_wrw_finalize: unsupported geometry CO=", CO,
              " CIr=", CIr, " T16=", T16);
  launch_check("conv5_wrw_finalize");
}

// One launch over up to 8 (src, dst) pairs of contiguous GPU tensors of
// equal length on the current device (finalize.hip). kind 0: fp32 -> bf16,
// kind 1: bf16 -> fp32 stored as x + 0.0f, kind 2: dst fp32 cleared.
static void many_launch(int kind, const char* what,
                        const std::vector<torch::Tensor>& src,
                        const std::vector<torch::Tensor>& dst) {
  const auto sdt = kind == 0 ? torch::kFloat32 : torch::kBFloat16;
  const auto ddt = kind == 0 ? torch::kBFloat16 : torch::kFloat32;
  TORCH_CHECK(!dst.empty() && dst.size() <= 8, what,
              ": 1 to 8 tensors per launch, got ", dst.size());
  TORCH_CHECK(kind == 2 || src.size() == dst.size(), what,
              ": as many sources as destinations");
  const void* ps[8];
  void* pd[8];
  long long n[8];
  for (size_t k = 0; k < dst.size(); ++k) {
    const auto& d = dst[k];
    TORCH_CHECK(d.is_cuda() && d.is_contiguous() && d.scalar_type() == ddt,
                what, ": destination ", k, " must be a contiguous GPU ",
                ddt, " tensor");
    check_on_current_device(d, "destination");
    pd[k] = d.data_ptr();
    n[k] = d.numel();
    ps[k] = nullptr;
    if (kind != 2) {
      const auto& s = src[k];
      TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                      s.scalar_type() == sdt && s.numel() == d.numel() &&
                      s.device() == d.device(),
                  what, ": source ", k, " must be a contiguous GPU ", sdt,
                  " tensor of its destination's length and device");
      ps[k] = s.data_ptr();
    }
  }
  const int rc = geops_many(kind, (int)dst.size(), ps, pd, n, cur_stream());
  TORCH_CHECK(rc == 0, what, ": nothing to do (every tensor is empty)");
  launch_check(what);
}

// The bf16 copies of up to 8 fp32 tensors (the bits of t.to(bfloat16)),
// each a fresh tensor of its source's shape, from one launch.
std::vector<torch::Tensor> cast_many_f32_bf16(
    std::vector<torch::Tensor> src) {
  std::vector<torch::Tensor> dst;
  for (const auto& s : src)
    dst.push_back(torch::empty(s.sizes(),
                               s.options().dtype(torch::kBFloat16)));
  many_launch(0, "cast_many_f32_bf16", src, dst);
  return dst;
}

// bf16 tensors -> caller-given fp32 destinations, stored as x + 0.0f:
// the bytes `zeros + src.float()` has.
void cast_many_bf16_f32_into(std::vector<torch::Tensor> src,
                             std::vector<torch::Tensor> dst) {
  many_launch(1, "cast_many_bf16_f32_into", src, dst);
}

void zero_many_f32(std::vector<torch::Tensor> dst) {
  many_launch(2, "zero_many_f32", {}, dst);
}

void pad_ch3to4_nhwc(torch::Tensor in, torch::Tensor out, int64_t npix) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda());
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16);
  const bool fp32 = in.scalar_type() == torch::kFloat32;
  TORCH_CHECK(fp32 || in.scalar_type() == torch::kBFloat16);
  geops_pad_ch3to4_nhwc(in.data_ptr(), (unsigned short*)out.data_ptr(),
                        npix, fp32 ? 1 : 0, cur_stream());
  launch_check("pad_ch3to4_nhwc");
}

// Pack an fp32 conv weight into bf16 MFMA fragment order through one or
// two gather tables of ops/conv.py (index == weight.numel() means zero)
// in one launch; returns one packed tensor per table.
std::vector<torch::Tensor> conv5_pack_frags(torch::Tensor weight,
                                            torch::Tensor idx0,
                                            c10::optional<torch::Tensor> idx1) {
  TORCH_CHECK(weight.is_cuda() && weight.is_contiguous() &&
                  weight.scalar_type() == torch::kFloat32,
              "conv5_pack_frags: weight must be contiguous fp32 on the GPU");
  const bool two = idx1.has_value() && idx1->defined();
  auto check_idx = [&](const torch::Tensor& t) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                    t.scalar_type() == torch::kInt64 &&
                    t.device() == weight.device() && t.numel() > 0 &&
                    t.numel() % 8 == 0,
                "conv5_pack_frags: index tables are contiguous int64 on the "
                "weight's device, a multiple of 8 long");
  };
  check_idx(idx0);
  if (two) check_idx(*idx1);
  const auto opts = weight.options().dtype(torch::kBFloat16);
  std::vector<torch::Tensor> out;
  out.push_back(torch::empty({idx0.numel()}, opts));
  if (two) out.push_back(torch::empty({idx1->numel()}, opts));
  const int rc = geops_conv5_pack_frags(
      weight.data_ptr<float>(), (long long)weight.numel(),
      (const long long*)idx0.data_ptr<int64_t>(),
      (unsigned short*)out[0].data_ptr(), (long long)idx0.numel(),
      two ? (const long long*)idx1->data_ptr<int64_t>() : nullptr,
      two ? (unsigned short*)out[1].data_ptr() : nullptr,
      two ? (long long)idx1->numel() : 0LL, cur_stream());
  TORCH_CHECK(rc == 0, "conv5_pack_frags: bad table sizes");
  launch_check("conv5_pack_frags");
  return out;
}

void sgd_update(torch::Tensor w, torch::Tensor g, double lr, double wd,
                double rescale) {
  check_f32(w, "w"); check_f32(g, "g");
  check_same_numel(w, g, "g");
  geops_sgd_update(w.data_ptr<float>(), g.data_ptr<float>(), (float)lr,
                   (float)wd, (float)rescale, w.numel(), cur_stream());
  launch_check("sgd_update");
}

void sgd_mom_update(torch::Tensor w, torch::Tensor g, torch::Tensor mom,
                    double lr, double momentum, double wd, double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(mom, "mom");
  check_same_numel(w, g, "g"); check_same_numel(w, mom, "mom");
  geops_sgd_mom_update(w.data_ptr<float>(), g.data_ptr<float>(),
                       mom.data_ptr<float>(), (float)lr, (float)momentum,
                       (float)wd, (float)rescale, w.numel(), cur_stream());
  launch_check("sgd_mom_update");
}

void adam_update(torch::Tensor w, torch::Tensor g, torch::Tensor m,
                 torch::Tensor v, int64_t t, double lr, double beta1,
                 double beta2, double eps, double wd, double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(m, "m"); check_f32(v, "v");
  check_same_numel(w, g, "g"); check_same_numel(w, m, "m");
  check_same_numel(w, v, "v");
  const double lr_t = adam_lr_t(lr, beta1, beta2, t);
  geops_adam_update(w.data_ptr<float>(), g.data_ptr<float>(),
                    m.data_ptr<float>(), v.data_ptr<float>(), (float)lr_t,
                    (float)beta1, (float)beta2, (float)eps, (float)wd,
                    (float)rescale, w.numel(), cur_stream());
  launch_check("adam_update");
}

void dcasgd_update(torch::Tensor w, torch::Tensor g, torch::Tensor prev_w,
                   torch::Tensor mom, double lr, double lamda,
                   double momentum, double wd, double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(prev_w, "prev_w");
  const bool has_mom = mom.defined() && mom.numel() > 0;
  if (has_mom) check_f32(mom, "mom");
  check_same_numel(w, g, "g"); check_same_numel(w, prev_w, "prev_w");
  if (has_mom) check_same_numel(w, mom, "mom");
  geops_dcasgd_update(w.data_ptr<float>(), g.data_ptr<float>(),
                      prev_w.data_ptr<float>(),
                      has_mom ? mom.data_ptr<float>() : nullptr, (float)lr,
                      (float)lamda, (float)momentum, (float)wd,
                      (float)rescale, w.numel(), has_mom, cur_stream());
  launch_check("dcasgd_update");
}

void rmsprop_update(torch::Tensor w, torch::Tensor g, torch::Tensor n,
                    double lr, double rho, double eps, double wd,
                    double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(n, "n");
  check_same_numel(w, g, "g"); check_same_numel(w, n, "n");
  geops_rmsprop_update(w.data_ptr<float>(), g.data_ptr<float>(),
                       n.data_ptr<float>(), (float)lr, (float)rho,
                       (float)eps, (float)wd, (float)rescale, w.numel(),
                       cur_stream());
  launch_check("rmsprop_update");
}

void adagrad_update(torch::Tensor w, torch::Tensor g, torch::Tensor h,
                    double lr, double eps, double wd, double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(h, "h");
  check_same_numel(w, g, "g"); check_same_numel(w, h, "h");
  geops_adagrad_update(w.data_ptr<float>(), g.data_ptr<float>(),
                       h.data_ptr<float>(), (float)lr, (float)eps,
                       (float)wd, (float)rescale, w.numel(), cur_stream());
  launch_check("adagrad_update");
}

void signsgd_update(torch::Tensor w, torch::Tensor g, double lr, double wd,
                    double rescale) {
  check_f32(w, "w"); check_f32(g, "g");
  check_same_numel(w, g, "g");
  geops_signsgd_update(w.data_ptr<float>(), g.data_ptr<float>(), (float)lr,
                       (float)wd, (float)rescale, w.numel(), cur_stream());
  launch_check("signsgd_update");
}

void signum_update(torch::Tensor w, torch::Tensor g, torch::Tensor mom,
                   double lr, double momentum, double wd, double rescale) {
  check_f32(w, "w"); check_f32(g, "g"); check_f32(mom, "mom");
  check_same_numel(w, g, "g"); check_same_numel(w, mom, "mom");
  geops_signum_update(w.data_ptr<float>(), g.data_ptr<float>(),
                      mom.data_ptr<float>(), (float)lr, (float)momentum,
                      (float)wd, (float)rescale, w.numel(), cur_stream());
  launch_check("signum_update");
}

// -- row-sparse push (rowsparse.hip) ---------------------------------------
// No 16-byte demand here: stored values and optimizer state may be views
// at odd element offsets; the launchers pick the scalar instantiation.
void check_rsp_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}

void check_rsp_i64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous() && t.dim() == 1, name,
              " must be contiguous 1-d");
  TORCH_CHECK(t.scalar_type() == torch::kInt64, name, " must be int64");
}

const long long* i64p(const torch::Tensor& t) {
  return (const long long*)t.data_ptr<int64_t>();
}

// shared shape contract of scatter / row updates: table [rows][width],
// merged [n_u][width], ids [n_u]
void check_rsp_rows(const torch::Tensor& table, const torch::Tensor& ids,
                    const torch::Tensor& merged) {
  check_rsp_f32(table, "table"); check_rsp_f32(merged, "merged");
  check_rsp_i64(ids, "ids");
  TORCH_CHECK(table.dim() == 2 && merged.dim() == 2,
              "table and merged must be 2-d");
  TORCH_CHECK(merged.size(0) == ids.numel() &&
              merged.size(1) == table.size(1),
              "merged must be [len(ids)][width]");
}

void check_rsp_state(const torch::Tensor& s, const torch::Tensor& table,
                     const char* name) {
  check_rsp_f32(s, name);
  TORCH_CHECK(s.sizes() == table.sizes(), name, " must match the table");
}

void rsp_merge(torch::Tensor sorted_ids, torch::Tensor perm,
               torch::Tensor seg, torch::Tensor vals, torch::Tensor out_ids,
               torch::Tensor out_vals) {
  check_rsp_i64(sorted_ids, "sorted_ids"); check_rsp_i64(perm, "perm");
  check_rsp_i64(seg, "seg"); check_rsp_i64(out_ids, "out_ids");
  check_rsp_f32(vals, "vals"); check_rsp_f32(out_vals, "out_vals");
  const long long nnz = sorted_ids.numel();
  TORCH_CHECK(perm.numel() == nnz && seg.numel() == nnz &&
              out_ids.numel() == nnz, "id arrays must all hold nnz entries");
  TORCH_CHECK(vals.dim() == 2 && vals.size(0) == nnz &&
              out_vals.sizes() == vals.sizes(),
              "vals and out_vals must be [nnz][width]");
  geops_rsp_merge(i64p(sorted_ids), i64p(perm), i64p(seg),
                  vals.data_ptr<float>(),
                  (long long*)out_ids.data_ptr<int64_t>(),
                  out_vals.data_ptr<float>(), nnz, vals.size(1),
                  cur_stream());
  launch_check("rsp_merge");
}

void rsp_scatter(torch::Tensor dense, torch::Tensor ids,
                 torch::Tensor merged, bool accumulate) {
  check_rsp_rows(dense, ids, merged);
  geops_rsp_scatter(i64p(ids), merged.data_ptr<float>(),
                    dense.data_ptr<float>(), ids.numel(), dense.size(0),
                    dense.size(1), accumulate, cur_stream());
  launch_check("rsp_scatter");
}

void rsp_sgd_update(torch::Tensor w, torch::Tensor ids, torch::Tensor merged,
                    double lr, double wd, double rescale) {
  check_rsp_rows(w, ids, merged);
  geops_rsp_sgd_update(i64p(ids), merged.data_ptr<float>(),
                       w.data_ptr<float>(), (float)lr, (float)wd,
                       (float)rescale, ids.numel(), w.size(0), w.size(1),
                       cur_stream());
  launch_check("rsp_sgd_update");
}

void rsp_sgd_mom_update(torch::Tensor w, torch::Tensor ids,
                        torch::Tensor merged, torch::Tensor mom, double lr,
                        double momentum, double wd, double rescale) {
  check_rsp_rows(w, ids, merged);
  check_rsp_state(mom, w, "mom");
  geops_rsp_sgd_mom_update(i64p(ids), merged.data_ptr<float>(),
                           w.data_ptr<float>(), mom.data_ptr<float>(),
                           (float)lr, (float)momentum, (float)wd,
                           (float)rescale, ids.numel(), w.size(0), w.size(1),
                           cur_stream());
  launch_check("rsp_sgd_mom_update");
}

void rsp_adam_update(torch::Tensor w, torch::Tensor ids, torch::Tensor merged,
                     torch::Tensor m, torch::Tensor v, int64_t t, double lr,
                     double beta1, double beta2, double eps, double wd,
                     double rescale) {
  check_rsp_rows(w, ids, merged);
  check_rsp_state(m, w, "m"); check_rsp_state(v, w, "v");
  const double lr_t = adam_lr_t(lr, beta1, beta2, t);
  geops_rsp_adam_update(i64p(ids), merged.data_ptr<float>(),
                        w.data_ptr<float>(), m.data_ptr<float>(),
                        v.data_ptr<float>(), (float)lr_t, (float)beta1,
                        (float)beta2, (float)eps, (float)wd, (float)rescale,
                        ids.numel(), w.size(0), w.size(1), cur_stream());
  launch_check("rsp_adam_update");
}

void rsp_adagrad_update(torch::Tensor w, torch::Tensor ids,
                        torch::Tensor merged, torch::Tensor h, double lr,
                        double eps, double wd, double rescale) {
  check_rsp_rows(w, ids, merged);
  check_rsp_state(h, w, "h");
  geops_rsp_adagrad_update(i64p(ids), merged.data_ptr<float>(),
                           w.data_ptr<float>(), h.data_ptr<float>(),
                           (float)lr, (float)eps, (float)wd, (float)rescale,
                           ids.numel(), w.size(0), w.size(1), cur_stream());
  launch_check("rsp_adagrad_update");
}

// -- layer-wise LARS (lars.hip) ---------------------------------------------
// seg_off[S+1] cuts the n elements into S segments, tile_start[S+1] is the
// prefix sum of ceil(len_s / LARS_TILE); ops builds and validates both on
// the host (the kernels bound every tile by n once more). VEC = 4 needs
// 16 B-aligned operands and offsets that are multiples of 4: `vec4` says
// that the offsets are, the pointers are looked at here. n_wg: 0 = default
// grid, > 0 that many workgroups (the tests' hook, as conv5_dgrad_nwg_nhwc).
struct LarsArgs {
  int S;
  long long total, n;
  int vec;
};

LarsArgs lars_check(const char* what, const torch::Tensor& w,
                    std::initializer_list<const torch::Tensor*> same,
                    const torch::Tensor& seg_off,
                    const torch::Tensor& tile_start,
                    const torch::Tensor& ratio, int64_t total, bool vec4,
                    int64_t n_wg) {
  check_rsp_f32(w, "w");
  check_rsp_f32(ratio, "ratio");
  check_rsp_i64(seg_off, "seg_off");
  check_rsp_i64(tile_start, "tile_start");
  bool aligned = ((uintptr_t)w.data_ptr() & 15) == 0;
  for (const torch::Tensor* t : same) {
    check_rsp_f32(*t, "g / mom");
    check_same_numel(w, *t, "g / mom");
    TORCH_CHECK(t->device() == w.device(), what, ": operands on one device");
    aligned = aligned && ((uintptr_t)t->data_ptr() & 15) == 0;
  }
  const int64_t S = ratio.numel(), n = w.numel();
  TORCH_CHECK(seg_off.numel() == S + 1 && tile_start.numel() == S + 1, what,
              ": seg_off and tile_start hold one entry more than ratio");
  TORCH_CHECK(seg_off.device() == w.device() &&
                  tile_start.device() == w.device() &&
                  ratio.device() == w.device(),
              what, ": tables on w's device");
  TORCH_CHECK(n <= INT32_MAX && S <= INT32_MAX, what, " serves n < 2^31");
  // a tile holds at least one element, and every segment at most one
  // partial tile
  TORCH_CHECK(total >= 0 && total <= n &&
                  total <= n / geops_lars_tile() + S,
              what, ": tile count ", total, " does not fit n = ", n);
  TORCH_CHECK(n_wg >= 0 && n_wg <= 65536, what, ": bad n_wg");
  return LarsArgs{(int)S, (long long)total, (long long)n,
                  (vec4 && aligned) ? 4 : 1};
}

void lars_sumsq(torch::Tensor w, torch::Tensor g, torch::Tensor seg_off,
                torch::Tensor tile_start, torch::Tensor partials,
                torch::Tensor ratio, int64_t total, double wd, bool vec4,
                int64_t n_wg) {
  const LarsArgs a = lars_check("lars_sumsq", w, {&g}, seg_off, tile_start,
                                ratio, total, vec4, n_wg);
  check_rsp_f32(partials, "partials");
  TORCH_CHECK(((uintptr_t)partials.data_ptr() & 7) == 0 &&
                  partials.numel() >= 2 * total,
              "lars_sumsq: partials holds one 8 B-aligned pair per tile");
  TORCH_CHECK(partials.device() == w.device(),
              "lars_sumsq: workspace on w's device");
  if (a.S == 0) return;
  geops_lars_sumsq(w.data_ptr<float>(), g.data_ptr<float>(), i64p(seg_off),
                   i64p(tile_start), partials.data_ptr<float>(),
                   ratio.data_ptr<float>(), a.S, a.total, a.n, wd, a.vec,
                   (int)n_wg, cur_stream());
  launch_check("lars_sumsq");
}

// mom empty (torch.Tensor()): plain sgd, as for dcasgd's mom
void lars_update(torch::Tensor w, torch::Tensor g, torch::Tensor mom,
                 torch::Tensor seg_off, torch::Tensor tile_start,
                 torch::Tensor ratio, int64_t total, double lr, double lbmult,
                 double momentum, double wd, double rescale, bool vec4,
                 int64_t n_wg) {
  const bool has_mom = mom.defined() && mom.numel() > 0;
  const LarsArgs a =
      has_mom ? lars_check("lars_update", w, {&g, &mom}, seg_off, tile_start,
                           ratio, total, vec4, n_wg)
              : lars_check("lars_update", w, {&g}, seg_off, tile_start, ratio,
                           total, vec4, n_wg);
  if (a.total == 0) return;
  geops_lars_update(w.data_ptr<float>(), g.data_ptr<float>(),
                    has_mom ? mom.data_ptr<float>() : nullptr, i64p(seg_off),
                    i64p(tile_start), ratio.data_ptr<float>(), a.S, a.total,
                    a.n, lr, lbmult, (float)momentum, (float)wd,
                    (float)rescale, a.vec, (int)n_wg, cur_stream());
  launch_check("lars_update");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "geomx_amd gfx950 kernel library";
  m.def("quantize_2bit", &quantize_2bit);
  m.def("dequantize_2bit", &dequantize_2bit);
  m.def("bsc_momentum", &bsc_momentum);
  m.def("bsc_pack", &bsc_pack);
  m.def("bsc_pull_pack", &bsc_pull_pack);
  m.def("bsc_compress_fused", &bsc_compress_fused);
  m.def("bsc_unpack", &bsc_unpack);
  m.def("bsc_boundary", &bsc_boundary);
  // samples the one-workgroup form of k_bsc_boundary holds in LDS
  m.attr("BSC_BOUNDARY_CAP") = geops_bsc_boundary_cap();
  m.def("dgt_contribution", &dgt_contribution);
  m.def("quantize_4bit", &quantize_4bit);
  m.def("dequantize_4bit", &dequantize_4bit);
  m.def("wire_sum_2bit", &wire_sum_2bit);
  m.def("wire_sum_f16", &wire_sum_f16);
  m.def("wire_sum_dgt", &wire_sum_dgt);
  m.def("wire_sum_bsc", &wire_sum_bsc);
  m.def("wire_sum_bsc_dgt", &wire_sum_bsc_dgt);
  // output elements per tile of k_wire_sum_bsc
  m.attr("WIRE_BSC_TILE") = geops_wire_sum_bsc_tile();
  m.def("dgt_encode", &dgt_encode);
  m.def("fp8_encode", &fp8_encode);
  m.def("wire_sum_fp8", &wire_sum_fp8);
  m.def("conv5_nhwc", &conv5_nhwc);
  m.def("pad_ch3to4_nhwc", &pad_ch3to4_nhwc);
  m.def("conv5_pack_frags", &conv5_pack_frags, py::arg("weight"),
        py::arg("idx0"), py::arg("idx1") = py::none());
  m.def("conv5_wrw_nhwc", &conv5_wrw_nhwc);
  m.def("conv5_wrw_unpool_nhwc", &conv5_wrw_unpool_nhwc);
  m.def("conv5_dgrad_unpool_nhwc", &conv5_dgrad_unpool_nhwc);
  m.def("conv5_direct_nhwc", &conv5_direct_nhwc);
  m.def("conv5_dgrad_nwg_nhwc", &conv5_dgrad_nwg_nhwc);
  m.def("conv5_pool_nhwc", &conv5_pool_nhwc);
  // (the trailing table: bf16 [1][256] with a uint8 x, else left out)
  m.def("conv5c1_pool", &conv5c1_pool, py::arg("x"), py::arg("w_frags"),
        py::arg("bias"), py::arg("out"), py::arg("mask"), py::arg("N"),
        py::arg("H"), py::arg("W"), py::arg("n_wg"),
        py::arg("table") = py::none());
  m.def("conv5c1_wrw", &conv5c1_wrw, py::arg("x"), py::arg("go"),
        py::arg("part"), py::arg("N"), py::arg("H"), py::arg("W"),
        py::arg("n_wg"), py::arg("table") = py::none());
  m.def("conv5c1_wrw_unpool", &conv5c1_wrw_unpool, py::arg("x"),
        py::arg("gp"), py::arg("mask"), py::arg("part"), py::arg("N"),
        py::arg("H"), py::arg("W"), py::arg("n_wg"),
        py::arg("table") = py::none());
  m.def("conv5_pool_nwg_nhwc", &conv5_pool_nwg_nhwc);
  m.def("conv5_pool_x32_nhwc", &conv5_pool_x32_nhwc);
  m.def("conv5_pool_x32_nwg_nhwc", &conv5_pool_x32_nwg_nhwc);
  m.def("conv5_pool_u8_nhwc", &conv5_pool_u8_nhwc);
  m.def("conv5_pool_u8_nwg_nhwc", &conv5_pool_u8_nwg_nhwc);
  m.def("fc_w_permute_bf16", &fc_w_permute_bf16);
  m.def("fc_w_unpermute_f32", &fc_w_unpermute_f32);
  m.def("fc_flatten_nchw", &fc_flatten_nchw);
  m.def("fc_w_pack2_bf16", &fc_w_pack2_bf16, py::arg("w"), py::arg("O"),
        py::arg("C"), py::arg("HW"), py::arg("want_perm"),
        py::arg("wb_out") = py::none(), py::arg("wp_out") = py::none());
  m.def("fc_w_unpermute_into", &fc_w_unpermute_into);
  m.def("conv5_wrw_finalize", &conv5_wrw_finalize);
  m.def("cast_many_f32_bf16", &cast_many_f32_bf16);
  m.def("cast_many_bf16_f32_into", &cast_many_bf16_f32_into);
  m.def("zero_many_f32", &zero_many_f32);
  m.def("tr16_probe2", [](torch::Tensor in, torch::Tensor addr,
                          torch::Tensor out) {
    TORCH_CHECK(in.is_cuda() && addr.is_cuda() && out.is_cuda());
    TORCH_CHECK(in.numel() == 512 && addr.numel() == 64 &&
                out.numel() == 256);
    TORCH_CHECK(addr.scalar_type() == torch::kInt32);
    geops_tr16_probe2((const unsigned short*)in.data_ptr(),
                      addr.data_ptr<int32_t>(),
                      (unsigned short*)out.data_ptr(), cur_stream());
    launch_check("tr16_probe2");
  });
  m.def("tr16_probe", [](torch::Tensor in, torch::Tensor out) {
    TORCH_CHECK(in.is_cuda() && out.is_cuda());
    TORCH_CHECK(in.numel() == 64 && out.numel() == 256);
    geops_tr16_probe((const unsigned short*)in.data_ptr(),
                     (unsigned short*)out.data_ptr(), cur_stream());
    launch_check("tr16_probe");
  });
  m.def("relu_maxpool2_fwd", &relu_maxpool2_fwd);
  m.def("relu_maxpool2_bwd", &relu_maxpool2_bwd);
  m.def("sgd_update", &sgd_update);
  m.def("sgd_mom_update", &sgd_mom_update);
  m.def("adam_update", &adam_update);
  m.def("dcasgd_update", &dcasgd_update);
  m.def("rmsprop_update", &rmsprop_update);
  m.def("adagrad_update", &adagrad_update);
  m.def("signsgd_update", &signsgd_update);
  m.def("signum_update", &signum_update);
  m.def("lars_sumsq", &lars_sumsq);
  m.def("lars_update", &lars_update);
  // elements per tile of the LARS kernels
  m.attr("LARS_TILE") = geops_lars_tile();
  m.def("rsp_merge", &rsp_merge);
  m.def("rsp_scatter", &rsp_scatter);
  m.def("rsp_sgd_update", &rsp_sgd_update);
  m.def("rsp_sgd_mom_update", &rsp_sgd_mom_update);
  m.def("rsp_adam_update", &rsp_adam_update);
  m.def("rsp_adagrad_update", &rsp_adagrad_update);
}
