// Torch bindings for the geomx_amd gfx950 kernel library: kernels.hip
// (kvstore compression, optimizer updates, fused ReLU+pool), conv.hip
// (5x5 conv forward / data gradient), convwrw2.hip (5x5 conv weight
// gradient, tr16 probes) and fc.hip (NHWC-native first dense layer
// layout kernels: permuting weight casts, transposing flatten).
//
// Thin checked wrappers: dtype/contiguity/device checks, stream plumbing
// (kernels run on the current torch stream so they order correctly with
// autograd/backward and RCCL collectives), and workspace management for
// the Bi-Sparse pack pipeline.

#include <torch/extension.h>

#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

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
  m.def("dgt_contribution", &dgt_contribution);
  m.def("quantize_4bit", &quantize_4bit);
  m.def("dequantize_4bit", &dequantize_4bit);
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
  m.def("conv5_pool_nwg_nhwc", &conv5_pool_nwg_nhwc);
  m.def("fc_w_permute_bf16", &fc_w_permute_bf16);
  m.def("fc_w_unpermute_f32", &fc_w_unpermute_f32);
  m.def("fc_flatten_nchw", &fc_flatten_nchw);
  m.def("fc_w_pack2_bf16", &fc_w_pack2_bf16, py::arg("w"), py::arg("O"),
        py::arg("C"), py::arg("HW"), py::arg("want_perm"),
        py::arg("wb_out") = py::none(), py::arg("wp_out") = py::none());
  m.def("fc_w_unpermute_into", &fc_w_unpermute_into);
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
  m.def("rsp_merge", &rsp_merge);
  m.def("rsp_scatter", &rsp_scatter);
  m.def("rsp_sgd_update", &rsp_sgd_update);
  m.def("rsp_sgd_mom_update", &rsp_sgd_mom_update);
  m.def("rsp_adam_update", &rsp_adam_update);
  m.def("rsp_adagrad_update", &rsp_adagrad_update);
}
