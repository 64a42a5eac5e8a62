// The server optimizers' update rules, written once for the dense kernels
// (kernels.hip) and the row-indexed ones (rowsparse.hip). A rule is a functor:
// hyper-parameters, NSTATE state tensors, and apply(w, g, s0, s1) for ONE
// element, mirroring the geomx_amd/ops/reference.py function named above it.
// The compiler contracts a*b + c, so expression and operand order decide the
// bits; tests/test_optim_golden_gpu.py holds every kernel to the recorded ones.
// Signum and DCASGD are not here: each has one kernel, which kept its own
// loop because it was slower through the shared one (see kernels.hip).

#pragma once

#include <hip/hip_runtime.h>

#define OPTIM_FN __device__ __forceinline__

// VEC consecutive floats of one lane; 4 is one 16 B-aligned access
template <int VEC> struct Granule;
template <> struct Granule<1> {
  float v[1];
  OPTIM_FN void load(const float* p) { v[0] = p[0]; }
  OPTIM_FN void store(float* p) const { p[0] = v[0]; }
};
template <> struct Granule<4> {
  float v[4];
  OPTIM_FN void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  OPTIM_FN void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// reference.sgd_update
struct SgdRule {
  float lr, wd, rescale;
  static constexpr int NSTATE = 0;
  OPTIM_FN void apply(float& w, float g, float&, float&) const {
    w -= lr * (g * rescale + wd * w);
  }
};

// reference.sgd_mom_update
struct SgdMomRule {
  float lr, momentum, wd, rescale;
  static constexpr int NSTATE = 1;
  OPTIM_FN void apply(float& w, float g, float& mom, float&) const {
    mom = mom * momentum - lr * (g * rescale + wd * w);
    w += mom;
  }
};

// reference.adam_update; lr_t: the host's bias-corrected rate
struct AdamRule {
  float lr_t, beta1, beta2, eps, wd, rescale;
  static constexpr int NSTATE = 2;
  OPTIM_FN void apply(float& w, float g, float& m, float& v) const {
    const float gg = g * rescale + wd * w;
    m = beta1 * m + (1.0f - beta1) * gg;
    v = beta2 * v + (1.0f - beta2) * gg * gg;
    w -= lr_t * m / (sqrtf(v) + eps);
  }
};

// reference.rmsprop_update
struct RmspropRule {
  float lr, rho, eps, wd, rescale;
  static constexpr int NSTATE = 1;
  OPTIM_FN void apply(float& w, float g, float& n, float&) const {
    const float gg = g * rescale + wd * w;
    n = rho * n + (1.0f - rho) * gg * gg;
    w -= lr * gg / (sqrtf(n) + eps);
  }
};

// reference.adagrad_update
struct AdagradRule {
  float lr, eps, wd, rescale;
  static constexpr int NSTATE = 1;
  OPTIM_FN void apply(float& w, float g, float& h, float&) const {
    const float gg = g * rescale + wd * w;
    h = h + gg * gg;
    w -= lr * gg / (sqrtf(h) + eps);
  }
};

OPTIM_FN float optim_sign(float x) {
  return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f);
}

// reference.signsgd_update
struct SignsgdRule {
  float lr, wd, rescale;
  static constexpr int NSTATE = 0;
  OPTIM_FN void apply(float& w, float g, float&, float&) const {
    w -= lr * optim_sign(g * rescale + wd * w);
  }
};

// One granule of one dense step: gradient at `g`, w and states at element
// offset `off`; a state the rule lacks is never turned into an address. Of
// two added products the compiler fuses ONE into an fma, picked by the order
// their operands were defined in: loading w first is part of the bits.
// k_rsp_update does not use this: see the comment on it in rowsparse.hip.
template <int VEC, typename OP>
OPTIM_FN void optim_apply(const OP& op, const float* g, float* w, float* s0,
                          float* s1, long long off) {
  Granule<VEC> gv, wv, a, b;
  wv.load(w + off);
  if (OP::NSTATE >= 1) a.load(s0 + off);
  if (OP::NSTATE >= 2) b.load(s1 + off);
  gv.load(g);
#pragma unroll
  for (int j = 0; j < VEC; ++j) op.apply(wv.v[j], gv.v[j], a.v[j], b.v[j]);
  wv.store(w + off);
  if (OP::NSTATE >= 1) a.store(s0 + off);
  if (OP::NSTATE >= 2) b.store(s1 + off);
}
