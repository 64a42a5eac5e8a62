// The flagship conv1 stage from the caller's fp32 image: the TIN = float
// form of k_conv5_pool2_nhwc (conv5_pool2.h), which converts to bf16 and
// inserts the zero 4th channel while staging, and writes the padded bf16
// copy that backward reads as a side output. It replaces the 3 -> 4
// channel pad pass (k_pad_ch3to4_nhwc<float>) in front of the forward.
// Built without packed fp32 instructions (setup.py).

#include <hip/hip_runtime.h>

#include "conv5_common.h"
#include "conv5_pool2.h"

extern "C" {

// x [N][Hi][Wi][3] fp32, CO = 16; out and mask as geops_conv5_pool_nhwc
// gives them for the padded bf16 copy of x, which is written to xb
// [N][Hi][Wi][4] unless xb is null. The 16 B loads and stores want
// Wi % 4 == 0 (a row is 12 * Wi bytes) and 16 B aligned x and xb.
// n_wg <= 0 picks the grid of the bf16 form (two resident rounds, 2048);
// n_wg > 0 is the test hook that lets small inputs reach the persistent
// loop. Returns 0, or -1 for operands the kernel does not serve.
int geops_conv5_pool_x32_nhwc(const float* x, const bf16_t* w_frags,
                              const float* bias, bf16_t* out, uint8_t* mask,
                              bf16_t* xb, int Nn, int Hi, int Wi, int Ho,
                              int Wo, int CO, int n_wg, hipStream_t s) {
  if (CO != 16 || Nn < 1 || Ho < 2 || Wo < 2 || (Ho & 1) || (Wo & 1) ||
      Hi != Ho + 4 || Wi != Wo + 4 || (Wi & 3) ||
      conv5_stage_width(Wo, 16, Wi) > 232 ||
      (((uintptr_t)x | (uintptr_t)xb) & 15))
    return -1;
  const long long blocks = (long long)Nn * (((Ho >> 1) + 1) >> 1);
  const long long g = n_wg > 0 ? n_wg : (blocks < 2048 ? blocks : 2048);
  hipLaunchKernelGGL((k_conv5_pool2_nhwc<232, float>), dim3((unsigned)g),
                     dim3(CONV_THREADS), 0, s, x, w_frags, bias, out, mask,
                     Nn, Hi, Wi, Ho, Wo, xb);
  return 0;
}

}  // extern "C"
