// The flagship conv1 stage from a uint8 image and a 256-entry value
// table: the TIN = uint8_t form of k_conv5_pool2_nhwc (conv5_pool2.h),
// which looks every byte up in the bf16 table while staging, inserts the
// zero 4th channel, and writes the padded bf16 copy that backward reads
// as a side output. It replaces the pass that expands the bytes to an
// fp32 image (ToTensor, with or without a per-channel normalisation) in
// front of the fp32 form. Built without packed fp32 instructions
// (setup.py), as that form is.

#include <hip/hip_runtime.h>

#include "conv5_common.h"
#include "conv5_pool2.h"

extern "C" {

// x [N][Hi][Wi][3] uint8, tab [3][256] bf16, CO = 16; out and mask as
// geops_conv5_pool_x32_nhwc gives them for the fp32 image table[c][x],
// whose padded bf16 copy is written to xb [N][Hi][Wi][4] unless xb is
// null. An item is 12 bytes in dword loads: Wi % 4 == 0 (a row is 3 * Wi
// bytes) and a 4 B aligned x; 16 B aligned xb, 4 B aligned tab. n_wg as
// in the fp32 form. Returns 0, or -1 for operands the kernel does not
// serve.
int geops_conv5_pool_u8_nhwc(const uint8_t* x, const bf16_t* tab,
                             const bf16_t* w_frags, const float* bias,
                             bf16_t* out, uint8_t* mask, bf16_t* xb, int Nn,
                             int Hi, int Wi, int Ho, int Wo, int CO, int n_wg,
                             hipStream_t s) {
  if (CO != 16 || Nn < 1 || Ho < 2 || Wo < 2 || (Ho & 1) || (Wo & 1) ||
      Hi != Ho + 4 || Wi != Wo + 4 || (Wi & 3) ||
      conv5_stage_width(Wo, 16, Wi) > 232 || !tab ||
      (((uintptr_t)x | (uintptr_t)tab) & 3) || ((uintptr_t)xb & 15))
    return -1;
  const long long blocks = (long long)Nn * (((Ho >> 1) + 1) >> 1);
  const long long g = n_wg > 0 ? n_wg : (blocks < 2048 ? blocks : 2048);
  hipLaunchKernelGGL((k_conv5_pool2_nhwc<232, uint8_t>), dim3((unsigned)g),
                     dim3(CONV_THREADS), 0, s, x, w_frags, bias, out, mask,
                     Nn, Hi, Wi, Ho, Wo, xb, tab);
  return 0;
}

}  // extern "C"
