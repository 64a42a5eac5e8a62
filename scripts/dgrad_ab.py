#!/usr/bin/env python3
"""A/B of the conv2 data gradient at the flagship shape (N=512, pooled
grad 53x53x32 + argmax codes -> 110x110x16): the LDS row-sliding kernel
in its pooled form at several grid sizes, the direct kernel on the
scattered + physically padded gradient (the bit-exact oracle), and ATen.

    python scripts/dgrad_ab.py [--n-wg 512 1024 2048 4096]

Times are per call, hipEvent-timed over ITERS calls after warm-up."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from geomx_amd import _geops
from geomx_amd.ops import conv as C

DEV = "cuda:0"
N, CI, CO, H = 512, 16, 32, 110
Ho = H - 4
ITERS = 20


def bench(f):
    for _ in range(5):
        f()
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    beg.record()
    for _ in range(ITERS):
        f()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-wg", type=int, nargs="*", default=[])
    args = ap.parse_args()

    torch.manual_seed(3)
    x = torch.randn(N, CI, H, H, device=DEV, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    w = torch.randn(CO, CI, 5, 5, device=DEV, dtype=torch.bfloat16) * 0.05
    gp = torch.randn(N, Ho // 2, Ho // 2, CO, device=DEV,
                     dtype=torch.bfloat16).permute(0, 3, 1, 2)
    mask = torch.randint(0, 4, (gp.numel(),), device=DEV, dtype=torch.uint8)
    go = torch.empty(N, CO, Ho, Ho, dtype=torch.bfloat16, device=DEV,
                     memory_format=torch.channels_last)
    _geops.relu_maxpool2_bwd(gp, mask, go, N, CO, Ho, Ho)
    gop = F.pad(go, (4, 4, 4, 4)).contiguous(
        memory_format=torch.channels_last)
    w_frags = C._w_frags(w, C.build_dgrad_index(w.shape).to(DEV))
    dims = (N, Ho + 8, Ho + 8, H, H, CO, CI)

    def out():
        return torch.empty(N, CI, H, H, dtype=torch.bfloat16, device=DEV,
                           memory_format=torch.channels_last)

    gx = out()

    def pooled():
        _geops.conv5_dgrad_unpool_nhwc(gp, mask, w_frags, gx, *dims)

    def aten():
        return torch.ops.aten.convolution_backward(
            go, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [True, False, False])[0]

    pooled()
    got = gx.clone()
    err = (aten().float() - got.float()).abs().max().item()
    print(f"pooled LDS vs ATen: max |diff| {err:.4f}")
    print(f"ATen dgrad (full-resolution grad)   {bench(aten):8.4f} ms")
    print(f"pooled LDS dgrad, default grid      {bench(pooled):8.4f} ms")

    if hasattr(_geops, "conv5_direct_nhwc"):
        ref = out()

        def direct():
            _geops.conv5_direct_nhwc(gop, w_frags, ref, *dims)

        direct()
        same = torch.equal(ref.view(torch.int16), got.view(torch.int16))
        print(f"direct kernel on padded grad        {bench(direct):8.4f} ms"
              f"  bit-equal to pooled LDS: {same}")
        for n_wg in args.n_wg:
            def f():
                _geops.conv5_dgrad_nwg_nhwc(gp, mask, w_frags, gx, *dims,
                                            n_wg)
            f()
            same = torch.equal(gx.view(torch.int16), got.view(torch.int16))
            print(f"pooled LDS dgrad, n_wg {n_wg:5d}        {bench(f):8.4f} ms"
                  f"  bit-equal: {same}")


if __name__ == "__main__":
    main()
