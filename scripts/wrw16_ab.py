#!/usr/bin/env python3
"""The conv2 weight gradient alone at the flagship shape (N=512,
110x110x16 input, pooled gradient 53x53x32 + argmax codes, 768
workgroups): k_conv5_wrw16_nhwc<2,136> in its pooled form and on the
scattered full-resolution gradient.

    python scripts/wrw16_ab.py [--iters 20] [--repeats 7] [--once]

Inputs are generated once. Times are per call, hipEvent-timed over
ITERS calls after warm-up; the median and the spread of REPEATS such
measurements are printed. --once runs each form a few times without
timing (for counter collection with rocprofv3 --pmc). The checksum
lines let two builds be compared on the same inputs."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from geomx_amd import _geops

DEV = "cuda:0"
N, CI, CO, H = 512, 16, 32, 110
Ho = H - 4
N_WG, T16 = 768, 416


def timed(f, iters):
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    beg.record()
    for _ in range(iters):
        f()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()

    torch.manual_seed(16)
    x = torch.randn(N, CI, H, H, device=DEV, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    gp = torch.randn(N, Ho // 2, Ho // 2, CO, device=DEV,
                     dtype=torch.bfloat16).permute(0, 3, 1, 2)
    mask = torch.randint(0, 4, (gp.numel(),), device=DEV, dtype=torch.uint8)
    go = torch.empty(N, CO, Ho, Ho, dtype=torch.bfloat16, device=DEV,
                     memory_format=torch.channels_last)
    _geops.relu_maxpool2_bwd(gp, mask, go, N, CO, Ho, Ho)
    part = torch.empty(N_WG, T16, CO, dtype=torch.float32, device=DEV)

    def pooled():
        _geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, N, H, H, Ho, Ho, CI,
                                     CO, N_WG)

    def full():
        _geops.conv5_wrw_nhwc(x, go, part, N, H, H, Ho, Ho, CI, CO, N_WG)

    for name, f in (("pooled + mask", pooled), ("full-resolution", full)):
        part.fill_(float("nan"))   # every slab row must be written
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        s = part.sum(dim=0).double()
        print(f"{name:16s} checksum {s.sum().item():.9e} "
              f"abs {s.abs().sum().item():.9e}")
        if args.once:
            continue
        ts = [timed(f, args.iters) for _ in range(args.repeats)]
        print(f"{name:16s} median {statistics.median(ts):.4f} ms  "
              f"min {min(ts):.4f}  max {max(ts):.4f}  "
              f"({args.repeats} x {args.iters} calls)")


if __name__ == "__main__":
    main()
