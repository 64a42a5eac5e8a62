#!/usr/bin/env python3
"""The conv1 weight gradient alone at the flagship shape (N=512,
224x224x4 input, pooled gradient 110x110x16 + argmax codes, 768
workgroups): k_conv5_wrw4_nhwc<232> in its pooled form and on the
scattered full-resolution gradient.

    python scripts/wrw_ab.py [--iters 20] [--repeats 7] [--once]

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
N, CI, CO, H = 512, 4, 16, 224
Ho = H - 4
N_WG, T16 = 768, 176


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

    torch.manual_seed(4)
    x = torch.randn(N, CI, H, H, device=DEV, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    gp = torch.randn(N, Ho // 2, Ho // 2, CO, device=DEV,
                     dtype=torch.bfloat16).permute(0, 3, 1, 2)
    mask = torch.randint(0, 4, (gp.numel(),), device=DEV, dtype=torch.uint8)
    go = torch.empty(N, CO, Ho, Ho, dtype=torch.bfloat16, device=DEV,
                     memory_format=torch.channels_last)
    _geops.relu_maxpool2_bwd(gp, mask, go, N, CO, Ho, Ho)
    part = torch.zeros(N_WG, T16, CO, dtype=torch.float32, device=DEV)
    # the 100 tap rows and the bias row; the other slab rows are not
    # part of the result (the 10-tile kernel left dead taps there)
    live = torch.tensor(
        [(kw * 2 + kh // 4) * 16 + (kh % 4) * 4 + ci for kh in range(5)
         for kw in range(5) for ci in range(CI)] + [T16 - 16], device=DEV)

    def pooled():
        _geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, N, H, H, Ho, Ho, CI,
                                     CO, N_WG)

    def full():
        _geops.conv5_wrw_nhwc(x, go, part, N, H, H, Ho, Ho, CI, CO, N_WG)

    for name, f in (("pooled + mask", pooled), ("full-resolution", full)):
        part.zero_()
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        s = part.sum(dim=0)[live].double()
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
