#!/usr/bin/env python3
"""Kernel-alone timing of the two fused forward conv + bias + ReLU +
max-pool kernels at the flagship shapes (N=512: conv1 224x224x4 -> 110x110
x16, conv2 110x110x16 -> 53x53x32), default grid and, where the build has
the conv5_pool_nwg_nhwc hook, the grids given with --n-wg.

    python scripts/fwd_ab.py [--n-wg 512 1024 2048] [--reps 5] [--once]

Times are per call, device-event-timed over ITERS calls after warm-up;
each line shows the minimum and the median of --reps such measurements.
A build without the hook (an older commit) prints its default-grid lines
only, so the same script times both sides of an A/B."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from geomx_amd import _geops
from geomx_amd.ops import conv as C

DEV = "cuda:0"
N = 512
ITERS = 50
SHAPES = [("conv1 fwd", 3, 16, 224), ("conv2 fwd", 16, 32, 110)]


def bench(f, reps):
    ts = []
    for _ in range(reps):
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
        ts.append(beg.elapsed_time(end) / ITERS)
    return min(ts), statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-wg", type=int, nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true",
                    help="one call per kernel and no timing, for counter "
                         "collection with rocprofv3 --pmc")
    args = ap.parse_args()
    hook = getattr(_geops, "conv5_pool_nwg_nhwc", None)

    for name, cir, co, h in SHAPES:
        torch.manual_seed(5)
        ci = (cir + 3) & ~3
        x = torch.randn(N, ci, h, h, device=DEV, dtype=torch.bfloat16) \
            .to(memory_format=torch.channels_last)
        if ci != cir:
            x[:, cir:] = 0
        w = torch.randn(co, cir, 5, 5, device=DEV) * 0.05
        b = torch.randn(co, device=DEV) * 0.1
        w_frags = C._w_frags(w, C.build_fwd_index(w.shape).to(DEV))
        hop = (h - 4) // 2
        out = torch.empty(N, hop, hop, co, device=DEV, dtype=torch.bfloat16)
        mask = torch.empty(out.numel(), device=DEV, dtype=torch.uint8)
        dims = (N, h, h, h - 4, h - 4, ci, co)

        def default():
            _geops.conv5_pool_nhwc(x, w_frags, b, out, mask, *dims)

        default()
        if args.once:
            torch.cuda.synchronize()
            print(f"{name}: one call, checksum "
                  f"{out.float().sum().item():.1f}")
            continue
        ref = (out.clone(), mask.clone())
        lo, med = bench(default, args.reps)
        print(f"{name}, default grid      min {lo:7.4f}  median {med:7.4f} ms")
        if hook is None:
            continue
        for n_wg in args.n_wg:
            def f():
                hook(x, w_frags, b, out, mask, *dims, n_wg)
            out.zero_()
            f()
            same = torch.equal(out.view(torch.int16),
                               ref[0].view(torch.int16)) and \
                torch.equal(mask, ref[1])
            lo, med = bench(f, args.reps)
            print(f"{name}, n_wg {n_wg:5d}        min {lo:7.4f}  "
                  f"median {med:7.4f} ms  equal to default: {same}")


if __name__ == "__main__":
    main()
