#!/usr/bin/env python3
"""Kernel-alone timing of the two fused forward conv + bias + ReLU +
max-pool kernels at the flagship shapes (N=512: conv1 224x224x4 -> 110x110
x16, conv2 110x110x16 -> 53x53x32), default grid and, where the build has
the conv5_pool_nwg_nhwc hook, the grids given with --n-wg.

    python scripts/fwd_ab.py [--n-wg 512 1024 2048] [--reps 5] [--once]

Times are per call, device-event-timed over ITERS calls after warm-up;
each line shows the minimum and the median of --reps such measurements.
A build without the hook (an older commit) prints its default-grid lines
only, so the same script times both sides of an A/B.

Where the build has conv5_pool_x32_nhwc, the conv1 input path is timed
both ways in the same run (the machines of the pool differ by ~5 %): the
3 -> 4 channel pad kernel plus the bf16 forward, against the forward that
reads the fp32 image itself, with and without its padded side output.

Where the build has conv5_pool_u8_nhwc, the uint8 form is timed in that
run too, with and without the side output, next to the standalone
x.float() / 255 pass it replaces in front of the fp32 form."""
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


def bench(f, reps, spread=False):
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
    if spread:
        return min(ts), statistics.median(ts), max(ts)
    return min(ts), statistics.median(ts)


def x32_ab(reps):
    torch.manual_seed(5)
    h, hop = 224, 110
    x = torch.randn(N, 3, h, h, device=DEV) \
        .to(memory_format=torch.channels_last)
    w = torch.randn(16, 3, 5, 5, device=DEV) * 0.05
    b = torch.randn(16, device=DEV) * 0.1
    w_frags = C._w_frags(w, C.build_fwd_index(w.shape).to(DEV))
    outs = [torch.empty(N, hop, hop, 16, device=DEV, dtype=torch.bfloat16)
            for _ in range(2)]
    masks = [torch.empty(outs[0].numel(), device=DEV, dtype=torch.uint8)
             for _ in range(2)]
    xbs = [C._empty_nhwc(N, 4, h, h, DEV) for _ in range(2)]
    dims = (N, h, h, h - 4, h - 4)

    def pad():
        _geops.pad_ch3to4_nhwc(x, xbs[0], N * h * h)

    def fwd():
        _geops.conv5_pool_nhwc(xbs[0], w_frags, b, outs[0], masks[0], *dims,
                               4, 16)

    def parent():
        pad()
        fwd()

    def fused():
        _geops.conv5_pool_x32_nhwc(x, w_frags, b, outs[1], masks[1], xbs[1],
                                   *dims, 16)

    def fused_no_copy():
        _geops.conv5_pool_x32_nhwc(x, w_frags, b, outs[1], masks[1],
                                   torch.Tensor(), *dims, 16)

    runs = [("pad kernel alone", pad), ("bf16 forward alone", fwd),
            ("pad + bf16 forward", parent), ("fp32 forward + copy", fused),
            ("fp32 forward, no copy", fused_no_copy),
            ("pad + bf16 forward", parent), ("fp32 forward + copy", fused)]
    if getattr(_geops, "conv5_pool_u8_nhwc", None) is not None:
        table = C.to_tensor_table(3, [0.485, 0.456, 0.406],
                                  [0.229, 0.224, 0.225]).to(DEV)
        tab = table.to(torch.bfloat16)
        xu = torch.randint(0, 256, (N, h, h, 3), device=DEV,
                           dtype=torch.uint8).permute(0, 3, 1, 2)
        x32 = C.table_gather(table, xu)
        out_u, mask_u = torch.empty_like(outs[0]), torch.empty_like(masks[0])
        xb_u = C._empty_nhwc(N, 4, h, h, DEV)

        def expand():    # the pass a uint8 dataset needs ahead of the fp32 form
            return xu.float() / 255

        def x32_copy():
            _geops.conv5_pool_x32_nhwc(x32, w_frags, b, outs[1], masks[1],
                                       xbs[1], *dims, 16)

        def x32_no_copy():
            _geops.conv5_pool_x32_nhwc(x32, w_frags, b, outs[1], masks[1],
                                       torch.Tensor(), *dims, 16)

        def u8_copy():
            _geops.conv5_pool_u8_nhwc(xu, tab, w_frags, b, out_u, mask_u,
                                      xb_u, *dims, 16)

        def u8_no_copy():
            _geops.conv5_pool_u8_nhwc(xu, tab, w_frags, b, out_u, mask_u,
                                      torch.Tensor(), *dims, 16)

        def expand_x32():
            expand()
            x32_copy()

        x32_copy()
        u8_copy()
        same_u = torch.equal(out_u.view(torch.int16),
                             outs[1].view(torch.int16)) and \
            torch.equal(mask_u, masks[1]) and \
            torch.equal(xb_u.view(torch.int16), xbs[1].view(torch.int16))
        print(f"conv1 uint8 form: out, mask, xb equal to the fp32 form on "
              f"table[c][x]: {same_u}")
        runs += [("uint8 -> fp32 pass alone", expand),
                 ("fp32 forward + copy (img)", x32_copy),
                 ("fp32 forward, no copy (img)", x32_no_copy),
                 ("uint8 forward + copy", u8_copy),
                 ("uint8 forward, no copy", u8_no_copy),
                 ("pass + fp32 forward + copy", expand_x32),
                 ("uint8 forward + copy", u8_copy),
                 ("bf16 forward alone", fwd)]

    parent()
    fused()
    same = all(torch.equal(a.view(torch.int16), c.view(torch.int16))
               for a, c in zip((outs[0], xbs[0].flatten()),
                               (outs[1], xbs[1].flatten()))) and \
        torch.equal(masks[0], masks[1])
    print(f"conv1 input path: fused out, mask, xb equal to pad + forward: "
          f"{same}")
    for name, f in runs:
        lo, med, hi = bench(f, reps, spread=True)
        print(f"conv1 {name:28s} min {lo:7.4f}  median {med:7.4f}  "
              f"max {hi:7.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-wg", type=int, nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true",
                    help="one call per kernel and no timing, for counter "
                         "collection with rocprofv3 --pmc")
    args = ap.parse_args()
    hook = getattr(_geops, "conv5_pool_nwg_nhwc", None)

    if getattr(_geops, "conv5_pool_x32_nhwc", None) is not None \
            and not args.once:
        x32_ab(args.reps)

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
