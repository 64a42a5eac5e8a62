#!/usr/bin/env python3
"""Record tests/golden/fwd_pool_parent.npz: pooled output and argmax
codes of the fused forward conv kernels (conv5_pool_nhwc) on the random-
valued cases of tests/fwd_golden_cases.py.

Run once on an MI355X from a checkout (and build) of the commit whose
results are the oracle, and pass that commit's hash:

    python scripts/record_fwd_golden.py --commit <hash> [--out FILE]

Every case runs twice and must agree with itself before anything is
written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fwd_golden_cases as G
from geomx_amd import _geops
from geomx_amd.ops import conv as C

DEV = "cuda:0"


def run_case(cir, co, h, w):
    x, weight, bias = G.random_inputs(cir, co, h, w)
    x = x.to(DEV)
    w_frags = C._w_frags(weight.to(DEV),
                         C.build_fwd_index(weight.shape).to(DEV))
    hop, wop = (h - 4) // 2, (w - 4) // 2
    res = []
    for _ in range(2):
        out = torch.full((G.N, hop, wop, co), float("nan"),
                         dtype=torch.bfloat16, device=DEV)
        mask = torch.full((out.numel(),), 77, dtype=torch.uint8, device=DEV)
        _geops.conv5_pool_nhwc(x, w_frags, bias.to(DEV), out, mask, G.N, h,
                               w, h - 4, w - 4, x.shape[1], co)
        res.append((out.view(torch.int16).cpu(), mask.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and \
        torch.equal(res[0][1], res[1][1]), (cir, co, h, w)
    assert (res[0][1] != 77).all() and (res[0][1] == 255).any() and \
        (res[0][1] < 4).any()
    return res[0][0].numpy(), res[0][1].numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=G.GOLDEN)
    args = ap.parse_args()
    arrays = {"commit": np.array(args.commit)}
    for case in G.CASES:
        out, mask = run_case(*case)
        arrays[G.key(*case) + "_out"] = out
        arrays[G.key(*case) + "_mask"] = mask
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print("wrote %s: %d cases, %d bytes, commit %s"
          % (args.out, len(G.CASES), size, args.commit))
    assert size < 512 * 1024, size


if __name__ == "__main__":
    main()
