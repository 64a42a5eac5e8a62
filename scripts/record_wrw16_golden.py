#!/usr/bin/env python3
"""Record tests/golden/wrw16_parent.npz: the per-workgroup slabs of the
conv2-class weight-gradient kernel (k_conv5_wrw16_nhwc) on the
GOLDEN_CASES of tests/wrw16_golden_cases.py.

Run once on an MI355X from a checkout (and build) of the commit whose
sums are the oracle, and pass that commit's hash:

    python scripts/record_wrw16_golden.py --commit <hash> [--out FILE]

Both forms of every case (full-resolution gout; pooled gradient + argmax
codes) must agree bit for bit before anything is written; one array per
case is stored (slab rows 0..400: the taps and the bias row)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import wrw16_golden_cases as G
from geomx_amd import _geops

DEV = "cuda:0"


def run_case(h, w, n_wg, co):
    x, go, gp, mask = (t.to(DEV) for t in G.build_inputs(h, w, co, False))
    ho, wo = h - 4, w - 4
    part = torch.zeros(n_wg, G.T16, co, dtype=torch.float32, device=DEV)
    _geops.conv5_wrw_nhwc(x, go, part, G.N, h, w, ho, wo, G.CI, co, n_wg)
    part2 = torch.zeros_like(part)
    _geops.conv5_wrw_unpool_nhwc(x, gp, mask, part2, G.N, h, w, ho, wo,
                                 G.CI, co, n_wg)
    assert torch.equal(part, part2), (h, w, n_wg, co)
    tail = part[:, G.BIAS_ROW + 1:]
    assert torch.equal(tail, torch.zeros_like(tail))
    assert part.abs().sum().item() > 0
    return part[:, :G.BIAS_ROW + 1].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=G.GOLDEN)
    args = ap.parse_args()
    arrays = {"commit": np.array(args.commit)}
    for case in G.GOLDEN_CASES:
        arrays[G.key(*case)] = run_case(*case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print("wrote %s: %d cases, %d bytes, commit %s"
          % (args.out, len(arrays) - 1, size, args.commit))
    assert size < 512 * 1024, size


if __name__ == "__main__":
    main()
