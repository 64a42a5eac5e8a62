#!/usr/bin/env python3
"""Record tests/golden/wrw_parent.npz: the per-workgroup slabs of the
conv1 weight-gradient kernel (k_conv5_wrw4_nhwc) on the cases of
tests/wrw_golden_cases.py, reduced to their live entries.

Run once on an MI355X from a checkout (and build) of the commit whose
sums are the oracle, and pass that commit's hash:

    python scripts/record_wrw_golden.py --commit <hash> [--out FILE]

Both forms of every even-height case (full-resolution gout; pooled
gradient + argmax codes) must agree bit for bit before anything is
written; one array per case is stored."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import wrw_golden_cases as G
from geomx_amd import _geops

DEV = "cuda:0"


def run_case(h, w, n_wg):
    x, go, gp, mask = (t if t is None else t.to(DEV)
                       for t in G.build_inputs(h, w))
    ho, wo = h - 4, w - 4
    part = torch.zeros(n_wg, G.T16, G.CO, dtype=torch.float32, device=DEV)
    _geops.conv5_wrw_nhwc(x, go, part, G.N, h, w, ho, wo, G.CI, G.CO, n_wg)
    red = G.reduce_slabs(part)
    if gp is not None:
        part2 = torch.zeros_like(part)
        _geops.conv5_wrw_unpool_nhwc(x, gp, mask, part2, G.N, h, w, ho, wo,
                                     G.CI, G.CO, n_wg)
        assert torch.equal(G.reduce_slabs(part2), red), (h, w, n_wg)
    assert red.abs().sum().item() > 0
    return red.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=G.GOLDEN)
    args = ap.parse_args()
    arrays = {"commit": np.array(args.commit)}
    for h, w, n_wg in G.CASES + [G.ODD_CASE]:
        arrays[G.key(h, w, n_wg)] = run_case(h, w, n_wg)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print("wrote %s: %d cases, %d bytes, commit %s"
          % (args.out, len(arrays) - 1, size, args.commit))
    assert size < 256 * 1024, size


if __name__ == "__main__":
    main()
