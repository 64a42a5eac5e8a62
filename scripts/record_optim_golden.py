#!/usr/bin/env python3
"""Record tests/golden/optim_parent.npz: one step of every server
optimizer kernel (the eight dense rules with both DCASGD momentum forms,
and the four row-sparse rules) on the cases of tests/optim_golden_cases.py.

Run once on an MI355X from a checkout (and build) of the commit whose
bits are the oracle, and pass that commit's hash:

    python scripts/record_optim_golden.py --commit <hash> [--out FILE]

Small cases are stored whole; of the grid-stride wrap cases only a
SHA-256 of each output."""
import argparse
import io
import os
import sys
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import optim_golden_cases as G
from geomx_amd import ops

DEV = "cuda:0"


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: recording the
    same commit again gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a),
                                      allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy",
                                   date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=G.GOLDEN)
    args = ap.parse_args()
    assert ops.native_available(), ops.native_error()
    arrays = {"commit": np.array(args.commit)}
    for name in G.VARIANTS:
        outs = [G.run_dense(ops, name, *G.dense_case(name, n), device=DEV)
                for n in G.DENSE_SIZES]
        big = G.run_dense(ops, name, *G.dense_case(name, G.big_n(name)),
                          device=DEV)
        for k in G.outputs(name):
            arrays["dense/%s/%s" % (name, k)] = np.concatenate(
                [o[k] for o in outs])
            arrays["big/%s/%s" % (name, k)] = np.array(G.digest(big[k]))
    for rule in G.ROW_RULES:
        for width, offset in G.ROW_CASES:
            out = G.run_row(ops, rule, *G.row_case(rule, width), offset,
                            device=DEV)
            for k in G.outputs(rule):
                arrays["row/%s/%s/%s" % (rule, G.row_tag(width, offset),
                                         k)] = out[k]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    save_npz(args.out, arrays)
    size = os.path.getsize(args.out)
    print("wrote %s: %d entries, %d bytes, commit %s"
          % (args.out, len(arrays) - 1, size, args.commit))
    assert size < 332 * 1024, size


if __name__ == "__main__":
    main()
