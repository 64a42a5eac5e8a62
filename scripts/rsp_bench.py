#!/usr/bin/env python3
"""Row-sparse push benchmark: rows-only route vs densify-and-push.

    python scripts/rsp_bench.py [--rows 1048576] [--width 128] [--nnz 16384]
                                [--pairs 20] [--json-out FILE]

World size 1 on cuda:0. Each case times `push_row_sparse` + `flush` on a
rows x width fp32 key with `nnz` ids, a quarter of them duplicates, and
compares it with the densify-and-push path that `push_row_sparse` had
before the rows-only route (a zeros [rows][width] tensor, index_add_,
dense push — reproduced verbatim in `densify_push` below, on a second
store with the same optimizer). The two alternate within each pair, and
each call is timed with device events. Also runs the row kernels alone.
Prints one JSON line per case.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geomx_amd import Config, ops  # noqa: E402
from geomx_amd.kvstore import create  # noqa: E402
from geomx_amd.kvstore.optimizer import OptimizerSpec  # noqa: E402

DEV = "cuda:0"


def densify_push(kv, key, row_ids, values, rows, width):
    """The pre-rows-only push_row_sparse body."""
    dense = torch.zeros(rows, width, dtype=torch.float32, device=DEV)
    dense.index_add_(0, row_ids.long(), values.reshape(-1, width).float())
    kv.push(key, dense)


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4),
            "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4)}


def make_ids(rows, nnz, gen):
    uniq = nnz - nnz // 4
    base = torch.randperm(rows, generator=gen)[:uniq]
    dup = base[torch.randint(0, uniq, (nnz - uniq,), generator=gen)]
    ids = torch.cat([base, dup])
    return ids[torch.randperm(nnz, generator=gen)].to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--nnz", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json-out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rsp_bench needs a GPU"
    assert ops.native_available(), ops.native_error()
    rows, width, nnz = args.rows, args.width, args.nnz
    gen = torch.Generator().manual_seed(0)
    ids = make_ids(rows, nnz, gen)
    vals = torch.randn(nnz, width, generator=gen).to(DEV)
    w0 = torch.randn(rows, width, generator=gen).to(DEV)
    out = []

    def emit(rec):
        out.append(rec)
        print(json.dumps(rec), flush=True)

    cases = [
        ("sgd_mom_lazy", dict(name="sgd_mom", lr=0.01, lazy_update=True)),
        ("sgd", dict(name="sgd", lr=0.01)),
        # not lazy: rows-only wire, dense update through the cached buffer
        ("sgd_mom_dense_update", dict(name="sgd_mom", lr=0.01)),
    ]
    for label, spec in cases:
        kv_new = create("dist_sync", cfg=Config.from_env(device=DEV))
        kv_old = create("dist_sync", cfg=Config.from_env(device=DEV))
        kv_new.set_optimizer(OptimizerSpec(**spec))
        kv_old.set_optimizer(OptimizerSpec(
            **{k: v for k, v in spec.items() if k != "lazy_update"}))
        kv_new.init("emb", w0)
        kv_old.init("emb", w0)

        def new():
            kv_new.push_row_sparse("emb", ids, vals)
            kv_new.flush()

        def old():
            densify_push(kv_old, "emb", ids, vals, rows, width)
            kv_old.flush()

        # first step from identical state: the touched rows must agree
        new()
        old()
        torch.cuda.synchronize()
        touched = torch.unique(ids)
        a = kv_new.keys["emb"].stored.reshape(rows, width)[touched]
        b = kv_old.keys["emb"].stored.reshape(rows, width)[touched]
        diff = (a - b).abs().max().item()
        for _ in range(args.warmup):
            new()
            old()
        t_new, t_old = [], []
        for _ in range(args.pairs):
            t_new.append(timed(new))
            t_old.append(timed(old))
        emit({"case": label, "rows": rows, "width": width, "nnz": nnz,
              "unique": int(touched.numel()), "pairs": args.pairs,
              "rows_only": stats(t_new), "densify_push": stats(t_old),
              "speedup_median": round(statistics.median(t_old)
                                      / statistics.median(t_new), 2),
              "faster_in_every_pair": all(n < o for n, o
                                          in zip(t_new, t_old)),
              "first_step_touched_max_abs_diff": diff})
        del kv_new, kv_old
        torch.cuda.empty_cache()

    # the kernels alone (merge includes its torch sort + scan prologue)
    m_ids, merged = ops.rsp_merge(ids, vals)
    w = w0.clone()
    mom = torch.zeros_like(w)
    kern = {
        "rsp_merge(+sort,scan)": lambda: ops.rsp_merge(ids, vals),
        "rsp_scatter": lambda: ops.rsp_scatter(w, m_ids, merged),
        "rsp_sgd_update": lambda: ops.rsp_sgd_update(w, m_ids, merged, 0.01),
        "rsp_sgd_mom_update": lambda: ops.rsp_sgd_mom_update(
            w, m_ids, merged, mom, 0.01),
    }
    for name, fn in kern.items():
        for _ in range(args.warmup):
            fn()
        emit({"kernel": name, **stats([timed(fn)
                                       for _ in range(args.pairs)])})

    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
