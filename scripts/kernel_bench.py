#!/usr/bin/env python3
"""Microbenchmark of the geops HIP kernels: effective HBM bandwidth vs
the ~6.3 TB/s MI355X ceiling. Run on a GPU box:

    python scripts/kernel_bench.py [--n 67108864] [--iters 50]

Prints one line per kernel: name, bytes moved per call, ms, GB/s.
"""

import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geomx_amd import ops  # noqa: E402
from geomx_amd.ops import reference as ref  # noqa: E402


def timeit(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def window_pair(fn_a, fn_b, iters, reps=7):
    """Seconds per call of two alternatives in each of `reps` alternating
    windows of `iters` calls, timed with device events, after a warm-up of
    both."""
    def window(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters
    for fn in (fn_a, fn_b):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fn_a))
        tb.append(window(fn_b))
    return ta, tb


def median_pair(fn_a, fn_b, iters, reps=7):
    """Median seconds per call of the two alternatives of window_pair."""
    ta, tb = window_pair(fn_a, fn_b, iters, reps)
    return sorted(ta)[reps // 2], sorted(tb)[reps // 2]


def bsc_boundary_rows(n, iters, report, results, small_n=200_000):
    """Sampled Bi-Sparse boundary, ratio 0.01, at n and at one small bucket:
    the ATen chain ops.bsc_boundary replaced (gathers, multiply, adds, abs,
    topk, slice, clone; kept here as the yardstick) against the op, in 5
    alternating windows. Bytes are the 16 S of the three 4 B gathers and the
    positions. The spread is (max - min) / median over the windows."""
    import geomx_amd.ops as _ops
    from geomx_amd.ops import reference as ref
    dev = "cuda:0"
    ratio, mu = 0.01, ref.BSC_MOMENTUM

    def chain(g, u, v):
        nn = v.numel()
        sample_size = min(ref.bsc_sample_size(nn, ratio), nn)
        top_k = max(1, int(sample_size * ratio))
        si = _ops._bsc_sample_idx(nn, sample_size, 42, v.device)
        sample = (v[si] + (u[si] * mu + g[si])).abs()
        k = min(top_k, sample.numel())
        return torch.topk(sample, k).values[k - 1:k].clone()

    for nn in (n, small_n):
        g, u, v = (torch.randn(nn, device=dev) for _ in range(3))
        assert torch.equal(chain(g, u, v),
                           _ops.bsc_boundary(v, ratio, g=g, u=u, momentum=mu))
        ta, tb = window_pair(
            lambda: chain(g, u, v),
            lambda: _ops.bsc_boundary(v, ratio, g=g, u=u, momentum=mu),
            iters, reps=5)
        S = min(ref.bsc_sample_size(nn, ratio), nn)
        for name, t in (("bsc_boundary chain", ta), ("bsc_boundary", tb)):
            t = sorted(t)
            report("%s n=%d" % (name, nn), 16 * S, t[2])
            results[-1]["spread"] = round((t[-1] - t[0]) / t[2], 3)
            print("    spread %.1f %%" % (100 * results[-1]["spread"]))
        del g, u, v


def dgt_encode_rows(n, iters, report, results):
    """Fused DGT mode-3 encode against the op chain it replaced in
    DGTState.compress (ref.dgt_encode on the GPU), chunk 1024, k = 0.5 and
    0.25. Bytes are those that must move: x and the residual in, the
    residual out, 4k bytes of exact rows and (1 - k) / 2 of codes per
    element. The spread is (max - min) / median over the 7 windows."""
    dev = "cuda:0"
    chunk = 1024
    iters = max(5, iters // 5)
    x = torch.randn(n, device=dev)
    contrib = ops.dgt_contribution(x, chunk)
    for k in (0.5, 0.25):
        n_keep = max(1, math.ceil(k * contrib.numel()))
        keep_idx = torch.topk(contrib, n_keep).indices.sort().values
        res_f = 0.05 * torch.randn(n, device=dev)
        res_c = res_f.clone()
        tf, tc = window_pair(
            lambda: ops.dgt_encode(x, res_f, contrib, keep_idx, chunk),
            lambda: ref.dgt_encode(x, res_c, contrib, keep_idx, chunk), iters)
        mf, mc = sorted(tf)[len(tf) // 2], sorted(tc)[len(tc) // 2]
        report("dgt_encode(k=%g)" % k,
               int(8 * n + 4 * n + 4 * k * n + (1 - k) * n / 2), mf)
        results[-1].update(chain_ms=round(mc * 1e3, 4),
                           speedup=round(mc / mf, 2),
                           spread=round((max(tf) - min(tf)) / mf, 3),
                           chain_spread=round((max(tc) - min(tc)) / mc, 3))
        print("%24s chain %8.3f ms, fused is %.2fx; spread between windows "
              "%.1f%% fused, %.1f%% chain"
              % ("", mc * 1e3, mc / mf, 100 * results[-1]["spread"],
                 100 * results[-1]["chain_spread"]))
        del res_f, res_c
        torch.cuda.empty_cache()


def fp8_wire_rows(n, iters, report, results, chunk=256, P=4):
    """FP8 wire tier. k_fp8_encode against its byte model (x and the
    residual in, the residual and one code byte per element out: 13 B per
    element, plus a scale byte per chunk), and k_wire_sum_fp8 at P parties
    beside k_wire_sum_f16 at the same n and P, in alternating windows. The
    spread is (max - min) / median over the 7 windows."""
    dev = "cuda:0"
    iters = max(5, iters // 5)
    grads = [torch.randn(n, device=dev) for _ in range(P)]
    res = 0.01 * torch.randn(n, device=dev)
    nbytes = ops.fp8_wire_bytes(n, chunk)
    dst = torch.empty(n, device=dev)
    pl = [ops.fp8_encode(g, None, chunk) for g in grads]
    hl = [g.half() for g in grads]
    del grads[1:]

    def encode():
        ops.fp8_encode(grads[0], res, chunk)
    te = sum(window_pair(encode, encode, iters), [])   # 14 windows of it
    me = sorted(te)[len(te) // 2]
    report("fp8_encode(c=%d)" % chunk, 12 * n + nbytes, me)
    results[-1].update(spread=round((max(te) - min(te)) / me, 3))
    print("%24s spread between windows %.1f%%"
          % ("", 100 * results[-1]["spread"]))
    t8, t16 = window_pair(
        lambda: ops.wire_sum_fp8(pl, n, chunk, out=dst),
        lambda: ops.wire_sum_fp16(hl, out=dst), iters)
    m8, m16 = sorted(t8)[len(t8) // 2], sorted(t16)[len(t16) // 2]
    report("wire_sum_fp8 P=%d" % P, P * nbytes + 4 * n, m8)
    results[-1].update(spread=round((max(t8) - min(t8)) / m8, 3))
    report("wire_sum_fp16 P=%d" % P, P * 2 * n + 4 * n, m16)
    results[-1].update(spread=round((max(t16) - min(t16)) / m16, 3))
    print("%24s fp8 / fp16 time %.3f; spread between windows %.1f%% fp8, "
          "%.1f%% fp16" % ("", m8 / m16, 100 * results[-2]["spread"],
                           100 * results[-1]["spread"]))


def wire_reduce_rows(n, iters, report, results):
    """Fused wire reduce against the chain of single-party ops it replaced
    at the receive sites, P = 2 and 8. Bytes are those that must move:
    every party's payload in, 4n out."""
    from geomx_amd.kvstore.dgt import DGTState
    dev = "cuda:0"
    dst = torch.empty(n, device=dev)
    iters = max(5, iters // 5)

    def row(name, P, nbytes, fused, chain):
        tf, tc = median_pair(fused, chain, iters)
        report("%s P=%d" % (name, P), nbytes, tf)
        results[-1].update(chain_ms=round(tc * 1e3, 4),
                           speedup=round(tc / tf, 2))
        print("%24s chain %8.3f ms, fused is %.2fx" % ("", tc * 1e3, tc / tf))

    for P in (2, 8):
        grads = [torch.randn(n, device=dev) for _ in range(P)]

        # 2bit: trainer / kvstore leader chain
        thr = 0.5
        pl = [ops.quantize_2bit(g, torch.zeros_like(g), thr) for g in grads]

        def chain_2bit():
            acc = torch.zeros(n, device=dev)
            tmp = torch.empty(n, device=dev)
            for w in pl:
                ops.dequantize_2bit(w, n, thr, out=tmp)
                acc += tmp
            dst.copy_(acc)
        row("wire_sum_2bit", P, P * pl[0].numel() * 4 + n * 4,
            lambda: ops.wire_sum_2bit(pl, n, thr, out=dst), chain_2bit)

        # fp16: kvstore WAN chain (P casts, P - 1 out-of-place adds)
        hl = [g.half() for g in grads]

        def chain_f16():
            contribs = [x.float() for x in hl]
            agg = contribs[0]
            for c in contribs[1:]:
                agg = agg + c
            return agg
        row("wire_sum_fp16", P, P * n * 2 + n * 4,
            lambda: ops.wire_sum_fp16(hl, out=dst), chain_f16)
        del hl

        # DGT mode 3, k = 0.5, chunk 1024: trainer chain
        sts = [DGTState(n, dev, chunk_elems=1024, k=0.5, mode=3)
               for _ in range(P)]
        dl = [st.compress(g) for st, g in zip(sts, grads)]
        for st in sts:
            st.residual = None  # not needed to decompress

        def chain_dgt():
            acc = torch.zeros(n, device=dev)
            for st, d in zip(sts, dl):
                acc += st.decompress(*d)
            dst.copy_(acc)
        row("wire_sum_dgt(k=.5)", P,
            sum(t.numel() * t.element_size() for d in dl for t in d) + n * 4,
            lambda: ops.wire_sum_dgt(dl, n, 1024, out=dst), chain_dgt)
        del grads, pl, dl, sts
        torch.cuda.empty_cache()


def wire_sparse_rows(n, iters, report, results):
    """Fused Bi-Sparse wire reduce (ops.wire_sum_bsc) against the two chains
    it replaced, ratio 0.01, P = 2 and 8, plain lists and the bsc_dgt coded
    form (chunk 1024, k = 0.5): the kvstore chain (P dense decodes, P - 1
    out-of-place adds) and the trainer chain (zeros, P accumulating unpacks,
    copy_). Each chain is timed against the fused op in alternating
    windows of its own. Bytes are those that must move: every party's
    payload in, 4n out. The spread is (max - min) / median over the 7
    windows."""
    from geomx_amd.kvstore.dgt import DGTState
    dev = "cuda:0"
    chunk = 1024
    dst = torch.empty(n, device=dev)
    iters = max(5, iters // 5)

    def med(ts):
        return sorted(ts)[len(ts) // 2]

    for P in (2, 8):
        plain, coded, sts = [], [], []
        u, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        for p in range(P):
            g = torch.randn(n, device=dev, generator=torch.Generator(
                device=dev).manual_seed(40 + p))
            vals, idx = ops.bsc_compress(g, u.zero_(), v.zero_(), 0.01)
            plain.append((vals, idx))
            st = DGTState(vals.numel(), dev, chunk_elems=chunk, k=0.5, mode=3)
            coded.append(st.compress(vals.masked_fill(idx < 0, 0.0)) + (idx,))
            sts.append(st)
        del g, u, v

        for name, pls, ce in (("wire_sum_bsc", plain, None),
                              ("wire_sum_bsc(dgt k=.5)", coded, chunk)):
            def values(p):
                if ce is None:
                    return pls[p][0]
                return sts[p].decompress(*pls[p][:4]).contiguous()

            def chain_kvstore():
                dense = [ops.bsc_decompress(values(p), pls[p][-1], n)
                         for p in range(P)]
                agg = dense[0]
                for c in dense[1:]:
                    agg = agg + c
                return agg

            def chain_trainer():
                acc = torch.zeros(n, device=dev)
                for p in range(P):
                    ops.bsc_decompress(values(p), pls[p][-1], n, out=acc,
                                       accumulate=True)
                dst.copy_(acc)

            nbytes = 4 * n + sum(t.numel() * t.element_size()
                                 for pl in pls for t in pl)
            for site, fused, chain in (
                    ("kvstore", lambda: ops.wire_sum_bsc(pls, n,
                                                         chunk_elems=ce),
                     chain_kvstore),
                    ("trainer", lambda: ops.wire_sum_bsc(pls, n, out=dst,
                                                         chunk_elems=ce),
                     chain_trainer)):
                tf, tc = window_pair(fused, chain, iters)
                mf, mc = med(tf), med(tc)
                report("%s P=%d %s" % (name, P, site), nbytes, mf)
                results[-1].update(
                    chain_ms=round(mc * 1e3, 4), speedup=round(mc / mf, 2),
                    spread=round((max(tf) - min(tf)) / mf, 3),
                    chain_spread=round((max(tc) - min(tc)) / mc, 3))
                print("%24s chain %8.3f ms, fused is %.2fx; spread between "
                      "windows %.1f%% fused, %.1f%% chain"
                      % ("", mc * 1e3, mc / mf, 100 * results[-1]["spread"],
                         100 * results[-1]["chain_spread"]))
        del plain, coded, sts
        torch.cuda.empty_cache()


def lars_rows(n, iters, report, results):
    """LBSGD 'lars' step (k_lars_sumsq + k_lars_update) at n elements, with
    one segment and with the flagship bucket's segments (the geomx_cnn
    parameters on 64-element boundaries, repeated to fill n), against
    k_sgd_mom_update and the PyTorch expression of the rule (two
    vector_norm and one update per segment) on the same buffers, in 5
    alternating windows. Necessary bytes: 8n for the sums, 20n for the
    update, as k_sgd_mom_update."""
    from geomx_amd.models import create_model
    dev = "cuda:0"
    iters = max(5, iters // 5)
    w = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev)
    m = torch.zeros(n, device=dev)
    lens = [(p.numel() + 63) // 64 * 64
            for p in create_model("geomx_cnn", image_size=224).parameters()]
    offs = [0]
    while offs[-1] < n:
        offs.append(min(n, offs[-1] + lens[(len(offs) - 1) % len(lens)]))
    layouts = {"1 seg": [0, n], "%d segs" % (len(offs) - 1): offs}

    def torch_rule(bounds):
        for a, b in zip(bounds[:-1], bounds[1:]):
            w2 = torch.linalg.vector_norm(w[a:b]) ** 2
            g2 = torch.linalg.vector_norm(g[a:b]) ** 2
            lr = 0.01 * torch.sqrt(w2 / (g2 + 1e-18)).clamp(0.01, 100.0)
            m[a:b].mul_(0.9).sub_(lr * g[a:b])
            w[a:b].add_(m[a:b])

    def sgd_mom():
        ops.sgd_mom_update(w, g, m, 0.01, 0.9)

    for name, bounds in layouts.items():
        seg = torch.tensor(bounds, dtype=torch.int64, device=dev)
        ratio = ops.lars_ratio(w, g, seg)
        tabs = ops._lars_tables(seg, n, w.device)
        ta, tb = window_pair(lambda: ops.lars_ratio(w, g, seg, out=ratio),
                             lambda: ops._geops.lars_update(
                                 w, g, m, tabs[0], tabs[1], ratio, tabs[2],
                                 0.01, 1.0, 0.9, 0.0, 1.0, tabs[3], 0),
                             iters, reps=5)
        tl, ts = window_pair(
            lambda: ops.lbsgd_update(w, g, m, seg, 0.01, 0.9), sgd_mom, iters,
            reps=5)
        # the eager rule is slow with many segments: one window of 2 calls
        tt, _ = window_pair(lambda: torch_rule(bounds), sgd_mom, 2, reps=1)
        for row, nbytes, t in (("k_lars_sumsq", 8 * n, ta),
                               ("k_lars_update", 20 * n, tb),
                               ("lbsgd_update", 28 * n, tl),
                               ("sgd_mom_update", 20 * n, ts),
                               ("torch lars rule", 28 * n, tt)):
            t = sorted(t)
            med = t[len(t) // 2]
            report("%s (%s)" % (row, name), nbytes, med)
            results[-1]["windows_ms"] = [round(x * 1e3, 4) for x in t]
        ml, ms = sorted(tl)[2], sorted(ts)[2]
        results[-1]["lbsgd_over_sgd_mom"] = round(ml / ms, 3)
        print("%24s lbsgd / sgd_mom = %.3f" % ("", ml / ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)  # 64M fp32 = 256 MB
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json-out", type=str, default=None)
    ap.add_argument("--only-wire", action="store_true",
                    help="only the wire reduce rows, dense and sparse")
    ap.add_argument("--only-bsc-boundary", action="store_true",
                    help="only the Bi-Sparse boundary rows, chain and kernel")
    ap.add_argument("--only-dgt", action="store_true",
                    help="only the fused DGT encode rows")
    ap.add_argument("--only-fp8", action="store_true",
                    help="only the FP8 wire rows, beside the fp16 sum")
    ap.add_argument("--only-lars", action="store_true",
                    help="only the LBSGD 'lars' rows")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    assert ops.native_available(), ops.native_error()
    from geomx_amd.ops import _geops as geops

    n = args.n
    dev = "cuda:0"
    g = torch.randn(n, device=dev)
    results = []

    def report(name, nbytes, sec):
        gbs = nbytes / sec / 1e9
        line = {"kernel": name, "bytes": nbytes, "ms": round(sec * 1e3, 4),
                "GBps": round(gbs, 1)}
        results.append(line)
        print(f"{name:24s} {nbytes/1e6:10.1f} MB {sec*1e3:8.3f} ms "
              f"{gbs:8.1f} GB/s")

    def dump():
        if args.json_out:
            with open(args.json_out, "w") as f:
                json.dump({"n": n, "iters": args.iters, "results": results},
                          f, indent=1)

    if args.only_wire:
        del g
        wire_reduce_rows(n, args.iters, report, results)
        wire_sparse_rows(n, args.iters, report, results)
        dump()
        return
    if args.only_bsc_boundary:
        del g
        bsc_boundary_rows(n, args.iters, report, results)
        dump()
        return
    if args.only_dgt:
        del g
        dgt_encode_rows(n, args.iters, report, results)
        dump()
        return
    if args.only_fp8:
        del g
        fp8_wire_rows(n, args.iters, report, results)
        dump()
        return
    if args.only_lars:
        del g
        lars_rows(n, args.iters, report, results)
        dump()
        return

    # --- 2bit quantize: read g + r, write r + n/16 words
    r = torch.zeros(n, device=dev)
    packed = torch.empty((n + 15) // 16, dtype=torch.int32, device=dev)
    sec = timeit(lambda: geops.quantize_2bit(g, r, packed, 0.5), args.iters)
    report("quantize_2bit", n * 4 * 3 + n // 4, sec)

    out = torch.empty(n, device=dev)
    sec = timeit(lambda: geops.dequantize_2bit(packed, out, 0.5), args.iters)
    report("dequantize_2bit", n * 4 + n // 4, sec)

    # --- bsc momentum: read g,u,v write u,v
    u = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    sec = timeit(lambda: geops.bsc_momentum(g, u, v, 0.9), args.iters)
    report("bsc_momentum", n * 4 * 5, sec)

    # --- bsc pack (1% capacity): read v (+u,v writes at 1%)
    k = int(n * 0.01)
    vals = torch.empty(k, device=dev)
    idx = torch.empty(k, dtype=torch.int32, device=dev)
    v.copy_(g)
    boundary = 2.3  # ~1% of a standard normal
    sec = timeit(lambda: geops.bsc_pack(v, u, vals, idx, boundary, -65530.0),
                 args.iters)
    report("bsc_pack(1%)", n * 4 * 2, sec)  # count pass + pack pass reads

    sec = timeit(lambda: geops.bsc_unpack(vals, idx, out, False), args.iters)
    report("bsc_unpack(1%)", n * 4 + k * 8, sec)

    # --- fused single-pass compress (momentum+count+pack), the
    # production bsc path: read g,u,v + write u,v in ONE sweep
    bt = torch.full((1,), 2.3, device=dev)
    sec = timeit(lambda: geops.bsc_compress_fused(g, u, v, vals, idx, bt,
                                                  0.9, -65530.0),
                 args.iters)
    report("bsc_fused(1%)", n * 4 * 5, sec)

    import geomx_amd.ops as _ops
    sec = timeit(lambda: _ops.bsc_compress(g, u, v, 0.01), args.iters)
    report("bsc_compress e2e", n * 4 * 5, sec)

    bsc_boundary_rows(n, args.iters, report, results)

    sec = timeit(lambda: geops.bsc_pull_pack(out, vals, idx, -65530.0),
                 args.iters)
    report("bsc_pull_pack", n * 4 * 2, sec)

    # --- dgt contribution
    nchunks = (n + 1023) // 1024
    contrib = torch.empty(nchunks, device=dev)
    sec = timeit(lambda: geops.dgt_contribution(g, contrib, 1024), args.iters)
    report("dgt_contribution", n * 4, sec)

    # --- 4bit quantize (minmax pass + pack pass)
    p4 = torch.empty((n + 1) // 2, dtype=torch.uint8, device=dev)
    mm = torch.empty(nchunks * 2, device=dev).reshape(nchunks, 2)
    empty = torch.Tensor()
    sec = timeit(lambda: geops.quantize_4bit(g, empty, p4, mm, 1024),
                 args.iters)
    report("quantize_4bit", n * 4 * 2 + n // 2, sec)

    sec = timeit(lambda: geops.dequantize_4bit(p4, mm, out, 1024), args.iters)
    report("dequantize_4bit", n // 2 + n * 4, sec)

    # --- optimizers
    w = torch.randn(n, device=dev)
    sec = timeit(lambda: geops.sgd_update(w, g, 0.01, 0.0, 1.0), args.iters)
    report("sgd_update", n * 4 * 3, sec)

    m = torch.zeros(n, device=dev)
    sec = timeit(lambda: geops.sgd_mom_update(w, g, m, 0.01, 0.9, 0.0, 1.0),
                 args.iters)
    report("sgd_mom_update", n * 4 * 5, sec)

    vv = torch.zeros(n, device=dev)
    sec = timeit(lambda: geops.adam_update(w, g, m, vv, 10, 0.01, 0.9, 0.999,
                                           1e-8, 0.0, 1.0), args.iters)
    report("adam_update", n * 4 * 7, sec)

    pw = w.clone()
    sec = timeit(lambda: geops.dcasgd_update(w, g, pw, empty, 0.01, 0.04, 0.0,
                                             0.0, 1.0), args.iters)
    report("dcasgd_update", n * 4 * 5, sec)

    sec = timeit(lambda: geops.dcasgd_update(w, g, pw, m, 0.01, 0.04, 0.9,
                                             0.0, 1.0), args.iters)
    report("dcasgd_update(mom)", n * 4 * 7, sec)

    sec = timeit(lambda: geops.rmsprop_update(w, g, vv, 0.01, 0.9, 1e-8, 0.0,
                                              1.0), args.iters)
    report("rmsprop_update", n * 4 * 5, sec)

    sec = timeit(lambda: geops.adagrad_update(w, g, vv, 0.01, 1e-7, 0.0, 1.0),
                 args.iters)
    report("adagrad_update", n * 4 * 5, sec)

    sec = timeit(lambda: geops.signsgd_update(w, g, 0.01, 0.0, 1.0),
                 args.iters)
    report("signsgd_update", n * 4 * 3, sec)

    sec = timeit(lambda: geops.signum_update(w, g, m, 0.01, 0.9, 0.0, 1.0),
                 args.iters)
    report("signum_update", n * 4 * 5, sec)

    del w, m, vv, pw, u, v, g, r, out, p4
    torch.cuda.empty_cache()
    wire_reduce_rows(n, args.iters, report, results)
    wire_sparse_rows(n, args.iters, report, results)
    dgt_encode_rows(n, args.iters, report, results)
    fp8_wire_rows(n, args.iters, report, results)
    lars_rows(n, args.iters, report, results)
    dump()


if __name__ == "__main__":
    main()
