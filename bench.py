#!/usr/bin/env python3
"""Flagship benchmark: CNN training samples/sec on 1..8 MI355X GPUs.

Measures the BASELINE.json headline metric — samples/sec (whole node)
for the GeoMX example CNN (examples/cnn.py:56-63 architecture) on
synthetic 3x224x224 data, random-init weights, bf16 autocast compute.

Modes:
  --mode flat  (default) : bucketed all_reduce data parallelism — the
                           baseline the HiPS speedup is measured against
  --mode hips            : two-tier HiPS (party tier + leader/WAN tier),
                           with --parties, --compress, --wan-gbps

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W           (single GPU)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times exactly --steps steps and prints
one JSON result line (ms_per_step = wall time of one timed step).
  --dump-outputs DIR : also write what the last timed step computed
                       (loss, logits, updated parameters) as float32
                       DIR/<name>.npy; same arguments, same inputs
  --full             : anything measured beyond the headline figure
                       runs only under this flag
"""

import argparse
import json
import os
import sys
import time

# MIOpen find: NORMAL find (1). The fast mode (3) is cheaper at warmup
# but non-robust: in r02 it picked a 2.5x slower conv1 wrw igemm
# (1.61 vs 0.64 ms/step). Override via env for quick smokes.
os.environ.setdefault("MIOPEN_FIND_MODE", "1")

import torch
import torch.distributed as distmod

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geomx_amd import Config  # noqa: E402
from geomx_amd.kvstore.optimizer import OptimizerSpec  # noqa: E402
from geomx_amd.models import create_model  # noqa: E402
from geomx_amd.parallel import GeoTrainer  # noqa: E402
from geomx_amd.topology import init_topology  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=512,
                   help="per-GPU batch (weak scaling)")
    p.add_argument("--model", type=str, default="geomx_cnn")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--num-classes", type=int, default=10)
    p.add_argument("--mode", type=str, default="flat", choices=["flat", "hips"])
    p.add_argument("--parties", type=int, default=0,
                   help="HiPS party count (default: world_size//2, min 2)")
    p.add_argument("--compress", type=str, default=None,
                   choices=[None, "bsc", "fp16", "mpq", "2bit", "dgt", "bsc_dgt"])
    p.add_argument("--bsc-ratio", type=float, default=0.01)
    p.add_argument("--wan-gbps", type=float, default=0.0)
    p.add_argument("--party-wan-gbps", type=str, default=None,
                   help="comma-separated per-party uplink Gbit/s "
                        "(heterogeneous WAN; overrides --wan-gbps)")
    p.add_argument("--bucket-mb", type=int, default=25)
    p.add_argument("--optimizer", type=str, default="sgd_mom")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--comm-dtype", type=str, default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--json-out", type=str, default=None)
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step computed (loss, logits, updated parameters) "
                        "as DIR/<name>.npy in float32")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure; a plain run times the steps and nothing "
                        "else (there are no extra measurements yet: this "
                        "is where they go)")
    p.add_argument("--backend", type=str, default="auto",
                   choices=["auto", "nccl", "gloo"])
    p.add_argument("--sync-mode", type=str, default="dist_sync",
                   choices=["dist_sync", "dist_async"],
                   help="dist_async = pipelined one-step-stale WAN tier")
    p.add_argument("--hip-graph", action="store_true",
                   help="capture the whole train step in a hipGraph "
                        "(measured ~1-2%% SLOWER than eager async launch "
                        "on this step at bs512 — r02 A/B — so off by "
                        "default; the flag remains for shorter steps)")
    p.add_argument("--no-channels-last", action="store_true",
                   help="disable NHWC layout (NHWC avoids MIOpen's "
                        "batched_transpose + slow NCHW pooling kernels)")
    return p.parse_args()


# --dump-outputs budget: arrays above the per-array cap are written as a
# fixed, seeded sample of their elements; everything together stays
# under 48 MB of float32
DUMP_ARRAY_ELEMS = 1 << 20
DUMP_TOTAL_ELEMS = 12 << 20


def dump_outputs(path, tensors):
    """Write each tensor as path/<name>.npy (float32). With the same
    arguments the sample indices are the same from run to run."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(1234)
    left = DUMP_TOTAL_ELEMS
    for name, t in tensors.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        cap = min(DUMP_ARRAY_ELEMS, left)
        if a.size > cap:
            idx = np.sort(rng.integers(0, a.size, size=cap))
            a = a.reshape(-1)[idx]
        left -= a.size
        np.save(os.path.join(path, name + ".npy"),
                np.ascontiguousarray(a, dtype=np.float32))


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))

    use_cuda = torch.cuda.is_available()
    device_str = "cuda" if use_cuda else "cpu"
    backend = ("nccl" if use_cuda else "gloo") if args.backend == "auto" \
        else args.backend

    parties = args.parties or (max(2, world // 4) if world > 1 else 1)
    if world % max(1, parties):
        parties = 1
    # flat mode: topology has ONE party (no hierarchy) but the WAN
    # accounting still uses `parties` so flat-vs-hips is charged the
    # same emulated inter-DC link
    topo_parties = parties if args.mode == "hips" and world > 1 else 1

    pw = [float(x) for x in args.party_wan_gbps.split(",")] \
        if args.party_wan_gbps else None
    cfg = Config.from_env(
        num_parties=parties, backend=backend, mode=args.sync_mode,
        compression=args.compress, bsc_ratio=args.bsc_ratio,
        wan_gbps=args.wan_gbps, party_wan_gbps=pw,
        bucket_mb=args.bucket_mb, comm_dtype=args.comm_dtype)
    topo = init_topology(topo_parties, None, backend,
                     "cuda" if use_cuda else None)
    device = topo.device

    # fail loudly if the native extension is missing on a GPU machine
    if use_cuda:
        from geomx_amd import ops
        if not ops.native_available():
            raise RuntimeError("GPU run without native _geops extension: "
                               + str(ops.native_error()))

    torch.manual_seed(1234)  # same random init on all ranks
    if use_cuda:
        torch.backends.cudnn.benchmark = True  # MIOpen find mode
    model = create_model(args.model, image_size=args.image_size,
                         num_classes=args.num_classes).to(device)
    channels_last = use_cuda and not args.no_channels_last
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    spec = OptimizerSpec(name=args.optimizer, lr=0.01, momentum=0.9)
    trainer = GeoTrainer(model, cfg, topo, spec, mode=args.mode)

    bs = args.batch_size
    x = torch.randn(bs, 3, args.image_size, args.image_size, device=device)
    if channels_last:
        x = x.to(memory_format=torch.channels_last)
    y = torch.randint(0, args.num_classes, (bs,), device=device)

    amp_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    amp = args.dtype == "bf16"

    last = {}  # what the most recent step returned (no sync: refs only)

    def one_step():
        with torch.autocast(device_type=device_str, dtype=amp_dtype,
                            enabled=amp):
            out = model(x)
            loss = torch.nn.functional.cross_entropy(out, y)
        last["logits"], last["loss"] = out, loss
        trainer.zero_grad()
        loss.backward()
        trainer.step()
        return loss

    for _ in range(args.warmup):
        one_step()

    # hipGraph capture: the N=1 step is launch-gap bound for ~13% of
    # wall (5.6 ms GPU-busy vs 6.5 ms wall, r02 profile); capturing the
    # whole fwd+bwd+update in one graph removes the gaps. Multi-rank
    # runs keep eager (RCCL collectives + WAN pacing are host-driven).
    step_fn = one_step
    if use_cuda and world == 1 and args.hip_graph:
        try:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                one_step()
            torch.cuda.synchronize()
            step_fn = graph.replay
        except Exception as e:  # noqa: BLE001 - fall back to eager
            print(f"# hipGraph capture unavailable ({type(e).__name__}): "
                  "eager steps", file=sys.stderr)
            step_fn = one_step

    if distmod.is_initialized():
        distmod.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step_fn()
    if use_cuda:
        torch.cuda.synchronize()
    if distmod.is_initialized():
        distmod.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if distmod.is_initialized() and world > 1:
        t = torch.tensor([elapsed], device=device if backend == "nccl" else "cpu")
        distmod.all_reduce(t, op=distmod.ReduceOp.MAX)
        elapsed = t.item()

    if args.dump_outputs and rank == 0:
        tensors = dict(last)
        for name, prm in model.named_parameters():
            tensors["param." + name] = prm
        dump_outputs(args.dump_outputs, tensors)

    samples = world * bs * args.steps
    sps = samples / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if rank == 0:
        result = {
            "metric": "samples/sec (whole node)",
            "value": round(sps, 2),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "input": f"3x{args.image_size}x{args.image_size}",
                "global_batch": world * bs,
                "per_gpu_batch": bs,
                "parallelism": (f"hips{topo.num_parties}x"
                                f"{world // max(1, topo.num_parties)}"
                                if args.mode == "hips" else f"dp{world}"),
                "compression": args.compress,
                "sync_mode": args.sync_mode,
                "wan_gbps": args.wan_gbps,
                "optimizer": args.optimizer,
            },
        }
        line = json.dumps(result)
        print(line)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")

    if distmod.is_initialized():
        distmod.destroy_process_group()


if __name__ == "__main__":
    main()
