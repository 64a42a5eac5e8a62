#!/usr/bin/env python3
"""FP8-transmission training: the sibling of cnn_fp16.py one tier down.
The WAN tier carries block-scaled E4M3 codes (one scale byte per
GEOMX_FP8_BLOCK elements, about 1 byte per element against fp16's 2) with
an error-feedback residual at each party leader; the server keeps its fp32
master copy. An extension: the reference stops at fp16 transmission."""

from common import base_parser, setup, train_loop

from geomx_amd.kvstore.optimizer import OptimizerSpec


def main():
    args = base_parser().parse_args()
    kv, net, device = setup(args, compression="fp8")
    kv.set_gradient_compression({"type": "fp8"})
    kv.set_optimizer(OptimizerSpec("adam", lr=args.learning_rate))
    steps = [0]

    def step(params, num_samples):
        for idx, p_ in enumerate(params):
            kv.push(idx, p_.grad / num_samples, priority=-idx)
            kv.pull(idx, p_.data, priority=-idx)
        steps[0] += 1

    train_loop(args, kv, net, device, step, tag="fp8")
    wan = getattr(kv, "wan", None)   # the distributed store's WAN meter
    if kv.rank == 0 and wan is not None and steps[0]:
        print("[fp8] WAN bytes per step %.0f"
              % (wan.stats()["total_bytes"] / steps[0]), flush=True)


if __name__ == "__main__":
    main()
