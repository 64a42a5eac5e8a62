"""FP8 wire tier on the CPU: the properties of the golden model
(ops.reference), one gloo run through the kvstore, and Config's rules."""

import pytest
import torch

from dist_helpers import run_dist

from geomx_amd import Config, ops
from geomx_amd.kvstore import create
from geomx_amd.ops import reference as ref
from geomx_amd.topology import init_topology

SHAPES = [(1, 64), (65, 64), (64 * 7 + 3, 64), (1000, 256)]


def fp8_data(n, chunk, seed=0):
    """x and a residual: random, with chunk 1 zero and chunk 2 one large
    element among many tiny ones (where the shape has those chunks)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    r = torch.randn(n, generator=g) * 0.01
    rows_x, rows_r = x.split(chunk), r.split(chunk)
    if len(rows_x) > 1:
        rows_x[1].zero_()
        rows_r[1].zero_()
    if len(rows_x) > 2:
        rows_x[2].mul_(1e-6)
        rows_x[2][3] = 300.0
    return x, r


@pytest.mark.parametrize("n,chunk", SHAPES)
def test_reference_properties(n, chunk):
    x, r = fp8_data(n, chunk)
    c = (x + r).double()
    payload = ref.fp8_encode(x, r, chunk)
    assert payload.numel() == ops.fp8_wire_bytes(n, chunk)
    nchunks = -(-n // chunk)
    scales = payload[nchunks * chunk:nchunks * chunk + nchunks]
    e = (scales.double() - 127).repeat_interleave(chunk)[:n]
    d = ops.fp8_decode(payload, n, chunk).double()
    # the error of an E4M3 rounding at a power-of-two scale is an fp32 value
    assert torch.equal(d + r.double(), c)
    assert (r.double().abs()
            <= torch.maximum(c.abs() / 16, 2.0 ** (e - 10))).all()
    assert (c.abs() * 2.0 ** -e <= 448).all()
    if nchunks > 1:
        assert scales[1] == 0 and not d[chunk:2 * chunk].any()


@pytest.mark.parametrize("k", [-3, 0, 10])
def test_scale_byte_at_the_boundary(k):
    at = torch.tensor(1.75 * 2.0 ** k)
    zero, inf = torch.tensor(0.0), torch.tensor(float("inf"))
    for amax, e in ((torch.nextafter(at, zero), k - 8), (at, k - 8),
                    (torch.nextafter(at, inf), k - 7)):
        x = torch.zeros(64)
        x[5] = -amax
        assert ref.fp8_encode(x, None, 64)[64] == e + 127


def _fp8_kv(rank, world):
    n, chunk, P = 64 * 7 + 3, 64, 2
    cfg = Config.from_env(num_parties=P, backend="gloo", device="cpu",
                          compression="fp8", fp8_block=chunk,
                          wan_gbps=100.0)   # a capped link counts bytes
    topo = init_topology(cfg.num_parties, cfg.party_sizes, "gloo", "cpu")
    kv = create("dist_sync", cfg=cfg, topo=topo)
    kv.set_gradient_compression({"type": "fp8"})
    kv.init("w", torch.zeros(n))
    res = [torch.zeros(n) for _ in range(P)]
    out = torch.empty(n)
    for push in range(2):   # the second push carries the residual over
        grads = [fp8_data(n, chunk, seed=10 * push + w)[0]
                 for w in range(world)]
        before = kv.wan.total_bytes
        kv.push("w", grads[rank])
        kv.pull("w", out)
        payloads = [ref.fp8_encode(grads[2 * p] + grads[2 * p + 1], res[p],
                                   chunk) for p in range(P)]
        assert torch.equal(out, ref.wire_sum_fp8(payloads, n, chunk)), rank
        if kv.topo.is_leader:
            assert kv.wan.total_bytes - before \
                == (P - 1) * ops.fp8_wire_bytes(n, chunk)


def test_fp8_kvstore_ws4():
    run_dist(4, _fp8_kv)


@pytest.mark.parametrize("bad", [{"fp8_block": 96}, {"enable_ts": True}])
def test_config_rejects(bad):
    with pytest.raises(ValueError):
        Config(compression="fp8", **bad)
