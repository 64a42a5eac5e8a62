"""FP8 wire kernels (k_fp8_encode, k_wire_sum_fp8) against the golden model
of ops.reference on the CPU copy of the same operands."""

import pytest
import torch

from test_fp8_wire_cpu import fp8_data

from geomx_amd import ops
from geomx_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (65, 64), (64 * 7 + 3, 64), (1000, 256),
          (2 * 8192 + 5, 8192)]


def boundary_data(n, chunk, seed=0):
    """fp8_data with amax = 1.75 * 2^3 = 14 (above every random element) in
    chunk 0, one ulp above it in chunk 3 and one below in chunk 4."""
    x, r = fp8_data(n, chunk, seed)
    at = torch.tensor(14.0)
    for ch, v in ((0, at), (3, torch.nextafter(at, torch.tensor(99.0))),
                  (4, torch.nextafter(at, torch.tensor(0.0)))):
        if ch * chunk < n:
            x[ch * chunk], r[ch * chunk] = v, 0.0
    return x, r


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("n,chunk", SHAPES)
def test_encode(n, chunk, with_res):
    x, r = boundary_data(n, chunk)
    rg = r.cuda() if with_res else None
    got = torch.empty(ops.fp8_wire_bytes(n, chunk), dtype=torch.uint8,
                      device="cuda")
    ops._geops.fp8_encode(x.cuda(), rg, got, chunk)
    want = ref.fp8_encode(x, r if with_res else None, chunk)
    ncodes = -(-n // chunk) * chunk
    got = got.cpu()
    assert torch.equal(got[ncodes:], want[ncodes:])      # scales, padding
    # the sign of a value that rounds to zero is not part of the contract
    codes, wcodes = got[:ncodes].clone(), want[:ncodes].clone()
    codes[codes == 0x80] = 0
    wcodes[wcodes == 0x80] = 0
    assert torch.equal(codes, wcodes)
    if with_res:
        assert torch.equal(rg.cpu(), r)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("P", [1, 3, 17])
@pytest.mark.parametrize("n,chunk", SHAPES[:3])
def test_wire_sum(n, chunk, P, accumulate):
    payloads = [ops.fp8_encode(fp8_data(n, chunk, seed=p)[0].cuda() * 2.0 ** p,
                               None, chunk) for p in range(P)]
    ds = [ref.fp8_decode(p.cpu(), n, chunk) for p in payloads]
    start = torch.randn(n) if accumulate else torch.zeros(n)
    buf = torch.full((n + 16,), 123.0, device="cuda")
    out = buf[:n]
    out.copy_(start)
    ops.wire_sum_fp8(payloads, n, chunk, out=out, accumulate=accumulate)
    chain = start.cuda()
    for d in ds:
        chain += d.cuda()
    assert torch.equal(out, chain)
    # at most P rounded adds, each within 2^-24 of a partial sum that the
    # sum of magnitudes bounds (the start value is a term of the sum)
    terms = torch.stack([start] + ds).double()
    assert ((out.cpu().double() - terms.sum(0)).abs()
            <= P * 2.0 ** -23 * terms.abs().sum(0)).all()
    assert (buf[n:] == 123.0).all()      # nothing stored at or past n


def _rejections():
    n, chunk = 128, 64
    x = torch.randn(n + 4, device="cuda")
    payload = torch.empty(ops.fp8_wire_bytes(n, chunk), dtype=torch.uint8,
                          device="cuda")
    out = torch.empty(n, device="cuda")
    g = ops._geops
    return {
        "payload length": lambda: g.wire_sum_fp8([payload[:-16]], out, chunk,
                                                 False),
        "chunk 96": lambda: g.fp8_encode(x[:n], None, payload, 96),
        "misaligned x": lambda: g.fp8_encode(x[1:n + 1], None, payload,
                                             chunk),
        "cpu out": lambda: g.wire_sum_fp8([payload], out.cpu(), chunk, False),
    }


@pytest.mark.parametrize("case", ["payload length", "chunk 96",
                                  "misaligned x", "cpu out"])
def test_rejections(case):
    with pytest.raises(RuntimeError):
        _rejections()[case]()
