"""Fused DGT encode (csrc/dgtencode.hip) on gfx950: ops.dgt_encode against
the op chain it replaces (ops.reference.dgt_encode) bit for bit, the codec
property of its output in float64, and DGTState.compress over three steps
of residual feedback."""
import math

import pytest
import torch

from geomx_amd import ops
from geomx_amd.kvstore.dgt import DGTState
from geomx_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL = (1024, 7 * 1024 + 5, 0.5)  # the case with the hand-built chunks
DEAD_LOSSY, DEAD_KEPT, CONSTANT = 1, 2, 4

# (chunk, numel, k, scale of the last chunk's values: large keeps it, small
# makes it lossy, None leaves it to chance)
CASES = [
    (1024, 8 * 1024, 0.5, None),
    SPECIAL + (100.0,),
    SPECIAL + (0.01,),
    (64, 64 * 9 + 2, 0.25, None),
    (128, 128 * 7 + 3, 0.5, 0.01),       # 32 lanes per chunk
    (256, 256 * 5 + 131, 0.5, None),
    (512, 512 * 4, 0.5, None),
    (2048, 2048 * 3 + 9, 0.25, 0.01),    # 2 granules per lane
    (4096, 4096 * 3 + 1, 0.34, None),
    (8192, 8192 * 2, 0.5, None),
    (1024, 300, 0.5, None),              # a single partial chunk
    (1024, 4 * 1024, 1.0, None),         # n_lossy = 0
    # more chunks than one sweep of the 2048-workgroup grid: 16 chunks of 64
    # per workgroup, and 1 chunk of 1024 (second trip of the LDS exchange)
    (64, 64 * (2048 * 16 + 40) + 2, 0.5, None),
    (1024, 1024 * (2048 + 3) + 7, 0.5, 0.01),
]


def _inputs(chunk, numel, k, tail):
    g = torch.Generator(device=DEV).manual_seed(chunk + numel)
    x = torch.randn(numel, device=DEV, generator=g)
    res = 0.05 * torch.randn(numel, device=DEV, generator=g)
    nchunks = (numel + chunk - 1) // chunk
    if tail is not None:
        x[(nchunks - 1) * chunk:] *= tail
    if (chunk, numel, k) == SPECIAL:
        for c in (DEAD_LOSSY, DEAD_KEPT):   # contrib == 0, residual nonzero
            x[c * chunk:(c + 1) * chunk] = 0.0
        x[CONSTANT * chunk:(CONSTANT + 1) * chunk] = 0.37   # hi == lo
        res[CONSTANT * chunk:(CONSTANT + 1) * chunk] = 0.0
    contrib = ops.dgt_contribution(x, chunk)
    rank = contrib.clone()
    if (chunk, numel, k) == SPECIAL:
        rank[DEAD_KEPT] = math.inf
    n_keep = max(1, int(math.ceil(k * nchunks)))
    keep_idx = torch.topk(rank, n_keep).indices.sort().values
    return x, res, contrib, keep_idx


@pytest.mark.parametrize("chunk,numel,k,tail", CASES)
def test_dgt_encode_equals_chain(chunk, numel, k, tail):
    x, res, contrib, keep_idx = _inputs(chunk, numel, k, tail)
    nchunks = contrib.numel()
    if (chunk, numel, k) == SPECIAL:
        kept = set(keep_idx.tolist())
        assert DEAD_KEPT in kept and DEAD_LOSSY not in kept \
            and CONSTANT not in kept
        assert ((nchunks - 1) in kept) == (tail > 1)
        assert contrib[DEAD_KEPT] == 0 and contrib[DEAD_LOSSY] == 0
    r_fused, r_chain = res.clone(), res.clone()
    fused = ops.dgt_encode(x, r_fused, contrib, keep_idx, chunk)
    chain = ref.dgt_encode(x, r_chain, contrib, keep_idx, chunk)
    for name, a, b in zip(("exact", "keep_idx", "packed", "minmax"),
                          fused, chain):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name
    assert torch.equal(r_fused, r_chain)


@pytest.mark.parametrize("chunk,numel,k,tail",
                         [SPECIAL + (0.01,), (64, 64 * 9 + 2, 0.25, None)])
def test_dgt_encode_codec_float64(chunk, numel, k, tail):
    x, res, contrib, keep_idx = _inputs(chunk, numel, k, tail)
    nchunks = contrib.numel()
    r_new = res.clone()
    _, _, packed, minmax = ops.dgt_encode(x, r_new, contrib, keep_idx, chunk)

    def rows(t, fill=0.0):  # [nchunks, chunk], zeros past numel
        p = torch.full((nchunks * chunk,), fill, dtype=t.dtype, device=DEV)
        p[:numel] = t
        return p.view(nchunks, chunk)
    lossy = torch.ones(nchunks, dtype=torch.bool, device=DEV)
    lossy[keep_idx] = False
    live = contrib[lossy] != 0           # dead rows carry a zeroed codebook
    f32 = rows(x + res)[lossy][live]     # what the kernel quantizes
    f64 = rows(x.double() + res.double())[lossy][live]
    rn = rows(r_new)[lossy][live].double()
    below = rows(torch.ones(numel, device=DEV))[lossy][live] > 0
    lo, hi = minmax[live, 0:1], minmax[live, 1:2]
    assert torch.equal(lo.double(), f32.double().min(dim=1, keepdim=True)[0])
    assert torch.equal(hi.double(), f32.double().max(dim=1, keepdim=True)[0])
    step = (torch.clamp(hi - lo, min=1e-30) / 16.0).double()  # fp32 step4
    pk = packed.view(-1, chunk // 2)[live]
    codes = torch.stack([pk & 0xF, pk >> 4], dim=2).reshape(-1, chunk)
    decoded = lo.double() + (codes.double() + 0.5) * step
    eps = 2.0 ** -22 * torch.maximum(lo.abs(), hi.abs()).double()
    err = (f64 - (decoded + rn)).abs()
    assert bool((err <= eps)[below].all()), (err - eps)[below].max().item()
    excess = rn.abs() - (step / 2 + eps)
    assert bool((excess <= 0)[below].all()), excess[below].max().item()


def test_dgt_state_three_steps():
    chunk, numel = 256, 256 * 6 + 10
    a = DGTState(numel, DEV, chunk_elems=chunk, k=0.5, mode=3)
    b = DGTState(numel, DEV, chunk_elems=chunk, k=0.5, mode=3)
    g = torch.Generator(device=DEV).manual_seed(3)
    for step in range(3):
        x = torch.randn(numel, device=DEV, generator=g)
        fused = a.compress(x)
        b._update_contrib(x)
        keep_idx = torch.topk(b.contrib, b.n_keep).indices.sort().values
        chain = ref.dgt_encode(x, b.residual, b.contrib, keep_idx, chunk)
        for t, u in zip(fused, chain):
            assert torch.equal(t, u), step
        assert torch.equal(a.residual, b.residual), step
        assert torch.equal(a.contrib, b.contrib), step
        assert bool(a.residual.any())
