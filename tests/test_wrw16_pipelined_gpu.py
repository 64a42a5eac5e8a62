"""conv2-class weight gradient (k_conv5_wrw16_nhwc, pipelined reads and
prefetched pooled staging), the one-launch weight packing
(k_conv5_pack_frags) and the slabs allocated without a zero fill.

  * exact oracle: integer inputs make every fp32 partial sum exact, so a
    slab must equal the float64 gradient over exactly the blocks its
    workgroup owns, in any order: torch.equal, no tolerance, no fixture.
  * order invariant: on normal inputs every (tap, o) accumulator must
    receive the parent kernel's MFMAs in the parent's order, so the slabs
    equal tests/golden/wrw16_parent.npz bit for bit.
  * packing: the kernel equals ops.conv._w_frags bit for bit.
  * wrw4 writes zeros to its dead slab rows, whatever the slab held.
Cases and builders: tests/wrw16_golden_cases.py."""

import numpy as np
import pytest
import torch

import geomx_amd.ops as ops
import geomx_amd.ops.conv as C
import wrw16_golden_cases as G
import wrw_golden_cases as G4

DEV = "cuda:0"


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


_inputs = {}
_blocks = {}


def _case_inputs(h, w, co, exact):
    k = (h, w, co, exact)
    if k not in _inputs:
        _inputs[k] = G.build_inputs(h, w, co, exact)
    return _inputs[k]


def _oracle(h, w, co, n_wg):
    """Expected slabs of an exact case; the per-block float64 gradients
    are computed once per geometry and shared by its grids and forms."""
    k = (h, w, co)
    if k not in _blocks:
        x, go, _, _ = _case_inputs(h, w, co, True)
        _blocks[k] = G.block_grads(x, go)
    return G.slab_oracle(_blocks[k], n_wg)


def _run(geops, h, w, n_wg, co, pooled, exact):
    x, go, gp, mask = (t if t is None else t.to(DEV)
                       for t in _case_inputs(h, w, co, exact))
    ho, wo = h - 4, w - 4
    # the kernel must write every slab row itself
    part = torch.full((n_wg, G.T16, co), float("nan"), dtype=torch.float32,
                      device=DEV)
    if pooled:
        geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, G.N, h, w, ho, wo,
                                    G.CI, co, n_wg)
    else:
        geops.conv5_wrw_nhwc(x, go, part, G.N, h, w, ho, wo, G.CI, co, n_wg)
    return part.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
@pytest.mark.parametrize("h,w,n_wg,co", G.EXACT_CASES)
def test_wrw16_exact(geops, h, w, n_wg, co, pooled):
    got = _run(geops, h, w, n_wg, co, pooled, exact=True)
    want = _oracle(h, w, co, n_wg)
    assert want[:, :G.BIAS_ROW + 1].abs().sum().item() > 0
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.gpu
def test_wrw16_exact_odd_ho(geops):
    """Ho = 5: the last block of each image has one row."""
    h, w, n_wg, co = G.ODD_CASE
    got = _run(geops, h, w, n_wg, co, False, exact=True)
    want = _oracle(h, w, co, n_wg)
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.fixture(scope="module")
def golden():
    with np.load(G.GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files if k != "commit"}


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
@pytest.mark.parametrize("h,w,n_wg,co", G.GOLDEN_CASES)
def test_wrw16_equals_parent(geops, golden, h, w, n_wg, co, pooled):
    got = _run(geops, h, w, n_wg, co, pooled, exact=False)
    want = golden[G.key(h, w, n_wg, co)]
    assert want.abs().sum().item() > 0
    assert torch.equal(got[:, :G.BIAS_ROW + 1], want), \
        (got[:, :G.BIAS_ROW + 1] - want).abs().max().item()
    tail = got[:, G.BIAS_ROW + 1:]
    assert torch.equal(tail, torch.zeros_like(tail))


def test_wrw16_golden_file_covers_the_cases():
    with np.load(G.GOLDEN) as z:
        assert len(str(z["commit"])) >= 7
        for h, w, n_wg, co in G.GOLDEN_CASES:
            a = z[G.key(h, w, n_wg, co)]
            assert a.shape == (n_wg, G.BIAS_ROW + 1, co)
            assert a.dtype == np.float32


# ---------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------

def _bf16_edge_weights(shape):
    """Random weights with the values a bf16 rounding can get wrong
    planted at the front: +-0, exact ties (round to even both ways),
    just above and below a tie, subnormals, the largest finite values
    (the last rounds to inf, as Tensor.to does)."""
    g = torch.Generator().manual_seed(31 + shape[0])
    w = torch.randn(shape, generator=g)
    bits = [0x00000000, 0x80000000,
            0x3F808000, 0x3F818000,      # ties: down to even, up to even
            0xBF808000, 0xBF818000,
            0x3F808001, 0x3F817FFF,      # just above / just below a tie
            0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF,
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF]
    edge = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32))
    w.view(-1)[:edge.numel()] = edge
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 3, 5, 5), (32, 16, 5, 5)])
def test_pack_frags_equals_w_frags(geops, shape):
    w = _bf16_edge_weights(shape).to(DEV)
    fwd = C.build_fwd_index(shape).to(DEV)
    dgrad = C.build_dgrad_index(shape).to(DEV)
    want_f = C._w_frags(w, fwd).view(torch.int16)
    want_d = C._w_frags(w, dgrad).view(torch.int16)
    assert want_f.abs().sum().item() > 0 and want_d.abs().sum().item() > 0
    one_f, = geops.conv5_pack_frags(w, fwd)
    one_d, = geops.conv5_pack_frags(w, dgrad)
    two_f, two_d = geops.conv5_pack_frags(w, fwd, dgrad)
    for got, want in ((one_f, want_f), (one_d, want_d), (two_f, want_f),
                      (two_d, want_d)):
        assert got.dtype == torch.bfloat16 and got.shape == want.shape
        assert torch.equal(got.view(torch.int16), want)
    # the route the conv stages take
    r_f, r_d = C._pack_frags(w, fwd, dgrad)
    assert torch.equal(r_f.view(torch.int16), want_f)
    assert torch.equal(r_d.view(torch.int16), want_d)


# ---------------------------------------------------------------------
# wrw4: dead slab rows
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
def test_wrw4_zeroes_its_dead_rows(geops, pooled):
    h, w, n_wg = G4.H, 40, 3
    x, go, gp, mask = (t.to(DEV) for t in G4.build_inputs(h, w))
    ho, wo = h - 4, w - 4

    def run(part):
        if pooled:
            geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, G4.N, h, w, ho,
                                        wo, G4.CI, G4.CO, n_wg)
        else:
            geops.conv5_wrw_nhwc(x, go, part, G4.N, h, w, ho, wo, G4.CI,
                                 G4.CO, n_wg)
        return part.cpu()

    ref = run(torch.zeros(n_wg, G4.T16, G4.CO, dtype=torch.float32,
                          device=DEV))
    got = run(torch.empty(n_wg, G4.T16, G4.CO, dtype=torch.float32,
                          device=DEV).fill_(-7.5))
    dead = got[:, G4.dead_rows()]
    assert torch.equal(dead, torch.zeros_like(dead))
    assert G4.reduce_slabs(ref).abs().sum().item() > 0
    assert torch.equal(G4.reduce_slabs(got), G4.reduce_slabs(ref))
    assert torch.equal(got, ref)
