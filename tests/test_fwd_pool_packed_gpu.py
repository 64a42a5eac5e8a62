"""Fused forward conv + bias + ReLU + max-pool kernels in their 4-row form
(k_conv5_pool16_nhwc, k_conv5_pool2_nhwc): weights in registers, double-
buffered prefetched staging, fragments shared between conv rows of equal
parity, packed 8-byte / 4-byte stores issued one block late.

Two oracles, both compared with torch.equal on out (bf16 bits) and mask:

* exact arithmetic: small-integer inputs, weights and bias make every
  partial sum exact in fp32 in any order, so a torch fp32 conv with an
  explicit first-maximum compare is the expected result bit for bit. Many
  windows tie and many clamp, which pins the tie rule, the codes and the
  packed store addressing.
* random values against tests/golden/fwd_pool_parent.npz, recorded from
  the 2-row kernels of the parent commit. This pins the accumulation
  order and the zeroed k-runs of chunk 12.

Every case runs on 1 and 2 workgroups (the persistent loop, every
prefetch hand-over, the one-pooled-row tail block after a full block)
and on the default grid. Shapes: tests/fwd_golden_cases.py."""

import numpy as np
import pytest
import torch

import fwd_golden_cases as G
import geomx_amd.ops as ops
from geomx_amd.ops import conv as C

DEV = "cuda:0"


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


_IDX = {}
_INPUTS = {}
_GOLDEN = []


def _w_frags(weight):
    shape = tuple(weight.shape)
    if shape not in _IDX:
        _IDX[shape] = C.build_fwd_index(shape)
    return C._w_frags(weight, _IDX[shape])


def _exact_case(case):
    """CPU inputs and expected tensors of one exact case, built once."""
    if case not in _INPUTS:
        x, weight, bias = G.exact_inputs(*case)
        out, codes = G.expected_exact(x, weight, bias)
        _INPUTS[case] = (x, _w_frags(weight), bias, out.view(torch.int16),
                         codes)
    return _INPUTS[case]


def _golden_case(case):
    if case not in _INPUTS:
        if not _GOLDEN:
            _GOLDEN.append(np.load(G.GOLDEN))
        x, weight, bias = G.random_inputs(*case)
        k = G.key(*case)
        _INPUTS[case] = (x, _w_frags(weight), bias,
                         torch.from_numpy(_GOLDEN[0][k + "_out"]),
                         torch.from_numpy(_GOLDEN[0][k + "_mask"]))
    return _INPUTS[case]


def _run(geops, x, w_frags, bias, co, n_wg):
    """out [N][Hop][Wop][CO] as int16 bits and flat codes, on the CPU.
    Both are pre-filled with values the kernel never writes."""
    n, ci, h, w = x.shape
    hop, wop = (h - 4) // 2, (w - 4) // 2
    out = torch.full((n, hop, wop, co), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    mask = torch.full((out.numel(),), 77, dtype=torch.uint8, device=DEV)
    b = bias.to(DEV) if bias is not None else torch.Tensor()
    args = (x.to(DEV), w_frags.to(DEV), b, out, mask, n, h, w, h - 4, w - 4,
            ci, co)
    if n_wg is None:
        geops.conv5_pool_nhwc(*args)
    else:
        geops.conv5_pool_nwg_nhwc(*args, n_wg)
    return out.view(torch.int16).cpu(), mask.cpu().reshape(out.shape)


def _tied(x, weight, bias):
    """Windows whose positive maximum is reached by more than one pixel."""
    import torch.nn.functional as F
    conv = F.conv2d(x[:, :weight.shape[1]].float(), weight, bias)
    q = torch.stack([conv[:, :, dy::2, dx::2]
                     for dy in range(2) for dx in range(2)])
    mx = q.max(dim=0).values
    return ((q == mx).sum(dim=0) > 1) & (mx > 0)


@pytest.mark.parametrize("case", [c for c in G.EXACT if c[4] == "int"],
                         ids=lambda c: "%d-%d-h%d-w%d-%s" % c)
def test_exact_cases_have_ties_and_clamps(case):
    """The expected tensors of the exact cases really hold what they are
    meant to pin: tied windows, clamped windows, all four quadrants."""
    x, weight, bias = G.exact_inputs(*case)
    _, codes = G.expected_exact(x, weight, bias)
    assert _tied(x, weight, bias).sum().item() >= 4
    present = set(codes.unique().tolist())
    assert present == {0, 1, 2, 3, 255}, present


def test_negative_bias_case_is_nearly_all_clamped():
    for case in G.EXACT:
        if case[4] != "neg":
            continue
        _, codes = G.expected_exact(*G.exact_inputs(*case))
        assert (codes == 255).float().mean().item() > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", G.GRIDS)
@pytest.mark.parametrize("case", G.EXACT,
                         ids=lambda c: "%d-%d-h%d-w%d-%s" % c)
def test_exact_arithmetic(geops, case, n_wg):
    x, w_frags, bias, want_out, want_codes = _exact_case(case)
    out, codes = _run(geops, x, w_frags, bias, case[1], n_wg)
    assert torch.equal(codes, want_codes), \
        (codes != want_codes).nonzero()[:8]
    assert torch.equal(out, want_out), (out != want_out).nonzero()[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", G.GRIDS)
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "%d-%d-h%d-w%d" % c)
def test_random_values_equal_parent(geops, case, n_wg):
    x, w_frags, bias, want_out, want_codes = _golden_case(case)
    out, codes = _run(geops, x, w_frags, bias, case[1], n_wg)
    assert torch.equal(codes, want_codes.reshape(codes.shape)), \
        (codes != want_codes.reshape(codes.shape)).nonzero()[:8]
    assert torch.equal(out, want_out), (out != want_out).nonzero()[:8]


@pytest.mark.gpu
def test_hook_rejects_bad_arguments(geops):
    def run(cir, co, h, w, n_wg, wi=None):
        ci = (cir + 3) & ~3
        x = torch.zeros(G.N, h, wi or w, ci, device=DEV,
                        dtype=torch.bfloat16).permute(0, 3, 1, 2)
        wf = _w_frags(torch.zeros(co, cir, 5, 5)).to(DEV)
        out = torch.zeros(G.N, (h - 4) // 2, (w - 4) // 2, co, device=DEV,
                          dtype=torch.bfloat16)
        mask = torch.zeros(out.numel(), dtype=torch.uint8, device=DEV)
        geops.conv5_pool_nwg_nhwc(x, wf, torch.Tensor(), out, mask, G.N, h,
                                  w, h - 4, w - 4, ci, co, n_wg)

    run(16, 32, 10, 20, 1)                  # the well-formed call passes
    for n_wg in (0, -1):
        with pytest.raises(RuntimeError):
            run(16, 32, 10, 20, n_wg)
    with pytest.raises(RuntimeError):       # wider than the 120-pixel table
        run(16, 32, 10, 118, 1)
    with pytest.raises(RuntimeError):       # odd conv height
        run(16, 32, 11, 20, 1)
    with pytest.raises(RuntimeError):       # odd conv width
        run(3, 16, 10, 21, 1)
    with pytest.raises(RuntimeError):       # no kernel for 16 -> 48
        run(16, 48, 10, 20, 1)
    with pytest.raises(RuntimeError):       # input smaller than the geometry
        run(16, 32, 10, 20, 1, wi=18)
