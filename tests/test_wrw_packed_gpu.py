"""conv1 weight gradient (k_conv5_wrw4_nhwc, 7 packed tap tiles) against
goldens recorded from the 10-tile parent kernel.

The packed kernel moves taps between A rows and changes when reads,
loads and stores are issued; every (tap, o) accumulator still receives
the same MFMAs in the same order, so each per-workgroup slab must equal
the parent's bit for bit: torch.equal, no tolerance. The goldens
(tests/golden/wrw_parent.npz, written by scripts/record_wrw_golden.py)
and the cases are described in tests/wrw_golden_cases.py."""

import numpy as np
import pytest
import torch

import geomx_amd.ops as ops
import wrw_golden_cases as G

DEV = "cuda:0"


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


@pytest.fixture(scope="module")
def golden():
    with np.load(G.GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files if k != "commit"}


_inputs = {}


def _case_inputs(h, w):
    if (h, w) not in _inputs:
        _inputs[(h, w)] = tuple(t if t is None else t.to(DEV)
                                for t in G.build_inputs(h, w))
    return _inputs[(h, w)]


def _run(geops, h, w, n_wg, pooled):
    x, go, gp, mask = _case_inputs(h, w)
    ho, wo = h - 4, w - 4
    part = torch.zeros(n_wg, G.T16, G.CO, dtype=torch.float32, device=DEV)
    if pooled:
        geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, G.N, h, w, ho, wo,
                                    G.CI, G.CO, n_wg)
    else:
        geops.conv5_wrw_nhwc(x, go, part, G.N, h, w, ho, wo, G.CI, G.CO,
                             n_wg)
    return part


def _check(geops, golden, h, w, n_wg, pooled):
    part = _run(geops, h, w, n_wg, pooled)
    want = golden[G.key(h, w, n_wg)].to(DEV)
    got = G.reduce_slabs(part)
    assert want.abs().sum().item() > 0
    assert torch.equal(got, want), (got - want).abs().max().item()
    # slab hygiene: rows outside the 100 taps and the bias row stay as
    # the caller zeroed them (guards the flush mapping)
    dead = part[:, G.dead_rows().to(DEV)]
    assert torch.equal(dead, torch.zeros_like(dead))


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
@pytest.mark.parametrize("h,w,n_wg", G.CASES)
def test_wrw4_packed_equals_parent(geops, golden, h, w, n_wg, pooled):
    _check(geops, golden, h, w, n_wg, pooled)


@pytest.mark.gpu
def test_wrw4_packed_odd_ho_equals_parent(geops, golden):
    """Ho = 5: the last block of each image has one row."""
    _check(geops, golden, *G.ODD_CASE, pooled=False)


@pytest.mark.gpu
def test_wrw4_idle_workgroups_leave_slabs_zero(geops):
    """More workgroups than row blocks: the spare slabs stay zero."""
    part = _run(geops, G.H, 26, 6, pooled=True)
    assert part[:4].abs().sum().item() > 0
    assert torch.equal(part[4:], torch.zeros_like(part[4:]))


def test_golden_file_covers_the_cases():
    with np.load(G.GOLDEN) as z:
        assert len(str(z["commit"])) >= 7
        for h, w, n_wg in G.CASES + [G.ODD_CASE]:
            a = z[G.key(h, w, n_wg)]
            assert a.shape == (n_wg, 101, G.CO) and a.dtype == np.float32
