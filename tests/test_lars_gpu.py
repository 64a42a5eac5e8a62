"""k_lars_sumsq / k_lars_update against the float64 golden model at the tile
edges, on both VEC instantiations and on grids that make a block walk
several tiles."""

import functools

import pytest
import torch

from geomx_amd import ops
from geomx_amd.kvstore.optimizer import OptimizerSpec, ServerOptimizer
from geomx_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 4096   # ops.LARS_TILE, asserted below

# segment lengths. VEC = 4 needs offsets that are multiples of 4, so the
# tile edges come twice: as such (VEC = 1) and rounded to granules (VEC = 4)
LAYOUTS = {
    "edges": [1, 63, T - 1, T, T + 1, 3 * T + 5],
    "edges4": [4, 64, T - 4, T, T + 4, 3 * T + 8],
    "single": [3 * T + 8],
    "one_between": [2 * T + 4, 1, 2 * T],
    "empty": [T + 4, 0, 2 * T, 0],
}

# Relative tolerance of a ratio against the float64 golden value. In the
# kernel as built an element's square passes through at most k = 24 fp32
# additions: 15 in its thread (16 elements folded in order; the fma rounds
# square and first addition together, but the thread's first square is
# rounded alone: 16 roundings), 6 in the wave butterfly, 3 over the four
# waves; the per-segment sum of the tile partials is in double (2^-53 per
# step, nothing here). All terms are >= 0, so each of W2 and G2 is within
# (1 +- u)^(k+1) of its exact value, u = 2^-24. ratio^2 is a quotient of two
# such sums (wd W2 and 1e-18 only pull it nearer), so it is off by at most
# 2 (k+1) u, its root by (k+1) u, and the store to fp32 adds u: (k+2) u, to
# first order in u (the next term, ~(k u)^2, is 1e-6 of this).
RTOL = (24 + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _case(layout, shift):
    """(w, g, seg_off, float64 golden ratios) on the GPU; shift = 1 puts a
    one-element segment in front, so no offset is a multiple of 4."""
    assert ops.LARS_TILE == T
    lens = [1] * shift + LAYOUTS[layout]
    seg = torch.tensor([0] + lens).cumsum(0)
    gen = torch.Generator().manual_seed(len(lens) + shift)
    w = torch.randn(int(seg[-1]), generator=gen)
    g = torch.randn(int(seg[-1]), generator=gen)
    gold = ref.lars_ratio(w, g, seg, 0.01, dtype=torch.float64)
    return w.to(DEV), g.to(DEV), seg.to(DEV), gold.to(DEV)


@pytest.mark.parametrize("n_wg", (1, 2, 0))
@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ratio(layout, shift, n_wg):
    w, g, seg, gold = _case(layout, shift)
    r1 = ops.lars_ratio(w, g, seg, 0.01, n_wg=n_wg)
    r2 = ops.lars_ratio(w, g, seg, 0.01, n_wg=n_wg)   # same workspace
    err = ((r1.double() - gold).abs() / gold).max().item()
    print("max relative error %.3g (bound %.3g)" % (err, RTOL))
    assert err <= RTOL
    assert torch.equal(r1, r2)   # counters were reset; no order dependence
    assert torch.equal(r1, ops.lars_ratio(w, g, seg, 0.01, n_wg=3))


def test_ratio_clamps():
    seg = torch.tensor([0, T + 4, T + 12, 3 * T + 12], device=DEV)
    w = torch.randn(3 * T + 12, device=DEV)
    g = torch.randn(3 * T + 12, device=DEV)
    w[T + 4:T + 12] = 0.0
    g[T + 4:T + 12] = 0.0
    g[T + 12:] *= 1e-6
    r = ops.lars_ratio(w, g, seg)
    assert r[1:].tolist() == [torch.tensor(0.01).item(), 100.0]


@pytest.mark.parametrize("momentum", (0.0, 0.9))
@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_update(layout, shift, momentum):
    w0, g, seg, _ = _case(layout, shift)
    w = w0.clone()
    mom = torch.zeros_like(w) if momentum else None
    w_ref, seg_ref = w0.cpu(), seg.cpu()
    mom_ref = torch.zeros_like(w_ref) if momentum else None
    ratio = torch.empty(seg.numel() - 1, device=DEV)
    for step in range(3):
        gs = g * (1.0 + step)
        got = ops.lbsgd_update(w, gs, mom, seg, 0.05, momentum, 0.01, 0.5,
                               2.0, ratio_out=ratio, n_wg=2)
        assert got is ratio
        ref.lbsgd_update(w_ref, gs.cpu(), mom_ref, seg_ref, 0.05, momentum,
                         0.01, 0.5, 2.0, ratio=ratio.cpu())
        torch.testing.assert_close(w.cpu(), w_ref, rtol=0, atol=1e-5)
        if momentum:
            torch.testing.assert_close(mom.cpu(), mom_ref, rtol=0, atol=1e-5)


def test_no_host_sync():
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        pytest.skip("sync debug mode does not raise on .item() in this build")
    w0, g, seg, _ = _case("edges4", 0)
    w, mom = w0.clone(), torch.zeros_like(w0)
    opt = ServerOptimizer(OptimizerSpec("lbsgd", warmup_strategy="lars",
                                        lr=0.05, clip_gradient=1.0))

    def calls():
        ops.lbsgd_update(w, g, mom, seg, 0.05, 0.9)
        opt.update("bucket", w, g, segments=seg)
        opt.update("key", w, g)     # one segment, as the kvstore calls it

    calls()   # first call: tables, workspace and state
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        calls()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(w).all().item() and not torch.equal(w, w0)
