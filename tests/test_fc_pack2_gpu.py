"""fc1 weight path (csrc/fc.hip): both bf16 weight layouts from one read
(k_fc_w_pack2_bf16), and the weight gradient un-permuted straight into
its span of the trainer's gradient bucket (k_fc_w_unpermute_into,
geomx_amd/gradsink.py).

The kernels only move and convert values, so every comparison is
torch.equal on integer views; no tolerance anywhere. Shapes are
(O, HW) with C = 32: odd and even HW, a lone partial tile, one full
128-pixel tile, a one-element tail, both parities of a row's first
element and a leftover element at both ends of a tile.
"""

import pytest
import torch
import torch.nn.functional as F

import geomx_amd.ops as ops
from geomx_amd.ops.fc import GeoFlattenLinear

DEV = "cuda:0"
C = 32
SHAPES = [(1, 1), (3, 127), (2, 128), (3, 129), (2, 257)]


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


# fp32 bit patterns planted among random values
_PLANTS = [
    0x00000000, 0x80000000,              # +-0
    0x7F800000, 0xFF800000,              # +-inf
    0x00000001, 0x80000001,              # smallest fp32 denormals
    0x00012345, 0x807FFFFF,              # denormals across the bf16 step
    0x3F808000, 0xBF808000,              # tie, bf16 lsb 0: rounds down
    0x3F818000, 0xBF818000,              # tie, bf16 lsb 1: rounds up
    0x3F808001, 0x3F807FFF,              # just above / below a tie
    0x7F7FFFFF, 0xFF7FFFFF,              # largest finite: rounds to inf
]
_NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF]


def _i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def _weight(O, HW, seed, plants):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(O * C * HW, generator=g)
    bits = w.view(torch.int32)
    n = w.numel()
    # spread over the tensor, first and last element included
    pos = [(i * (n - 1)) // (len(plants) - 1) for i in range(len(plants))]
    assert len(set(pos)) == len(pos) or n < len(plants)
    for p, v in zip(pos, plants):
        bits[p] = _i32(v)
    return w.view(O, C * HW).to(DEV), pos


SENT = 0x7B7B  # bf16 sentinel bits


def _sentinel_bf16(n, lead):
    buf = torch.full((lead + n + 24,), SENT, dtype=torch.int16, device=DEV)
    return buf, buf[lead:lead + n].view(torch.bfloat16)


def _intact(buf, lead, n):
    return bool((buf[:lead] == SENT).all()) and \
        bool((buf[lead + n:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("O,HW", SHAPES)
def test_pack2_bits(geops, O, HW):
    w, _ = _weight(O, HW, seed=O * 1000 + HW, plants=_PLANTS)
    n = w.numel()
    # wb at a 4 B-, wp at a 16 B-aligned offset of sentinel-filled buffers
    bb, wb_out = _sentinel_bf16(n, 2)
    pb, wp_out = _sentinel_bf16(n, 8)
    wb, wp = geops.fc_w_pack2_bf16(w, O, C, HW, True, wb_out.view(O, -1),
                                   wp_out.view(O, -1))
    torch.cuda.synchronize()
    assert wb.data_ptr() == wb_out.data_ptr()
    assert wp.data_ptr() == wp_out.data_ptr()
    ref_b = w.to(torch.bfloat16)
    ref_p = geops.fc_w_permute_bf16(w, O, C, HW)
    assert torch.equal(wb.view(torch.int16).view(-1),
                       ref_b.view(torch.int16).view(-1))
    assert torch.equal(wp.view(torch.int16).view(-1),
                       ref_p.view(torch.int16).view(-1))
    assert _intact(bb, 2, n) and _intact(pb, 8, n)
    # the default route: freshly allocated outputs, same bits
    wb2, wp2 = geops.fc_w_pack2_bf16(w, O, C, HW, True)
    assert wb2.shape == (O, C * HW) and wp2.shape == (O, HW * C)
    assert torch.equal(wb2.view(torch.int16), ref_b.view(torch.int16))
    assert torch.equal(wp2.view(torch.int16), ref_p.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("O,HW", SHAPES)
def test_pack2_without_perm(geops, O, HW):
    w, _ = _weight(O, HW, seed=7 + HW, plants=_PLANTS)
    n = w.numel()
    bb, wb_out = _sentinel_bf16(n, 2)
    wb, wp = geops.fc_w_pack2_bf16(w, O, C, HW, False, wb_out.view(O, -1))
    torch.cuda.synchronize()
    assert wp is None
    assert torch.equal(wb.view(torch.int16).view(-1),
                       w.to(torch.bfloat16).view(torch.int16).view(-1))
    assert _intact(bb, 2, n)
    wb2, wp2 = geops.fc_w_pack2_bf16(w, O, C, HW, False)
    assert wp2 is None
    assert torch.equal(wb2.view(torch.int16), wb.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("O,HW", [(3, 129)])
def test_pack2_nan(geops, O, HW):
    w, pos = _weight(O, HW, seed=5, plants=_NANS)
    wb, wp = geops.fc_w_pack2_bf16(w, O, C, HW, True)
    nan = torch.isnan(w)
    assert int(nan.sum()) == len(_NANS)
    assert torch.equal(torch.isnan(wb), nan)
    # wp[o][hw][c] = w[o][c][hw]
    nan_p = nan.view(O, C, HW).permute(0, 2, 1).reshape(O, HW * C)
    assert torch.equal(torch.isnan(wp), nan_p)
    ok = ~nan
    assert torch.equal(wb[ok].view(torch.int16),
                       w.to(torch.bfloat16)[ok].view(torch.int16))
    ref_p = geops.fc_w_permute_bf16(w, O, C, HW)
    assert torch.equal(wp.view(torch.int16), ref_p.view(torch.int16))


def _permuted_grad(O, HW, seed):
    g = torch.Generator().manual_seed(seed)
    gp = torch.randn(O * HW * C, generator=g).to(torch.bfloat16)
    bits = gp.view(torch.int16)
    n = gp.numel()
    plants = [0x8000, 0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80,
              0x8000]
    for i, v in enumerate(plants):   # first and last element included
        bits[(i * (n - 1)) // (len(plants) - 1)] = \
            v - (1 << 16) if v >= (1 << 15) else v
    return gp.view(O, HW * C).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("O,HW", SHAPES)
@pytest.mark.parametrize("off", [0, 1, 64])
def test_unpermute_into(geops, O, HW, off):
    gp = _permuted_grad(O, HW, seed=O * 100 + HW)
    n = gp.numel()
    ref_f = geops.fc_w_unpermute_f32(gp, O, C, HW)
    ref = torch.zeros(O, C * HW, device=DEV) + ref_f
    # the planted -0 reaches the plain kernel's output as -0 ...
    neg0 = ref_f.view(torch.int32) == -(1 << 31)
    assert bool(neg0.any())
    sent = 0x4B4B4B4B
    buf = torch.full((off + n + 67,), sent, dtype=torch.int32, device=DEV)
    dst = buf[off:off + n].view(torch.float32).view(O, C * HW)
    assert geops.fc_w_unpermute_into(gp, dst, O, C, HW) is None
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int32), ref.view(torch.int32))
    # ... and is +0 here, as `0 + x` made it
    assert bool((dst.view(torch.int32)[neg0] == 0).all())
    assert bool((buf[:off] == sent).all())
    assert bool((buf[off + n:] == sent).all())


def _trainer_run(sinks, steps, probe=None, reg_first=False):
    from geomx_amd import Config
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    from geomx_amd.parallel import GeoTrainer
    from geomx_amd.topology import init_topology
    N, H, W, O = 4, 3, 3, 8
    torch.manual_seed(0)
    model = torch.nn.Sequential(GeoFlattenLinear(C * H * W, O)).to(DEV)
    w = model[0].weight
    if probe is not None:
        # registered before the trainer's hook: sees what autograd
        # installed, before any repair
        w.register_post_accumulate_grad_hook(
            lambda p: probe.append(p.grad.data_ptr()))
    tr = GeoTrainer(model, Config.from_env(),
                    init_topology(1, None, None, DEV),
                    OptimizerSpec("sgd_mom", lr=0.05), grad_sinks=sinks)
    b, i = tr.param_bucket[w]
    span = b.views[i]
    flats = []
    g = torch.Generator().manual_seed(1)
    for s in range(steps):
        x = torch.randn(N, C, H, W, generator=g).to(DEV) \
            .contiguous(memory_format=torch.channels_last).requires_grad_()
        y = torch.randint(0, O, (N,), generator=g).to(DEV)
        tr.zero_grad()
        assert (w.grad is None) == sinks
        if reg_first:
            # the weight's first gradient of the step by another route:
            # the sink must be spent when the native backward runs
            (0.1 * w.pow(2).sum()).backward()
            assert w.grad.data_ptr() == span.data_ptr()
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(model(x), y)
        loss.backward()
        assert w.grad.data_ptr() == span.data_ptr()
        assert x.grad is not None
        flats.append([bk.flat.clone() for bk in tr.buckets] + [x.grad])
        tr.step()
    return flats, [p.detach().clone() for p in model.parameters()], span


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 3])
def test_module_under_trainer(geops, steps):
    probe = []
    fa, pa, span = _trainer_run(True, steps, probe)
    # adopted without a copy: autograd itself installed the bucket span
    assert probe == [span.data_ptr()] * steps
    fb, pb, _ = _trainer_run(False, steps)
    for sa, sb in zip(fa, fb):
        for a, b in zip(sa, sb):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(pa, pb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_module_under_trainer_other_route_first(geops):
    """A regulariser's own backward before the main one: the native
    backward must add to the span, as without a sink."""
    fa, pa, _ = _trainer_run(True, 2, reg_first=True)
    fb, pb, _ = _trainer_run(False, 2, reg_first=True)
    for sa, sb in zip(fa, fb):
        for a, b in zip(sa, sb):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(pa, pb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the regulariser's part is there: differs from the plain run
    fc, _, _ = _trainer_run(True, 1)
    assert not torch.equal(fa[0][0], fc[0][0])
