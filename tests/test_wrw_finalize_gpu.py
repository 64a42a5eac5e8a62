"""k_conv5_wrw_finalize (csrc/finalize.hip) and the conv gradient sinks.

The kernel ships in the form that takes the summed slab: the reduction
over the workgroups stays ATen's `part.sum(0)`, and the kernel replaces
the gather, the reshape and the two `0 + x` accumulations of the Python
chain. It only moves values, so every comparison is torch.equal on
integer views against that chain (sum, gather, reshape, then
`zeros_span += dw`), with every destination inside a sentinel-filled
buffer whose guard regions must stay untouched.
"""

import pytest
import torch
import torch.nn.functional as F

import geomx_amd.ops as ops
from geomx_amd.ops.conv import build_wrw_unpack_index

DEV = "cuda:0"
SENT = 0x7B7B7B7B
GUARD = 96

# (CIr, CO): wrw4 (CI=4, T16=176), wrw16 with CO=32 and CO=16 (T16=416)
SHAPES = [(3, 16), (16, 32), (16, 16)]
N_WG = [1, 2, 3, 64, 768]


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _span(numel, lead):
    """(buffer, lead offset): int32 sentinels, GUARD + lead in front."""
    buf = torch.full((GUARD + lead + numel + GUARD,), SENT, dtype=torch.int32,
                     device=DEV)
    return buf, GUARD + lead


def _view(buf, off, shape, channels_last):
    flat = buf.view(torch.float32)
    n = 1
    for s in shape:
        n *= s
    if channels_last:
        O, C, H, W = shape
        return flat[off:off + n].as_strided(shape, (C * H * W, 1, W * C, C),
                                            off)
    return flat[off:off + n].view(shape)


def _guards_intact(buf, off, n):
    return bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", N_WG)
@pytest.mark.parametrize("CIr,CO", SHAPES)
def test_finalize_matches_python_chain(geops, CIr, CO, n_wg):
    shape = (CO, CIr, 5, 5)
    idx, T16 = build_wrw_unpack_index(shape)
    assert T16 == (176 if CIr == 3 else 416)
    idx = idx.to(DEV)
    g = torch.Generator().manual_seed(1000 * CO + 10 * CIr + n_wg)
    part = torch.randn(n_wg, T16, CO, generator=g)
    # slab columns whose every partial is -0, in a weight tap row and in
    # the bias row. (ATen's sum starts from +0, so they come out of it as
    # +0 already; a -0 handed to the kernel itself is the next test.)
    part[:, 0, :4] = -0.0
    part[:, 17, 1] = -0.0
    part[:, T16 - 16, ::3] = -0.0
    part = part.to(DEV)
    full = part.sum(dim=0)
    dw_ref = full.reshape(-1)[idx].reshape(shape)
    db_ref = full[T16 - 16]
    n = dw_ref.numel()
    for channels_last in (False, True):
        for lead in (0, 1, 64):
            wbuf, woff = _span(n, lead)
            bbuf, boff = _span(CO, lead)
            dw = _view(wbuf, woff, shape, channels_last)
            db = bbuf.view(torch.float32)[boff:boff + CO]
            # the parent: a cleared span of the same geometry, then +=
            want_w = torch.zeros_like(dw)   # preserves the strides
            assert want_w.stride() == dw.stride()
            want_w += dw_ref
            want_b = torch.zeros(CO, device=DEV)
            want_b += db_ref
            assert geops.conv5_wrw_finalize(full, idx, dw, db, CO, CIr,
                                            T16) is None
            assert torch.equal(dw.view(torch.int32) if not channels_last
                               else dw.permute(0, 2, 3, 1).contiguous()
                               .view(torch.int32),
                               want_w.view(torch.int32) if not channels_last
                               else want_w.permute(0, 2, 3, 1).contiguous()
                               .view(torch.int32)), (channels_last, lead)
            # memory order too: the span as the bucket holds it
            assert torch.equal(
                wbuf[woff:woff + n],
                want_w.as_strided((n,), (1,)).view(torch.int32))
            assert torch.equal(db.view(torch.int32), want_b.view(torch.int32))
            assert _guards_intact(wbuf, woff, n), (channels_last, lead)
            assert _guards_intact(bbuf, boff, CO), (channels_last, lead)
            assert not bool((wbuf[woff:woff + n] == -(1 << 31)).any())
            assert not bool((bbuf[boff:boff + CO] == -(1 << 31)).any())


@pytest.mark.gpu
def test_finalize_single_destination_and_checks(geops):
    shape = (16, 3, 5, 5)
    idx, T16 = build_wrw_unpack_index(shape)
    idx = idx.to(DEV)
    full = torch.randn(T16, 16, device=DEV)
    # a summed slab that holds -0 (a sum of another kind could give one):
    # the stores are x + 0.0f, so the spans get +0 as `zeros += x` would
    full[0, :4] = -0.0
    full[T16 - 16, ::3] = -0.0
    assert int((full.view(torch.int32) == -(1 << 31)).sum()) == 10
    wbuf, woff = _span(1200, 1)
    dw = _view(wbuf, woff, shape, False)
    geops.conv5_wrw_finalize(full, idx, dw, None, 16, 3, T16)
    want = torch.zeros(shape, device=DEV)
    want += full.reshape(-1)[idx].reshape(shape)
    assert torch.equal(dw.view(torch.int32), want.view(torch.int32))
    assert int((dw == 0).sum()) == 4
    assert not bool((dw.view(torch.int32) == -(1 << 31)).any())
    assert _guards_intact(wbuf, woff, 1200)
    bbuf, boff = _span(16, 0)
    db = bbuf.view(torch.float32)[boff:boff + 16]
    geops.conv5_wrw_finalize(full, idx, None, db, 16, 3, T16)
    want = torch.zeros(16, device=DEV)
    want += full[T16 - 16]
    assert torch.equal(db.view(torch.int32), want.view(torch.int32))
    assert int((db == 0).sum()) == 6
    assert not bool((db.view(torch.int32) == -(1 << 31)).any())
    assert _guards_intact(bbuf, boff, 16)
    with pytest.raises(RuntimeError):
        geops.conv5_wrw_finalize(full, idx, None, None, 16, 3, T16)
    with pytest.raises(RuntimeError):   # a slab of another size
        geops.conv5_wrw_finalize(full[:-1].contiguous(), idx, dw, None, 16, 3,
                                 T16)
    with pytest.raises(RuntimeError):   # a destination of another shape
        geops.conv5_wrw_finalize(full, idx, dw[:, :2], None, 16, 3, T16)


# ---------------------------------------------------------------------
# the conv route under a trainer
# ---------------------------------------------------------------------

def _trainer(model, sinks):
    from geomx_amd import Config
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    from geomx_amd.parallel import GeoTrainer
    from geomx_amd.topology import init_topology
    cfg = Config.from_env()
    topo = init_topology(1, None, None, DEV)
    return GeoTrainer(model, cfg, topo,
                      OptimizerSpec("sgd_mom", lr=0.05, momentum=0.9),
                      grad_sinks=sinks)


def _train(sinks, steps):
    from geomx_amd.models import create_model
    torch.manual_seed(7)
    model = create_model("geomx_cnn", image_size=20).to(DEV) \
        .to(memory_format=torch.channels_last)
    tr = _trainer(model, sinks)
    assert len(tr.sinks) == (10 if sinks else 0)
    flats = []
    for s in range(steps):
        g = torch.Generator().manual_seed(100 + s)
        x = torch.randn(6, 3, 20, 20, generator=g).to(DEV) \
            .to(memory_format=torch.channels_last)
        y = torch.randint(0, 10, (6,), generator=g).to(DEV)
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(model(x), y)
        tr.zero_grad()
        loss.backward()
        for p in model.parameters():
            b, i = tr.param_bucket[p]
            assert p.grad is not None
            assert p.grad.data_ptr() == b.views[i].data_ptr()
            assert p.grad.stride() == b.views[i].stride()
        flats.append([b.flat.clone() for b in tr.buckets])
        tr.step()
    return flats, [p.detach().clone() for p in model.parameters()], tr


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 3])
def test_trainer_conv_sinks_bit_equal(geops, steps):
    fa, pa, tr = _train(True, steps)
    fb, pb, _ = _train(False, steps)
    # every parameter has a sink: nothing is left for zero_grad to fill
    assert all(not b.clear and not b.gaps for b in tr.buckets)
    for sa, sb in zip(fa, fb):
        for a, b in zip(sa, sb):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(pa, pb):
        assert a.stride() == b.stride()
        assert torch.equal(a.view(torch.int32) if a.is_contiguous()
                           else a.permute(0, 2, 3, 1).contiguous()
                           .view(torch.int32),
                           b.view(torch.int32) if b.is_contiguous()
                           else b.permute(0, 2, 3, 1).contiguous()
                           .view(torch.int32))
