"""CPU tests of the conv5 route plan and its index cache (no extension,
no tensors on a GPU): the plan is a pure function of geometry."""

import pytest
import torch

from geomx_amd.ops import conv as C

CONV1 = (16, 3, 5, 5)
CONV2 = (32, 16, 5, 5)
ALL_FWD = frozenset(C._SUPPORTED_FWD)

# (weight shape, H, W, pooled, enabled_shapes) -> (fwd, dgrad, wrw)
PLAN_TABLE = [
    # flagship stages
    (CONV1, 224, 224, True, None, ("pool", "direct_padded", "wrw4")),
    (CONV2, 110, 110, True, None, ("pool", "lds_pad4", "wrw16")),
    # wrw4 needs an even Wi
    (CONV1, 8, 35, False, None, ("direct", "direct_padded", "aten")),
    (CONV1, 8, 36, False, None, ("direct", "direct_padded", "wrw4")),
    # pool16 stages 120 pixels: ceil16(Wo)+4 <= 120
    (CONV2, 8, 116, True, None, ("pool", "lds_pad4", "wrw16")),
    (CONV2, 8, 118, True, None, ("aten", "lds_pad4", "wrw16")),
    # lds_pad4 stages 232 pixels: ceil16(Wi)+4 <= 232
    (CONV2, 8, 224, False, ALL_FWD, ("direct", "lds_pad4", "wrw16")),
    (CONV2, 8, 226, False, ALL_FWD, ("direct", "direct_padded", "wrw16")),
    # wrw stages 232 pixels: ceil32(Wo)+4 <= 232; the CI=4 pool forward
    # has a register-only kernel beyond its LDS variant
    (CONV1, 8, 228, True, None, ("pool", "direct_padded", "wrw4")),
    (CONV1, 8, 230, True, None, ("pool", "direct_padded", "aten")),
    (CONV2, 8, 228, False, None, ("aten", "direct_padded", "wrw16")),
    (CONV2, 8, 230, False, None, ("aten", "direct_padded", "aten")),
    # pooling needs even Ho; a pooled stage never takes the direct kernel
    (CONV1, 9, 36, True, None, ("aten", "direct_padded", "wrw4")),
    (CONV1, 9, 36, False, None, ("direct", "direct_padded", "wrw4")),
    # 16 -> 16: pooled forward, dgrad on the direct kernel
    ((16, 16, 5, 5), 8, 20, True, None, ("pool", "direct_padded", "wrw16")),
    # forward-only shape, and a shape outside every set
    ((32, 32, 5, 5), 8, 20, False, ALL_FWD, ("direct", "aten", "aten")),
    ((64, 32, 5, 5), 8, 20, True, ALL_FWD, ("aten", "aten", "aten")),
]


@pytest.mark.parametrize("ws,H,W,pooled,enabled,expect", PLAN_TABLE)
def test_plan_table(ws, H, W, pooled, enabled, expect):
    kw = {} if enabled is None else {"enabled_shapes": enabled}
    assert tuple(C.plan_conv5(ws, H, W, pooled, **kw)) == expect


@pytest.mark.parametrize("ws,H,W,pooled,enabled,expect", PLAN_TABLE[:2])
def test_plan_without_native_is_all_aten(ws, H, W, pooled, enabled, expect):
    assert tuple(C.plan_conv5(ws, H, W, pooled, native=False)) == \
        ("aten", "aten", "aten")


def test_module_routes_cpu_input_to_aten():
    m = C.GeoConv5Pool(3, 16)
    plan, idx = m._route(torch.zeros(1, 3, 36, 36))
    assert tuple(plan) == ("aten", "aten", "aten") and idx is None
    # a conv the kernels do not implement never takes a custom route
    m = C.GeoConv5(16, 32, stride=2)
    assert m(torch.zeros(1, 16, 9, 9)).shape == (1, 32, 3, 3)


def test_wrw_unpack_index_layouts():
    idx, t16 = C.build_wrw_unpack_index(CONV1)
    assert t16 == 176 and idx.numel() == 16 * 3 * 25
    assert len(set(idx.tolist())) == idx.numel() and int(idx.max()) < 160 * 16
    # weight[o=5][ci=2][kh=4][kw=3] -> slot (3*2+1)*16 + 0*4 + 2
    assert int(idx.reshape(CONV1)[5, 2, 4, 3]) == (7 * 16 + 2) * 16 + 5
    idx, t16 = C.build_wrw_unpack_index(CONV2)
    assert t16 == 416 and idx.numel() == 32 * 16 * 25
    assert len(set(idx.tolist())) == idx.numel() and int(idx.max()) < 400 * 32
    assert int(idx.reshape(CONV2)[7, 9, 2, 1]) == ((2 * 5 + 1) * 16 + 9) * 32 + 7


@pytest.mark.parametrize("ws", [(16, 8, 5, 5), (32, 32, 5, 5), (8, 3, 5, 5)])
def test_wrw_unpack_index_rejects_unserved_shape(ws):
    with pytest.raises(ValueError):
        C.build_wrw_unpack_index(ws)


def test_index_cache_shared_between_modules():
    a, b = C.GeoConv5Pool(3, 16), C.GeoConv5(3, 16)
    ia = C._conv5_indices(a.weight.shape, "cpu")
    ib = C._conv5_indices(b.weight.shape, torch.device("cpu"))
    assert ia is ib
    assert ia.fwd is ib.fwd and ia.dgrad is ib.dgrad and ia.wrw is ib.wrw
    assert torch.equal(ia.fwd, C.build_fwd_index(CONV1))
    assert torch.equal(ia.dgrad, C.build_dgrad_index(CONV1))
    assert torch.equal(ia.wrw, C.build_wrw_unpack_index(CONV1)[0])
    assert ia.t16 == 176
    # forward-only shape: no wrw kernel, no wrw index
    assert C._conv5_indices((32, 32, 5, 5), "cpu").wrw is None
