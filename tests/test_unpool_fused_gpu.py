"""Max-pool backward fused into the conv weight/data-gradient kernels.

The fused kernels build the same LDS gout image the scatter kernel
(relu_maxpool2_bwd) would have produced in HBM and reorder no
arithmetic, so every comparison is torch.equal against the unfused
chain with the same n_wg: no tolerance."""

import pytest
import torch

import geomx_amd.ops as ops
from geomx_amd.ops import conv as C

DEV = "cuda:0"
N = 2


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _pooled_grad(co, hp, wp, seed):
    """Random pooled gradient [N][co][hp][wp] (NHWC memory) and codes
    from {0,1,2,3,255}; a few pooled pixels are all-255 and a few route
    every channel to one quadrant."""
    g = torch.Generator().manual_seed(seed)
    gp = torch.randn(N, hp, wp, co, generator=g).to(torch.bfloat16)
    codes = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8)
    mask = codes[torch.randint(0, 5, (N, hp, wp, co), generator=g)]
    mask[0, 0, 0] = 255
    mask[1, hp - 1, wp - 1] = 255
    mask[0, hp - 1, wp // 2] = 255
    for quad in range(4):
        mask[quad % N, quad % hp, (1 + 2 * quad) % wp] = quad
    return (gp.to(DEV).permute(0, 3, 1, 2),
            mask.to(DEV).reshape(-1).contiguous())


def _scatter(geops, gp, mask, co, ho, wo):
    go = torch.empty(N, co, ho, wo, dtype=torch.bfloat16, device=DEV,
                     memory_format=torch.channels_last)
    geops.relu_maxpool2_bwd(gp, mask, go, N, co, ho, wo)
    return go


def _check_wrw(geops, ci, co, H, W, n_wg, seed):
    ho, wo = H - 4, W - 4
    torch.manual_seed(seed)
    x = torch.randn(N, ci, H, W, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    gp, mask = _pooled_grad(co, ho // 2, wo // 2, seed)
    t16 = 176 if ci == 4 else 416
    ref = torch.zeros(n_wg, t16, co, dtype=torch.float32, device=DEV)
    geops.conv5_wrw_nhwc(x, _scatter(geops, gp, mask, co, ho, wo), ref, N,
                         H, W, ho, wo, ci, co, n_wg)
    got = torch.zeros_like(ref)
    geops.conv5_wrw_unpool_nhwc(x, gp, mask, got, N, H, W, ho, wo, ci, co,
                                n_wg)
    assert ref.abs().sum().item() > 0
    # whole slabs: every tap tile and the fused-bias tile (last 16 rows)
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    assert torch.equal(got[:, t16 - 16], ref[:, t16 - 16])


# N * Ho/2 = 4 row blocks: n_wg 4 stages LDS once per workgroup, n_wg 3
# and 1 restage it (a tail left over from the previous block would show)
@pytest.mark.gpu
@pytest.mark.parametrize("W,n_wg", [(26, 4), (40, 4), (138, 4), (228, 4),
                                    (40, 3), (228, 3), (26, 1)])
def test_wrw4_unpool_bit_equal(geops, W, n_wg):
    _check_wrw(geops, 4, 16, 8, W, n_wg, seed=W)


@pytest.mark.gpu
@pytest.mark.parametrize("co,W,n_wg", [(32, 20, 4), (32, 26, 4),
                                       (32, 116, 4), (16, 20, 4),
                                       (32, 26, 3), (32, 116, 1),
                                       (16, 228, 3), (32, 228, 3)])
def test_wrw16_unpool_bit_equal(geops, co, W, n_wg):
    _check_wrw(geops, 16, co, 8, W, n_wg, seed=100 + W)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 26), (8, 116), (10, 26), (8, 224)])
def test_dgrad_unpool_bit_equal(geops, H, W):
    co, cir = 32, 16
    ho, wo = H - 4, W - 4
    torch.manual_seed(H * 1000 + W)
    weight = torch.randn(co, cir, 5, 5, device=DEV) * 0.1
    idx = C.build_dgrad_index(weight.shape).to(DEV)
    w_frags = C._w_frags(weight, idx)
    gp, mask = _pooled_grad(co, ho // 2, wo // 2, H * 1000 + W)
    ref = torch.empty(N, cir, H, W, dtype=torch.bfloat16, device=DEV,
                      memory_format=torch.channels_last)
    geops.conv5_nhwc(_scatter(geops, gp, mask, co, ho, wo), w_frags,
                     torch.Tensor(), ref, N, ho + 8, wo + 8, H, W, co, cir,
                     4)
    got = torch.full_like(ref, float("nan"))
    geops.conv5_dgrad_unpool_nhwc(gp, mask, w_frags, got, N, ho + 8, wo + 8,
                                  H, W, co, cir)
    assert ref.float().abs().sum().item() > 0
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.gpu
def test_unpool_bindings_reject_odd_sizes(geops):
    x = torch.zeros(N, 16, 9, 20, device=DEV, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    gp = torch.zeros(N, 2, 8, 32, device=DEV,
                     dtype=torch.bfloat16).permute(0, 3, 1, 2)
    mask = torch.zeros(gp.numel(), dtype=torch.uint8, device=DEV)
    part = torch.zeros(4, 416, 32, device=DEV)
    with pytest.raises(RuntimeError):
        geops.conv5_wrw_unpool_nhwc(x, gp, mask, part, N, 9, 20, 5, 16, 16,
                                    32, 4)
    out = torch.zeros(N, 16, 9, 20, device=DEV, dtype=torch.bfloat16)
    wf = torch.zeros(25 * 64 * 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        geops.conv5_dgrad_unpool_nhwc(gp, mask, wf, out, N, 13, 24, 9, 20,
                                      32, 16)


def _module_grads(mod, x, r):
    mod.zero_grad()
    x.grad = None
    (mod(x).float() * r).sum().backward()
    return (mod.weight.grad.clone(), mod.bias.grad.clone(), x.grad.clone())


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,W,scatters", [(16, 32, 116, 0),
                                                 (3, 16, 228, 1)])
def test_module_grads_equal_unfused(geops, monkeypatch, cin, cout, W,
                                    scatters):
    """(16,32): wrw16 + lds_pad4 both take the pooled form, the scatter
    kernel never runs. (3,16) with x.requires_grad: wrw4 takes it while
    the direct_padded dgrad forces the full-resolution tensor, once."""
    torch.manual_seed(5)
    mod = C.GeoConv5Pool(cin, cout).to(DEV)
    x = torch.randn(N, cin, 8, W, device=DEV, requires_grad=True)
    plan, _ = mod._route(x)
    assert plan.fwd == "pool"
    fuse = C.unpool_fusable(plan)
    assert fuse == ((True, True) if cin == 16 else (False, True))
    r = torch.randn(N, cout, 2, (W - 4) // 2, device=DEV)

    calls = []
    real = geops.relu_maxpool2_bwd
    monkeypatch.setattr(geops, "relu_maxpool2_bwd",
                        lambda *a: (calls.append(1), real(*a))[1])
    got = _module_grads(mod, x, r)
    assert len(calls) == scatters
    monkeypatch.setattr(C, "unpool_fusable",
                        lambda plan: C.Conv5Unpool(False, False))
    ref = _module_grads(mod, x, r)
    assert len(calls) == scatters + 1
    for a, b in zip(got, ref):
        assert a.abs().sum().item() > 0
        assert torch.equal(a, b)


def test_unpool_routing_cpu():
    """The predicate, and the full-resolution gradient being built only
    when a needed consumer cannot take the pooled form (stubs, no
    device)."""
    P = C.Conv5Plan
    assert C.unpool_fusable(P("pool", "lds_pad4", "wrw16")) == (True, True)
    assert C.unpool_fusable(P("pool", "direct_padded", "wrw4")) == \
        (False, True)
    assert C.unpool_fusable(P("pool", "aten", "aten")) == (False, False)
    assert C.unpool_fusable(P("pool", "lds_pad4", "aten")) == (True, False)
    # the flagship stages
    assert C.unpool_fusable(C.plan_conv5((16, 3, 5, 5), 224, 224, True)) \
        == (False, True)
    assert C.unpool_fusable(C.plan_conv5((32, 16, 5, 5), 110, 110, True)) \
        == (True, True)

    def run(fuse, need_x, need_w):
        log = []

        def scatter():
            log.append("scatter")
            return "full"

        def dgrad(g, m):
            log.append(("dgrad", g, m))
            return "gx"

        def wrw(g, m):
            log.append(("wrw", g, m))
            return ("gw", "gb")

        out = C._pooled_backward(C.Conv5Unpool(*fuse), need_x, need_w, "gp",
                                 "mask", scatter, dgrad, wrw)
        return out, log

    # everything fused: no scatter, consumers see (gp, mask)
    out, log = run((True, True), True, True)
    assert out == ("gx", ("gw", "gb"))
    assert log == [("dgrad", "gp", "mask"), ("wrw", "gp", "mask")]
    # conv1 on the flagship: dgrad not fusable but not needed either
    out, log = run((False, True), False, True)
    assert out == (None, ("gw", "gb"))
    assert log == [("wrw", "gp", "mask")]
    # mixed: the unfusable dgrad forces the scatter, wrw stays pooled
    out, log = run((False, True), True, True)
    assert log == ["scatter", ("dgrad", "full", None),
                   ("wrw", "gp", "mask")]
    # nothing fused: ONE scatter shared by both consumers
    out, log = run((False, False), True, True)
    assert log == ["scatter", ("dgrad", "full", None),
                   ("wrw", "full", None)]
    # fusable dgrad, unfusable wrw that is not needed: no scatter
    out, log = run((True, False), True, False)
    assert out == ("gx", None)
    assert log == [("dgrad", "gp", "mask")]
    # nothing needed
    assert run((False, False), False, False) == ((None, None), [])
