"""The grayscale conv1 stage (conv1c.hip: k_conv5c1_pool, k_conv5c1_wrw)
against float64 oracles.

Inputs are small integers as in tests/conv_exact_cases.py (activations
and gradients in [-2, 2], weights in {-1, 0, 1}, integer bias): |conv| <=
53 < 256 and the largest wrw sum is 2*10*224*9 < 2^24, so every fp32 sum
is exact in any order and every check is torch.equal. Output buffers are
NaN (out between NaN guards) or a marker byte before the launch. One
random-valued case per kernel is held to the rounding bound instead."""

import pytest
import torch

import conv_exact_cases as X
import fwd_golden_cases as FG
import geomx_amd.ops as ops
from geomx_amd.ops import conv as C
from test_conv_exact_gpu import DEV, GUARD, NAN, _Guarded, _bits, _cached

G16 = X.G16
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
# H: one pooled row; 4 conv rows + a 2-row tail; full blocks. W: every
# lane clamps; one tile; a tile + 2 pixels; MNIST; the widest served row
FWD_CASES = ([(h, w, "int", 0) for h in (6, 10, 12)
              for w in (6, 20, 22, 28, 228)]
             + [(10, 22, "neg", 0), (10, 22, "none", 0)]
             + [(12, 22, "int", 1), (12, 22, "int", 2)])
# W 36: exactly one K window; 38: a window and a 2-pixel tail
WRW_CASES = [(h, w, g) for h in (6, 10) for w in (6, 28, 36, 38, 228)
             for g in (1, 3, 0)]


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _fwd_case(h, w, kind):
    def build():
        x, weight, bias = FG.exact_inputs(1, 16, h, w, kind)
        return (x.contiguous(), weight, bias) + FG.expected_exact(x, weight,
                                                                  bias)
    return _cached(("c1fwd", h, w, kind), build)


def _run_fwd(geops, x, weight, bias, h, w, n_wg):
    n = x.shape[0]
    frags, = geops.conv5_pack_frags(
        weight.to(DEV), C.build_c1_fwd_index(weight.shape).to(DEV))
    g = _Guarded(n, (h - 4) // 2, (w - 4) // 2, 16)
    mask = torch.full((g.out.numel() + 2 * GUARD,), 77, dtype=torch.uint8,
                      device=DEV)
    geops.conv5c1_pool(x.to(DEV), frags,
                       torch.Tensor() if bias is None else bias.to(DEV),
                       g.out, mask[GUARD:-GUARD], n, h, w, n_wg)
    m = mask.cpu()
    assert (m[:GUARD] == 77).all() and (m[-GUARD:] == 77).all()
    return g, m[GUARD:-GUARD]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("h,w,kind,n_wg", FWD_CASES)
def test_forward(geops, h, w, kind, n_wg, dtype):
    x, weight, bias, want, codes = _fwd_case(h, w, kind)
    g, m = _run_fwd(geops, x.to(dtype), weight, bias, h, w, n_wg)
    g.check(want.double())
    assert torch.equal(m.reshape(codes.shape), codes)


@pytest.mark.gpu
def test_width_past_the_row_image_raises(geops):
    x = torch.zeros(1, 1, 6, 230, device=DEV)
    frags = torch.zeros(1024, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(1, 1, 113, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        geops.conv5c1_pool(x, frags, torch.Tensor(), out,
                           torch.zeros(out.numel(), dtype=torch.uint8,
                                       device=DEV), 1, 6, 230, 0)
    go = torch.zeros(1, 2, 226, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        geops.conv5c1_wrw(x, go, torch.empty(1, 32, 16, device=DEV), 1, 6,
                          230, 0)


def _wrw_case(h, w):
    """x, the pooled gradient on the forward's own codes (255 included),
    its scatter, and the float64 (dW, db)."""
    def build():
        x, _, _, _, codes = _fwd_case(h, w, "int")
        assert (codes == 255).any() and (codes < 4).any()
        gen = torch.Generator().manual_seed(31000 + 1000 * h + w)
        gp = torch.randint(-2, 3, codes.shape, generator=gen) \
            .to(torch.bfloat16)
        go = G16._scatter(gp, codes)
        dw, db = X.wgrad_oracle(x.permute(0, 2, 3, 1), go, 1)
        return x, gp, codes.reshape(-1).contiguous(), go, dw, db
    return _cached(("c1wrw", h, w), build)


def _run_wrw(geops, x, go, gp, mask, h, w, n_wg, pooled):
    n = x.shape[0]
    slabs = n_wg or min(768, n * ((h - 4 + 1) // 2))
    part = torch.full((slabs, 32, 16), NAN, device=DEV)
    if pooled:
        geops.conv5c1_wrw_unpool(x, gp.to(DEV), mask.to(DEV), part, n, h, w,
                                 n_wg)
    else:
        geops.conv5c1_wrw(x, go.to(DEV), part, n, h, w, n_wg)
    return part.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "full"])
@pytest.mark.parametrize("h,w,n_wg", WRW_CASES)
def test_wrw_slabs(geops, h, w, n_wg, pooled, dtype):
    x, gp, mask, go, dw, db = _wrw_case(h, w)
    xg = x.to(DEV, dtype)
    part = _run_wrw(geops, xg, go, gp, mask, h, w, n_wg, pooled)
    assert not torch.isnan(part).any()
    assert (part[:, 26:] == 0).all()
    full = part.sum(0)
    assert torch.equal(full[:25].T.reshape(16, 1, 5, 5), dw.float())
    assert torch.equal(full[25], db.float())
    again = _run_wrw(geops, xg, go, gp, mask, h, w, n_wg, pooled)
    assert torch.equal(part.view(torch.int32), again.view(torch.int32))


def _module(cls, x, weight, bias, go):
    m = cls(weight.shape[1], 16)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    m = m.to(DEV)
    xg = x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
    plan = tuple(m._route(xg)[0])
    y = m(xg)
    y.backward(go.to(DEV).permute(0, 3, 1, 2))
    return m, plan, y


@pytest.mark.gpu
@pytest.mark.parametrize("pooled,w", [(True, 28), (True, 38), (False, 38)])
def test_modules(geops, pooled, w):
    x, weight, bias, go = X.module_inputs(1, 16, w, pooled)
    y64, _, dw64, db64 = X.module_oracle(x, weight, bias, go, pooled)
    m, plan, y = _module(C.GeoConv5Pool if pooled else C.GeoConv5, x, weight,
                         bias, go)
    assert plan == (("pool1" if pooled else "aten"), "aten", "wrw1")
    if pooled:
        assert torch.equal(_bits(y), _bits(X.to_bf16(y64).permute(0, 3, 1, 2)))
    assert torch.equal(m.weight.grad.cpu(), dw64.float())
    assert torch.equal(m.bias.grad.cpu(), db64.float())


@pytest.mark.gpu
def test_two_channel_stage_runs(geops):
    x, weight, bias, go = X.module_inputs(2, 16, 28, True)
    m, _, y = _module(C.GeoConv5Pool, x, weight, bias, go)
    assert torch.isfinite(y.float()).all()
    assert torch.isfinite(m.weight.grad).all()


@pytest.mark.gpu
def test_mnist_shaped_cnn_trains_a_step(geops):
    from geomx_amd.models import geo_cnn
    torch.manual_seed(0)
    net = geo_cnn(in_channels=1, image_size=28).to(DEV)
    x = torch.randn(4, 1, 28, 28, device=DEV)
    assert tuple(net.features[0]._route(x)[0]) == ("pool1", "aten", "wrw1")
    net(x).float().square().mean().backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


@pytest.mark.gpu
def test_random_values_within_the_rounding_bound(geops):
    """Random normals at H = 10, W = 28 against float64 on the bf16-
    rounded operands: out within 2^-8 |ref| + 25 * 2^-23 (|x| * |w|)
    (the largest of a window for a pooled pixel), dW and db within
    n_terms * 2^-23 (|x| * |g|). The mask is not compared: near-ties may
    legitimately differ from float64."""
    h, w, n = 10, 28, 2
    gen = torch.Generator().manual_seed(515)
    x = torch.randn(n, 1, h, w, generator=gen)
    weight = (torch.randn(16, 1, 5, 5, generator=gen) * 0.2) \
        .to(torch.bfloat16).float()
    bias = torch.randn(16, generator=gen) * 0.5
    xb = x.to(torch.bfloat16).permute(0, 2, 3, 1)

    def pool(t):
        return torch.stack([t[:, dy::2, dx::2] for dy in range(2)
                            for dx in range(2)]).max(0).values

    ref = pool(X.conv_oracle(xb, weight, bias)).clamp(min=0)
    bound = 2.0 ** -8 * ref.abs() + 25 * 2.0 ** -23 * pool(
        X.conv_oracle(xb.abs(), weight.abs()))
    g, _ = _run_fwd(geops, x, weight, bias, h, w, 0)
    err = (g.out.cpu().double() - ref).abs()
    print("fwd max err / bound", (err / bound).max().item())
    assert (err <= bound).all()

    gp = torch.randn(n, 3, 12, 16, generator=gen).to(torch.bfloat16)
    mask = G16._codes(gen, gp.shape)
    go = G16._scatter(gp, mask)
    dw, db = X.wgrad_oracle(xb, go, 1)
    bw, bb = X.wgrad_oracle(xb.abs(), go.abs(), 1)
    part = _run_wrw(geops, x.to(DEV), go, gp, mask.reshape(-1), h, w, 0, True)
    full = part.sum(0).double()
    terms = n * 6 * 24 * 2.0 ** -23
    print("wrw max err / bound",
          ((full[:25].T.reshape(16, 1, 5, 5) - dw).abs() / (terms * bw)).max()
          .item(), ((full[25] - db).abs() / (terms * bb)).max().item())
    assert ((full[:25].T.reshape(16, 1, 5, 5) - dw).abs() <= terms * bw).all()
    assert ((full[25] - db).abs() <= terms * bb).all()
