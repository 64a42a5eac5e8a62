"""NHWC-native backward of the first dense layer (csrc/fc.hip,
ops/fc.py).

Every shape is (N, C, H, W, O). Inputs are exactly representable in
bf16. The permute kernels only move and convert values: torch.equal, no
tolerance; neither does the flatten kernel. The module's forward is the
eager head's own math on the same operands: torch.equal. Its gradients are compared with the eager head's under

    |g - ref| <= 2^-8 |ref| + K 2^-23 (|a| . |b|^T)

The first term is the bf16 rounding of a GEMM output (unit roundoff
2^-9) with a 2x margin; the second is the standard bound on an fp32
accumulation of K products in any order (K 2^-24 sum|a_k b_k|) with a
2x margin. K is the reduction length: O for the data gradient, N for
the weight and bias gradients.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import geomx_amd.ops as ops
from geomx_amd.ops import fc as FC

DEV = "cuda:0"

SMALL = (3, 32, 5, 5, 16)      # HW < one 128-pixel permute tile
MID = (17, 32, 7, 11, 256)     # odd HW, O at the workload's size
WORK = (8, 32, 53, 53, 256)    # the workload's own HW: 21 full tiles + 121


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _bf16_exact(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)
    return t.float().to(DEV)


def _bucket_view(t):
    """`t` as a view at a 256 B-aligned, otherwise arbitrary offset of a
    larger fp32 buffer (what GeoTrainer's bucket views look like)."""
    off = 3 * 64  # elements: 768 B
    buf = torch.zeros(off + t.numel() + 64, device=t.device, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == 0
    return v


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands of a shape, built once."""
    N, C, H, W, O = shape
    x = _bf16_exact(N, C, H, W, seed=N + H).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = _bucket_view(_bf16_exact(O, C * H * W, seed=O + W,
                                 scale=(C * H * W) ** -0.5))
    b = _bf16_exact(O, seed=7)
    return x, w, b


def _bound(ref, mag, K):
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag


def _check(name, got, ref, mag, K):
    err = (got.double() - ref).abs()
    bound = _bound(ref, mag, K)
    print("%s: max err %.3e, max err/bound %.3f"
          % (name, err.max().item(), (err / bound).max().item()))
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (name, (err / bound).max().item())


# ---------------------------------------------------------------------
# permute / unpermute
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SMALL, MID, WORK])
def test_permute_unpermute_exact(geops, shape):
    _, C, H, W, O = shape
    HW = H * W
    g = torch.Generator().manual_seed(HW)
    w = _bucket_view(torch.randn(O, C * HW, generator=g).to(DEV))
    want = w.to(torch.bfloat16).view(O, C, HW).transpose(1, 2) \
        .reshape(O, HW * C)
    wp = geops.fc_w_permute_bf16(w, O, C, HW)
    assert wp.dtype == torch.bfloat16 and wp.shape == (O, HW * C)
    assert torch.equal(wp, want)

    gp = torch.randn(O, HW * C, generator=g).to(torch.bfloat16).to(DEV)
    want32 = gp.view(O, HW, C).transpose(1, 2).reshape(O, C * HW).float()
    g32 = geops.fc_w_unpermute_f32(gp, O, C, HW)
    assert g32.dtype == torch.float32 and g32.shape == (O, C * HW)
    assert torch.equal(g32, want32)
    # and the two are inverses of each other
    assert torch.equal(geops.fc_w_unpermute_f32(wp, O, C, HW),
                       w.to(torch.bfloat16).float())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SMALL, MID, WORK, (2, 32, 16, 16, 16)])
def test_flatten_nchw_exact(geops, shape):
    """Odd HW puts every other output row on an odd 2 B parity; the
    last shape has even HW and two full tiles."""
    N, C, H, W, _ = shape
    x = _bf16_exact(N, C, H, W, seed=H * W).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    xf = x.permute(0, 2, 3, 1).reshape(N, H * W * C)
    got = geops.fc_flatten_nchw(xf, N, C, H * W)
    assert got.dtype == torch.bfloat16 and got.shape == (N, C * H * W)
    assert torch.equal(got, torch.flatten(x, 1))


# ---------------------------------------------------------------------
# module: forward and the three gradients against eager Flatten+Linear
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SMALL, MID, WORK])
def test_module_matches_eager(geops, shape):
    N, C, H, W, O = shape
    x0, w, b = _case(shape)
    dy = _bf16_exact(N, O, seed=11).to(torch.bfloat16)

    mod = FC.GeoFlattenLinear(C * H * W, O).to(DEV)
    eager = torch.nn.Sequential(torch.nn.Flatten(),
                                torch.nn.Linear(C * H * W, O)).to(DEV)
    with torch.no_grad():
        for lin in (mod, eager[1]):
            lin.weight.copy_(w)
            lin.bias.copy_(b)

    out = []
    for net in (mod, eager):
        x = x0.clone().requires_grad_(True)
        assert x.is_contiguous(memory_format=torch.channels_last)
        with torch.autocast("cuda", torch.bfloat16):
            if net is mod:
                assert FC.native_route(x, mod.weight)
            y = net(x)
        y.backward(dy)
        lin = mod if net is mod else eager[1]
        out.append((y.detach(), x.grad, lin.weight.grad, lin.bias.grad))
    (y, gx, gw, gb), (ye, gxe, gwe, gbe) = out

    assert y.dtype == ye.dtype == torch.bfloat16
    assert gx.dtype == gxe.dtype and gx.shape == gxe.shape
    assert gx.is_contiguous(memory_format=torch.channels_last)
    assert gw.dtype == torch.float32 and gw.shape == (O, C * H * W)
    assert gb.dtype == torch.float32 and gb.shape == (O,)

    xd = torch.flatten(x0, 1).double()
    dyd, wd = dy.double(), w.double()
    assert torch.equal(y, ye)  # the same casts and the same GEMM
    _check("module x.grad", torch.flatten(gx, 1),
           torch.flatten(gxe, 1).double(), dyd.abs() @ wd.abs(), O)
    _check("module weight.grad", gw, gwe.double(), dyd.abs().t() @ xd.abs(),
           N)
    _check("module bias.grad", gb, gbe.double(), dyd.abs().sum(0), N)


# ---------------------------------------------------------------------
# everything else is today's math, bit for bit
# ---------------------------------------------------------------------

def _eager(mod, x):
    return F.linear(torch.flatten(x, 1), mod.weight, mod.bias)


@pytest.mark.gpu
def test_fallback_fp32_without_autocast(geops):
    N, C, H, W, O = MID
    x = _case(MID)[0].float()
    mod = FC.GeoFlattenLinear(C * H * W, O).to(DEV)
    assert not FC.native_route(x, mod.weight)
    assert torch.equal(mod(x), _eager(mod, x))


@pytest.mark.gpu
def test_fallback_nchw_dense_input(geops):
    N, C, H, W, O = MID
    x = _case(MID)[0].contiguous()
    assert not x.is_contiguous(memory_format=torch.channels_last)
    mod = FC.GeoFlattenLinear(C * H * W, O).to(DEV)
    with torch.autocast("cuda", torch.bfloat16):
        assert not FC.native_route(x, mod.weight)
        assert torch.equal(mod(x), _eager(mod, x))


@pytest.mark.gpu
@pytest.mark.parametrize("C,O", [(16, 256), (64, 16)])
def test_fallback_outside_kernel_table(geops, C, O):
    N, H, W = 5, 7, 11
    x = _bf16_exact(N, C, H, W, seed=C + O).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    mod = FC.GeoFlattenLinear(C * H * W, O).to(DEV)
    with torch.autocast("cuda", torch.bfloat16):
        assert not FC.native_route(x, mod.weight)
        assert torch.equal(mod(x), _eager(mod, x))
