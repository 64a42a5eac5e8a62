"""conv2 data gradient: the row-sliding LDS kernel against the direct kernel.

k_conv5_lds_nhwc<32, 1, ...> walks the staged rows of a (16-pixel tile,
4 output rows) unit once and keeps the weight fragments in registers. Each
accumulator still receives the 25 MFMAs of k_conv5_nhwc<32, 1> in the same
order with the same fragments, so every comparison is torch.equal on the
int16 view against that kernel run on the scattered, physically padded
gradient (conv5_direct_nhwc): no tolerance.

ROWS = 4, so the dgrad output heights are 6 (one group + a 2-row tail),
8 (two groups) and 10 (two groups + tail); widths cover a partial tile,
7 full tiles (the widest 120-pixel row), the flagship 110, the first row
that needs the 232-pixel variant and the widest it serves."""

import pytest
import torch
import torch.nn.functional as F

import geomx_amd.ops as ops
from geomx_amd.ops import conv as C

DEV = "cuda:0"
N, CO, CIR = 2, 32, 16          # gradient channels -> dgrad output channels

SHAPES = [(6, 26), (8, 26), (10, 20), (8, 112), (8, 110), (8, 116),
          (8, 224)]
PERSISTENT = [(10, 26), (8, 110)]
PAD0 = [(8, 26), (8, 110)]


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _pooled_grad(hp, wp, seed):
    """Random pooled gradient (NHWC memory) and codes from {0,1,2,3,255};
    a few pooled pixels are all-255 and a few route every channel to one
    quadrant."""
    g = torch.Generator().manual_seed(seed)
    gp = torch.randn(N, hp, wp, CO, generator=g).to(torch.bfloat16)
    codes = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8)
    mask = codes[torch.randint(0, 5, (N, hp, wp, CO), generator=g)]
    mask[0, 0, 0] = 255
    mask[1, hp - 1, wp - 1] = 255
    mask[0, hp - 1, wp // 2] = 255
    for quad in range(4):
        mask[quad % N, quad % hp, (1 + 2 * quad) % wp] = quad
    return (gp.to(DEV).permute(0, 3, 1, 2),
            mask.to(DEV).reshape(-1).contiguous())


_CASES = {}


def _case(geops, H, W):
    """Inputs and the direct-kernel oracle of one (H, W), built once."""
    if (H, W) in _CASES:
        return _CASES[(H, W)]
    ho, wo = H - 4, W - 4
    seed = H * 1000 + W
    torch.manual_seed(seed)
    weight = torch.randn(CO, CIR, 5, 5, device=DEV) * 0.1
    w_frags = C._w_frags(weight, C.build_dgrad_index(weight.shape).to(DEV))
    gp, mask = _pooled_grad(ho // 2, wo // 2, seed)
    go = torch.empty(N, CO, ho, wo, dtype=torch.bfloat16, device=DEV,
                     memory_format=torch.channels_last)
    geops.relu_maxpool2_bwd(gp, mask, go, N, CO, ho, wo)
    gop = F.pad(go, (4, 4, 4, 4)).contiguous(
        memory_format=torch.channels_last)
    ref = _nan_out(H, W)
    geops.conv5_direct_nhwc(gop, w_frags, ref, N, H + 4, W + 4, H, W, CO,
                            CIR)
    assert torch.isfinite(ref.float()).all()
    assert ref.float().abs().sum().item() > 0
    _CASES[(H, W)] = dict(gp=gp, mask=mask, go=go, gop=gop, w_frags=w_frags,
                          ref=ref.view(torch.int16))
    return _CASES[(H, W)]


def _nan_out(H, W):
    return torch.full((N, CIR, H, W), float("nan"), dtype=torch.bfloat16,
                      device=DEV).contiguous(
                          memory_format=torch.channels_last)


def _run(geops, c, H, W, form, n_wg=None):
    got = _nan_out(H, W)
    dims = (N, H + 4, W + 4, H, W, CO, CIR)
    if form == "pooled":
        if n_wg is None:
            geops.conv5_dgrad_unpool_nhwc(c["gp"], c["mask"], c["w_frags"],
                                          got, *dims)
        else:
            geops.conv5_dgrad_nwg_nhwc(c["gp"], c["mask"], c["w_frags"], got,
                                       *dims, n_wg)
    elif form == "pad4":
        if n_wg is None:
            geops.conv5_nhwc(c["go"], c["w_frags"], torch.Tensor(), got,
                             *dims, 4)
        else:
            geops.conv5_dgrad_nwg_nhwc(c["go"], torch.Tensor(), c["w_frags"],
                                       got, *dims, n_wg)
    else:
        geops.conv5_nhwc(c["gop"], c["w_frags"], torch.Tensor(), got, *dims,
                         0)
    return got.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pooled", "pad4"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_rows_kernel_equals_direct(geops, H, W, form):
    c = _case(geops, H, W)
    assert torch.equal(_run(geops, c, H, W, form), c["ref"])


# N * ceil(H/4) = 6 (H=10) or 4 (H=8) blocks: n_wg 1 and 2 run several
# blocks per workgroup, restaging LDS (a stale row would show) and, in the
# pooled form, prefetching the next block while this one computes (a
# prefetch of the wrong block would show)
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pooled", "pad4"])
@pytest.mark.parametrize("n_wg", [1, 2, None])
@pytest.mark.parametrize("H,W", PERSISTENT)
def test_persistent_loop_equals_direct(geops, H, W, n_wg, form):
    c = _case(geops, H, W)
    assert torch.equal(_run(geops, c, H, W, form, n_wg), c["ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", PAD0)
def test_pad0_lds_equals_direct(geops, H, W):
    c = _case(geops, H, W)
    assert torch.equal(_run(geops, c, H, W, "pad0"), c["ref"])


@pytest.mark.gpu
def test_hook_bindings_reject_bad_geometry(geops):
    wf = torch.zeros(25 * 64 * 8, device=DEV, dtype=torch.bfloat16)

    def bf(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.bfloat16)

    # pooled form, odd full-resolution sizes (H = 9)
    gp = bf(N, 2, 8, CO)
    mask = torch.zeros(gp.numel(), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        geops.conv5_dgrad_nwg_nhwc(gp, mask, wf, bf(N, 9, 20, CIR), N, 13,
                                   24, 9, 20, CO, CIR, 1)
    # both forms, a row wider than the 232-pixel table (W = 232 -> 236)
    gp = bf(N, 2, 114, CO)
    mask = torch.zeros(gp.numel(), dtype=torch.uint8, device=DEV)
    out = bf(N, 8, 232, CIR)
    with pytest.raises(RuntimeError):
        geops.conv5_dgrad_nwg_nhwc(gp, mask, wf, out, N, 12, 236, 8, 232,
                                   CO, CIR, 1)
    with pytest.raises(RuntimeError):
        geops.conv5_dgrad_nwg_nhwc(bf(N, 4, 228, CO), torch.Tensor(), wf,
                                   out, N, 12, 236, 8, 232, CO, CIR, 1)
    # n_wg must be positive
    with pytest.raises(RuntimeError):
        geops.conv5_dgrad_nwg_nhwc(bf(N, 4, 16, CO), torch.Tensor(), wf,
                                   bf(N, 8, 20, CIR), N, 12, 24, 8, 20, CO,
                                   CIR, 0)
    # the direct oracle serves 32 -> 16 on an input padded by exactly 4
    with pytest.raises(RuntimeError):
        geops.conv5_direct_nhwc(bf(N, 12, 25, CO), wf, bf(N, 8, 20, CIR), N,
                                12, 25, 8, 20, CO, CIR)
    with pytest.raises(RuntimeError):
        geops.conv5_direct_nhwc(bf(N, 12, 24, 16), wf, bf(N, 8, 20, CIR), N,
                                12, 24, 8, 20, 16, CIR)
