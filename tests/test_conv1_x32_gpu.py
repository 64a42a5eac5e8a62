"""The conv1 forward from the caller's fp32 image (k_conv5_pool2_nhwc<232,
float>, binding conv5_pool_x32_nhwc) against the route it replaces on the
same build: pad_ch3to4_nhwc, then conv5_pool_nhwc on the padded bf16 copy.
Every comparison is torch.equal on integer views.

Kernel level: Hi = 6, 10, 12 (1, 3 and 4 pooled rows: a lone tail block,
a block plus a tail, two blocks), N = 3 (the persistent loop crosses
image boundaries), n_wg = 1, 2 and the default grid through the hook.
Widths 20 (one tile), 28 (clamped tail tile), 224 (flagship) and 228.
228 is the widest row the kernel's launch table admits: a row needs
ceil16(Wi - 4) + 4 <= 232 staged pixels, which Wi = 232 (244) is not.
Wi = 232 is kept as a routing case instead: the binding refuses it, and
the module takes the pad kernel and the register-only forward for it,
as it did before.

The inputs are seeded random fp32 with planted +-0, denormals, the
largest values that still round to a finite bf16, and bf16 rounding ties
in both directions (halfway above an even and above an odd kept bit)."""

import pytest
import torch

import geomx_amd.ops as ops
from geomx_amd.ops import conv as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64               # bf16 elements on either side of xb
SENTINEL = 0x7FC1        # a NaN pattern no conversion produces
N = 3
PLANTED = [0x00000000, 0x80000000,                # +-0
           0x00000001, 0x807FFFFF, 0x00008000,    # denormals
           0x7F7F7FFF, 0xFF7F7FFF,                # largest with finite bf16
           0x3F808000, 0xBF808000,                # tie, even kept bit: down
           0x3F818000, 0xBF818000,                # tie, odd kept bit: up
           0x3F808001, 0x3F807FFF]                # just off the tie


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _image(Hi, Wi, seed):
    """[N][3][Hi][Wi] fp32, channels_last, with the planted bit patterns
    at the corners of the image and at seeded positions."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(N * Hi * Wi * 3, generator=g).view(torch.int32)
    vals = torch.tensor(PLANTED, dtype=torch.int64)
    vals = torch.where(vals >= 2 ** 31, vals - 2 ** 32, vals).to(torch.int32)
    pos = torch.randperm(flat.numel(), generator=g)[:4 * len(PLANTED)]
    flat[pos] = vals.repeat(4)
    flat[:len(PLANTED)] = vals                    # first pixels of image 0
    flat[-len(PLANTED):] = vals                   # last pixels of the last
    x = flat.view(torch.float32).view(N, Hi, Wi, 3).permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert torch.isfinite(x).all()
    return x.to(DEV)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(16, 3, 5, 5, generator=g) * 0.05).to(DEV)
    b = (torch.randn(16, generator=g) * 0.1).to(DEV)
    return w, b, C._pack_frags(w, C.build_fwd_index(w.shape).to(DEV))[0]


def _parent_route(geops, x, w_frags, b):
    """(out, mask, xb) of pad_ch3to4_nhwc + conv5_pool_nhwc."""
    n, _, Hi, Wi = x.shape
    xb = C._empty_nhwc(n, 4, Hi, Wi, DEV)
    geops.pad_ch3to4_nhwc(x, xb, n * Hi * Wi)
    out = C._empty_nhwc(n, 16, (Hi - 4) // 2, (Wi - 4) // 2, DEV)
    mask = torch.empty(out.numel(), dtype=torch.uint8, device=DEV)
    geops.conv5_pool_nhwc(xb, w_frags, b, out, mask, n, Hi, Wi, Hi - 4,
                          Wi - 4, 4, 16)
    return out, mask, xb


def _bits(t):
    """The memory of a dense bf16 tensor as int16, in storage order."""
    return torch.as_strided(t, (t.numel(),), (1,)).view(torch.int16).cpu()


@pytest.mark.parametrize("Wi", [20, 28, 224, 228])
@pytest.mark.parametrize("Hi", [6, 10, 12])
def test_x32_forward_and_copy(geops, Hi, Wi):
    x = _image(Hi, Wi, seed=Hi * 1000 + Wi)
    w, b, w_frags = _params(7)
    ref_out, ref_mask, ref_xb = _parent_route(geops, x, w_frags, b)
    # channel 3 of the oracle itself is zero
    assert not ref_xb[:, 3].any()
    dims = (N, Hi, Wi, Hi - 4, Wi - 4, 16)
    npx = N * Hi * Wi * 4
    for n_wg in (1, 2, 0):
        for with_xb in (True, False):
            out = torch.full_like(ref_out, float("nan"))
            mask = torch.full_like(ref_mask, 77)
            buf = torch.full((npx + 2 * GUARD,), SENTINEL,
                             dtype=torch.int16, device=DEV)
            xb = buf[GUARD:GUARD + npx].view(torch.bfloat16) if with_xb \
                else torch.Tensor()
            if n_wg:
                geops.conv5_pool_x32_nwg_nhwc(x, w_frags, b, out, mask, xb,
                                              *dims, n_wg)
            else:
                geops.conv5_pool_x32_nhwc(x, w_frags, b, out, mask, xb,
                                          *dims)
            tag = f"n_wg {n_wg}, xb {with_xb}"
            assert torch.equal(_bits(out), _bits(ref_out)), tag
            assert torch.equal(mask.cpu(), ref_mask.cpu()), tag
            got = buf.cpu()
            assert (got[:GUARD] == SENTINEL).all(), f"store ahead, {tag}"
            assert (got[-GUARD:] == SENTINEL).all(), f"store behind, {tag}"
            if with_xb:
                assert torch.equal(got[GUARD:-GUARD], _bits(ref_xb)), tag
            else:
                assert (got == SENTINEL).all(), tag


def test_x32_binding_refuses_what_the_kernel_does_not_serve(geops):
    w, b, w_frags = _params(7)

    def call(x, Hi, Wi):
        out = C._empty_nhwc(N, 16, (Hi - 4) // 2, (Wi - 4) // 2, DEV)
        mask = torch.empty(out.numel(), dtype=torch.uint8, device=DEV)
        geops.conv5_pool_x32_nhwc(x, w_frags, b, out, mask, torch.Tensor(),
                                  N, Hi, Wi, Hi - 4, Wi - 4, 16)

    for Wi in (22, 232):           # not whole granules; past the row image
        with pytest.raises(RuntimeError):
            call(_image(6, Wi, 1), 6, Wi)
    with pytest.raises(RuntimeError):                     # NCHW memory
        call(_image(6, 20, 1).contiguous(), 6, 20)
    with pytest.raises(RuntimeError):                     # 4 B aligned base
        flat = torch.zeros(N * 6 * 20 * 3 + 1, device=DEV)
        call(flat[1:].view(N, 6, 20, 3), 6, 20)


def _module_run(x, x32_input, train=True):
    torch.manual_seed(11)
    m = C.GeoConv5Pool(3, 16).to(DEV)
    m.x32_input = x32_input
    plan, _ = m._route(x)
    took = x32_input and C._x32_operand(x, plan) is not None
    with torch.autocast("cuda", torch.bfloat16):
        if not train:
            with torch.no_grad():
                return took, m(x), None, None
        y = m(x)
    g = torch.Generator().manual_seed(3)
    y.backward(torch.randn(y.shape, generator=g).to(DEV).to(y.dtype))
    return took, y.detach(), m.weight.grad, m.bias.grad


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    ia = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.contiguous().view(ia), b.contiguous().view(ia))


def test_module_forward_backward_equals_the_pad_route(geops):
    x = _image(12, 28, 5)[:2]
    took, y, gw, gb = _module_run(x, True)
    took0, y0, gw0, gb0 = _module_run(x, False)
    assert took and not took0
    assert _same(y, y0) and _same(gw, gw0) and _same(gb, gb0)
    # no weight gradient wanted: no copy is written, same output
    took, yn, _, _ = _module_run(x, True, train=False)
    assert took and _same(yn, y0)


def test_routing(geops):
    # widths the kernel does not serve and a bf16 image keep the pad route
    for x in (_image(12, 22, 6)[:2],
              _image(12, 28, 6)[:2].to(torch.bfloat16)):
        took, y, gw, gb = _module_run(x, True)
        _, y0, gw0, gb0 = _module_run(x, False)
        assert not took
        assert _same(y, y0) and _same(gw, gw0) and _same(gb, gb0)
    # (forward only: at this width the weight gradient is a library call)
    x = _image(12, 232, 6)[:2]
    took, y, _, _ = _module_run(x, True, train=False)
    _, y0, _, _ = _module_run(x, False, train=False)
    assert not took and _same(y, y0)
    # an NCHW-contiguous fp32 image gives the bits of its channels_last copy
    xc = _image(12, 28, 6)[:2]
    xn = xc.contiguous()
    assert xn.is_contiguous() and not xn.is_contiguous(
        memory_format=torch.channels_last)
    took, y, gw, gb = _module_run(xn, True)
    _, y0, gw0, gb0 = _module_run(xc, True)
    assert took
    assert _same(y, y0) and _same(gw, gw0) and _same(gb, gb0)
