"""Every conv kernel of the step against an exact float64 oracle.

Inputs are small integers (tests/conv_exact_cases.py), so every fp32
partial sum of a kernel is exact in any order and the float64 result is
the expected output bit for bit: every comparison is torch.equal, on the
int16 view for bf16 outputs. tests/test_conv_exact_cpu.py asserts, case by
case, the conditions this rests on. Every output buffer (slabs included)
is NaN before the launch, so an element that is not written fails, and
the bf16 outputs are the middle of a longer NaN buffer whose ends must
stay NaN.

Which case reaches which kernel instantiation (launch tables of conv.hip
and convwrw2.hip):

  k_conv5_nhwc<4,1>    test_direct (3,16); test_direct_grid_stride
  k_conv5_nhwc<16,2>   test_direct (16,32)
  k_conv5_nhwc<16,1>   test_direct (16,16); test_dgrad_conv1_class
  k_conv5_nhwc<32,2>   test_direct (32,32)
  k_conv5_nhwc<32,1>   test_direct_hook (conv5_direct_nhwc);
                       test_direct_wide_row (conv5_nhwc, Wi = 233);
                       test_dgrad_conv2_past_the_lds_table (pad 0, W 228)
  k_conv5_lds_nhwc<32,1,PIX,PAD,UNPOOL>, test_dgrad_conv2[form]:
      <120,4,true>   pooled, W 20 26 112     <232,4,true>   W 116 118 224
      <120,4,false>  pad4,   W 20 26 112     <232,4,false>  W 116 118 224
      <120,0,false>  pad0,   W 20 26 112     <232,0,false>  W 116 118 224
    and test_dgrad_conv2_nwg: <120,4,*> at W 26, <232,4,*> at W 116
  k_conv5_wrw4_nhwc<PIX,UNPOOL>, test_wrw4_slabs[form]:
      <136,false> / <136,true>   W 26 40 132
      <232,false> / <232,true>   W 138 228
  k_conv5_pool_nhwc<4>   test_pool4 (W 230 and 244)
  k_pad_ch3to4_nhwc<float> / <bf16_t>   test_pad_ch3to4[fp32 / bf16]"""

import pytest
import torch

import conv_exact_cases as X
import geomx_amd.ops as ops
import wrw_golden_cases as G4
from geomx_amd.ops import conv as C
from test_kernels_gpu import ROUTING_CASES

DEV = "cuda:0"
GUARD = 64          # bf16 elements on either side of an output
NAN = float("nan")


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


_CACHE = {}


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


class _Guarded:
    """A bf16 output [shape] in the middle of a NaN-filled buffer."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.bfloat16,
                              device=DEV)
        self.out = self.buf[GUARD:GUARD + n].view(*shape)
        assert self.out.data_ptr() == self.buf.data_ptr() + 2 * GUARD

    def check(self, want64):
        """The output equals the oracle bit for bit, the guards are NaN."""
        b = self.buf.cpu()
        assert torch.isnan(b[:GUARD].float()).all(), "store ahead of out"
        assert torch.isnan(b[-GUARD:].float()).all(), "store behind out"
        want = X.to_bf16(want64)
        got = self.out.cpu()
        assert got.shape == want.shape
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (got.double() - want64).abs().max().item()


def _frags(weight, index, geops=None):
    """Fragments through ops.conv._w_frags (CPU gather) or, with geops,
    through the packing kernel."""
    idx = _cached(("idx", index.__name__, tuple(weight.shape)),
                  lambda: index(tuple(weight.shape)))
    if geops is None:
        return C._w_frags(weight, idx).to(DEV)
    f, = geops.conv5_pack_frags(weight.to(DEV), idx.to(DEV))
    return f


# ---------------------------------------------------------------------
# 1. the direct kernel
# ---------------------------------------------------------------------

def _direct_case(cir, co, ho, wo):
    def build():
        x, weight, bias = X.direct_inputs(cir, co, ho, wo)
        return x, weight, bias, X.conv_oracle(x, weight)
    return _cached(("direct", cir, co, ho, wo), build)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cir,co,ho,wo", X.DIRECT_CASES)
def test_direct(geops, cir, co, ho, wo, with_bias):
    """<4,1>, <16,2>, <16,1>, <32,2> through conv5_nhwc, pad 0."""
    x, weight, bias, conv = _direct_case(cir, co, ho, wo)
    g = _Guarded(X.N, ho, wo, co)
    b = bias.to(DEV) if with_bias else torch.Tensor()
    geops.conv5_nhwc(x.to(DEV), _frags(weight, C.build_fwd_index), b, g.out,
                     X.N, ho + 4, wo + 4, ho, wo, x.shape[-1], co, 0)
    g.check(conv + bias.double() if with_bias else conv)


@pytest.mark.gpu
@pytest.mark.parametrize("cir,co,ho,wo", X.DIRECT_HOOK_CASES)
def test_direct_hook(geops, cir, co, ho, wo):
    """<32,1> through conv5_direct_nhwc: the oracle of
    test_conv2_dgrad_rows_gpu.py and test_unpool_fused_gpu.py."""
    x, weight, _, conv = _direct_case(cir, co, ho, wo)
    g = _Guarded(X.N, ho, wo, co)
    geops.conv5_direct_nhwc(x.to(DEV), _frags(weight, C.build_fwd_index),
                            g.out, X.N, ho + 4, wo + 4, ho, wo, cir, co)
    g.check(conv)


@pytest.mark.gpu
def test_direct_wide_row(geops):
    """<32,1> through conv5_nhwc: Wi = 233 is past the 232-pixel LDS
    table; 14 tiles and a 5-pixel tail tile, with bias."""
    cir, co, ho, wo = X.DIRECT_WIDE_CASE
    x, weight, bias, conv = _direct_case(cir, co, ho, wo)
    g = _Guarded(X.N, ho, wo, co)
    geops.conv5_nhwc(x.to(DEV), _frags(weight, C.build_fwd_index),
                     bias.to(DEV), g.out, X.N, ho + 4, wo + 4, ho, wo, cir,
                     co, 0)
    g.check(conv + bias.double())


@pytest.mark.gpu
def test_direct_grid_stride(geops):
    """<4,1> with more rows than the 32768-block grid has waves: the
    grid-stride loop. The batch is 7 images tiled along N."""
    c = X.GRID_CASE
    n, per, ho, wo = c["n"], c["period"], c["h"] - 4, c["w"] - 4
    x7, weight, bias = X.direct_inputs(c["cir"], c["co"], ho, wo, n=per)
    want7 = X.to_bf16(X.conv_oracle(x7, weight, bias))
    reps = (n + per - 1) // per
    x = x7.to(DEV).repeat(reps, 1, 1, 1)[:n].contiguous()
    want = want7.to(DEV).repeat(reps, 1, 1, 1)[:n].contiguous()
    g = _Guarded(n, ho, wo, c["co"])
    geops.conv5_nhwc(x, _frags(weight, C.build_fwd_index), bias.to(DEV),
                     g.out, n, c["h"], c["w"], ho, wo, 4, c["co"], 0)
    assert torch.isnan(g.buf[:GUARD].float()).all()
    assert torch.isnan(g.buf[-GUARD:].float()).all()
    assert torch.equal(g.out.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------
# 2. data gradient
# ---------------------------------------------------------------------

def _dgrad_case(co, cir, h, w):
    def build():
        weight, go, gp, mask = X.dgrad_inputs(co, cir, h, w)
        return weight, go, gp, mask, X.dgrad_oracle(go, weight)
    return _cached(("dgrad", co, cir, h, w), build)


def _dgrad2_run(geops, h, w, form, packed, n_wg=None):
    co, cir = X.DGRAD2_SHAPE
    weight, go, gp, mask, gx = _dgrad_case(co, cir, h, w)
    wf = _frags(weight, C.build_dgrad_index, geops if packed else None)
    g = _Guarded(X.N, h, w, cir)
    dims = (X.N, h + 4, w + 4, h, w, co, cir)
    if form == "pooled":
        if n_wg is None:
            geops.conv5_dgrad_unpool_nhwc(gp.to(DEV), mask.to(DEV), wf,
                                          g.out, *dims)
        else:
            geops.conv5_dgrad_nwg_nhwc(gp.to(DEV), mask.to(DEV), wf, g.out,
                                       *dims, n_wg)
    elif form == "pad4":
        if n_wg is None:
            geops.conv5_nhwc(go.to(DEV), wf, torch.Tensor(), g.out, *dims, 4)
        else:
            geops.conv5_dgrad_nwg_nhwc(go.to(DEV), torch.Tensor(), wf, g.out,
                                       *dims, n_wg)
    else:
        geops.conv5_nhwc(X.pad4(go).to(DEV), wf, torch.Tensor(), g.out,
                         *dims, 0)
    g.check(gx)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True], ids=["w_frags", "packed"])
@pytest.mark.parametrize("form", ["pooled", "pad4", "pad0"])
@pytest.mark.parametrize("h,w", X.DGRAD2_CASES)
def test_dgrad_conv2(geops, h, w, form, packed):
    """All six k_conv5_lds_nhwc forms against the float64 transposed
    conv; fragments from build_dgrad_index by both packers."""
    _dgrad2_run(geops, h, w, form, packed)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pooled", "pad4"])
@pytest.mark.parametrize("n_wg", X.DGRAD2_NWG)
@pytest.mark.parametrize("h,w", X.DGRAD2_NWG_CASES)
def test_dgrad_conv2_nwg(geops, h, w, n_wg, form):
    """6 blocks on 1 and 2 workgroups: the persistent loop, restaged LDS
    and the pooled form's cross-block prefetch."""
    _dgrad2_run(geops, h, w, form, False, n_wg)


@pytest.mark.gpu
@pytest.mark.parametrize("h", X.DGRAD2_HS)
def test_dgrad_conv2_past_the_lds_table(geops, h):
    """W = 228 needs a 244-pixel staging row: the pad-0 form falls back
    to the direct kernel <32,1>; the pad-4 and pooled forms have no
    kernel and must raise, not run something else."""
    w = X.DGRAD2_WIDE_W
    _dgrad2_run(geops, h, w, "pad0", False)
    for form in ("pad4", "pooled"):
        with pytest.raises(RuntimeError):
            _dgrad2_run(geops, h, w, form, False)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True], ids=["w_frags", "packed"])
@pytest.mark.parametrize("co,cir,h,w", X.DGRAD1_CASES)
def test_dgrad_conv1_class(geops, co, cir, h, w, packed):
    """Route 'direct_padded': <16,1> over the physically padded gradient.
    The channels past CIr of the 16-channel result are exactly +0."""
    weight, go, _, _, gx = _dgrad_case(co, cir, h, w)
    wf = _frags(weight, C.build_dgrad_index, geops if packed else None)
    g = _Guarded(X.N, h, w, 16)
    geops.conv5_nhwc(X.pad4(go).to(DEV), wf, torch.Tensor(), g.out, X.N,
                     h + 4, w + 4, h, w, co, 16, 0)
    want = torch.zeros(X.N, h, w, 16, dtype=torch.float64)
    want[..., :cir] = gx
    g.check(want)
    pad = _bits(g.out[..., cir:])
    assert torch.equal(pad, torch.zeros_like(pad))      # +0, not -0


# ---------------------------------------------------------------------
# 3. conv1 weight gradient
# ---------------------------------------------------------------------

def _wrw4_case(h, w, ch4_zero=False):
    def build():
        x, go, gp, mask = X.wrw_inputs(4, 16, h, w, ch4_zero=ch4_zero)
        return x, go, gp, mask, X.wrw4_block_grads(x, go)
    return _cached(("wrw4", h, w, ch4_zero), build)


def _wrw4_run(geops, h, w, n_wg, pooled, ch4_zero=False):
    x, go, gp, mask, blocks = _wrw4_case(h, w, ch4_zero)
    part = torch.full((n_wg, G4.T16, G4.CO), NAN, dtype=torch.float32,
                      device=DEV)
    dims = (X.N, h, w, h - 4, w - 4, 4, G4.CO, n_wg)
    if pooled:
        geops.conv5_wrw_unpool_nhwc(x.to(DEV), gp.to(DEV), mask.to(DEV),
                                    part, *dims)
    else:
        geops.conv5_wrw_nhwc(x.to(DEV), go.to(DEV), part, *dims)
    got, want = part.cpu(), X.slab_oracle(blocks, n_wg)
    assert torch.equal(got, want), (got - want).abs().max().item()
    dead = got[:, G4.dead_rows()]
    assert torch.equal(dead, torch.zeros_like(dead))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
@pytest.mark.parametrize("h,w,n_wg", X.WRW4_CASES)
def test_wrw4_slabs(geops, h, w, n_wg, pooled):
    """Each slab is the float64 sum over exactly its workgroup's two-row
    blocks; the 75 dead rows are zero stores over NaN. The 4th input
    channel carries data, so its 25 rows are checked."""
    _wrw4_run(geops, h, w, n_wg, pooled)


@pytest.mark.gpu
def test_wrw4_slabs_odd_ho(geops):
    """Ho = 5: the last block of each image has one row."""
    _wrw4_run(geops, *X.WRW4_ODD_CASE, pooled=False)


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
def test_wrw4_slabs_zero_4th_channel(geops, pooled):
    """The production input: the padding channel is zero."""
    _wrw4_run(geops, *X.WRW4_CH4_ZERO_CASE, pooled, ch4_zero=True)


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
def test_wrw4_idle_workgroups_write_zero_slabs(geops, pooled):
    """More workgroups than blocks. The flush of k_conv5_wrw4_nhwc is
    unconditional: an idle workgroup stores its zero accumulators to the
    live rows and zeros to the dead ones, so its slab is all zero
    whatever it held (here NaN)."""
    h, w, n_wg = X.WRW4_IDLE_CASE
    got = _wrw4_run(geops, h, w, n_wg, pooled)
    assert got[:4].abs().sum().item() > 0
    assert torch.equal(got[4:], torch.zeros_like(got[4:]))


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", [False, True], ids=["full", "pooled"])
@pytest.mark.parametrize("cir,co,n,h,w", X.WRW_E2E_CASES)
def test_wrw_via_kernel(geops, cir, co, n, h, w, pooled):
    """ops.conv.wrw_via_kernel: the kernel at its default grid (768
    workgroups in the last case), the slab sum and
    build_wrw_unpack_index give the float64 dW (OIHW) and bias gradient."""
    def build():
        x, go, gp, mask = X.wrw_inputs(cir, co, h, w, n=n)
        return x, go, gp, mask, X.wgrad_oracle(x, go, cir)
    x, go, gp, mask, (dw, db) = _cached(("e2e", cir, co, n, h, w), build)
    shape = (co, cir, 5, 5)
    idx, t16 = C.build_wrw_unpack_index(shape)
    xb = x.to(DEV).permute(0, 3, 1, 2)
    if pooled:
        got = C.wrw_via_kernel(xb, gp.to(DEV).permute(0, 3, 1, 2),
                               idx.to(DEV), t16, shape, want_bias=True,
                               mask=mask.to(DEV))
    else:
        got = C.wrw_via_kernel(xb, go.to(DEV).permute(0, 3, 1, 2),
                               idx.to(DEV), t16, shape, want_bias=True)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32
    assert torch.equal(got[0].cpu(), dw.float())
    assert torch.equal(got[1].cpu(), db.float())


# ---------------------------------------------------------------------
# 4. register-only conv1 forward
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_wg", X.POOL4_GRIDS)
@pytest.mark.parametrize("case", X.POOL4_CASES,
                         ids=lambda c: "%d-%d-h%d-w%d-%s" % c)
def test_pool4(geops, case, n_wg):
    """k_conv5_pool_nhwc<4>: rows off the 232-pixel table, against the
    oracle of fwd_golden_cases (out and codes)."""
    def build():
        x, weight, bias = X.pool_inputs(*case)
        return (x, weight, bias) + tuple(X.pool_oracle(x, weight, bias))
    x, weight, bias, want, codes = _cached(("pool4", case), build)
    cir, co, h, w, _ = case
    n, hop, wop = x.shape[0], (h - 4) // 2, (w - 4) // 2
    g = _Guarded(n, hop, wop, co)
    mask = torch.full((g.out.numel() + 2 * GUARD,), 77, dtype=torch.uint8,
                      device=DEV)
    b = bias.to(DEV) if bias is not None else torch.Tensor()
    args = (x.to(DEV), _frags(weight, C.build_fwd_index), b, g.out,
            mask[GUARD:-GUARD], n, h, w, h - 4, w - 4, 4, co)
    if n_wg is None:
        geops.conv5_pool_nhwc(*args)
    else:
        geops.conv5_pool_nwg_nhwc(*args, n_wg)
    g.check(want.double())
    m = mask.cpu()
    assert (m[:GUARD] == 77).all() and (m[-GUARD:] == 77).all()
    assert torch.equal(m[GUARD:-GUARD].reshape(codes.shape), codes)


# ---------------------------------------------------------------------
# 5. modules at the routing boundaries
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind,ci,co,W,routes", ROUTING_CASES)
def test_modules_at_routing_boundaries(geops, kind, ci, co, W, routes):
    """The rows of ROUTING_CASES again with integer data: what each op on
    a native route returns (y for fwd; x.grad for dgrad; weight.grad and
    bias.grad for wrw) equals the float64 chain conv -> ReLU -> first-
    maximum pool -> scatter through those codes. Ops on 'aten' are left
    to the tolerance test: library kernels promise no exact sums."""
    from geomx_amd.ops.conv import GeoConv5, GeoConv5Pool, _SUPPORTED_FWD
    pooled = kind == "pool"
    x, weight, bias, go = X.module_inputs(ci, co, W, pooled)
    want = _cached(("module", ci, co, W, pooled),
                   lambda: X.module_oracle(x, weight, bias, go, pooled))
    y64, gx64, dw64, db64 = want
    if pooled:
        m = GeoConv5Pool(ci, co)
    elif kind == "direct":
        m = GeoConv5(ci, co, enabled_shapes=_SUPPORTED_FWD)
    else:
        m = GeoConv5(ci, co)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    m = m.to(DEV)
    xg = x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
    assert tuple(m._route(xg)[0]) == routes
    assert any(r != "aten" for r in routes)
    y = m(xg)
    y.backward(go.to(DEV).permute(0, 3, 1, 2))

    def nchw(v64):
        return _bits(X.to_bf16(v64).permute(0, 3, 1, 2))

    fwd, dgrad, wrw = routes
    if fwd != "aten":
        assert y.dtype == torch.bfloat16
        assert torch.equal(_bits(y), nchw(y64))
    if dgrad != "aten":
        assert xg.grad.dtype == torch.bfloat16
        assert torch.equal(_bits(xg.grad), nchw(gx64))
    if wrw != "aten":
        assert m.weight.grad.dtype == torch.float32
        assert torch.equal(m.weight.grad.cpu(), dw64.float())
        assert torch.equal(m.bias.grad.cpu(), db64.float())


# ---------------------------------------------------------------------
# 6. channel pad
# ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix", X.PAD_NPIX)
def test_pad_ch3to4(geops, npix, fp32):
    """Equals torch.cat([x.to(bf16), zeros], -1) bit for bit (ties both
    ways, +-0, subnormals, overflow to inf, +-inf), the 4th channel is
    +0 and nothing behind npix * 4 elements is touched."""
    x = X.pad_inputs(npix, fp32)
    want = X.pad_oracle(x)
    out = torch.full((npix * 4 + X.PAD_GUARD,), NAN, dtype=torch.bfloat16,
                     device=DEV)
    before = out[npix * 4:].clone()
    geops.pad_ch3to4_nhwc(x.to(DEV), out, npix)
    got = out.view(torch.int16)
    assert torch.equal(got[:npix * 4].reshape(npix, 4).cpu(), want)
    assert torch.equal(got[:npix * 4].reshape(npix, 4)[:, 3].cpu(),
                       torch.zeros(npix, dtype=torch.int16))
    assert torch.equal(got[npix * 4:], before.view(torch.int16))
