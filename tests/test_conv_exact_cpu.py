"""The cases of tests/conv_exact_cases.py really are exact, and not empty
(CPU only).

tests/test_conv_exact_gpu.py compares kernels with float64 oracles by
torch.equal. That is sound only while every oracle value is an integer
that the kernel's number formats hold exactly (|v| <= 256 for a bf16
output, < 2^24 for an fp32 slab or gradient), and it is worth something
only while the expected tensors are not mostly zero, every weight tap is
used and the pooled forms see every code. Each condition is asserted per
case, and each hand-written oracle is checked against an independent
formulation: autograd of a float64 F.conv2d."""

import pytest
import torch

import conv_exact_cases as X
import wrw_golden_cases as G4
from geomx_amd.ops import conv as C

BF16_EXACT = 256.0
FP32_EXACT = float(2 ** 24)


def _is_int(t):
    return torch.equal(t, t.round())


def _mostly_nonzero(t):
    return (t != 0).double().mean().item() > 0.5


def _weight_is_live(weight):
    """Every tap (kh, kw) and every (ci, o) pair has a non-zero weight."""
    nz = weight != 0
    return bool(nz.any(dim=0).any(dim=0).all()) and \
        bool(nz.any(dim=3).any(dim=2).all())


def _check_bf16_oracle(v, what):
    assert _is_int(v), what
    assert v.abs().max().item() <= BF16_EXACT, (what, v.abs().max().item())
    assert torch.equal(X.to_bf16(v).double(), v), what
    assert _mostly_nonzero(v), (what, (v != 0).double().mean().item())


ALL_CODES = {0, 1, 2, 3, 255}


# ---------------------------------------------------------------------
# 1. direct kernel
# ---------------------------------------------------------------------

@pytest.mark.parametrize("cir,co,ho,wo",
                         X.DIRECT_CASES + X.DIRECT_HOOK_CASES
                         + [X.DIRECT_WIDE_CASE])
def test_direct_cases_are_exact(cir, co, ho, wo):
    x, weight, bias = X.direct_inputs(cir, co, ho, wo)
    assert _weight_is_live(weight)
    assert (x[..., cir:] == 0).all()
    for b in (bias, None):
        v = X.conv_oracle(x, weight, b)
        assert v.shape == (X.N, ho, wo, co)
        if ho * wo >= 16:
            _check_bf16_oracle(v, (cir, co, ho, wo, b is not None))
        else:  # a handful of pixels: "mostly non-zero" is left to chance
            assert _is_int(v) and v.abs().max().item() <= BF16_EXACT
            assert v.abs().sum().item() > 0
    assert bias.abs().sum().item() > 0


def test_grid_stride_case_is_exact():
    c = X.GRID_CASE
    ho, wo = c["h"] - 4, c["w"] - 4
    assert c["n"] * ho > 32768 * 4          # more rows than waves
    assert c["n"] % c["period"] != 0        # the last period is cut short
    x, weight, bias = X.direct_inputs(c["cir"], c["co"], ho, wo,
                                      n=c["period"])
    v = X.conv_oracle(x, weight, bias)
    _check_bf16_oracle(v, "grid")
    # the 7 images differ pairwise, so a row read from a wrong image shows
    for i in range(c["period"]):
        for j in range(i):
            assert not torch.equal(v[i], v[j])


# ---------------------------------------------------------------------
# 2. data gradient
# ---------------------------------------------------------------------

def _check_dgrad(co, cir, h, w):
    weight, go, gp, mask = X.dgrad_inputs(co, cir, h, w)
    assert _weight_is_live(weight)
    gx = X.dgrad_oracle(go, weight)
    assert gx.shape == (X.N, h, w, cir)
    _check_bf16_oracle(gx, (co, cir, h, w))
    x0 = torch.zeros(X.N, h, w, cir)
    assert torch.equal(gx, X.autograd_grads(x0, go, weight)[0])
    if mask is not None:
        assert set(mask.unique().tolist()) == ALL_CODES
        assert gp.abs().max().item() <= 2
    assert go.abs().max().item() <= 2


@pytest.mark.parametrize("h,w", X.DGRAD2_CASES
                         + [(h, X.DGRAD2_WIDE_W) for h in X.DGRAD2_HS])
def test_dgrad_conv2_cases_are_exact(h, w):
    _check_dgrad(*X.DGRAD2_SHAPE, h, w)


@pytest.mark.parametrize("co,cir,h,w", X.DGRAD1_CASES)
def test_dgrad_conv1_cases_are_exact(co, cir, h, w):
    _check_dgrad(co, cir, h, w)


def test_dgrad_widths_sit_on_the_table_edges():
    """The staging-row arithmetic of conv5_lds_launch, restated: the
    width set holds the last row of the 120-pixel variants, the first
    and the last of the 232-pixel ones and the first past the table."""
    def need(w):
        return max((w + 15) // 16 * 16 + 4, w + 4)
    ws = X.DGRAD2_LDS_WS
    assert max(w for w in ws if need(w) <= 120) == 112
    assert need(112 + 2) > 120
    assert min(w for w in ws if need(w) > 120) == 116
    assert max(ws) == 224 and need(224) <= 232 < need(224 + 2)
    assert need(X.DGRAD2_WIDE_W) > 232
    for h, w in X.DGRAD2_NWG_CASES:
        assert (h, w) in X.DGRAD2_CASES


# ---------------------------------------------------------------------
# 3. conv1 weight gradient
# ---------------------------------------------------------------------

_WRW4_GEOMS = sorted({(h, w, False) for h, w, _ in
                      X.WRW4_CASES + [X.WRW4_ODD_CASE, X.WRW4_IDLE_CASE]}
                     | {X.WRW4_CH4_ZERO_CASE[:2] + (True,)})


@pytest.mark.parametrize("h,w,ch4_zero", _WRW4_GEOMS)
def test_wrw4_slab_oracle_is_exact(h, w, ch4_zero):
    x, go, gp, mask = X.wrw_inputs(4, 16, h, w, ch4_zero=ch4_zero)
    blocks = X.wrw4_block_grads(x, go)
    assert _is_int(blocks)
    total = blocks.sum(dim=0)
    assert total.abs().max().item() < FP32_EXACT
    # the layout: 100 tap rows and the bias row live, 75 rows dead
    live = torch.cat([G4.live_rows(), torch.tensor([G4.BIAS_ROW])])
    assert live.numel() == 101 and G4.dead_rows().numel() == 75
    assert (blocks[:, G4.dead_rows()] == 0).all()
    ch4 = torch.tensor([X.wrw4_slot(kh, kw, 3) for kh in range(5)
                        for kw in range(5)])
    if ch4_zero:
        assert (total[ch4] == 0).all()
        rest = torch.tensor(sorted(set(live.tolist()) - set(ch4.tolist())))
        assert _mostly_nonzero(total[rest])
    else:
        assert _mostly_nonzero(total[ch4])
        assert _mostly_nonzero(total[live])
    # summed over the workgroups and gathered through the unpack index,
    # the slabs are the float64 weight gradient of the autograd form
    _, dw, db = X.autograd_grads(x, go, torch.zeros(16, 4, 5, 5))
    for n_wg in (1, 3, 4, 6):
        slabs = X.slab_oracle(blocks, n_wg)
        assert slabs.dtype == torch.float32
        full = slabs.double().sum(dim=0)
        assert torch.equal(full, total)
        idx, t16 = C.build_wrw_unpack_index((16, 4, 5, 5))
        assert t16 == G4.T16
        assert torch.equal(full.reshape(-1)[idx].reshape(16, 4, 5, 5), dw)
        assert torch.equal(full[G4.BIAS_ROW], db)
    if mask is not None:
        assert set(mask.unique().tolist()) == ALL_CODES


def test_wrw4_idle_case_has_idle_workgroups():
    h, w, n_wg = X.WRW4_IDLE_CASE
    x, go, _, _ = X.wrw_inputs(4, 16, h, w)
    blocks = X.wrw4_block_grads(x, go)
    assert blocks.shape[0] == 4 < n_wg
    slabs = X.slab_oracle(blocks, n_wg)
    assert slabs.shape == (n_wg, G4.T16, 16)
    assert (slabs[4:] == 0).all() and slabs[:4].abs().sum().item() > 0


@pytest.mark.parametrize("cir,co,n,h,w", X.WRW_E2E_CASES)
def test_wrw_e2e_cases_are_exact(cir, co, n, h, w):
    x, go, gp, mask = X.wrw_inputs(cir, co, h, w, n=n)
    dw, db = X.wgrad_oracle(x, go, cir)
    assert _is_int(dw) and _is_int(db)
    assert max(dw.abs().max().item(), db.abs().max().item()) < FP32_EXACT
    assert _mostly_nonzero(dw) and _mostly_nonzero(db)
    _, dw2, db2 = X.autograd_grads(x, go, torch.zeros(co, cir, 5, 5))
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert set(mask.unique().tolist()) == ALL_CODES
    if cir == 3:    # data in the padding channel: the unpack must drop it
        assert x[..., 3].abs().sum().item() > 0


def test_wrw_e2e_cap_case_reaches_the_cap():
    cir, co, n, h, w = X.WRW_E2E_CASES[-1]
    assert n * ((h - 4 + 3) // 4) > C._WRW_NWG


# ---------------------------------------------------------------------
# 4. register-only conv1 forward
# ---------------------------------------------------------------------

@pytest.mark.parametrize("case", X.POOL4_CASES,
                         ids=lambda c: "%d-%d-h%d-w%d-%s" % c)
def test_pool4_cases_are_exact(case):
    cir, co, h, w, kind = case
    # off the 232-pixel table of the LDS kernel, so the register-only
    # kernel serves the row (conv5_pool_launch)
    assert w % 2 == 0 and (w - 4 + 15) // 16 * 16 + 4 > 232
    assert C.plan_conv5((co, cir, 5, 5), h, w, pooled=True).fwd == "pool"
    x, weight, bias = X.pool_inputs(*case)
    assert _weight_is_live(weight)
    out, codes = X.pool_oracle(x, weight, bias)
    v = out.double()
    assert _is_int(v) and v.abs().max().item() <= BF16_EXACT
    # the fp32 conv of the shared oracle is the float64 one
    conv = X.conv_oracle(x.permute(0, 2, 3, 1), weight, bias)
    assert conv.abs().max().item() <= BF16_EXACT
    mx = torch.stack([conv[:, dy::2, dx::2] for dy in range(2)
                      for dx in range(2)]).max(dim=0).values.clamp(min=0)
    assert torch.equal(mx, v)
    if kind == "neg":
        # bias -60 under |conv| <= 50: the all-clamped output, code 255
        assert set(codes.unique().tolist()) == {255} and (v == 0).all()
    else:
        assert set(codes.unique().tolist()) == ALL_CODES
        assert _mostly_nonzero(v)


# ---------------------------------------------------------------------
# 5. modules at the routing boundaries
# ---------------------------------------------------------------------

# (kind, ci, co, W) of ROUTING_CASES in tests/test_kernels_gpu.py; the
# GPU test takes the table itself and asserts the plan
_MODULE_SHAPES = [(True, 3, 16, 228), (True, 3, 16, 230), (True, 16, 32, 116),
                  (True, 16, 32, 118), (True, 16, 16, 20),
                  (False, 3, 16, 35), (False, 16, 32, 224),
                  (False, 16, 32, 226), (False, 16, 32, 230)]


@pytest.mark.parametrize("pooled,ci,co,w", _MODULE_SHAPES)
def test_module_cases_are_exact(pooled, ci, co, w):
    x, weight, bias, go = X.module_inputs(ci, co, w, pooled)
    assert _weight_is_live(weight)
    y, gx, dw, db = X.module_oracle(x, weight, bias, go, pooled)
    assert y.shape == go.shape
    for v in (y, gx):
        _check_bf16_oracle(v, (pooled, ci, co, w))
    for v in (dw, db):
        assert _is_int(v) and v.abs().max().item() < FP32_EXACT
        assert _mostly_nonzero(v)
    # the chain again through autograd: float64 conv, ReLU, max-pool.
    # max_pool2d sends a tied window's gradient to its first maximum in
    # the order (0,0), (0,1), (1,0), (1,1), like the kernels' codes.
    F = torch.nn.functional
    x64 = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    w64 = weight.double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    y2 = F.conv2d(x64, w64, b64)
    if pooled:
        y2 = F.max_pool2d(F.relu(y2), 2, 2)
    y2.backward(go.permute(0, 3, 1, 2).double())
    assert torch.equal(y2.detach().permute(0, 2, 3, 1), y)
    assert torch.equal(x64.grad.permute(0, 2, 3, 1), gx)
    assert torch.equal(w64.grad, dw) and torch.equal(b64.grad, db)


# ---------------------------------------------------------------------
# 6. channel pad
# ---------------------------------------------------------------------

@pytest.mark.parametrize("npix", X.PAD_NPIX)
def test_pad_inputs_hold_the_edges(npix):
    x = X.pad_inputs(npix, fp32=True)
    assert x.shape == (npix, 3) and x.dtype == torch.float32
    assert not torch.isnan(x).any()
    want = X.pad_oracle(x)
    assert want.shape == (npix, 4) and (want[:, 3] == 0).all()
    xb = X.pad_inputs(npix, fp32=False)
    assert xb.dtype == torch.bfloat16
    assert torch.equal(X.pad_oracle(xb), want)
    if npix < 44:
        return
    bits = x.view(torch.int32)
    edge = X._bits_to_f32(X.PAD_EDGE_BITS).view(torch.int32)
    for e in edge.tolist():                 # every value in every channel
        assert (bits == e).any(dim=0).all(), hex(e & 0xFFFFFFFF)
    got = want[:, :3].reshape(-1).tolist()
    # ties went both ways, the largest finite values became inf, the
    # subnormals and the signed zeros kept their signs
    for b in (0x3F80, 0x3F82, 0x7F80, 0xFF80 - 0x10000, 0x8000 - 0x10000,
              0x0002, 0x0080, 0x8080 - 0x10000):
        assert b in got, hex(b & 0xFFFF)
