"""The conv1 stage from uint8 images and a value table (k_conv5_pool2_nhwc
<232, uint8_t>, PixPair<uint8_t>, input_table of GeoConv5 / GeoConv5Pool)
against the fp32 route of the same build on x32 = table[c][x]; every
comparison is torch.equal on integer views. Images are seeded bytes with
every value planted in every channel (a batch of fewer than 256 pixels
gets the head of a permutation). Each table has three different rows:
ToTensor with rows 1, 2 rotated by 85, 170 entries; a mean/std table;
random values with +-0, a denormal, the largest values with a finite bf16
and bf16 ties both ways planted. Row c of a table is a grayscale table."""

import os
import subprocess
import sys

import pytest
import torch

from geomx_amd.ops import conv as C
from test_conv1_x32_gpu import geops  # noqa: F401  (the fixture)

DEV = "cuda:0"
N = 3
GUARD = 64
SENTINEL = 0x7FC1        # a NaN pattern no table entry holds
FLT_MAX = 3.4028234663852886e38
PLANTED = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7F7FFF,
           0xFF7F7FFF, 0x3F808000, 0xBF808000, 0x3F818000, 0xBF818000]


def _table(kind):
    if kind == "totensor":
        t = C.to_tensor_table(3)
        return torch.stack([t[c].roll(85 * c) for c in range(3)])
    if kind == "meanstd":
        return C.to_tensor_table(3, [0.485, 0.456, 0.406],
                                 [0.229, 0.224, 0.225])
    g = torch.Generator().manual_seed(99)
    t = torch.randn(3, 256, generator=g) * torch.tensor([[1.], [3.], [.2]])
    vals = torch.tensor(PLANTED, dtype=torch.int64)
    vals = torch.where(vals >= 2 ** 31, vals - 2 ** 32, vals).to(torch.int32)
    for c in range(3):
        t[c, torch.randperm(256, generator=g)[:len(PLANTED)]] = \
            vals.view(torch.float32)
    return t


TABLES = ["totensor", "meanstd", "special"]


def _image(ch, H, W, seed):
    """[N][ch][H][W] uint8 on the GPU, channels_last."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N * H * W, ch), generator=g, dtype=torch.uint8)
    k = min(256, N * H * W)
    for c in range(ch):
        x[torch.randperm(N * H * W, generator=g)[:k], c] = \
            torch.randperm(256, generator=g)[:k].to(torch.uint8)
    return x.view(N, H, W, ch).permute(0, 3, 1, 2).to(DEV)


def _same(a, b):
    iv = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.detach().contiguous().view(iv), b.detach().contiguous().view(iv))


def _params(ch, seed=7):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(16, ch, 5, 5, generator=g) * 0.05).to(DEV)
    b = (torch.randn(16, generator=g) * 0.1).to(DEV)
    index = C.build_fwd_index if ch == 3 else C.build_c1_fwd_index
    return w, b, C._pack_frags(w, index(w.shape).to(DEV))[0]


def _outputs(Hi, Wi):
    out = torch.full((N, 16, (Hi - 4) // 2, (Wi - 4) // 2), float("nan"),
                     dtype=torch.bfloat16, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    return out, torch.full((out.numel(),), 77, dtype=torch.uint8, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("Wi", [20, 28, 224, 228])
@pytest.mark.parametrize("Hi", [6, 10, 12])
def test_u8_forward_and_copy(geops, Hi, Wi, kind):
    table = _table(kind)
    tab = table.to(DEV, torch.bfloat16)
    x = _image(3, Hi, Wi, seed=Hi * 1000 + Wi)
    _, b, w_frags = _params(3)
    dims = (N, Hi, Wi, Hi - 4, Wi - 4, 16)
    npx = N * Hi * Wi * 4
    ref_out, ref_mask = _outputs(Hi, Wi)
    ref_xb = C._empty_nhwc(N, 4, Hi, Wi, DEV)
    geops.conv5_pool_x32_nhwc(C.table_gather(table, x), w_frags, b, ref_out,
                              ref_mask, ref_xb, *dims)
    for n_wg in (1, 2, 0):
        for with_xb in (True, False):
            out, mask = _outputs(Hi, Wi)
            buf = torch.full((npx + 2 * GUARD,), SENTINEL,
                             dtype=torch.int16, device=DEV)
            xb = buf[GUARD:GUARD + npx].view(torch.bfloat16) if with_xb \
                else torch.Tensor()
            if n_wg:
                geops.conv5_pool_u8_nwg_nhwc(x, tab, w_frags, b, out, mask,
                                             xb, *dims, n_wg)
            else:
                geops.conv5_pool_u8_nhwc(x, tab, w_frags, b, out, mask, xb,
                                         *dims)
            tag = f"n_wg {n_wg}, xb {with_xb}"
            assert _same(out, ref_out) and _same(mask, ref_mask), tag
            want = torch.full_like(buf, SENTINEL)
            if with_xb:
                want[GUARD:-GUARD] = ref_xb.permute(0, 2, 3, 1).reshape(-1) \
                    .view(torch.int16)
            assert torch.equal(buf, want), tag


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("H,W", [(6, 6), (10, 28), (28, 28), (12, 228)])
def test_grayscale_forward_and_wrw(geops, H, W, kind):
    c = TABLES.index(kind)
    table = _table(kind)[c:c + 1]
    tab = table.to(DEV, torch.bfloat16)
    x = _image(1, H, W, seed=H * 1000 + W)
    _, b, w_frags = _params(1)
    g = torch.Generator().manual_seed(H + W)
    gp = torch.randn(N, (H - 4) // 2, (W - 4) // 2, 16, generator=g) \
        .to(DEV, torch.bfloat16)
    go = torch.randn(N, H - 4, W - 4, 16, generator=g).to(DEV, torch.bfloat16)
    res = {}
    for name, xin, t in (("x32", C.table_gather(table, x), None),
                         ("u8", x, tab)):
        for n_wg in (0, 2):
            out, mask = _outputs(H, W)
            geops.conv5c1_pool(xin, w_frags, b, out, mask, N, H, W, n_wg, t)
            slabs = n_wg or min(768, N * ((H - 4 + 1) // 2))
            pooled = torch.full((slabs, 32, 16), float("nan"), device=DEV)
            full = pooled.clone()
            codes = res["x32", 0][1] if res else mask
            geops.conv5c1_wrw_unpool(xin, gp, codes, pooled, N, H, W, n_wg, t)
            geops.conv5c1_wrw(xin, go, full, N, H, W, n_wg, t)
            res[name, n_wg] = (out, mask, pooled, full)
    for n_wg in (0, 2):
        for a, r in zip(res["u8", n_wg], res["x32", n_wg]):
            assert _same(a, r), n_wg


def _module_run(ch, x, table, autocast=True, train=True):
    torch.manual_seed(11)
    m = C.GeoConv5Pool(ch, 16, input_table=table).to(DEV)
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        y = m(x)
    if not train:
        return y.detach(), None, None
    g = torch.Generator().manual_seed(3)
    y.backward(torch.randn(y.shape, generator=g).to(DEV).to(y.dtype))
    return y.detach(), m.weight.grad, m.bias.grad


@pytest.mark.gpu
@pytest.mark.parametrize("ch,autocast", [(3, True), (3, False), (1, True),
                                         (1, False)])
def test_module_equals_the_fp32_image(geops, ch, autocast):
    table = _table("special")[:ch]
    x = _image(ch, 12, 28, 5)
    m = C.GeoConv5Pool(ch, 16, input_table=table).to(DEV)
    assert m.input_table.is_cuda and "input_table" not in m.state_dict()
    assert C._u8_operand(x, m._route(x)[0]) is not None
    got = _module_run(ch, x, table, autocast)
    ref = _module_run(ch, C.table_gather(table, x), None, autocast)
    assert got[0].dtype == (torch.bfloat16 if autocast else torch.float32)
    assert all(_same(a, r) for a, r in zip(got, ref))


@pytest.mark.gpu
def test_routing_and_refusals(geops):
    table = _table("meanstd")
    flat = torch.zeros(N * 12 * 28 * 3 + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = _image(3, 12, 28, 6).permute(0, 2, 3, 1).reshape(-1)
    for x, train in [(_image(3, 12, 22, 6), True),
                     (_image(3, 12, 232, 6), False),   # (wrw: a library call)
                     (_image(3, 12, 28, 6).contiguous(), True),
                     (flat[1:].view(N, 12, 28, 3).permute(0, 3, 1, 2), True)]:
        m = C.GeoConv5Pool(3, 16, input_table=table).to(DEV)
        assert C._u8_operand(x, m._route(x)[0]) is None
        got = _module_run(3, x, table, train=train)
        ref = _module_run(3, C.table_gather(table, x), None, train=train)
        assert all(_same(a, r) for a, r in zip(got, ref) if r is not None)

    tab = table.to(DEV, torch.bfloat16)
    for ch in (3, 1):
        x = _image(ch, 6, 20, 1)
        _, b, w_frags = _params(ch)

        def call(x, t):
            out, mask = _outputs(6, 20)
            if ch == 3:
                geops.conv5_pool_u8_nhwc(x, t, w_frags, b, out, mask,
                                         torch.Tensor(), N, 6, 20, 2, 16, 16)
            else:
                geops.conv5c1_pool(x, w_frags, b, out, mask, N, 6, 20, 0, t)

        ok = tab[:ch].contiguous()
        call(x, ok)
        for xb, tb in [(x, tab[:2].contiguous()), (x, ok.float()),
                       (x.float(), ok), (x.bfloat16(), ok)]:
            with pytest.raises(RuntimeError):
                call(xb, tb)


def test_gather_semantics_and_rounding_on_the_cpu():
    table = _table("special")
    assert torch.equal(C.to_tensor_table(2)[1], torch.arange(256) / 255)
    # cf2bf in integers against the cast the host rounds the table with,
    # +-FLT_MAX (finite, rounds to infinity) included
    u = torch.cat([table.reshape(-1), torch.tensor([FLT_MAX, -FLT_MAX])]) \
        .view(torch.int32).long() & 0xFFFFFFFF
    cf2bf = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    assert torch.equal(cf2bf, u.int().view(torch.float32).bfloat16()
                       .view(torch.int16).long() & 0xFFFF)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (2, 3, 12, 12), generator=g, dtype=torch.uint8)
    x32 = C.table_gather(table, x)
    for c in range(3):
        assert torch.equal(x32[:, c].view(torch.int32),
                           table[c][x[:, c].long()].view(torch.int32))
    m = C.GeoConv5Pool(3, 16, input_table=table)
    y = m(x)
    y.sum().backward()
    gw = m.weight.grad.clone()
    m.zero_grad()
    m(x32).sum().backward()
    assert y.dtype == torch.float32 and torch.equal(y, m(x32))
    assert torch.equal(gw, m.weight.grad)
    with pytest.raises(ValueError):
        C.GeoConv5Pool(3, 16, input_table=table[:2])
    with pytest.raises(RuntimeError):   # no table: as before, no image
        C.GeoConv5Pool(3, 16)(x)


@pytest.mark.parametrize("script", ["cnn.py", "resnet50.py"])
def test_example_runs_with_uint8_input(script):
    ex = os.path.join(os.path.dirname(os.path.dirname(__file__)), "examples")
    r = subprocess.run(
        [sys.executable, os.path.join(ex, script), "--uint8-input",
         "--max-iters", "2", "-bs", "8", "--data-n", "64", "--image-size",
         "20"], capture_output=True, text=True, timeout=600, cwd=ex)
    assert r.returncode == 0 and "Iteration 2" in r.stdout, r.stderr[-2000:]
