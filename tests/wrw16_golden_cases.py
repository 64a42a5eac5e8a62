"""Case tables, input builders and the exact oracle of the conv2-class
weight-gradient kernel k_conv5_wrw16_nhwc (helper, not a test; used by
scripts/record_wrw16_golden.py and tests/test_wrw16_pipelined_gpu.py).

Two kinds of input:
  * exact: small integers (|v| <= 3) in bf16. Every product and every
    partial sum is an integer far below 2^24, so the fp32 accumulators
    are exact in any order and the expected slab is the float64 sum over
    exactly the blocks a workgroup owns (slab_oracle).
  * normal: seeded CPU randn cast to bf16, the same bytes on any
    machine. tests/golden/wrw16_parent.npz holds the per-workgroup slabs
    of the parent kernel on GOLDEN_CASES, recorded on an MI355X from the
    commit named in the file's `commit` entry; a kernel that keeps every
    accumulator's MFMA order reproduces them bit for bit.
The full-resolution gradient of a pooled case is the CPU scatter of the
pooled one, so both forms of a case share one expected value."""

import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "wrw16_parent.npz")

N = 2
CI = 16
T16 = 416           # slab rows: 25 tap tiles + the bias tile
BIAS_ROW = 400
# 26: one window with a tail; 40: tail inside the second window; 110:
# the flagship; 132: PIX=136 full (Wo=128); 138: first width on PIX=232;
# 228: 7 windows, the launcher's maximum
WIDTHS = (26, 40, 110, 132, 138, 228)
# N=2, H=8 -> four 2-row blocks: n_wg 1 walks them all (every cross-
# block prefetch, and the last block with nothing to prefetch), 3 is
# uneven (one workgroup restages), 4 never restages
GRIDS = (1, 3, 4)
COS = (32, 16)
H = 8
# (H, W, n_wg, CO); both forms (full-resolution gout, pooled + mask)
EXACT_CASES = [(H, w, g, co) for co in COS for w in WIDTHS for g in GRIDS]
# odd Ho (5): a one-row tail block; full-resolution form only
ODD_CASE = (9, 40, 1, 32)
# order-invariant cases, chosen to keep the golden file small
GOLDEN_CASES = [(H, 110, 1, 32), (H, 110, 3, 32), (H, 138, 1, 32),
                (H, 40, 1, 16), (H, 40, 3, 16)]


def key(h, w, n_wg, co):
    return "wrw16_h%d_w%d_g%d_co%d" % (h, w, n_wg, co)


def _codes(g, shape):
    """As tests/wrw_golden_cases.py::_pooled_grad: codes from
    {0,1,2,3,255}, a few all-255 pixels, a few single-quadrant ones."""
    n, hp, wp, co = shape
    codes = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8)
    mask = codes[torch.randint(0, 5, shape, generator=g)]
    mask[0, 0, 0] = 255
    mask[1, hp - 1, wp - 1] = 255
    mask[0, hp - 1, wp // 2] = 255
    for quad in range(4):
        mask[quad % n, quad % hp, (1 + 2 * quad) % wp] = quad
    return mask


def _scatter(gp, mask):
    """Max-pool backward on the CPU: code == dy*2+dx ? g : 0."""
    n, hp, wp, co = gp.shape
    full = torch.zeros(n, 2 * hp, 2 * wp, co, dtype=gp.dtype)
    for dy in range(2):
        for dx in range(2):
            full[:, dy::2, dx::2] = torch.where(
                mask == dy * 2 + dx, gp, torch.zeros_like(gp))
    return full


def build_inputs(h, w, co, exact):
    """CPU tensors of one geometry: x [N][16][h][w] and go [N][co][h-4]
    [w-4] (NHWC memory, bf16); for even h also the pooled gradient gp
    [N][co][(h-4)/2][(w-4)/2] (NHWC memory) and its flat codes, with go
    their scatter. (x, go, gp, mask); gp and mask None for odd h.
    `exact` draws integers in [-3, 3], otherwise standard normals."""
    g = torch.Generator().manual_seed(
        16000 + 1000 * h + w + (50000 if exact else 0) + 7 * co)

    def draw(*shape):
        if exact:
            return torch.randint(-3, 4, shape, generator=g) \
                .to(torch.bfloat16)
        return torch.randn(*shape, generator=g).to(torch.bfloat16)

    ho, wo = h - 4, w - 4
    x = draw(N, h, w, CI).permute(0, 3, 1, 2)
    if ho % 2:
        return x, draw(N, ho, wo, co).permute(0, 3, 1, 2), None, None
    gp = draw(N, ho // 2, wo // 2, co)
    mask = _codes(g, gp.shape)
    go = _scatter(gp, mask)
    return (x, go.permute(0, 3, 1, 2), gp.permute(0, 3, 1, 2),
            mask.reshape(-1).contiguous())


def block_grads(x, go):
    """Float64 weight and bias gradient of every two-row block, as slabs:
    [N * ceil(Ho/2)][416][co], block index n * blocks_h + bh, row
    (kh*5+kw)*16 + ci, bias in row 400, rows 401..415 zero."""
    xn = x.permute(0, 2, 3, 1).double()       # [N][h][w][ci]
    gn = go.permute(0, 2, 3, 1).double()      # [N][ho][wo][co]
    n, ho, wo, co = gn.shape
    blocks_h = (ho + 1) // 2
    out = torch.zeros(n * blocks_h, T16, co, dtype=torch.float64)
    for i in range(n):
        for bh in range(blocks_h):
            r0, r1 = 2 * bh, min(2 * bh + 2, ho)
            gb = gn[i, r0:r1]
            slab = out[i * blocks_h + bh]
            for kh in range(5):
                for kw in range(5):
                    xs = xn[i, r0 + kh:r1 + kh, kw:kw + wo]
                    t = (kh * 5 + kw) * 16
                    slab[t:t + 16] = torch.einsum("hwc,hwo->co", xs, gb)
            slab[BIAS_ROW] = gb.sum(dim=(0, 1))
    return out


def slab_oracle(blocks, n_wg):
    """Expected fp32 slabs [n_wg][416][co]: workgroup wg owns blocks wg,
    wg + n_wg, ... of block_grads()."""
    nb = blocks.shape[0]
    return torch.stack([blocks[wg:nb:n_wg].sum(dim=0)
                        for wg in range(n_wg)]).float()
