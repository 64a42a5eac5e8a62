"""Case table and input builder of the conv1 weight-gradient goldens
(helper, not a test; used by scripts/record_wrw_golden.py and
tests/test_wrw_packed_gpu.py).

tests/golden/wrw_parent.npz holds, per case, the per-workgroup slabs of
k_conv5_wrw4_nhwc reduced to their live entries, recorded on an MI355X
from the commit named in the file's `commit` entry (the parent of the
7-tile kernel). Inputs come from a seeded CPU generator and are cast to
bf16, so they are the same bytes on any machine. The full-resolution
gradient of a pooled case is the CPU scatter of the pooled one, so both
forms of a case share one golden (the parent computes them bit-equal;
the recorder checks that before it writes)."""

import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "wrw_parent.npz")

N = 2
CI, CO = 4, 16
T16 = 176           # slab rows: 10 tap tiles + the bias tile
BIAS_ROW = 160
# 26: one window with a tail; 40: tail inside the second window; 132:
# PIX=136 full (Wo=128); 138: first width on PIX=232; 228: 7 windows,
# the launcher's maximum
WIDTHS = (26, 40, 132, 138, 228)
# N=2, H=8 -> four 2-row blocks: n_wg 1 walks them all (every cross-
# block prefetch, and the last block with nothing to prefetch), 3 is
# uneven (one workgroup restages), 4 never restages
GRIDS = (1, 3, 4)
H = 8
# (H, W, n_wg); both forms (full-resolution gout, pooled + mask)
CASES = [(H, w, g) for w in WIDTHS for g in GRIDS]
# odd Ho (5): a one-row tail block; full-resolution form only
ODD_CASE = (9, 40, 1)


def key(h, w, n_wg):
    return "wrw4_h%d_w%d_g%d" % (h, w, n_wg)


def live_rows():
    """Slab rows of the 100 taps: (kw*2 + kh//4)*16 + (kh%4)*4 + ci."""
    rows = [(kw * 2 + kh // 4) * 16 + (kh % 4) * 4 + ci
            for kh in range(5) for kw in range(5) for ci in range(CI)]
    return torch.tensor(sorted(rows), dtype=torch.int64)


def reduce_slabs(part):
    """[n_wg][176][16] -> [n_wg][101][16]: the live tap rows, then the
    bias row."""
    idx = torch.cat([live_rows(), torch.tensor([BIAS_ROW])])
    return part[:, idx.to(part.device)]


def dead_rows():
    live = set(live_rows().tolist()) | {BIAS_ROW}
    return torch.tensor([r for r in range(T16) if r not in live],
                        dtype=torch.int64)


def _pooled_grad(g, hp, wp):
    """As tests/test_unpool_fused_gpu.py::_pooled_grad: codes from
    {0,1,2,3,255}, a few all-255 pixels, a few single-quadrant ones."""
    gp = torch.randn(N, hp, wp, CO, generator=g).to(torch.bfloat16)
    codes = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8)
    mask = codes[torch.randint(0, 5, (N, hp, wp, CO), generator=g)]
    mask[0, 0, 0] = 255
    mask[1, hp - 1, wp - 1] = 255
    mask[0, hp - 1, wp // 2] = 255
    for quad in range(4):
        mask[quad % N, quad % hp, (1 + 2 * quad) % wp] = quad
    return gp, mask


def _scatter(gp, mask):
    """Max-pool backward on the CPU: code == dy*2+dx ? g : 0."""
    n, hp, wp, co = gp.shape
    full = torch.zeros(n, 2 * hp, 2 * wp, co, dtype=gp.dtype)
    for dy in range(2):
        for dx in range(2):
            full[:, dy::2, dx::2] = torch.where(
                mask == dy * 2 + dx, gp, torch.zeros_like(gp))
    return full


def build_inputs(h, w):
    """CPU tensors of one geometry: x [N][4][h][w] and go [N][16][h-4]
    [w-4] (NHWC memory, bf16); for even h also the pooled gradient gp
    [N][16][(h-4)/2][(w-4)/2] (NHWC memory) and its flat codes, with
    go their scatter. (x, go, gp, mask); gp and mask None for odd h."""
    g = torch.Generator().manual_seed(7000 + 1000 * h + w)
    ho, wo = h - 4, w - 4
    x = torch.randn(N, h, w, CI, generator=g).to(torch.bfloat16) \
        .permute(0, 3, 1, 2)
    if ho % 2:
        go = torch.randn(N, ho, wo, CO, generator=g).to(torch.bfloat16)
        return x, go.permute(0, 3, 1, 2), None, None
    gp, mask = _pooled_grad(g, ho // 2, wo // 2)
    go = _scatter(gp, mask)
    return (x, go.permute(0, 3, 1, 2), gp.permute(0, 3, 1, 2),
            mask.reshape(-1).contiguous())
