"""Case tables and input builders of the fused forward conv + bias + ReLU
+ max-pool tests (helper, not a test; used by
scripts/record_fwd_golden.py and tests/test_fwd_pool_packed_gpu.py).

tests/golden/fwd_pool_parent.npz holds, per random-valued case, the
pooled output (bf16 bits as int16) and the argmax codes that
conv5_pool_nhwc gave on an MI355X at the commit named in the file's
`commit` entry: the parent of the 4-row kernels, whose result does not
depend on its grid. Inputs come from a seeded CPU generator and are cast
to bf16, so they are the same bytes on any machine."""

import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "fwd_pool_parent.npz")

N = 2               # the block -> (image, row) decode crosses an image
# Hop = 1 (a lone tail block), 3 (a full block, then a one-row tail), 4
HEIGHTS = (6, 10, 12)
# conv2 (CI = 16): one tile and three idle waves; Wo = 34 (a clamped tail
# tile and pooled pixels past Wop); the flagship's 7 tiles; the widest row
# the 120-pixel table admits
WIDTHS16 = (20, 38, 110, 116)
# conv1 (CIr = 3 padded to 4): the same, with the flagship 224 and the
# widest row of the 232-pixel table
WIDTHS4 = (20, 38, 224, 228)
# (CIr, CO, H, W)
CASES = ([(16, 32, h, w) for h in HEIGHTS for w in WIDTHS16]
         + [(16, 16, 10, 38)]
         + [(3, 16, h, w) for h in HEIGHTS for w in WIDTHS4])
GRIDS = (1, 2, None)    # n_wg of the test hook; None = the default grid

# exact-arithmetic cases: (CIr, CO, H, W, bias kind)
EXACT = ([(cir, co, h, w, "int")
          for cir, co, ws in ((16, 32, WIDTHS16), (3, 16, WIDTHS4))
          for h in HEIGHTS for w in ws]
         + [(16, 16, 10, 38, "int"),
            (16, 32, 10, 38, "neg"), (3, 16, 10, 38, "neg"),
            (16, 32, 10, 38, "none"), (3, 16, 10, 38, "none")])


def key(cir, co, h, w):
    return "c%d_o%d_h%d_w%d" % (cir, co, h, w)


def _nhwc4(x):
    """[N][CIr][H][W] bf16 -> the kernel's input: NHWC memory, 3 channels
    zero-padded to 4."""
    if x.shape[1] == 3:
        x = F.pad(x, (0, 0, 0, 0, 0, 1))
    return x.contiguous(memory_format=torch.channels_last)


def random_inputs(cir, co, h, w):
    """(x [N][CI][h][w] NHWC bf16, weight OIHW fp32, bias fp32), CPU."""
    g = torch.Generator().manual_seed(9000 + 100000 * cir + 10000 * co
                                      + 1000 * h + w)
    x = torch.randn(N, cir, h, w, generator=g).to(torch.bfloat16)
    weight = torch.randn(co, cir, 5, 5, generator=g) * 0.1
    bias = torch.randn(co, generator=g) * 0.5
    return _nhwc4(x), weight, bias


def exact_inputs(cir, co, h, w, kind):
    """Inputs from {-2..2}, weights from {-1, 0, 1}, integer bias: every
    partial sum is an integer far below 2^24, so the fp32 result is exact
    in any summation order, and bf16 holds the pooled value exactly
    whenever it is below 256 (it is rounded like the kernel's otherwise).
    `kind`: 'int' bias in {-3..3}, 'neg' bias -60 (nearly every window
    clamps), 'none' no bias."""
    g = torch.Generator().manual_seed(4000 + 100000 * cir + 10000 * co
                                      + 1000 * h + w + len(kind))
    x = torch.randint(-2, 3, (N, cir, h, w), generator=g).to(torch.bfloat16)
    weight = torch.randint(-1, 2, (co, cir, 5, 5), generator=g).float()
    if kind == "int":
        bias = torch.randint(-3, 4, (co,), generator=g).float()
    elif kind == "neg":
        bias = torch.full((co,), -60.0)
    else:
        bias = None
    return _nhwc4(x), weight, bias


def expected_exact(x, weight, bias):
    """fp32 conv + bias, first-maximum 4-way compare in the order (0,0),
    (0,1), (1,0), (1,1), `<= 0` clamp to (0, code 255), bf16. Returns
    (out [N][Hop][Wop][CO] bf16, codes, same shape, uint8)."""
    cir = weight.shape[1]
    conv = F.conv2d(x[:, :cir].float(), weight, bias)
    q = [conv[:, :, dy::2, dx::2] for dy in range(2) for dx in range(2)]
    mx = q[0].clone()
    arg = torch.zeros_like(mx, dtype=torch.uint8)
    for k in (1, 2, 3):
        win = q[k] > mx
        mx = torch.where(win, q[k], mx)
        arg = torch.where(win, torch.full_like(arg, k), arg)
    dead = mx <= 0
    mx = torch.where(dead, torch.zeros_like(mx), mx)
    arg = torch.where(dead, torch.full_like(arg, 255), arg)
    return (mx.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous(),
            arg.permute(0, 2, 3, 1).contiguous())
