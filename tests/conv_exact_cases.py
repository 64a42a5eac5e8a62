"""Case tables, seeded CPU input builders and float64 oracles of the exact
conv tests (helper, not a test; used by tests/test_conv_exact_cpu.py and
tests/test_conv_exact_gpu.py).

Every input is a small integer: activations and gradients in [-2, 2]
(bf16), weights in {-1, 0, 1} (fp32, exact in bf16), bias in [-3, 3]
(fp32), weight-gradient operands in [-3, 3] as in wrw16_golden_cases.
Every product and every partial sum of a kernel is then an integer far
below 2^24, so its fp32 accumulators are exact in any order and the
float64 value computed here is the expected result bit for bit; a bf16
output holds it exactly while its magnitude is at most 256.
tests/test_conv_exact_cpu.py asserts those conditions case by case.

All tensors built here live on the CPU. Activations and gradients are
returned in NHWC memory order as plain contiguous [N][H][W][C] tensors,
which is what the kernels read."""

import torch
import torch.nn.functional as F

import fwd_golden_cases as FG
import wrw16_golden_cases as G16
import wrw_golden_cases as G4

N = 2               # the row -> (image, row) decode crosses an image


def _gen(*key):
    seed = 77000
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31 - 1))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def to_bf16(v64):
    """double -> float -> bfloat16, the kernels' own rounding chain."""
    return v64.float().to(torch.bfloat16)


# ---------------------------------------------------------------------
# 1. the direct kernel k_conv5_nhwc
# ---------------------------------------------------------------------

# (CIr, CO) -> instantiation <CI, COT> of the launch table in conv.hip
# (geops_conv5_nhwc, pad 0): <4,1>, <16,2>, <16,1>, <32,2>. (32, 16) is
# <32,1>: through the hook conv5_direct_nhwc at any width, through
# conv5_nhwc only on rows wider than the 232-pixel LDS table.
DIRECT_SHAPES = ((3, 16), (16, 32), (16, 16), (32, 32))
DIRECT_HOOK_SHAPE = (32, 16)
# fewer rows than the four waves of a block, and more
DIRECT_HOS = (1, 3, 6)
# 1: every lane clamps to pixel 0; 16: one full tile; 17: a full tile and
# a one-pixel tail tile; 35: two tiles and a tail (cross-tile prefetch)
DIRECT_WOS = (1, 16, 17, 35)
DIRECT_CASES = [(cir, co, ho, wo) for cir, co in DIRECT_SHAPES
                for ho in DIRECT_HOS for wo in DIRECT_WOS]
DIRECT_HOOK_CASES = [DIRECT_HOOK_SHAPE + (ho, wo) for ho in DIRECT_HOS
                     for wo in DIRECT_WOS]
# Wi = 233: past the 232-pixel table, 14 tiles and a 5-pixel tail tile
DIRECT_WIDE_CASE = DIRECT_HOOK_SHAPE + (3, 229)
# grid-stride loop: N * Ho = 131200 rows > 32768 blocks x 4 waves. The
# batch is 7 distinct images tiled along N (7 is coprime with every
# power-of-two stride), so the oracle is computed for 7 images only.
GRID_CASE = dict(cir=3, co=16, n=8200, h=20, w=21, period=7)


def direct_inputs(cir, co, ho, wo, n=N):
    """(x [n][ho+4][wo+4][CI] bf16 with CIr padded to a multiple of 4 by
    zero channels, weight OIHW fp32, bias fp32)."""
    g = _gen(1, cir, co, ho, wo, n)
    ci = (cir + 3) & ~3
    x = torch.zeros(n, ho + 4, wo + 4, ci, dtype=torch.bfloat16)
    x[..., :cir] = _ints(g, -2, 2, n, ho + 4, wo + 4, cir).to(torch.bfloat16)
    weight = _ints(g, -1, 1, co, cir, 5, 5).float()
    bias = _ints(g, -3, 3, co).float()
    return x, weight, bias


def conv_oracle(x, weight, bias=None):
    """float64 conv2d(x, w) + bias of an NHWC x; [n][ho][wo][co]."""
    cir = weight.shape[1]
    y = F.conv2d(x[..., :cir].permute(0, 3, 1, 2).double(), weight.double(),
                 None if bias is None else bias.double())
    return y.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------
# 2. data gradient
# ---------------------------------------------------------------------

# conv2 class: weight (32, 16, 5, 5) -> dgrad conv CI' = 32, CO' = 16 on
# k_conv5_lds_nhwc<32, 1, PIX, PAD, UNPOOL>. H, W are the sizes of the
# data gradient (the layer's input); the kernel's staging row holds
# max(ceil(W/16)*16 + 4, W + 4) pixels.
DGRAD2_SHAPE = (32, 16)
# one 4-row group plus a tail, and two groups plus a tail
DGRAD2_HS = (6, 10)
# 20, 26: two tiles, the last partial; 112: seven full tiles, the widest
# row of the 120-pixel variants (staging row 116); 116 and 118: eight
# tiles, the first widths on the 232-pixel variants; 224: the widest row
# they serve (staging row 228)
DGRAD2_LDS_WS = (20, 26, 112, 116, 118, 224)
# 228 is past the LDS table (staging row 244): the pad-0 form falls back
# to the direct kernel <32,1>, the pad-4 and pooled forms are rejected
DGRAD2_WIDE_W = 228
DGRAD2_CASES = [(h, w) for h in DGRAD2_HS for w in DGRAD2_LDS_WS]
DGRAD2_NWG_CASES = [(10, 26), (10, 116)]
DGRAD2_NWG = (1, 2)
# conv1 class and (16, 16): the direct kernel <16,1> over the physically
# padded gradient (route 'direct_padded'); (CO, CIr, H, W)
DGRAD1_CASES = [(16, 3, 6, 21), (16, 3, 6, 35), (16, 16, 6, 21),
                (16, 16, 6, 35)]


def dgrad_inputs(co, cir, h, w):
    """(weight OIHW fp32, go [N][h-4][w-4][co] bf16, gp, mask). With even
    h and w, gp [N][(h-4)/2][(w-4)/2][co] is a pooled gradient, mask its
    flat argmax codes (uint8) and go their CPU scatter; otherwise go is
    drawn directly and gp, mask are None."""
    g = _gen(2, co, cir, h, w)
    weight = _ints(g, -1, 1, co, cir, 5, 5).float()
    ho, wo = h - 4, w - 4
    if (ho | wo) & 1:
        go = _ints(g, -2, 2, N, ho, wo, co).to(torch.bfloat16)
        return weight, go, None, None
    gp = _ints(g, -2, 2, N, ho // 2, wo // 2, co).to(torch.bfloat16)
    mask = G16._codes(g, gp.shape)
    go = G16._scatter(gp, mask)
    return weight, go, gp, mask.reshape(-1).contiguous()


def pad4(go):
    """The physical 4-pixel zero border of the pad-0 forms."""
    return F.pad(go, (0, 0, 4, 4, 4, 4)).contiguous()


def dgrad_oracle(go, weight):
    """float64 transposed conv, tap by tap and without a flip:
    gx[n, y, x, ci] = sum_{o, kh, kw} go[n, y-kh, x-kw, o] * w[o, ci, kh,
    kw], go zero outside the image. [N][ho+4][wo+4][cir]."""
    n, ho, wo, co = go.shape
    cir = weight.shape[1]
    g64, w64 = go.double(), weight.double()
    gx = torch.zeros(n, ho + 4, wo + 4, cir, dtype=torch.float64)
    for kh in range(5):
        for kw in range(5):
            gx[:, kh:kh + ho, kw:kw + wo] += torch.einsum(
                "nhwo,oc->nhwc", g64, w64[:, :, kh, kw])
    return gx


def wgrad_oracle(x, go, cir):
    """float64 weight and bias gradient, tap by tap: dW[o, ci, kh, kw] =
    sum_{n, y, x} x[n, y+kh, x+kw, ci] * go[n, y, x, o]. (dW OIHW, db)."""
    n, ho, wo, co = go.shape
    x64, g64 = x[..., :cir].double(), go.double()
    dw = torch.zeros(co, cir, 5, 5, dtype=torch.float64)
    for kh in range(5):
        for kw in range(5):
            dw[:, :, kh, kw] = torch.einsum(
                "nhwc,nhwo->oc", x64[:, kh:kh + ho, kw:kw + wo], g64)
    return dw, g64.sum(dim=(0, 1, 2))


def autograd_grads(x, go, weight):
    """The independent formulation: autograd of a float64 F.conv2d.
    (gx NHWC, dW OIHW, db), float64."""
    cir = weight.shape[1]
    x64 = x[..., :cir].permute(0, 3, 1, 2).double().requires_grad_(True)
    w64 = weight.double().requires_grad_(True)
    b64 = torch.zeros(weight.shape[0], dtype=torch.float64,
                      requires_grad=True)
    F.conv2d(x64, w64, b64).backward(go.permute(0, 3, 1, 2).double())
    return x64.grad.permute(0, 2, 3, 1).contiguous(), w64.grad, b64.grad


# ---------------------------------------------------------------------
# 3. conv1 weight gradient k_conv5_wrw4_nhwc
# ---------------------------------------------------------------------

WRW4_CASES = G4.CASES           # (H, W, n_wg): widths 26..228, grids 1 3 4
WRW4_ODD_CASE = G4.ODD_CASE     # Ho = 5: a one-row tail block
# N * ceil(Ho/2) = 4 blocks on 6 workgroups: two are idle
WRW4_IDLE_CASE = (G4.H, 26, 6)
# the 4th input channel zero, as the channel pad leaves it in production
WRW4_CH4_ZERO_CASE = (G4.H, 40, 3)
# end to end through ops.conv.wrw_via_kernel: (CIr, CO, n, H, W); the
# last reaches the 768-workgroup cap (n * ceil(Ho/4) = 800)
WRW_E2E_CASES = [(3, 16, N, 8, 40), (16, 32, N, 8, 40), (16, 16, N, 8, 40),
                 (3, 16, 200, 20, 26)]


def wrw_inputs(cir, co, h, w, n=N, ch4_zero=False):
    """(x [n][h][w][CI] bf16, go [n][h-4][w-4][co] bf16, gp, mask) from
    integers in [-3, 3]. CI = 4 for cir <= 4: the 4th channel carries
    data unless ch4_zero, for cir == 3 too: the unpack index must drop
    it. gp, mask as dgrad_inputs (None for odd h)."""
    g = _gen(3, cir, co, h, w, n, int(ch4_zero))
    ci = (cir + 3) & ~3
    x = _ints(g, -3, 3, n, h, w, ci).to(torch.bfloat16)
    if ch4_zero:
        x[..., 3] = 0
    ho, wo = h - 4, w - 4
    if ho & 1:
        return x, _ints(g, -3, 3, n, ho, wo, co).to(torch.bfloat16), None, None
    gp = _ints(g, -3, 3, n, ho // 2, wo // 2, co).to(torch.bfloat16)
    mask = G16._codes(g, gp.shape)
    return x, G16._scatter(gp, mask), gp, mask.reshape(-1).contiguous()


def wrw4_slot(kh, kw, ci):
    return (kw * 2 + kh // 4) * 16 + (kh % 4) * 4 + ci


def wrw4_block_grads(x, go):
    """Float64 weight and bias gradient of every two-row block in the
    slab layout of k_conv5_wrw4_nhwc: [n * ceil(Ho/2)][176][16], block
    index n * blocks_h + bh, tap row wrw4_slot(kh, kw, ci), bias in row
    160, the 75 other rows zero."""
    n, ho, wo, co = go.shape
    x64, g64 = x.double(), go.double()
    blocks_h = (ho + 1) // 2
    out = torch.zeros(n * blocks_h, G4.T16, co, dtype=torch.float64)
    for i in range(n):
        for bh in range(blocks_h):
            r0, r1 = 2 * bh, min(2 * bh + 2, ho)
            gb = g64[i, r0:r1]
            slab = out[i * blocks_h + bh]
            for kh in range(5):
                for kw in range(5):
                    xs = x64[i, r0 + kh:r1 + kh, kw:kw + wo]
                    t = wrw4_slot(kh, kw, 0)
                    slab[t:t + 4] = torch.einsum("hwc,hwo->co", xs, gb)
            slab[G4.BIAS_ROW] = gb.sum(dim=(0, 1))
    return out


slab_oracle = G16.slab_oracle   # workgroup wg owns blocks wg, wg + n_wg, ...


# ---------------------------------------------------------------------
# 4. register-only conv1 forward k_conv5_pool_nhwc<4>
# ---------------------------------------------------------------------

# rows past the 232-pixel table of k_conv5_pool2_nhwc. 230: Wo = 226, 14
# tiles and a tail tile of one pooled pixel; 244: 15 full tiles
POOL4_CASES = [(3, 16, h, w, kind) for h in (6, 10) for w in (230, 244)
               for kind in ("int", "neg", "none")]
POOL4_GRIDS = (1, 2, None)
pool_inputs = FG.exact_inputs       # x NCHW-shaped, NHWC memory
pool_oracle = FG.expected_exact


# ---------------------------------------------------------------------
# 5. modules at the routing boundaries
# ---------------------------------------------------------------------

MODULE_N, MODULE_H = 2, 8


def module_inputs(ci, co, w, pooled):
    """(x [N][8][w][ci] bf16, weight, bias, grad_out NHWC bf16); grad_out
    has the shape of the module's output."""
    g = _gen(5, ci, co, w, int(pooled))
    x = _ints(g, -2, 2, MODULE_N, MODULE_H, w, ci).to(torch.bfloat16)
    weight = _ints(g, -1, 1, co, ci, 5, 5).float()
    bias = _ints(g, -3, 3, co).float()
    ho, wo = MODULE_H - 4, w - 4
    if pooled:
        ho, wo = ho // 2, wo // 2
    go = _ints(g, -2, 2, MODULE_N, ho, wo, co).to(torch.bfloat16)
    return x, weight, bias, go


def module_oracle(x, weight, bias, go, pooled):
    """The float64 chain conv -> [ReLU -> first-maximum pool -> scatter of
    grad_out through those codes] -> gradients. (y, gx, dW, db), float64,
    y and gx NHWC."""
    conv = conv_oracle(x, weight, bias)
    if not pooled:
        y, gfull = conv, go
    else:
        q = [conv[:, dy::2, dx::2] for dy in range(2) for dx in range(2)]
        mx = q[0].clone()
        arg = torch.zeros(mx.shape, dtype=torch.uint8)
        for k in (1, 2, 3):
            win = q[k] > mx
            mx = torch.where(win, q[k], mx)
            arg = torch.where(win, torch.full_like(arg, k), arg)
        dead = mx <= 0
        y = torch.where(dead, torch.zeros_like(mx), mx)
        arg = torch.where(dead, torch.full_like(arg, 255), arg)
        gfull = G16._scatter(go, arg)
    dw, db = wgrad_oracle(x, gfull, weight.shape[1])
    return y, dgrad_oracle(gfull, weight), dw, db


# ---------------------------------------------------------------------
# 6. k_pad_ch3to4_nhwc
# ---------------------------------------------------------------------

# 2048*256 + 3: more than one trip of the 2048-block grid
PAD_NPIX = (1, 255, 257, 2048 * 256 + 3)
PAD_GUARD = 64      # elements behind the output

# fp32 bit patterns a bf16 rounding can get wrong
PAD_EDGE_BITS = [
    0x00000000, 0x80000000,                  # +-0
    0x3F808000, 0x3F818000,                  # ties: down to even, up to even
    0xBF808000, 0xBF818000,
    0x3F808001, 0x3F817FFF,                  # just above / below a tie
    0x00000001, 0x80000001, 0x00008000,      # subnormals (a tie among them)
    0x00018000, 0x007FFFFF, 0x807FFFFF,
    0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000,      # largest finite values:
    0x7F7FFFFF, 0xFF7FFFFF,                  # the last three round to inf
    0x7F800000, 0xFF800000,                  # +-inf
    0x3F800000,                              # 1.0 (22 values: coprime
]                                            # with the 3 channels)


def pad_inputs(npix, fp32):
    """[npix][3] input: the edge values in rotation over pixel and
    channel among seeded normals. bf16 inputs are the same values
    rounded (the kernel copies them)."""
    g = _gen(6, npix)
    x = torch.randn(npix * 3, generator=g)
    edge = _bits_to_f32(PAD_EDGE_BITS)
    # every second element is an edge value; 22 values against the
    # period of 3 channels put each value into each channel
    pos = torch.arange(0, npix * 3, 2)
    x[pos] = edge[torch.arange(pos.numel()) % edge.numel()]
    x = x.reshape(npix, 3)
    return x if fp32 else x.to(torch.bfloat16)


def _bits_to_f32(bits):
    t = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits],
                     dtype=torch.int32)
    return t.view(torch.float32)


def pad_oracle(x):
    """torch.cat([x.to(bf16), zeros], -1), as int16 bits [npix][4]."""
    xb = x.to(torch.bfloat16)
    return torch.cat([xb, torch.zeros(x.shape[0], 1, dtype=torch.bfloat16)],
                     dim=-1).view(torch.int16)
