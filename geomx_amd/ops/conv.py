"""GeoConv5 / GeoConv5Pool: 5x5 stride-1 convolution stages on the
hand-written gfx950 MFMA kernels (csrc/conv.hip, convwrw2.hip,
conv1c.hip).

Each of the three ops of a stage is routed on its own, from geometry
alone (plan_conv5):
  * forward: fused conv+bias+ReLU+maxpool kernels (k_conv5_pool*) for
    GeoConv5Pool, the direct kernel (k_conv5_nhwc) for the shapes a
    GeoConv5 enables, F.conv2d otherwise.
  * data gradient: LDS-staged conv with in-kernel virtual padding
    (k_conv5_lds_nhwc) for the conv2 class, the direct kernel on a
    physically padded grad_out for the other supported shapes.
  * weight+bias gradients: ds_read_b64_tr_b16 fragment kernels
    (convwrw2.hip) with the bias fused as an all-ones tap tile.
Behind a fused-pool forward the wrw and lds_pad4 kernels take the
pooled gradient and the argmax mask as they are (unpool_fusable) and do
the max-pool backward while staging; no full-resolution gradient is
built unless another route needs it.
A one-channel first layer (CIr = 1, CO = 16: the grayscale conv1 stage)
has kernels of its own (conv1c.hip): forward 'pool1' and weight gradient
'wrw1' read the [N][1][H][W] input as it is, fp32 or bf16, with no pad,
cast or layout kernel in front; its data gradient stays on ATen.
A stage built with an `input_table` ([CIr][256] fp32) takes uint8 images:
byte v of channel c stands for table[c][v] (to_tensor_table: ToTensor with
an optional per-channel normalisation). The 'pool' forward and the
grayscale kernels read the bytes themselves and look them up in a bf16
copy of the table in LDS (_u8_operand); any other uint8 input is expanded
by the gather table[c][x] and runs as the fp32 image it stands for.
Whatever no kernel serves goes to ATen (same math, library kernels);
one op on ATen does not move the other two off the custom kernels.
"""

from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from .. import gradsink
from . import native_available

_SUPPORTED_FWD = {(4, 16), (16, 32), (16, 16), (32, 32)}
_SUPPORTED_DGRAD = {(32, 16), (16, 16)}
_POOL_SHAPES = {(4, 16), (16, 32), (16, 16)}
_WRW_SHAPES = {(4, 16), (16, 32), (16, 16)}
_WRW_NWG = 768  # partial slabs (3 workgroups per CU)
_C1_SHAPE = (1, 16)   # (CIr, CO) of the grayscale conv1 stage
_C1_MAXW = 228        # its kernels' row image: 14 tiles / 7 K windows + 4

# shapes where the direct forward kernel MEASURES faster than MIOpen on
# MI355X (conv1 3->16 @224px: 0.73 vs 1.63 ms). conv2-class shapes tie
# or trail MIOpen's igemm (0.63 vs 0.54 fwd) and stay on F.conv2d;
# flip them on here as the kernel improves.
DEFAULT_ENABLED = {(4, 16)}


def _frag_index(CO: int, CI: int, numel: int, entry) -> torch.Tensor:
    """Build the gather index mapping weight.flatten() -> w_frags layout
    [CO/16][nK][64][8]; index `numel` means 'zero' (the caller appends a
    zero element to the flat weight). `entry(o, k)` returns the flat
    weight index for output channel o, im2col position k, or None."""
    S = 5 * CI
    Sp = (S + 7) & ~7
    K = 5 * Sp
    nK = (K + 31) // 32
    cot = CO // 16
    idx = torch.full((cot, nK, 64, 8), numel, dtype=torch.int64)
    for ct in range(cot):
        for km in range(nK):
            for lane in range(64):
                q, n = lane >> 4, lane & 15
                o = ct * 16 + n
                for j in range(8):
                    k = km * 32 + q * 8 + j
                    if k >= K:
                        continue
                    kh, jj = divmod(k, Sp)
                    if jj >= S or kh >= 5:
                        continue
                    kw, ci = divmod(jj, CI)
                    e = entry(o, kh, kw, ci)
                    if e is not None:
                        idx[ct, km, lane, j] = e
    return idx.reshape(-1)


def build_fwd_index(weight_shape) -> torch.Tensor:
    """weight [CO][CIr][5][5] (torch OIHW), CI zero-padded to mult of 4."""
    CO, CIr, KH, KW = weight_shape
    CI = (CIr + 3) & ~3
    numel = CO * CIr * KH * KW

    def entry(o, kh, kw, ci):
        if ci >= CIr:
            return None
        return ((o * CIr + ci) * KH + kh) * KW + kw

    return _frag_index(CO, CI, numel, entry)


def build_c1_fwd_index(weight_shape) -> torch.Tensor:
    """Gather table of k_conv5c1_pool's two B fragments, [2][64][8], for
    a [16][1][5][5] weight: K-slot k = kh*8 + kw, so lane (q, n) of chunk
    km holds w[n][0][4*km + q][0..4] and three dead slots; kh > 4 (chunk
    1, q >= 1) is dead too. Dead slots index the zero element."""
    CO, CIr, KH, KW = weight_shape
    assert (CIr, CO, KH, KW) == _C1_SHAPE + (5, 5), weight_shape
    km, lane, j = torch.meshgrid(torch.arange(2), torch.arange(64),
                                 torch.arange(8), indexing="ij")
    kh, n = km * 4 + (lane >> 4), lane & 15
    live = (kh < KH) & (j < KW)
    idx = torch.where(live, (n * KH + kh) * KW + j,
                      torch.full_like(j, CO * KH * KW))
    return idx.reshape(-1)


def build_dgrad_index(weight_shape) -> torch.Tensor:
    """Data-grad pass: roles swap (CI'=CO, CO'=CIr padded to 16) and the
    kernel is spatially flipped: W'[o'=ci][kh][kw][ci'=o] =
    W[o][ci][4-kh][4-kw]."""
    CO, CIr, KH, KW = weight_shape
    COp = (CIr + 15) & ~15
    numel = CO * CIr * KH * KW

    def entry(op, kh, kw, cip):
        # op: output channel of the dgrad conv = original input channel
        if op >= CIr:
            return None
        o, ci = cip, op
        return ((o * CIr + ci) * KH + (4 - kh)) * KW + (4 - kw)

    return _frag_index(COp, CO, numel, entry)


def build_wrw_unpack_index(weight_shape):
    """Gather index from the wrw kernel slab [T16][CO] back to OIHW;
    returns (index, T16). The last 16 slab rows are the fused-bias tile.

    CI=16: slot = (kh*5+kw)*16 + ci                    (25 tap tiles)
    CI=4 (kh-interleaved): slot = (kw*2 + kh//4)*16 + (kh%4)*4 + ci
    (10 tap tiles; 38% of the 160 slots are dead kh>4 padding, dropped
    here).
    """
    CO, CIr, KH, KW = weight_shape
    CI = (CIr + 3) & ~3
    if (CI, CO) not in _WRW_SHAPES:
        raise ValueError("no wrw kernel serves weight shape %s"
                         % (tuple(weight_shape),))
    o, ci, kh, kw = torch.meshgrid(torch.arange(CO), torch.arange(CIr),
                                   torch.arange(KH), torch.arange(KW),
                                   indexing="ij")
    if CI == 4:
        slot, tiles = (kw * 2 + kh // 4) * 16 + (kh % 4) * 4 + ci, 10
    else:
        slot, tiles = (kh * 5 + kw) * 16 + ci, 25
    return (slot * CO + o).reshape(-1), (tiles + 1) * 16


def _wrw_slab_sum(xb_padded: torch.Tensor, go: torch.Tensor, T16: int,
                  mask: torch.Tensor = None) -> torch.Tensor:
    """The wrw4 / wrw16 kernel's partial slabs summed over the
    workgroups: fp32 [T16][CO], tap rows in the kernel's slot order and
    the fused bias in row T16-16. With `mask`, `go` is the max-POOLED
    gradient and mask its argmax codes: the kernel unpools while staging
    (same slabs, same sums, bit-identical result)."""
    from geomx_amd import _geops
    N, CI, Hi, Wi = xb_padded.shape
    CO = go.shape[1]
    Ho, Wo = (Hi - 4, Wi - 4) if mask is not None else go.shape[2:]
    n_blocks = N * ((Ho + 3) // 4)
    n_wg = min(_WRW_NWG, n_blocks)
    # both kernels write every row of every slab (wrw4 zeroes its dead
    # rows in the flush), so nothing has to be cleared first
    part = torch.empty(n_wg, T16, CO, dtype=torch.float32,
                       device=go.device)
    if mask is not None:
        _geops.conv5_wrw_unpool_nhwc(xb_padded, go, mask, part, N, Hi, Wi,
                                     Ho, Wo, CI, CO, n_wg)
    else:
        _geops.conv5_wrw_nhwc(xb_padded, go, part, N, Hi, Wi, Ho, Wo, CI,
                              CO, n_wg)
    return part.sum(dim=0)


def wrw_via_kernel(xb_padded: torch.Tensor, go: torch.Tensor,
                   unpack_idx: torch.Tensor, T16: int, weight_shape,
                   want_bias: bool = False, mask: torch.Tensor = None):
    """Run the custom wrw kernel; returns dW in OIHW fp32 (and, with
    want_bias, the bias gradient the kernel fused via its all-ones tap
    tile — slab row T16-16). `mask` as in _wrw_slab_sum."""
    full = _wrw_slab_sum(xb_padded, go, T16, mask)
    dw = full.reshape(-1)[unpack_idx].reshape(weight_shape)
    if want_bias:
        return dw, full[T16 - 16]
    return dw


def wrw_into_sinks(xb_padded: torch.Tensor, go: torch.Tensor,
                   unpack_idx: torch.Tensor, T16: int, weight: torch.Tensor,
                   w_sink, b_sink, want_bias: bool,
                   mask: torch.Tensor = None):
    """The wrw4 / wrw16 gradients written where the trainer consumes
    them (gradsink.py): the same slabs and the same ATen sum over them as
    wrw_via_kernel, then ONE launch of k_conv5_wrw_finalize in place of
    the gather, the reshape and autograd's two `0 + x` accumulations. It
    writes the weight gradient into the weight's span (the parameter's
    own strides, OIHW or channels_last) and the bias gradient into the
    bias's span, or into a fresh tensor where the bias has no armed
    sink. Returns (grad_w, grad_b), or None where the weight's sink
    hands out no span (none attached, or spent): the caller then runs
    wrw_via_kernel."""
    if w_sink is None or weight.dtype != torch.float32:
        return None
    gw = w_sink.take()
    if gw is None:
        return None
    from geomx_amd import _geops
    gb = None
    if want_bias:
        gb = None if b_sink is None else b_sink.take()
        if gb is None:
            gb = torch.empty(weight.shape[0], dtype=torch.float32,
                             device=go.device)
    full = _wrw_slab_sum(xb_padded, go, T16, mask)
    _geops.conv5_wrw_finalize(full, unpack_idx, gw, gb, weight.shape[0],
                              weight.shape[1], T16)
    return gw, gb


def wrw1_via_kernel(x: torch.Tensor, go: torch.Tensor,
                    mask: torch.Tensor = None, table: torch.Tensor = None):
    """(dW [16][1][5][5], db [16]) in fp32 from k_conv5c1_wrw: x is the
    [N][1][H][W] input, fp32 or bf16, read as it is, or uint8 with its
    bf16 [1][256] `table`; go the NHWC bf16 gradient, or with `mask` the
    pooled gradient and its argmax codes. Slab rows 0..24 are the taps
    kh*5+kw, row 25 is the bias."""
    from geomx_amd import _geops
    N, _, H, W = x.shape
    n_wg = min(_WRW_NWG, N * ((H - 4 + 1) // 2))
    part = torch.empty(n_wg, 32, 16, dtype=torch.float32, device=x.device)
    if mask is not None:
        _geops.conv5c1_wrw_unpool(x, go, mask, part, N, H, W, 0, table)
    else:
        _geops.conv5c1_wrw(x, go, part, N, H, W, 0, table)
    full = part.sum(dim=0)
    return full[:25].T.reshape(16, 1, 5, 5), full[25]


# ---------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------

Conv5Plan = namedtuple("Conv5Plan", "fwd dgrad wrw")
_ALL_ATEN = Conv5Plan("aten", "aten", "aten")


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def plan_conv5(weight_shape, H: int, W: int, pooled: bool = False,
               enabled_shapes=DEFAULT_ENABLED,
               native: bool = True) -> Conv5Plan:
    """Route of each op of a 5x5 stride-1 pad-0 conv stage on an
    [N][CIr][H][W] input, from geometry alone:

        fwd    'pool' | 'pool1' | 'direct' | 'aten'
        dgrad  'lds_pad4' | 'direct_padded' | 'aten'
        wrw    'wrw4' | 'wrw16' | 'wrw1' | 'aten'   (weight + bias gradient)

    The predicates restate the launch tables of geops_conv5_nhwc,
    geops_conv5_pool_nhwc (conv.hip) and geops_conv5_wrw{4,16}_nhwc
    (convwrw2.hip) and geops_conv5c1_{pool,wrw} (conv1c.hip): each LDS kernel is compiled for a fixed staging
    width and serves a row only while tiles*tile_width + 4 halo pixels
    fit in it. The bindings raise on anything outside those tables, so
    drift between this function and the launchers fails loudly."""
    CO, CIr = weight_shape[0], weight_shape[1]
    if not native or H < 5 or W < 5:
        return _ALL_ATEN
    CI = (CIr + 3) & ~3
    Ho, Wo = H - 4, W - 4

    # the grayscale first layer: kernels of its own on the one-channel
    # row image, even W up to 228; a first layer gets no dgrad kernel
    if (CIr, CO) == _C1_SHAPE:
        if W % 2 or not 6 <= W <= _C1_MAXW:
            return _ALL_ATEN
        return Conv5Plan("pool1" if pooled and Ho % 2 == 0 else "aten",
                         "aten", "wrw1")

    # pool16 (CI=16) stages 120 pixels; CI=4 has the LDS kernel up to
    # 232 and the register-only k_conv5_pool_nhwc<4> beyond
    if (pooled and (CI, CO) in _POOL_SHAPES and Ho % 2 == 0 and W % 2 == 0
            and (CI == 4 or _ceil(Wo, 16) + 4 <= 120)):
        fwd = "pool"
    elif (not pooled and (CI, CO) in _SUPPORTED_FWD
          and (CI, CO) in enabled_shapes):
        # a pooled stage off the fused kernel pools an UNROUNDED conv
        # (_Conv5Fn), which the bf16-output direct kernel cannot give
        fwd = "direct"
    else:
        fwd = "aten"

    # the data gradient is a conv with CI' = CO, CO' = CIr padded to 16,
    # over grad_out with a 4-pixel zero border, W output pixels per row
    dshape = (CO, (CIr + 15) & ~15)
    if dshape == (32, 16) and _ceil(W, 16) + 4 <= 232:
        dgrad = "lds_pad4"
    elif dshape in _SUPPORTED_DGRAD:
        dgrad = "direct_padded"
    else:
        dgrad = "aten"

    # K windows of 32 gout pixels; wrw4 stages 2-pixel (16 B) granules
    wrw = "aten"
    if (CI, CO) in _WRW_SHAPES and _ceil(Wo, 32) + 4 <= 232:
        if CI == 16:
            wrw = "wrw16"
        elif W % 2 == 0:
            wrw = "wrw4"
    return Conv5Plan(fwd, dgrad, wrw)


_Conv5Index = namedtuple("_Conv5Index", "fwd dgrad wrw t16")
_index_cache = {}


def _conv5_indices(weight_shape, device) -> _Conv5Index:
    """The fwd / dgrad / wrw gather indices of a weight shape on a
    device, built once and shared by every module of that shape."""
    key = (tuple(weight_shape), torch.device(device))
    ent = _index_cache.get(key)
    if ent is None:
        CO, CIr = key[0][:2]
        wrw, t16 = (None, 0)
        if (CIr, CO) == _C1_SHAPE:
            ent = _index_cache[key] = _Conv5Index(
                build_c1_fwd_index(key[0]).to(device), None, None, 0)
            return ent
        if (((CIr + 3) & ~3), CO) in _WRW_SHAPES:
            wrw, t16 = build_wrw_unpack_index(key[0])
            wrw = wrw.to(device)
        ent = _Conv5Index(build_fwd_index(key[0]).to(device),
                          build_dgrad_index(key[0]).to(device), wrw, t16)
        _index_cache[key] = ent
    return ent


# ---------------------------------------------------------------------
# the steps shared by every route
# ---------------------------------------------------------------------

def _nhwc_bf16(x: torch.Tensor) -> torch.Tensor:
    """Input as NHWC bf16, channels zero-padded to a multiple of 4
    (conv1: 3 -> 4 in one pad kernel; any other count through F.pad).
    The flagship conv1 stage does not come here: on the 'pool' route an
    fp32 3-channel image goes to the forward kernel as it is
    (_x32_operand), and that kernel writes this tensor's bits itself."""
    N, CIr, Hi, Wi = x.shape
    if CIr % 4 == 0:
        return x.to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
    if CIr != 3:
        return F.pad(x.to(torch.bfloat16), (0, 0, 0, 0, 0, -CIr % 4)) \
            .contiguous(memory_format=torch.channels_last)
    from geomx_amd import _geops
    xc = x.contiguous(memory_format=torch.channels_last)
    xb = torch.empty(N, 4, Hi, Wi, dtype=torch.bfloat16, device=x.device,
                     memory_format=torch.channels_last)
    _geops.pad_ch3to4_nhwc(xc, xb, N * Hi * Wi)
    return xb


def _x32_operand(x: torch.Tensor, plan: Conv5Plan):
    """The caller's image as conv5_pool_x32_nhwc reads it, or None where
    that kernel does not serve it, from facts about the tensor alone:
    fwd 'pool' on a CUDA fp32 3-channel image whose rows are whole 16 B
    granules (12 * Wi bytes: Wi % 4 == 0, 16 B aligned base), dense in
    channels_last, and fit the 232-pixel row image of the LDS kernel
    (wider rows run the register-only forward, which has no fp32 form).
    Everything else takes _nhwc_bf16 and the pad kernel."""
    if not (plan.fwd == "pool" and x.is_cuda and x.dtype == torch.float32
            and x.shape[1] == 3 and x.shape[3] % 4 == 0
            and _ceil(x.shape[3] - 4, 16) + 4 <= 232):
        return None
    xc = x.detach().contiguous(memory_format=torch.channels_last)
    return xc if xc.data_ptr() % 16 == 0 else None


def to_tensor_table(channels: int, mean=None, std=None) -> torch.Tensor:
    """The [channels][256] fp32 table of ToTensor, v -> v / 255, followed
    where `mean` / `std` (one value per channel) are given by the
    normalisation (v / 255 - mean[c]) / std[c]."""
    t = (torch.arange(256, dtype=torch.float32) / 255).repeat(channels, 1)
    if mean is not None:
        t = t - torch.as_tensor(mean, dtype=torch.float32).reshape(-1, 1)
    if std is not None:
        t = t / torch.as_tensor(std, dtype=torch.float32).reshape(-1, 1)
    return t.contiguous()


def table_gather(table: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The fp32 image a uint8 image [N][C][H][W] stands for under a
    [C][256] table: out[n][c][h][w] = table[c][x[n][c][h][w]], in x's
    memory format. This is the definition of a stage with an
    input_table; the kernels that read the bytes give its bits."""
    C = x.shape[1]
    idx = x.long() + 256 * torch.arange(C, device=x.device).view(1, C, 1, 1)
    out = torch.take(table.to(x.device).float().contiguous(), idx)
    if not x.is_contiguous() and \
            x.is_contiguous(memory_format=torch.channels_last):
        out = out.contiguous(memory_format=torch.channels_last)
    return out


def _u8_operand(x: torch.Tensor, plan: Conv5Plan):
    """A uint8 image as the table kernels read it, or None where they do
    not serve it, from facts about the tensor alone. 3 channels: fwd
    'pool' on a CUDA tensor dense in channels_last whose rows are whole
    12-byte items (Wi % 4 == 0) on a 4 B aligned base and fit the
    232-pixel row image (conv5_pool_u8_nhwc). 1 channel: the 'wrw1'
    plan's widths on a contiguous CUDA tensor with a 2 B aligned base
    (conv5c1_*). Everything else is expanded by table_gather."""
    if not (x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4):
        return None
    if x.shape[1] == 1 and plan.wrw == "wrw1":
        ok = x.is_contiguous() and x.data_ptr() % 2 == 0
    else:
        ok = (plan.fwd == "pool" and x.shape[1] == 3
              and x.is_contiguous(memory_format=torch.channels_last)
              and x.shape[3] % 4 == 0
              and _ceil(x.shape[3] - 4, 16) + 4 <= 232
              and x.data_ptr() % 4 == 0)
    return x.detach() if ok else None


def _w_frags(weight: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Regather the OIHW weight into per-lane MFMA B-fragment order."""
    wb = weight.detach().to(torch.bfloat16).reshape(-1)
    wz = torch.cat([wb, wb.new_zeros(1)])
    return wz[idx].contiguous()


def _pack_frags(weight: torch.Tensor, *idx):
    """Fragment-order bf16 copies of the weight for one or two gather
    tables, as a list: one launch of k_conv5_pack_frags for an fp32
    weight on the GPU, _w_frags per table on the CPU, without the
    extension, or for another dtype (same values either way)."""
    w = weight.detach()
    if w.is_cuda and w.dtype == torch.float32 and native_available():
        from geomx_amd import _geops
        return _geops.conv5_pack_frags(w.contiguous(), *idx)
    return [_w_frags(w, i) for i in idx]


def _empty_nhwc(N, C, H, W, device) -> torch.Tensor:
    return torch.empty(N, C, H, W, dtype=torch.bfloat16, device=device,
                       memory_format=torch.channels_last)


Conv5Unpool = namedtuple("Conv5Unpool", "dgrad wrw")


def unpool_fusable(plan: Conv5Plan) -> Conv5Unpool:
    """Which backward ops of a fwd='pool' stage take the POOLED grad_out
    plus the argmax mask directly (their kernels do the max-pool
    backward while staging gout into LDS). Every other route reads the
    full-resolution gradient relu_maxpool2_bwd scatters."""
    return Conv5Unpool(dgrad=plan.dgrad == "lds_pad4",
                       wrw=plan.wrw in ("wrw4", "wrw16", "wrw1"))


def _pooled_backward(fuse: Conv5Unpool, need_x: bool, need_w: bool, gp,
                     mask, scatter, dgrad, wrw):
    """Backward of a fused-pool stage. `dgrad(go, mask)` / `wrw(go,
    mask)` run one consumer, on the pooled gradient when given a mask
    and on the full-resolution one when mask is None. `scatter()` builds
    the full-resolution gradient; it runs at most once, and only when a
    needed consumer cannot take the pooled form."""
    full = []

    def go_full():
        if not full:
            full.append(scatter())
        return full[0]

    grad_x = grad_wb = None
    if need_x:
        grad_x = dgrad(gp, mask) if fuse.dgrad else dgrad(go_full(), None)
    if need_w:
        grad_wb = wrw(gp, mask) if fuse.wrw else wrw(go_full(), None)
    return grad_x, grad_wb


def _dgrad(route, go, x_real, weight, idx, mask=None, w_frags=None):
    """grad_x of the conv from grad_out `go` (NHWC bf16); with `mask`
    (route 'lds_pad4' only) `go` is the pooled gradient. `w_frags`: the
    dgrad fragments where the forward packed them already."""
    N, CIr, Hi, Wi = x_real.shape
    CO = go.shape[1]
    Ho, Wo = Hi - 4, Wi - 4
    if mask is not None:
        assert route == "lds_pad4", route
        from geomx_amd import _geops
        COp = (CIr + 15) & ~15
        gx = _empty_nhwc(N, COp, Hi, Wi, go.device)
        if w_frags is None:
            w_frags, = _pack_frags(weight, idx.dgrad)
        _geops.conv5_dgrad_unpool_nhwc(go, mask, w_frags, gx, N, Ho + 8,
                                       Wo + 8, Hi, Wi, CO, COp)
        return gx[:, :CIr] if COp != CIr else gx
    if route == "aten":
        return torch.ops.aten.convolution_backward(
            go, x_real, weight.detach().to(torch.bfloat16), None, [1, 1],
            [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    from geomx_amd import _geops
    COp = (CIr + 15) & ~15
    if w_frags is None:
        w_frags, = _pack_frags(weight, idx.dgrad)
    pad = 4
    if route == "direct_padded":
        # physical zero border: the direct kernel is interior-only (an
        # in-kernel masked path cost it 256 VGPRs -> 1 wave/SIMD); the
        # LDS kernel instead materialises the border while staging
        go = F.pad(go, (4, 4, 4, 4)) \
            .contiguous(memory_format=torch.channels_last)
        pad = 0
    gx = _empty_nhwc(N, COp, Hi, Wi, go.device)
    _geops.conv5_nhwc(go, w_frags, torch.Tensor(), gx, N, Ho + 8, Wo + 8,
                      Hi, Wi, CO, COp, pad)
    return gx[:, :CIr] if COp != CIr else gx


def _wrw(route, go, xb, x_real, weight, idx, has_bias, mask=None,
         table=None, sinks=(None, None)):
    """(grad_w, grad_b) in the weight's dtype; grad_b None without bias.
    With `mask` (custom routes only) `go` is the pooled gradient.
    `sinks`: the gradient sinks of weight and bias the forward recorded;
    on the wrw4 / wrw16 routes an armed weight sink gets the gradients
    written into the spans (wrw_into_sinks)."""
    if route in ("wrw4", "wrw16"):
        done = wrw_into_sinks(xb, go, idx.wrw, idx.t16, weight, sinks[0],
                              sinks[1], has_bias, mask)
        if done is not None:
            return done
    if route == "wrw1":
        # xb: the caller's tensor (uint8 with its table)
        gw, gb = wrw1_via_kernel(xb, go, mask, table)
    elif route == "aten":
        assert mask is None
        _, gw, gb = torch.ops.aten.convolution_backward(
            go, x_real, weight.detach().to(torch.bfloat16),
            [weight.shape[0]] if has_bias else None, [1, 1], [0, 0],
            [1, 1], False, [0, 0], 1, [False, True, has_bias])
    else:
        gw, gb = wrw_via_kernel(xb, go, idx.wrw, idx.t16, weight.shape,
                                want_bias=True, mask=mask)
    return (gw.to(weight.dtype),
            gb.to(weight.dtype) if has_bias else None)


def _out_dtype(x: torch.Tensor) -> torch.dtype:
    # outside autocast (fp32 graphs) the downstream layers expect the
    # input dtype back; under autocast bf16 IS the compute dtype. A uint8
    # image only comes here with its table: it stands for an fp32 image
    if x.dtype == torch.bfloat16 or torch.is_autocast_enabled():
        return torch.bfloat16
    return torch.float32 if x.dtype == torch.uint8 else x.dtype


class _Conv5Fn(torch.autograd.Function):
    """One conv stage under a Conv5Plan. fwd='pool' is conv5 + bias +
    ReLU + 2x2 maxpool in ONE kernel: the full-resolution conv output
    (1.55 GB at the bench shape) never exists, and in backward the wrw
    and lds_pad4 kernels read the pooled gradient through the recorded
    argmax-quadrant mask (unpool_fusable); the other routes get it
    scattered to full resolution first (relu_maxpool2_bwd). fwd='aten' with a custom wrw is the split
    backward (0.21 ms vs the 1.61 ms igemm MIOpen picks in-step).
    With `pooled`, fwd='aten' returns the conv in fp32: the fused kernel
    argmaxes its fp32 accumulators, and the eager ReLU + max-pool that
    replaces it must pick the same pixels, not those that win after
    rounding to bf16 (ties there would route gradient elsewhere).
    `table` (bf16 [CIr][256]) comes with a uint8 x that _u8_operand
    serves: the kernels that would read the fp32 image read the bytes
    and the table instead, and give the same bits."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan, idx, pooled, x32_input=True,
                table=None):
        N, CIr, Hi, Wi = x.shape
        CO = weight.shape[0]
        Ho, Wo = Hi - 4, Wi - 4
        c1 = "pool1" == plan.fwd or "wrw1" == plan.wrw
        x32 = _x32_operand(x, plan) if x32_input else None
        if table is not None and not c1:
            x32 = x   # the 3-channel uint8 image takes the fp32 image's place
        if x32 is not None:
            # the forward kernel reads the fp32 image and writes xb, the
            # bits of _nhwc_bf16(x), for the weight gradient (the only
            # backward op that reads the input's values; without one no
            # copy is written and backward keeps the shape alone)
            xb = None
            if ctx.needs_input_grad[1] or (bias is not None and
                                           ctx.needs_input_grad[2]):
                xb = _empty_nhwc(N, 4, Hi, Wi, x.device)
        elif c1:
            # the one-channel kernels read the caller's tensor (they round
            # fp32 while staging); it is what backward saves
            xb = x if (x.dtype in (torch.float32, torch.bfloat16)
                       or table is not None) else x.to(torch.bfloat16)
            xb = xb.detach().contiguous()
        elif plan.fwd == "aten" and plan.wrw == "aten":
            xb = x.to(torch.bfloat16)
        else:
            xb = _nhwc_bf16(x)
        mask = w_dfrags = None
        if plan.fwd == "aten":
            if table is not None:   # c1, uint8: the bf16 image it stands for
                xa = torch.take(table, xb.long())
            else:
                xa = xb.to(torch.bfloat16) if c1 else xb[:, :CIr]
            args = [xa,
                    weight.detach().to(torch.bfloat16),
                    None if bias is None else bias.detach().to(torch.bfloat16)]
            if pooled:
                with torch.autocast("cuda", enabled=False):
                    out = F.conv2d(*[a if a is None else a.float()
                                     for a in args])
            else:
                out = F.conv2d(*args)
        else:
            from geomx_amd import _geops
            # one launch packs the forward fragments and, where backward
            # will run a native data gradient, its fragments too
            if plan.dgrad != "aten" and ctx.needs_input_grad[0]:
                w_frags, w_dfrags = _pack_frags(weight, idx.fwd, idx.dgrad)
            else:
                w_frags, = _pack_frags(weight, idx.fwd)
            b = bias.detach().float() if bias is not None else torch.Tensor()
            if plan.fwd == "pool1":
                out = _empty_nhwc(N, CO, Ho // 2, Wo // 2, x.device)
                mask = torch.empty(out.numel(), dtype=torch.uint8,
                                   device=x.device)
                _geops.conv5c1_pool(xb, w_frags, b, out, mask, N, Hi, Wi, 0,
                                    table)
            elif plan.fwd == "pool":
                out = _empty_nhwc(N, CO, Ho // 2, Wo // 2, x.device)
                mask = torch.empty(out.numel(), dtype=torch.uint8,
                                   device=x.device)
                if table is not None:
                    _geops.conv5_pool_u8_nhwc(
                        x32, table, w_frags, b, out, mask,
                        torch.Tensor() if xb is None else xb, N, Hi, Wi, Ho,
                        Wo, CO)
                elif x32 is not None:
                    _geops.conv5_pool_x32_nhwc(
                        x32, w_frags, b, out, mask,
                        torch.Tensor() if xb is None else xb, N, Hi, Wi, Ho,
                        Wo, CO)
                else:
                    _geops.conv5_pool_nhwc(xb, w_frags, b, out, mask, N, Hi,
                                           Wi, Ho, Wo, xb.shape[1], CO)
            else:
                out = _empty_nhwc(N, CO, Ho, Wo, x.device)
                _geops.conv5_nhwc(xb, w_frags, b, out, N, Hi, Wi, Ho, Wo,
                                  xb.shape[1], CO, 0)
        # xb keeps its padded channels: the custom wrw wants CI % 4 == 0,
        # the ATen routes take the view xb[:, :CIr]. On the fp32-image
        # route xb is the forward kernel's side output (or None).
        # the weight is saved too, so autograd's version check covers the
        # dgrad fragments against an in-place change before backward
        ctx.save_for_backward(xb, weight, mask)
        ctx.w_dfrags = w_dfrags
        ctx.table = table   # a constant of the stage: no gradient, no version
        ctx.plan, ctx.idx = plan, idx
        ctx.has_bias = bias is not None
        ctx.sinks = (gradsink.sink_of(weight),
                     None if bias is None else gradsink.sink_of(bias))
        ctx.CIr = CIr
        ctx.x_shape = tuple(x.shape)
        if out.dtype == torch.float32:  # the module rounds after pooling
            return out
        return out.to(_out_dtype(x))

    @staticmethod
    def backward(ctx, grad_out):
        xb, weight, mask = ctx.saved_tensors
        plan, idx = ctx.plan, ctx.idx
        if xb is None:   # no weight gradient: the dgrad wants the shape
            x_real = torch.empty(ctx.x_shape, dtype=torch.bfloat16,
                                 device="meta")
        else:
            x_real = xb[:, :ctx.CIr]
        if plan.wrw == "wrw1" and ctx.needs_input_grad[0]:
            x_real = xb.to(torch.bfloat16)   # the ATen dgrad's operand
        go = grad_out.to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and
                                             ctx.needs_input_grad[2])

        def dgrad(g, m):
            return _dgrad(plan.dgrad, g, x_real, weight, idx, m,
                          ctx.w_dfrags)

        def wrw(g, m):
            # the spans are written only where autograd asked for the
            # weight's gradient and will accumulate what is returned
            sinks = ctx.sinks if ctx.needs_input_grad[1] else (None, None)
            if not (ctx.has_bias and ctx.needs_input_grad[2]):
                sinks = (sinks[0], None)
            return _wrw(plan.wrw, g, xb, x_real, weight, idx, ctx.has_bias,
                        m, ctx.table, sinks)

        if mask is not None:
            # fused-pool stage: `go` is the pooled gradient. The wrw and
            # lds_pad4 kernels unpool it while staging; only a consumer
            # on another route gets the scattered full-resolution tensor
            def scatter():
                from geomx_amd import _geops
                N, _, Hi, Wi = ctx.x_shape
                CO = weight.shape[0]
                full = _empty_nhwc(N, CO, Hi - 4, Wi - 4, go.device)
                _geops.relu_maxpool2_bwd(go, mask, full, N, CO, Hi - 4,
                                         Wi - 4)
                return full

            grad_x, grad_wb = _pooled_backward(
                unpool_fusable(plan), need_x, need_w, go, mask, scatter,
                dgrad, wrw)
        else:
            grad_x = dgrad(go, None) if need_x else None
            grad_wb = wrw(go, None) if need_w else None
        grad_w, grad_b = grad_wb if grad_wb is not None else (None, None)
        return grad_x, grad_w, grad_b, None, None, None, None, None


class GeoConv5(torch.nn.Conv2d):
    """nn.Conv2d drop-in (kernel 5, stride 1, pad 0) whose forward, data
    gradient and weight gradient each run on a gfx950 kernel where one
    serves the geometry (plan_conv5) and on ATen elsewhere.
    `enabled_shapes` selects the (CI, CO) whose forward takes the direct
    kernel; routes are fixed per input shape at first use.
    `input_table`, a finite fp32 [in_channels][256] tensor (see
    to_tensor_table), makes the stage take uint8 images: it computes what
    it computes for the fp32 image table[c][x] (table_gather), bit for
    bit, and the input gets no gradient. Without a table, or for an input
    of another dtype, nothing changes."""

    _POOLED = False

    def __init__(self, in_channels, out_channels, enabled_shapes=None,
                 input_table=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size=5, **kw)
        if input_table is not None:
            input_table = torch.as_tensor(input_table, dtype=torch.float32)
            if tuple(input_table.shape) != (in_channels, 256) or \
                    not torch.isfinite(input_table).all():
                raise ValueError("input_table must be a finite [%d][256] "
                                 "tensor" % in_channels)
            input_table = input_table.detach().clone().contiguous()
        self.register_buffer("input_table", input_table, persistent=False)
        self._table_bf16 = None   # (key, the kernels' copy)
        self.enabled_shapes = (DEFAULT_ENABLED if enabled_shapes is None
                               else enabled_shapes)
        # False keeps an fp32 3-channel image on the pad kernel in front
        # of the forward (the route every other input takes)
        self.x32_input = True
        self._routes = {}  # (input shape, device) -> (plan, indices)

    def grad_sink_parameters(self):
        """The parameters whose gradient the backward can write in place
        (gradsink.py): weight and bias, on the wrw4 / wrw16 routes. On
        every other route they arrive through autograd and the trainer's
        hook puts them into the span."""
        return (self.weight,) if self.bias is None \
            else (self.weight, self.bias)

    def _route(self, x):
        key = (x.shape, x.device)
        ent = self._routes.get(key)
        if ent is None:
            native = (x.is_cuda and x.dim() == 4 and native_available()
                      and self.stride == (1, 1) and self.padding == (0, 0)
                      and self.dilation == (1, 1) and self.groups == 1)
            plan = plan_conv5(tuple(self.weight.shape), x.shape[-2],
                              x.shape[-1], self._POOLED,
                              self.enabled_shapes, native)
            idx = None if plan == _ALL_ATEN else \
                _conv5_indices(self.weight.shape, x.device)
            ent = self._routes[key] = (plan, idx)
        return ent

    def _input(self, x, plan):
        """(x, table): a uint8 image of a stage with a table either stays
        as it is, with the bf16 copy of the table its kernels look it up
        in, or becomes the fp32 image it stands for. The copy is rounded
        to nearest even as cf2bf rounds (the table is finite), once per
        table tensor."""
        t = self.input_table
        if t is None or x.dtype != torch.uint8 or x.dim() != 4:
            return x, None
        if plan == _ALL_ATEN or _u8_operand(x, plan) is None:
            return table_gather(t, x), None
        # (the cache holds the table tensor itself: a new buffer, an
        # in-place change or another device make a new copy)
        c = self._table_bf16
        if c is None or c[0] is not t or c[1:3] != (t._version, x.device):
            c = self._table_bf16 = (t, t._version, x.device,
                                    t.to(x.device, torch.bfloat16)
                                    .contiguous())
        return x.detach(), c[3]

    def _conv(self, x, plan, idx, table=None):
        if plan == _ALL_ATEN:
            return torch.nn.Conv2d.forward(self, x)
        return _Conv5Fn.apply(x, self.weight, self.bias, plan, idx,
                              self._POOLED, self.x32_input, table)

    def forward(self, x):
        plan, idx = self._route(x)
        x, table = self._input(x, plan)
        return self._conv(x, plan, idx, table)


class GeoConv5Pool(GeoConv5):
    """Drop-in for GeoConv5 -> ReLU -> MaxPool2d(2,2): one fused kernel
    where plan_conv5 routes the forward to 'pool', otherwise an ATen
    conv followed by eager ReLU + max-pool (over the fp32 conv on the
    GPU, so both forms pool the same pixels). Parameters live on this
    module exactly as on GeoConv5 (state-dict compatible)."""

    _POOLED = True

    def forward(self, x):
        plan, idx = self._route(x)
        x, table = self._input(x, plan)
        y = self._conv(x, plan, idx, table)
        if plan.fwd in ("pool", "pool1"):
            return y
        y = F.max_pool2d(F.relu(y), 2, 2)
        return y if plan == _ALL_ATEN else y.to(_out_dtype(x))
