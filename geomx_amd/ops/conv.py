"""GeoConv5 / GeoConv5Pool: 5x5 stride-1 convolution stages on the
hand-written gfx950 MFMA kernels (csrc/conv.hip, convwrw2.hip).

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
Whatever no kernel serves goes to ATen (same math, library kernels);
one op on ATen does not move the other two off the custom kernels.
"""

from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from . import native_available

_SUPPORTED_FWD = {(4, 16), (16, 32), (16, 16), (32, 32)}
_SUPPORTED_DGRAD = {(32, 16), (16, 16)}
_POOL_SHAPES = {(4, 16), (16, 32), (16, 16)}
_WRW_SHAPES = {(4, 16), (16, 32), (16, 16)}
_WRW_NWG = 768  # partial slabs (3 workgroups per CU)

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


def wrw_via_kernel(xb_padded: torch.Tensor, go: torch.Tensor,
                   unpack_idx: torch.Tensor, T16: int, weight_shape,
                   want_bias: bool = False, mask: torch.Tensor = None):
    """Run the custom wrw kernel; returns dW in OIHW fp32 (and, with
    want_bias, the bias gradient the kernel fused via its all-ones tap
    tile — slab row T16-16). With `mask`, `go` is the max-POOLED
    gradient and mask its argmax codes: the kernel unpools while
    staging (same slabs, same sums, bit-identical result)."""
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
    full = part.sum(dim=0)
    dw = full.reshape(-1)[unpack_idx].reshape(weight_shape)
    if want_bias:
        return dw, full[T16 - 16]
    return dw


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

        fwd    'pool' | 'direct' | 'aten'
        dgrad  'lds_pad4' | 'direct_padded' | 'aten'
        wrw    'wrw4' | 'wrw16' | 'aten'      (weight + bias gradient)

    The predicates restate the launch tables of geops_conv5_nhwc,
    geops_conv5_pool_nhwc (conv.hip) and geops_conv5_wrw{4,16}_nhwc
    (convwrw2.hip): each LDS kernel is compiled for a fixed staging
    width and serves a row only while tiles*tile_width + 4 halo pixels
    fit in it. The bindings raise on anything outside those tables, so
    drift between this function and the launchers fails loudly."""
    CO, CIr = weight_shape[0], weight_shape[1]
    if not native or H < 5 or W < 5:
        return _ALL_ATEN
    CI = (CIr + 3) & ~3
    Ho, Wo = H - 4, W - 4

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
    (conv1: 3 -> 4, one fused kernel)."""
    N, CIr, Hi, Wi = x.shape
    if CIr % 4 == 0:
        return x.to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
    assert CIr == 3, "channel pad kernel is 3 -> 4 only"
    from geomx_amd import _geops
    xc = x.contiguous(memory_format=torch.channels_last)
    xb = torch.empty(N, 4, Hi, Wi, dtype=torch.bfloat16, device=x.device,
                     memory_format=torch.channels_last)
    _geops.pad_ch3to4_nhwc(xc, xb, N * Hi * Wi)
    return xb


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
                       wrw=plan.wrw in ("wrw4", "wrw16"))


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


def _wrw(route, go, xb, x_real, weight, idx, has_bias, mask=None):
    """(grad_w, grad_b) in the weight's dtype; grad_b None without bias.
    With `mask` (custom routes only) `go` is the pooled gradient."""
    if route == "aten":
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
    # input dtype back; under autocast bf16 IS the compute dtype
    if x.dtype == torch.bfloat16 or torch.is_autocast_enabled():
        return torch.bfloat16
    return x.dtype


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
    rounding to bf16 (ties there would route gradient elsewhere)."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan, idx, pooled):
        N, CIr, Hi, Wi = x.shape
        CO = weight.shape[0]
        Ho, Wo = Hi - 4, Wi - 4
        if plan.fwd == "aten" and plan.wrw == "aten":
            xb = x.to(torch.bfloat16)
        else:
            xb = _nhwc_bf16(x)
        mask = w_dfrags = None
        if plan.fwd == "aten":
            args = [xb[:, :CIr], weight.detach().to(torch.bfloat16),
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
            if plan.fwd == "pool":
                out = _empty_nhwc(N, CO, Ho // 2, Wo // 2, x.device)
                mask = torch.empty(out.numel(), dtype=torch.uint8,
                                   device=x.device)
                _geops.conv5_pool_nhwc(xb, w_frags, b, out, mask, N, Hi, Wi,
                                       Ho, Wo, xb.shape[1], CO)
            else:
                out = _empty_nhwc(N, CO, Ho, Wo, x.device)
                _geops.conv5_nhwc(xb, w_frags, b, out, N, Hi, Wi, Ho, Wo,
                                  xb.shape[1], CO, 0)
        # xb keeps its padded channels: the custom wrw wants CI % 4 == 0,
        # the ATen routes take the view xb[:, :CIr]
        # the weight is saved too, so autograd's version check covers the
        # dgrad fragments against an in-place change before backward
        ctx.save_for_backward(xb, weight, mask)
        ctx.w_dfrags = w_dfrags
        ctx.plan, ctx.idx = plan, idx
        ctx.has_bias = bias is not None
        ctx.CIr = CIr
        if out.dtype == torch.float32:  # the module rounds after pooling
            return out
        return out.to(_out_dtype(x))

    @staticmethod
    def backward(ctx, grad_out):
        xb, weight, mask = ctx.saved_tensors
        plan, idx = ctx.plan, ctx.idx
        x_real = xb[:, :ctx.CIr]
        go = grad_out.to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and
                                             ctx.needs_input_grad[2])

        def dgrad(g, m):
            return _dgrad(plan.dgrad, g, x_real, weight, idx, m,
                          ctx.w_dfrags)

        def wrw(g, m):
            return _wrw(plan.wrw, g, xb, x_real, weight, idx, ctx.has_bias,
                        m)

        if mask is not None:
            # fused-pool stage: `go` is the pooled gradient. The wrw and
            # lds_pad4 kernels unpool it while staging; only a consumer
            # on another route gets the scattered full-resolution tensor
            def scatter():
                from geomx_amd import _geops
                N, _, Hi, Wi = xb.shape
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
        return grad_x, grad_w, grad_b, None, None, None


class GeoConv5(torch.nn.Conv2d):
    """nn.Conv2d drop-in (kernel 5, stride 1, pad 0) whose forward, data
    gradient and weight gradient each run on a gfx950 kernel where one
    serves the geometry (plan_conv5) and on ATen elsewhere.
    `enabled_shapes` selects the (CI, CO) whose forward takes the direct
    kernel; routes are fixed per input shape at first use."""

    _POOLED = False

    def __init__(self, in_channels, out_channels, enabled_shapes=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size=5, **kw)
        self.enabled_shapes = (DEFAULT_ENABLED if enabled_shapes is None
                               else enabled_shapes)
        self._routes = {}  # (input shape, device) -> (plan, indices)

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

    def _conv(self, x, plan, idx):
        if plan == _ALL_ATEN:
            return torch.nn.Conv2d.forward(self, x)
        return _Conv5Fn.apply(x, self.weight, self.bias, plan, idx,
                              self._POOLED)

    def forward(self, x):
        return self._conv(x, *self._route(x))


class GeoConv5Pool(GeoConv5):
    """Drop-in for GeoConv5 -> ReLU -> MaxPool2d(2,2): one fused kernel
    where plan_conv5 routes the forward to 'pool', otherwise an ATen
    conv followed by eager ReLU + max-pool (over the fp32 conv on the
    GPU, so both forms pool the same pixels). Parameters live on this
    module exactly as on GeoConv5 (state-dict compatible)."""

    _POOLED = True

    def forward(self, x):
        plan, idx = self._route(x)
        y = self._conv(x, plan, idx)
        if plan.fwd == "pool":
            return y
        y = F.max_pool2d(F.relu(y), 2, 2)
        return y if plan == _ALL_ATEN else y.to(_out_dtype(x))
