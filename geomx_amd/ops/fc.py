"""GeoFlattenLinear: Flatten + Linear on a channels_last feature map
whose backward runs in the K order the data already has (csrc/fc.hip).

nn.Linear behind nn.Flatten wants the features in (c, h, w) order. The
conv stack produces them in channels_last memory, (h, w, c) order, so
the eager pair copies the whole activation into NCHW order in forward
and its gradient back to channels_last in backward. The backward copy
is not needed: both backward GEMMs reduce over O or N, not over K, so
running them with K in (h, w, c) order only permutes their output
columns and every output element is the same sum in the same order.

  * forward: the same F.linear on the same flattened operands (the
    forward GEMM reduces over K; any other K order changes its
    rounding, and a training run amplifies that, so it keeps the NCHW
    order); only the flatten copy itself is a tiled transpose kernel
    (k_fc_flatten_nchw) instead of a strided elementwise copy;
  * both bf16 copies of the weight come from one read of the fp32
    master in forward (k_fc_w_pack2_bf16): the plain cast the GEMM
    takes, and, when the input needs a gradient, the cast-AND-permuted
    [O][HW][C] operand of the data-gradient GEMM, which rides on the
    autograd context to backward;
  * data gradient: dy @ Wp; the result is already the NHWC gradient the
    conv backward wants, returned as a channels_last view;
  * weight gradient: dy^T @ x on the channels_last activation as it
    is, then cast AND un-permuted to fp32 [O][C][HW], in place of the
    plain bf16 -> fp32 cast. Under a trainer that attached a gradient
    sink to the weight (geomx_amd/gradsink.py) the un-permute writes
    straight into the weight's span of the gradient bucket
    (k_fc_w_unpermute_into) and that view is the returned gradient;
    otherwise it is a fresh tensor (k_fc_w_unpermute_f32).

The module's parameters are exactly nn.Linear's (weight [O, C*H*W] in
NCHW-flatten order), so state dicts and checkpoints are interchangeable
with Flatten + Linear. Routing comes from shapes, dtypes and layout
alone (native_route); everything the kernels do not serve runs
F.linear(torch.flatten(x, 1), weight, bias) under plain autograd.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import gradsink
from . import native_available

FC_CHANNELS = 32   # k_fc_w_*: a pixel's channels are one 64 B record


def supported(C: int, O: int, N: int, HW: int) -> bool:
    """The launch table of geops_fc_w_* (fc.hip)."""
    return (C == FC_CHANNELS and 0 < O <= 65535 and N > 0
            and 0 < HW <= (1 << 24))


def native_route(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when the backward takes the NHWC route: a GPU tensor with the
    extension loaded, bf16 compute (autocast to bf16, or a bf16 input),
    a channels_last-dense 4-D input, an fp32 dense weight and a
    (C, O, N) the kernels serve."""
    if not (x.is_cuda and x.dim() == 4 and native_available()):
        return False
    if torch.is_autocast_enabled("cuda"):
        if torch.get_autocast_dtype("cuda") != torch.bfloat16 or \
                x.dtype not in (torch.bfloat16, torch.float32):
            return False
    elif x.dtype != torch.bfloat16:
        return False
    N, C, H, W = x.shape
    if not supported(C, weight.shape[0], N, H * W):
        return False
    if weight.dtype != torch.float32 or not weight.is_contiguous() \
            or weight.shape[1] != C * H * W:
        return False
    # dense in channels_last and NOT also NCHW-dense (H = W = 1 is
    # both): strides must be exactly (HWC, 1, WC, C)
    return x.stride() == (H * W * C, 1, W * C, C)


class _FlattenLinearFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias):
        from geomx_amd import _geops
        N, C, H, W = x.shape
        xf = x.detach().to(torch.bfloat16).permute(0, 2, 3, 1) \
            .reshape(N, H * W * C)         # a view: x is NHWC-dense
        # weight.to(bfloat16) and, if backward will want it, the
        # permuted data-gradient operand: one read of the fp32 weight
        wb, wp = _geops.fc_w_pack2_bf16(weight.detach(), weight.shape[0],
                                        C, H * W, ctx.needs_input_grad[0])
        # torch.flatten(x, 1) as a tiled transpose, the casts autocast
        # would make, then the same library GEMM on the same operands
        with torch.autocast("cuda", enabled=False):
            y = F.linear(_geops.fc_flatten_nchw(xf, N, C, H * W), wb,
                         None if bias is None
                         else bias.detach().to(torch.bfloat16))
        ctx.save_for_backward(xf)
        ctx.wp = wp
        ctx.sink = gradsink.sink_of(weight)
        ctx.geom = (N, C, H, W, weight.shape[0])
        ctx.x_dtype = x.dtype
        ctx.b_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, grad_out):
        from geomx_amd import _geops
        xf, = ctx.saved_tensors
        N, C, H, W, O = ctx.geom
        dy = grad_out.to(torch.bfloat16).contiguous()
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            # [N][HW*C] IS the NHWC gradient: hand it on as a
            # channels_last view, no copy
            grad_x = torch.mm(dy, ctx.wp).view(N, H, W, C).permute(0, 3, 1, 2) \
                .to(ctx.x_dtype)
        if ctx.needs_input_grad[1]:
            gp = torch.mm(dy.t(), xf)
            # the weight's span of the trainer's gradient bucket, once
            # per zero_grad(); returned so that autograd adopts it
            grad_w = None if ctx.sink is None else ctx.sink.take()
            if grad_w is not None:
                _geops.fc_w_unpermute_into(gp, grad_w, O, C, H * W)
            else:
                grad_w = _geops.fc_w_unpermute_f32(gp, O, C, H * W)
        if ctx.b_dtype is not None and ctx.needs_input_grad[2]:
            grad_b = dy.sum(0).to(ctx.b_dtype)
        return grad_x, grad_w, grad_b


class GeoFlattenLinear(torch.nn.Linear):
    """Drop-in for nn.Flatten() -> nn.Linear(C*H*W, O) that takes the
    4-D feature map."""

    def grad_sink_parameters(self):
        """The parameters whose gradient the backward can write in place
        (gradsink.py): the weight."""
        return (self.weight,)

    def forward(self, x):
        if native_route(x, self.weight):
            return _FlattenLinearFn.apply(x, self.weight, self.bias)
        return F.linear(torch.flatten(x, 1), self.weight, self.bias)
