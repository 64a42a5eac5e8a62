"""Gradient sinks: let an op write a parameter's gradient where the
trainer consumes it.

GeoTrainer keeps every gradient in a flat fp32 bucket. For most
parameters the gradient is small and autograd's `grad += new` into the
bucket view costs nothing. For a parameter whose gradient is large, the
pair "clear the span, then add the freshly computed gradient into it" is
two passes over memory that compute `0 + x`. A sink removes both: the
op's backward asks the sink for the parameter's span of the bucket,
writes the gradient there itself and RETURNS that view as the gradient.
With `p.grad` undefined, autograd's AccumulateGrad adopts a returned
tensor that nothing else references without copying it, so `p.grad`
becomes the bucket span with the gradient already in it.

The protocol:

  * A module names the parameters it can write in place through
    `grad_sink_parameters()` (an iterable of its own parameters).
  * The trainer attaches a GradSink to each (`attach`), and in its
    `zero_grad()` sets `p.grad = None` and re-arms the sink instead of
    clearing the span.
  * The op's backward calls `sink.take()`: the first call after a
    `zero_grad()` returns a FRESH view of the span, every later call
    returns None until the next `zero_grad()`. A fresh view per call and
    no reference kept here, because AccumulateGrad adopts only a tensor
    it holds the sole reference to.
  * The span is handed out only while `p.grad` is None. As soon as the
    parameter has a gradient again, by any route, `p.grad` aliases the
    span and the sink is spent: `take()` checks `p.grad` itself, and the
    trainer disarms the sink wherever it re-attaches the view.
  * The op writes the complete gradient (every element; `+0` where the
    sum `0 + x` would have produced it) and returns the view. It must
    return it: other contributions to the same parameter (a second use
    of the module, a regulariser) are summed by autograd before the
    gradient reaches `p.grad`, which is why the op does not write
    behind autograd's back and return None.

Whatever autograd then does (adopt, clone, sum into another tensor),
the trainer's post-accumulate hook checks that `p.grad` lives at the
span's address and copies it there if not, so a sink never changes a
result; it removes passes on the route where adoption happens.
"""

from __future__ import annotations

import weakref
from typing import Optional

import torch

_ATTR = "_geo_grad_sink"


class GradSink:
    """One parameter's span of a gradient bucket, handed out once per
    zero_grad()."""

    __slots__ = ("_flat", "_off", "_size", "_stride", "_armed", "_param")

    def __init__(self, flat: torch.Tensor, view: torch.Tensor,
                 param: torch.Tensor):
        # `view` is the trainer's view of the span; only its geometry is
        # kept, never a tensor that take() would return. The parameter is
        # held weakly (it holds the sink).
        self._param = weakref.ref(param)
        self._flat = flat
        self._off = view.storage_offset() - flat.storage_offset()
        self._size = tuple(view.shape)
        self._stride = tuple(view.stride())
        self._armed = False

    def view(self) -> torch.Tensor:
        """A fresh view of the span (shape and strides of the parameter)."""
        return self._flat.as_strided(self._size, self._stride,
                                     self._flat.storage_offset() + self._off)

    def data_ptr(self) -> int:
        return self._flat.data_ptr() + 4 * self._off

    def arm(self) -> None:
        self._armed = True

    @property
    def armed(self) -> bool:
        return self._armed

    def disarm(self) -> None:
        self._armed = False

    def take(self) -> Optional[torch.Tensor]:
        """The span, once per arm() and only while the parameter has no
        gradient. Once p.grad is set, by whatever route (the trainer's
        hook repaired a gradient that arrived otherwise, a step without
        a gradient was settled, the user assigned one), p.grad aliases
        the span: writing the span would overwrite that gradient and
        autograd would then add the span to itself."""
        p = self._param()
        if not self._armed or p is None or p.grad is not None:
            self._armed = False
            return None
        self._armed = False
        return self.view()


def attach(p: torch.Tensor, sink: GradSink) -> None:
    setattr(p, _ATTR, sink)


def detach(p: torch.Tensor) -> None:
    if hasattr(p, _ATTR):
        delattr(p, _ATTR)


def sink_of(p: torch.Tensor) -> Optional[GradSink]:
    return getattr(p, _ATTR, None)
