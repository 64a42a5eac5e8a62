"""Routes of the grayscale conv1 stage (weight [16][1][5][5]) and the
gather table of its forward fragments; no GPU."""

import pytest
import torch

from geomx_amd.ops.conv import build_c1_fwd_index, plan_conv5

SHAPE = (16, 1, 5, 5)
ATEN = ("aten", "aten", "aten")


@pytest.mark.parametrize("h,w,pooled,want", [
    (28, 28, True, ("pool1", "aten", "wrw1")),
    (8, 228, True, ("pool1", "aten", "wrw1")),   # the widest served row
    (8, 230, True, ATEN),
    (9, 36, True, ("aten", "aten", "wrw1")),     # odd Ho: nothing to pool
    (8, 35, True, ATEN),                         # odd W: no pixel pairs
    (8, 36, False, ("aten", "aten", "wrw1")),
])
def test_plan(h, w, pooled, want):
    assert tuple(plan_conv5(SHAPE, h, w, pooled)) == want
    assert tuple(plan_conv5(SHAPE, h, w, pooled, native=False)) == ATEN


def test_fwd_index_is_a_permutation_plus_zero_slots():
    idx = build_c1_fwd_index(SHAPE)
    assert idx.shape == (2 * 64 * 8,)
    live = idx[idx < 400]
    assert torch.equal(live.sort().values, torch.arange(400))
    assert (idx[idx >= 400] == 400).all()
    # chunk 0, lane (q=2, n=5), slot 3: w[5][0][2][3]; chunk 1 is kh = 4
    # in q = 0 and dead elsewhere
    assert idx[(2 * 16 + 5) * 8 + 3] == 5 * 25 + 2 * 5 + 3
    assert idx[512 + 5 * 8 + 1] == 5 * 25 + 4 * 5 + 1
    assert (idx[512 + 16 * 8:] == 400).all()
