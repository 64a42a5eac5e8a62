"""Every server optimizer kernel, dense and row-sparse, reproduces bit for
bit what the kernels of the commit named in tests/golden/optim_parent.npz
wrote (tests/optim_golden_cases.py): the update rules live once in
csrc/optim_rules.h, and this is what holds every instantiation to the
arithmetic it had when each kernel spelled its rule out by hand."""

import numpy as np
import pytest
import torch

import geomx_amd.ops as ops

import kvstore_edge_cases as K
import optim_golden_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def _equal(got, want):
    return torch.equal(torch.from_numpy(got).view(torch.int32),
                       torch.from_numpy(np.ascontiguousarray(want))
                       .view(torch.int32))


@pytest.mark.parametrize("name", G.VARIANTS)
def test_dense_bits_match_parent(name, golden):
    """All of DENSE_SIZES: w and every state, compared whole."""
    want = {k: G.split_dense(golden["dense/%s/%s" % (name, k)])
            for k in G.outputs(name)}
    for n in G.DENSE_SIZES:
        got = G.run_dense(ops, name, *G.dense_case(name, n), device=DEV)
        assert sorted(got) == sorted(want)
        for k in got:
            assert _equal(got[k], want[k][n]), (name, n, k)


@pytest.mark.parametrize("name", G.VARIANTS)
def test_grid_stride_wrap_digest_matches_parent(name, golden):
    """One element group past 2048 blocks x 256 threads: the SHA-256 of
    every output. On a miss the message carries the worst error/bound
    ratio of the float64 oracle, to tell a rounding from a wrong index."""
    st0, g = G.dense_case(name, G.big_n(name))
    got = G.run_dense(ops, name, st0, g, device=DEV)
    missed = [k for k in G.outputs(name)
              if G.digest(got[k]) != str(golden["big/%s/%s" % (name, k)])]
    if missed:
        try:
            ratio = K.opt_check_step(name, st0, got, g, G.hp_of(name))
        except AssertionError as e:
            ratio = e
        pytest.fail("%s n=%d: digest of %s differs; oracle error/bound "
                    "(worst, sign-excluded share): %s"
                    % (name, G.big_n(name), missed, ratio))


@pytest.mark.parametrize("width,offset", G.ROW_CASES)
@pytest.mark.parametrize("rule", G.ROW_RULES)
def test_row_bits_match_parent(rule, width, offset, golden):
    """The whole table and states: touched rows, untouched rows and the
    rows that out-of-range ids name."""
    got = G.run_row(ops, rule, *G.row_case(rule, width), offset, device=DEV)
    for k in G.outputs(rule):
        want = golden["row/%s/%s/%s" % (rule, G.row_tag(width, offset), k)]
        assert _equal(got[k], want), (rule, width, offset, k)
