"""tests/golden/optim_parent.npz without a GPU: the recorded bits are within
the float64 oracle's derived bound (so a golden recorded from a broken
kernel cannot be committed), the row goldens touch exactly the rows the
valid ids name, the inputs contain the edge cases they are there for, and
the fp32 reference model stays within the same bounds on the same inputs."""

import numpy as np
import pytest

from geomx_amd.ops import reference as ref

import kvstore_edge_cases as K
import optim_golden_cases as G


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def _check(name, before, after, g):
    worst, excluded = K.opt_check_step(name, before, after, g, G.hp_of(name))
    assert worst <= 1.0
    assert excluded < K.SIGN_EXCLUDED_CAP, (name, excluded)
    return worst


def _gathered(arrays, ids):
    rows = ids[G.row_valid(ids)]
    return {k: v[rows].reshape(-1) for k, v in arrays.items()}


def test_golden_holds_every_case_and_nothing_else(golden):
    keys = {"commit"}
    for name in G.VARIANTS:
        for k in G.outputs(name):
            keys |= {"dense/%s/%s" % (name, k), "big/%s/%s" % (name, k)}
            assert len(str(golden["big/%s/%s" % (name, k)])) == 64
    for rule in G.ROW_RULES:
        for width, offset in G.ROW_CASES:
            for k in G.outputs(rule):
                key = "row/%s/%s/%s" % (rule, G.row_tag(width, offset), k)
                keys.add(key)
                assert golden[key].shape == (G.ROWS, width)
                assert golden[key].dtype == np.float32
    assert set(golden.files) == keys
    assert len(str(golden["commit"])) == 40


def test_inputs_contain_what_they_claim():
    assert sorted(K.OPT_HP) == G.VARIANTS and len(G.VARIANTS) == 10
    sizes = G.DENSE_SIZES
    assert {n % 4 for n in sizes if n > 4} == {0, 1, 3}     # tails 0, 1, 3
    assert {1, 3} <= set(sizes)                 # tail only
    assert 4 in sizes                           # one vector, no tail
    assert 1023 in sizes and 1023 // 4 == 255   # 255 vectors + 3
    for name in G.VARIANTS:                     # one group past the grid
        per = 4 if name in K.OPT_FLOAT4 else 1
        assert G.big_n(name) // per == 2048 * 256 + 1
        st, g = G.dense_case(name, 64)
        assert all(np.abs(a).sum() > 0 for a in st.values())    # non-zero
    for rule in G.ROW_RULES:
        for width, offset in G.ROW_CASES:
            st, ids, merged = G.row_case(rule, width)
            assert ids.shape == (G.SLOTS,) and merged.shape == (G.SLOTS,
                                                                width)
            live = ids[G.row_valid(ids)]
            assert live.size == np.unique(live).size == 14
            assert (ids == -1).sum() == 3
            assert {24, 29, -7} <= set(ids.tolist())
            assert live.size < G.ROWS           # some rows stay untouched
            ops_t = G.row_operands(st, ids, merged, offset)
            for t in list(ops_t[0].values()) + [ops_t[2]]:
                assert (t.data_ptr() % 16 != 0) == offset
    assert [w % 4 == 0 for w, _ in G.ROW_CASES] == [False, True, True, True]
    assert G.SLOTS * (64 // 4) > 256            # width 64: a second block


@pytest.mark.parametrize("name", G.VARIANTS)
def test_dense_golden_within_oracle_bound(name, golden):
    want = {k: G.split_dense(golden["dense/%s/%s" % (name, k)])
            for k in G.outputs(name)}
    worst = 0.0
    for n in G.DENSE_SIZES:
        st0, g = G.dense_case(name, n)
        worst = max(worst, _check(name, st0, {k: v[n] for k, v
                                              in want.items()}, g))
        # the fp32 reference model on the same inputs
        _check(name, st0, G.run_dense(ref, name, st0, g), g)
    print("%s golden worst error/bound %.3f" % (name, worst))


@pytest.mark.parametrize("width,offset", G.ROW_CASES)
@pytest.mark.parametrize("rule", G.ROW_RULES)
def test_row_golden_touches_only_valid_rows(rule, width, offset, golden):
    st0, ids, merged = G.row_case(rule, width)
    want = {k: golden["row/%s/%s/%s" % (rule, G.row_tag(width, offset), k)]
            for k in G.outputs(rule)}
    g = merged[G.row_valid(ids)].reshape(-1)
    _check(rule, _gathered(st0, ids), _gathered(want, ids), g)
    _check(rule, _gathered(st0, ids),
           _gathered(G.run_row(ref, rule, st0, ids, merged, offset), ids), g)
    rest = np.setdiff1d(np.arange(G.ROWS), ids[G.row_valid(ids)])
    for k in want:
        assert np.array_equal(want[k][rest].view(np.int32),
                              st0[k][rest].view(np.int32)), (rule, k)
        assert (want[k][ids[G.row_valid(ids)]] != st0[k][ids[G.row_valid(
            ids)]]).any(), (rule, k)

