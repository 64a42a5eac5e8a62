"""Row-sparse push on CPU (gloo): rows-only wire, lazy row updates,
fallbacks and ordering. Data is integer-valued and sgd uses lr=0.5, so
every sum and update is exact and results compare with torch.equal."""

import pytest
import torch

from dist_helpers import run_dist

from geomx_amd import Config
from geomx_amd.kvstore import create
from geomx_amd.kvstore.optimizer import OptimizerSpec, ServerOptimizer
from geomx_amd.kvstore.wan import cross_party_bytes
from geomx_amd.ops import reference as ref
from geomx_amd.topology import init_topology

ROWS, WIDTH = 64, 3

# overlapping + duplicated id lists, one rank empty
# party 0 = ranks 0,1 -> unique {1,4,7}; party 1 = ranks 2,3 -> {0,1,2,4,7,63}
IDS = {0: [1, 4, 1, 7], 1: [], 2: [4, 4, 63, 0], 3: [7, 1, 2]}


def _mk(mode="dist_sync", num_parties=1, **over):
    cfg = Config.from_env(num_parties=num_parties, backend="gloo",
                          device="cpu", **over)
    topo = init_topology(cfg.num_parties, cfg.party_sizes, "gloo", "cpu")
    return create(mode, cfg=cfg, topo=topo)


def _grad(rank, ids=None):
    ids = torch.tensor(IDS[rank] if ids is None else ids, dtype=torch.int64)
    n = ids.numel()
    vals = (torch.arange(n * WIDTH).reshape(n, WIDTH) % 5 + rank + 1).float()
    return ids, vals


def _densify(ids, vals):
    d = torch.zeros(ROWS, WIDTH)
    d.index_add_(0, ids, vals)  # integer-valued: order cannot matter
    return d


def _w0():
    return (torch.arange(ROWS * WIDTH).reshape(ROWS, WIDTH) % 7).float()


def _pull(kv, key):
    out = torch.empty(ROWS, WIDTH)
    kv.pull(key, out)
    return out


# ---------------------------------------------------------------------------
# ws4: 2 parties x 2 workers, result equals the dense push
# ---------------------------------------------------------------------------

def _ws4_result(rank, world, mode, global_mode, with_opt):
    kv = _mk(mode, num_parties=2)
    kv.global_mode = global_mode
    if with_opt:
        kv.set_optimizer(OptimizerSpec(name="sgd", lr=0.5))
    kv.init("s", _w0())
    kv.init("d", _w0())
    for step in range(2):  # second round exercises reuse of all buffers
        ids, vals = _grad(rank)
        vals = vals + step
        kv.push_row_sparse("s", ids, vals)
        kv.push("d", _densify(ids, vals))
        s, d = _pull(kv, "s"), _pull(kv, "d")
        assert torch.equal(s, d), (rank, step, (s - d).abs().max())
    assert not torch.equal(s, _w0())


@pytest.mark.parametrize("mode", ["dist_sync", "dist_async"])
@pytest.mark.parametrize("global_mode", ["replicated", "sharded"])
def test_push_row_sparse_matches_dense_ws4(mode, global_mode):
    run_dist(4, _ws4_result, mode, global_mode, True)


def test_push_row_sparse_update_on_worker_ws4():
    # no optimizer: pull returns the aggregated gradient
    run_dist(4, _ws4_result, "dist_sync", "sharded", False)


# ---------------------------------------------------------------------------
# wire bytes: rows-only formula, below the dense path's charge
# ---------------------------------------------------------------------------

def _wire_bytes(rank, world, global_mode):
    kv = _mk("dist_sync", num_parties=2, wan_gbps=1000.0)
    kv.global_mode = global_mode
    kv.set_optimizer(OptimizerSpec(name="sgd", lr=0.5))
    kv.init("s", _w0())  # first key: owner party 0
    before = kv.wan.total_bytes
    ids, vals = _grad(rank)
    kv.push_row_sparse("s", ids, vals)
    kv.flush()
    got = kv.wan.total_bytes - before
    P = 2
    cnt = [3, 6]  # unique rows per party, see IDS
    row_bytes = WIDTH * 4 + 8
    if not kv.topo.is_leader:
        expect = dense = 0.0
    elif global_mode == "replicated":
        expect = cross_party_bytes("all_gather", 8, P) \
            + cross_party_bytes("all_gather", max(cnt) * row_bytes, P)
        dense = cross_party_bytes("all_gather", ROWS * WIDTH * 4, P)
    else:
        # party 1's leader ships its 6 rows to the owner (party 0);
        # both ends of the transfer are charged on their own link
        expect = float(cnt[1] * row_bytes)
        dense = cross_party_bytes("reduce", ROWS * WIDTH * 4, P)
    assert got == expect, (rank, got, expect)
    if kv.topo.is_leader:
        assert got < dense, (rank, got, dense)
    # the result is still right
    kv.init("d", _w0())
    kv.push("d", _densify(ids, vals))
    assert torch.equal(_pull(kv, "s"), _pull(kv, "d"))


@pytest.mark.parametrize("global_mode", ["replicated", "sharded"])
def test_push_row_sparse_wire_bytes_ws4(global_mode):
    run_dist(4, _wire_bytes, global_mode)


# ---------------------------------------------------------------------------
# lazy semantics, single process
# ---------------------------------------------------------------------------

def _lazy_kv(lazy):
    kv = _mk()
    kv.set_optimizer(OptimizerSpec(name="sgd_mom", lr=0.5, momentum=0.5,
                                   lazy_update=lazy))
    kv.init("emb", torch.ones(6, 2))
    return kv


def test_lazy_update_keeps_untouched_rows():
    kv = _lazy_kv(True)
    w0 = torch.ones(6, 2)
    untouched = [0, 2, 3, 5]
    for _ in range(2):
        kv.push_row_sparse("emb", torch.tensor([1, 4]), torch.ones(2, 2))
        out = torch.empty(6, 2)
        kv.pull("emb", out)
        mom = kv.optimizer.state["emb"]["mom"].reshape(6, 2)
        assert torch.equal(out[untouched], w0[untouched])
        assert torch.equal(mom[untouched], torch.zeros(4, 2))
    # two steps of sgd_mom on the touched rows: mom -0.5 then -0.75
    assert torch.equal(out[[1, 4]], torch.full((2, 2), 1.0 - 0.5 - 0.75))
    # a push that names other rows leaves rows 1,4 and their momentum alone
    kv.push_row_sparse("emb", torch.tensor([2]), torch.ones(1, 2))
    out2 = torch.empty(6, 2)
    kv.pull("emb", out2)
    assert torch.equal(out2[[1, 4]], out[[1, 4]])
    assert torch.equal(mom[[1, 4]], torch.full((2, 2), -0.75))
    assert kv.optimizer.step_count["emb"] == 3


def test_dense_update_momentum_keeps_moving_rows():
    kv = _lazy_kv(False)
    kv.push_row_sparse("emb", torch.tensor([1, 4]), torch.ones(2, 2))
    out = torch.empty(6, 2)
    kv.pull("emb", out)
    assert torch.equal(out[[1, 4]], torch.full((2, 2), 0.5))
    kv.push_row_sparse("emb", torch.tensor([2]), torch.ones(1, 2))
    out2 = torch.empty(6, 2)
    kv.pull("emb", out2)
    # today's behaviour: momentum decays into rows 1,4 although absent
    assert torch.equal(out2[[1, 4]], torch.full((2, 2), 0.25))
    assert torch.equal(out2[2], torch.full((2,), 0.5))
    assert torch.equal(out2[[0, 3, 5]], torch.ones(3, 2))


def test_lazy_spec_roundtrips_and_old_blobs_default():
    opt = ServerOptimizer(OptimizerSpec(name="adam", lazy_update=True))
    blob = opt.state_dict()
    assert blob["spec"]["lazy_update"] is True
    del blob["spec"]["lazy_update"]  # a checkpoint from before the field
    opt.load_state_dict(blob)
    assert opt.spec.lazy_update is False


@pytest.mark.parametrize("name", ["sgd", "sgd_mom", "adam", "adagrad",
                                  "rmsprop"])
@pytest.mark.parametrize("lazy", [False, True])
def test_update_rows_matches_dense_on_touched_rows(name, lazy):
    """update_rows against update() on the densified gradient: equal
    everywhere when not lazy (or the optimizer has no row kernel), equal
    on the touched rows and frozen elsewhere when lazy."""
    torch.manual_seed(3)
    rows, width = 9, 5
    w0 = torch.randn(rows, width)
    a = ServerOptimizer(OptimizerSpec(name=name, lr=0.1, wd=0.01,
                                      clip_gradient=0.8, lazy_update=lazy))
    b = ServerOptimizer(OptimizerSpec(name=name, lr=0.1, wd=0.01,
                                      clip_gradient=0.8))
    wa, wb = w0.clone(), w0.clone()
    ids = torch.tensor([-1, 2, 7, 8, -1])  # merged form: unique + padding
    touched = [2, 7, 8]
    for _ in range(2):
        g = torch.randn(5, width)
        dense = torch.zeros(rows, width)
        dense[touched] = g[1:4]
        a.update_rows("k", wa, ids, g)
        b.update("k", wb.reshape(-1), dense.reshape(-1))
        assert torch.allclose(wa[touched], wb[touched], atol=1e-6)
        if not (lazy and name != "rmsprop"):
            assert torch.allclose(wa, wb, atol=1e-6)
    if lazy and name != "rmsprop":
        untouched = [0, 1, 3, 4, 5, 6]
        assert torch.equal(wa[untouched], w0[untouched])
        for s in a.state["k"].values():
            assert torch.equal(s.reshape(rows, width)[untouched],
                               torch.zeros(6, width))
    assert a.step_count["k"] == 2
    a.update_rows("k", wa, ids[:0], torch.zeros(0, width))
    assert a.step_count["k"] == 3  # an empty push still counts a step


# ---------------------------------------------------------------------------
# golden model of the merge
# ---------------------------------------------------------------------------

def test_reference_merge_order_and_padding():
    ids = torch.tensor([5, 2, 5, 0, 2, 5])
    # magnitudes chosen so fp32 addition order is visible
    vals = torch.tensor([[1e8], [1.0], [-1e8], [3.0], [2.0], [1.0]])
    out_ids, out_vals = ref.rsp_merge(ids, vals)
    assert out_ids.tolist() == [0, 2, 5, -1, -1, -1]
    # row 5 adds positions 0, 2, 5 in that order: (1e8 - 1e8) + 1 = 1
    assert out_vals[:, 0].tolist() == [3.0, 3.0, 1.0, 0.0, 0.0, 0.0]
    e_ids, e_vals = ref.rsp_merge(ids[:0], vals[:0])
    assert e_ids.numel() == 0 and e_vals.shape == (0, 1)


def test_reference_scatter_skips_out_of_range():
    dense = torch.ones(4, 2)
    ids = torch.tensor([-1, 3, 4, 0])
    merged = torch.arange(8.0).reshape(4, 2)
    ref.rsp_scatter(dense, ids, merged, accumulate=True)
    assert torch.equal(dense, torch.tensor([[7., 8.], [1., 1.], [1., 1.],
                                            [3., 4.]]))
    ref.rsp_scatter(dense, ids, merged)
    assert torch.equal(dense[[0, 3]], merged[[3, 1]])


# ---------------------------------------------------------------------------
# fallbacks keep the densify-and-push path
# ---------------------------------------------------------------------------

def _fallback(rank, world, case):
    over = {}
    if case == "hfa":
        over = dict(use_hfa=True, hfa_k2=1)
    elif case == "sliced":
        over = dict(bigarray_bound=64)
    kv = _mk("dist_sync", num_parties=2, **over)
    if case == "updater":
        kv.set_updater(lambda key, g, w: w.sub_(g))
    else:
        kv.set_optimizer(OptimizerSpec(name="sgd", lr=0.5))
    if case == "bsc":
        kv.set_gradient_compression({"type": "bsc", "threshold": 0.25,
                                     "size_lower_bound": 16})
    kv.init("s", _w0())
    kv.init("d", _w0())
    assert not kv._rsp_rows_route(kv.keys["s"])
    if case == "sliced":
        assert kv.keys["s"].sliced
    ids, vals = _grad(rank * 2)  # ranks 0,1 use the lists of ranks 0,2
    kv.push_row_sparse("s", ids, vals)
    kv.push("d", _densify(ids, vals))
    s, d = _pull(kv, "s"), _pull(kv, "d")
    assert torch.equal(s, d), (rank, case)
    assert not torch.equal(s, _w0())


@pytest.mark.parametrize("case", ["bsc", "hfa", "sliced", "updater"])
def test_push_row_sparse_fallbacks_ws2(case):
    run_dist(2, _fallback, case)


# ---------------------------------------------------------------------------
# host id check
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [[0, 6], [-1, 2]])
def test_cpu_ids_out_of_range_raise(bad):
    kv = _mk()
    kv.init("emb", torch.zeros(6, 3))
    with pytest.raises(ValueError):
        kv.push_row_sparse("emb", torch.tensor(bad), torch.ones(2, 3))


def test_sparse_coo_push_routes_to_row_sparse():
    kv = _mk()
    kv.init("emb", torch.zeros(6, 3))
    emb = torch.nn.Embedding(6, 3, sparse=True)
    emb(torch.tensor([1, 4, 1])).sum().backward()
    assert emb.weight.grad.layout == torch.sparse_coo
    kv.push("emb", emb.weight.grad)
    out = torch.empty(6, 3)
    kv.pull("emb", out)
    assert torch.equal(out, emb.weight.grad.to_dense())
    assert torch.equal(out[1], torch.full((3,), 2.0))


# ---------------------------------------------------------------------------
# priority order of the deferred tier
# ---------------------------------------------------------------------------

def _rsp_priority(rank, world):
    kv = _mk(num_parties=2)
    kv.global_mode = "replicated"
    kv.set_optimizer(OptimizerSpec(name="sgd", lr=0.5))
    keys = ["a", "b", "c"]
    for k in keys:
        kv.init(k, _w0())
    order = []
    post = kv._rsp_post
    kv._rsp_post = lambda key, st, party: (order.append(key),
                                           post(key, st, party))
    ids, vals = _grad(rank)
    for k, prio in zip(keys, [0, 5, 2]):
        kv.push_row_sparse(k, ids, vals, priority=prio)
    assert len(kv._pending) == 3 and order == []
    # divergent pull orders: the flush order must not depend on them
    first = keys[rank % 3]
    got = {first: _pull(kv, first)}
    assert order == ["b", "c", "a"], (rank, order)
    for k in keys:
        got.setdefault(k, _pull(kv, k))
    assert torch.equal(got["a"], got["b"]) and torch.equal(got["a"], got["c"])
    assert not torch.equal(got["a"], _w0())


def test_push_row_sparse_priority_order_ws4():
    run_dist(4, _rsp_priority)
