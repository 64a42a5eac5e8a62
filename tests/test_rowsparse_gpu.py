"""Row-sparse push kernels on gfx950 (csrc/rowsparse.hip) against the
pure-torch golden models, and the rows-only kvstore route on cuda:0."""

import pytest
import torch

import geomx_amd.ops as ops
from geomx_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = 1000


@pytest.fixture(autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"


def _ids(pattern, nnz, rows=ROWS):
    g = torch.Generator().manual_seed(nnz * 7 + len(pattern))
    if pattern == "distinct":
        return torch.randperm(rows, generator=g)[:nnz]
    if pattern == "equal":
        return torch.full((nnz,), 7, dtype=torch.int64)
    # mixed: about a third as many distinct ids as entries, both table
    # ends present
    ids = torch.randint(0, max(2, nnz // 3), (nnz,), generator=g) * 3
    if nnz >= 2:
        ids[nnz // 2] = 0
        ids[0] = rows - 1
    return ids


def _vals(nnz, width, seed=0):
    g = torch.Generator().manual_seed(seed + nnz + width)
    return torch.randn(nnz, width, generator=g)


def _offset_view(t):
    """Same values as `t`, stored one element into a larger buffer: a
    4-byte-aligned view that the 16-byte path must not take."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["distinct", "equal", "mixed"])
@pytest.mark.parametrize("width", [1, 3, 4, 5, 8, 130, 1024])
def test_rsp_merge_equals_reference(width, pattern):
    for nnz in (0, 1, 64, 65, 300):
        ids, vals = _ids(pattern, nnz), _vals(nnz, width)
        e_ids, e_vals = ref.rsp_merge(ids, vals)
        g_ids, g_vals = ops.rsp_merge(ids.to(DEV), vals.to(DEV))
        assert g_ids.shape == (nnz,) and g_vals.shape == (nnz, width)
        assert torch.equal(g_ids.cpu(), e_ids), (nnz, width, pattern)
        # same sequential order of fp32 adds: bit-equal, not just close
        assert torch.equal(g_vals.cpu(), e_vals), (nnz, width, pattern)
        n_u = len(set(ids.tolist()))
        assert (g_ids[n_u:] == -1).all() and (g_ids[:n_u] >= 0).all()
        if pattern == "equal" and nnz:
            assert n_u == 1  # one segment of nnz rows (300 > one block)


# ---------------------------------------------------------------------------
# scatter
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("width", [1, 5, 8, 130])
def test_rsp_scatter_equals_reference(width, accumulate):
    ids, merged = ref.rsp_merge(_ids("mixed", 300), _vals(300, width))
    dense = _vals(ROWS, width, seed=5)
    d_gpu = dense.clone().to(DEV)
    ops.rsp_scatter(d_gpu, ids.to(DEV), merged.to(DEV), accumulate)
    ref.rsp_scatter(dense, ids, merged, accumulate)
    assert torch.equal(d_gpu.cpu(), dense)


# ---------------------------------------------------------------------------
# row updates
# ---------------------------------------------------------------------------

# (ops function, state tensor count, args after the states, atol) — the
# tolerances are those of the dense tests of the same optimizer in
# test_kernels_gpu.py (adagrad as sgd_mom)
OPTS = {
    "sgd": ("rsp_sgd_update", "sgd_update", 0, (0.1, 1e-4, 2.0), 1e-6),
    "sgd_mom": ("rsp_sgd_mom_update", "sgd_mom_update", 1,
                (0.1, 0.9, 1e-4, 1.0), 1e-5),
    "adam": ("rsp_adam_update", "adam_update", 2, (0.01,), 1e-5),
    "adagrad": ("rsp_adagrad_update", "adagrad_update", 1,
                (0.1, 1e-7, 1e-4, 1.0), 1e-5),
}


def _run_update(mod, fname, name, w, ids, merged, states, step):
    extra = OPTS[name][3]
    if name == "adam":
        getattr(mod, fname)(w, ids, merged, *states, step, *extra)
    else:
        getattr(mod, fname)(w, ids, merged, *states, *extra)


@pytest.mark.parametrize("width", [5, 8, 130])
@pytest.mark.parametrize("name", list(OPTS))
def test_rsp_update_matches_reference(name, width):
    fname, dense_fname, nstate, extra, atol = OPTS[name]
    ids, _ = ref.rsp_merge(_ids("mixed", 300), _vals(300, width))
    touched = ids[ids >= 0]
    mask = torch.zeros(ROWS, dtype=torch.bool)
    mask[touched] = True
    w0 = _vals(ROWS, width, seed=11)
    # non-zero starting state, so that untouched state rows prove something
    s0 = [_vals(ROWS, width, seed=20 + i).abs() for i in range(nstate)]
    w_c, s_c = w0.clone(), [s.clone() for s in s0]
    w_g, s_g = w0.clone().to(DEV), [s.clone().to(DEV) for s in s0]
    w_d, s_d = w0.clone().to(DEV), [s.clone().to(DEV) for s in s0]
    for step in range(1, 4):
        merged = _vals(300, width, seed=step)
        _run_update(ref, fname, name, w_c, ids, merged, s_c, step)
        _run_update(ops, fname, name, w_g, ids.to(DEV), merged.to(DEV), s_g,
                    step)
        # dense kernel on the densified gradient, for the bit-equality note
        dense = torch.zeros(ROWS, width)
        ref.rsp_scatter(dense, ids, merged)
        if name == "adam":
            ops.adam_update(w_d, dense.to(DEV), *s_d, step, *extra)
        else:
            getattr(ops, dense_fname)(w_d, dense.to(DEV), *s_d, *extra)
    print(f"rsp_{name} width={width}: touched rows bit-equal to the dense "
          f"kernel: w={torch.equal(w_g[mask.to(DEV)], w_d[mask.to(DEV)])}"
          + "".join(f" s{i}={torch.equal(a[mask.to(DEV)], b[mask.to(DEV)])}"
                    for i, (a, b) in enumerate(zip(s_g, s_d)))
          + f"; max |gpu-ref| w={(w_g.cpu() - w_c).abs().max():.3g}")
    assert torch.allclose(w_g.cpu()[mask], w_c[mask], atol=atol)
    for a, b in zip(s_g, s_c):
        assert torch.allclose(a.cpu()[mask], b[mask], atol=atol)
    # lazy: rows no id names keep weight AND state, exactly
    assert torch.equal(w_g.cpu()[~mask], w0[~mask])
    for a, b in zip(s_g, s0):
        assert torch.equal(a.cpu()[~mask], b[~mask])


# ---------------------------------------------------------------------------
# alignment: views one element into a larger buffer take the scalar path
# ---------------------------------------------------------------------------

def test_rsp_unaligned_views():
    width = 8
    ids, vals = _ids("mixed", 300), _vals(300, width)
    e_ids, e_merged = ref.rsp_merge(ids, vals)
    g_ids, g_merged = ops.rsp_merge(ids.to(DEV), _offset_view(vals.to(DEV)))
    assert torch.equal(g_ids.cpu(), e_ids)
    assert torch.equal(g_merged.cpu(), e_merged)

    dense = _vals(ROWS, width, seed=5)
    for acc in (False, True):
        d_g = _offset_view(dense.to(DEV))
        d_c = dense.clone()
        ops.rsp_scatter(d_g, g_ids, _offset_view(g_merged), acc)
        ref.rsp_scatter(d_c, e_ids, e_merged, acc)
        assert torch.equal(d_g.cpu(), d_c)

    w0, m0 = _vals(ROWS, width, seed=11), _vals(ROWS, width, seed=12)
    w_g, m_g = _offset_view(w0.to(DEV)), _offset_view(m0.to(DEV))
    w_c, m_c = w0.clone(), m0.clone()
    ops.rsp_sgd_mom_update(w_g, g_ids, g_merged, m_g, 0.1, 0.9, 1e-4, 1.0)
    ref.rsp_sgd_mom_update(w_c, e_ids, e_merged, m_c, 0.1, 0.9, 1e-4, 1.0)
    assert torch.allclose(w_g.cpu(), w_c, atol=1e-5)
    assert torch.allclose(m_g.cpu(), m_c, atol=1e-5)
    mask = torch.zeros(ROWS, dtype=torch.bool)
    mask[e_ids[e_ids >= 0]] = True
    assert torch.equal(w_g.cpu()[~mask], w0[~mask])
    assert torch.equal(m_g.cpu()[~mask], m0[~mask])


# ---------------------------------------------------------------------------
# out-of-range ids are skipped, never dereferenced
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("width", [5, 8])
def test_rsp_out_of_range_ids_skipped(width):
    rows, guard = 50, 2
    good = torch.tensor([0, 3, 49, 17])
    bad = torch.tensor([-1, rows, -2, rows + 1])
    ids = torch.cat([bad[:2], good, bad[2:]])
    vals = _vals(ids.numel(), width) + 1.0
    m_ids, merged = ops.rsp_merge(ids.to(DEV), vals.to(DEV))
    k_ids, k_merged = ops.rsp_merge(good.to(DEV), vals[2:6].to(DEV))

    def table(seed):
        # the table is a slice in the MIDDLE of a larger allocation: a
        # stray row write lands in a guard row the test owns
        alloc = _vals(rows + 2 * guard, width, seed=seed).to(DEV)
        return alloc, alloc[guard:guard + rows]

    def check(run):
        a1, t1 = table(31)
        s1a, s1 = table(32)
        a2, t2 = table(31)
        s2a, s2 = table(32)
        w_before, s_before = a1.clone(), s1a.clone()
        run(t1, s1, m_ids, merged)
        run(t2, s2, k_ids, k_merged)
        # equal to the run with the bad entries removed ...
        assert torch.equal(a1, a2) and torch.equal(s1a, s2a)
        # ... the guard rows never moved, and the table did
        for a, b in ((a1, w_before), (s1a, s_before)):
            assert torch.equal(a[:guard], b[:guard])
            assert torch.equal(a[-guard:], b[-guard:])
        assert not torch.equal(t1, w_before[guard:guard + rows])

    check(lambda t, s, i, m: ops.rsp_scatter(t, i, m, False))
    check(lambda t, s, i, m: ops.rsp_scatter(t, i, m, True))
    check(lambda t, s, i, m: ops.rsp_sgd_update(t, i, m, 0.1, 1e-4, 1.0))
    check(lambda t, s, i, m: ops.rsp_sgd_mom_update(t, i, m, s, 0.1, 0.9,
                                                    1e-4, 1.0))
    check(lambda t, s, i, m: ops.rsp_adagrad_update(t, i, m, s.abs_(), 0.1))
    a, t = table(31)
    va, v = table(33)
    ops.rsp_adam_update(t, m_ids, merged, table(32)[1], v.abs_(), 1, 0.01)
    a2, t2 = table(31)
    ops.rsp_adam_update(t2, k_ids, k_merged, table(32)[1], table(33)[1].abs_(),
                        1, 0.01)
    assert torch.equal(a, a2)


# ---------------------------------------------------------------------------
# kvstore on cuda:0, world size 1
# ---------------------------------------------------------------------------

def _kv(spec=None):
    from geomx_amd import Config
    from geomx_amd.kvstore import create
    kv = create("dist_sync", cfg=Config.from_env(device=DEV))
    if spec is not None:
        kv.set_optimizer(spec)
    return kv


def _int_w(rows, width):
    return (torch.arange(rows * width, device=DEV).reshape(rows, width)
            % 7).float()


@pytest.mark.parametrize("name,lazy", [("sgd", False), ("sgd_mom", False),
                                       ("sgd_mom", True), (None, False)])
def test_kvstore_push_row_sparse_gpu(name, lazy):
    """push_row_sparse (GPU ids, duplicates), then an EMPTY push, against
    dense pushes of the equivalent gradients on a second store. Integer
    data and lr = momentum = 0.5 keep every step exact."""
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    rows, width = 96, 8
    mk = lambda: None if name is None else OptimizerSpec(  # noqa: E731
        name=name, lr=0.5, momentum=0.5, lazy_update=lazy)
    kv_s, kv_d = _kv(mk()), _kv(mk())
    kv_s.init("emb", _int_w(rows, width))
    kv_d.init("emb", _int_w(rows, width))
    assert kv_s._rsp_rows_route(kv_s.keys["emb"])
    ids = torch.tensor([5, 95, 5, 0, 40, 5, 0], device=DEV)
    vals = (torch.arange(7 * width, device=DEV).reshape(7, width) % 5
            + 1).float()
    dense = torch.zeros(rows, width, device=DEV).index_add_(0, ids, vals)
    outs = []
    for i, v, d in ((ids, vals, dense),
                    (ids[:0], vals[:0], torch.zeros_like(dense))):
        kv_s.push_row_sparse("emb", i, v)
        kv_d.push("emb", d)
        o_s = torch.empty(rows, width, device=DEV)
        o_d = torch.empty(rows, width, device=DEV)
        kv_s.pull("emb", o_s)
        kv_d.pull("emb", o_d)
        outs.append((o_s, o_d))
    (a_s, a_d), (b_s, b_d) = outs
    assert torch.equal(a_s, a_d)
    assert not torch.equal(a_s, _int_w(rows, width))
    if lazy:
        # the empty push moves nothing, where dense momentum keeps going
        assert torch.equal(b_s, a_s)
        assert not torch.equal(b_d, a_d)
    else:
        assert torch.equal(b_s, b_d)


def test_kvstore_push_sparse_embedding_grad_gpu():
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    rows, width = 64, 12
    emb = torch.nn.Embedding(rows, width, sparse=True).to(DEV)
    tok = torch.tensor([[3, 9, 3], [63, 0, 3]], device=DEV)
    (emb(tok).sum() * 2).backward()
    grad = emb.weight.grad
    assert grad.layout == torch.sparse_coo
    kv_s = _kv(OptimizerSpec(name="sgd", lr=0.5))
    kv_d = _kv(OptimizerSpec(name="sgd", lr=0.5))
    kv_s.init("emb", _int_w(rows, width))
    kv_d.init("emb", _int_w(rows, width))
    kv_s.push("emb", grad)
    kv_d.push("emb", grad.to_dense())
    o_s = torch.empty(rows, width, device=DEV)
    o_d = torch.empty(rows, width, device=DEV)
    kv_s.pull("emb", o_s)
    kv_d.pull("emb", o_d)
    assert torch.equal(o_s, o_d)
    assert torch.equal(o_s[3], _int_w(rows, width)[3] - 0.5 * 6.0)


def test_kvstore_push_row_sparse_no_host_sync():
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        pytest.skip("sync debug mode does not raise on .item() in this build")
    rows, width = 512, 16
    ids = torch.randint(0, rows, (200,), device=DEV)
    vals = torch.randn(200, width, device=DEV)
    for spec in (OptimizerSpec(name="sgd_mom", lr=0.1, lazy_update=True),
                 OptimizerSpec(name="sgd", lr=0.1),
                 OptimizerSpec(name="adam", lr=0.1)):  # dense fallback
        kv = _kv(spec)
        kv.init("emb", torch.zeros(rows, width, device=DEV))
        kv.push_row_sparse("emb", ids, vals)  # first call: state allocation
        kv.flush()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            kv.push_row_sparse("emb", ids, vals)
            kv.flush()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        out = torch.empty(rows, width, device=DEV)
        kv.pull("emb", out)
        assert out.abs().sum().item() > 0
