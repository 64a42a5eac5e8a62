"""CPU checks of tests/kvstore_edge_cases.py: the seeded inputs contain the
edges they claim, the exact oracles agree with the fp32 reference, and the
fp32 reference alone stays within every derived bound the GPU tests apply
to the kernels. No test here needs a GPU."""

from fractions import Fraction

import numpy as np
import pytest
import torch

import geomx_amd.ops as ops
from geomx_amd.ops import reference as ref

import kvstore_edge_cases as K


# ---------------------------------------------------------------------------
# 2-bit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("thr", K.TWOBIT_THRESHOLDS)
def test_twobit_inputs_hold_the_edges(thr):
    t = np.float32(thr)
    up, dn = np.nextafter(t, np.float32(9)), np.nextafter(t, np.float32(0))
    r0, grads, sums = K.twobit_case(1025, thr)
    assert (r0 != 0).mean() > 0.85            # non-zero starting residual
    for step, s in enumerate(sums):
        for edge in (t, up, dn, -t, -up, -dn):
            assert (s == edge).sum() >= 8, (step, edge)
        assert ((s == 0) & ~np.signbit(s)).sum() >= 8, step
        assert (np.abs(s) > 2 * t).sum() >= 8, step
    assert ((sums[0] == 0) & np.signbit(sums[0])).sum() >= 8
    if thr == 0.1:      # not a dyadic fraction
        assert float(t) != 0.1 and float(t) * 2 ** 20 != int(float(t) * 2 ** 20)


@pytest.mark.parametrize("thr", K.TWOBIT_THRESHOLDS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1025])
def test_twobit_oracle_is_the_reference(n, thr):
    r0, grads, _ = K.twobit_case(n, thr)
    r_o, r_t = r0.copy(), torch.from_numpy(r0.copy())
    for g in grads:
        w_o, r_o = K.twobit_oracle(r_o, g, thr)
        w_t = ref.quantize_2bit(torch.from_numpy(g), r_t, thr)
        assert np.array_equal(w_t.numpy(), w_o)
        assert np.array_equal(r_t.numpy().view(np.int32),
                              r_o.view(np.int32))


def test_twobit_dequant_words_hold_all_codes():
    n = 1023
    w = K.twobit_dequant_case(n)
    assert w.size > (n + 15) // 16            # longer than needed
    codes = (w.view(np.uint32)[:, None] >> (np.arange(16) * 2)) & 3
    assert set(np.unique(codes[:n // 16])) == {0, 1, 2, 3}
    o = K.twobit_dequant_oracle(w, n, 0.1)
    t = ref.dequantize_2bit(torch.from_numpy(w), n, 0.1)
    assert np.array_equal(t.numpy(), o)
    assert {x % 4 for x in K.TWOBIT_DEQUANT_SIZES} == {0, 1, 2, 3}
    assert all(x % 16 for x in K.TWOBIT_DEQUANT_SIZES)


# ---------------------------------------------------------------------------
# Bi-Sparse
# ---------------------------------------------------------------------------

def test_bsc_flip_instance():
    c = K.bsc_flip_case()
    n, ratio = K.FLIP_N, K.FLIP_RATIO
    assert ref.bsc_sample_size(n, ratio) == 1000
    assert ref.bsc_capacity(n, ratio) == 400
    si = ref.bsc_sample_indices(n, 1000, 42)
    for p in list(c["pos9"].tolist()) + [c["flip"]]:
        assert int((si == p).sum()) == 1
    # the searched triple, settled in exact arithmetic: the correctly
    # rounded fused result is the fp32 number just below the two-rounding one
    mu = np.float32(K.BSC_MU)
    uu, gg = np.float32(c["u"][c["flip"]]), np.float32(c["g"][c["flip"]])
    sep = np.float32(np.float32(uu * mu) + gg)
    exact = Fraction(float(uu)) * Fraction(float(mu)) + Fraction(float(gg))
    below = np.nextafter(sep, np.float32(0))
    assert abs(exact - Fraction(float(below))) < \
        abs(exact - Fraction(float(sep)))
    assert c["fma"] == float(below) < c["sep"] == float(sep)
    assert float(c["v"][c["flip"]]) == 0.0
    # reference: boundary is that element, ten elements are sent
    u, v = c["u"].clone(), c["v"].clone()
    vals, idx = ref.bsc_compress(c["g"], u, v, ratio)
    sent = idx[idx >= 0].tolist()
    assert sorted(sent) == sorted(c["pos9"].tolist() + [c["flip"]])
    assert float(vals[sent.index(c["flip"])]) == c["sep"]
    # a kernel that contracts the flip element computes c["fma"] < boundary
    assert c["fma"] < c["sep"]


def test_bsc_tie_instance():
    g, u0, v0, at, below = K.bsc_tie_case()
    b = K.BSC_TIE_BOUNDARY
    u, v = u0.clone(), v0.clone()
    vals, idx = ref.bsc_compress(g, u, v, K.ratio_for(g.numel(), 3000),
                                 boundary=b)
    sent = set(idx[idx >= 0].tolist())
    assert set(at.tolist()) <= sent
    assert not (set(below.tolist()) & sent)
    assert len(sent) > 200 and len(sent) < 3000
    vv = v0 + (u0 * K.BSC_MU + g)
    assert (vv[at].abs() == b).all()
    assert (vv[below].abs() == float(np.nextafter(np.float32(b),
                                                  np.float32(0)))).all()


def test_bsc_pull_instance():
    x = K.bsc_pull_case()
    head = x[:1024].numpy()
    sub = (head != 0) & (np.abs(head) < 2.0 ** -126)
    assert sub.sum() >= 8
    assert ((head == 0) & np.signbit(head)).sum() >= 4
    assert ((head == 0) & ~np.signbit(head)).sum() >= 4
    vals, idx = ref.bsc_pull_compress(x, x.numel())
    assert int((idx >= 0).sum()) == int((x != 0).sum())
    # the reference keeps the subnormals
    assert set(np.nonzero(sub)[0].tolist()) <= set(idx.tolist())


def test_bsc_sizes_and_chain_state():
    assert {1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385} <= \
        set(K.BSC_SIZES)
    assert K.BSC_BIG_N == 16384 * 1024 - 5
    u0, v0, gs = K.bsc_chain_case(2049)
    assert len(gs) == 4 and (u0 != 0).all() and (v0 != 0).all()
    # u*mu is inexact for most elements: that is what the chain exercises
    exact = (u0.double() * float(np.float32(K.BSC_MU))).float().double() \
        == u0.double() * float(np.float32(K.BSC_MU))
    assert exact.float().mean() < 0.2


# ---------------------------------------------------------------------------
# DGT, 4-bit
# ---------------------------------------------------------------------------

def test_dgt_cases_and_reference():
    chunks = {c for _, c in K.DGT_CASES}
    assert chunks == {4, 63, 64, 1000, 1023, 1024}
    assert any(n % c == 1 and n > c for n, c in K.DGT_CASES)
    assert any(n < c for n, c in K.DGT_CASES)
    assert any((n + c - 1) // c >= 2049 for n, c in K.DGT_CASES)
    for n, chunk in K.DGT_CASES:
        g = K.dgt_int_case(n)
        assert np.abs(g).max() <= 3
        o = K.dgt_oracle(g, chunk)
        r = ref.dgt_contribution(torch.from_numpy(g), chunk)
        assert np.array_equal(r.numpy(), o.astype(np.float32)), (n, chunk)
        # randn: the fp32 reference (its own summation order) within the
        # kernel's bound
        x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        r = ref.dgt_contribution(torch.from_numpy(x), chunk).numpy()
        err = np.abs(r.astype(np.float64) - K.dgt_oracle(x, chunk))
        assert (err <= K.dgt_bound(x, chunk)).all(), (n, chunk)


def _ref_q4(x, chunk, res):
    p, mm = ops.quantize_4bit_chunked(torch.from_numpy(x), chunk, res)
    return p.numpy(), mm.numpy()


def test_q4_grid_holds_the_edges_and_reference_is_exact():
    assert {c for _, c in K.Q4_CASES} == {4, 8, 64, 1024}
    assert {n % 4 for n, c in K.Q4_CASES if n % c} >= {1, 2, 3}
    assert any((n + c - 1) // c >= 2049 and c == 4 for n, c in K.Q4_CASES)
    for n, chunk in K.Q4_CASES:
        chain = K.q4_grid_chain(n, chunk)
        res_t = torch.from_numpy(chain[0][1].copy())
        assert (chain[0][1] != 0).any()
        seen = set()
        for x, res, f in chain:
            assert np.array_equal(res_t.numpy(), res), (n, chunk)
            mm, codes, deq, r_new = K.q4_oracle(f, chunk)
            seen |= set(codes.tolist())
            # every quantity is fp32-representable: the oracle is exact
            for a in (mm, deq, r_new):
                assert np.array_equal(a.astype(np.float32).astype(np.float64),
                                      a)
            if chunk % 2 == 0:      # the reference packs chunk by chunk
                p, mm_r = _ref_q4(x, chunk, res_t)
                assert np.array_equal(mm_r, mm.astype(np.float32))
                assert np.array_equal(p, K.q4_pack(codes)), (n, chunk)
                assert np.array_equal(res_t.numpy(), r_new.astype(np.float32))
            const = mm[:, 0] == mm[:, 1]
            if mm.shape[0] >= 5:
                assert const.any()
            assert (f == np.repeat(mm[:, 1], chunk)[:n]).any()   # x == max
        if n >= 64:
            assert seen == set(range(16))


def test_q4_randn_reference_within_bound():
    for n, chunk in K.Q4_CASES:
        rng = np.random.default_rng(n + chunk)
        x = rng.standard_normal(n).astype(np.float32)
        res0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
        f = (x + res0).astype(np.float32)
        res = torch.from_numpy(res0.copy())
        p, mm = _ref_q4(x, chunk, res)
        mm_o, _, _, _ = K.q4_oracle(f, chunk)
        assert np.array_equal(mm, mm_o.astype(np.float32))
        codes = K.q4_unpack(p, n)
        assert codes.min() >= 0 and codes.max() <= 15
        deq = ops.dequantize_4bit_chunked(torch.from_numpy(p),
                                          torch.from_numpy(mm), n,
                                          chunk).numpy().astype(np.float64)
        bound, _ = K.q4_randn_bound(mm, n, chunk)
        assert (np.abs(deq - f) <= bound).all(), (n, chunk)
        assert (np.abs(res.numpy() - (f.astype(np.float64) - deq)) <=
                bound - _half_step(mm, n, chunk)).all()


def _half_step(mm, n, chunk):
    return K.q4_randn_bound(mm, n, chunk)[1] / 2


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------

def _torch_state(st):
    return {k: torch.from_numpy(v.copy()) for k, v in st.items()}


def _np_state(st):
    return {k: v.detach().cpu().numpy().copy() for k, v in st.items()}


@pytest.mark.parametrize("name", sorted(K.OPT_HP))
def test_fp32_reference_within_the_optimizer_bounds(name):
    """The same per-step check the GPU test applies to the kernel, applied
    to the fp32 torch reference: it must hold for the reference alone."""
    hp = dict(K.OPT_HP[name])
    worst, worst_excl = 0.0, 0.0
    for n in K.LADDER + [4099]:
        st0, gs = K.opt_case(name, n)
        st = _torch_state(st0)
        for step, g in enumerate(gs):
            hp["t"] = step + 1
            before = _np_state(st)
            K.opt_call(ref, name, st, torch.from_numpy(g), hp)
            r, ex = K.opt_check_step(name, before, _np_state(st), g, hp)
            worst, worst_excl = max(worst, r), max(worst_excl, ex)
            if name == "dcasgd_mom0":
                assert np.array_equal(_np_state(st)["mom"], before["mom"])
    assert worst <= 1.0
    st0, gs = K.opt_case(name, 4099)
    assert (st0["w"][0::16] == 0).all() and (gs[0][0::16] == 0).all()
    if name in ("signsgd", "signum"):
        # the cap on excluded elements holds on the big inputs as well
        n = K.OPT_BIG_SCALAR
        st0, gs = K.opt_case(name, n)
        st = _torch_state(st0)
        for step, g in enumerate(gs):
            before = _np_state(st)
            K.opt_call(ref, name, st, torch.from_numpy(g), hp)
            _, ex = K.opt_check_step(name, before, _np_state(st), g, hp)
            assert ex <= K.SIGN_EXCLUDED_CAP, (name, step, ex)
            pre = K.opt_oracle(name, before, g, hp)["pre"]
            zero = pre.v == 0
            assert zero.sum() >= n // 16
            assert np.array_equal(_np_state(st)["w"][zero],
                                  before["w"][zero])


def test_adam_large_t_reference():
    hp = dict(K.OPT_HP["adam"], t=10000)
    st0, gs = K.opt_case("adam", 1025)
    st = _torch_state(st0)
    K.opt_call(ref, "adam", st, torch.from_numpy(gs[0]), hp)
    r, _ = K.opt_check_step("adam", st0, _np_state(st), gs[0], hp)
    assert r <= 1.0


def test_err_counts_roundings():
    """Err is the rounding count times 2^-24 times the magnitudes: for
    w - lr*(g*rs + wd*w) with unit terms that is 3 + 1 + 1 roundings."""
    one = K.Err(np.ones(1))
    e = one - 1.0 * (one * 1.0 + 1.0 * one)
    # g*rs: u; wd*w: u; sum 2: 2u + 2u; lr*: +2u; w - .: |-1| u
    assert e.e[0] == pytest.approx(7 * K.U32)


# ---------------------------------------------------------------------------
# pooling, wrapper helper
# ---------------------------------------------------------------------------

def test_pool_inputs_tie_and_oracle_is_aten():
    assert {s[1] for s in K.POOL_SHAPES} == {8, 16, 24}
    assert any(s[2] == 2 for s in K.POOL_SHAPES)
    assert any(s[3] == 2 for s in K.POOL_SHAPES)
    assert any((s[2] // 2) % 2 == 1 and (s[3] // 2) % 2 == 1
               for s in K.POOL_SHAPES)
    n, c, h, w = K.POOL_SHAPES[-1]
    assert n * h * w * c // 8 > 524288
    for shape in K.POOL_SHAPES[:-1]:
        x, go = K.pool_case(shape)
        out, codes, gin = K.pool_oracle(x, go)
        xf = x.float()
        win = torch.stack([xf[:, :, 0::2, 0::2], xf[:, :, 0::2, 1::2],
                           xf[:, :, 1::2, 0::2], xf[:, :, 1::2, 1::2]])
        mx = win.max(0).values
        ties = ((win == mx).sum(0) > 1) & (mx > 0)
        if xf.numel() >= 96:
            assert ties.float().mean() > 0.1       # ties are common
            assert (codes == 255).float().mean() > 0.05
        xr = xf.clone().requires_grad_(True)
        y = torch.nn.functional.max_pool2d(torch.nn.functional.relu(xr), 2, 2)
        y.backward(go.float())
        assert torch.equal(y.detach(), out)
        assert torch.equal(xr.grad, gin)


def test_flat_inplace_views_or_raises():
    t = torch.zeros(4, 6)
    flat = ops._flat_inplace(t, "w")
    flat[5] = 1.0
    assert t[0, 5] == 1.0                       # a view, never a copy
    with pytest.raises(ValueError, match="mom .*contiguous"):
        ops._flat_inplace(t.t(), "mom")
    with pytest.raises(ValueError, match="residual"):
        ops._flat_inplace(torch.zeros(10)[::2], "residual")
