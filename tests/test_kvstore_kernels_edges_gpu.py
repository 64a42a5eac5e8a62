"""Edge-exact tests of the kvstore kernels (csrc/kernels.hip) on gfx950:
2-bit, Bi-Sparse (fused, fallback chain, pinned boundary), DGT, 4-bit,
the eight server optimizers and the unfused ReLU+pool, against the seeded
inputs and oracles of tests/kvstore_edge_cases.py. Bit-equality wherever
the arithmetic is exact; a derived per-element bound elsewhere
(docs/testing.md, "kvstore kernel edges")."""

import numpy as np
import pytest
import torch

import geomx_amd.ops as ops
from geomx_amd.ops import reference as ref

import kvstore_edge_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"


def _dev(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.to(DEV)


def _bits(t):
    """fp32 tensor or array as int32 bit patterns on the host: compares
    -0.0 / +0.0 and subnormals exactly."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _offset_view(t):
    """Same values as `t`, stored one element into a larger buffer: a
    4-byte-aligned view the float4 kernels must refuse."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------
# 2-bit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("thr", K.TWOBIT_THRESHOLDS)
def test_quantize_2bit_exact_on_threshold_grid(thr):
    """Three chained calls from a non-zero residual; residual + grad lies
    on +/-thr, one ulp either side, +/-0 and far away. Words AND residual
    are bit-equal: each residual is one fp32 add and one subtract."""
    for n in K.TWOBIT_SIZES:
        r0, grads, _ = K.twobit_case(n, thr)
        r_g, r_o = _dev(r0.copy()), r0
        for step, g in enumerate(grads):
            w_g = ops.quantize_2bit(_dev(g), r_g, thr)
            w_o, r_o = K.twobit_oracle(r_o, g, thr)
            assert np.array_equal(w_g.cpu().numpy(), w_o), (n, step)
            assert np.array_equal(_bits(r_g), _bits(r_o)), (n, step)
            d_g = ops.dequantize_2bit(w_g, n, thr)
            assert np.array_equal(
                _bits(d_g), _bits(K.twobit_dequant_oracle(w_o, n, thr)))


@pytest.mark.parametrize("thr", K.TWOBIT_THRESHOLDS)
def test_dequantize_2bit_arbitrary_words(thr):
    """Arbitrary words (all four codes, the invalid 01 included), n % 4
    in 0..3 and never a multiple of 16, packed buffer longer than needed."""
    for n in K.TWOBIT_DEQUANT_SIZES:
        w = K.twobit_dequant_case(n)
        out = torch.full((n + 8,), 7.0, device=DEV)
        ops.dequantize_2bit(_dev(w), n, thr, out=out[:n])
        assert np.array_equal(_bits(out[:n]),
                              _bits(K.twobit_dequant_oracle(w, n, thr))), n
        assert (out[n:] == 7.0).all(), n        # nothing past n is written


# ---------------------------------------------------------------------------
# Bi-Sparse
# ---------------------------------------------------------------------------

def _bsc_gpu(path, g, u, v, ratio, boundary, monkeypatch):
    """One compress step on the device through `path`."""
    geops = ops._geops
    if path == "fused":
        return ops.bsc_compress(g, u, v, ratio)
    if path == "fallback":
        with monkeypatch.context() as m:
            m.setattr(geops, "bsc_compress_fused", lambda *a: False)
            return ops.bsc_compress(g, u, v, ratio)
    k = ref.bsc_capacity(g.numel(), ratio)
    vals = torch.empty(k, device=DEV)
    idx = torch.empty(k, dtype=torch.int32, device=DEV)
    if path == "pinned":
        geops.bsc_momentum(g, u, v, K.BSC_MU)
        geops.bsc_pack(v, u, vals, idx, boundary, ref.BSC_PLACEHOLDER)
    else:   # "fused_pinned": the fused kernel with a given boundary
        bt = torch.tensor([boundary], device=DEV)
        assert geops.bsc_compress_fused(g, u, v, vals, idx, bt, K.BSC_MU,
                                        ref.BSC_PLACEHOLDER)
    return vals, idx


def _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, tag):
    assert torch.equal(got[1].cpu(), want[1]), tag
    assert np.array_equal(_bits(got[0]), _bits(want[0])), tag
    assert np.array_equal(_bits(u_g), _bits(u_c)), tag
    assert np.array_equal(_bits(v_g), _bits(v_c)), tag


@pytest.mark.parametrize("path", ["fused", "fallback", "pinned",
                                  "fused_pinned"])
def test_bsc_chain_bit_equal(path, monkeypatch):
    """4-step error-feedback chain from non-zero u and v: u, v, vals and
    idx are bit-equal to ref.bsc_compress at every size and step."""
    ratio = 0.01
    for n in K.BSC_SIZES:
        u0, v0, gs = K.bsc_chain_case(n)
        u_c, v_c = u0.clone(), v0.clone()
        u_g, v_g = u0.to(DEV), v0.to(DEV)
        pinned = path in ("pinned", "fused_pinned")
        for step, g in enumerate(gs):
            b = 2.5 + step if pinned else None
            want = ref.bsc_compress(g, u_c, v_c, ratio, boundary=b)
            got = _bsc_gpu(path, g.to(DEV), u_g, v_g, ratio, b, monkeypatch)
            _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, (n, step))


@pytest.mark.parametrize("path", ["fused", "fallback"])
def test_bsc_boundary_flip(path, monkeypatch):
    """The element that defines the sampled boundary is sent: its |v|
    must be rounded as the boundary prediction rounds it (multiply, then
    add). A fused multiply-add lands one ulp below and sends 9, not 10."""
    c = K.bsc_flip_case()
    u_c, v_c = c["u"].clone(), c["v"].clone()
    want = ref.bsc_compress(c["g"], u_c, v_c, K.FLIP_RATIO)
    u_g, v_g = c["u"].to(DEV), c["v"].to(DEV)
    got = _bsc_gpu(path, c["g"].to(DEV), u_g, v_g, K.FLIP_RATIO, None,
                   monkeypatch)
    sent = got[1][got[1] >= 0].cpu().tolist()
    print("flip: sent %d, flip element sent: %s" % (len(sent),
                                                    c["flip"] in sent))
    assert len(sent) == 10 and c["flip"] in sent
    _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, path)


@pytest.mark.parametrize("path", ["pinned", "fused_pinned"])
def test_bsc_boundary_ties(path, monkeypatch):
    """|v| == boundary is sent, nextafter(boundary, 0) is kept, both
    signs."""
    g, u0, v0, at, below = K.bsc_tie_case()
    ratio = K.ratio_for(g.numel(), 3000)
    u_c, v_c = u0.clone(), v0.clone()
    want = ref.bsc_compress(g, u_c, v_c, ratio, boundary=K.BSC_TIE_BOUNDARY)
    u_g, v_g = u0.to(DEV), v0.to(DEV)
    got = _bsc_gpu(path, g.to(DEV), u_g, v_g, ratio, K.BSC_TIE_BOUNDARY,
                   monkeypatch)
    sent = set(got[1][got[1] >= 0].cpu().tolist())
    assert set(at.tolist()) <= sent and not (set(below.tolist()) & sent)
    _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, path)


def test_bsc_1024_blocks_single_step():
    """n = 16384*1024 - 5: 1024 blocks, the whole decoupled-lookback chain
    of the fused kernel; one step from non-zero state."""
    n = K.BSC_BIG_N
    u0, v0, gs = K.bsc_chain_case(n, steps=1)
    u_c, v_c = u0.clone(), v0.clone()
    want = ref.bsc_compress(gs[0], u_c, v_c, 0.01)
    u_g, v_g = u0.to(DEV), v0.to(DEV)
    got = ops.bsc_compress(gs[0].to(DEV), u_g, v_g, 0.01)
    _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, n)


@pytest.mark.parametrize("path", ["pinned", "fused_pinned"])
def test_bsc_capacity_cases(path, monkeypatch):
    """Capacity cut inside one thread's 4 (pack) / 8 (fused) elements,
    count == capacity, nothing selected, capacity 0."""
    n = 5000
    u0, v0, gs = K.bsc_chain_case(n, seed=9, steps=1)
    g = gs[0]
    vv = v0 + (u0 * K.BSC_MU + g)
    b = 1.0
    count = int((vv.abs() >= b).sum())
    first = (vv.abs() >= b).nonzero().reshape(-1)
    # a cut after the 1st, 2nd, 3rd, 5th, 6th selected element of the
    # first threads, and inside a later thread's group
    cases = [(b, c) for c in (0, 1, 2, 3, 5, 6, 7, count - 1, count,
                              count + 1, count + 9)]
    cases += [(1e30, 16), (1e30, 0)]            # nothing selected
    # all of the first 8 elements selected, cut in the middle of them
    dense = g.clone()
    dense[:16] = 40.0
    for boundary, cap in cases + [("dense", 3), ("dense", 6)]:
        gg = g
        if boundary == "dense":
            gg, boundary = dense, b
        ratio = K.ratio_for(n, cap)
        u_c, v_c = u0.clone(), v0.clone()
        want = ref.bsc_compress(gg, u_c, v_c, ratio, boundary=boundary)
        u_g, v_g = u0.to(DEV), v0.to(DEV)
        got = _bsc_gpu(path, gg.to(DEV), u_g, v_g, ratio, boundary,
                       monkeypatch)
        assert got[0].numel() == cap
        _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, (boundary, cap))
    assert first.numel() == count and count > 16


def test_bsc_ratio_one_sends_everything():
    n = 5000
    gen = torch.Generator().manual_seed(11)
    g = torch.where(torch.rand(n, generator=gen) < 0.5, 3.0, -3.0)
    u_c, v_c = torch.zeros(n), torch.zeros(n)
    want = ref.bsc_compress(g, u_c, v_c, 1.0)
    u_g, v_g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    got = ops.bsc_compress(g.to(DEV), u_g, v_g, 1.0)
    assert torch.equal(got[1].cpu(), torch.arange(n, dtype=torch.int32))
    _assert_bsc_equal(got, u_g, v_g, want, u_c, v_c, "ratio 1")
    assert not u_g.any() and not v_g.any()


@pytest.mark.parametrize("cap", ["all", "count", "cut", 0])
def test_bsc_pull_pack_subnormals_and_zeros(cap):
    """Subnormals are packed, -0.0 / +0.0 are not, in the first block: the
    count kernel (x != 0) and the pack kernel (|x| >= 2^-149) agree."""
    x = K.bsc_pull_case()
    count = int((x != 0).sum())
    cap = {"all": x.numel(), "count": count, "cut": count - 7, 0: 0}[cap]
    want = ref.bsc_pull_compress(x, cap)
    got = ops.bsc_pull_compress(x.to(DEV), cap)
    assert torch.equal(got[1].cpu(), want[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))


def test_bsc_unpack_accumulate_and_overwrite():
    """Accumulation runs on atomics in no fixed order. It equals the
    sequential sum bit for bit only when at most two values share a slot of
    a zeroed `out` (fp32 addition is commutative, not associative); that is
    what this test uses. With a non-zero `out` the indices are unique."""
    n, k = 3000, 1500
    gen = torch.Generator().manual_seed(12)
    vals = torch.randn(k, generator=gen)
    idx = torch.randperm(n, generator=gen)[:k].to(torch.int32)
    idx[1000:] = idx[:500]                      # 500 slots get two values
    idx[7], idx[1400] = -1, -1                  # placeholders
    # zeroed out, pairs
    want = K.bsc_unpack_oracle(vals, idx, torch.zeros(n), True)
    got = ops.bsc_decompress(_dev(vals), _dev(idx), n)
    assert np.array_equal(_bits(got), _bits(want))
    # non-zero out, unique indices, accumulate and overwrite
    base = torch.randn(n, generator=gen)
    for acc in (True, False):
        want = K.bsc_unpack_oracle(vals[:1000], idx[:1000], base.clone(),
                                   acc)
        out = base.to(DEV)
        ops.bsc_decompress(_dev(vals[:1000]), _dev(idx[:1000]), n, out=out,
                           accumulate=acc)
        assert np.array_equal(_bits(out), _bits(want)), acc


@pytest.mark.parametrize("accumulate", [True, False])
def test_bsc_unpack_skips_out_of_range(accumulate):
    """Indices n .. n+guard-1 come off the wire from another rank: they
    are skipped. `out` is the front of a larger buffer, so those indices
    stay inside the allocation; the guard region must not change."""
    n, guard = 1000, 64
    buf = torch.full((n + guard,), 5.0, device=DEV)
    out = buf[:n]
    gen = torch.Generator().manual_seed(13)
    idx = torch.cat([torch.randperm(n, generator=gen)[:200],
                     torch.arange(n, n + guard),
                     torch.tensor([-1, -1])]).to(torch.int32)
    idx = idx[torch.randperm(idx.numel(), generator=gen)]
    vals = torch.randn(idx.numel(), generator=gen)
    assert int(idx.max()) == n + guard - 1 < buf.numel()
    want = K.bsc_unpack_oracle(vals, idx, torch.full((n,), 5.0), accumulate)
    ops.bsc_decompress(_dev(vals), _dev(idx), n, out=out,
                       accumulate=accumulate)
    assert np.array_equal(_bits(out), _bits(want))
    assert (buf[n:] == 5.0).all()


# ---------------------------------------------------------------------------
# DGT contribution
# ---------------------------------------------------------------------------

def test_dgt_contribution_exact_on_integers():
    """|g| <= 3 integers: every partial sum is exact in fp32 and the divide
    is correctly rounded, so the result is the float64 mean rounded once.
    Chunks that are no multiple of 4 take the scalar loop."""
    for n, chunk in K.DGT_CASES:
        g = K.dgt_int_case(n)
        got = ops.dgt_contribution(_dev(g), chunk)
        want = K.dgt_oracle(g, chunk).astype(np.float32)
        assert got.numel() == (n + chunk - 1) // chunk
        assert np.array_equal(_bits(got), _bits(want)), (n, chunk)


def test_dgt_contribution_randn_within_summation_bound():
    worst = 0.0
    for n, chunk in K.DGT_CASES:
        g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        got = ops.dgt_contribution(_dev(g), chunk).cpu().numpy()
        err = np.abs(got.astype(np.float64) - K.dgt_oracle(g, chunk))
        ratio = float((err / K.dgt_bound(g, chunk)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (n, chunk, ratio)
    print("dgt worst error/bound: %.3f" % worst)


# ---------------------------------------------------------------------------
# 4-bit
# ---------------------------------------------------------------------------

def test_quantize_4bit_exact_on_dyadic_grid():
    """3-step residual chain on a grid where step, 1/step and every product
    are exact: minmax, codes, dequantised values and residual are bit-equal
    to the float64 oracle. Bin edges, x == max, constant chunks, chunks of
    4 and 8, ragged tails, more chunks than blocks."""
    for n, chunk in K.Q4_CASES:
        chain = K.q4_grid_chain(n, chunk)
        res = _dev(chain[0][1].copy())
        for step, (x, res_in, f) in enumerate(chain):
            tag = (n, chunk, step)
            assert np.array_equal(_bits(res), _bits(res_in)), tag
            mm, codes, deq, r_new = K.q4_oracle(f, chunk)
            p, mm_g = ops.quantize_4bit_chunked(_dev(x), chunk, res)
            assert np.array_equal(_bits(mm_g), _bits(mm)), tag
            assert np.array_equal(p.cpu().numpy(), K.q4_pack(codes)), tag
            assert np.array_equal(_bits(res), _bits(r_new)), tag
            y = ops.dequantize_4bit_chunked(p, mm_g, n, chunk)
            assert np.array_equal(_bits(y), _bits(deq)), tag
        # without a residual: x is quantised as it is
        x, _, f = chain[0]
        mm, codes, _, _ = K.q4_oracle(x, chunk)
        p, mm_g = ops.quantize_4bit_chunked(_dev(x), chunk)
        assert np.array_equal(_bits(mm_g), _bits(mm)), (n, chunk)
        assert np.array_equal(p.cpu().numpy(), K.q4_pack(codes)), (n, chunk)


def test_quantize_4bit_randn_within_half_step():
    worst = 0.0
    for n, chunk in K.Q4_CASES:
        rng = np.random.default_rng(n + chunk)
        x = rng.standard_normal(n).astype(np.float32)
        res0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
        f = (x + res0).astype(np.float32)
        res = _dev(res0.copy())
        p, mm_g = ops.quantize_4bit_chunked(_dev(x), chunk, res)
        mm = mm_g.cpu().numpy()
        assert np.array_equal(_bits(mm), _bits(K.q4_oracle(f, chunk)[0]))
        codes = K.q4_unpack(p.cpu().numpy(), n)
        assert codes.min() >= 0 and codes.max() <= 15
        deq = ops.dequantize_4bit_chunked(p, mm_g, n, chunk).cpu().numpy() \
            .astype(np.float64)
        bound, step = K.q4_randn_bound(mm, n, chunk)
        e1 = np.abs(deq - f)
        e2 = np.abs(res.cpu().numpy() - (f.astype(np.float64) - deq))
        assert (e1 <= bound).all(), (n, chunk)
        assert (e2 <= bound - step / 2).all(), (n, chunk)
        worst = max(worst, float(((e1 - step / 2) /
                                  (bound - step / 2)).max()),
                    float((e2 / (bound - step / 2)).max()))
    print("4-bit worst excess over step/2, in units of the ulp term: %.3f"
          % worst)


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------

def _to_dev(st):
    return {k: _dev(v.copy()) for k, v in st.items()}


def _to_np(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


@pytest.mark.parametrize("name", sorted(K.OPT_HP))
def test_optimizer_within_derived_bound(name):
    """3 steps with wd and rescale non-trivial. Each step is compared with
    the float64 oracle started from the kernel's own fp32 state, element by
    element, against twice the running rounding bound. For the sign
    optimizers an element is left out of the comparison of w only where
    the oracle's pre-sign magnitude is below its own bound (<= 0.1 %);
    exact zeros are compared and leave w unchanged."""
    hp = dict(K.OPT_HP[name])
    worst, worst_excl = 0.0, 0.0
    for n in K.opt_sizes(name):
        st0, gs = K.opt_case(name, n)
        st = _to_dev(st0)
        for step, g in enumerate(gs):
            hp["t"] = step + 1
            before = _to_np(st)
            K.opt_call(ops, name, st, _dev(g), hp)
            after = _to_np(st)
            r, ex = K.opt_check_step(name, before, after, g, hp)
            worst, worst_excl = max(worst, r), max(worst_excl, ex)
            if n > 1025:
                assert ex <= K.SIGN_EXCLUDED_CAP, (name, n, step, ex)
            if name == "dcasgd_mom0":       # mom given, momentum == 0
                assert np.array_equal(_bits(after["mom"]),
                                      _bits(before["mom"]))
            if name in ("signsgd", "signum"):
                zero = K.opt_oracle(name, before, g, hp)["pre"].v == 0
                assert zero[0::16].all()
                assert np.array_equal(_bits(after["w"][zero]),
                                      _bits(before["w"][zero]))
    print("%s worst error/bound %.3f, excluded %.2e" % (name, worst,
                                                       worst_excl))


@pytest.mark.parametrize("t", [1, 10000])
def test_adam_step_count_and_exact_fixed_point(t):
    """t = 1 and t = 10000 (lr_t is formed in double on the host); with
    wd = 0, elements whose g, m and v are all 0 keep w bit for bit."""
    hp = dict(K.OPT_HP["adam"], t=t)
    for n in (1025, K.OPT_BIG_FLOAT4):
        st0, gs = K.opt_case("adam", n)
        st = _to_dev(st0)
        K.opt_call(ops, "adam", st, _dev(gs[0]), hp)
        r, _ = K.opt_check_step("adam", st0, _to_np(st), gs[0], hp)
        assert r <= 1.0
    hp["wd"] = 0.0
    st0, gs = K.opt_case("adam", 1027)
    st0["w"] = np.random.default_rng(1).standard_normal(1027) \
        .astype(np.float32)
    fixed = (gs[0] == 0) & (st0["m"] == 0) & (st0["v"] == 0)
    assert fixed.sum() >= 64 and (st0["w"][fixed] != 0).all()
    st = _to_dev(st0)
    K.opt_call(ops, "adam", st, _dev(gs[0]), hp)
    after = _to_np(st)
    for k in ("w", "m", "v"):
        assert np.array_equal(_bits(after[k][fixed]), _bits(st0[k][fixed]))
    assert K.opt_check_step("adam", st0, after, gs[0], hp)[0] <= 1.0


@pytest.mark.parametrize("name", ["signsgd", "signum"])
def test_sign_of_exact_zero_leaves_w(name):
    """wd = 0, g = 0 (and mom = 0): the pre-sign value is exactly 0 for a
    non-zero w, which must come back bit for bit."""
    hp = dict(K.OPT_HP[name], wd=0.0)
    n = 1025
    st0, gs = K.opt_case(name, n)
    st0["w"] = np.random.default_rng(2).standard_normal(n).astype(np.float32)
    zero = gs[0] == 0
    if name == "signum":
        zero &= st0["mom"] == 0
    assert zero.sum() >= 64
    st = _to_dev(st0)
    K.opt_call(ops, name, st, _dev(gs[0]), hp)
    after = _to_np(st)
    assert np.array_equal(_bits(after["w"][zero]), _bits(st0["w"][zero]))
    assert (after["w"][~zero] != st0["w"][~zero]).any()


# ---------------------------------------------------------------------------
# ReLU + pool
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=str)
def test_relu_pool_ties_match_first_maximum(shape):
    """Small-integer bf16 inputs: most windows tie or clamp. Output and
    input gradient equal ATen's; the recorded codes equal the explicit
    first-maximum oracle (order (0,0),(0,1),(1,0),(1,1); 255 where the
    maximum is <= 0)."""
    geops = ops._geops
    n, c, h, w = shape
    x, go = K.pool_case(shape)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    gd = go.to(DEV).contiguous(memory_format=torch.channels_last)
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.bfloat16,
                      device=DEV, memory_format=torch.channels_last)
    codes = torch.empty(n * (h // 2) * (w // 2) * c, dtype=torch.uint8,
                        device=DEV)
    geops.relu_maxpool2_fwd(xd, out, codes, n, c, h, w)
    gin = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=DEV,
                      memory_format=torch.channels_last)
    geops.relu_maxpool2_bwd(gd, codes, gin, n, c, h, w)
    o_out, o_codes, o_gin = K.pool_oracle(x, go)
    assert torch.equal(codes.cpu().view(o_codes.shape), o_codes)
    assert torch.equal(out.cpu().float(), o_out)
    assert torch.equal(gin.cpu().float(), o_gin)
    xr = xd.detach().clone().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(torch.nn.functional.relu(xr), 2, 2)
    y.backward(gd)
    assert torch.equal(out, y.detach())
    assert torch.equal(gin, xr.grad)


# ---------------------------------------------------------------------------
# wrapper contract
# ---------------------------------------------------------------------------

def _opt_args(name, n=64):
    st0, gs = K.opt_case(name, n)
    return _to_dev(st0), _dev(gs[0]), dict(K.OPT_HP[name], t=1)


@pytest.mark.parametrize("name", ["sgd", "sgd_mom", "adam", "rmsprop",
                                  "adagrad", "signsgd", "signum",
                                  "dcasgd_mom"])
def test_noncontiguous_inplace_operand_raises(name):
    """w and every state: a non-contiguous tensor is an error naming the
    argument, raised before any launch, and nothing is modified."""
    st, g, hp = _opt_args(name)
    for key in st:
        bad = {k: v.clone() for k, v in st.items()}
        wide = torch.zeros(64, 2, device=DEV)
        wide[:, 0] = st[key]
        bad[key] = wide[:, 0]
        assert not bad[key].is_contiguous()
        keep = {k: v.clone() for k, v in bad.items()}
        arg = {"prev_w": "prev_w"}.get(key, key)
        with pytest.raises(ValueError, match="^" + arg + " is updated in place"):
            K.opt_call(ops, name, bad, g, hp)
        for k in bad:
            assert torch.equal(bad[k], keep[k])


@pytest.mark.parametrize("n", [64, 63])
@pytest.mark.parametrize("name", ["sgd", "sgd_mom", "adam", "rmsprop",
                                  "adagrad", "signsgd", "signum",
                                  "dcasgd_mom"])
def test_short_operand_raises(name, n):
    """g and every state one element short of w: the kernels take their
    length from w, so this is an error naming the argument, raised before
    any launch, and nothing is modified."""
    st, g, hp = _opt_args(name, n)
    for key in ["g"] + K.OPT_STATES[name]:
        bad = {k: v.clone() for k, v in st.items()}
        bad_g = g.clone()
        if key == "g":
            bad_g = bad_g[:n - 1]
        else:
            bad[key] = bad[key][:n - 1]
        keep = {k: v.clone() for k, v in bad.items()}
        with pytest.raises(RuntimeError,
                           match="^" + key + " must have as many elements as w"):
            K.opt_call(ops, name, bad, bad_g, hp)
        for k in bad:
            assert torch.equal(bad[k], keep[k])
        assert torch.equal(bad_g, g[:bad_g.numel()])


def test_noncontiguous_residual_and_out_raise():
    n = 64
    wide = torch.zeros(n, 2, device=DEV)
    g = torch.randn(n, device=DEV)
    with pytest.raises(ValueError, match="^residual is updated in place"):
        ops.quantize_2bit(g, wide[:, 0], 0.5)
    with pytest.raises(ValueError, match="^residual is updated in place"):
        ops.quantize_4bit_chunked(g, 8, wide[:, 0])
    w = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="^out is updated in place"):
        ops.dequantize_2bit(w, n, 0.5, out=wide[:, 0])
    p, mm = ops.quantize_4bit_chunked(g, 8)
    with pytest.raises(ValueError, match="^out is updated in place"):
        ops.dequantize_4bit_chunked(p, mm, n, 8, out=wide[:, 0])
    vals = torch.ones(2, device=DEV)
    idx = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="^out is updated in place"):
        ops.bsc_decompress(vals, idx, n, out=wide[:, 0], accumulate=True)
    for bad in ("u", "v"):
        u = wide[:, 0] if bad == "u" else torch.zeros(n, device=DEV)
        v = wide[:, 0] if bad == "v" else torch.zeros(n, device=DEV)
        with pytest.raises(ValueError, match="^" + bad + " is updated in place"):
            ops.bsc_compress(g, u, v, 0.5)
    assert not wide.any()


def test_misaligned_view_raises_naming_the_argument():
    """A 4-byte-offset view cannot take the float4 path: the binding
    refuses it by name instead of issuing a misaligned 16-byte access."""
    st, g, hp = _opt_args("sgd_mom")
    for key, arg in (("w", "w"), ("mom", "mom")):
        bad = dict(st)
        bad[key] = _offset_view(st[key])
        with pytest.raises(RuntimeError,
                           match=arg + " must be 16-byte aligned"):
            K.opt_call(ops, "sgd_mom", bad, g, hp)
    with pytest.raises(RuntimeError, match="g must be 16-byte aligned"):
        K.opt_call(ops, "sgd_mom", st, _offset_view(g), hp)
    with pytest.raises(RuntimeError,
                       match="residual must be 16-byte aligned"):
        ops.quantize_2bit(g, _offset_view(torch.zeros_like(g)), 0.5)
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        ops.bsc_decompress(torch.ones(2, device=DEV),
                           torch.tensor([1, 2], dtype=torch.int32,
                                        device=DEV), 64,
                           out=_offset_view(torch.zeros(64, device=DEV)),
                           accumulate=True)
