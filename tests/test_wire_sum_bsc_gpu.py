"""Fused Bi-Sparse wire reduce (csrc/wiresparse.hip) on gfx950. Every case
checks ops.wire_sum_bsc twice, as test_wire_reduce_gpu.py does: bit for bit
against the chain of single-party ops the call sites used to run (per party
DGTState.decompress for the coded form, then ops.bsc_decompress with
accumulate=True), and against a float64 sum of float64 decodes within
(P + 2) * 2^-23 * sum_p a_p (a_p = |value|, or 2|lo| + |hi| for a 4-bit
code; a prior `out` counts as one more party). The CPU test at the end
checks the reference sequence the gloo call sites run."""
import pytest
import torch

from geomx_amd import ops
from geomx_amd.kvstore.dgt import DGTState
from geomx_amd.ops import reference as ref

from test_wire_reduce_gpu import _check, _dgt_f64

gpu = pytest.mark.gpu
DEV = "cuda:0"
T = ops.WIRE_BSC_TILE or 8192  # the kernel's tile; None without the extension
HOT = (1e8, 1.0, -1e8, 3.0)    # a wrong fold order changes these bits


def _lists(n, P, dev, chunk=0):
    """P lists (vals, idx) of one length k, each ascending with an entry
    >= n and the placeholders behind it. Every party with entries names
    index n // 2, with the values HOT; party 0 names 0, n - 1 and T - 1 but
    not T, the last party T but not T - 1; with P >= 3, party 1 is all
    placeholders and party 2 lies inside the tile of n // 2; the longest
    party has no placeholder. `chunk`: party 0's first two chunks of values
    are 0.0, dead chunks for DGT; the last party names their indices too (a
    dead code decodes to 3e-32 where a_p is 0, as in test_wire_reduce_gpu)."""
    gen = torch.Generator(device=dev).manual_seed(1000 * P + n % 997)
    dens = 0.5 if n <= 4 * T else 0.01
    hot = n // 2
    sets = []
    for p in range(P):
        m = torch.rand(n, device=dev, generator=gen) < dens
        if P >= 3 and p == 1:
            m[:] = False
        else:
            if P >= 3 and p == 2:
                m[:hot // T * T] = False
                m[(hot // T + 1) * T:] = False
            m[hot] = True
            if p == 0:
                m[0] = m[n - 1] = True
            elif chunk and p == P - 1:
                m[sets[0][:2 * chunk].long()] = True
            for q, e in ((0, T - 1), (P - 1, T)):
                if e < n and e != hot and P > 1:
                    m[e] = p == q
        sets.append(m.nonzero().reshape(-1).to(torch.int32))
    k = max(s.numel() for s in sets) + 1
    out = []
    for p, s in enumerate(sets):
        idx = torch.full((k,), -1, dtype=torch.int32, device=dev)
        vals = torch.full((k,), ref.BSC_PLACEHOLDER, device=dev)
        idx[:s.numel()] = s
        idx[s.numel()] = n + p  # skipped as k_bsc_unpack skips it
        vals[:s.numel() + 1] = torch.randn(s.numel() + 1, device=dev,
                                           generator=gen)
        if chunk and p == 0 and s.numel() > 3 * chunk:
            vals[:2 * chunk] = 0.0
        vals[:s.numel()][s == hot] = HOT[p % 4]
        out.append((vals, idx))
    assert any((i >= 0).all() for _, i in out)
    return out


def _run(n, P, accumulate, unaligned=False, chunk=0, kfrac=1.0):
    lists = _lists(n, P, DEV, chunk)
    k = lists[0][1].numel()
    if chunk:  # exactly as the bsc_dgt call sites make the payload
        states = [DGTState(k, DEV, chunk_elems=chunk, k=kfrac, mode=3)
                  for _ in range(P)]
        payloads = [st.compress(v.masked_fill(i < 0, 0.0)) + (i,)
                    for st, (v, i) in zip(states, lists)]
        assert (payloads[0][2].numel() == 0) == (kfrac == 1.0 or k <= chunk)
    else:
        payloads = lists
    prior = torch.randn(n, device=DEV) if accumulate else None
    out = torch.full((n + 1,), 7.0, device=DEV)[1:] if unaligned \
        else torch.full((n,), 7.0, device=DEV)
    if accumulate:
        out.copy_(prior)
    fused = ops.wire_sum_bsc(payloads, n, out=out, accumulate=accumulate,
                             chunk_elems=chunk or None)
    assert fused.data_ptr() == out.data_ptr()

    chain = prior.clone() if accumulate else torch.zeros(n, device=DEV)
    ref64 = chain.double()
    a64 = ref64.abs()
    for p, pl in enumerate(payloads):
        idx = pl[-1]
        if chunk:
            vals = states[p].decompress(*pl[:4]).contiguous()
            v64, m64 = _dgt_f64(pl[:4], k, chunk)
        else:
            vals = pl[0]
            v64, m64 = vals.double(), vals.double().abs()
        ops.bsc_decompress(vals, idx, n, out=chain, accumulate=True)
        ok = (idx >= 0) & (idx < n)
        ref64.index_add_(0, idx[ok].long(), v64[ok])
        a64.index_add_(0, idx[ok].long(), m64[ok])
    _check(fused, ref64, a64, chain, P + int(accumulate))


NS = (1, 7, T - 1, T, T + 1, 3 * T + 5)


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n,P", [(n, P) for n in NS
                                 for P in (1, 2, 5, 16, 17, 33)]
                         + [(2048 * T + T + 3, 2)])  # grid-stride twice
def test_wire_sum_bsc_plain(n, P, accumulate):
    _run(n, P, accumulate)


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n,P", [(7, 2), (T + 1, 5), (3 * T + 5, 5)])
def test_wire_sum_bsc_unaligned_out(n, P, accumulate):
    _run(n, P, accumulate, unaligned=True)


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("kfrac", [0.5, 1.0])
@pytest.mark.parametrize("chunk", [64, 1024])
@pytest.mark.parametrize("n,P", [(7, 2), (T + 1, 5), (3 * T + 5, 3),
                                 (3 * T + 5, 17)])
def test_wire_sum_bsc_coded(n, P, chunk, kfrac, accumulate):
    _run(n, P, accumulate, chunk=chunk, kfrac=kfrac)


@pytest.mark.parametrize("n,P", [(7, 2), (3 * T + 5, 5)])
def test_reference_wire_sum_bsc_cpu(n, P):
    lists = _lists(n, P, "cpu")
    prior = torch.randn(n)
    for accumulate in (False, True):
        want = prior.clone() if accumulate else torch.zeros(n)
        for v, i in lists:
            ref.bsc_decompress(v[i < n], i[i < n], n, out=want,
                               accumulate=True)
        out = prior.clone()
        got = ops.wire_sum_bsc(lists, n, out=out, accumulate=accumulate)
        assert got is out and torch.equal(got, want)
        if not accumulate:
            assert torch.equal(ops.wire_sum_bsc(lists, n), want)
