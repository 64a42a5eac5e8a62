"""Fused wire reduce (csrc/wirereduce.hip) on gfx950. Every case checks
the fused sum twice: against a float64 sum of float64 decodes, within
(P + 2) * 2^-23 * sum_p a_p elementwise (a_p bounds party p's decode: at
most three roundings of magnitude <= 2|lo| + |hi| for a 4-bit code, none
otherwise; the fold adds at most P roundings of the running sum; the 2
covers second-order terms; a prior `out` counts as one more party), and
bit for bit against the chain of single-party ops the call sites used to
run."""
import pytest
import torch

from geomx_amd import ops
from geomx_amd.kvstore.dgt import DGTState

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = 2048 * 256  # threads of a full grid


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _check(fused, ref64, a64, chain, parties):
    bound = (parties + 2) * 2.0 ** -23 * a64
    err = (fused.double() - ref64).abs()
    assert bool((err <= bound).all()), \
        "max excess %g" % (err - bound).max().item()
    assert torch.equal(fused, chain)


def _prior(n, accumulate):
    if not accumulate:
        return None
    return torch.randn(n, device=DEV, generator=_gen(999))


def _run(fused_fn, decodes64, mags64, chain_decode, n, P, accumulate):
    """fused_fn(out, accumulate) -> tensor; chain_decode(p) -> fp32 dense."""
    prior = _prior(n, accumulate)
    out = prior.clone() if accumulate else torch.full((n,), 7.0, device=DEV)
    fused = fused_fn(out, accumulate)
    chain = prior.clone() if accumulate else torch.zeros(n, device=DEV)
    for p in range(P):
        chain += chain_decode(p)
    ref64 = sum(decodes64)
    a64 = sum(mags64)
    if accumulate:
        ref64 = ref64 + prior.double()
        a64 = a64 + prior.double().abs()
    _check(fused, ref64, a64, chain, P + int(accumulate))


# -- 2bit -------------------------------------------------------------------

N_BIG_2BIT = 2 * GRID * 4 + 7  # the grid-stride loop twice, and the tail
CASES_2BIT = [(n, P) for n in (1, 15, 16, 17, 63, 65, 4099)
              for P in (1, 2, 5, 16, 17, 33)] \
    + [(N_BIG_2BIT, 2), (N_BIG_2BIT, 17)]


def _decode2_f64(words, n, thr):
    shifts = torch.arange(16, device=DEV) * 2
    codes = ((words.long().unsqueeze(1) >> shifts) & 3).reshape(-1)[:n]
    t = float(torch.tensor(thr, dtype=torch.float32))  # what the kernel gets
    z = torch.zeros(n, dtype=torch.float64, device=DEV)
    return torch.where(codes == 3, z + t, torch.where(codes == 2, z - t, z))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n,P", CASES_2BIT)
def test_wire_sum_2bit(n, P, accumulate):
    for thr in (0.5, 0.3):  # 0.3 has a full mantissa: 3 * thr rounds
        payloads = []
        for p in range(P):
            g = torch.randn(n, device=DEV, generator=_gen(100 + p)) * thr * 1.5
            payloads.append(ops.quantize_2bit(
                g, torch.zeros(n, device=DEV), thr))
        dec = [_decode2_f64(w, n, thr) for w in payloads]
        if n >= 63:  # all three codes occur
            assert torch.stack(dec).unique().numel() == 3
        _run(lambda out, acc: ops.wire_sum_2bit(payloads, n, thr, out=out,
                                                accumulate=acc),
             dec, [d.abs() for d in dec],
             lambda p: ops.dequantize_2bit(payloads[p], n, thr),
             n, P, accumulate)


# -- fp16 -------------------------------------------------------------------

CASES_F16 = [(n, P, False) for n in (1, 7, 8, 9, 4099, GRID * 8 + 13)
             for P in (1, 3, 16, 17)] + [(4099, 3, True)]
SPECIAL_F16 = [0.0, -0.0, 6e-8, -6e-8, 6.0e-5, 65504.0, -65504.0]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n,P,misaligned", CASES_F16)
def test_wire_sum_fp16(n, P, misaligned, accumulate):
    payloads = []
    for p in range(P):
        h = torch.randn(n + 1, device=DEV, generator=_gen(200 + p)).half()
        sp = torch.tensor(SPECIAL_F16, device=DEV).half().roll(p)
        h[1:1 + min(n, sp.numel())] = sp[:n]
        # party 1 is a [1:] slice view (2 B past a 16 B boundary) in the
        # misaligned case; every other payload owns its storage
        payloads.append(h[1:] if misaligned and p == 1 else h[1:].clone())
    if misaligned:
        assert payloads[1].data_ptr() % 16 != 0
    dec = [h.double() for h in payloads]
    _run(lambda out, acc: ops.wire_sum_fp16(payloads, out=out,
                                            accumulate=acc),
         dec, [d.abs() for d in dec], lambda p: payloads[p].float(),
         n, P, accumulate)


# -- DGT mode 3 -------------------------------------------------------------

def _dgt_f64(payload, numel, chunk):
    exact, keep_idx, packed, minmax = payload
    nchunks = (numel + chunk - 1) // chunk
    keep = torch.zeros(nchunks, dtype=torch.bool, device=DEV)
    keep[keep_idx.long()] = True
    dense = torch.zeros(nchunks, chunk, dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(dense)
    n_lossy = nchunks - keep_idx.numel()
    if n_lossy:
        codes = torch.stack([packed & 15, packed >> 4], 1) \
            .reshape(n_lossy, chunk).double()
        lo = minmax.view(n_lossy, 2)[:, 0:1].double()
        hi = minmax.view(n_lossy, 2)[:, 1:2].double()
        dense[~keep] = lo + (codes + 0.5) * (hi - lo).clamp(min=1e-30) / 16
        mag[~keep] = (2 * lo.abs() + hi.abs()).expand(n_lossy, chunk)
    dense[keep] = exact.view(-1, chunk).double()
    mag[keep] = exact.view(-1, chunk).double().abs()
    return dense.reshape(-1)[:numel], mag.reshape(-1)[:numel]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("P", [1, 3, 17])
@pytest.mark.parametrize("k", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("numel,chunk", [(64, 64), (65, 64), (64 * 7 + 3, 64),
                                         (1024 * 37 + 1000, 1024)])
def test_wire_sum_dgt(numel, chunk, k, P, accumulate):
    states, payloads = [], []
    for p in range(P):
        x = torch.randn(numel, device=DEV, generator=_gen(300 + p)) * (p + 1)
        # per-chunk scale, different per party, so the keep sets differ
        x *= 1 + (torch.arange(numel, device=DEV) // chunk * (p + 3) % 5)
        if P > 1 and p == 0:
            x[:chunk] = 0.0       # a dead chunk for party 0 ...
        if p == 1:
            x[:chunk] *= 100.0    # ... that party 1 keeps at every k
        st = DGTState(numel, DEV, chunk_elems=chunk, k=k, mode=3)
        states.append(st)
        payloads.append(st.compress(x))
    if P > 1:
        assert 0 in payloads[1][1].tolist()
        if 0.0 < k < 1.0 and numel > chunk:
            assert 0 not in payloads[0][1].tolist()
        if numel > 4 * chunk and k == 0.5:
            assert payloads[0][1].tolist() != payloads[1][1].tolist()
    dm = [_dgt_f64(pl, numel, chunk) for pl in payloads]
    _run(lambda out, acc: ops.wire_sum_dgt(payloads, numel, chunk, out=out,
                                           accumulate=acc),
         [d for d, _ in dm], [m for _, m in dm],
         lambda p: states[p].decompress(*payloads[p]), numel, P, accumulate)


# -- binding rejections -----------------------------------------------------

def _good():
    n = 128
    w = torch.zeros(8, dtype=torch.int32, device=DEV)
    h = torch.zeros(n, dtype=torch.float16, device=DEV)
    dgt = (torch.zeros(64, device=DEV),
           torch.zeros(1, dtype=torch.int32, device=DEV),
           torch.zeros(32, dtype=torch.uint8, device=DEV),
           torch.zeros(1, 2, device=DEV))
    return n, w, h, dgt, torch.zeros(n, device=DEV)


REJECTS = {
    "dtype": lambda n, w, h, d, o: ops.wire_sum_2bit([w, w.float()], n, .5,
                                                     out=o),
    "cpu_payload": lambda n, w, h, d, o: ops.wire_sum_fp16([h, h.cpu()],
                                                           out=o),
    "numel": lambda n, w, h, d, o: ops.wire_sum_fp16([h, h[:-8]], out=o),
    "out_strided": lambda n, w, h, d, o: ops.wire_sum_2bit(
        [w], n, .5, out=torch.zeros(n, 2, device=DEV)[:, 0]),
    "no_party": lambda n, w, h, d, o: ops.wire_sum_2bit([], n, .5, out=o),
    "chunk48": lambda n, w, h, d, o: ops.wire_sum_dgt([d], n, 48, out=o),
}


@pytest.mark.parametrize("case", sorted(REJECTS))
def test_wire_sum_rejects(case):
    n, w, h, dgt, out = _good()
    # the operands themselves are accepted ...
    ops.wire_sum_2bit([w], n, .5, out=out)
    ops.wire_sum_fp16([h], out=out)
    ops.wire_sum_dgt([dgt], n, 64, out=out)
    # ... and each malformed call is refused
    with pytest.raises((RuntimeError, ValueError)):
        REJECTS[case](n, w, h, dgt, out)
    torch.cuda.synchronize()
