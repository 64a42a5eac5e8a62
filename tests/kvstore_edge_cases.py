"""Seeded inputs and plain oracles for the kvstore kernels of
csrc/kernels.hip (2-bit, Bi-Sparse, DGT, 4-bit, the eight server
optimizers, the unfused ReLU+pool). Imports without a GPU.

Two kinds of oracle live here:

  * exact ones (2-bit, DGT on integers, 4-bit on a dyadic grid, pooling):
    integer or float64 arithmetic in which every fp32 operation of the
    kernel is exact, so the kernel result must be BIT-equal;
  * float64 ones with a per-element error bound (optimizers, DGT and 4-bit
    on randn inputs). The bound is a running first-order error analysis
    of the kernel's expression (class Err): every fp32 rounding adds
    2^-24 x |intermediate|, and errors propagate through the later
    operations by the magnitude of the other operand. That is the
    per-element form of "number of roundings x 2^-24 x sum of the term
    magnitudes". The tests use TWICE that figure: the compiler is free to
    contract a*b+c into one fused multiply-add, which removes roundings but
    changes which intermediate is rounded.

tests/test_kvstore_edge_cases_cpu.py checks without a GPU that the inputs
contain the edges they claim and that the fp32 reference alone stays within
every bound; tests/test_kvstore_kernels_edges_gpu.py runs the kernels.
"""

from fractions import Fraction

import numpy as np
import torch

from geomx_amd.ops import reference as ref

U32 = 2.0 ** -24           # fp32 unit roundoff
F32_TINY = 2.0 ** -149     # smallest subnormal: absolute floor of a bound
MARGIN = 2.0               # contraction freedom, see the module docstring

LADDER = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024,
          1025]


def f32(x):
    return np.asarray(x, dtype=np.float32)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def p32(x: float) -> float:
    """A Python scalar as the kernels and the fp32 reference see it."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------
# 2-bit
# ---------------------------------------------------------------------------

TWOBIT_THRESHOLDS = (0.5, 0.1)
TWOBIT_SIZES = LADDER + [2 * 524288 + 37]
# kinds of target for residual + grad, by position modulo len(TWOBIT_KINDS)
TWOBIT_KINDS = ("at+", "below+", "above+", "at-", "below-", "above-",
                "zero+", "zero-", "far", "far", "near", "near")


def _twobit_targets(n, thr, rng):
    t = np.float32(thr)
    kind = np.arange(n) % len(TWOBIT_KINDS)
    kind = kind[rng.permutation(n)] if n > 1 else kind
    up = np.nextafter(t, np.float32(np.inf))
    dn = np.nextafter(t, np.float32(0))
    table = {
        0: np.full(n, t), 1: np.full(n, dn), 2: np.full(n, up),
        3: np.full(n, -t), 4: np.full(n, -dn), 5: np.full(n, -up),
        6: np.full(n, np.float32(0.0)), 7: np.full(n, np.float32(-0.0)),
    }
    far = f32(rng.standard_normal(n) * 4 * thr)
    near = f32(rng.uniform(-1.5, 1.5, n) * thr)
    out = np.where(kind >= 10, near, far).astype(np.float32)
    for k, v in table.items():
        out = np.where(kind == k, v, out)
    return out.astype(np.float32), kind


def twobit_oracle(residual, grad, thr):
    """One call of the 2-bit quantiser in numpy: (words int32, residual)."""
    t = np.float32(thr)
    r = (f32(residual) + f32(grad)).astype(np.float32)
    pos, neg = r >= t, r <= -t
    codes = np.zeros(r.size, dtype=np.uint64)
    codes[pos], codes[neg] = 3, 2
    r = np.where(pos, r - t, np.where(neg, r + t, r)).astype(np.float32)
    nw = (r.size + 15) // 16
    padded = np.zeros(nw * 16, dtype=np.uint64)
    padded[:r.size] = codes
    shifts = (np.arange(16, dtype=np.uint64) * 2)
    words = (padded.reshape(nw, 16) << shifts).sum(axis=1)
    return words.astype(np.uint32).view(np.int32), r


def twobit_case(n, thr, seed=0, steps=3):
    """(residual0, [grad_1..grad_steps], [sum_1..]) where sum_k is the fp32
    value of residual + grad in call k. Call 1 hits its targets exactly:
    grad is taken in [target/2, 2*target], so residual0 = target - grad is
    exact (Sterbenz) and non-zero. Later calls use grad = fl(target -
    residual), which hits the target wherever that subtraction is exact."""
    rng = np.random.default_rng(1000 * seed + n % 9973 + int(thr * 100))
    tgt, _ = _twobit_targets(n, thr, rng)
    g1 = (tgt * f32(rng.uniform(0.5, 2.0, n))).astype(np.float32)
    zero = tgt == 0
    g1 = np.where(zero & ~np.signbit(tgt),
                  f32(rng.uniform(0.25, 1.0, n)), g1).astype(np.float32)
    r0 = (tgt - g1).astype(np.float32)
    r0 = np.where(zero & np.signbit(tgt), np.float32(-0.0), r0)
    g1 = np.where(zero & np.signbit(tgt), np.float32(-0.0), g1)
    r0, g1 = f32(r0), f32(g1)
    grads, sums, r = [g1], [(r0 + g1).astype(np.float32)], r0
    for _ in range(steps - 1):
        _, r = twobit_oracle(r, grads[-1], thr)
        tgt, _ = _twobit_targets(n, thr, rng)
        g = (tgt - r).astype(np.float32)
        grads.append(g)
        sums.append((r + g).astype(np.float32))
    return r0, grads, sums


def twobit_dequant_oracle(words, n, thr):
    w = np.asarray(words).view(np.uint32).astype(np.uint64)
    codes = ((w[:, None] >> (np.arange(16, dtype=np.uint64) * 2)) & 3)
    codes = codes.reshape(-1)[:n]
    t = np.float32(thr)
    out = np.zeros(n, dtype=np.float32)
    out[codes == 3] = t
    out[codes == 2] = -t
    return out


# n % 4 = 0..3, n % 16 != 0; the last is one float4 per thread of the
# whole 2048 x 256 grid plus a scalar tail
TWOBIT_DEQUANT_SIZES = [1, 2, 3, 5, 17, 18, 19, 1021, 1022, 1023, 4100,
                        524288 * 4 + 6]


def twobit_dequant_case(n, seed=0, extra_words=3):
    rng = np.random.default_rng(seed + n)
    nw = (n + 15) // 16 + extra_words
    return rng.integers(-2 ** 31, 2 ** 31, nw, dtype=np.int64) \
        .astype(np.int32)


# ---------------------------------------------------------------------------
# Bi-Sparse
# ---------------------------------------------------------------------------

BSC_MU = ref.BSC_MOMENTUM
# each side of 1024 / 2048 (one iteration of pack / fused), of 16384 (one
# block or two); 16385 gives the fused kernel two blocks of 8200: block
# 0 ends in a partial 2048-span, block 1 is 15 short of a full chunk
BSC_SIZES = [1, 5, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385,
             40003]
BSC_BIG_N = 16384 * 1024 - 5    # 1024 blocks: the whole lookback chain


def bsc_chain_case(n, seed=0, steps=4):
    """(u0, v0, [g_1..g_steps]) with non-zero state, so u*mu is inexact."""
    gen = torch.Generator().manual_seed(7919 * seed + n)
    u0 = torch.randn(n, generator=gen)
    v0 = torch.randn(n, generator=gen)
    gs = [torch.randn(n, generator=gen) * (1 + s) for s in range(steps)]
    return u0, v0, gs


def ratio_for(n, capacity):
    """A ratio with ref.bsc_capacity(n, ratio) == capacity."""
    r = (capacity + 0.5) / n
    assert ref.bsc_capacity(n, r) == capacity
    return r


def fma_f32(a, b, c):
    """Correctly rounded fp32 fused multiply-add of three fp32 scalars."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    # a*b is exact in float64; the sum may round, so settle it exactly:
    # take the float64-rounded candidate and its two fp32 neighbours
    cand = np.float32(float(a) * float(b) + float(c))
    best = None
    for x in (np.nextafter(cand, np.float32(-np.inf)), cand,
              np.nextafter(cand, np.float32(np.inf))):
        d = abs(Fraction(float(x)) - exact)
        if best is None or d < best[0]:
            best = (d, x)
    return np.float32(best[1])


FLIP_N, FLIP_RATIO = 40000, 0.01


def bsc_flip_case():
    """The boundary-flip instance: n = 40000, ratio 0.01 (sample 1000,
    top-k 10, capacity 400). Nine sampled positions carry g = 50; a tenth
    sampled position carries (u, g, v = 0) with
        fma(u, mu, g)  <  fl(fl(u*mu) + g),
    everything else is 0.1*randn. The reference's boundary is that tenth
    element's |v|; a kernel that contracts u*mu + g computes a |v| one ulp
    below its own boundary there and sends 9 elements instead of 10.
    Returns dict(g, u, v, pos9, flip, sep, fma)."""
    n = FLIP_N
    gen = torch.Generator().manual_seed(20240)
    g = 0.1 * torch.randn(n, generator=gen)
    u = 0.1 * torch.randn(n, generator=gen)
    v = 0.1 * torch.randn(n, generator=gen)
    ss = min(ref.bsc_sample_size(n, FLIP_RATIO), n)
    si = ref.bsc_sample_indices(n, ss, 42)
    once = (torch.bincount(si, minlength=n) == 1).nonzero().reshape(-1)
    pos = once[:10]
    pos9, flip = pos[:9], int(pos[9])
    g[pos9] = 50.0
    mu = np.float32(BSC_MU)
    rng = np.random.default_rng(5)
    while True:
        uu = np.float32(rng.uniform(1.0, 5.0))
        gg = np.float32(10.5 - 0.9 * float(uu) + rng.uniform(-0.05, 0.05))
        sep = np.float32(np.float32(uu * mu) + gg)
        fused = fma_f32(uu, mu, gg)
        if fused < sep:
            break
    u[flip], g[flip], v[flip] = float(uu), float(gg), 0.0
    return dict(g=g, u=u, v=v, pos9=pos9, flip=flip, sep=float(sep),
                fma=float(fused))


BSC_TIE_BOUNDARY = 1.25


def bsc_tie_case(n=5000, seed=3):
    """(g, u0, v0, at, below): post-momentum v is exactly +/-boundary at
    `at` (sent) and nextafter(boundary, 0) at `below` (kept); u0 = v0 = 0
    at those positions so v == g there, randn state elsewhere, scaled so
    that a fair share of the rest is selected too."""
    gen = torch.Generator().manual_seed(seed)
    g = 0.6 * torch.randn(n, generator=gen)
    u0 = 0.3 * torch.randn(n, generator=gen)
    v0 = 0.3 * torch.randn(n, generator=gen)
    perm = torch.randperm(n, generator=gen)
    at, below = perm[:64], perm[64:128]
    b = np.float32(BSC_TIE_BOUNDARY)
    dn = float(np.nextafter(b, np.float32(0)))
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    u0[perm[:128]] = 0.0
    v0[perm[:128]] = 0.0
    g[at] = sign * float(b)
    g[below] = sign * dn
    return g, u0, v0, at, below


def bsc_pull_case(n=40003, seed=4):
    """Dense-ish x whose FIRST block holds subnormals, -0.0 and +0.0: a
    count/pack disagreement on any of them would shift every later block."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen)
    x[torch.rand(n, generator=gen) < 0.5] = 0.0
    sub = float(np.float32(2.0 ** -149))
    big_sub = float(np.float32(2.0 ** -127))
    x[0:12] = torch.tensor([sub, -sub, 0.0, -0.0, big_sub, -big_sub, 1.0,
                            -0.0, sub, 0.0, -sub, -0.0])
    x[1021:1027] = torch.tensor([sub, -0.0, -sub, 0.0, big_sub, -0.0])
    return x


def bsc_unpack_oracle(vals, idx, out, accumulate):
    """ref.bsc_decompress on the entries with 0 <= idx < out.numel()."""
    n = out.numel()
    keep = (idx >= 0) & (idx < n)
    return ref.bsc_decompress(vals[keep], idx[keep], n, out=out,
                              accumulate=accumulate)


# ---------------------------------------------------------------------------
# DGT contribution
# ---------------------------------------------------------------------------

# (n, chunk): chunks 4, 63, 64, 1000, 1023, 1024; a last chunk of one
# element; n < chunk; more chunks than the 2048-block grid
DGT_CASES = [(4, 4), (9, 4), (63, 63), (63 * 5 + 1, 63), (64, 64),
             (64 * 3 + 1, 64), (1000 * 3 + 1, 1000), (999, 1000),
             (1023 * 4 + 1, 1023), (1022, 1023), (1024 * 3 + 1, 1024),
             (1024 * 2 + 1023, 1024), (17, 1024), (1, 64),
             (2049 * 64, 64), (2049 * 64 + 1, 64), (4100 * 4 + 3, 4)]


def dgt_int_case(n, seed=0):
    rng = np.random.default_rng(seed + n)
    return rng.integers(-3, 4, n).astype(np.float32)


def dgt_oracle(g, chunk):
    """float64 mean(|g|) per chunk, rounded to fp32 once."""
    a = np.abs(f64(g))
    nch = (a.size + chunk - 1) // chunk
    out = np.empty(nch, dtype=np.float64)
    for c in range(nch):
        sl = a[c * chunk:(c + 1) * chunk]
        out[c] = sl.sum() / sl.size
    return out


def dgt_depth(chunk):
    """Roundings on the longest path of k_dgt_contribution for one chunk:
    per 1024 elements a thread adds a 4-term sum (3 adds) to its partial
    (1 add); the scalar tail adds at most ceil(1023/256) = 4 more; then 6
    shuffle levels, 4 wave partials, one divide."""
    return 4 * ((chunk + 1023) // 1024) + 4 + 6 + 4 + 1


def dgt_bound(g, chunk):
    """|kernel - oracle| <= gamma_D * mean|g| per chunk (all terms are
    non-negative, so the classical summation bound applies), + the final
    rounding of the oracle itself."""
    d = dgt_depth(chunk)
    gamma = d * U32 / (1 - d * U32)
    return MARGIN * gamma * dgt_oracle(g, chunk) + F32_TINY


# ---------------------------------------------------------------------------
# 4-bit
# ---------------------------------------------------------------------------

# (n, chunk); n % 4 in 1..3 puts the scalar tail inside a ragged last chunk
Q4_CASES = [(4, 4), (8, 4), (11, 4), (8, 8), (29, 8), (64, 64), (64 * 3 + 2,
            64), (1024 * 2, 1024), (1024 * 2 + 515, 1024), (2049 * 4 - 1, 4),
            (2049 * 4 + 4 * 37, 4)]
Q4_CLAMP = float(np.float32(1e-30))


def q4_oracle(f, chunk):
    """float64 model of quantize_4bit on f = x + residual (already summed,
    fp32-representable). Returns minmax[nch,2], codes, deq, residual, all
    float64 / int; packed bytes via q4_pack."""
    f = f64(f)
    n = f.size
    nch = (n + chunk - 1) // chunk
    mm = np.empty((nch, 2))
    codes = np.empty(n, dtype=np.int64)
    deq = np.empty(n)
    for c in range(nch):
        sl = slice(c * chunk, min((c + 1) * chunk, n))
        lo, hi = f[sl].min(), f[sl].max()
        step = max(hi - lo, Q4_CLAMP) / 16.0
        cd = np.clip(np.floor((f[sl] - lo) / step), 0, 15).astype(np.int64)
        mm[c] = lo, hi
        codes[sl] = cd
        deq[sl] = lo + (cd + 0.5) * step
    return mm, codes, deq, f - deq


def q4_pack(codes):
    c = np.asarray(codes, dtype=np.uint8)
    if c.size % 2:
        c = np.concatenate([c, np.zeros(1, dtype=np.uint8)])
    return (c[0::2] | (c[1::2] << 4)).astype(np.uint8)


def q4_unpack(packed, n):
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack([p & 15, p >> 4], axis=1).reshape(-1)[:n].astype(np.int64)


def q4_grid_chain(n, chunk, seed=0, steps=3):
    """[(x_t, f_t)] for a 3-step residual chain on an exact grid. Per
    chunk: an integer lo in [-8, 8], k in [-2, 3], span 16*2^k, so step =
    2^k; the elements are lo + j*step/4, j in 0..64: every bin edge (j %
    4 == 0), interior points, and x == max (j = 64, code 15). j = 0 and
    j = 64 are always present when the chunk has two elements or more;
    every fifth chunk is constant (the 1e-30 clamp). x_t = f_t -
    residual_{t-1} is exact, and so is every fp32 operation of the kernel."""
    rng = np.random.default_rng(31 * seed + n + chunk)
    nch = (n + chunk - 1) // chunk
    res = np.zeros(n)
    # non-zero starting residual on the grid of the first step
    out = []
    lo_c = rng.integers(-8, 9, nch).astype(np.float64)
    k_c = rng.integers(-2, 4, nch)
    for t in range(steps):
        f = np.empty(n)
        for c in range(nch):
            sl = slice(c * chunk, min((c + 1) * chunk, n))
            m = sl.stop - sl.start
            step = 2.0 ** k_c[c]
            if c % 5 == 4 or m == 1:
                j = np.zeros(m)
                lo = lo_c[c] if lo_c[c] != 0 else 3.0
            else:
                lo = lo_c[c]
                j = rng.integers(0, 65, m).astype(np.float64)
                j[rng.integers(0, m)] = 64      # hi present: code 15 clamp
                where0 = rng.integers(0, m)
                if j[where0] == 64 and (j == 64).sum() == 1:
                    where0 = (where0 + 1) % m
                j[where0] = 0                   # lo present
            f[sl] = lo + j * step / 4
        if t == 0:
            # start from a non-zero residual: a quarter step either way
            r0 = np.empty(n)
            for c in range(nch):
                sl = slice(c * chunk, min((c + 1) * chunk, n))
                r0[sl] = (2.0 ** k_c[c]) / 4 * rng.integers(-1, 2,
                                                             sl.stop - sl.start)
            res = r0
        x = f - res
        assert np.array_equal(f32(x).astype(np.float64), x)
        assert np.array_equal((f32(x) + f32(res)).astype(np.float64), f)
        out.append((f32(x), f32(res), f32(f)))
        _, _, _, res = q4_oracle(f, chunk)
    return out


Q4_ULPS = 8.0


def q4_randn_bound(mm, n, chunk):
    """Per element: step/2 + Q4_ULPS * 2^-24 * (|lo| + |hi|).
    code = floor((f - lo) * inv): f - lo, hi - lo, 1/step and the product
    round once each, so the bin index is off by at most 16*4u bins, i.e.
    the code may be the neighbour's when f is within 4u*span of an edge;
    deq = lo + (code + .5)*step carries step's rounding (hi - lo), the
    product's and the sum's: 2u*span + u*max(|lo|, |hi|). With span <=
    |lo| + |hi| that is 7u(|lo| + |hi|); 8 is used."""
    mm = f64(mm)
    step = np.maximum(mm[:, 1] - mm[:, 0], Q4_CLAMP) / 16.0
    b = step / 2 + Q4_ULPS * U32 * (np.abs(mm[:, 0]) + np.abs(mm[:, 1]))
    return np.repeat(b, chunk)[:n], np.repeat(step, chunk)[:n]


# ---------------------------------------------------------------------------
# Optimizers: float64 oracle with a running error bound
# ---------------------------------------------------------------------------

class Err:
    """A float64 value with a first-order bound on the error an fp32
    evaluation of the same expression can have. Inputs are exact."""

    def __init__(self, val, err=None):
        self.v = f64(val)
        self.e = np.zeros_like(self.v) if err is None else f64(err)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Err) else Err(np.float64(x))

    def _rounded(self, v, e):
        return Err(v, e + U32 * np.abs(v))

    def __mul__(self, o):
        o = Err.lift(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e +
                             np.abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __add__(self, o):
        o = Err.lift(o)
        return self._rounded(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = Err.lift(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return Err(-self.v, self.e)

    def __truediv__(self, o):
        o = Err.lift(o)
        q = self.v / o.v
        den = np.maximum(np.abs(o.v) - o.e, F32_TINY)
        return self._rounded(q, (self.e + np.abs(q) * o.e) / den)

    def sqrt(self):
        hi = np.sqrt(self.v + self.e)
        lo = np.sqrt(np.maximum(self.v - self.e, 0.0))
        return self._rounded(np.sqrt(self.v), hi - lo)

    def bound(self):
        return MARGIN * self.e + F32_TINY


def _gg(w, g, wd, rs):
    return g * p32(rs) + p32(wd) * w


def _sign(pre, w, lr):
    s = np.sign(pre.v)
    return Err(w.v - p32(lr) * s, U32 * np.abs(w.v - p32(lr) * s))


def opt_oracle(name, st, g, hp):
    """One step. st: dict of fp32 arrays (w and the states), g: fp32, hp:
    dict of Python floats. Returns {name: Err} of the new w and states,
    plus 'pre' (the pre-sign value) for the sign optimizers."""
    w, g = Err(st["w"]), Err(g)
    lr, wd, rs = hp["lr"], hp["wd"], hp["rescale"]
    if name == "sgd":
        return {"w": w - p32(lr) * _gg(w, g, wd, rs)}
    if name == "sgd_mom":
        mom = Err(st["mom"]) * p32(hp["momentum"]) - \
            p32(lr) * _gg(w, g, wd, rs)
        return {"mom": mom, "w": w + mom}
    if name == "adam":
        b1, b2 = p32(hp["beta1"]), p32(hp["beta2"])
        lr_t = p32(lr * np.sqrt(1.0 - hp["beta2"] ** hp["t"]) /
                   (1.0 - hp["beta1"] ** hp["t"]))
        gg = _gg(w, g, wd, rs)
        # 1 - beta is formed in fp32 by the kernel; exact for fp32 betas
        m = b1 * Err(st["m"]) + (1.0 - b1) * gg
        v = b2 * Err(st["v"]) + (1.0 - b2) * gg * gg
        return {"m": m, "v": v,
                "w": w - lr_t * m / (v.sqrt() + p32(hp["eps"]))}
    if name == "rmsprop":
        rho = p32(hp["rho"])
        gg = _gg(w, g, wd, rs)
        n = rho * Err(st["n"]) + (1.0 - rho) * gg * gg
        return {"n": n, "w": w - p32(lr) * gg / (n.sqrt() + p32(hp["eps"]))}
    if name == "adagrad":
        gg = _gg(w, g, wd, rs)
        h = Err(st["h"]) + gg * gg
        return {"h": h, "w": w - p32(lr) * gg / (h.sqrt() + p32(hp["eps"]))}
    if name == "signsgd":
        pre = _gg(w, g, wd, rs)
        return {"pre": pre, "w": _sign(pre, w, lr)}
    if name == "signum":
        mu = p32(hp["momentum"])
        mom = mu * Err(st["mom"]) + (1.0 - mu) * _gg(w, g, wd, rs)
        return {"pre": mom, "mom": mom, "w": _sign(mom, w, lr)}
    if name in ("dcasgd", "dcasgd_mom", "dcasgd_mom0"):
        gs = g * p32(rs)
        upd = -(p32(lr) * (gs + p32(wd) * w + p32(hp["lamda"]) * gs * gs *
                           (w - Err(st["prev_w"]))))
        out = {"prev_w": Err(st["w"])}
        if name == "dcasgd_mom":
            upd = Err(st["mom"]) * p32(hp["momentum"]) + upd
            out["mom"] = upd
        elif name == "dcasgd_mom0":
            out["mom"] = Err(st["mom"])     # given but momentum == 0
        out["w"] = w + upd
        return out
    raise KeyError(name)


# betas / rho / momentum of the optimizers that form 1 - x are dyadic: the
# kernel computes 1.0f - (float)x, the fp32 reference (float)(1.0 - x); for
# x = 0.9 these differ by 2.2e-7 relative, a parameter difference, not a
# rounding of the update (docs/testing.md)
OPT_HP = {
    "sgd": dict(lr=0.1, wd=1e-2, rescale=0.37),
    "sgd_mom": dict(lr=0.1, momentum=0.9, wd=1e-2, rescale=0.37),
    "adam": dict(lr=0.01, beta1=0.875, beta2=1 - 2.0 ** -9, eps=1e-8,
                 wd=1e-2, rescale=0.37),
    "rmsprop": dict(lr=0.01, rho=0.875, eps=1e-8, wd=1e-2, rescale=0.37),
    "adagrad": dict(lr=0.1, eps=1e-7, wd=1e-2, rescale=0.37),
    "signsgd": dict(lr=0.01, wd=1e-2, rescale=0.37),
    "signum": dict(lr=0.01, momentum=0.875, wd=1e-2, rescale=0.37),
    "dcasgd": dict(lr=0.01, lamda=0.04, momentum=0.0, wd=1e-2,
                   rescale=0.37),
    "dcasgd_mom": dict(lr=0.01, lamda=0.04, momentum=0.9, wd=1e-2,
                       rescale=0.37),
    "dcasgd_mom0": dict(lr=0.01, lamda=0.04, momentum=0.0, wd=1e-2,
                        rescale=0.37),
}
OPT_STATES = {
    "sgd": [], "sgd_mom": ["mom"], "adam": ["m", "v"], "rmsprop": ["n"],
    "adagrad": ["h"], "signsgd": [], "signum": ["mom"],
    "dcasgd": ["prev_w"], "dcasgd_mom": ["prev_w", "mom"],
    "dcasgd_mom0": ["prev_w", "mom"],
}
OPT_FLOAT4 = ("sgd", "sgd_mom", "adam", "rmsprop")
OPT_BIG_FLOAT4 = 2048 * 256 * 4 + 7
OPT_BIG_SCALAR = 2048 * 256 + 1
SIGN_EXCLUDED_CAP = 1e-3


def opt_sizes(name):
    return LADDER + [OPT_BIG_FLOAT4 if name in OPT_FLOAT4
                     else OPT_BIG_SCALAR]


def opt_case(name, n, seed=0, steps=3):
    """(state0 dict of fp32 arrays, [g_1..g_steps]). Second-moment states
    are non-negative. Every 16th element (from 0) has w = g = state = 0: the
    pre-sign value of the sign optimizers is exactly 0 there."""
    rng = np.random.default_rng(97 * seed + n + len(name))
    st = {"w": f32(rng.standard_normal(n))}
    for s in OPT_STATES[name]:
        x = rng.standard_normal(n)
        st[s] = f32(x * x * 0.1 if s in ("v", "n", "h") else x * 0.1)
    gs = [f32(rng.standard_normal(n)) for _ in range(steps)]
    for a in list(st.values()) + gs:
        a[0::16] = 0.0
    return st, gs


def opt_call(mod, name, st, g, hp):
    """Run one step through `mod` (geomx_amd.ops or its reference module);
    st and g are torch tensors, updated in place."""
    lr, wd, rs = hp["lr"], hp["wd"], hp["rescale"]
    w = st["w"]
    if name == "sgd":
        mod.sgd_update(w, g, lr, wd, rs)
    elif name == "sgd_mom":
        mod.sgd_mom_update(w, g, st["mom"], lr, hp["momentum"], wd, rs)
    elif name == "adam":
        mod.adam_update(w, g, st["m"], st["v"], hp["t"], lr, hp["beta1"],
                        hp["beta2"], hp["eps"], wd, rs)
    elif name == "rmsprop":
        mod.rmsprop_update(w, g, st["n"], lr, hp["rho"], hp["eps"], wd, rs)
    elif name == "adagrad":
        mod.adagrad_update(w, g, st["h"], lr, hp["eps"], wd, rs)
    elif name == "signsgd":
        mod.signsgd_update(w, g, lr, wd, rs)
    elif name == "signum":
        mod.signum_update(w, g, st["mom"], lr, hp["momentum"], wd, rs)
    else:
        mod.dcasgd_update(w, g, st["prev_w"], st.get("mom"), lr,
                          hp["lamda"], hp["momentum"], wd, rs)


def opt_check_step(name, before, after, g, hp):
    """Compare one step's fp32 result `after` with the float64 oracle run
    from the fp32 state `before`. Returns (worst error/bound ratio over all
    outputs, fraction of elements excluded from the sign comparison);
    raises AssertionError naming the output on a miss."""
    orc = opt_oracle(name, before, g, hp)
    worst, excluded = 0.0, 0.0
    keep = np.ones(g.size, dtype=bool)
    if "pre" in orc:
        pre = orc["pre"]
        keep = ~(np.abs(pre.v) < pre.bound())
        keep |= pre.e == 0          # an exact 0 is compared, never excluded
        excluded = 1.0 - keep.mean()
    for k, o in orc.items():
        if k == "pre":
            continue
        err = np.abs(f64(after[k]) - o.v)
        b = o.bound()
        sel = keep if k == "w" else np.ones_like(keep)
        if sel.any():
            ratio = float((err[sel] / b[sel]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, k, ratio, int(np.argmax(
                np.where(sel, err / b, 0))))
    return worst, excluded


# ---------------------------------------------------------------------------
# ReLU + 2x2 max pool
# ---------------------------------------------------------------------------

# (N, C, H, W): C = 8, 16, 24; H or W of 2; 2 x odd; the last has 528392
# input vectors, more than one 524288-vector grid-stride trip of the
# backward kernel
POOL_SHAPES = [(1, 8, 2, 2), (3, 8, 2, 6), (2, 16, 6, 2), (2, 24, 10, 14),
               (5, 16, 18, 22), (2, 8, 514, 514)]


def pool_case(shape, seed=0):
    """(x, grad_out) as NCHW-shaped bf16 tensors (callers make them
    channels_last): small integers in [-2, 2], so most windows tie."""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(seed + n * h * w + c)
    x = torch.randint(-2, 3, shape, generator=gen).to(torch.bfloat16)
    go = torch.randint(-3, 4, (n, c, h // 2, w // 2), generator=gen) \
        .to(torch.bfloat16)
    return x, go


def pool_oracle(x, go):
    """Explicit first-maximum oracle. Window order (0,0),(0,1),(1,0),(1,1);
    a later element wins only if strictly greater; code 255 and output 0
    where the maximum is <= 0. Returns (out NCHW f32, codes [N,Ho,Wo,C]
    uint8, grad_in NCHW f32)."""
    xf, gf = x.float(), go.float()
    q = [xf[:, :, 0::2, 0::2], xf[:, :, 0::2, 1::2],
         xf[:, :, 1::2, 0::2], xf[:, :, 1::2, 1::2]]
    m = q[0].clone()
    arg = torch.zeros_like(m, dtype=torch.int64)
    for k in (1, 2, 3):
        gt = q[k] > m
        m = torch.where(gt, q[k], m)
        arg = torch.where(gt, torch.full_like(arg, k), arg)
    dead = m <= 0
    out = torch.where(dead, torch.zeros_like(m), m)
    codes = torch.where(dead, torch.full_like(arg, 255), arg)
    gin = torch.zeros_like(xf)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gin[:, :, dy::2, dx::2] = torch.where(codes == k, gf,
                                              torch.zeros_like(gf))
    return out, codes.permute(0, 2, 3, 1).contiguous().to(torch.uint8), gin
