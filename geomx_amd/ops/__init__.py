"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (matches the project contract):
  - CUDA (ROCm) tensors MUST go through the native `_geops` extension;
    if the extension is missing on a GPU machine the op RAISES — there
    is no silent eager fallback on the GPU path.
  - CPU tensors use the pure-torch reference implementations
    (`geomx_amd.ops.reference`), which also serve as the golden model
    for the HIP kernels in tests.
"""

from __future__ import annotations


from typing import Optional, Tuple

import torch

from . import reference as ref

_geops = None
_geops_err: Optional[str] = None
try:
    from geomx_amd import _geops as _geops_mod  # built in-tree by setup.py
    _geops = _geops_mod
except Exception as e:  # pragma: no cover - exercised only when ext missing
    _geops_err = repr(e)


def native_available() -> bool:
    return _geops is not None


def native_error() -> Optional[str]:
    return _geops_err


def _require_native():
    if _geops is None:
        raise RuntimeError(
            "geomx_amd native extension (_geops) is required for GPU tensors "
            "but failed to import: %s. Build it with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950)."
            % _geops_err)
    return _geops


def _on_gpu(*tensors) -> bool:
    return any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))


def _flat_inplace(t: torch.Tensor, name: str) -> torch.Tensor:
    """1-d VIEW of an operand a kernel writes. `.reshape(-1)` of a
    non-contiguous tensor is a copy: the kernel would update the copy and
    the caller's tensor would silently stay as it was. Such a tensor is an
    error here, never a copy."""
    if not t.is_contiguous():
        raise ValueError(
            "%s is updated in place by the kernel and must be contiguous "
            "(shape %s, strides %s)" % (name, tuple(t.shape), t.stride()))
    return t.view(-1)


def zero_many_f32(ranges) -> None:
    """Clear contiguous fp32 tensors: on the GPU one launch of
    k_zero_many_f32 per 8 of them (finalize.hip), on the CPU zero_()."""
    ranges = [r for r in ranges if r.numel()]
    if not _on_gpu(*ranges):
        for r in ranges:
            r.zero_()
        return
    lib = _require_native()
    for i in range(0, len(ranges), 8):
        lib.zero_many_f32(ranges[i:i + 8])


# ---------------------------------------------------------------------------
# 2bit
# ---------------------------------------------------------------------------

def quantize_2bit(grad: torch.Tensor, residual: torch.Tensor, threshold: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n = grad.numel()
    nw = ref.quantized_words(n)
    if _on_gpu(grad):
        g = _require_native()
        if out is None:
            out = torch.empty(nw, dtype=torch.int32, device=grad.device)
        g.quantize_2bit(grad.reshape(-1), _flat_inplace(residual, "residual"),
                        _flat_inplace(out, "out"), threshold)
        return out
    packed = ref.quantize_2bit(grad, residual, threshold)
    if out is not None:
        out.copy_(packed)
        return out
    return packed


def dequantize_2bit(packed: torch.Tensor, n: int, threshold: float,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _on_gpu(packed):
        g = _require_native()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=packed.device)
        g.dequantize_2bit(packed, _flat_inplace(out, "out"), threshold)
        return out
    return ref.dequantize_2bit(packed, n, threshold, out=out)


# ---------------------------------------------------------------------------
# Bi-Sparse
# ---------------------------------------------------------------------------

def bsc_compress(grad, u, v, ratio, momentum=ref.BSC_MOMENTUM, seed=42
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(grad):
        g = _require_native()
        n = grad.numel()
        k = ref.bsc_capacity(n, ratio)
        vals = torch.empty(k, dtype=torch.float32, device=grad.device)
        idx = torch.empty(k, dtype=torch.int32, device=grad.device)
        gflat = grad.reshape(-1)
        u, v = _flat_inplace(u, "u"), _flat_inplace(v, "v")
        # boundary PREDICTED from the seeded sample of post-momentum v
        # (v + mu*u + g at the sample positions, read BEFORE the fused
        # kernel mutates them) as a DEVICE scalar, so the fused kernel
        # path never synchronizes with the host
        bt = bsc_boundary(v, ratio, seed, g=gflat, u=u, momentum=momentum)
        if g.bsc_compress_fused(gflat, u, v, vals, idx, bt, momentum,
                                ref.BSC_PLACEHOLDER):
            return vals, idx
        # huge-n fallback: momentum + count + scan + pack chain
        g.bsc_momentum(gflat, u, v, momentum)
        boundary = _bsc_boundary_gpu(v, ratio, seed)
        g.bsc_pack(v, u, vals, idx, boundary, ref.BSC_PLACEHOLDER)
        return vals, idx
    return ref.bsc_compress(grad, u, v, ratio, momentum, seed)


_bsc_idx_cache: dict = {}


def _bsc_sample_idx(n: int, sample_size: int, seed: int, device,
                    dtype=torch.int64):
    """Seeded sample positions on `device`, generated once per (n,
    sample_size, seed) on the CPU generator. int32 is what k_bsc_boundary
    reads, int64 what the ATen expression indexes with."""
    ck = (n, sample_size, seed, device, dtype)
    idx = _bsc_idx_cache.get(ck)
    if idx is None:
        if len(_bsc_idx_cache) > 64:
            _bsc_idx_cache.clear()
        idx = ref.bsc_sample_indices(n, sample_size, seed).to(
            device=device, dtype=dtype)
        _bsc_idx_cache[ck] = idx
    return idx


# samples the one-workgroup form of k_bsc_boundary holds (None without the
# extension)
BSC_BOUNDARY_CAP = getattr(_geops, "BSC_BOUNDARY_CAP", None)


def _bsc_boundary_served(n: int, sample_size: int, *operands) -> bool:
    """What k_bsc_boundary serves: contiguous fp32 GPU operands, n < 2^31
    and at least one sample. The kernel beats the ATen chain at every
    sample size measured (docs/kernels.md), so no size range is held back."""
    return (n < 2 ** 31 and sample_size >= 1
            and all(t.is_cuda and t.dtype == torch.float32
                    and t.is_contiguous() for t in operands))


def bsc_boundary(v: torch.Tensor, ratio: float, seed: int = 42,
                 g: Optional[torch.Tensor] = None,
                 u: Optional[torch.Tensor] = None,
                 momentum: float = ref.BSC_MOMENTUM) -> torch.Tensor:
    """Sampled top-k boundary of Bi-Sparse as a one-element fp32 tensor: the
    k-th largest |v| over the seeded sample of ref.bsc_boundary, or, with
    `g` and `u`, of the POST-momentum |v + (momentum*u + g)| computed from
    (g, u, v) as they are before the momentum pass (same op order as the
    golden model, so the same bits). On the GPU one select kernel writes it
    into storage of its own (k_bsc_fused reads it with a uniform scalar
    load) and the host never waits; operands the kernel does not serve, and
    CPU tensors, take the ATen expression."""
    if (g is None) != (u is None):
        raise ValueError("bsc_boundary takes g and u together or neither")
    mom = g is not None
    n = v.numel()
    sample_size = min(ref.bsc_sample_size(n, ratio), n)
    k = min(max(1, int(sample_size * ratio)), sample_size)
    operands = (v, g, u) if mom else (v,)
    if _on_gpu(*operands) and _bsc_boundary_served(n, sample_size, *operands):
        si = _bsc_sample_idx(n, sample_size, seed, v.device, torch.int32)
        out = torch.empty(1, dtype=torch.float32, device=v.device)
        # contiguous: these are views. Empty tensors for the |v| form
        gu = (g.reshape(-1), u.reshape(-1)) if mom \
            else (torch.Tensor(), torch.Tensor())
        _require_native().bsc_boundary(v.reshape(-1), *gu, si, k, momentum,
                                       out, 0)
        return out
    si = _bsc_sample_idx(n, sample_size, seed, v.device)
    flat = v.reshape(-1)
    if mom:
        sample = (flat[si] + (u.reshape(-1)[si] * momentum
                              + g.reshape(-1)[si])).abs()
    else:
        sample = flat[si].abs()
    # clone: a slice view is 4B-aligned at best; the fused kernel's
    # uniform scalar load wants its own 16B-aligned storage
    return torch.topk(sample, k).values[k - 1:k].clone()


def _bsc_boundary_gpu(v: torch.Tensor, ratio: float, seed: int) -> float:
    """Boundary of the huge-n fallback route as a host float: the same
    seeded-sample estimator as the CPU golden model (ref.bsc_boundary) over
    the post-momentum |v|. That route synchronizes anyway, for bsc_pack's
    float argument."""
    return bsc_boundary(v, ratio, seed).item()


def bsc_pull_compress(x: torch.Tensor, capacity: int
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(x):
        g = _require_native()
        vals = torch.empty(capacity, dtype=torch.float32, device=x.device)
        idx = torch.empty(capacity, dtype=torch.int32, device=x.device)
        g.bsc_pull_pack(x.reshape(-1), vals, idx, ref.BSC_PLACEHOLDER)
        return vals, idx
    return ref.bsc_pull_compress(x, capacity)


def bsc_decompress(vals, idx, n, out=None, accumulate=False) -> torch.Tensor:
    if _on_gpu(vals):
        g = _require_native()
        if out is None:
            out = torch.zeros(n, dtype=torch.float32, device=vals.device)
            g.bsc_unpack(vals, idx, out, True)
            return out
        g.bsc_unpack(vals, idx, _flat_inplace(out, "out"), accumulate)
        return out
    return ref.bsc_decompress(vals, idx, n, out=out, accumulate=accumulate)


# ---------------------------------------------------------------------------
# DGT
# ---------------------------------------------------------------------------

def dgt_contribution(grad: torch.Tensor, chunk_elems: int) -> torch.Tensor:
    if _on_gpu(grad):
        g = _require_native()
        n = grad.numel()
        nchunks = (n + chunk_elems - 1) // chunk_elems
        out = torch.empty(nchunks, dtype=torch.float32, device=grad.device)
        g.dgt_contribution(grad.reshape(-1), out, chunk_elems)
        return out
    return ref.dgt_contribution(grad, chunk_elems)


def quantize_4bit_chunked(x: torch.Tensor, chunk_elems: int,
                          residual: Optional[torch.Tensor] = None):
    """Per-chunk min/max 4-bit quantization. Returns (packed u8, minmax f32[nchunks,2])."""
    n = x.numel()
    nchunks = (n + chunk_elems - 1) // chunk_elems
    if _on_gpu(x):
        g = _require_native()
        packed = torch.empty((n + 1) // 2, dtype=torch.uint8, device=x.device)
        minmax = torch.empty((nchunks, 2), dtype=torch.float32, device=x.device)
        res = _flat_inplace(residual, "residual") \
            if residual is not None else torch.Tensor()
        g.quantize_4bit(x.reshape(-1), res, packed, minmax, chunk_elems)
        return packed, minmax
    packs, mins, maxs = [], [], []
    f = x.reshape(-1)
    for c in range(nchunks):
        sl = f[c * chunk_elems:(c + 1) * chunk_elems]
        rsl = residual.reshape(-1)[c * chunk_elems:(c + 1) * chunk_elems] \
            if residual is not None else None
        p, lo, hi = ref.quantize_4bit(sl, rsl)
        packs.append(p)
        mins.append(lo)
        maxs.append(hi)
    minmax = torch.tensor([[lo, hi] for lo, hi in zip(mins, maxs)],
                          dtype=torch.float32)
    return torch.cat(packs), minmax


def dequantize_4bit_chunked(packed: torch.Tensor, minmax: torch.Tensor,
                            n: int, chunk_elems: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    nchunks = minmax.shape[0]
    if _on_gpu(packed):
        g = _require_native()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=packed.device)
        g.dequantize_4bit(packed, minmax, _flat_inplace(out, "out"),
                          chunk_elems)
        return out
    res = []
    # CPU reference packs each chunk independently (chunk_elems even except last)
    half = (chunk_elems + 1) // 2
    for c in range(nchunks):
        lo, hi = minmax[c, 0].item(), minmax[c, 1].item()
        m = min(chunk_elems, n - c * chunk_elems)
        res.append(ref.dequantize_4bit(packed[c * half:c * half + (m + 1) // 2],
                                       m, lo, hi))
    full = torch.cat(res)
    if out is not None:
        out.reshape(-1).copy_(full)
        return out
    return full


def _dgt_encode_served(x: torch.Tensor, residual: torch.Tensor,
                       chunk_elems: int) -> bool:
    """What k_dgt_encode serves: a power-of-two chunk in [64, 8192] and
    contiguous fp32 operands on 16 B boundaries."""
    return (64 <= chunk_elems <= 8192
            and chunk_elems & (chunk_elems - 1) == 0
            and x.numel() > 0
            and all(t.dtype == torch.float32 and t.is_contiguous()
                    and t.data_ptr() % 16 == 0 for t in (x, residual)))


def dgt_encode(x: torch.Tensor, residual: torch.Tensor, contrib: torch.Tensor,
               keep_idx: torch.Tensor, chunk_elems: int):
    """DGT mode-3 wire payload of a bucket: (exact, keep_idx i32, packed,
    minmax), the tuple of DGTState.compress. `residual` is updated in
    place; `contrib` is the per-chunk EWMA (0 marks a dead chunk) and
    `keep_idx` the sorted indices of the chunks that travel exact. On the
    GPU one kernel writes the whole payload; a chunk size or operand
    outside what it serves, and CPU tensors, take the op sequence of
    ref.dgt_encode, whose bits the kernel reproduces."""
    flat = x.reshape(-1)
    if _on_gpu(flat, residual) \
            and _dgt_encode_served(flat, residual, chunk_elems):
        g = _require_native()
        res = _flat_inplace(residual, "residual")
        numel = flat.numel()
        nchunks = (numel + chunk_elems - 1) // chunk_elems
        keep32 = keep_idx.to(torch.int32).contiguous()
        n_keep = keep32.numel()
        n_lossy = nchunks - n_keep
        dev = flat.device
        exact = torch.empty(n_keep * chunk_elems, device=dev)
        packed = torch.empty(n_lossy * (chunk_elems // 2), dtype=torch.uint8,
                             device=dev)
        minmax = torch.empty((n_lossy, 2), device=dev)
        g.dgt_encode(flat, res, contrib.float().contiguous(), keep32, exact,
                     packed, minmax.view(-1), chunk_elems)
        return exact, keep32, packed, minmax
    return ref.dgt_encode(x, residual, contrib, keep_idx, chunk_elems)


# ---------------------------------------------------------------------------
# Wire reduce: decode every party's payload and sum them in one kernel.
#   out = (out if accumulate else +0) + c_0 + c_1 + ... + c_{P-1}
# fp32, folded in list order: bit-equal to `acc = zeros; acc += decode(p)`.
# ---------------------------------------------------------------------------

def wire_sum_2bit(payloads, n: int, threshold: float,
                  out: Optional[torch.Tensor] = None,
                  accumulate: bool = False) -> torch.Tensor:
    """Sum of the 2bit payloads (packed int32 words) of all parties."""
    if _on_gpu(out, *payloads):
        g = _require_native()
        if out is None:
            out = torch.empty(n, dtype=torch.float32,
                              device=payloads[0].device)
            accumulate = False
        g.wire_sum_2bit(list(payloads), _flat_inplace(out, "out"), threshold,
                        accumulate)
        return out
    return ref.wire_sum_2bit(payloads, n, threshold, out, accumulate)


def wire_sum_fp16(payloads, out: Optional[torch.Tensor] = None,
                  accumulate: bool = False) -> torch.Tensor:
    """Sum of the fp16 wire tensors of all parties, in fp32."""
    if _on_gpu(out, *payloads):
        g = _require_native()
        if out is None:
            out = torch.empty(payloads[0].numel(), dtype=torch.float32,
                              device=payloads[0].device)
            accumulate = False
        g.wire_sum_f16([p.reshape(-1) for p in payloads],
                       _flat_inplace(out, "out"), accumulate)
        return out
    return ref.wire_sum_fp16(payloads, out, accumulate)


def wire_sum_dgt(payloads, numel: int, chunk_elems: int,
                 out: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """Sum of the DGT mode-3 payloads of all parties. Each payload is the
    tuple of DGTState.compress: (exact, keep_idx, packed, minmax)."""
    if _on_gpu(out, *(t for p in payloads for t in p)):
        g = _require_native()
        if out is None:
            out = torch.empty(numel, dtype=torch.float32,
                              device=payloads[0][0].device)
            accumulate = False
        exacts, keeps, packeds, minmaxs = (list(x) for x in zip(*payloads))
        g.wire_sum_dgt(exacts, keeps, packeds,
                       [m.reshape(-1) for m in minmaxs],
                       _flat_inplace(out, "out"), chunk_elems, accumulate)
        return out
    return ref.wire_sum_dgt(payloads, numel, chunk_elems, out, accumulate)


# ---------------------------------------------------------------------------
# FP8 wire tier: block-scaled E4M3 codes with error feedback (the format is
# set out in ops.reference). k_fp8_encode is the send side, k_wire_sum_fp8
# the fused receive side under the fold contract above.
# ---------------------------------------------------------------------------

fp8_wire_bytes = ref.fp8_wire_bytes


def _fp8_aligned(*operands) -> bool:
    """Contiguous fp32 / uint8 operands on 16 B boundaries, as the fp8
    kernels read and write them (None: an absent residual)."""
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0
               and t.dtype in (torch.float32, torch.uint8)
               for t in operands if t is not None)


def fp8_encode(x: torch.Tensor, residual: Optional[torch.Tensor],
               chunk: int = 256) -> torch.Tensor:
    """FP8 wire payload (uint8, fp8_wire_bytes(n, chunk)) of x + residual.
    `residual` is updated in place with the quantization error; None means
    zeros and no write-back. On the GPU one kernel does it all; operands it
    does not serve (not fp32, or a view off a 16 B boundary) and CPU tensors
    take ref.fp8_encode, whose bits the kernel reproduces up to the sign of
    a code that is zero. A chunk outside the table raises on either path."""
    flat = x.reshape(-1)
    n = flat.numel()
    nbytes = fp8_wire_bytes(n, chunk)
    if _on_gpu(flat, residual) and 1 <= n < 2 ** 31 \
            and _fp8_aligned(flat, residual):
        g = _require_native()
        res = None if residual is None else _flat_inplace(residual, "residual")
        payload = torch.empty(nbytes, dtype=torch.uint8, device=flat.device)
        g.fp8_encode(flat, res, payload, chunk)
        return payload
    return ref.fp8_encode(x, residual, chunk)


def wire_sum_fp8(payloads, n: int, chunk: int = 256,
                 out: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """Sum of the FP8 wire payloads of all parties, in fp32. On the GPU one
    kernel decodes and sums them; payloads that are views off a 16 B
    boundary, and CPU tensors, take the op sequence of ref.wire_sum_fp8."""
    if _on_gpu(out, *payloads) and _fp8_aligned(*payloads):
        g = _require_native()
        if out is None:
            out = torch.empty(n, dtype=torch.float32,
                              device=payloads[0].device)
            accumulate = False
        g.wire_sum_fp8(list(payloads), _flat_inplace(out, "out"), chunk,
                       accumulate)
        return out
    return ref.wire_sum_fp8(payloads, n, chunk, out, accumulate)


def fp8_decode(payload: torch.Tensor, n: int, chunk: int = 256
               ) -> torch.Tensor:
    """Dense fp32 tensor of one FP8 wire payload: the one-party case of
    wire_sum_fp8 (a code that is -0 comes back as +0)."""
    return wire_sum_fp8([payload], n, chunk)


# output elements per tile of k_wire_sum_bsc (None without the extension)
WIRE_BSC_TILE = getattr(_geops, "WIRE_BSC_TILE", None)

_BSC_WIRE_DTYPES = {
    2: (torch.float32, torch.int32),
    5: (torch.float32, torch.int32, torch.uint8, torch.float32, torch.int32),
}


def _wire_sum_bsc_served(payloads, n: int, out: Optional[torch.Tensor],
                         chunk_elems: Optional[int]) -> bool:
    """What k_wire_sum_bsc serves: 1 <= n < 2^31, every party's payload of
    the same form, dtypes and lengths, contiguous, lists of fewer than 2^30
    slots, a contiguous fp32 `out`; for the coded form a power-of-two chunk
    in [64, 8192] and at least one slot."""
    form = len(payloads[0])
    k = payloads[0][-1].numel()
    if not 1 <= n < 2 ** 31 or k >= 2 ** 30:
        return False
    if form == 5 and (k < 1 or chunk_elems is None
                      or not 64 <= chunk_elems <= 8192
                      or chunk_elems & (chunk_elems - 1)):
        return False
    if out is not None and (out.dtype != torch.float32 or out.numel() != n
                            or not out.is_contiguous()):
        return False
    first = payloads[0]
    return all(len(pl) == form
               and all(t.dtype == d and t.is_contiguous()
                       and t.numel() == f.numel()
                       for t, d, f in zip(pl, _BSC_WIRE_DTYPES[form], first))
               for pl in payloads)


def wire_sum_bsc(payloads, n: int, out: Optional[torch.Tensor] = None,
                 accumulate: bool = False,
                 chunk_elems: Optional[int] = None) -> torch.Tensor:
    """Dense sum of the Bi-Sparse lists of all parties, in party order. A
    payload is (vals f32[k], idx i32[k]) or, with `chunk_elems`, the coded
    form (exact, keep_idx, packed, minmax, idx): the DGTState.compress tuple
    of the zero-masked values, and the exact indices. Entries with idx < 0
    (placeholders) or idx >= n are skipped.

    Precondition: every list is in ascending index order with its
    placeholders last, as every packer writes it (bsc_compress,
    bsc_pull_compress). For a list that breaks this the values of the result
    are unspecified (no address leaves the operands). On the GPU one kernel
    does the whole sum; operands outside what it serves, and CPU tensors,
    take the op sequence of ref.wire_sum_bsc, whose bits it reproduces."""
    if not payloads or len(payloads[0]) not in _BSC_WIRE_DTYPES:
        raise ValueError("wire_sum_bsc needs at least one party, and 2 or 5 "
                         "tensors per payload")
    if _on_gpu(out, *(t for p in payloads for t in p)) \
            and _wire_sum_bsc_served(payloads, n, out, chunk_elems):
        g = _require_native()
        if out is None:
            out = torch.empty(n, dtype=torch.float32,
                              device=payloads[0][0].device)
            accumulate = False
        lists = [list(x) for x in zip(*payloads)]
        if len(lists) == 2:
            g.wire_sum_bsc(lists[0], lists[1], _flat_inplace(out, "out"),
                           accumulate)
        else:
            lists[3] = [m.reshape(-1) for m in lists[3]]
            g.wire_sum_bsc_dgt(*lists, _flat_inplace(out, "out"), chunk_elems,
                               accumulate)
        return out
    return ref.wire_sum_bsc(payloads, n, out, accumulate, chunk_elems)


# ---------------------------------------------------------------------------
# Fused optimizer updates
# ---------------------------------------------------------------------------

def sgd_update(w, g, lr, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().sgd_update(_flat_inplace(w, "w"), g.reshape(-1),
                                     lr, wd, rescale)
        return
    ref.sgd_update(w, g, lr, wd, rescale)


def sgd_mom_update(w, g, mom, lr, momentum=0.9, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().sgd_mom_update(
            _flat_inplace(w, "w"), g.reshape(-1), _flat_inplace(mom, "mom"),
            lr, momentum, wd, rescale)
        return
    ref.sgd_mom_update(w, g, mom, lr, momentum, wd, rescale)


def adam_update(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0,
                rescale=1.0):
    if _on_gpu(w):
        _require_native().adam_update(
            _flat_inplace(w, "w"), g.reshape(-1), _flat_inplace(m, "m"),
            _flat_inplace(v, "v"), t, lr, beta1, beta2, eps, wd, rescale)
        return
    ref.adam_update(w, g, m, v, t, lr, beta1, beta2, eps, wd, rescale)


def rmsprop_update(w, g, n, lr, rho=0.9, eps=1e-8, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().rmsprop_update(
            _flat_inplace(w, "w"), g.reshape(-1), _flat_inplace(n, "n"),
            lr, rho, eps, wd, rescale)
        return
    ref.rmsprop_update(w, g, n, lr, rho, eps, wd, rescale)


def adagrad_update(w, g, h, lr, eps=1e-7, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().adagrad_update(
            _flat_inplace(w, "w"), g.reshape(-1), _flat_inplace(h, "h"),
            lr, eps, wd, rescale)
        return
    ref.adagrad_update(w, g, h, lr, eps, wd, rescale)


def signsgd_update(w, g, lr, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().signsgd_update(_flat_inplace(w, "w"),
                                         g.reshape(-1), lr, wd, rescale)
        return
    ref.signsgd_update(w, g, lr, wd, rescale)


def signum_update(w, g, mom, lr, momentum=0.9, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().signum_update(
            _flat_inplace(w, "w"), g.reshape(-1), _flat_inplace(mom, "mom"),
            lr, momentum, wd, rescale)
        return
    ref.signum_update(w, g, mom, lr, momentum, wd, rescale)


def dcasgd_update(w, g, prev_w, mom, lr, lamda=0.04, momentum=0.0, wd=0.0,
                  rescale=1.0):
    if _on_gpu(w):
        # as the golden model: a momentum state is used (and written) only
        # when momentum != 0; otherwise the kernel gets no state at all
        use_mom = mom is not None and momentum != 0.0
        _require_native().dcasgd_update(
            _flat_inplace(w, "w"), g.reshape(-1),
            _flat_inplace(prev_w, "prev_w"),
            _flat_inplace(mom, "mom") if use_mom else torch.Tensor(),
            lr, lamda, momentum, wd, rescale)
        return
    ref.dcasgd_update(w, g, prev_w, mom, lr, lamda, momentum, wd, rescale)


# ---------------------------------------------------------------------------
# Layer-wise LARS (LBSGD, warmup_strategy='lars') over a flat bucket whose
# layers are the segments [seg_off[s], seg_off[s+1]): k_lars_sumsq writes the
# tiles' sums of squares, k_lars_ratio the trust ratios, k_lars_update
# applies sgd / sgd-momentum with lr * ratio[s]. Three launches and no host
# wait, whatever the number of segments.
# ---------------------------------------------------------------------------

# elements per tile of the LARS kernels (None without the extension)
LARS_TILE = getattr(_geops, "LARS_TILE", None)

_lars_table_cache: dict = {}
_lars_ws_cache: dict = {}


def _lars_tables(seg_off: torch.Tensor, n: int, device):
    """(seg_off, tile_start, tile count, offsets all multiples of 4) on
    `device` for one offsets tensor: read and checked on the host ONCE per
    distinct tensor (storage, length and version), then cached. The cache
    keeps the tensor alive, so its address names it."""
    ck = (seg_off.device, seg_off.data_ptr(), seg_off.numel(),
          seg_off._version, n, device)
    hit = _lars_table_cache.get(ck)
    if hit is None:
        if seg_off.dtype != torch.int64 or seg_off.dim() != 1 \
                or seg_off.numel() < 1:
            raise ValueError("seg_off is a 1-d int64 tensor of S+1 offsets")
        offs = seg_off.tolist()
        if offs[0] != 0 or offs[-1] != n \
                or any(b < a for a, b in zip(offs[:-1], offs[1:])):
            raise ValueError("seg_off must ascend from 0 to w.numel() = %d"
                             % n)
        tile_start = [0]
        for a, b in zip(offs[:-1], offs[1:]):
            tile_start.append(tile_start[-1] + (b - a + LARS_TILE - 1)
                              // LARS_TILE)
        if len(_lars_table_cache) > 64:
            _lars_table_cache.clear()
        hit = _lars_table_cache[ck] = (
            seg_off.to(device).contiguous(),
            torch.tensor(tile_start, dtype=torch.int64).to(device),
            tile_start[-1], all(o % 4 == 0 for o in offs), seg_off)
    return hit[:4]


def _lars_workspace(device, tiles: int) -> torch.Tensor:
    """The tiles' (sum w^2, sum g^2) pairs per (device, tile count): one
    call at a time uses it (calls on one stream do)."""
    ck = (device, tiles)
    ws = _lars_ws_cache.get(ck)
    if ws is None:
        if len(_lars_ws_cache) > 64:
            _lars_ws_cache.clear()
        ws = _lars_ws_cache[ck] = torch.empty(
            2 * max(tiles, 1), dtype=torch.float32, device=device)
    return ws


def _lars_served(*operands) -> bool:
    """What the LARS kernels serve: contiguous fp32 GPU operands of fewer
    than 2^31 elements (any alignment: VEC = 1 takes what VEC = 4 cannot)."""
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               and t.numel() < 2 ** 31 for t in operands)


def lars_ratio(w: torch.Tensor, g: torch.Tensor, seg_off: torch.Tensor,
               wd: float = 0.0, out: Optional[torch.Tensor] = None,
               n_wg: int = 0) -> torch.Tensor:
    """fp32 [S] trust ratios of LBSGD's 'lars' strategy, one per segment of
    the flat `w` / `g` (ref.lars_ratio; empty segments get 0.01). On the GPU
    two launches, reproducible bit for bit and without a host wait once the
    tables of `seg_off` are cached (the first call with a new `seg_off`
    reads it on the host). `n_wg` is the tests' grid hook (0 = default)."""
    if _on_gpu(w, g) and _lars_served(w, g):
        gk = _require_native()
        seg, tile_start, tiles, vec4 = _lars_tables(seg_off, w.numel(),
                                                    w.device)
        S = seg.numel() - 1
        if out is None:
            out = torch.empty(S, dtype=torch.float32, device=w.device)
        gk.lars_sumsq(w.view(-1), g.view(-1), seg, tile_start,
                      _lars_workspace(w.device, tiles), out, tiles, wd, vec4,
                      n_wg)
        return out
    r = ref.lars_ratio(w, g, seg_off, wd)
    if out is not None:
        out.copy_(r)
        return out
    return r


def lbsgd_update(w, g, mom, seg_off, lr, momentum=0.0, wd=0.0, rescale=1.0,
                 lbmult=1.0, ratio_out: Optional[torch.Tensor] = None,
                 g_norm: Optional[torch.Tensor] = None, n_wg: int = 0):
    """One LBSGD 'lars' step of the flat bucket `w`: segment s is updated
    by sgd (momentum == 0: no state, `mom` may be None) or sgd-momentum with
    the rate lr * ratio[s] * lbmult (ref.lbsgd_update). The ratios are taken
    of `g` before `rescale`, or of `g_norm` when given (the unclipped
    gradient), and returned (in `ratio_out` when given). On the GPU this is
    three launches and no host wait."""
    use_mom = momentum != 0.0
    if use_mom and mom is None:
        raise ValueError("lbsgd_update with momentum needs its state")
    gn = g if g_norm is None else g_norm
    operands = (w, g, gn) + ((mom,) if use_mom else ())
    if _on_gpu(*operands) and _lars_served(*operands):
        gk = _require_native()
        wf = _flat_inplace(w, "w")
        ratio = lars_ratio(wf, gn, seg_off, wd, out=ratio_out, n_wg=n_wg)
        seg, tile_start, tiles, vec4 = _lars_tables(seg_off, wf.numel(),
                                                    w.device)
        gk.lars_update(wf, g.view(-1),
                       _flat_inplace(mom, "mom") if use_mom
                       else torch.Tensor(),
                       seg, tile_start, ratio, tiles, lr, lbmult, momentum,
                       wd, rescale, vec4, n_wg)
        return ratio
    ratio = ref.lbsgd_update(w, g, mom, seg_off, lr, momentum, wd, rescale,
                             lbmult, g_norm=g_norm)
    if ratio_out is not None:
        ratio_out.copy_(ratio)
        return ratio_out
    return ratio


# ---------------------------------------------------------------------------
# Row-sparse push: duplicate merge, row scatter, row-indexed updates.
# Tables, states and merged rows are 2-d [rows][width] fp32; ids are int64.
# Ids outside [0, rows) (the -1 padding included) are skipped.
# ---------------------------------------------------------------------------

def rsp_merge(ids: torch.Tensor, vals: torch.Tensor
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sum duplicate rows deterministically (ascending original position).
    Returns (out_ids[nnz], out_vals[nnz][width]): unique ids ascending,
    unused tail slots id -1 / zero rows. The outputs are sized by the
    upper bound nnz, so the GPU path never reads a count to the host."""
    if _on_gpu(ids, vals):
        g = _require_native()
        ids = ids.reshape(-1).long()
        nnz = ids.numel()
        if vals.dim() != 2:
            vals = vals.reshape(nnz, -1)
        vals = vals.float().contiguous()
        out_ids = torch.full((nnz,), -1, dtype=torch.int64,
                             device=vals.device)
        out_vals = torch.zeros_like(vals)
        if nnz == 0:
            return out_ids, out_vals
        sorted_ids, perm = torch.sort(ids, stable=True)
        head = torch.zeros_like(sorted_ids)
        head[1:] = sorted_ids[1:] != sorted_ids[:-1]
        seg = torch.cumsum(head, 0)  # seg[p] = unique index of position p
        g.rsp_merge(sorted_ids, perm, seg, vals, out_ids, out_vals)
        return out_ids, out_vals
    return ref.rsp_merge(ids, vals)


def rsp_scatter(dense, ids, merged, accumulate=False):
    if _on_gpu(dense):
        _require_native().rsp_scatter(dense, ids, merged, accumulate)
        return
    ref.rsp_scatter(dense, ids, merged, accumulate)


def rsp_sgd_update(w, ids, merged, lr, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().rsp_sgd_update(w, ids, merged, lr, wd, rescale)
        return
    ref.rsp_sgd_update(w, ids, merged, lr, wd, rescale)


def rsp_sgd_mom_update(w, ids, merged, mom, lr, momentum=0.9, wd=0.0,
                       rescale=1.0):
    if _on_gpu(w):
        _require_native().rsp_sgd_mom_update(w, ids, merged, mom, lr,
                                             momentum, wd, rescale)
        return
    ref.rsp_sgd_mom_update(w, ids, merged, mom, lr, momentum, wd, rescale)


def rsp_adam_update(w, ids, merged, m, v, t, lr, beta1=0.9, beta2=0.999,
                    eps=1e-8, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().rsp_adam_update(w, ids, merged, m, v, t, lr, beta1,
                                          beta2, eps, wd, rescale)
        return
    ref.rsp_adam_update(w, ids, merged, m, v, t, lr, beta1, beta2, eps, wd,
                        rescale)


def rsp_adagrad_update(w, ids, merged, h, lr, eps=1e-7, wd=0.0, rescale=1.0):
    if _on_gpu(w):
        _require_native().rsp_adagrad_update(w, ids, merged, h, lr, eps, wd,
                                             rescale)
        return
    ref.rsp_adagrad_update(w, ids, merged, h, lr, eps, wd, rescale)
