"""DGT (Differential Gradient Transmission) for the WAN tier.

Reference behavior (3rdparty/ps-lite: kv_app.h:842-995, van.cc:707-824):
each push tensor is split into fixed-size chunks; a per-chunk EWMA
"contribution" (mean |g|) ranks them; the top DMLC_K fraction travels
reliably at full precision, the rest over lossy low-priority channels,
optionally 4-bit linearly quantized with residual feedback
(ENABLE_DGT=3).

MI355X-native mapping: xGMI/RCCL has no lossy transport, so
"unimportant" chunks become 4-bit-quantized chunks (same traffic
reduction, deterministic instead of lossy) and the priority ordering
becomes the charge model: exact bytes for important chunks + half-byte
per element for the rest.
"""

from __future__ import annotations

import math
from typing import Tuple

import torch

from .. import ops


class DGTState:
    def __init__(self, numel: int, device, chunk_elems: int = 1024,
                 k: float = 0.5, alpha: float = 0.3, mode: int = 3):
        """mode mirrors ENABLE_DGT (van.cc:736-748 Unimportant_send):
        1 = UDP lossy full-precision, 2 = TCP full-precision low
        priority, 3 = TCP + 4-bit encode. Modes 1/2 keep unimportant
        chunks exact on the wire (full bytes charged); only mode 3
        quantizes them. Mode 1's packet loss has no RCCL analog — its
        deterministic stand-in is the zero-contribution chunk drop that
        all modes share (the receiver zero-fills, van.cc:356-366)."""
        self.numel = numel
        self.chunk = chunk_elems
        self.k = k
        self.alpha = alpha
        self.mode = mode if mode in (1, 2, 3) else 3
        self.nchunks = (numel + chunk_elems - 1) // chunk_elems
        self.contrib = None
        self.residual = torch.zeros(numel, device=device)
        self.n_keep = max(1, int(math.ceil(self.k * self.nchunks)))

    # ------------------------------------------------------------------
    # wire form (mode 3): what actually crosses the leader tier.
    # The reference ships exact bytes for important chunks and 4-bit
    # codes + a per-chunk codebook for the rest (van.cc:750-824); here
    # the payload is a fixed-shape tuple so RCCL all_gather can carry it
    # without variable-length framing:
    #   exact    f32 [n_keep*chunk]   important chunks, full precision
    #   keep_idx i32 [n_keep]         which chunks are exact (sorted)
    #   packed   u8  [n_lossy*chunk/2] 4-bit codes of the rest
    #   minmax   f32 [n_lossy, 2]     per-chunk codebook (lo, hi)
    # Zero-contribution chunks reconstruct to ~0 (minmax zeroed), the
    # deterministic analog of the reference dropping them from the send
    # (kv_app.h:973, receiver zero-fill van.cc:356-366).
    # ------------------------------------------------------------------
    def _update_contrib(self, flat: torch.Tensor) -> None:
        contrib = ops.dgt_contribution(flat, self.chunk)
        if self.contrib is None or self.contrib.numel() != contrib.numel():
            self.contrib = contrib
        else:
            self.contrib = (self.alpha * self.contrib
                            + (1 - self.alpha) * contrib)

    def wire_bytes(self) -> int:
        """Real bytes per payload (mode 3)."""
        n_lossy = self.nchunks - self.n_keep
        return (self.n_keep * self.chunk * 4 + self.n_keep * 4
                + n_lossy * (self.chunk // 2 + 8))

    def compress(self, x: torch.Tensor):
        """Mode-3 wire payload. Same EWMA/residual state machine as
        transform(); shapes are identical on every rank for the same
        (numel, chunk_elems, k), so the tuple all_gathers directly."""
        assert self.mode >= 3, "wire payload exists only for mode 3"
        flat = x.reshape(-1)
        self._update_contrib(flat)
        keep_idx = torch.topk(self.contrib, self.n_keep).indices \
            .sort().values
        # exact rows, 4-bit rows, codebooks and the residual update (zero
        # for kept chunks, quantization error for the rest): one kernel on
        # the GPU, the op sequence of ops.reference.dgt_encode elsewhere
        return ops.dgt_encode(flat, self.residual, self.contrib, keep_idx,
                              self.chunk)

    def decompress(self, exact: torch.Tensor, keep_idx: torch.Tensor,
                   packed: torch.Tensor, minmax: torch.Tensor) -> torch.Tensor:
        """Rebuild a dense tensor from a wire payload (any rank's)."""
        dev = exact.device
        n_keep = keep_idx.numel()
        n_lossy = self.nchunks - n_keep
        keep_mask = torch.zeros(self.nchunks, dtype=torch.bool, device=dev)
        keep_mask[keep_idx.long()] = True
        lossy_idx = (~keep_mask).nonzero(as_tuple=True)[0]
        out = torch.zeros(self.nchunks, self.chunk, device=dev)
        if n_lossy:
            deq = ops.dequantize_4bit_chunked(
                packed, minmax.view(n_lossy, 2), n_lossy * self.chunk,
                self.chunk)
            out[lossy_idx] = deq.to(dev).view(n_lossy, self.chunk)
            # minmax == (0,0) marks an untransmitted (dead) chunk: the
            # 1e-30 span dequantizes to ~3e-32, i.e. exact zero fill
        out[keep_idx.long()] = exact.view(n_keep, self.chunk)
        return out.reshape(-1)[:self.numel]

    def transform(self, x: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """Return (lossy reconstruction, wire bytes). Important chunks
        pass through exactly; unimportant chunks are 4-bit quantized
        with residual feedback."""
        flat = x.reshape(-1)
        contrib = ops.dgt_contribution(flat, self.chunk)
        if self.contrib is None or self.contrib.numel() != contrib.numel():
            self.contrib = contrib
        else:
            # EWMA per the reference (kv_app.h:875): alpha weights the
            # OLD value: c = alpha*c_old + (1-alpha)*mean|g|
            self.contrib = (self.alpha * self.contrib
                            + (1 - self.alpha) * contrib)
        n_keep = max(1, int(math.ceil(self.k * self.nchunks)))
        keep = torch.topk(self.contrib, n_keep).indices
        keep_mask = torch.zeros(self.nchunks, dtype=torch.bool,
                                device=flat.device)
        keep_mask[keep] = True
        # zero-contribution chunks are not transmitted at all (the
        # reference drops them from the send, kv_app.h:973; the
        # receiver zero-fills)
        dead_mask = self.contrib == 0
        n_dead = int(dead_mask.sum())
        elem_keep = keep_mask.repeat_interleave(self.chunk)[:self.numel]
        elem_dead = dead_mask.repeat_interleave(self.chunk)[:self.numel]
        if self.mode >= 3:
            packed, minmax = ops.quantize_4bit_chunked(flat, self.chunk,
                                                       self.residual)
            deq = ops.dequantize_4bit_chunked(packed,
                                              minmax.to(flat.device),
                                              self.numel, self.chunk)
            out = torch.where(elem_keep, flat, deq.to(flat.device))
            # residual only meaningful for quantized chunks; zero it for
            # exact chunks (they carried no error)
            self.residual[elem_keep] = 0.0
            lossy_elem_bytes = self.chunk // 2 + 8
        else:
            # modes 1/2: unimportant chunks travel exact (low priority /
            # lossy channel, but full precision on the wire)
            out = flat.clone()
            lossy_elem_bytes = self.chunk * 4
        out = torch.where(elem_dead, torch.zeros((), device=flat.device),
                          out)
        n_lossy = self.nchunks - n_keep - max(0, n_dead - int(
            (dead_mask & keep_mask).sum()))
        exact_bytes = n_keep * self.chunk * 4
        wire = min(self.numel * 4, exact_bytes) \
            + max(0, n_lossy) * lossy_elem_bytes
        return out, wire
