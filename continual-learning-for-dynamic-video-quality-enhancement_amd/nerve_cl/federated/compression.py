"""Compressed client updates on the client matrix (csrc/compress.hip): top-k sparsification with error
feedback (Stich et al. 2018, "Sparsified SGD with memory"; Lin et al. 2018, "Deep Gradient Compression") and stochastic uniform
quantisation (QSGD, Alistarh et al. 2017).

The compressed update is written back into the client's row, so every aggregation rule, the update clip, the server optimizers
and the noise work on it unchanged.  The arithmetic is the contract of ``nvq_fed_compress`` (include/nvq.h): every step a single
correctly rounded IEEE operation, so the CPU path here and the kernel give the same values.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import numpy as np
import torch

from nerve_cl import _engine, _nvq
from nerve_cl.federated import _philox
from nerve_cl.federated._flat import check_clients

__all__ = ["compress_updates_", "topk_count", "wire_bytes", "COMPRESSIONS"]

COMPRESSIONS = ("topk", "quant", "topk_quant")


def topk_count(n: int, ratio: float) -> int:
    """the number of coordinates a top-k of ``ratio`` keeps of ``n``: ``max(1, ceil(ratio * n))``"""
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"invalid ratio: {ratio}")
    return max(1, math.ceil(ratio * n))


def wire_bytes(n: int, kept: int, levels: int) -> int:
    """What a row of ``n`` coordinates of which ``kept`` are non-zero costs to send, in bytes.
    This is a model, not a measurement: nothing here is serialised.  A value costs 4 bytes, or with ``levels > 0`` the ``ceil(log2(2 levels + 1))`` bits
    of its signed level; a sparse row (``kept < n``) sends a 4-byte index and the value in whole bytes per kept coordinate, a
    dense quantised row the packed bits of all ``n`` values and its 4-byte scale, a dense row ``4 n``."""
    if n < 0 or not 0 <= kept <= n or not 0 <= levels <= _nvq.FED_COMPRESS_MAX_LEVELS:
        raise ValueError(f"wire_bytes: n = {n}, kept = {kept}, levels = {levels}")
    bits = (2 * levels).bit_length() if levels > 0 else 32        # ceil(log2(2 levels + 1))
    if kept < n:
        return kept * (4 + (bits + 7) // 8)
    if levels > 0:
        return (n * bits + 7) // 8 + 4
    return 4 * n


def _check_slots(slots, K: int, rows: int, dev) -> Optional[torch.Tensor]:
    """``slots`` as K int32 values on ``dev``; a host list is checked for duplicates and range, a tensor on the GPU is the caller's"""
    if slots is None:
        if rows < K:
            raise ValueError(f"residual: {rows} rows for {K} clients")
        return None
    if isinstance(slots, torch.Tensor) and slots.is_cuda:
        if slots.dtype != torch.int32 or slots.numel() != K:
            raise ValueError(f"slots: device slots are {K} int32 values")
        return slots
    host = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
    if len(host) != K:
        raise ValueError(f"{len(host)} slots for {K} clients")
    if len(set(host)) != K or any(not 0 <= s < rows for s in host):
        raise ValueError(f"slots: distinct rows in 0 .. {rows - 1}, got {host}")
    return torch.tensor(host, dtype=torch.int32).to(dev)


def _compress_cpu(clients, base, k, levels, residual, slots, seed, offset) -> torch.Tensor:
    K, n = clients.shape
    rows = list(range(K)) if slots is None else [int(s) for s in slots.tolist()]
    x = clients.detach().double().numpy()
    b32 = base.detach().reshape(1, n).numpy() if base is not None else np.zeros((1, n), dtype=np.float32)
    b = b32.astype(np.float64)
    with np.errstate(all="ignore"):
        a64 = x - b
        if residual is not None:
            a64 = a64 + residual.detach()[rows, :n].double().numpy()
        a = np.ascontiguousarray(a64.astype(np.float32))
        key = a.view(np.uint32) & np.uint32(0x7FFFFFFF)
        key[key > 0x7F800000] = 0x7FFFFFFF
        keep = np.ones((K, n), dtype=bool)
        if k is not None and k < n:
            keep = key >= np.partition(key, n - k, axis=1)[:, n - k:n - k + 1]
        c = a.copy()
        if levels > 0 and n > 0:
            top = key.max(axis=1)
            s = float(levels)
            for r in np.nonzero((top != 0) & (top < 0x7F800000))[0]:
                scale = float(top[r:r + 1].view(np.float32)[0])
                w = _philox.words(seed, offset + int(r), 0, (n + 3) // 4).reshape(-1)[:n]
                u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
                ar = a[r].astype(np.float64)
                xi = np.floor(np.abs(ar) * s / scale + u)
                c[r] = (np.sign(ar) * xi * scale / s).astype(np.float32)
        xn = np.where(keep, (b + c.astype(np.float64)).astype(np.float32), np.broadcast_to(b32, (K, n)))
        e = (a.astype(np.float64) - (xn.astype(np.float64) - b)).astype(np.float32)
        e[~np.isfinite(e)] = 0.0
    clients.copy_(torch.from_numpy(xn))
    if residual is not None:
        residual[rows, :n] = torch.from_numpy(e)
    return torch.from_numpy(keep.sum(axis=1).astype(np.int32))


def compress_updates_(clients: torch.Tensor, base: Optional[torch.Tensor] = None, *, k: Optional[int] = None, levels: int = 0,
                      residual: Optional[torch.Tensor] = None, slots: "Union[None, Sequence[int], torch.Tensor]" = None,
                      seed: int = 0, offset: int = 0) -> torch.Tensor:
    """Compress the updates ``clients[r] - base`` of a ``[K, n]`` fp32 matrix in place and return ``kept``, K int32 values on the
    matrix's device (a row stride above n is fine; no ``base``: zeros).

    Per row, ``a = (x - base) + e`` with ``e`` the row's residual (none without ``residual``).  ``k``: only the k coordinates of
    largest ``|a|`` are kept, every other one goes back to ``base``; ties at the k-th magnitude are all kept, so ``kept[r] >= k``
    (``None`` or ``k >= n``: all are kept).  ``levels = s > 0``: a kept ``a_i`` becomes ``sgn(a_i) * xi_i * scale / s`` with ``scale
    = max |a|`` of the row and ``xi_i = floor(|a_i| s / scale + u_i)``, ``u_i`` uniform from the Philox stream ``(seed, offset + r)``:
    QSGD, unbiased; a row whose ``scale`` is 0, inf or NaN is not quantised.  The row then holds ``x' = base + c`` (or ``base``) and,
    with ``residual`` (an ``[M, >= n]`` fp32 matrix), row ``slots[r]`` of it (``slots`` None: row r) receives ``a - (x' - base)``,
    what was not sent and the rounding of ``x'``, for the next round; a value that is not finite is stored as 0.  ``slots`` on the
    host is checked (distinct, in range: ``ValueError``) and written to a small device tensor; given as an int32 tensor on the
    device it is used as it is.

    On the GPU: one ``nvq_fed_compress`` (include/nvq.h has the contract to the last rounding), nothing read back.  CPU tensors
    take the same formula in float64 numpy operations and give the same values."""
    check_clients(clients, base)
    K, n = clients.shape
    if k is not None and (int(k) != k or k < 1):
        raise ValueError(f"invalid k: {k} (None: no top-k)")
    if int(levels) != levels or not 0 <= levels <= _nvq.FED_COMPRESS_MAX_LEVELS:
        raise ValueError(f"levels: 0 .. {_nvq.FED_COMPRESS_MAX_LEVELS}, got {levels}")
    if seed < 0 or offset < 0:
        raise ValueError("seed and offset are non-negative")
    dev = clients.device
    if base is not None and base.device != dev:
        raise ValueError("base lives on another device than clients")
    if residual is None:
        if slots is not None:
            raise ValueError("slots without a residual")
        slots_t = None
    else:
        if residual.dim() != 2 or residual.dtype != torch.float32 or residual.shape[1] < n or residual.device != dev:
            raise ValueError("residual: an [M, >= n] float32 matrix on the device of clients")
        slots_t = _check_slots(slots, K, residual.shape[0], dev)
    k, levels = None if k is None else int(k), int(levels)
    if not clients.is_cuda:
        return _compress_cpu(clients, base, k, levels, residual, slots_t, seed, offset)
    kept = torch.empty(K, dtype=torch.int32, device=dev)
    with _nvq.device_guard(dev):
        _nvq.fed_compress(clients, n, None if base is None else base.reshape(-1), k or 0, levels, residual, slots_t, kept,
                          _engine.workspace(dev), seed=seed, offset=offset)
    return kept
