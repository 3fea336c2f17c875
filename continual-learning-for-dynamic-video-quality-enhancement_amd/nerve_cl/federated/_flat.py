"""What ``aggregate_flat``, ``aggregate_flat_clustered``, ``aggregate_flat_trimmed`` and ``krum_aggregate_flat`` share: the checks
of the ``[K, n]`` client matrix and of the weights, and the CPU epilogue.  A further aggregation rule starts from these."""
from __future__ import annotations

from typing import List, Optional

import torch

from nerve_cl import _nvq
from nerve_cl.federated import _philox


def check_clients(clients: torch.Tensor, base: Optional[torch.Tensor] = None) -> None:
    if clients.dim() != 2 or clients.dtype != torch.float32:
        raise ValueError("clients: a [K, n] float32 matrix")
    if not 1 <= clients.shape[0] <= _nvq.FED_MAX_CLIENTS:
        raise ValueError(f"clients: 1 .. {_nvq.FED_MAX_CLIENTS} rows")
    if base is not None and (base.dtype != torch.float32 or base.numel() != clients.shape[1]):
        raise ValueError("base: a float32 vector of n elements")


def host_weights(weights, K: int, what: str, *, allow_none: bool, need: str) -> Optional[List[float]]:
    """The weights as K host floats, checked; None when they are None (``allow_none``) or a tensor on the device, which is used as
    it is after a dtype / size check.  ``need``: ``"sum"``, none negative and not all zero (a weighted mean divides by their sum), or
    ``"live"``, at least one positive (they only say which rows are live)."""
    if weights is None and allow_none:
        return None
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if weights.dtype != torch.float64 or weights.numel() != K:
            raise ValueError(f"{what}: device weights are {K} float64 values")
        return None
    host = [float(w) for w in (weights.tolist() if isinstance(weights, torch.Tensor) else weights)]
    if len(host) != K:
        raise ValueError(f"{len(host)} weights for {K} clients" if need == "sum" else f"{what}: {len(host)} weights for {K} clients")
    if need == "sum" and (any(w < 0 for w in host) or not sum(host) > 0):
        raise ValueError(f"{what}: the weights are non-negative and not all zero")
    if need == "live" and not any(w > 0 for w in host):
        raise ValueError(f"{what}: no weight is positive, so no row is live")
    return host


def device_weights(weights, host: Optional[List[float]], dev) -> Optional[torch.Tensor]:
    """``host`` (from ``host_weights``) as a float64 tensor on ``dev``; without it ``weights`` itself (None or already there)"""
    if host is not None:
        return torch.tensor(host, dtype=torch.float64).to(dev)
    return weights


def finish_cpu(v: torch.Tensor, noise_std: float, seed: int, offset: int, out: torch.Tensor) -> torch.Tensor:
    """The CPU epilogue of the kernels: the float64 result rounded to fp32, the Philox stream (seed, offset) added in double and
    rounded again, copied into ``out``."""
    v = v.to(torch.float32)
    if noise_std != 0.0:
        v = (v.double() + noise_std * torch.from_numpy(_philox.normals(seed, offset, v.numel()))).to(torch.float32)
    out.copy_(v)
    return out
