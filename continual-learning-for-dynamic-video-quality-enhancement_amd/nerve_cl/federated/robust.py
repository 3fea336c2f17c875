"""Byzantine-robust aggregation on the client matrix: coordinate-wise trimmed mean and median (Yin et al., "Byzantine-Robust
Distributed Learning: Towards Optimal Statistical Rates", 2018) and Krum / multi-Krum (Blanchard et al., "Machine Learning with
Adversaries: Byzantine Tolerant Gradient Descent", 2017) on the ``[K, n]`` matrix whose rows are the clients' weights
(csrc/robust.hip).

A row is *live* when ``weights`` is None or its weight is positive; ``m`` is the number of live rows.  A row that is not live is
never read by the aggregation pass: a client without samples whose row holds NaN does not reach the result (through
``aggregate_flat`` it does, as ``0 * NaN``).

- ``aggregate_flat_trimmed``: per coordinate the live rows' values are sorted (NaN after +inf, as ``np.sort``), the ``t = min(trim,
  (m - 1) // 2)`` lowest and highest are dropped and the rest averaged; ``trim = 0`` is the unweighted mean of the live rows,
  ``aggregate_flat_median`` the coordinate-wise median (numpy's: the mean of the two middle values for an even ``m``).
- ``krum_select``: from the Gram matrix of the updates (``update_gram``), ``D_ij = max(0, G_ii + G_jj - 2 G_ij)`` (a NaN distance
  counts as +inf), the score of a live row is the sum of its ``c = clamp(m - f - 2, 1, m - 1)`` smallest distances to the other
  live rows, and the ``num_selected`` rows with the lowest (score, index) get weight 1, all others 0.
- ``krum_aggregate_flat``: ``update_gram``, ``krum_select`` and the trim-0 pass with the selection as weights: the mean of the
  selected rows, the rejected rows never touched.

On CUDA tensors these are HIP kernels and nothing is read back; CPU tensors take the same definitions in float64 torch operations.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from nerve_cl import _nvq
from nerve_cl.federated._flat import check_clients, device_weights, finish_cpu, host_weights
from nerve_cl.federated.clustering import update_gram

__all__ = ["KrumResult", "aggregate_flat_trimmed", "aggregate_flat_median", "krum_select", "krum_aggregate_flat"]

TRIM_MEDIAN = _nvq.FED_TRIM_MEDIAN


def aggregate_flat_trimmed(clients: torch.Tensor, trim: int, weights=None, base: Optional[torch.Tensor] = None,
                           server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0, offset: int = 0,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = base[i] + server_lr * a_i + noise_std * z_i`` for a ``[K, n]`` fp32 matrix of client weight vectors, ``a_i`` the
    trimmed mean over the live rows of ``clients[k, i] - base[i]``: the values sorted ascending (NaN last), positions ``t .. m - 1 -
    t`` added in that order in float64 and divided by ``m - 2 t``, ``t = min(trim, (m - 1) // 2)``.  No ``base``: zeros.  ``z`` is the
    Philox stream (seed, offset) of ``nerve_cl.federated._philox``, as in ``aggregate_flat``.  ``out`` may be ``base``.

    ``weights`` only say which rows are live (None: all): a sequence or CPU tensor is checked on the host and raises ``ValueError``
    without a positive entry; a float64 tensor on the device is used as it is.  On the GPU one ``nvq_fed_trimmed_aggregate``,
    nothing read back."""
    check_clients(clients, base)
    K, n = clients.shape
    trim = int(trim)
    if trim < 0:
        raise ValueError(f"invalid trim: {trim}")
    host = host_weights(weights, K, "aggregate_flat_trimmed", allow_none=True, need="live")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=clients.device)
    if clients.is_cuda:
        dev = clients.device
        with _nvq.device_guard(dev):
            _nvq.fed_trimmed_aggregate(clients, n, base, device_weights(weights, host, dev), trim, out, server_lr=server_lr,
                                       noise_std=noise_std, seed=seed, offset=offset)
        return out
    if host is None and weights is not None:
        raise ValueError("aggregate_flat_trimmed: device weights with clients on the CPU")
    live = [k for k in range(K) if host is None or host[k] > 0]
    m = len(live)
    t = min(trim, (m - 1) // 2)
    b = base.double() if base is not None else torch.zeros(n, dtype=torch.float64)
    d = torch.sort(clients[live], dim=0).values.double() - b.view(1, n)        # torch.sort puts NaN last, as np.sort does
    a = torch.zeros(n, dtype=torch.float64)
    for j in range(t, m - t):
        a = a + d[j]
    a = a / (m - 2 * t)
    return finish_cpu(b + server_lr * a, noise_std, seed, offset, out)


def aggregate_flat_median(clients: torch.Tensor, weights=None, base: Optional[torch.Tensor] = None, server_lr: float = 1.0,
                          noise_std: float = 0.0, seed: int = 0, offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``aggregate_flat_trimmed`` with the largest trim: the coordinate-wise median of the live rows (an odd ``m``: the middle
    value, bit for bit with no ``base`` and ``server_lr = 1``; an even ``m``: the mean of the two middle values)"""
    return aggregate_flat_trimmed(clients, TRIM_MEDIAN, weights=weights, base=base, server_lr=server_lr, noise_std=noise_std,
                                  seed=seed, offset=offset, out=out)


class KrumResult(NamedTuple):
    """``weights`` float64 [K]: 1.0 for the selected rows, else 0.0; ``scores`` float64 [K]: the Krum scores (+inf for a row that is
    not live); ``order`` int32 [K]: the live rows by (score, index) ascending, then the other rows by index: tensors on the Gram's
    device"""
    weights: torch.Tensor
    scores: torch.Tensor
    order: torch.Tensor


def krum_select(gram: torch.Tensor, num_byzantine: int, num_selected: int = 1, weights=None) -> KrumResult:
    """Krum (``num_selected = 1``) and multi-Krum selection from the ``(K, K)`` float64 Gram matrix of the updates: see the module
    text.  ``num_byzantine`` is ``f``, the number of rows assumed hostile; Krum's guarantee needs ``m >= 2 f + 3``, and ``m < f + 3``
    (known on the host: ``weights`` None, a sequence or a CPU tensor) raises ``ValueError``.  On the GPU one
    ``nvq_fed_krum_select``, one workgroup, nothing read back."""
    if gram.dim() != 2 or gram.shape[0] != gram.shape[1] or gram.dtype != torch.float64:
        raise ValueError("gram: a (K, K) float64 matrix")
    K = gram.shape[0]
    if not 1 <= K <= _nvq.FED_MAX_CLIENTS:
        raise ValueError(f"gram: 1 .. {_nvq.FED_MAX_CLIENTS} rows")
    f, q = int(num_byzantine), int(num_selected)
    if f < 0:
        raise ValueError(f"invalid num_byzantine: {f}")
    if q < 1:
        raise ValueError(f"invalid num_selected: {q}")
    host = host_weights(weights, K, "krum_select", allow_none=True, need="live")   # None: no weights, or used as they are
    if host is None and weights is not None and not gram.is_cuda:
        raise ValueError("krum_select: device weights with a Gram matrix on the CPU")
    if weights is None or host is not None:
        m = K if host is None else sum(w > 0 for w in host)
        if m < f + 3:
            raise ValueError(f"krum_select: {m} live rows with num_byzantine = {f}: Krum needs at least f + 3")
    if gram.is_cuda:
        dev = gram.device
        out_w = torch.empty(K, dtype=torch.float64, device=dev)
        scores = torch.empty(K, dtype=torch.float64, device=dev)
        order = torch.empty(K, dtype=torch.int32, device=dev)
        with _nvq.device_guard(dev):
            _nvq.fed_krum_select(gram.contiguous(), K, device_weights(weights, host, dev), f, q, out_w, scores, order)
        return KrumResult(out_w, scores, order)
    live = [k for k in range(K) if host is None or host[k] > 0]
    m = len(live)
    c = min(max(m - f - 2, 1), m - 1)
    diag = gram.diagonal()
    D = (diag.view(K, 1) + diag.view(1, K) - 2.0 * gram).clamp_min(0.0)
    D = torch.where(D != D, torch.full_like(D, float("inf")), D)                # a NaN distance counts as the largest
    scores = torch.full((K,), float("inf"), dtype=torch.float64)
    for i in live:
        d = torch.sort(D[i, [j for j in live if j != i]]).values
        s = torch.zeros((), dtype=torch.float64)
        for p in range(c):
            s = s + d[p]
        scores[i] = s
    sv = scores.tolist()
    ranked = sorted(live, key=lambda i: (sv[i] != sv[i], sv[i] if sv[i] == sv[i] else 0.0, i))
    order = ranked + [k for k in range(K) if k not in live]
    out_w = torch.zeros(K, dtype=torch.float64)
    out_w[ranked[:min(q, m)]] = 1.0
    return KrumResult(out_w, scores, torch.tensor(order, dtype=torch.int32))


def krum_aggregate_flat(clients: torch.Tensor, num_byzantine: int, num_selected: int = 1, base: Optional[torch.Tensor] = None,
                        weights=None, server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0, offset: int = 0,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = base + server_lr * mean over the selected rows of (clients[k] - base) + noise_std * z``: the rows are selected by
    ``krum_select`` on ``update_gram(clients, base)`` and averaged by ``aggregate_flat_trimmed`` with ``trim = 0`` and the selection
    as weights.  On the GPU four launches (the Gram pass and its finishing launch, the selection, the mean) and no synchronisation.
    ``out`` may be ``base``."""
    check_clients(clients, base)
    K = clients.shape[0]
    host = host_weights(weights, K, "krum_aggregate_flat", allow_none=True, need="live")
    if clients.is_cuda:
        weights = device_weights(weights, host, clients.device)
        if host is not None and sum(w > 0 for w in host) < int(num_byzantine) + 3:
            raise ValueError(f"krum_aggregate_flat: {sum(w > 0 for w in host)} live rows with num_byzantine = {num_byzantine}: "
                             "Krum needs at least f + 3")
    elif host is not None:
        weights = host
    res = krum_select(update_gram(clients, base), num_byzantine, num_selected, weights=weights)
    return aggregate_flat_trimmed(clients, 0, weights=res.weights, base=base, server_lr=server_lr, noise_std=noise_std, seed=seed,
                                  offset=offset, out=out)
