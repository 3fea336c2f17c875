"""Federated optimisation for clients that differ (csrc/fedopt.hip).

FedOpt (Reddi et al. 2021, "Adaptive Federated Optimization"; FedAvgM: Hsu et al. 2019) treats the aggregated client update as a
pseudo-gradient and lets the server run momentum, Adagrad, Adam or Yogi on it: ``ServerOptimizer``.  FedProx (Li et al. 2020) adds
``mu / 2 |theta - theta_round|^2`` to every client's objective; its gradient on a flat bucket is ``prox_grad_``.

Both are one launch over the flat buffers on the GPU and the same formula in float64 torch operations on CPU tensors.  The
library takes the hyper-parameters as fp32 values, so both paths use them rounded to fp32."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from nerve_cl import _engine, _nvq
from nerve_cl.federated._flat import check_clients, device_weights, finish_cpu, host_weights

__all__ = ["SERVER_OPTIMIZERS", "ServerOptimizer", "prox_grad_"]

SERVER_OPTIMIZERS = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")
_RULES = {"fedavgm": _nvq.FED_OPT_AVGM, "fedadagrad": _nvq.FED_OPT_ADAGRAD, "fedadam": _nvq.FED_OPT_ADAM,
          "fedyogi": _nvq.FED_OPT_YOGI}


def _f32(x: float) -> float:
    """x as the library receives it: rounded to fp32"""
    return float(np.float32(x))


class ServerOptimizer:
    """``ServerOptimizer(rule, lr=1.0, betas=(0.9, 0.99), tau=1e-3)``: the server's optimizer state for ONE parameter vector.

    ``rule``: one of ``SERVER_OPTIMIZERS``.  With ``D = sum_k c_k (x_k - base)`` the aggregated update of a round (``c_k`` as in
    ``aggregate_flat``), everything per element in float64:

    * ``fedavgm``: ``m = beta1 * m + D``, ``step = m`` (``beta1 = 0`` is plain FedAvg, to the bit).
    * the adaptive rules: ``m = beta1 * m + (1 - beta1) * D`` and ``fedadagrad``: ``v = v + D^2``; ``fedadam``: ``v = beta2 * v +
      (1 - beta2) * D^2``; ``fedyogi``: ``v = v - (1 - beta2) * D^2 * sign(v - D^2)``; ``step = m / (sqrt(v) + tau)``.

    ``out = base + lr * step (+ noise)``.  ``m`` and ``v`` are fp32 vectors, each the float64 value rounded once; the step uses the
    unrounded values.  ``m`` starts at zero and ``v`` at ``tau**2``, the paper's ``v_{-1} >= tau^2`` (Flower's strategies start
    ``v`` at 0, so a first round differs from theirs).  An adaptive rule moves every coordinate by about ``lr`` per round whatever
    the size of the update: the default ``lr = 1.0`` is a FedAvg value and far too large for ``fedadagrad`` / ``fedadam`` /
    ``fedyogi``, where 1e-3 .. 1e-1 of the weights' scale is usual."""

    def __init__(self, rule: str, lr: float = 1.0, betas: Sequence[float] = (0.9, 0.99), tau: float = 1e-3):
        if rule not in SERVER_OPTIMIZERS:
            raise ValueError(f"rule {rule!r}: one of {', '.join(SERVER_OPTIMIZERS)}")
        if len(betas) != 2 or not all(0.0 <= _f32(b) < 1.0 for b in betas):
            raise ValueError(f"invalid betas: {tuple(betas)} (two values in [0, 1))")
        if not _f32(tau) > 0.0:
            raise ValueError(f"invalid tau: {tau}")
        if not lr == lr:
            raise ValueError(f"invalid lr: {lr}")
        self.rule, self.lr, self.betas, self.tau = rule, float(lr), (float(betas[0]), float(betas[1])), float(tau)
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None

    @property
    def adaptive(self) -> bool:
        return self.rule != "fedavgm"

    def _state(self, n: int, dev) -> None:
        if self.m is None:
            self.m = torch.zeros(n, dtype=torch.float32, device=dev)
            self.v = torch.full((n,), _f32(self.tau) ** 2, dtype=torch.float32, device=dev) if self.adaptive else None
        if self.m.numel() != n or self.m.device != dev:
            raise ValueError(f"the server state holds {self.m.numel()} floats on {self.m.device}, the clients have {n} on {dev}")

    def step(self, clients: torch.Tensor, weights, base: torch.Tensor, *, clip_norm: Optional[float] = None, noise_std: float = 0.0,
             seed: int = 0, offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One server step from ``base`` with the ``[K, n]`` fp32 client matrix (a row stride above n is fine); ``weights``,
        ``clip_norm`` and the noise stream ``(seed, offset)`` as in ``aggregate_flat``; ``out`` may be ``base``.  ``K = 1`` with
        ``weights = [1.0]`` steps towards a vector that another rule has aggregated.

        On the GPU: ``nvq_fed_delta_norms`` (only with ``clip_norm``) and one ``nvq_fed_server_opt``, nothing read back.  CPU
        tensors take the same formula in float64 torch operations."""
        check_clients(clients, base)
        if base is None:
            raise ValueError("base: the weights the round started from are required")
        K, n = clients.shape
        host = host_weights(weights, K, "ServerOptimizer.step", allow_none=False, need="sum")
        self._state(n, clients.device)
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=clients.device)
        b1, b2 = self.betas
        if clients.is_cuda:
            dev = clients.device
            weights = device_weights(weights, host, dev)
            with _nvq.device_guard(dev):
                sq = None
                if clip_norm is not None:
                    sq = torch.empty(K, dtype=torch.float64, device=dev)
                    _nvq.fed_delta_norms(clients, n, base, sq, _engine.workspace(dev))
                _nvq.fed_server_opt(clients, n, base, weights, sq, _RULES[self.rule], self.m, self.v, out,
                                    clip_norm=clip_norm or 0.0, server_lr=self.lr, beta1=b1, beta2=b2, tau=self.tau,
                                    noise_std=noise_std, seed=seed, offset=offset)
            return out
        b1, b2, tau, lr = _f32(b1), _f32(b2), _f32(self.tau), _f32(self.lr)
        w = torch.as_tensor(host if host is not None else weights, dtype=torch.float64)
        b = base.double().view(1, n)
        d = clients.double() - b
        c = w / w.sum()
        if clip_norm is not None:
            c = c * torch.clamp(_f32(clip_norm) / (d.pow(2).sum(1).sqrt() + 1e-6), max=1.0)
        D = (c.view(K, 1) * d).sum(0)
        mp = self.m.double()
        if not self.adaptive:
            m1 = b1 * mp + D
            stepv = m1
        else:
            m1 = b1 * mp + (1.0 - b1) * D
            vp, d2 = self.v.double(), D * D
            if self.rule == "fedadagrad":
                v1 = vp + d2
            elif self.rule == "fedadam":
                v1 = b2 * vp + (1.0 - b2) * d2
            else:
                v1 = vp - (1.0 - b2) * d2 * torch.sign(vp - d2)
            stepv = m1 / (v1.sqrt() + tau)
            self.v.copy_(v1.to(torch.float32))
        res = b[0] + lr * stepv                        # before m changes: out may be base, never m
        self.m.copy_(m1.to(torch.float32))
        return finish_cpu(res, noise_std, seed, offset, out)

    def state_dict(self) -> Dict[str, object]:
        """the moments (clones, None before the first step), the rule and the hyper-parameters"""
        return {"rule": self.rule, "lr": self.lr, "betas": self.betas, "tau": self.tau,
                "m": None if self.m is None else self.m.clone(), "v": None if self.v is None else self.v.clone()}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        probe = ServerOptimizer(state["rule"], state["lr"], state["betas"], state["tau"])    # the same checks
        m, v = state["m"], state["v"]
        if m is not None and (m.dtype != torch.float32 or m.dim() != 1):
            raise ValueError("m: a flat float32 vector")
        if m is not None and probe.adaptive and (v is None or v.dtype != torch.float32 or v.shape != m.shape):
            raise ValueError("v: a float32 vector like m for an adaptive rule")
        self.rule, self.lr, self.betas, self.tau = probe.rule, probe.lr, probe.betas, probe.tau
        self.m = None if m is None else m.clone()
        self.v = None if (m is None or v is None or not probe.adaptive) else v.clone()


def prox_grad_(grad: torch.Tensor, theta: torch.Tensor, anchor: torch.Tensor, mu: float) -> torch.Tensor:
    """``grad += mu * (theta - anchor)`` in place: the gradient of FedProx's ``mu / 2 |theta - anchor|^2``.  Flat fp32 HIP
    tensors: one ``nvq_fed_prox_grad`` (float64 arithmetic, rounded once); CPU tensors: the same in float64 torch operations.
    ``mu = 0`` touches nothing."""
    if not mu >= 0.0:
        raise ValueError(f"invalid mu: {mu}")
    if theta.shape != grad.shape or anchor.shape != grad.shape:
        raise ValueError("grad, theta and anchor have one shape")
    if mu == 0.0:
        return grad
    if grad.is_cuda:
        if grad.dim() != 1 or not all(t.dtype == torch.float32 and t.is_contiguous() for t in (grad, theta, anchor)):
            raise ValueError("prox_grad_ on the device: flat contiguous float32 tensors")
        with _nvq.device_guard(grad.device):
            _nvq.fed_prox_grad(grad, theta, anchor, mu)
        return grad
    with torch.no_grad():
        grad.copy_((grad.double() + _f32(mu) * (theta.double() - anchor.double())).to(grad.dtype))
    return grad
