"""float64 numpy oracle of csrc/fedopt.hip and nerve_cl.federated.fedopt: the FedOpt server rules and the
FedProx gradient, from the fp32 inputs as stored.  A round is teacher-forced: the previous ``m`` and ``v`` are what the code under
test left, so its errors never compound.  The library takes its hyper-parameters as fp32 values; ``f32`` rounds them the same way.

The kernel rounds one double chain to fp32 once per stored value; this oracle differs from it by double rounding and by the
fmas the kernel contracts (~1e-16 relative), so every value is asserted within ONE fp32 ulp of the float64 value (``within_ulps``,
the criterion of tests/test_federated_gpu.py)."""
from fractions import Fraction

import numpy as np
import torch

RULES = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")


def f32(x):
    return float(np.float32(x))


def np64(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def within_ulps(got, want, ulps=1):
    """tests/test_federated_gpu.py's _within_ulps for a tensor ``got`` and a float64 numpy ``want``"""
    want = torch.from_numpy(np.ascontiguousarray(want))
    w32 = want.abs().to(torch.float32)
    ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
    return bool(((got.detach().cpu().double() - want).abs() <= ulps * ulp).all())


def pseudo_gradient(clients, base, weights, clip_norm=None):
    """D = sum_k c_k (x_k - base), c_k = w_k / W * min(1, clip / (|x_k - base| + 1e-6))"""
    x, b, w = np64(clients), np64(base), np64(weights)
    d = x - b[None, :]
    c = w / w.sum()
    if clip_norm is not None:
        c = c * np.minimum(f32(clip_norm) / (np.sqrt((d * d).sum(1)) + 1e-6), 1.0)
    return (c[:, None] * d).sum(0)


def server_step(rule, D, base, m, v, lr=1.0, betas=(0.9, 0.99), tau=1e-3):
    """(out, m', v') in float64 from the pseudo-gradient and the stored fp32 state; v' is None for fedavgm"""
    b, mp = np64(base), np64(m)
    lr, b1, b2, tau = f32(lr), f32(betas[0]), f32(betas[1]), f32(tau)
    if rule == "fedavgm":
        m1 = b1 * mp + D
        return b + lr * m1, m1, None
    vp, d2 = np64(v), D * D
    m1 = b1 * mp + (1.0 - b1) * D
    if rule == "fedadagrad":
        v1 = vp + d2
    elif rule == "fedadam":
        v1 = b2 * vp + (1.0 - b2) * d2
    else:
        assert rule == "fedyogi", rule
        v1 = vp - (1.0 - b2) * d2 * np.sign(vp - d2)
    return b + lr * (m1 / (np.sqrt(v1) + tau)), m1, v1


def yogi_margin(D, v):
    """min |v - D^2| / max(v, D^2): how far every element is from the discontinuity of Yogi's sign"""
    vp, d2 = np64(v), np64(D) ** 2
    return float((np.abs(vp - d2) / np.maximum(vp, d2)).min())


def initial_state(rule, n, tau=1e-3):
    """m = 0 and v = tau^2 (the paper's v_{-1} >= tau^2) as the fp32 tensors a fresh ServerOptimizer holds"""
    m = torch.zeros(n, dtype=torch.float32)
    v = None if rule == "fedavgm" else torch.full((n,), f32(tau) ** 2, dtype=torch.float32)
    return m, v


def prox_grad(grad, theta, anchor, mu, exact=False):
    """grad + mu (theta - anchor) in float64.  ``exact``: rational arithmetic rounded to float64 once, for inputs built to cancel
    (g ~ -mu d), where the float64 product's own rounding is no longer small against the result."""
    g, t, a, mu = np64(grad), np64(theta), np64(anchor), f32(mu)
    if not exact:
        return g + mu * (t - a)
    fm = Fraction(mu)
    return np.array([float(Fraction(gi) + fm * (Fraction(ti) - Fraction(ai))) for gi, ti, ai in zip(g, t, a)], dtype=np.float64)
