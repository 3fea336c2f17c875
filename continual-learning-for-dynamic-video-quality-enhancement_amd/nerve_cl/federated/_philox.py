"""Host form of the noise stream of csrc/federated.hip: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
1, 2, 3", SC 2011; the Random123 constants) and the Box-Muller normals the kernels form from it, in numpy.

``normals(seed, offset, n)[i]`` is the z_i of include/nvq.h: key = (seed low, seed high), counter = (q low, q high, offset low,
offset high) with q = i >> 2, u_j = ((r_j >> 8) + 0.5) 2^-24, elements 4q .. 4q + 3 = sqrt(-2 ln u0) cos(2 pi u1),
sqrt(-2 ln u0) sin(2 pi u1) and the same from (u2, u3).  Everything after the integer rounds is float64 here; the kernels use
fp32 ``logf`` / ``sincospif`` and agree to about 1e-6."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter: np.ndarray, key: np.ndarray) -> np.ndarray:
    """counter (..., 4), key (..., 2) of 32-bit words (any integer type) -> (..., 4) uint32"""
    c = np.asarray(counter).astype(np.uint64) & _MASK
    k = np.asarray(key).astype(np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed: int, offset: int, first_quad: int, quads: int) -> np.ndarray:
    """(quads, 4) uint32: the Philox output of quads first_quad .. first_quad + quads - 1"""
    if seed < 0 or offset < 0 or first_quad < 0:
        raise ValueError("seed, offset and the quad index are non-negative")
    q = np.arange(first_quad, first_quad + quads, dtype=np.uint64)
    ctr = np.stack([q & _MASK, q >> np.uint64(32), np.full_like(q, offset & 0xFFFFFFFF), np.full_like(q, (offset >> 32) & 0xFFFFFFFF)],
                   axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (quads, 2)))


def normals(seed: int, offset: int, n: int, first: int = 0) -> np.ndarray:
    """float64 z_first .. z_(first + n - 1) of the stream (seed, offset)"""
    if n <= 0:
        return np.zeros(0, dtype=np.float64)
    q0, q1 = first >> 2, (first + n + 3) >> 2
    r = words(seed, offset, q0, q1 - q0)
    u = ((r >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    m0, m1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([m0 * np.cos(a0), m0 * np.sin(a0), m1 * np.cos(a1), m1 * np.sin(a1)], axis=-1).reshape(-1)
    lo = first - 4 * q0
    return z[lo:lo + n]
