"""The yardstick of the federated tests, independent of the package: Philox4x32-10 written from the Random123 description with
Python integers per round (vectorised over counters with numpy uint64), the Box-Muller normals of include/nvq.h in float64, and
the float64 formulas of the aggregation and of the per-slot DP step."""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in counter]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def normals(seed, offset, n):
    """z_0 .. z_(n-1) of the stream (seed, offset) in float64"""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    zeros = np.zeros(nq, dtype=np.uint64)
    r = philox([q & _LO, q >> _S32, zeros + np.uint64(offset & 0xFFFFFFFF), zeros + np.uint64(offset >> 32)],
               (seed & 0xFFFFFFFF, seed >> 32))
    u = [((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for w in r]
    m0, m1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    z = np.stack([m0 * np.cos(2 * np.pi * u[1]), m0 * np.sin(2 * np.pi * u[1]),
                  m1 * np.cos(2 * np.pi * u[3]), m1 * np.sin(2 * np.pi * u[3])], axis=1).reshape(-1)
    return z[:n]


def aggregate(x, w, base=None, clip_norm=None, server_lr=1.0):
    """float64: base + server_lr * sum_k w_k / W * s_k * (x_k - base); x [K, n] float64"""
    x = np.asarray(x, dtype=np.float64)
    b = np.zeros(x.shape[1]) if base is None else np.asarray(base, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    d = x - b
    c = w / w.sum()
    if clip_norm is not None:
        c = c * np.minimum(1.0, clip_norm / (np.sqrt((d * d).sum(1)) + 1e-6))
    return b + server_lr * (c[:, None] * d).sum(0)


def ulp32(v):
    """the spacing of float32 at |v| (float64 array in, float64 out)"""
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def padded_layout(numels):
    offs, off = [], 0
    for k in numels:
        offs.append(off)
        off += (k + 3) // 4 * 4
    return offs, off
