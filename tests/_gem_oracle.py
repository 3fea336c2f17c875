"""The float64 oracle of the GEM tests: the exact optimum of

    min 1/2 v'Pv + q'v   subject to   v >= margin,      P symmetric positive definite,

by enumeration of the active sets, independent of the package's solvers.  With u = v - margin and c = q + margin P 1 a subset F
of free indices is the answer when the solution of P_FF u_F = -c_F is positive and w = P u + c is non-negative on the bound
set; P is positive definite, so exactly one subset passes (up to rounding on degenerate inputs, which the cases here are not).
All subsets of one size are solved in one batched call: 2^15 subsets take well under a second.  ``kkt_residuals`` certifies
an answer without reference to how it was found; the tests call it on the oracle's own answer before they use it.

Also here: the inputs the CPU and the GPU tests share (``CASES``), so both see the same rows."""
import itertools

import numpy as np

EPS_F32 = float(np.float32(1e-3))      # the ridge travels through the C ABI as a float
TOL = 1e-9


def ridge_of(RR, eps=EPS_F32, eps_relative=False):
    return eps * float(np.diag(RR).max()) if eps_relative else eps


def solve_enumerate(P, q, margin):
    """-> (v, free index list) of the exact optimum"""
    P, q = np.asarray(P, np.float64), np.asarray(q, np.float64)
    T = q.shape[0]
    c = q + margin * P.sum(axis=1)
    scale = np.abs(c).max() + 1e-300
    best = None
    for k in range(T + 1):
        combos = list(itertools.combinations(range(T), k))
        subsets = np.array(combos, dtype=np.int64).reshape(len(combos), k)
        u = np.zeros((subsets.shape[0], T))
        if k:
            A = P[subsets[:, :, None], subsets[:, None, :]]
            uf = np.linalg.solve(A, -c[subsets][:, :, None])[:, :, 0]
            np.put_along_axis(u, subsets, uf, axis=1)
            ok = (uf > 0).all(axis=1)
        else:
            ok = np.ones(1, dtype=bool)
        w = u @ P + c
        bound = np.ones((subsets.shape[0], T), dtype=bool)
        if k:
            np.put_along_axis(bound, subsets, False, axis=1)
        ok &= (np.where(bound, w, 0.0) >= -1e-12 * scale).all(axis=1)
        for i in np.flatnonzero(ok):
            obj = 0.5 * u[i] @ P @ u[i] + c @ u[i]
            if best is None or obj < best[0]:
                best = (obj, u[i].copy(), [int(j) for j in subsets[i]])
    assert best is not None, "no active set passed: P is not positive definite?"
    return best[1] + margin, best[2]


def kkt_residuals(P, q, margin, v):
    """(primal, dual, complementarity) violations relative to the problem's scale: all ~1e-16 at the optimum"""
    P, q, v = np.asarray(P, np.float64), np.asarray(q, np.float64), np.asarray(v, np.float64)
    w = P @ v + q
    scale = np.abs(q).max() + np.abs(P).max() * max(np.abs(v).max(), 1.0)
    vs = max(np.abs(v).max(), 1.0)
    return (max(0.0, float((margin - v).max())) / vs, max(0.0, float((-w).max())) / scale,
            float(np.abs((v - margin) * w).max()) / (scale * vs))


def certified(P, q, margin):
    v, free = solve_enumerate(P, q, margin)
    assert max(kkt_residuals(P, q, margin, v)) <= TOL, kkt_residuals(P, q, margin, v)
    return v, free


def gram_of(rows, g):
    """16 x 16 float64 Gram matrix of the fp32 rows and g (index T), as nvq_gem_gram defines it"""
    A = np.concatenate([np.asarray(rows, np.float64), np.asarray(g, np.float64)[None]], axis=0)
    G = np.zeros((16, 16))
    G[:A.shape[0], :A.shape[0]] = A @ A.T
    return G


def expected_stats(G, T, margin, v):
    """float64 values of the stats slots 0, 1, 5, 6, 7 for multipliers v"""
    RR, q, gg = G[:T, :T], G[:T, T], G[T, T]
    den = np.sqrt(gg * np.diag(RR))
    return {0: float((q < 0).sum()), 1: float((v[:T] > margin + 1e-9 * max(1.0, np.abs(v).max())).sum()), 5: gg,
            6: gg + 2 * v[:T] @ q + v[:T] @ RR @ v[:T], 7: float((q / den).min())}


def _rows(kind, T, n, seed):
    """Rows of norm about 1 and a gradient of norm about 6, so that margin = 0.5 neither dominates nor vanishes."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    noise = rng.standard_normal((T, n)).astype(np.float32)
    if kind == "random":
        R = noise
        if not ((R.astype(np.float64) @ g.astype(np.float64)) < 0).any():
            R[0] = -R[0]
    elif kind == "conflict":                       # conflicts of graded strength, the last rows agree
        a = np.linspace(1.5, -0.25, T).astype(np.float32)[:, None]
        R = -a * g[None] + np.float32(0.8) * noise
    elif kind == "common":                         # rows of graded length that share one component: P = rank one + diagonal
        common = rng.standard_normal(n).astype(np.float32)
        s = np.linspace(0.6, 1.4, T).astype(np.float32)[:, None]
        R = s * (np.float32(1.25) * common[None] + noise)
        w = np.cos(2.5 * np.arange(T)).astype(np.float32)[:, None]
        g = -common + np.float32(0.5) * g + (w * noise).sum(0)
    elif kind == "agree":
        R = g[None] + np.float32(0.3) * noise
    else:
        raise KeyError(kind)
    sc = np.float32(1.0 / np.sqrt(n))
    return np.ascontiguousarray((R * sc).astype(np.float32)), (g * sc * np.float32(6.0)).astype(np.float32)


# per T: seeds of random_problem; at T >= 3 the later ones make the method bind a multiplier it had freed (found by search)
RANDOM_SEEDS = {1: (0, 1), 3: (0, 9, 23), 6: (0, 15, 20), 15: (0, 7, 25)}


def random_problem(T, seed):
    """A 16 x 16 Gram matrix made on the host directly (a random positive definite R R' of condition ~50, a random q with both
    signs): problems on which the active-set method also has to bind multipliers it had freed."""
    rng = np.random.default_rng(1000 * T + seed)
    A = rng.standard_normal((T, T))
    Q, _ = np.linalg.qr(A)
    RR = (Q * np.geomspace(1.0, 50.0, T)) @ Q.T
    RR = 0.5 * (RR + RR.T)
    q = rng.standard_normal(T) * 3.0
    q[0] = -abs(q[0]) - 0.1
    G = np.zeros((16, 16))
    G[:T, :T], G[:T, T], G[T, :T] = RR, q, q
    G[T, T] = float(q @ np.linalg.solve(RR, q)) + 1.0          # g.g >= q' (RR')^-1 q: a Gram matrix of real vectors
    return G


# name -> (kind, T, n, seed): the six cases of the issue
CASES = {
    "random_T1": ("random", 1, 1025, 1),
    "random_T3": ("random", 3, 1025, 2),
    "conflict_T6": ("conflict", 6, 1025, 3),
    "conflict_T15": ("conflict", 15, 1025, 4),
    "common_T15": ("common", 15, 4099, 5),
    "agree_T8": ("agree", 8, 1025, 6),
}
MARGINS = (0.5, 0.0)


def case(name):
    """-> (R [T][n] fp32, g [n] fp32)"""
    return _rows(*CASES[name])
