"""GPU: the kernels of csrc/ks.hip behind nerve_cl.drift.ks_2samp and KSDriftDetector.

Yardsticks are np.sort, the integer rank formula and the lattice walk restated here in numpy, an exact path count in
fractions.Fraction, and the reference detector's recorded answers (tests/golden/ks_*.npz); never nerve_cl code.

Bounds.  Sorted values and the integer h must agree exactly, and D must be the double h / lcm(n1, n2) bit for bit.  A p-value
is a sum of positive cell masses, each a product of at most n1 + n2 correctly rounded ratios: 3 (n1 + n2) 2^-53 relative; with
the margin for the yardstick's own rounding the tests allow 8 (n1 + n2) 2^-53 relative, with an absolute floor of 1e-300 where
a value underflows.  A score is one p-value times d: the same relative bound."""
import glob
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = ["clips_48v40x3x8x8", "same_1000v999x4", "same_64v64x24", "shift_64v48x24", "ties_100v37x12", "window_1000v999x4"]
SENTINEL = -12345.0
_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"ks_{name}.npz"))


def _sizes(n1, n2):
    g = math.gcd(n1, n2)
    return n2 // g, n1 // g, n1 // g * n2                               # a, b, lcm


def _bound(n1, n2):
    return 8.0 * (n1 + n2) * 2.0 ** -53


def _bits(t):
    return t.detach().clone().view(torch.int64)


def test_fixture_list_is_complete():
    assert sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN, "ks_*.npz"))) == FIXTURES


# ------------------------------------------------------------------------------------------------- sort

def _sort_inputs(n, d):
    """name -> (x (rows, d) fp32, row indices or None)"""
    rng = np.random.default_rng(100 * n + d)
    rnd = rng.standard_normal((n, d)).astype(np.float32)
    special = rnd.copy()
    special.ravel()[rng.permutation(n * d)[: max(n * d // 3, 1)]] = rng.choice(
        np.array([0.0, -0.0, np.inf, -np.inf], dtype=np.float32), size=max(n * d // 3, 1))
    if n * d >= 2:
        special.ravel()[:2] = [-0.0, 0.0]
    rows = n + 1 + n // 2
    big = rng.standard_normal((rows, d)).astype(np.float32)
    return {
        "random": (rnd, None),
        "ascending": (np.sort(rnd, axis=0), None),
        "descending": (np.sort(rnd, axis=0)[::-1].copy(), None),
        "equal": (np.full((n, d), 1.5, dtype=np.float32), None),
        "duplicates": (rng.integers(-3, 4, size=(n, d)).astype(np.float32), None),
        "zeros_infs": (special, None),
        "gathered": (big, rng.permutation(rows)[:n].astype(np.int32)),
    }


@pytest.mark.parametrize("d", [1, 5, 33])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 257, 1000, 4096])
def test_sort_columns_equals_np_sort(n, d):
    from nerve_cl import _nvq
    guard = 64
    for kind, (x_np, idx_np) in _sort_inputs(n, d).items():
        x = torch.from_numpy(x_np).to(_dev())
        idx = None if idx_np is None else torch.from_numpy(idx_np).to(_dev())
        buf = torch.full((d * n + guard,), SENTINEL, dtype=torch.float32, device=_dev())
        _nvq.sort_columns(x, idx, buf[: d * n].view(d, n))
        got = buf.cpu().numpy()
        used = x_np if idx_np is None else x_np[idx_np]
        want = np.sort(used, axis=0).T                                  # (d, n)
        out = got[: d * n].reshape(d, n)
        assert np.array_equal(out, want), (kind, n, d)                  # ==: -0.0 equals +0.0, inf equals inf
        assert not np.signbit(out[out == 0]).any(), kind                # -0.0 canonicalised
        assert (got[d * n:] == SENTINEL).all(), kind                    # exactly n values per feature, no padding written
        assert np.isinf(out).sum() == np.isinf(used).sum(), kind


# ------------------------------------------------------------------------------------------------- statistic

STAT_SHAPES = [(1, 1, 1), (5, 7, 3), (16, 16, 4), (17, 33, 5), (64, 48, 33), (100, 37, 7), (257, 255, 2), (1000, 999, 3),
               (4096, 4095, 1), (4096, 1000, 2)]


def np_h(rs, cs):
    """(d,) int64 from ascending (d, n1), (d, n2): max |a #{ref <= v} - b #{cur <= v}| over every value of either sample"""
    a, b, _ = _sizes(rs.shape[1], cs.shape[1])
    out = []
    for r, c in zip(rs.astype(np.float64), cs.astype(np.float64)):
        both = np.concatenate([r, c])
        c1 = np.searchsorted(r, both, side="right").astype(np.int64)
        c2 = np.searchsorted(c, both, side="right").astype(np.int64)
        out.append(int(np.abs(a * c1 - b * c2).max()))
    return np.array(out, dtype=np.int64)


def _stat_inputs(n1, n2, d):
    rng = np.random.default_rng(7 * n1 + 3 * n2 + d)
    g = math.gcd(n1, n2)
    base = rng.standard_normal((d, g)).astype(np.float32)
    ref = rng.standard_normal((d, n1)).astype(np.float32)
    return {
        "random": (ref, (rng.standard_normal((d, n2)) + 0.3).astype(np.float32)),
        "ties": ((np.round(rng.standard_normal((d, n1)) * 2) / 2).astype(np.float32),
                 (np.round(rng.standard_normal((d, n2)) * 2 + 0.6) / 2).astype(np.float32)),
        "identical": (np.repeat(base, n1 // g, axis=1), np.repeat(base, n2 // g, axis=1)),      # the same distribution function
        "disjoint": (ref, (ref.max(axis=1, keepdims=True) + 1.0 + np.abs(rng.standard_normal((d, n2)))).astype(np.float32)),
    }


def _statistic(rs_np, cs_np):
    from nerve_cl import _nvq
    d = rs_np.shape[0]
    h = torch.full((d,), -7, dtype=torch.int32, device=_dev())
    stat = torch.full((d,), float("nan"), dtype=torch.float64, device=_dev())
    _nvq.ks_statistic(torch.from_numpy(rs_np).to(_dev()), torch.from_numpy(cs_np).to(_dev()), h, stat)
    return h.cpu().numpy(), stat.cpu().numpy()


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_statistic_is_the_exact_integer(shape):
    n1, n2, d = shape
    _, _, lcm = _sizes(n1, n2)
    for kind, (r, c) in _stat_inputs(n1, n2, d).items():
        rs, cs = np.ascontiguousarray(np.sort(r, axis=1)), np.ascontiguousarray(np.sort(c, axis=1))
        h, stat = _statistic(rs, cs)
        want = np_h(rs, cs)
        assert np.array_equal(h, want), (kind, shape)
        assert np.array_equal(stat, want.astype(np.float64) / float(lcm)), (kind, shape)       # one division: bit for bit
        if kind == "identical":
            assert (h == 0).all()
        if kind == "disjoint":
            assert (h == lcm).all() and (stat == 1.0).all()


# ------------------------------------------------------------------------------------------------- p-value

def exact_p(h, n1, n2):
    """P(max |a x - b y| >= h over a uniformly drawn lattice path (0, 0) -> (n1, n2)) as a Fraction: paths that stay strictly
    inside the band, counted in integers, against all C(n1 + n2, n1)"""
    a, b, _ = _sizes(n1, n2)
    paths = [[0] * (n2 + 1) for _ in range(n1 + 1)]
    for x in range(n1 + 1):
        for y in range(n2 + 1):
            if abs(a * x - b * y) >= h:
                continue
            paths[x][y] = 1 if x == y == 0 else (paths[x - 1][y] if x else 0) + (paths[x][y - 1] if y else 0)
    return Fraction(math.comb(n1 + n2, n1) - paths[n1][n2], math.comb(n1 + n2, n1))


def np_walk(h, n1, n2):
    """the recurrence of the issue in float64 numpy, every x of an anti-diagonal at once (no band bookkeeping)"""
    if h <= 0:
        return 1.0
    a, b, _ = _sizes(n1, n2)
    x = np.arange(n1 + 1, dtype=np.int64)
    mass = np.zeros(n1 + 1)
    mass[0] = 1.0
    p = 0.0
    for s in range(1, n1 + n2 + 1):
        y_prev = s - 1 - x                                              # the cell (x, y - 1) a draw from the second sample leaves
        new = mass * np.clip(n2 - y_prev, 0, n2)
        new[1:] += mass[:-1] * (n1 - x[:-1])
        new /= float(n1 + n2 - (s - 1))
        out = np.abs(a * x - b * (s - x)) >= h
        p += new[out].sum()
        new[out] = 0.0
        mass = new
    return min(p, 1.0)


def _pvalues(hs, n1, n2):
    from nerve_cl import _nvq
    h = torch.tensor(list(hs), dtype=torch.int32, device=_dev())
    p = torch.full((h.numel(),), float("nan"), dtype=torch.float64, device=_dev())
    _nvq.ks_pvalue(h, n1, n2, p)
    again = torch.full_like(p, float("nan"))
    _nvq.ks_pvalue(h, n1, n2, again)
    assert torch.equal(_bits(p), _bits(again))                          # a function of (n1, n2, h): the same bits
    return p.cpu().numpy()


def _assert_p(got, want, n1, n2, what):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    tol = np.maximum(_bound(n1, n2) * want, 1e-300)
    print(f"{what}: worst error / bound {np.max(err / tol):.3g}")
    assert (err <= tol).all(), (what, got[err > tol], want[err > tol])


@pytest.mark.parametrize("n1,n2", [(5, 7), (6, 4), (8, 8), (9, 12)])
def test_pvalue_of_every_h_against_exact_rationals(n1, n2):
    _, _, lcm = _sizes(n1, n2)
    hs = range(0, lcm + 1)
    exact = [exact_p(h, n1, n2) for h in hs]
    assert exact[0] == 1 and exact[-1] == Fraction(2, math.comb(n1 + n2, n1))   # D = 1: all of one sample first, two paths
    got = _pvalues(hs, n1, n2)
    assert got[0] == 1.0
    _assert_p(got, [float(e) for e in exact], n1, n2, f"p-values {n1} v {n2}")
    walk = np.array([np_walk(h, n1, n2) for h in hs])                   # the numpy yardstick of the larger sizes, checked here
    _assert_p(walk, [float(e) for e in exact], n1, n2, f"numpy walk {n1} v {n2}")


def _path_hs(n1, n2):
    """h on both sides of the single-wave threshold (2 ceil(h / (a + b)) + 1 <= 64), small, wide and the largest; four of them
    where the numpy walk of one h takes most of a second"""
    a, b, lcm = _sizes(n1, n2)
    A = a + b
    hs = (A, 31 * A, 31 * A + 1, lcm) if n1 + n2 > 4000 else (1, A, 3 * A + 1, 31 * A, 31 * A + 1, 40 * A, lcm // 3, lcm - 1, lcm)
    return sorted({h for h in hs if 1 <= h <= lcm})


@pytest.mark.parametrize("n1,n2", [(100, 37), (257, 255), (1000, 999), (1000, 1000), (1024, 37), (1025, 37), (4096, 1000),
                                   (4096, 4095)])
def test_pvalue_against_the_numpy_walk(n1, n2):
    key = (n1, n2)
    if key not in _cache:
        hs = _path_hs(n1, n2)
        _cache[key] = (hs, [np_walk(h, n1, n2) for h in hs])
    hs, want = _cache[key]
    _assert_p(_pvalues(hs, n1, n2), want, n1, n2, f"p-values {n1} v {n2} at h = {hs}")


@pytest.mark.parametrize("name", FIXTURES)
def test_pvalues_and_statistics_of_the_fixtures(name):
    from nerve_cl import drift
    f = _fixture(name)
    n1, n2 = len(f["ref"]), len(f["cur"])
    _, _, lcm = _sizes(n1, n2)
    h = np.rint(f["statistic"] * lcm).astype(np.int64)
    assert np.array_equal(h.astype(np.float64) / float(lcm), f["statistic"])
    _assert_p(_pvalues(h.tolist(), n1, n2), f["p_values"], n1, n2, f"{name}: p-values from the recorded statistics")
    stat, p = drift.ks_2samp(torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev()))
    assert stat.is_cuda and p.is_cuda and stat.dtype == torch.float64 and p.dtype == torch.float64
    assert np.array_equal(stat.cpu().numpy(), f["statistic"])           # bit for bit
    _assert_p(p.cpu().numpy(), f["p_values"], n1, n2, f"{name}: ks_2samp")


# ------------------------------------------------------------------------------------------------- detector

@pytest.mark.parametrize("name", FIXTURES)
def test_detector_against_the_reference(name):
    from nerve_cl.drift import DriftResult, KSDriftDetector
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev())
    det = KSDriftDetector(threshold=float(f["threshold"]), window_size=len(f["cur"]))
    det.set_reference(ref)
    assert det.reference_data.is_cuda
    r = det.detect(cur)
    want = float(f["score"])
    assert isinstance(r, DriftResult) and r.method == "ks" and r.threshold == float(f["threshold"])
    print(f"{name}: score {r.score:.17g} reference {want:.17g}")
    assert abs(r.score - want) <= _bound(len(f["ref"]), len(f["cur"])) * want
    assert r.is_drift == bool(f["is_drift"])
    p, stat = r.details["p_values"], r.details["statistics"]
    assert p.is_cuda and stat.is_cuda and p.dtype == torch.float64 and p.shape == f["p_values"].shape
    assert np.array_equal(stat.cpu().numpy(), f["statistic"])
    score, flag = det.detect_device(cur)
    assert score.is_cuda and flag.is_cuda and score.dtype == torch.float64 and flag.dtype == torch.bool and score.dim() == 0
    assert score.item() == r.score and bool(flag.item()) == r.is_drift
    again = det.detect(cur)
    assert torch.equal(_bits(again.details["p_values"]), _bits(p)) and again.score == r.score          # equal bits
    if len(f["cur"]) <= 64:
        for row in cur[:-1]:
            assert det.update(row) is None
        r2 = det.update(cur[-1])
        assert r2.score == r.score and r2.is_drift == r.is_drift       # the window holds the same rows
        assert det._window.is_cuda and det.update(cur[0]) is None


def test_threshold_is_compared_in_double():
    from nerve_cl import _nvq
    p = torch.tensor([0.5, 0.125, 0.25], dtype=torch.float64, device=_dev())
    score = torch.zeros((), dtype=torch.float64, device=_dev())
    flag = torch.zeros((), dtype=torch.bool, device=_dev())
    for thr, want in ((0.375, False), (np.nextafter(0.375, 1.0), True), (0.3750000001, True), (1e-300, False)):
        _nvq.ks_finish(p, float(thr), score, flag)
        assert score.item() == 0.375 and bool(flag.item()) == want, thr


def test_max_samples_draws_rows_on_the_device():
    from nerve_cl.drift import KSDriftDetector, ks_2samp
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.standard_normal((2000, 6)).astype(np.float32)).to(_dev())
    b = torch.from_numpy((rng.standard_normal((2000, 6)) + 0.1).astype(np.float32)).to(_dev())
    det = KSDriftDetector(max_samples=512, generator=torch.Generator(device=_dev()).manual_seed(3))
    twin = torch.Generator(device=_dev()).manual_seed(3)                # the rule restated: randperm(n)[:max_samples] per set
    ia = torch.randperm(2000, generator=twin, device=_dev())[:512]
    ib = torch.randperm(2000, generator=twin, device=_dev())[:512]
    det.set_reference(a)
    assert det._ref_sorted.shape == (6, 512)
    r = det.detect(b)
    stat, p = ks_2samp(a[ia], b[ib])
    assert torch.equal(_bits(r.details["p_values"]), _bits(p)) and torch.equal(_bits(r.details["statistics"]), _bits(stat))
    assert r.score == p.min().item() * 6


def test_detect_device_does_not_synchronise():
    from nerve_cl.drift import KSDriftDetector
    f = _fixture("shift_64v48x24")
    ref, cur = torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev())
    det = KSDriftDetector()
    det.set_reference(ref)
    det.detect_device(cur)                                              # warm-up: code objects loaded
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = det.detect_device(cur)
        try:
            out[0].item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if not control_raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this PyTorch build: the check would be vacuous")
    assert bool(out[1].item()) == bool(f["is_drift"])


# ------------------------------------------------------------------------------------------------- refusals

def test_entry_points_refuse_before_any_launch():
    from nerve_cl import _nvq
    lib, ptr, st = _nvq.lib(), _nvq.ptr, _nvq.stream()
    x = torch.zeros(8, 3, device=_dev())
    cols = torch.full((3, 8), SENTINEL, device=_dev())
    h = torch.full((3,), -7, dtype=torch.int32, device=_dev())
    v = torch.full((3,), SENTINEL, dtype=torch.float64, device=_dev())
    flag = torch.zeros((), dtype=torch.bool, device=_dev())
    import ctypes
    thr = ctypes.byref(ctypes.c_double(0.05))
    calls = [
        lib.nvq_sort_columns(ptr(x), None, 4097, 8, 3, ptr(cols), st),
        lib.nvq_sort_columns(ptr(x), None, 0, 8, 3, ptr(cols), st),
        lib.nvq_sort_columns(ptr(x), None, 8, 8, 0, ptr(cols), st),
        lib.nvq_sort_columns(None, None, 8, 8, 3, ptr(cols), st),
        lib.nvq_sort_columns(ptr(x), None, 8, 8, 3, None, st),
        lib.nvq_sort_columns(ptr(x), None, 9, 8, 3, ptr(cols), st),       # more rows than the matrix has, no index
        lib.nvq_ks_statistic(ptr(cols), ptr(cols), 4097, 8, 3, ptr(h), ptr(v), st),
        lib.nvq_ks_statistic(ptr(cols), ptr(cols), 8, 0, 3, ptr(h), ptr(v), st),
        lib.nvq_ks_statistic(ptr(cols), ptr(cols), 8, 8, 0, ptr(h), ptr(v), st),
        lib.nvq_ks_statistic(None, ptr(cols), 8, 8, 3, ptr(h), ptr(v), st),
        lib.nvq_ks_statistic(ptr(cols), ptr(cols), 8, 8, 3, None, ptr(v), st),
        lib.nvq_ks_pvalue(ptr(h), 4097, 8, 3, ptr(v), st),
        lib.nvq_ks_pvalue(ptr(h), 8, 0, 3, ptr(v), st),
        lib.nvq_ks_pvalue(ptr(h), 8, 8, 0, ptr(v), st),
        lib.nvq_ks_pvalue(None, 8, 8, 3, ptr(v), st),
        lib.nvq_ks_pvalue(ptr(h), 8, 8, 3, None, st),
        lib.nvq_ks_finish(ptr(v), 0, thr, ptr(v), ptr(flag), st),
        lib.nvq_ks_finish(None, 3, thr, ptr(v), ptr(flag), st),
        lib.nvq_ks_finish(ptr(v), 3, None, ptr(v), ptr(flag), st),
        lib.nvq_ks_finish(ptr(v), 3, thr, None, ptr(flag), st),
    ]
    assert all(rc == calls[0] and rc != 0 for rc in calls), calls       # the library's one error code for bad arguments
    torch.cuda.synchronize()
    assert (cols == SENTINEL).all() and (h == -7).all() and (v == SENTINEL).all()              # nothing ran
    with pytest.raises(RuntimeError, match="sort_columns"):
        _nvq.sort_columns(torch.zeros(4097, 1, device=_dev()), None, torch.zeros(1, 4097, device=_dev()))
