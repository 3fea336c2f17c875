"""CPU: nerve_cl.drift's Kolmogorov-Smirnov route on CPU tensors (its float64 torch composition) against the reference detector's
recorded answers (tests/golden/ks_*.npz, written by tools/make_ks_fixtures.py), the refusals, the exports and the windowing of
update().

Bounds.  The statistic is h / lcm(n1, n2) with an exact integer h: bit-equal to scipy's.  A p-value is a sum of positive cell
masses, each a product of at most n1 + n2 correctly rounded ratios: 3 (n1 + n2) 2^-53 relative; with the margin for scipy's own
rounding the tests allow 8 (n1 + n2) 2^-53 relative (and 1e-300 absolute where a value underflows).  The score is one p-value
times d: the same relative bound."""
import glob
import os

import numpy as np
import pytest
import torch

import nerve_cl
from nerve_cl import drift
from nerve_cl.drift import DriftDetector, DriftResult, KSDriftDetector, ks_2samp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[len("ks_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ks_*.npz")))
EXPECTED = {"same_64v64x24", "shift_64v48x24", "ties_100v37x12", "clips_48v40x3x8x8", "window_1000v999x4", "same_1000v999x4"}


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"ks_{name}.npz"))


def _bound(f):
    return 8.0 * (len(f["ref"]) + len(f["cur"])) * 2.0 ** -53


def test_fixtures_are_the_cases_of_the_tool():
    assert set(FIXTURES) == EXPECTED
    decisions = set()
    for name in FIXTURES:
        f = _fixture(name)
        assert f["ref"].dtype == np.float32 and f["cur"].dtype == np.float32 and f["ref"].shape[1:] == f["cur"].shape[1:]
        d = int(np.prod(f["ref"].shape[1:]))
        assert f["p_values"].shape == (d,) and f["statistic"].shape == (d,)
        score, thr = float(f["score"]), float(f["threshold"])
        assert score == float(f["p_values"].min()) * d and bool(f["is_drift"]) == (score < thr)
        assert abs(score - thr) >= 0.2 * thr
        decisions.add(bool(f["is_drift"]))
    assert decisions == {True, False}
    assert float(_fixture("same_1000v999x4")["score"]) > 1.0             # Bonferroni without a clamp
    ties = _fixture("ties_100v37x12")
    zeros = np.concatenate([ties["ref"][ties["ref"] == 0], ties["cur"][ties["cur"] == 0]])
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()      # both signs of zero
    assert len(np.unique(ties["ref"])) < ties["ref"].size // 4          # heavy ties


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_ks_2samp_against_the_reference(name):
    f = _fixture(name)
    stat, p = ks_2samp(torch.from_numpy(f["ref"]), torch.from_numpy(f["cur"]))
    assert stat.dtype == torch.float64 and p.dtype == torch.float64 and stat.shape == p.shape == f["p_values"].shape
    assert np.array_equal(stat.numpy(), f["statistic"])                 # bit for bit
    err = np.abs(p.numpy() - f["p_values"])
    tol = np.maximum(_bound(f) * f["p_values"], 1e-300)
    print(f"{name}: worst p-value error / bound {np.max(err / tol):.3g}")
    assert (err <= tol).all()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_detector_against_the_reference(name):
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]), torch.from_numpy(f["cur"])
    det = KSDriftDetector(threshold=float(f["threshold"]), window_size=len(cur))
    det.set_reference(ref)
    r = det.detect(cur)
    assert isinstance(r, DriftResult) and r.method == "ks" and r.threshold == float(f["threshold"])
    want = float(f["score"])
    assert abs(r.score - want) <= _bound(f) * want
    assert r.is_drift == bool(f["is_drift"])
    assert np.array_equal(r.details["statistics"].numpy(), f["statistic"])
    assert r.details["p_values"].dtype == torch.float64 and r.score == float(r.details["p_values"].min()) * len(f["p_values"])
    score, flag = det.detect_device(cur)
    assert score.dtype == torch.float64 and flag.dtype == torch.bool and float(score) == r.score and bool(flag) == r.is_drift
    if len(cur) <= 64:                                                  # the window: a result exactly at window_size
        for row in cur[:-1]:
            assert det.update(row) is None
        r2 = det.update(cur[-1])
        assert r2.score == r.score and r2.is_drift == r.is_drift
        assert det.update(cur[0]) is None


def test_update_returns_a_result_exactly_at_window_size():
    g = torch.Generator().manual_seed(0)
    det = KSDriftDetector(window_size=5)
    det.set_reference(torch.randn(20, 3, generator=g))
    rows = torch.randn(11, 3, generator=g)
    got = [det.update(r) for r in rows]
    assert [r is not None for r in got] == [False] * 4 + [True] + [False] * 4 + [True] + [False]
    window = det._window
    assert got[4].score == det.detect(rows[:5]).score and got[9].score == det.detect(rows[5:10]).score
    assert det._window is window and window.shape == (5, 3)             # the preallocated window is reused


def test_special_values_tie_as_numpy_compares_them():
    ref = torch.tensor([[-0.0], [0.0], [float("inf")], [-float("inf")], [1.0], [1.0]])
    cur = torch.tensor([[0.0], [-0.0], [float("inf")], [1.0]])
    stat, p = ks_2samp(ref, cur)
    # right ranks (ref, cur): -inf (1, 0), 0 (3, 2), 1 (5, 3), inf (6, 4); a = 2, b = 3: |2 - 0|, |6 - 6|, |10 - 9|, |12 - 12|
    assert stat.item() == 2.0 / 12.0
    assert 0.0 < p.item() <= 1.0
    same = ks_2samp(ref, ref.flip(0))
    assert same[0].item() == 0.0 and same[1].item() == 1.0


def test_subsample_follows_the_modules_rule():
    g = torch.Generator().manual_seed(4)
    ref, cur = torch.randn(90, 5, generator=g), torch.randn(70, 5, generator=g) + 0.3
    det = KSDriftDetector(max_samples=32, generator=torch.Generator().manual_seed(9))
    twin = torch.Generator().manual_seed(9)                             # the rule restated: randperm(n)[:max_samples] per set
    ia, ib = torch.randperm(90, generator=twin)[:32], torch.randperm(70, generator=twin)[:32]
    det.set_reference(ref)
    r = det.detect(cur)
    stat, p = ks_2samp(ref[ia], cur[ib])
    assert torch.equal(r.details["p_values"], p) and torch.equal(r.details["statistics"], stat)


def test_refusals():
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="max_samples"):
            KSDriftDetector(max_samples=bad)
    with pytest.raises(ValueError, match="window_size"):
        KSDriftDetector(window_size=0)
    det = KSDriftDetector()
    with pytest.raises(ValueError, match="Reference data not set"):
        det.detect(torch.zeros(4, 3))
    det.set_reference(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="features"):
        det.detect(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="features"):
        ks_2samp(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(ValueError, match="at most 4096"):
        ks_2samp(torch.zeros(4097, 1), torch.zeros(4, 1))
    with pytest.raises(ValueError, match="non-empty"):
        ks_2samp(torch.zeros(0, 3), torch.zeros(4, 3))


def test_the_old_entry_point_still_refuses():
    with pytest.raises(NotImplementedError, match="scipy"):
        DriftDetector(method="ks")


def test_exports_and_no_scipy():
    assert {"ks_2samp", "KSDriftDetector"} <= set(nerve_cl.__all__) and {"ks_2samp", "KSDriftDetector"} <= set(drift.__all__)
    assert nerve_cl.ks_2samp is ks_2samp and nerve_cl.KSDriftDetector is KSDriftDetector
    src = open(drift.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src
