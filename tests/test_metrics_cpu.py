"""CPU: nerve_cl.metrics' pure functions of the eight quality sums against the formulas written out on the arrays (float64
numpy), QualityMeter.compute from hand-made sums, and the refusal of CPU tensors wherever an image would have to be read."""
import math

import numpy as np
import pytest
import torch

from nerve_cl import metrics, ops


def sums_of(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    x, y = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    d = x - y
    return np.array([x.size, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(), np.abs(d).sum(), (d * d).sum()])


def ssim_global_direct(x: np.ndarray, y: np.ndarray, L: float = 1.0) -> float:
    """unbiased variances (n - 1), biased covariance (n): the mix of the published table"""
    x, y = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    mx, my = x.mean(), y.mean()
    vx, vy = x.var(ddof=1), y.var(ddof=1)
    cxy = ((x - mx) * (y - my)).mean()
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


@pytest.fixture
def pair():
    rng = np.random.default_rng(3)
    y = rng.random((3, 17, 23))
    x = np.clip(y + 0.05 * rng.standard_normal(y.shape), 0, 1)
    return x, y


def test_mse_mae_psnr(pair):
    x, y = pair
    s = sums_of(x, y)
    want_mse = ((x - y) ** 2).mean()
    assert metrics.mse(s).item() == pytest.approx(want_mse, rel=1e-12)
    assert metrics.mae(s).item() == pytest.approx(np.abs(x - y).mean(), rel=1e-12)
    assert metrics.psnr(s).item() == pytest.approx(20 * math.log10(1.0 / math.sqrt(want_mse)), rel=1e-12)
    assert metrics.psnr(s, data_range=255.0).item() == pytest.approx(20 * math.log10(255.0 / math.sqrt(want_mse)), rel=1e-12)
    assert metrics.mse(s).dtype == torch.float64


def test_psnr_is_infinite_at_zero_error(pair):
    x, _ = pair
    p = metrics.psnr(sums_of(x, x)).item()
    assert math.isinf(p) and p > 0
    assert metrics.mse(sums_of(x, x)).item() == 0.0


def test_ssim_global_uses_unbiased_variance_and_biased_covariance(pair):
    x, y = pair
    s = sums_of(x, y)
    got = metrics.ssim_global(s).item()
    assert got == pytest.approx(ssim_global_direct(x, y), rel=1e-9)
    # the all-biased and the all-unbiased formulas are different numbers at this n: the mix is what is computed
    xr, yr = x.ravel(), y.ravel()
    n = xr.size
    mx, my = xr.mean(), yr.mean()
    cb = ((xr - mx) * (yr - my)).mean()
    c1, c2 = 1e-4, 9e-4

    def form(vx, vy, c):
        return ((2 * mx * my + c1) * (2 * c + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))

    all_biased = form(xr.var(), yr.var(), cb)
    all_unbiased = form(xr.var(ddof=1), yr.var(ddof=1), cb * n / (n - 1))
    assert abs(got - all_biased) > 1e-6 and abs(got - all_unbiased) > 1e-6
    assert metrics.ssim_global(s, data_range=2.0).item() == pytest.approx(ssim_global_direct(x, y, 2.0), rel=1e-9)


def test_ssim_global_of_a_constant_image():
    x = np.full((3, 12, 12), 0.25)
    v = metrics.ssim_global(sums_of(x, x)).item()
    assert math.isfinite(v) and v == pytest.approx(1.0, abs=1e-9)
    y = np.full((3, 12, 12), 0.75)
    w = metrics.ssim_global(sums_of(x, y)).item()
    assert math.isfinite(w) and w == pytest.approx(ssim_global_direct(x, y), abs=1e-9)


def test_rows_and_sums_of_rows(pair):
    x, y = pair
    rows = np.stack([sums_of(x[i], y[i]) for i in range(3)])
    per = metrics.mse(rows)
    assert per.shape == (3,)
    for i in range(3):
        assert per[i].item() == pytest.approx(((x[i] - y[i]) ** 2).mean(), rel=1e-12)
    assert metrics.ssim_global(rows.sum(0)).item() == pytest.approx(ssim_global_direct(x, y), rel=1e-9)
    assert metrics.mae(torch.from_numpy(rows)).shape == (3,)
    with pytest.raises(ValueError):
        metrics.mse(np.zeros(7))


def test_quality_meter_from_hand_made_sums(pair):
    x, y = pair
    m = metrics.QualityMeter()
    m.update_sums(np.stack([sums_of(x[0], y[0]), sums_of(x[1], y[1])]))   # a batch of two
    m.update_sums(sums_of(x[2], y[2]))                                    # a batch of one
    m.all_reduce()                                                          # no process group: a no-op
    r = m.compute()
    assert set(r) == {"psnr", "ssim_global", "mae", "mse", "n"}
    assert all(isinstance(v, float) for v in r.values())
    want_mse = ((x - y) ** 2).mean()
    assert r["n"] == x.size
    assert r["mse"] == pytest.approx(want_mse, rel=1e-12)
    assert r["mae"] == pytest.approx(np.abs(x - y).mean(), rel=1e-12)
    assert r["psnr"] == pytest.approx(20 * math.log10(1 / math.sqrt(want_mse)), rel=1e-12)
    assert r["ssim_global"] == pytest.approx(ssim_global_direct(x, y), rel=1e-9)

    b = metrics.QualityMeter(averaging="batch")
    b.update_sums(np.stack([sums_of(x[0], y[0]), sums_of(x[1], y[1])]))
    b.update_sums(sums_of(x[2], y[2]))
    rb = b.compute()
    p01 = 20 * math.log10(1 / math.sqrt(((x[:2] - y[:2]) ** 2).mean()))
    p2 = 20 * math.log10(1 / math.sqrt(((x[2] - y[2]) ** 2).mean()))
    assert rb["psnr"] == pytest.approx((p01 + p2) / 2, rel=1e-12)      # the mean of per-batch PSNR, as the scripts print it
    assert rb["n"] == x.size
    with pytest.raises(RuntimeError):
        metrics.QualityMeter().compute()
    with pytest.raises(ValueError):
        metrics.QualityMeter(averaging="epoch")


@pytest.mark.parametrize("fn", [metrics.quality_sums, metrics.ssim, ops.l1_loss, ops.charbonnier_loss, ops.ssim_loss,
                                lambda a, b: ops.mse_loss(a, b, reduction="none"),
                                lambda a, b: metrics.QualityMeter().update(a, b)])
def test_cpu_tensors_are_refused(fn):
    a, b = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(a, b)


def test_reduction_names():
    a = torch.rand(2, 3, 16, 16)
    for fn in (ops.l1_loss, ops.mse_loss, ops.ssim_loss, metrics.ssim):
        with pytest.raises(ValueError, match="reduction"):
            fn(a, a, reduction="sum")
    assert set(ops.LOSSES) == {"mse", "l1", "charbonnier", "ssim"}
