"""CPU: nerve_cl.drift on CPU tensors (its float64 torch composition) against the reference detector's recorded answers
(tests/golden/drift_*.npz, written by tools/make_drift_fixtures.py) and against the formulas restated here in float64 numpy;
the windowing of update(), the refusals, ModelDriftMonitor's host route and the --drift flags of train_continual.py.

Bounds.  MMD: both sides evaluate the same float64 formula, in another summation order; the exponent's rounding error is at
most gamma (d + 3) 2^-53 (|x|^2 + |y|^2 + 2 |x.y|) per pair and |d exp| <= 1, which stays below 1e-12 for every fixture
(d <= 384, unit-variance rows with offsets up to 1), so 1e-10 absolute on a score that is a difference of three means holds
with two orders to spare.  PSI: the counts are integers and must agree exactly, which leaves the rounding of ten logarithms:
1e-12 relative."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from nerve_cl import drift
from nerve_cl.drift import DriftDetector, DriftResult, ModelDriftMonitor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[len("drift_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "drift_*.npz"))
                  if not p.endswith("drift_monitor.npz"))


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"drift_{name}.npz"))


def np_mmd(ref, cur, gamma=None):
    """the biased estimator in float64 numpy, each Gram matrix divided by its own size"""
    x = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    y = np.asarray(cur, dtype=np.float64).reshape(len(cur), -1)
    g = 1.0 / x.shape[1] if gamma is None else gamma

    def k(a, b):
        d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
        return np.exp(-g * d)
    return k(x, x).mean() + k(y, y).mean() - 2.0 * k(x, y).mean()


def np_psi(ref, cur):
    r = np.asarray(ref, dtype=np.float64).ravel()
    c = np.asarray(cur, dtype=np.float64).ravel()
    bins = np.unique(np.percentile(r, np.arange(0, 101, 10)))
    rp = np.histogram(r, bins=bins)[0] / len(r) + 1e-10
    cp = np.histogram(c, bins=bins)[0] / len(c) + 1e-10
    return np.sum((cp - rp) * np.log(cp / rp))


def test_fixtures_cover_both_decisions_with_margin():
    assert len(FIXTURES) >= 4
    seen = set()
    for name in FIXTURES:
        f = _fixture(name)
        assert f["ref"].dtype == np.float32 and f["ref"].shape == f["cur"].shape and len(f["ref"]) <= 500
        for m in ("mmd", "psi"):
            s, t = float(f[f"{m}_score"]), float(f[f"{m}_threshold"])
            assert abs(s - t) >= 0.2 * t, (name, m, s)
            assert bool(f[f"{m}_drift"]) == (s > t)
            seen.add((m, bool(f[f"{m}_drift"])))
    assert seen == {("mmd", True), ("mmd", False), ("psi", True), ("psi", False)}


@pytest.mark.parametrize("name", FIXTURES)
def test_mmd_matches_the_reference(name):
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]), torch.from_numpy(f["cur"])
    want = float(f["mmd_score"])
    got = drift.mmd_rbf(ref, cur)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - want) <= 1e-10, (got.item(), want)
    det = DriftDetector(method="mmd", threshold=0.05)
    det.set_reference(ref)
    r = det.detect(cur)
    assert isinstance(r, DriftResult) and r.method == "mmd" and r.threshold == 0.05 and r.details is None
    assert abs(r.score - want) <= 1e-10 and r.is_drift == bool(f["mmd_drift"])
    s, flag = det.detect_device(cur)
    assert s.item() == r.score and bool(flag) == r.is_drift


@pytest.mark.parametrize("name", FIXTURES)
def test_psi_matches_the_reference(name):
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]), torch.from_numpy(f["cur"])
    want = float(f["psi_score"])
    edges, counts, n = drift.psi_reference(ref)
    bins = np.unique(np.percentile(f["ref"].astype(np.float64).ravel(), np.arange(0, 101, 10)))
    assert np.array_equal(edges.numpy(), bins) and n == f["ref"].size
    assert np.array_equal(counts.numpy(), np.histogram(f["ref"].astype(np.float64).ravel(), bins=bins)[0])
    got = drift.psi(edges, counts, n, cur)
    assert got.dtype == torch.float64 and abs(got.item() - want) <= 1e-12 * abs(want), (got.item(), want)
    det = DriftDetector(method="psi")
    det.set_reference(ref)
    r = det.detect(cur)
    assert r.method == "psi" and r.threshold == 0.2 and r.is_drift == bool(f["psi_drift"])
    assert abs(r.score - want) <= 1e-12 * abs(want)


def test_histogram_rule_is_numpys():
    edges = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
    x = np.array([-1.5, -1.0, -0.25, -0.2500001, 0.0, 0.49999997, 0.5, 2.0, 2.0000002, np.nan, 1.0], dtype=np.float32)
    got = drift._histogram_cpu(torch.from_numpy(x), torch.from_numpy(edges))
    assert np.array_equal(got.numpy(), np.histogram(x.astype(np.float64), bins=edges)[0])


def test_constant_reference_has_no_bins_and_a_zero_index():
    ref = torch.full((40,), 3.0)
    edges, counts, n = drift.psi_reference(ref)
    assert edges.numel() == 1 and counts.numel() == 0 and n == 40
    assert drift.psi(edges, counts, n, torch.randn(17)).item() == 0.0 == np_psi(ref.numpy(), np.zeros(17))
    half = torch.cat([torch.zeros(60), torch.arange(40.0)])            # repeated percentiles: fewer than 11 edges
    edges, counts, n = drift.psi_reference(half)
    assert 2 <= edges.numel() < 11
    cur = torch.arange(-5.0, 45.0)
    want = np_psi(half.numpy(), cur.numpy())
    assert abs(drift.psi(edges, counts, n, cur).item() - want) <= 1e-12 * abs(want)


def test_unequal_set_sizes_divide_each_gram_sum_by_its_own_count():
    g = torch.Generator().manual_seed(3)
    ref, cur = torch.randn(37, 29, generator=g), torch.randn(21, 29, generator=g) + 0.3
    want = np_mmd(ref.numpy(), cur.numpy())
    assert abs(drift.mmd_rbf(ref, cur).item() - want) <= 1e-10
    det = DriftDetector()
    det.set_reference(ref)
    assert abs(det.detect(cur).score - want) <= 1e-10
    assert abs(drift.mmd_rbf(ref, cur, gamma=0.125).item() - np_mmd(ref.numpy(), cur.numpy(), 0.125)) <= 1e-10


def test_max_samples_subsamples_each_set_on_its_own():
    g = torch.Generator().manual_seed(4)
    ref, cur = torch.randn(30, 12, generator=g), torch.randn(9, 12, generator=g)
    # the rule restated: a set of more than max_samples rows is cut to randperm(n)[:max_samples] of the given generator, the
    # reference set first; a set of at most max_samples rows is used whole and draws nothing
    idx = torch.randperm(30, generator=torch.Generator().manual_seed(9))[:10]
    want = np_mmd(ref[idx].numpy(), cur.numpy())
    got = drift.mmd_rbf(ref, cur, max_samples=10, generator=torch.Generator().manual_seed(9))
    assert abs(got.item() - want) <= 1e-10
    det = DriftDetector(max_samples=10, generator=torch.Generator().manual_seed(9))
    det.set_reference(ref)
    first = det.detect(cur).score
    assert abs(first - want) <= 1e-10
    assert det.detect(cur).score == first                               # the reference subsample was fixed by set_reference
    both = torch.Generator().manual_seed(5)
    i = torch.randperm(30, generator=torch.Generator().manual_seed(5))
    gen2 = torch.Generator().manual_seed(5)
    ia = torch.randperm(30, generator=gen2)[:8]
    ib = torch.randperm(30, generator=gen2)[:8]
    assert torch.equal(ia, i[:8])
    want2 = np_mmd(ref[ia].numpy(), ref[ib].numpy())
    assert abs(drift.mmd_rbf(ref, ref, max_samples=8, generator=both).item() - want2) <= 1e-10


def test_update_fills_the_window_then_starts_over():
    f = _fixture("shift_clips_48x3x8x8")
    ref, cur = torch.from_numpy(f["ref"]), torch.from_numpy(f["cur"])
    det = DriftDetector(method="mmd", window_size=48)
    det.set_reference(ref)
    for i in range(47):
        assert det.update(cur[i]) is None                               # samples of shape (3, 8, 8): flattened per row
    r = det.update(cur[47])
    assert isinstance(r, DriftResult) and abs(r.score - float(f["mmd_score"])) <= 1e-10 and r.is_drift
    assert det.update(cur[0]) is None                                   # the window was reset
    for i in range(1, 47):
        assert det.update(ref[i]) is None
    r2 = det.update(ref[47])
    want = np_mmd(f["ref"], np.concatenate([f["cur"][:1], f["ref"][1:48]]))
    assert abs(r2.score - want) <= 1e-10


def test_refusals():
    with pytest.raises(ValueError, match="Reference data not set"):
        DriftDetector().detect(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="Reference data not set"):
        DriftDetector(method="psi").detect_device(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="scipy"):
        DriftDetector(method="ks")
    with pytest.raises(ValueError, match="Unknown method"):
        DriftDetector(method="chi2")
    det = DriftDetector()
    det.set_reference(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="features"):
        det.detect(torch.zeros(4, 5))
    with pytest.raises(ValueError):
        drift.frame_descriptor(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="grid"):
        drift.frame_descriptor(torch.zeros(1, 1, 4, 4), grid=(5, 2))


def test_frame_descriptor_cpu_composition():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 5, 7, generator=g)
    d = drift.frame_descriptor(x, grid=(2, 3))
    assert d.shape == (2, 2 * 3 * 2 * 3) and d.dtype == torch.float32
    xd = x.double()
    for (i, j) in ((0, 0), (1, 2)):
        h0, h1 = i * 5 // 2, -((-(i + 1) * 5) // 2)
        w0, w1 = j * 7 // 3, -((-(j + 1) * 7) // 3)
        cell = xd[1, 2, h0:h1, w0:w1]
        k = (2 * 2 + i) * 3 + j
        assert abs(d[1, k].item() - cell.mean().item()) <= 2.0 ** -23 * abs(cell.mean().item()) + 1e-9
        assert abs(d[1, 18 + k].item() - cell.std(unbiased=False).item()) <= 2.0 ** -23 * cell.std(unbiased=False).item() + 1e-6
    clip = torch.randn(2, 4, 3, 8, 8, generator=g)
    assert torch.equal(drift.frame_descriptor(clip, grid=4), drift.frame_descriptor(clip.reshape(2, 12, 8, 8), grid=(4, 4)))


def test_monitor_host_route_follows_the_reference_sequence():
    f = np.load(os.path.join(GOLDEN, "drift_monitor.npz"))
    mon = ModelDriftMonitor(metric_threshold=float(f["threshold"]), window_size=int(f["window"]))
    mon.set_baseline(float(f["baseline"]))
    got = [mon.update(float(m)) for m in f["metrics"]]
    assert got == [bool(b) for b in f["flags"]] and any(got) and not all(got)
    assert all(isinstance(b, bool) for b in got)
    assert mon.poll() is False                                          # no device update was made


def test_exports():
    import nerve_cl
    assert {"DriftDetector", "DriftResult", "ModelDriftMonitor"} <= set(nerve_cl.__all__)
    assert nerve_cl.DriftDetector is DriftDetector


def test_the_script_takes_the_drift_flags():
    sys.path.insert(0, os.path.join(REPO, "experiments"))               # (the scripts import their sibling _common.py)
    spec = importlib.util.spec_from_file_location("train_continual_for_drift", os.path.join(REPO, "experiments", "train_continual.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    d = parser.parse_args([])
    assert d.drift == "off" and d.drift_grid == 8
    a = parser.parse_args(["--drift", "psi", "--drift-grid", "4"])
    assert a.drift == "psi" and a.drift_grid == 4
    with pytest.raises(SystemExit):
        parser.parse_args(["--drift", "ks"])
    lines = []
    rep = mod.DriftReport("mmd", 4, torch.device("cpu"))
    g = torch.Generator().manual_seed(8)
    rep(0, torch.randn(16, 3, 16, 16, generator=g), lines.append)
    assert lines == []
    rep(1, torch.randn(16, 3, 16, 16, generator=g) + 0.4, lines.append)
    assert len(lines) == 1 and lines[0].startswith("drift task 0 -> 1: method=mmd score=") and lines[0].endswith("drift=True")
    mod.report_drift({"drift": None}, 1, torch.zeros(1), lines.append)
    assert len(lines) == 1
