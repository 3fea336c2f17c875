"""GPU: the kernels of csrc/drift.hip behind nerve_cl.drift, and experiments/train_continual.py --drift.

Yardsticks are the formulas written here in float64 numpy / torch, np.histogram, and the reference detector's recorded answers
(tests/golden/drift_*.npz); never nerve_cl code.

Bounds.  Gram sums: the kernel forms |x|^2 + |y|^2 - 2 x.y in float64 from exactly widened inputs; the rounding of the three
d-term sums and their combination moves the exponent by at most gamma (d + 3) 2^-53 (|x|^2 + |y|^2 + 2 |x.y|), and |d exp| <= 1.
The tests allow 8 times that bound, summed over the pairs of their own data, plus 1e-14 na nb for the final sum; an MMD is three
such sums divided by their counts, and its bound is the same combination of theirs.  Integer-valued rows make the distance an
exact integer: gamma = 0 must give na nb exactly, gamma = 1024 exactly the number of identical pairs (exp(-1024 k) is 0 in double
for k >= 1), and gamma = 2^-6 leaves only the rounding of exp itself, at most one ulp of a value <= 1 on each side and the
summation: 3 * 2^-52 per pair.  PSI: integer counts must agree exactly, the index to 1e-12 relative.  Descriptors: the sums are
float64, the result is stored as fp32: 2^-23 relative on the mean, and on the deviation with a floor of 1e-6."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[len("drift_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "drift_*.npz"))
                  if not p.endswith("drift_monitor.npz"))
SHAPES = [(1, 1, 1), (16, 16, 4), (17, 33, 5), (64, 64, 64), (65, 63, 67), (100, 37, 1031), (500, 500, 48), (40, 40, 3072)]
_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"drift_{name}.npz"))


def _data(shape):
    """(a, b) float32 numpy, and their float64 Gram sums with bounds; computed once per shape"""
    if shape not in _cache:
        na, nb, d = shape
        rng = np.random.default_rng(1000 + na + 7 * nb + 13 * d)
        a = rng.standard_normal((na, d)).astype(np.float32)
        b = (rng.standard_normal((nb, d)) + 0.25).astype(np.float32)
        g = 1.0 / d
        _cache[shape] = (a, b, {k: (np_gram(x, y, g), gram_tol(x, y, g)) for k, (x, y) in
                                (("aa", (a, a)), ("bb", (b, b)), ("ab", (a, b)))})
    return _cache[shape]


def np_gram(x, y, gamma):
    x, y = x.astype(np.float64), y.astype(np.float64)
    dist = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T
    return float(np.exp(-gamma * dist).sum())


def gram_tol(x, y, gamma):
    x, y = x.astype(np.float64), y.astype(np.float64)
    d = x.shape[1]
    mag = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] + 2.0 * np.abs(x @ y.T)
    return 8.0 * float((abs(gamma) * (d + 3) * 2.0 ** -53 * mag).sum()) + 1e-14 * x.shape[0] * y.shape[0]


def _gram(a, b, gamma=None, symmetric=False, ia=None, ib=None):
    """one nvq_rbf_gram_sum call on device tensors; returns the float64 device scalar"""
    from nerve_cl import _nvq
    na = a.shape[0] if ia is None else ia.numel()
    nb = b.shape[0] if ib is None else ib.numel()
    ws = torch.empty(max(_nvq.lib().nvq_rbf_gram_workspace_bytes(na, nb, 0) // 8, 1), dtype=torch.float64, device=_dev())
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=_dev())
    gt = None if gamma is None else torch.tensor([gamma], dtype=torch.float64, device=_dev())
    _nvq.rbf_gram_sum(a, b, out, ws, a_index=ia, b_index=ib, gamma=gt, symmetric=symmetric)
    return out


def _bits(t):
    return t.detach().clone().view(torch.int64)


# ------------------------------------------------------------------------------------------------- Gram sums, MMD

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_sum_against_float64(shape):
    a_np, b_np, want = _data(shape)
    a, b = torch.from_numpy(a_np).to(_dev()), torch.from_numpy(b_np).to(_dev())
    got = _gram(a, b)
    err = abs(got.item() - want["ab"][0])
    print(f"rbf_gram_sum {shape}: sum {want['ab'][0]:.12g} error {err:.3e} bound {want['ab'][1]:.3e}")
    assert err <= want["ab"][1]
    assert torch.equal(_bits(got), _bits(_gram(a, b)))                  # no atomics, a fixed order: the same bits
    rect = _gram(a, a)
    assert abs(rect.item() - want["aa"][0]) <= want["aa"][1]
    assert torch.equal(_bits(_gram(a, a, symmetric=True)), _bits(rect))  # upper-triangle tiles, mirrored: bit for bit
    assert torch.equal(_bits(_gram(b, b, symmetric=True)), _bits(_gram(b, b)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mmd_rbf_against_float64(shape):
    from nerve_cl import drift
    a_np, b_np, want = _data(shape)
    na, nb, _ = shape
    got = drift.mmd_rbf(torch.from_numpy(a_np).to(_dev()), torch.from_numpy(b_np).to(_dev()))
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    ref = want["aa"][0] / na ** 2 + want["bb"][0] / nb ** 2 - 2.0 * want["ab"][0] / (na * nb)
    tol = want["aa"][1] / na ** 2 + want["bb"][1] / nb ** 2 + 2.0 * want["ab"][1] / (na * nb)
    err = abs(got.item() - ref)
    print(f"mmd_rbf {shape}: mmd {ref:.12g} error {err:.3e} bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("shape", [(16, 16, 4), (17, 33, 5), (65, 63, 67)], ids=lambda s: "x".join(map(str, s)))
def test_integer_rows_are_exact(shape):
    na, nb, d = shape
    rng = np.random.default_rng(5 + na)
    a_np = rng.integers(-3, 4, size=(na, d)).astype(np.float32)
    b_np = rng.integers(-3, 4, size=(nb, d)).astype(np.float32)
    a_np[:, 0] = np.arange(na) + 10                                     # all rows of a distinct
    b_np[:, 0] = -np.arange(nb) - 10                                    # and none of them in b ...
    same = [(j, (5 * j + 2) % na) for j in range(0, nb, 3)]             # ... but these: b_j = a_i, not symmetric in (i, j)
    for j, i in same:
        b_np[j] = a_np[i]
    a, b = torch.from_numpy(a_np).to(_dev()), torch.from_numpy(b_np).to(_dev())
    assert _gram(a, b, gamma=0.0).item() == float(na * nb)
    assert _gram(a, b, gamma=1024.0).item() == float(len(same))
    assert _gram(a, a, gamma=1024.0).item() == float(na)
    dist = ((a_np.astype(np.int64)[:, None, :] - b_np.astype(np.int64)[None, :, :]) ** 2).sum(-1)      # exact integers
    want = float(np.exp(-(2.0 ** -6) * dist.astype(np.float64)).sum())
    assert abs(_gram(a, b, gamma=2.0 ** -6).item() - want) <= 3 * 2.0 ** -52 * na * nb


def test_row_indices_are_gathered_in_the_kernel():
    a_np, b_np, want = _data((65, 63, 67))
    a, b = torch.from_numpy(a_np).to(_dev()), torch.from_numpy(b_np).to(_dev())
    g = torch.Generator().manual_seed(2)
    pa, pb = torch.randperm(65, generator=g), torch.randperm(63, generator=g)
    got = _gram(a, b, ia=pa.to(_dev(), torch.int32), ib=pb.to(_dev(), torch.int32))
    assert abs(got.item() - want["ab"][0]) <= want["ab"][1]             # a permutation: the same sum in another order
    sa, sb = pa[:21], pb[:40]                                           # strict subsets, other counts than the matrices' rows
    got = _gram(a, b, ia=sa.to(_dev(), torch.int32), ib=sb.to(_dev(), torch.int32))
    xa, xb = a_np[sa.numpy()], b_np[sb.numpy()]
    assert abs(got.item() - np_gram(xa, xb, 1.0 / 67)) <= gram_tol(xa, xb, 1.0 / 67)
    idx = sa.to(_dev(), torch.int32)
    sym = _gram(a, a, ia=idx, ib=idx, symmetric=True)
    assert torch.equal(_bits(sym), _bits(_gram(a, a, ia=idx, ib=idx)))
    assert abs(sym.item() - np_gram(xa, xa, 1.0 / 67)) <= gram_tol(xa, xa, 1.0 / 67)


def test_gram_sum_refuses_bad_arguments():
    from nerve_cl import _nvq
    a = torch.zeros(4, 3, device=_dev())
    out = torch.zeros(1, dtype=torch.float64, device=_dev())
    with pytest.raises(RuntimeError, match="workspace"):
        _nvq.rbf_gram_sum(torch.zeros(130, 3, device=_dev()), a, out, torch.zeros(1, dtype=torch.float64, device=_dev()))
    with pytest.raises(RuntimeError, match="symmetric"):
        _nvq.rbf_gram_sum(a, a.clone(), out, torch.zeros(8, dtype=torch.float64, device=_dev()), symmetric=True)
    assert _nvq.lib().nvq_rbf_gram_sum(_nvq.ptr(a), _nvq.ptr(a), None, None, 0, 4, 4, 4, 3, None, 0, _nvq.ptr(out), _nvq.ptr(out), 8,
                                      _nvq.stream()) != 0


# ------------------------------------------------------------------------------------------------- PSI

EDGES = np.array([-1.5, -0.75, -0.25, 0.0, 0.125, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0])


def _psi_values(n, seed):
    """n fp32 values: every edge itself, values below the first and above the last edge, neighbours of edges, then noise"""
    rng = np.random.default_rng(seed)
    special = np.concatenate([EDGES, [-1.5000001, -7.0, 3.0000002, 9.0], np.nextafter(EDGES.astype(np.float32), np.float32(9)),
                              np.nextafter(EDGES.astype(np.float32), np.float32(-9))]).astype(np.float32)
    x = np.concatenate([special, rng.standard_normal(max(n, 0)).astype(np.float32) * 1.5])
    return rng.permutation(x)[:n] if n < len(special) else x[:n]


@pytest.mark.parametrize("n", [1, 3, 255, 257, 4099])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
def test_psi_counts_equal_np_histogram(n, offset):
    from nerve_cl import _nvq
    x_np = _psi_values(n, 40 + n)
    assert len(x_np) == n
    x = torch.from_numpy(np.concatenate([np.zeros(offset, np.float32), x_np])).to(_dev())[offset:]
    assert x.data_ptr() % 16 == 4 * offset
    for edges in (EDGES, EDGES[:2], EDGES[3:8]):
        counts = torch.full((len(edges) - 1,), -7, dtype=torch.int32, device=_dev())
        _nvq.psi_counts(x, torch.from_numpy(edges).to(_dev()), counts)
        assert np.array_equal(counts.cpu().numpy(), np.histogram(x_np.astype(np.float64), bins=edges)[0]), (n, len(edges))


def test_psi_reference_with_repeated_percentiles():
    from nerve_cl import drift
    half = np.concatenate([np.zeros(60, np.float32), np.arange(40, dtype=np.float32)])
    bins = np.unique(np.percentile(half.astype(np.float64), np.arange(0, 101, 10)))
    assert 2 <= len(bins) < 11
    edges, counts, n = drift.psi_reference(torch.from_numpy(half).to(_dev()))
    assert edges.is_cuda and np.array_equal(edges.cpu().numpy(), bins) and n == 100
    assert np.array_equal(counts.cpu().numpy(), np.histogram(half.astype(np.float64), bins=bins)[0])
    edges, counts, n = drift.psi_reference(torch.full((33,), 2.5, device=_dev()))      # constant: one edge, no bin, index 0
    assert edges.numel() == 1 and counts.numel() == 0
    score = drift.psi(edges, counts, n, torch.randn(9, device=_dev()))
    assert score.is_cuda and score.item() == 0.0


def np_psi(ref, cur):
    r, c = ref.astype(np.float64).ravel(), cur.astype(np.float64).ravel()
    bins = np.unique(np.percentile(r, np.arange(0, 101, 10)))
    rp = np.histogram(r, bins=bins)[0] / len(r) + 1e-10
    cp = np.histogram(c, bins=bins)[0] / len(c) + 1e-10
    return float(np.sum((cp - rp) * np.log(cp / rp)))


@pytest.mark.parametrize("name", FIXTURES)
def test_psi_against_the_reference_and_the_oracle(name):
    from nerve_cl import drift
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev())
    edges, counts, n = drift.psi_reference(ref)
    got = drift.psi(edges, counts, n, cur)
    assert got.is_cuda and got.dtype == torch.float64
    for want in (float(f["psi_score"]), np_psi(f["ref"], f["cur"])):
        assert abs(got.item() - want) <= 1e-12 * abs(want), (got.item(), want)
    short = f["cur"].ravel()[: f["cur"].size // 3 + 1]                   # another length than the reference's
    want = np_psi(f["ref"], short)
    assert abs(drift.psi(edges, counts, n, torch.from_numpy(short).to(_dev())).item() - want) <= 1e-12 * abs(want)


# ------------------------------------------------------------------------------------------------- descriptors

def _descriptor_oracle(x, gh, gw):
    xd = x.double().cpu()
    B, C, H, W = xd.shape
    mean = F.adaptive_avg_pool2d(xd, (gh, gw))
    std = torch.empty_like(mean)
    for i in range(gh):
        for j in range(gw):
            h0, h1 = i * H // gh, -((-(i + 1) * H) // gh)
            w0, w1 = j * W // gw, -((-(j + 1) * W) // gw)
            cell = xd[:, :, h0:h1, w0:w1]
            m = F.adaptive_avg_pool2d(cell, 1)
            assert torch.allclose(m[:, :, 0, 0], mean[:, :, i, j], rtol=1e-13, atol=1e-15)      # the bounds are torch's
            std[:, :, i, j] = F.adaptive_avg_pool2d((cell - m) ** 2, 1)[:, :, 0, 0].sqrt()
    return torch.cat([mean.flatten(1), std.flatten(1)], 1)


@pytest.mark.parametrize("shape,grid", [((2, 3, 8, 8), (8, 8)), ((1, 1, 5, 7), (2, 3)), ((3, 9, 64, 64), (8, 8)),
                                        ((2, 3, 17, 33), (4, 4)), ((2, 2, 16, 24), (3, 5))])
def test_cell_descriptor(shape, grid):
    from nerve_cl import drift
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) + 0.5
    n = x.numel()
    flat = torch.empty(n + 1, device=_dev())
    flat[1:].copy_(x.reshape(-1))
    shifted = flat[1:].view(*shape)                                     # 4 bytes past a 16-byte boundary: the scalar form
    xa = x.to(_dev())
    assert xa.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    got = drift.frame_descriptor(xa, grid=grid)
    assert got.shape == (shape[0], 2 * shape[1] * grid[0] * grid[1]) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), drift.frame_descriptor(shifted, grid=grid).view(torch.int32))
    want = _descriptor_oracle(x, *grid)
    half = want.shape[1] // 2
    err = (got.double().cpu() - want).abs()
    assert (err[:, :half] <= 2.0 ** -23 * want[:, :half].abs()).all(), (err[:, :half] / want[:, :half].abs()).max()
    assert (err[:, half:] <= torch.clamp(2.0 ** -23 * want[:, half:], min=1e-6)).all()


def test_descriptor_of_a_clip_reads_time_as_channels():
    from nerve_cl import drift
    clip = torch.randn(2, 3, 2, 12, 12, generator=torch.Generator().manual_seed(1)).to(_dev())
    assert torch.equal(drift.frame_descriptor(clip, grid=(3, 3)), drift.frame_descriptor(clip.reshape(2, 6, 12, 12), grid=(3, 3)))


# ------------------------------------------------------------------------------------------------- detector, monitor

def _mmd_tol(ref, cur):
    x = ref.reshape(len(ref), -1)
    y = cur.reshape(len(cur), -1)
    g = 1.0 / x.shape[1]
    return gram_tol(x, x, g) / len(x) ** 2 + gram_tol(y, y, g) / len(y) ** 2 + 2.0 * gram_tol(x, y, g) / (len(x) * len(y))


@pytest.mark.parametrize("name", FIXTURES)
def test_detector_against_the_reference(name):
    from nerve_cl.drift import DriftDetector, DriftResult
    f = _fixture(name)
    ref, cur = torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev())
    tol = {"mmd": _mmd_tol(f["ref"], f["cur"]), "psi": 1e-12 * abs(float(f["psi_score"]))}
    for method in ("mmd", "psi"):
        want, drifted = float(f[f"{method}_score"]), bool(f[f"{method}_drift"])
        det = DriftDetector(method=method, threshold=0.05, window_size=len(f["cur"]))
        det.set_reference(ref)
        assert det.reference_data.is_cuda
        r = det.detect(cur)
        assert isinstance(r, DriftResult) and r.method == method and r.threshold == float(f[f"{method}_threshold"])
        assert abs(r.score - want) <= tol[method], (method, r.score, want)
        assert r.is_drift == drifted
        score, flag = det.detect_device(cur)
        assert score.is_cuda and flag.is_cuda and score.dtype == torch.float64 and flag.dtype == torch.bool
        assert score.item() == r.score and bool(flag.item()) == drifted
        for row in cur[:-1]:
            assert det.update(row) is None
        r2 = det.update(cur[-1])
        assert r2.score == r.score and r2.is_drift == drifted           # the window holds the same rows in the same order
        assert det.update(cur[0]) is None


def test_detect_device_does_not_synchronise():
    from nerve_cl.drift import DriftDetector
    f = _fixture("shift_100x48")
    ref, cur = torch.from_numpy(f["ref"]).to(_dev()), torch.from_numpy(f["cur"]).to(_dev())
    dets = {m: DriftDetector(method=m) for m in ("mmd", "psi")}
    for det in dets.values():
        det.set_reference(ref)
        det.detect_device(cur)                                          # warm-up: code objects loaded, workspace allocated
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = {m: det.detect_device(cur) for m, det in dets.items()}
        try:
            out["mmd"][0].item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if not control_raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this PyTorch build: the check would be vacuous")
    assert bool(out["mmd"][1].item()) == bool(f["mmd_drift"]) and bool(out["psi"][1].item()) == bool(f["psi_drift"])


def test_max_samples_draws_rows_on_the_device():
    from nerve_cl.drift import DriftDetector
    a_np, b_np, _ = _data((65, 63, 67))
    a, b = torch.from_numpy(a_np).to(_dev()), torch.from_numpy(b_np).to(_dev())
    gen = torch.Generator(device=_dev()).manual_seed(3)
    det = DriftDetector(max_samples=20, generator=gen)
    twin = torch.Generator(device=_dev()).manual_seed(3)                # the rule restated: randperm(n)[:max_samples] per set
    ia = torch.randperm(65, generator=twin, device=_dev())[:20].cpu().numpy()
    ib = torch.randperm(63, generator=twin, device=_dev())[:20].cpu().numpy()
    det.set_reference(a)                                                # draws the reference rows, once
    assert np.array_equal(det._ref_index.cpu().numpy(), ia) and len(set(ia.tolist())) == 20
    r = det.detect(b)                                                   # 63 > 20 rows: draws a subsample of b
    xa, xb = a_np[ia], b_np[ib]
    g = 1.0 / 67
    want = np_gram(xa, xa, g) / 400 + np_gram(xb, xb, g) / 400 - 2.0 * np_gram(xa, xb, g) / 400
    assert abs(r.score - want) <= (gram_tol(xa, xa, g) + gram_tol(xb, xb, g) + 2.0 * gram_tol(xa, xb, g)) / 400
    whole = DriftDetector(max_samples=65)                               # at most max_samples rows: every row, nothing drawn
    whole.set_reference(a)
    assert whole._ref_index is None
    _, _, sums = _data((65, 63, 67))
    want = sums["aa"][0] / 65 ** 2 + sums["bb"][0] / 63 ** 2 - 2.0 * sums["ab"][0] / (65 * 63)
    assert abs(whole.detect(b).score - want) <= sums["aa"][1] / 65 ** 2 + sums["bb"][1] / 63 ** 2 + 2.0 * sums["ab"][1] / (65 * 63)


def test_monitor_device_route_agrees_with_the_host_route():
    from nerve_cl.drift import ModelDriftMonitor
    f = np.load(os.path.join(GOLDEN, "drift_monitor.npz"))
    kw = dict(metric_threshold=float(f["threshold"]), window_size=int(f["window"]))
    host, dev = ModelDriftMonitor(**kw), ModelDriftMonitor(**kw)
    host.set_baseline(float(f["baseline"]))
    dev.set_baseline(float(f["baseline"]))
    metrics = [float(m) for m in f["metrics"]]
    flags, means = [], []
    for m in metrics:
        flag = dev.update(torch.tensor(m, dtype=torch.float64, device=_dev()))
        assert flag.is_cuda and flag.dtype == torch.bool
        assert dev.poll() == bool(flag.item())
        flags.append(dev.poll())
        means.append(dev.recent_mean().item())
    want = [host.update(m) for m in metrics]
    assert flags == want == [bool(b) for b in f["flags"]] and any(flags) and not flags[-1]
    w = int(f["window"])
    for k, mean in enumerate(means):                                    # multiples of 1/8: every mean is exact
        held = metrics[max(0, k + 1 - w):k + 1]
        assert mean == sum(held) / len(held)


# ------------------------------------------------------------------------------------------------- script

@pytest.mark.parametrize("method", ["mmd", "psi", "off"])
def test_train_continual_reports_drift(method, tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_continual.py"),
           "--tasks", "2", "--samples", "16", "--epochs", "1", "--features", "16", "--blocks", "1", "--drift", method]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("drift task")]
    if method == "off":
        assert lines == []
        return
    assert len(lines) == 1 and lines[0].startswith(f"drift task 0 -> 1: method={method} score=")
    assert lines[0].split("drift=")[1] in ("True", "False")
    assert r.stdout.index("drift task 0 -> 1") < r.stdout.index("Training on Task 1")
