"""Drift detection on device-resident samples: the reference's ``mlops/drift/detector.py`` (``DriftDetector`` with the RBF-kernel
MMD and the population stability index, ``ModelDriftMonitor``) as libnvq kernels (csrc/drift.hip).

The reference works on numpy arrays on the host; here a window of samples stays where the training step left it.  HIP tensors
run the kernels: the Gram sums of the MMD in float64 on the matrix cores, an ``np.histogram``-exact histogram for the PSI, and
``frame_descriptor`` (per-cell mean and standard deviation of a clip) as one launch.  ``detect_device`` returns the score and the
decision as device tensors without a host synchronisation; ``detect`` copies the two to the host once.  CPU tensors take a float64
torch composition of the same formulas (the package's rule for CPU modules).

Deliberate differences from the reference:

* Each set is used whole when it has at most ``max_samples`` rows and is otherwise subsampled on its own with ``torch.randperm``
  (an optional ``generator``).  The reference cuts BOTH sets to the smaller size and draws with numpy's global RNG, so there
  ``n_ref == n_cur`` always; here ``n_ref != n_cur`` is allowed and the estimator divides each Gram sum by its own count.
* The reference subsample is drawn once in ``set_reference`` (its Gram sum is cached), not at every ``detect``.
* PSI bin edges are computed on the host in float64 from one copy of the reference, once per reference (``psi_reference``): the
  single host round trip of this module.
* The reference's ``method="ks"`` lives in a class of its own, ``KSDriftDetector`` (``ks_2samp`` underneath; csrc/ks.hip,
  DESIGN.md section 27): per-feature sorts in LDS and the exact two-sided p-value as a lattice walk, without scipy.
  ``DriftDetector(method="ks")`` itself still refuses.
* On the device the decision thresholds travel as fp32 kernel arguments: a score within 2^-24 relative of the threshold may be
  decided differently from the float64 comparison of the CPU composition.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from nerve_cl import _nvq

__all__ = ["DriftResult", "DriftDetector", "ModelDriftMonitor", "mmd_rbf", "psi", "psi_reference", "frame_descriptor",
           "ks_2samp", "KSDriftDetector"]

PSI_THRESHOLD = 0.2          # reference detector.py:155
PSI_EPS = 1e-10

_gram_ws: Dict = {}


@dataclass
class DriftResult:
    """Result of drift detection (the reference's fields)."""
    is_drift: bool
    score: float
    threshold: float
    method: str
    details: Dict = None


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """(n, d) fp32, contiguous: a sample of any shape is flattened per row (reference detector.py:83-85)"""
    x = torch.as_tensor(x)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"{what}: needs a non-empty (n, ...) tensor")
    return x.detach().reshape(x.shape[0], -1).float().contiguous()


def _workspace(device, na: int, nb: int) -> torch.Tensor:
    """the per-tile partial sums of one Gram launch (float64); grown on demand, stream-ordered reuse"""
    need = max(int(_nvq.lib().nvq_rbf_gram_workspace_bytes(na, nb, 0)) // 8, 1)
    ws = _gram_ws.get(device)
    if ws is None or ws.numel() < need:
        ws = _gram_ws[device] = torch.empty(max(need, 1024), dtype=torch.float64, device=device)
    return ws


def _subsample(n: int, max_samples: int, device, generator: Optional[torch.Generator]) -> Optional[torch.Tensor]:
    """None when all n rows are used, else max_samples distinct row indices (int32 on `device`)"""
    if n <= max_samples:
        return None
    gdev = generator.device if generator is not None else device
    perm = torch.randperm(n, generator=generator, device=gdev)[:max_samples]
    return perm.to(device=device, dtype=torch.int32)


def _gamma_tensor(gamma: Optional[float], device) -> Optional[torch.Tensor]:
    return None if gamma is None else torch.tensor([float(gamma)], dtype=torch.float64, device=device)


def _gram_cpu(a: torch.Tensor, b: torch.Tensor, gamma: float) -> torch.Tensor:
    a, b = a.double(), b.double()
    dist = (a * a).sum(1, keepdim=True) + (b * b).sum(1, keepdim=True).T - 2.0 * (a @ b.T)
    return torch.exp(-gamma * dist).sum()


def _gram(a: torch.Tensor, b: torch.Tensor, ia, ib, gamma_t, out: torch.Tensor, symmetric: bool) -> None:
    na = a.shape[0] if ia is None else ia.numel()
    nb = b.shape[0] if ib is None else ib.numel()
    _nvq.rbf_gram_sum(a, b, out, _workspace(a.device, na, nb), a_index=ia, b_index=ib, gamma=gamma_t, symmetric=symmetric)


def mmd_rbf(ref: torch.Tensor, cur: torch.Tensor, gamma: Optional[float] = None, max_samples: int = 500,
            generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Biased squared MMD with the kernel exp(-gamma |x - y|^2), gamma = 1 / d by default (reference detector.py:92-105), as a
    float64 scalar on the samples' device."""
    a, b = _rows(ref, "ref"), _rows(cur, "cur")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"mmd_rbf: rows of {a.shape[1]} and {b.shape[1]} features")
    if a.device != b.device:
        raise ValueError(f"mmd_rbf: ref on {a.device}, cur on {b.device}")
    ia = _subsample(a.shape[0], max_samples, a.device, generator)
    ib = _subsample(b.shape[0], max_samples, b.device, generator)
    if not a.is_cuda:
        g = 1.0 / a.shape[1] if gamma is None else float(gamma)
        a = a if ia is None else a[ia.long()]
        b = b if ib is None else b[ib.long()]
        n, m = a.shape[0], b.shape[0]
        return _gram_cpu(a, a, g) / (n * n) + _gram_cpu(b, b, g) / (m * m) - 2.0 * _gram_cpu(a, b, g) / (n * m)
    n = a.shape[0] if ia is None else ia.numel()
    m = b.shape[0] if ib is None else ib.numel()
    sums = torch.empty(3, dtype=torch.float64, device=a.device)
    score = torch.empty((), dtype=torch.float64, device=a.device)
    flag = torch.empty((), dtype=torch.bool, device=a.device)
    with _nvq.device_guard(a.device):
        gt = _gamma_tensor(gamma, a.device)
        _gram(a, a, ia, ia, gt, sums[0:1], True)
        _gram(b, b, ib, ib, gt, sums[1:2], True)
        _gram(a, b, ia, ib, gt, sums[2:3], False)
        _nvq.mmd_finish(sums, n, m, 0.0, score, flag)
    return score


def _histogram_cpu(x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """np.histogram's counts for increasing edges: [e_i, e_{i+1}), the last bin closed; comparisons in double"""
    v, e = x.double().reshape(-1), edges.double()
    inside = (v >= e[0]) & (v <= e[-1])
    bins = (v[inside].unsqueeze(1) >= e[1:-1].unsqueeze(0)).sum(1)
    return torch.bincount(bins, minlength=e.numel() - 1).to(torch.int32)


def _counts(x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    if edges.numel() < 2:                                    # np.histogram with a single edge: no bins
        return torch.empty(0, dtype=torch.int32, device=x.device)
    if not x.is_cuda:
        return _histogram_cpu(x, edges)
    counts = torch.empty(edges.numel() - 1, dtype=torch.int32, device=x.device)
    with _nvq.device_guard(x.device):
        _nvq.psi_counts(x, edges, counts)
    return counts


def _flat(x: torch.Tensor, what: str) -> torch.Tensor:
    x = torch.as_tensor(x)
    if x.numel() == 0:
        raise ValueError(f"{what}: needs a non-empty tensor")
    return x.detach().reshape(-1).float().contiguous()


def psi_reference(ref: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(edges, counts, n) of a reference for ``psi``: the edges are np.unique(np.percentile(ref, 0, 10, .., 100)) computed on
    the host in float64 from one copy of the reference (the single host round trip of this module; reference
    detector.py:141-142), returned as a float64 tensor on the reference's device; the counts are the reference's own
    histogram over them (int32, same device), n its number of elements."""
    r = _flat(ref, "ref")
    edges_np = np.unique(np.percentile(r.cpu().numpy().astype(np.float64), np.arange(0, 101, 10)))
    edges = torch.from_numpy(edges_np).to(r.device)          # a constant reference leaves one edge: no bin, and a PSI of 0
    return edges, _counts(r, edges), r.numel()


def _psi_device(ref_counts: torch.Tensor, n_ref: int, cur_counts: torch.Tensor, n_cur: int):
    score = torch.empty((), dtype=torch.float64, device=cur_counts.device)
    flag = torch.empty((), dtype=torch.bool, device=cur_counts.device)
    with _nvq.device_guard(cur_counts.device):
        _nvq.psi_finish(cur_counts, ref_counts, n_cur, n_ref, score, flag)
    return score, flag


def _psi_scores(ref_edges, ref_counts, n_ref: int, cur):
    c = _flat(cur, "cur")
    if ref_edges.device != c.device:
        raise ValueError(f"psi: reference on {ref_edges.device}, cur on {c.device}")
    cur_counts = _counts(c, ref_edges)
    if cur_counts.numel() == 0:                              # the empty sum of the reference's formula
        return torch.zeros((), dtype=torch.float64, device=c.device), torch.zeros((), dtype=torch.bool, device=c.device)
    if c.is_cuda:
        return _psi_device(ref_counts, int(n_ref), cur_counts, c.numel())
    rp = ref_counts.double() / float(n_ref) + PSI_EPS
    cp = cur_counts.double() / float(c.numel()) + PSI_EPS
    score = ((cp - rp) * torch.log(cp / rp)).sum()
    return score, score > PSI_THRESHOLD


def psi(ref_edges: torch.Tensor, ref_counts: torch.Tensor, n_ref: int, cur: torch.Tensor) -> torch.Tensor:
    """Population stability index of ``cur`` (any shape, flattened) against a reference summarised by ``psi_reference``:
    sum (c_i - r_i) log(c_i / r_i) with c_i = count_i / len(cur) + 1e-10 (reference detector.py:145-152: the array lengths,
    not the counted totals).  A float64 scalar on the device of ``cur``."""
    return _psi_scores(ref_edges, ref_counts, n_ref, cur)[0]


def frame_descriptor(frames: torch.Tensor, grid=(8, 8)) -> torch.Tensor:
    """(B, 2 * C * gh * gw) fp32: the mean, then the population standard deviation, of every cell of a gh x gw grid over each
    channel of (B, C, H, W) frames; a clip (B, T, C, H, W) is read as (B, T * C, H, W).  Cell bounds are those of
    ``adaptive_avg_pool2d``.  One launch on HIP tensors."""
    gh, gw = (grid, grid) if isinstance(grid, int) else grid
    x = torch.as_tensor(frames).detach()
    if x.dim() == 5:
        x = x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3], x.shape[4])
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"frame_descriptor: needs (B, C, H, W) or (B, T, C, H, W) frames, got {tuple(frames.shape)}")
    B, Cc, H, W = x.shape
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f"frame_descriptor: grid {gh} x {gw} on {H} x {W} frames")
    x = x.float().contiguous()
    if not x.is_cuda:
        import torch.nn.functional as F
        xd = x.double()
        mean = F.adaptive_avg_pool2d(xd, (gh, gw))
        var = (F.adaptive_avg_pool2d(xd * xd, (gh, gw)) - mean * mean).clamp_min(0.0)
        return torch.cat([mean.flatten(1), var.sqrt().flatten(1)], 1).float()
    out = torch.empty(B, 2 * Cc * gh * gw, dtype=torch.float32, device=x.device)
    with _nvq.device_guard(x.device):
        _nvq.cell_descriptor(x, gh, gw, out)
    return out


class DriftDetector:
    """The reference's DriftDetector on torch tensors of either device.  ``update`` and ``detect`` return a ``DriftResult`` as
    the reference does (one host copy of score and decision); ``detect_device`` returns them as device tensors and never
    synchronises."""

    def __init__(self, method: str = "mmd", threshold: float = 0.05, window_size: int = 1000, max_samples: int = 500,
                 generator: Optional[torch.Generator] = None):
        if method == "ks":
            raise NotImplementedError(
                "method='ks' is not implemented: the reference's Kolmogorov-Smirnov path needs per-feature sorts and scipy's "
                "exact small-sample p-values; use 'mmd' or 'psi'")
        if method not in ("mmd", "psi"):
            raise ValueError(f"Unknown method: {method}")
        if window_size < 1 or max_samples < 1:
            raise ValueError("window_size and max_samples must be >= 1")
        self.method, self.threshold, self.window_size, self.max_samples = method, threshold, window_size, max_samples
        self.generator = generator
        self.reference_data: Optional[torch.Tensor] = None
        self._window: Optional[torch.Tensor] = None
        self._fill = 0
        self._ref_index: Optional[torch.Tensor] = None
        self._n_ref = 0
        self._sums: Optional[torch.Tensor] = None          # float64 (3,): sum K(ref, ref) cached in slot 0
        self._ref_cpu = self._sxx_cpu = None               # CPU composition: the reference rows in use and their Gram sum
        self._edges = self._ref_counts = None

    # ---------------------------------------------------------------------------------------------------- reference
    def set_reference(self, data: torch.Tensor) -> None:
        """Set the reference distribution.  The data stay on their device; MMD: the reference subsample is fixed here and its
        Gram sum cached; PSI: the bin edges (one host copy, ``psi_reference``) and the reference counts."""
        if self.method == "mmd":
            ref = _rows(data, "reference")
            self.reference_data = ref
            self._ref_index = _subsample(ref.shape[0], self.max_samples, ref.device, self.generator)
            self._n_ref = ref.shape[0] if self._ref_index is None else self._ref_index.numel()
            if ref.is_cuda:
                self._sums = torch.zeros(3, dtype=torch.float64, device=ref.device)
                with _nvq.device_guard(ref.device):
                    _gram(ref, ref, self._ref_index, self._ref_index, None, self._sums[0:1], True)
            else:
                self._ref_cpu = ref if self._ref_index is None else ref[self._ref_index.long()]
                self._sxx_cpu = _gram_cpu(self._ref_cpu, self._ref_cpu, 1.0 / ref.shape[1])
        else:
            ref = _flat(data, "reference")
            self.reference_data = ref
            self._edges, self._ref_counts, self._n_ref = psi_reference(ref)

    # ---------------------------------------------------------------------------------------------------- detection
    def _scores(self, current: torch.Tensor):
        if self.reference_data is None:
            raise ValueError("Reference data not set")
        if self.method == "psi":
            return _psi_scores(self._edges, self._ref_counts, self._n_ref, current)
        ref, cur = self.reference_data, _rows(current, "current")
        if cur.shape[1] != ref.shape[1]:
            raise ValueError(f"current rows have {cur.shape[1]} features, the reference {ref.shape[1]}")
        if cur.device != ref.device:
            raise ValueError(f"current data on {cur.device}, the reference on {ref.device}")
        ic = _subsample(cur.shape[0], self.max_samples, cur.device, self.generator)
        n, m = self._n_ref, cur.shape[0] if ic is None else ic.numel()
        if not cur.is_cuda:
            g = 1.0 / ref.shape[1]
            c = cur if ic is None else cur[ic.long()]
            score = self._sxx_cpu / (n * n) + _gram_cpu(c, c, g) / (m * m) - 2.0 * _gram_cpu(self._ref_cpu, c, g) / (n * m)
            return score, score > self.threshold
        score = torch.empty((), dtype=torch.float64, device=cur.device)
        flag = torch.empty((), dtype=torch.bool, device=cur.device)
        with _nvq.device_guard(cur.device):
            _gram(cur, cur, ic, ic, None, self._sums[1:2], True)
            _gram(ref, cur, self._ref_index, ic, None, self._sums[2:3], False)
            _nvq.mmd_finish(self._sums, n, m, self.threshold, score, flag)
        return score, flag

    def detect_device(self, current: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(score, is_drift) as a float64 and a bool scalar tensor on the data's device; no host synchronisation."""
        return self._scores(current)

    def detect(self, current: torch.Tensor) -> DriftResult:
        """Detect drift between the reference and ``current``; raises ValueError("Reference data not set") without one."""
        score, flag = self._scores(current)
        if score.is_cuda:
            both = torch.stack([score, flag.double()]).cpu()            # the one host copy
            s, f = float(both[0]), bool(both[1] != 0)
        else:
            s, f = float(score), bool(flag)
        return DriftResult(is_drift=f, score=s, threshold=self.threshold if self.method == "mmd" else PSI_THRESHOLD,
                           method=self.method)

    def update(self, sample: torch.Tensor) -> Optional[DriftResult]:
        """Add one sample (any shape) to the preallocated window on its device; a DriftResult once ``window_size`` samples
        have arrived (the window then starts over), else None."""
        row = torch.as_tensor(sample).detach().reshape(-1)
        if self._window is None or self._window.shape[1] != row.numel() or self._window.device != row.device:
            self._window = torch.empty(self.window_size, row.numel(), dtype=torch.float32, device=row.device)
            self._fill = 0
        self._window[self._fill].copy_(row)
        self._fill += 1
        if self._fill < self.window_size:
            return None
        self._fill = 0
        return self.detect(self._window)


class ModelDriftMonitor:
    """The reference's performance monitor: retraining is recommended when the mean of the last ``window_size`` metrics has
    fallen by more than ``metric_threshold`` relative to the baseline (reference detector.py:186-202).

    ``update`` with a python float goes the reference's host route and returns a bool.  ``update`` with a device scalar (for
    example ``nerve_cl.metrics.psnr(...)``) pushes it into a device ring with one launch and returns the decision as a device
    bool tensor without a synchronisation; ``poll()`` reads the latest device decision to the host.  The two routes keep
    separate histories."""

    def __init__(self, metric_threshold: float = 0.1, window_size: int = 100):
        if window_size < 1:
            raise ValueError("window_size must be >= 1")
        self.metric_threshold, self.window_size = metric_threshold, window_size
        self.baseline_metric: Optional[float] = None
        self.metric_history: List[float] = []
        self._ring = self._state = self._mean = self._flag = None

    def set_baseline(self, metric) -> None:
        """Set the baseline metric (a tensor is read to the host once, here)."""
        self.baseline_metric = float(metric)

    def update(self, metric):
        if isinstance(metric, torch.Tensor) and metric.is_cuda:
            return self._update_device(metric)
        self.metric_history.append(float(metric))
        if len(self.metric_history) < self.window_size:
            return False
        recent = np.mean(self.metric_history[-self.window_size:])
        degradation = (self.baseline_metric - recent) / self.baseline_metric
        return bool(degradation > self.metric_threshold)

    def _update_device(self, metric: torch.Tensor) -> torch.Tensor:
        if self.baseline_metric is None:
            raise ValueError("Baseline metric not set")
        if metric.numel() != 1:
            raise ValueError("ModelDriftMonitor.update: a scalar metric")
        dev = metric.device
        if self._ring is None or self._ring.device != dev:
            self._ring = torch.zeros(self.window_size, dtype=torch.float32, device=dev)
            self._state = torch.zeros(2, dtype=torch.int32, device=dev)
            self._mean = torch.zeros((), dtype=torch.float64, device=dev)
            self._flag = torch.zeros((), dtype=torch.bool, device=dev)
        value = metric.detach().reshape(1).float()
        with _nvq.device_guard(dev):
            _nvq.metric_window_update(value, self._ring, self._state, self.baseline_metric, self.metric_threshold, self._mean,
                                      self._flag)
        return self._flag

    def recent_mean(self) -> Optional[torch.Tensor]:
        """the device route's mean over the values held (float64 device scalar; None before the first device update)"""
        return self._mean

    def poll(self) -> bool:
        """the device route's latest decision, read to the host"""
        return bool(self._flag.item()) if self._flag is not None else False


# ----------------------------------------------------------------------------------------------- Kolmogorov-Smirnov (csrc/ks.hip)
KS_MAX_SAMPLES = _nvq.KS_MAX_N          # one column of a set is sorted in LDS


def _ks_sizes(n1: int, n2: int) -> Tuple[int, int, int]:
    """(a, b, lcm): the distribution functions differ by (a x - b y) / lcm after x values of the first and y of the second set"""
    g = math.gcd(n1, n2)
    return n2 // g, n1 // g, n1 // g * n2


def _ks_sorted(x: torch.Tensor, index: Optional[torch.Tensor]) -> torch.Tensor:
    """The rows of x (rows, d) fp32 in use as ascending feature-major columns (d, n): fp32 from one launch on a HIP tensor,
    float64 from torch.sort on the CPU (where -0.0 and +0.0 compare equal as well)."""
    if not x.is_cuda:
        rows = x if index is None else x[index.long()]
        return torch.sort(rows.double().T.contiguous(), dim=1).values
    n = x.shape[0] if index is None else index.numel()
    out = torch.empty(x.shape[1], n, dtype=torch.float32, device=x.device)
    with _nvq.device_guard(x.device):
        _nvq.sort_columns(x, index, out)
    return out


def _ks_statistic_cpu(rs: torch.Tensor, cs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(h, D): h = lcm * D as exact integers, from right ranks of every value of either sample in both sorted samples"""
    a, b, lcm = _ks_sizes(rs.shape[1], cs.shape[1])
    both = torch.cat([rs, cs], 1)
    c1 = torch.searchsorted(rs, both, right=True)
    c2 = torch.searchsorted(cs, both, right=True)
    h = (a * c1 - b * c2).abs().max(1).values
    return h, h.double() / float(lcm)


def _ks_pvalue_cpu(h: torch.Tensor, n1: int, n2: int) -> torch.Tensor:
    """The exact two-sided p-value of every h (int64, (d,)): the walk of csrc/ks.hip, one anti-diagonal x + y = s of the lattice
    per step for all features at once.  The mass at (x, y) moves to (x + 1, y) with weight (n1 - x) / rem and to (x, y + 1)
    with (n2 - y) / rem, rem = n1 + n2 - (x + y); what arrives outside |a x - b y| < h is added to p and leaves the walk.  Only
    the cells that the widest band (the largest h) can reach are carried."""
    a, b, _ = _ks_sizes(n1, n2)
    A, N = a + b, n1 + n2
    d = h.numel()
    hmax = int(h.max())
    p = torch.zeros(d, dtype=torch.float64)
    if hmax > 0:
        hcol = h.reshape(d, 1)
        mass, m0 = torch.ones(d, 1, dtype=torch.float64), 0                 # mass[:, i] is cell x = m0 + i of the previous step
        for s in range(1, N + 1):
            t = b * (s - 1)
            lo = max(0, s - 1 - n2, (t - hmax) // A + 1)                    # live cells of step s - 1 under the widest band
            hi = min(n1, s - 1, -((-(t + hmax)) // A) - 1)
            x0, x1 = max(lo, s - n2), min(hi + 1, n1, s)                    # the cells they reach
            if lo > hi or x0 > x1:
                break
            pad = torch.nn.functional.pad(mass, (1, 1))                     # pad[:, j] is cell m0 - 1 + j
            x = torch.arange(x0, x1 + 1)
            left, own = pad[:, x0 - m0:x1 - m0 + 1], pad[:, x0 - m0 + 1:x1 - m0 + 2]
            new = (left * (n1 - x + 1).double() + own * (n2 - (s - 1 - x)).clamp(min=0).double()) / float(N - s + 1)
            outside = (A * x - b * s).abs().reshape(1, -1) >= hcol
            p += torch.where(outside, new, torch.zeros(())).sum(1)
            mass, m0 = torch.where(outside, torch.zeros(()), new), x0
    p[h <= 0] = 1.0
    return p.clamp_(max=1.0)


def _ks_from_sorted(rs: torch.Tensor, cs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(statistic, pvalue), float64 (d,), from ascending feature-major columns of either device"""
    d, n1 = rs.shape
    n2 = cs.shape[1]
    if not rs.is_cuda:
        h, stat = _ks_statistic_cpu(rs, cs)
        return stat, _ks_pvalue_cpu(h, n1, n2)
    h = torch.empty(d, dtype=torch.int32, device=rs.device)
    stat = torch.empty(d, dtype=torch.float64, device=rs.device)
    p = torch.empty(d, dtype=torch.float64, device=rs.device)
    with _nvq.device_guard(rs.device):
        _nvq.ks_statistic(rs, cs, h, stat)
        _nvq.ks_pvalue(h, n1, n2, p)
    return stat, p


def _ks_check_rows(n: int, what: str) -> None:
    if n > KS_MAX_SAMPLES:
        raise ValueError(f"{what}: {n} rows, a Kolmogorov-Smirnov set has at most {KS_MAX_SAMPLES}")


def ks_2samp(ref: torch.Tensor, cur: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two-sided two-sample Kolmogorov-Smirnov test of every feature: ``ref`` (n1, ...) and ``cur`` (n2, ...) are flattened per
    row to d features; returns (statistic, pvalue), two float64 (d,) tensors on the samples' device, the numbers that
    ``scipy.stats.ks_2samp`` gives in its exact mode (which its ``auto`` picks for sets this small).  A set has at most 4096
    rows.  Values that compare equal are ties (-0.0 and +0.0 too), infinities are ordinary values; NaN is not supported (the
    result is then unspecified)."""
    a, b = _rows(ref, "ref"), _rows(cur, "cur")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"ks_2samp: rows of {a.shape[1]} and {b.shape[1]} features")
    if a.device != b.device:
        raise ValueError(f"ks_2samp: ref on {a.device}, cur on {b.device}")
    _ks_check_rows(a.shape[0], "ks_2samp: ref")
    _ks_check_rows(b.shape[0], "ks_2samp: cur")
    return _ks_from_sorted(_ks_sorted(a, None), _ks_sorted(b, None))


class KSDriftDetector:
    """The reference's ``DriftDetector(method="ks")``: a two-sample Kolmogorov-Smirnov test per feature, the score
    ``min(p_values) * d`` (Bonferroni without a clamp: it can exceed 1), drift when ``score < threshold``.  The methods and
    their contracts are ``DriftDetector``'s; ``detect`` also names the features: ``details["p_values"]`` and
    ``details["statistics"]`` are float64 (d,) tensors on the data's device.  A set with more than ``max_samples`` rows is
    subsampled by the module's rule, the reference once in ``set_reference`` (where it is also sorted, once), the current set at
    every detect."""

    def __init__(self, threshold: float = 0.05, window_size: int = 1000, max_samples: int = KS_MAX_SAMPLES,
                 generator: Optional[torch.Generator] = None):
        if not 1 <= max_samples <= KS_MAX_SAMPLES:
            raise ValueError(f"max_samples must be in [1, {KS_MAX_SAMPLES}]")
        if window_size < 1:
            raise ValueError("window_size must be >= 1")
        self.method, self.threshold, self.window_size, self.max_samples = "ks", threshold, window_size, max_samples
        self.generator = generator
        self.reference_data: Optional[torch.Tensor] = None
        self._window: Optional[torch.Tensor] = None
        self._fill = 0
        self._ref_index: Optional[torch.Tensor] = None
        self._ref_sorted: Optional[torch.Tensor] = None      # (d, n_ref) ascending columns of the reference rows in use

    def set_reference(self, data: torch.Tensor) -> None:
        """Set the reference distribution: the data stay on their device, the subsample is drawn and its columns sorted here."""
        ref = _rows(data, "reference")
        self.reference_data = ref
        self._ref_index = _subsample(ref.shape[0], self.max_samples, ref.device, self.generator)
        self._ref_sorted = _ks_sorted(ref, self._ref_index)

    def _scores(self, current: torch.Tensor):
        if self.reference_data is None:
            raise ValueError("Reference data not set")
        ref, cur = self.reference_data, _rows(current, "current")
        if cur.shape[1] != ref.shape[1]:
            raise ValueError(f"current rows have {cur.shape[1]} features, the reference {ref.shape[1]}")
        if cur.device != ref.device:
            raise ValueError(f"current data on {cur.device}, the reference on {ref.device}")
        ic = _subsample(cur.shape[0], self.max_samples, cur.device, self.generator)
        stat, p = _ks_from_sorted(self._ref_sorted, _ks_sorted(cur, ic))
        if not cur.is_cuda:
            score = p.min() * float(p.numel())
            return score, score < self.threshold, p, stat
        score = torch.empty((), dtype=torch.float64, device=cur.device)
        flag = torch.empty((), dtype=torch.bool, device=cur.device)
        with _nvq.device_guard(cur.device):
            _nvq.ks_finish(p, self.threshold, score, flag)
        return score, flag, p, stat

    def detect_device(self, current: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(score, is_drift) as a float64 and a bool scalar tensor on the data's device; no host synchronisation."""
        return self._scores(current)[:2]

    def detect(self, current: torch.Tensor) -> DriftResult:
        """Detect drift between the reference and ``current``; raises ValueError("Reference data not set") without one."""
        score, flag, p, stat = self._scores(current)
        if score.is_cuda:
            both = torch.stack([score, flag.double()]).cpu()            # the one host copy
            s, f = float(both[0]), bool(both[1] != 0)
        else:
            s, f = float(score), bool(flag)
        return DriftResult(is_drift=f, score=s, threshold=self.threshold, method="ks", details={"p_values": p, "statistics": stat})

    def update(self, sample: torch.Tensor) -> Optional[DriftResult]:
        """Add one sample (any shape) to the preallocated window on its device; a DriftResult once ``window_size`` samples
        have arrived (the window then starts over), else None."""
        row = torch.as_tensor(sample).detach().reshape(-1)
        if self._window is None or self._window.shape[1] != row.numel() or self._window.device != row.device:
            self._window = torch.empty(self.window_size, row.numel(), dtype=torch.float32, device=row.device)
            self._fill = 0
        self._window[self._fill].copy_(row)
        self._fill += 1
        if self._fill < self.window_size:
            return None
        self._fill = 0
        return self.detect(self._window)
