"""Evaluation metrics of the reference's table (PSNR, SSIM, MAE, MSE) without torch arithmetic over the images.

``quality_sums`` is ONE libnvq pass over a prediction and its target that leaves eight float64 numbers per sample on the
device; ``mse``, ``mae``, ``psnr`` and ``ssim_global`` are pure functions of such sums, so they work on one row, on the sum
of rows (sums add: a dataset's metric is the metric of its summed rows) and on CPU tensors alike.  ``ssim`` is the windowed
SSIM of ``nerve_cl.ops.ssim_loss`` as a metric, ``ms_ssim`` the multi-scale one.  ``QualityMeter`` accumulates over an epoch without a host synchronisation.
No autograd here; HIP tensors only for everything that reads images (there is no CPU fallback).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from nerve_cl import _engine, _nvq, ops

# columns of a sums row
N, SX, SY, SXX, SYY, SXY, SABS, SSQ = range(8)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """fp32, contiguous and 16-byte aligned (a slice such as x[1:2] of an odd-sized tensor is contiguous but not aligned)"""
    t = t.detach().float().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _pair(name: str, pred: torch.Tensor, target: torch.Tensor):
    _nvq.require_device(pred, "prediction")
    _nvq.require_device(target, "target")
    if pred.shape != target.shape:
        raise RuntimeError(f"{name}: shapes differ, {tuple(pred.shape)} vs {tuple(target.shape)}")
    if pred.dim() < 1 or pred.numel() == 0:
        raise RuntimeError(f"{name}: needs non-empty (B, ...) tensors")
    return _aligned(pred), _aligned(target)


def quality_sums(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(B, 8) float64 on the device, per sample: n, sum x, sum y, sum x^2, sum y^2, sum xy, sum |x - y|, sum (x - y)^2
    (x = pred, y = target), from one pass over both tensors."""
    a, b = _pair("quality_sums", pred, target)
    out = torch.empty(a.shape[0], 8, dtype=torch.float64, device=a.device)
    with _nvq.device_guard(a.device):
        _nvq.quality_sums(a, b, out, _engine.workspace(a.device))
    return out


def _sums(s) -> torch.Tensor:
    s = torch.as_tensor(s)
    if s.shape[-1] != 8:
        raise ValueError(f"expected (..., 8) quality sums, got {tuple(s.shape)}")
    return s.double()


def mse(sums) -> torch.Tensor:
    s = _sums(sums)
    return s[..., SSQ] / s[..., N]


def mae(sums) -> torch.Tensor:
    s = _sums(sums)
    return s[..., SABS] / s[..., N]


def psnr(sums, data_range: float = 1.0) -> torch.Tensor:
    """20 log10(data_range / sqrt(mse)) (the formula of experiments/_common.compute_psnr); +inf at mse = 0."""
    return 20.0 * torch.log10(data_range / torch.sqrt(mse(sums)))


def ssim_global(sums, data_range: float = 1.0) -> torch.Tensor:
    """The global-statistics SSIM of the reference's evaluation table: one window that is the whole image,
    ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)), C1 = (0.01 L)^2, C2 = (0.03 L)^2.
    s_x^2 and s_y^2 are the UNBIASED variances (divide by n - 1) while s_xy is the BIASED covariance (divide by n): that mix
    is what the published table was computed with, so it is kept here on purpose."""
    s = _sums(sums)
    n = s[..., N]
    mx, my = s[..., SX] / n, s[..., SY] / n
    vx = (s[..., SXX] - n * mx * mx) / (n - 1.0)
    vy = (s[..., SYY] - n * my * my) / (n - 1.0)
    cxy = s[..., SXY] / n - mx * my
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, reduction: str = "mean") -> torch.Tensor:
    """Windowed SSIM (Wang et al. 2004) of (B, C, H, W) tensors: per channel an 11 x 11 Gaussian window, sigma 1.5, valid
    positions only; ``"mean"``: a scalar over the batch, ``"none"``: (B,) per sample.  The forward kernel of ssim_loss."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none' (per sample), got {reduction!r}")
    a, b = _pair("ssim", pred, target)
    if a.dim() != 4 or a.shape[2] < 11 or a.shape[3] < 11:
        raise RuntimeError(f"ssim: needs (B, C, H, W) with H, W >= 11, got {tuple(a.shape)}")
    out = torch.empty(a.shape[0] if reduction == "none" else 1, dtype=torch.float32, device=a.device)
    with _nvq.device_guard(a.device):
        _nvq.ssim_forward(a, b, float(data_range), False, out, _engine.workspace(a.device))
    return out if reduction == "none" else out.reshape(())


def ms_ssim(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, weights: Optional[Sequence[float]] = None,
            reduction: str = "mean") -> torch.Tensor:
    """Multi-scale SSIM of (B, C, H, W) tensors, the forward of ``nerve_cl.ops.ms_ssim_loss`` as a metric (its definition and
    arguments): ``"mean"``: a scalar over the batch, ``"none"``: (B,) per sample."""
    per_sample = ops._check_reduction(reduction)
    w, a, b = ops._ms_ssim_args("ms_ssim", pred, target, weights)
    out, _, _ = ops._ms_ssim_forward(a, b, float(data_range), w, per_sample, False)
    return out if per_sample else out.reshape(())


class QualityMeter:
    """Accumulates quality sums over batches on the device.

    ``update`` launches kernels and adds; it never synchronises with the host.  ``all_reduce`` is one SUM all-reduce of the
    accumulator across data-parallel ranks.  ``compute`` is the only host synchronisation.

    averaging="dataset" (default): the metrics of the summed sums, i.e. of all elements seen.
    averaging="batch": psnr, ssim_global, mae and mse are means of the per-batch values (what the training scripts print
    today: the mean of per-batch PSNR); the per-batch values stay on the device until ``compute``.
    """

    def __init__(self, data_range: float = 1.0, averaging: str = "dataset"):
        if averaging not in ("dataset", "batch"):
            raise ValueError(f"averaging must be 'dataset' or 'batch', got {averaging!r}")
        self.data_range = float(data_range)
        self.averaging = averaging
        self._acc: Optional[torch.Tensor] = None   # 8 sums, then sum over batches of (psnr, ssim_global, mae, mse), then #batches

    def reset(self) -> None:
        self._acc = None

    def update_sums(self, sums) -> None:
        """Add one batch given as (8,) or (B, 8) sums (any device; the accumulator lives where the first batch does)."""
        s = _sums(sums).reshape(-1, 8).sum(0)
        per_batch = torch.stack([psnr(s, self.data_range), ssim_global(s, self.data_range), mae(s), mse(s)])
        row = torch.cat([s, per_batch, torch.ones(1, dtype=torch.float64, device=s.device)])
        self._acc = row if self._acc is None else self._acc + row

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        self.update_sums(quality_sums(pred, target))

    def all_reduce(self, group=None) -> None:
        import torch.distributed as dist
        if self._acc is not None and dist.is_available() and dist.is_initialized():
            dist.all_reduce(self._acc, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> Dict[str, float]:
        if self._acc is None:
            raise RuntimeError("QualityMeter.compute() before any update()")
        acc = self._acc
        s = acc[:8]
        if self.averaging == "batch":
            vals = acc[8:12] / acc[12]
        else:
            vals = torch.stack([psnr(s, self.data_range), ssim_global(s, self.data_range), mae(s), mse(s)])
        host = torch.cat([vals, s[:1]]).tolist()   # the one device-to-host copy
        return {"psnr": host[0], "ssim_global": host[1], "mae": host[2], "mse": host[3], "n": host[4]}
