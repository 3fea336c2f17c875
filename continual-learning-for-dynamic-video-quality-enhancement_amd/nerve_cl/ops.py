"""Differentiable single-kernel ops of the training loop that sit OUTSIDE the network modules.

``mse_loss`` / ``MSELoss`` replace ``nn.MSELoss()`` / ``F.mse_loss`` of the reference's loops
(experiments/train_baseline.py:64,86, train_continual.py:31,55, nerve_cl/continual/ewc.py:125): mean over all elements,
gradient 2 (x - y) / numel w.r.t. the prediction only (the target carries no gradient in any caller).
HIP tensors only; there is no CPU fallback.

``l1_loss``, ``charbonnier_loss`` and ``ssim_loss`` (csrc/quality.hip) follow the same shape: one autograd node, the gradient
with respect to the prediction only.  Every loss takes ``reduction="mean"`` (a scalar) or ``reduction="none"``, which here
means PER SAMPLE: a ``(B,)`` tensor holding the mean over each sample's elements (what an importance-weighted replay
needs), not one value per element.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor):
        _nvq.require_device(pred, "prediction")
        _nvq.require_device(target, "target")
        if pred.shape != target.shape:
            raise RuntimeError(f"mse_loss: shapes differ, {tuple(pred.shape)} vs {tuple(target.shape)}")
        a, b = pred.detach().float().contiguous(), target.detach().float().contiguous()
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        with _nvq.device_guard(a.device):
            _nvq.mse_forward(a, b, out, _engine.workspace(a.device))
        ctx.save_for_backward(a, b)
        ctx.shape = pred.shape
        return out.reshape(())

    @staticmethod
    def backward(ctx, go):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a)
        with _nvq.device_guard(a.device):
            _nvq.mse_backward(a, b, go.detach().float().reshape(1).contiguous(), da)
        return da.view(ctx.shape), None


def _check_reduction(reduction: str) -> bool:
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none' (per sample), got {reduction!r}")
    return reduction == "none"


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """fp32, contiguous and 16-byte aligned (a slice such as x[1:2] of an odd-sized tensor is contiguous but not aligned)"""
    t = t.detach().float().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _pair(name: str, pred: torch.Tensor, target: torch.Tensor):
    _nvq.require_device(pred, "prediction")
    _nvq.require_device(target, "target")
    if pred.shape != target.shape:
        raise RuntimeError(f"{name}: shapes differ, {tuple(pred.shape)} vs {tuple(target.shape)}")
    if pred.numel() == 0:
        raise RuntimeError(f"{name}: empty tensors")
    return _aligned(pred), _aligned(target)


class _PixelLossFn(torch.autograd.Function):
    """mean of |d|, sqrt(d^2 + eps^2) or d^2 (d = pred - target) over the whole tensor or over each sample"""

    @staticmethod
    def forward(ctx, pred, target, kind: int, eps: float, per_sample: bool, name: str):
        a, b = _pair(name, pred, target)
        if per_sample and pred.dim() < 1:
            raise RuntimeError(f"{name}: reduction='none' needs a batch dimension")
        out = torch.empty(a.shape[0] if per_sample else 1, dtype=torch.float32, device=a.device)
        with _nvq.device_guard(a.device):
            _nvq.pixel_loss_forward(a, b, kind, eps, out, _engine.workspace(a.device))
        ctx.save_for_backward(a, b)
        ctx.meta = (pred.shape, kind, eps)
        return out if per_sample else out.reshape(())

    @staticmethod
    def backward(ctx, go):
        a, b = ctx.saved_tensors
        shape, kind, eps = ctx.meta
        da = torch.empty_like(a)
        with _nvq.device_guard(a.device):
            _nvq.pixel_loss_backward(a, b, kind, eps, go.detach().float().reshape(-1).contiguous(), da)
        return da.view(shape), None, None, None, None, None


class _SSIMLossFn(torch.autograd.Function):
    """1 - windowed SSIM; the forward saves only the two inputs, the backward recomputes the local moments per tile"""

    @staticmethod
    def forward(ctx, pred, target, data_range: float, per_sample: bool):
        a, b = _pair("ssim_loss", pred, target)
        _check_ssim_shape("ssim_loss", a)
        out = torch.empty(a.shape[0] if per_sample else 1, dtype=torch.float32, device=a.device)
        with _nvq.device_guard(a.device):
            _nvq.ssim_forward(a, b, data_range, True, out, _engine.workspace(a.device))
        ctx.save_for_backward(a, b)
        ctx.meta = (pred.shape, data_range)
        return out if per_sample else out.reshape(())

    @staticmethod
    def backward(ctx, go):
        a, b = ctx.saved_tensors
        shape, data_range = ctx.meta
        da = torch.empty_like(a)
        with _nvq.device_guard(a.device):
            _nvq.ssim_backward(a, b, data_range, go.detach().float().reshape(-1).contiguous(), -1.0, da)
        return da.view(shape), None, None, None


def _check_ssim_shape(name: str, x: torch.Tensor) -> None:
    if x.dim() != 4 or x.shape[2] < 11 or x.shape[3] < 11:
        raise RuntimeError(f"{name}: needs (B, C, H, W) with H, W >= 11 (an 11 x 11 window, valid positions only), "
                           f"got {tuple(x.shape)}")


def mse_loss(pred: torch.Tensor, target: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """mean((pred - target)^2) as two libnvq launches forward and one backward; ``reduction="none"``: one mean per sample."""
    if _check_reduction(reduction):
        return _PixelLossFn.apply(pred, target, _nvq.LOSS_MSE, 0.0, True, "mse_loss")
    return _MSEFn.apply(pred, target)


def l1_loss(pred: torch.Tensor, target: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """mean |pred - target|; gradient sign(pred - target) / n with sign(0) = 0, as F.l1_loss."""
    return _PixelLossFn.apply(pred, target, _nvq.LOSS_L1, 0.0, _check_reduction(reduction), "l1_loss")


def charbonnier_loss(pred: torch.Tensor, target: torch.Tensor, eps: float = 1e-3, reduction: str = "mean") -> torch.Tensor:
    """mean sqrt((pred - target)^2 + eps^2): the smooth L1 of the super-resolution literature."""
    return _PixelLossFn.apply(pred, target, _nvq.LOSS_CHARBONNIER, float(eps), _check_reduction(reduction),
                              "charbonnier_loss")


def ssim_loss(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, reduction: str = "mean") -> torch.Tensor:
    """1 - SSIM on (B, C, H, W): per channel an 11 x 11 Gaussian window (sigma 1.5), valid positions only, biased local
    statistics, C1 = (0.01 L)^2, C2 = (0.03 L)^2; the map is averaged over a sample's valid positions and channels."""
    return _SSIMLossFn.apply(pred, target, float(data_range), _check_reduction(reduction))


class MSELoss(nn.Module):
    """Drop-in for ``nn.MSELoss()`` (mean reduction) on HIP tensors."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return mse_loss(pred, target)


class _Reduced(nn.Module):
    def __init__(self, reduction: str = "mean"):
        super().__init__()
        _check_reduction(reduction)
        self.reduction = reduction


class L1Loss(_Reduced):
    """Drop-in for ``nn.L1Loss()`` on HIP tensors (``reduction="none"`` is per sample here)."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return l1_loss(pred, target, self.reduction)


class CharbonnierLoss(_Reduced):
    def __init__(self, eps: float = 1e-3, reduction: str = "mean"):
        super().__init__(reduction)
        self.eps = eps

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return charbonnier_loss(pred, target, self.eps, self.reduction)


class SSIMLoss(_Reduced):
    def __init__(self, data_range: float = 1.0, reduction: str = "mean"):
        super().__init__(reduction)
        self.data_range = data_range

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ssim_loss(pred, target, self.data_range, self.reduction)


LOSSES = {"mse": mse_loss, "l1": l1_loss, "charbonnier": charbonnier_loss, "ssim": ssim_loss}
