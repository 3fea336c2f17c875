"""Differentiable single-kernel ops of the training loop that sit OUTSIDE the network modules.

``mse_loss`` / ``MSELoss`` replace ``nn.MSELoss()`` / ``F.mse_loss`` of the reference's loops
(experiments/train_baseline.py:64,86, train_continual.py:31,55, nerve_cl/continual/ewc.py:125): mean over all elements,
gradient 2 (x - y) / numel w.r.t. the prediction only (the target carries no gradient in any caller).
HIP tensors only; there is no CPU fallback.

``l1_loss``, ``charbonnier_loss`` and ``ssim_loss`` (csrc/quality.hip) follow the same shape: one autograd node, the gradient
with respect to the prediction only.  Every loss takes ``reduction="mean"`` (a scalar) or ``reduction="none"``, which here
means PER SAMPLE: a ``(B,)`` tensor holding the mean over each sample's elements (what an importance-weighted replay
needs), not one value per element.

``ms_ssim_loss`` / ``MSSSIMLoss`` (multi-scale SSIM) and the ``ms_ssim_l1_loss`` mix follow the same rules.

``distill_loss`` / ``DistillLoss`` (the output term of a distillation step: teacher and target terms from one pass over the
student output) and ``cosine_feature_loss`` / ``CosineFeatureLoss`` (feature distillation on ``return_intermediate`` tensors)
are csrc/distill.hip; their gradient is with respect to the student only.

``ppo_loss`` (csrc/abr.hip) is the clipped-surrogate PPO loss of the ABR agent over the actor-critic's head
outputs: one pass that also writes the gradient, one autograd node; CPU tensors take a float64 torch composition.

``clip_grad_norm_`` is not a loss: global 2-norm gradient clipping on the flat gradient buckets without a host read
(csrc/bucket_ops.hip).
"""
from __future__ import annotations

import weakref
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import Segment, grad_pairs, segments_of, sum_moments


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


# the five standard MS-SSIM scale weights (Wang, Simoncelli, Bovik 2003), finest scale first
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_ms_weight_cache = {}


def ms_ssim_weights(scales: int) -> Tuple[float, ...]:
    """The first ``scales`` (1 to 5) standard weights divided by their sum (the published five sum to 1.0001, so
    ``ms_ssim_weights(5)`` is the standard tuple to four digits)."""
    if not 1 <= int(scales) <= len(MS_SSIM_WEIGHTS):
        raise ValueError(f"ms_ssim_weights: scales must be 1 to {len(MS_SSIM_WEIGHTS)}, got {scales}")
    head = MS_SSIM_WEIGHTS[:int(scales)]
    return tuple(w / sum(head) for w in head)


def ms_ssim_max_scales(H: int, W: int) -> int:
    """The largest number of scales M <= 5 whose coarsest scale still holds an 11 x 11 window: min(H, W) >> (M - 1) >= 11
    (0 when not even one scale fits)."""
    m = 0
    while m < len(MS_SSIM_WEIGHTS) and (min(H, W) >> m) >= 11:
        m += 1
    return m


def _ms_ssim_args(name: str, pred: torch.Tensor, target: torch.Tensor, weights: Optional[Sequence[float]]):
    """The checked weights as a tuple and the aligned inputs; every argument error comes before anything touches the device"""
    w = MS_SSIM_WEIGHTS if weights is None else tuple(float(v) for v in weights)
    if not 1 <= len(w) <= 8 or not all(0.0 < v < float("inf") for v in w):
        raise ValueError(f"{name}: weights must be 1 to 8 positive numbers, got {w}")
    if pred.dim() != 4 or (min(pred.shape[2], pred.shape[3]) >> (len(w) - 1)) < 11:
        raise RuntimeError(f"{name}: needs (B, C, H, W) with min(H, W) >> {len(w) - 1} >= 11 (the coarsest of {len(w)} scales "
                           f"must hold an 11 x 11 window: H, W >= {11 << (len(w) - 1)}), got {tuple(pred.shape)}")
    a, b = _pair(name, pred, target)
    return w, a, b


def _ms_weights_on(device: torch.device, w: Tuple[float, ...]) -> torch.Tensor:
    key = (device, w)
    t = _ms_weight_cache.get(key)
    if t is None:
        t = _ms_weight_cache[key] = torch.tensor(w, dtype=torch.float32, device=device)
    return t


def _pool_pair(x: torch.Tensor, y: torch.Tensor):
    """the 2 x 2 means of x and y (one launch) as temporaries of PyTorch's allocator"""
    shape = (*x.shape[:-2], x.shape[-2] // 2, x.shape[-1] // 2)
    px, py = x.new_empty(shape), x.new_empty(shape)
    _nvq.avgpool2_pair(x, y, px, py)
    return px, py


def _ms_ssim_forward(a: torch.Tensor, b: torch.Tensor, data_range: float, w: Tuple[float, ...], per_sample: bool, as_loss: bool):
    """(out, mtable, dtable) of nvq_msssim_finalize: 2 M launches (M scale passes, M - 1 poolings, the finalize)"""
    B, Cc, H, W = a.shape
    M = len(w)
    out = torch.empty(B if per_sample else 1, dtype=torch.float32, device=a.device)
    mt = torch.empty(M, B * Cc, dtype=torch.float32, device=a.device)
    dt = torch.empty_like(mt)
    with _nvq.device_guard(a.device):
        ws = _engine.workspace(a.device)
        x, y = a, b
        for j in range(M):
            _nvq.msssim_scale_forward(x, y, H, W, M, j, data_range, ws)
            if j + 1 < M:
                x, y = _pool_pair(x, y)
        _nvq.msssim_finalize(ws, B, Cc, H, W, _ms_weights_on(a.device, w), as_loss, out, mt, dt)
    return out, mt, dt


class _MSSSIMLossFn(torch.autograd.Function):
    """1 - MS-SSIM; saves the two inputs and the finalize's two (M, B * C) tables, the backward recomputes the pyramid"""

    @staticmethod
    def forward(ctx, pred, target, data_range: float, weights, per_sample: bool):
        w, a, b = _ms_ssim_args("ms_ssim_loss", pred, target, weights)
        out, mt, dt = _ms_ssim_forward(a, b, data_range, w, per_sample, True)
        ctx.save_for_backward(a, b, mt, dt)
        ctx.meta = (pred.shape, data_range, len(w))
        return out if per_sample else out.reshape(())

    @staticmethod
    def backward(ctx, go):
        a, b, _, dt = ctx.saved_tensors
        shape, data_range, M = ctx.meta
        H, W = a.shape[2:]
        go = go.detach().float().reshape(-1).contiguous()
        with _nvq.device_guard(a.device):
            levels = [(a, b)]
            for _ in range(M - 1):
                levels.append(_pool_pair(*levels[-1]))
            dx = None
            for j in range(M - 1, -1, -1):           # coarsest first: each launch folds in the pooling adjoint of the one before
                x, y = levels[j]
                d = torch.empty_like(x)
                _nvq.msssim_scale_backward(x, y, H, W, M, j, data_range, dt, go, -1.0, dx, d)
                dx = d
        return dx.view(shape), None, None, None, None


def ms_ssim_loss(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, weights: Optional[Sequence[float]] = None,
                 reduction: str = "mean") -> torch.Tensor:
    """1 - MS-SSIM on (B, C, H, W).  Scale j of the 2 x 2 mean pyramid gives, per plane, the mean over the valid positions of
    cs = (2 s_xy + C2) / (s_xx + s_yy + C2) (the last scale: of the SSIM map, window and constants of ``ssim_loss``); a plane's
    value is prod_j max(mean_j, 0)^w_j, a sample's the mean over its channels.  ``weights``: 1 to 8 positive numbers, default
    the five standard ones; the coarsest scale must hold a window (``ms_ssim_max_scales``, ``ms_ssim_weights``).  A clamped
    term gives the value 0 and a zero gradient."""
    per_sample = _check_reduction(reduction)
    return _MSSSIMLossFn.apply(pred, target, float(data_range), weights, per_sample)


def ms_ssim_l1_loss(pred: torch.Tensor, target: torch.Tensor, alpha: float = 0.84, data_range: float = 1.0,
                    weights: Optional[Sequence[float]] = None, reduction: str = "mean") -> torch.Tensor:
    """alpha * ms_ssim_loss + (1 - alpha) * l1_loss (Zhao et al. 2017, without the Gaussian weighting of the L1 term)"""
    return (alpha * ms_ssim_loss(pred, target, data_range, weights, reduction)
            + (1.0 - alpha) * l1_loss(pred, target, reduction))


# ------------------------------------------------------------------------------------------------ distillation (section 18)

def _distill_args(name: str, student: torch.Tensor, teacher: torch.Tensor, target: Optional[torch.Tensor], per_sample: bool):
    """every argument error of the output term, then the refusal of CPU tensors, before anything touches the device"""
    if student.shape != teacher.shape:
        raise RuntimeError(f"{name}: shapes differ, student {tuple(student.shape)} vs teacher {tuple(teacher.shape)}")
    if target is not None and target.shape != student.shape:
        raise RuntimeError(f"{name}: shapes differ, student {tuple(student.shape)} vs target {tuple(target.shape)}")
    if student.numel() == 0:
        raise RuntimeError(f"{name}: empty tensors")
    if per_sample and student.dim() < 1:
        raise RuntimeError(f"{name}: reduction='none' needs a batch dimension")
    _nvq.require_device(student, "student output")
    _nvq.require_device(teacher, "teacher output")
    if target is not None:
        _nvq.require_device(target, "target")


class _DistillFn(torch.autograd.Function):
    """wt * mean (s - t)^2 + wy * mean (s - y)^2 from one pass over s, t, y (two launches); the backward is one launch that
    writes ds once.  Outputs (value, d, m); d and m are report values without a gradient."""

    @staticmethod
    def forward(ctx, student, teacher, target, wt: float, wy: float, per_sample: bool):
        s, t = _aligned(student), _aligned(teacher)
        y = None if target is None else _aligned(target)
        G = s.shape[0] if per_sample else 1
        out = torch.empty(3, G, dtype=torch.float32, device=s.device)
        with _nvq.device_guard(s.device):
            _nvq.distill_forward(s, t, y, wt, wy, out, _engine.workspace(s.device))
        if y is None:
            ctx.save_for_backward(s, t)
        else:
            ctx.save_for_backward(s, t, y)
        ctx.meta = (student.shape, wt, wy)
        value, d, m = (out[0], out[1], out[2]) if per_sample else (out[0, 0], out[1, 0], out[2, 0])
        ctx.mark_non_differentiable(d, m)
        ctx.set_materialize_grads(False)     # (no zero tensors for d and m; the value's gradient is never None in backward)
        return value, d, m

    @staticmethod
    def backward(ctx, go, _gd, _gm):
        s, t, *rest = ctx.saved_tensors
        shape, wt, wy = ctx.meta
        ds = torch.empty_like(s)
        with _nvq.device_guard(s.device):
            _nvq.distill_backward(s, t, rest[0] if rest else None, wt, wy, go.detach().float().reshape(-1).contiguous(), ds)
        return ds.view(shape), None, None, None, None, None


def _distill_weighted(student: torch.Tensor, teacher: torch.Tensor, target: Optional[torch.Tensor], wt: float, wy: float,
                      reduction: str = "mean", name: str = "distill_loss"):
    """(wt * mse(s, t) + wy * mse(s, y), mse(s, t), mse(s, y)) with free weights: ``distill_loss`` is (alpha, 1 - alpha), a
    distillation step with its MSE task term folded in is (alpha, 2 - alpha)"""
    per_sample = _check_reduction(reduction)
    _distill_args(name, student, teacher, target, per_sample)
    return _DistillFn.apply(student, teacher, target, float(wt), float(wy) if target is not None else 0.0, per_sample)


def distill_loss(student: torch.Tensor, teacher: torch.Tensor, target: Optional[torch.Tensor] = None, alpha: float = 0.5,
                 reduction: str = "mean", return_terms: bool = False):
    """alpha * mse(student, teacher) + (1 - alpha) * mse(student, target), or mse(student, teacher) without a target: one
    autograd node, one pass over the tensors forward and one backward.  The gradient is with respect to ``student`` only.
    ``return_terms``: also the two means d = mse(student, teacher) and m = mse(student, target) (0 without a target), which
    carry no gradient."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distill_loss: alpha must be in [0, 1], got {alpha}")
    wt, wy = (1.0, 0.0) if target is None else (alpha, 1.0 - alpha)
    value, d, m = _distill_weighted(student, teacher, target, wt, wy, reduction)
    return (value, d, m) if return_terms else value


def _cosine_args(name: str, student: torch.Tensor, teacher: torch.Tensor) -> None:
    if student.dim() != 4:
        raise RuntimeError(f"{name}: needs (B, C, H, W) feature tensors, got {tuple(student.shape)}")
    if student.shape != teacher.shape:
        raise RuntimeError(f"{name}: shapes differ, student {tuple(student.shape)} vs teacher {tuple(teacher.shape)}")
    if student.numel() == 0:
        raise RuntimeError(f"{name}: empty tensors")


class _CosineFn(torch.autograd.Function):
    """mean over the positions of 1 - cos(s_p, t_p); saves the two inputs only, the backward recomputes the moments"""

    @staticmethod
    def forward(ctx, student, teacher, eps: float, per_sample: bool):
        s, t = _aligned(student), _aligned(teacher)
        out = torch.empty(s.shape[0] if per_sample else 1, dtype=torch.float32, device=s.device)
        with _nvq.device_guard(s.device):
            _nvq.cosine_distill_forward(s, t, eps, per_sample, out, _engine.workspace(s.device))
        ctx.save_for_backward(s, t)
        ctx.meta = (student.shape, eps, per_sample)
        return out if per_sample else out.reshape(())

    @staticmethod
    def backward(ctx, go):
        s, t = ctx.saved_tensors
        shape, eps, per_sample = ctx.meta
        ds = torch.empty_like(s)
        with _nvq.device_guard(s.device):
            _nvq.cosine_distill_backward(s, t, eps, go.detach().float().reshape(-1).contiguous(), per_sample, ds)
        return ds.view(shape), None, None, None


Features = Union[torch.Tensor, Sequence[torch.Tensor]]


def cosine_feature_loss(student: Features, teacher: Features, eps: float = 1e-8, reduction: str = "mean") -> torch.Tensor:
    """Feature distillation on (B, C, H, W) tensors: v_p = 1 - <s_p, t_p> / (max(|s_p|, eps) max(|t_p|, eps)) over the channels
    of every position, averaged over the positions (of the batch, or of each sample with ``reduction="none"``).  Lists of such
    tensors (the ``features`` and ``aligned`` entries of ``return_intermediate``) give the mean over the list's entries, one
    launch pair per entry.  The gradient is with respect to ``student`` only; where |s_p| <= eps the norm is the constant eps."""
    per_sample = _check_reduction(reduction)
    eps = float(eps)
    if not eps > 0.0:
        raise ValueError(f"cosine_feature_loss: eps must be > 0, got {eps}")
    is_list = not isinstance(student, torch.Tensor)
    if is_list != (not isinstance(teacher, torch.Tensor)):
        raise TypeError("cosine_feature_loss: student and teacher must both be tensors or both be lists of tensors")
    ss: List[torch.Tensor] = list(student) if is_list else [student]
    ts: List[torch.Tensor] = list(teacher) if is_list else [teacher]
    if len(ss) != len(ts) or not ss:
        raise RuntimeError(f"cosine_feature_loss: needs two non-empty lists of equal length, got {len(ss)} and {len(ts)}")
    for a, b in zip(ss, ts):
        _cosine_args("cosine_feature_loss", a, b)
    for a, b in zip(ss, ts):
        _nvq.require_device(a, "student features")
        _nvq.require_device(b, "teacher features")
    total = None
    for a, b in zip(ss, ts):
        v = _CosineFn.apply(a, b, eps, per_sample)
        total = v if total is None else total + v
    return total / len(ss) if len(ss) > 1 else total


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


class MSSSIMLoss(_Reduced):
    def __init__(self, data_range: float = 1.0, weights: Optional[Sequence[float]] = None, reduction: str = "mean"):
        super().__init__(reduction)
        self.data_range = data_range
        self.weights = None if weights is None else tuple(float(v) for v in weights)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ms_ssim_loss(pred, target, self.data_range, self.weights, self.reduction)


class DistillLoss(_Reduced):
    """``distill_loss`` as a module: forward(student, teacher, target=None)"""

    def __init__(self, alpha: float = 0.5, reduction: str = "mean"):
        super().__init__(reduction)
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"DistillLoss: alpha must be in [0, 1], got {alpha}")
        self.alpha = float(alpha)

    def forward(self, student: torch.Tensor, teacher: torch.Tensor, target: Optional[torch.Tensor] = None) -> torch.Tensor:
        return distill_loss(student, teacher, target, self.alpha, self.reduction)


class CosineFeatureLoss(_Reduced):
    """``cosine_feature_loss`` as a module: forward(student, teacher) on (B, C, H, W) tensors or lists of them"""

    def __init__(self, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(reduction)
        if not float(eps) > 0.0:
            raise ValueError(f"CosineFeatureLoss: eps must be > 0, got {eps}")
        self.eps = float(eps)

    def forward(self, student: Features, teacher: Features) -> torch.Tensor:
        return cosine_feature_loss(student, teacher, self.eps, self.reduction)


LOSSES = {"mse": mse_loss, "l1": l1_loss, "charbonnier": charbonnier_loss, "ssim": ssim_loss}


_clip_segments: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()      # module -> its segments (the walk costs > 1 ms)


def clip_grad_norm_(module_or_parameters, max_norm: float, refresh: bool = False) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for the 2-norm, in place: every gradient is scaled by ``max_norm / (total_norm + 1e-6)``
    when that is below 1 and left untouched otherwise.  Returns the total norm as a 0-dim tensor on the gradients' device; the
    decision is taken on the device, so the call never synchronises with the host.

    Given a module, every bucketed network inside whose ``.grad`` tensors are the views of its last gradient bucket (the plain
    zero_grad -> backward -> step loop) costs two reduction launches and one scale launch on the bucket in place; loose
    parameters, accumulated gradients and a plain iterable of parameters go per tensor.  The sums are taken in double from
    exact squares.  Gradients on the CPU defer to ``torch.nn.utils.clip_grad_norm_``.  In a data-parallel run a parameter outside
    the bucketed networks that carries a gradient raises: its gradient is not synchronised, so the ranks would scale differently.

    A module's split into bucketed networks and loose parameters is worked out on the first call and kept (as ``AGEM`` and ``EWC``
    keep theirs from construction); ``refresh=True`` repeats it after parameters were added to or removed from the module."""
    if isinstance(module_or_parameters, nn.Module):
        segs = None if refresh else _clip_segments.get(module_or_parameters)
        if segs is None:
            segs = _clip_segments[module_or_parameters] = segments_of(module_or_parameters)
        params = [p for sg in segs for _, p in sg.named]
    else:
        params = [module_or_parameters] if isinstance(module_or_parameters, torch.Tensor) else list(module_or_parameters)
        segs = [Segment(None, [(str(i), p) for i, p in enumerate(params)])]
    grads = [p.grad for p in params if p.grad is not None]
    if not grads or not grads[0].is_cuda:
        return torch.nn.utils.clip_grad_norm_(params, max_norm)
    dev = grads[0].device
    pairs = grad_pairs(segs, None, "clip_grad_norm_")
    acc = torch.empty(5, dtype=torch.float64, device=dev)        # the first moments call writes the slots that are read
    norm = torch.empty((), dtype=torch.float32, device=dev)
    with _nvq.device_guard(dev):
        sum_moments(pairs, acc, _engine.workspace(dev))
        for g, _, dst in pairs:
            _nvq.bucket_clip(g, acc, float(max_norm), norm)
            if dst is not None:
                dst.copy_(g.view(dst.shape))
    return norm


# ------------------------------------------------------------------------------------------------ PPO loss (section 26)
PPO_STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")


def ppo_loss_composition(x: torch.Tensor, heads: Sequence[int], actions: torch.Tensor, old_log_probs: torch.Tensor,
                         advantages: torch.Tensor, returns: torch.Tensor, clip_ratio: float, value_coef: float, entropy_coef: float,
                         adv_stats: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float64):
    """The rule of ``ppo_loss`` as a differentiable torch composition in ``dtype`` on x's device -> (loss, stats (6,)).  ``x``: the
    (M, P) head outputs, or the forward's tuple (logits_0, .., value (M, 1)); with the tuple every head's gradient reaches its
    Linear as a contiguous tensor, as in a loop written on the forward's outputs directly."""
    if isinstance(x, torch.Tensor):
        x = x.to(dtype)
        offs = [sum(heads[:j]) for j in range(len(heads) + 1)]
        parts = [x[:, offs[j]:offs[j + 1]] for j in range(len(heads))] + [x[:, offs[-1]:offs[-1] + 1]]
    else:
        parts = [p.to(dtype) for p in x]
    adv, old, ret = advantages.reshape(-1).to(dtype), old_log_probs.reshape(-1).to(dtype), returns.reshape(-1).to(dtype)
    mean, std = (adv.mean(), adv.std()) if adv_stats is None else (adv_stats[0].to(dtype), adv_stats[1].to(dtype))
    adv = (adv - mean) / (std + 1e-8)
    a = actions.long()
    new, ent = 0, 0
    for j, logits in enumerate(parts[:-1]):
        # the operations of torch.distributions.Categorical(logits=), so that fp32 results are those of a loop written with it
        lp = logits - logits.logsumexp(dim=-1, keepdim=True)
        new = new + lp.gather(1, a[:, j:j + 1])[:, 0]
        ent = ent + (-(lp * torch.softmax(lp, dim=-1)).sum(-1)).mean()
    value = parts[-1].squeeze(-1)
    log_ratio = new - old
    ratio = log_ratio.exp()
    pol = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip_ratio, 1 + clip_ratio) * adv).mean()
    val = ((value - ret) ** 2).mean()
    loss = pol + value_coef * val - entropy_coef * ent
    with torch.no_grad():
        stats = torch.stack([loss, pol, val, ent, ((ratio - 1) - log_ratio).mean(),
                             ((ratio - 1).abs() > clip_ratio).to(dtype).mean()]).detach()
    return loss, stats


class _PPOLossFn(torch.autograd.Function):
    """nvq_ppo_loss: the forward writes the loss, the statistics and the gradient; the backward scales the stored gradient.  The head
    outputs arrive as one (M, P) tensor or as the forward's tuple; the tuple's gradients go back as contiguous tensors, so the
    Linear layers behind them run their GEMMs on dense operands."""

    @staticmethod
    def forward(ctx, actions, old_log_probs, advantages, returns, adv_stats, heads, clip_ratio, value_coef, entropy_coef, *parts):
        xa = (parts[0] if len(parts) == 1 else torch.cat([p.detach() for p in parts], dim=-1)).detach().float().contiguous()
        M = xa.shape[0]
        f = lambda t: t.detach().reshape(-1).float().contiguous()      # noqa: E731
        adv = f(advantages)
        grad = torch.empty_like(xa)
        out = torch.empty(6, dtype=torch.float64, device=xa.device)
        with _nvq.device_guard(xa.device):
            if adv_stats is None:
                adv_stats = torch.empty(2, dtype=torch.float64, device=xa.device)
                _nvq.abr_adv_stats(adv, adv_stats)
            _nvq.ppo_loss(xa, actions.detach().reshape(M, -1).int().contiguous(), f(old_log_probs), adv,
                          adv_stats.detach().double().contiguous(), f(returns), heads, clip_ratio, value_coef, entropy_coef, grad, out)
        ctx.save_for_backward(grad)
        ctx.meta = [(p.shape[-1], p.dtype) for p in parts]
        loss, stats = out[0], out
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss, stats

    @staticmethod
    def backward(ctx, go, _gs):
        (grad,) = ctx.saved_tensors
        g = grad * go.detach().to(grad.dtype)
        if len(ctx.meta) == 1:
            outs = [g.to(ctx.meta[0][1])]
        else:
            outs = [piece.contiguous().to(dt) for piece, (_, dt) in zip(torch.split(g, [w for w, _ in ctx.meta], dim=-1), ctx.meta)]
        return (None,) * 9 + tuple(outs)


def ppo_loss(head_outputs, actions: torch.Tensor, old_log_probs: torch.Tensor, advantages: torch.Tensor, returns: torch.Tensor,
             clip_ratio: float, value_coef: float, entropy_coef: float, adv_stats: Optional[torch.Tensor] = None,
             heads: Optional[Sequence[int]] = None, return_stats: bool = False):
    """The PPO loss over M samples: policy + value_coef * value - entropy_coef * entropy with
    policy = -mean(min(r A, clamp(r, 1 - clip, 1 + clip) A)), r = exp(new log-prob - old), A = (adv - mean) / (std + 1e-8),
    value = mean((v - returns)^2), entropy = the sum over the heads of the mean entropy.

    ``head_outputs``: what the actor-critic's forward returns, a sequence (logits_0 (M, n_0), .., value (M, 1)), or one (M, P)
    tensor of the same columns with ``heads=(n_0, ..)``.  ``actions`` (M, heads) integers; ``advantages`` raw: ``adv_stats`` = a
    2-element float64 tensor {mean, unbiased std} (``None``: formed here, on the device by one reduction launch).
    On HIP tensors this is one autograd node (nvq_ppo_loss: the loss, the statistics and the gradient from one pass, per sample
    in double, bit-reproducible); its backward scales the stored gradient by ``grad_output``.  CPU tensors take the float64 torch
    composition.  The loss is a float64 scalar; ``return_stats``: also a (6,) float64 tensor in the order of ``PPO_STATS``."""
    if isinstance(head_outputs, torch.Tensor):
        if heads is None:
            raise ValueError("ppo_loss: a single head_outputs tensor needs heads=(n_0, ...)")
        parts = (head_outputs,)
    else:
        parts = tuple(head_outputs)
        if heads is None:
            heads = [int(t.shape[-1]) for t in parts[:-1]]
    heads = tuple(int(n) for n in heads)
    M, P = parts[0].shape[0], sum(int(t.shape[-1]) for t in parts)
    if any(t.dim() != 2 or t.shape[0] != M for t in parts) or P != sum(heads) + 1 or M < 1 or \
            (len(parts) > 1 and [int(t.shape[-1]) for t in parts] != list(heads) + [1]):
        raise RuntimeError(f"ppo_loss: head outputs {[tuple(t.shape) for t in parts]} are not (M, n_j) for heads {heads} and (M, 1)")
    if actions.numel() != M * len(heads) or old_log_probs.numel() != M or advantages.numel() != M or returns.numel() != M:
        raise RuntimeError("ppo_loss: actions / old_log_probs / advantages / returns do not hold M samples")
    if not parts[0].is_cuda:
        loss, stats = ppo_loss_composition(parts[0] if len(parts) == 1 else parts, heads, actions.reshape(M, -1), old_log_probs,
                                           advantages, returns, clip_ratio, value_coef, entropy_coef, adv_stats)
    else:
        loss, stats = _PPOLossFn.apply(actions, old_log_probs, advantages, returns, adv_stats, heads, float(clip_ratio),
                                       float(value_coef), float(entropy_coef), *parts)
    return (loss, stats) if return_stats else loss
