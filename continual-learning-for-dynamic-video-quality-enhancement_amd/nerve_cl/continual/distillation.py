"""Teacher/student distillation (reference nerve_cl/continual/distillation.py): after every task the student is deep-copied
into a frozen teacher, and the next task's loss pulls the student's output - and, optionally, its intermediate features -
towards the teacher's.  On HIP tensors the loss terms are the fused kernels of csrc/distill.hip (``nerve_cl.ops.distill_loss``,
``cosine_feature_loss``); on CPU tensors (plain modules) the torch composition of the same formulas.
Works on any module that survives copy.deepcopy."""
from __future__ import annotations

import copy
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from nerve_cl import ops


class DistillationLoss(nn.Module):
    """alpha * mse(student, teacher) + (1 - alpha) * mse(student, target); mse(student, teacher) without a target"""

    def __init__(self, temperature: float = 4.0, alpha: float = 0.5):
        super().__init__()
        self.temperature, self.alpha = temperature, alpha

    def forward(self, student_output, teacher_output, target: Optional[torch.Tensor] = None):
        if student_output.is_cuda:
            return ops.distill_loss(student_output, teacher_output, target, self.alpha)
        d = F.mse_loss(student_output, teacher_output.detach())
        if target is None:
            return d
        return self.alpha * d + (1 - self.alpha) * F.mse_loss(student_output, target)


def _cosine_torch(student, teacher, eps: float) -> torch.Tensor:
    """``ops.cosine_feature_loss`` (mean reduction) as torch ops, for CPU tensors: sqrt(max(a, eps^2)) = max(sqrt(a), eps), with
    a zero (not a 0 * inf) gradient where the norm is clamped"""
    if isinstance(student, torch.Tensor):
        student, teacher = [student], [teacher]
    total = 0.0
    for s, t in zip(student, teacher):
        t = t.detach()
        ns = (s * s).sum(1).clamp_min(eps * eps).sqrt()
        nt = (t * t).sum(1).clamp_min(eps * eps).sqrt()
        total = total + (1.0 - (s * t).sum(1) / (ns * nt)).mean()
    return total / len(student)


def _is_mean_mse(fn) -> bool:
    return isinstance(fn, ops.MSELoss) or (isinstance(fn, nn.MSELoss) and fn.reduction == "mean")


class ContinualDistillation:
    """``compute_loss(inputs, targets, task_loss_fn)`` -> {"task", "distill", "total"}: total = task + distill, every entry
    differentiable; distill is 0 until the first ``register_task()`` makes a teacher.

    ``feature_weight > 0`` (with a teacher): student and teacher are called as ``model(inputs, return_intermediate=True)`` and
    must return ``(output, dict)`` (``SuperResolutionNet``'s signature); total gains ``feature_weight * sum over feature_keys of
    cosine_feature_loss(student[key], teacher[key])`` and the dict a "feature" entry (0 before the first teacher).  A key's
    entry may be a (B, C, H, W) tensor or a list of them.

    ``fold_task=True`` (HIP tensors only; ``task_loss_fn`` must be ``nn.MSELoss`` / ``ops.MSELoss`` with mean reduction,
    anything else raises): task + distill = alpha * mse(s, t) + (2 - alpha) * mse(s, y) comes from ONE ``distill`` launch pair
    instead of three MSE nodes.  Then only "total" is differentiable: "task" and "distill" are detached report values.
    Before the first teacher there is nothing to fold and the step is the plain task loss."""

    def __init__(self, model: nn.Module, temperature: float = 4.0, alpha: float = 0.5, feature_weight: float = 0.0,
                 feature_keys: Sequence[str] = ("aggregated",), fold_task: bool = False):
        if fold_task and not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"ContinualDistillation: fold_task needs alpha in [0, 1], got {alpha}")
        if float(feature_weight) < 0.0:
            raise ValueError(f"ContinualDistillation: feature_weight must be >= 0, got {feature_weight}")
        self.student, self.teacher = model, None
        self.distill_loss = DistillationLoss(temperature, alpha)
        self.feature_weight, self.feature_keys, self.fold_task = float(feature_weight), tuple(feature_keys), bool(fold_task)
        self.task_count = 0
        self.last_output: Optional[torch.Tensor] = None      # the student's (detached) output of the last compute_loss

    def register_task(self) -> None:
        self.teacher = copy.deepcopy(self.student).eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.task_count += 1

    def _forward(self, model, inputs, want_features: bool):
        if not want_features:
            return model(inputs), None
        res = model(inputs, return_intermediate=True)
        if not (isinstance(res, tuple) and len(res) == 2 and isinstance(res[1], dict)):
            raise TypeError("ContinualDistillation: with feature_weight > 0 the model must return (output, dict) for "
                            "return_intermediate=True")
        return res

    def compute_loss(self, inputs, targets, task_loss_fn) -> Dict[str, torch.Tensor]:
        if self.fold_task and not _is_mean_mse(task_loss_fn):
            raise ValueError("ContinualDistillation: fold_task=True folds an MSE task term into the distillation kernel; the "
                             f"criterion must be nn.MSELoss / ops.MSELoss with mean reduction, got {task_loss_fn!r}")
        want_features = self.feature_weight > 0 and self.teacher is not None
        out, inter = self._forward(self.student, inputs, want_features)
        self.last_output = out.detach()
        if self.teacher is None:
            task = task_loss_fn(out, targets)
            losses = {"task": task, "distill": torch.zeros((), device=out.device), "total": task}
            if self.feature_weight > 0:
                losses["feature"] = torch.zeros((), device=out.device)
            return losses
        with torch.no_grad():
            t_out, t_inter = self._forward(self.teacher, inputs, want_features)
        if self.fold_task:
            alpha = self.distill_loss.alpha
            total, d, m = ops._distill_weighted(out, t_out, targets, alpha, 2.0 - alpha, name="ContinualDistillation(fold_task)")
            losses = {"task": m.detach(), "distill": (alpha * d + (1.0 - alpha) * m).detach(), "total": total}
        else:
            task = task_loss_fn(out, targets)
            distill = self.distill_loss(out, t_out, targets)
            losses = {"task": task, "distill": distill, "total": task + distill}
        if want_features:
            feature = None
            for key in self.feature_keys:
                s_f, t_f = inter[key], t_inter[key]
                v = ops.cosine_feature_loss(s_f, t_f) if out.is_cuda else _cosine_torch(s_f, t_f, 1e-8)
                feature = v if feature is None else feature + v
            losses["feature"] = feature
            losses["total"] = losses["total"] + self.feature_weight * feature
        return losses
