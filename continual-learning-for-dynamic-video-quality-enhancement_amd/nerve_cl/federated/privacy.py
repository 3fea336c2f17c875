"""Differential privacy for federated training: the reference's ``PrivacyConfig`` / ``DPOptimizer`` / ``make_private`` surface
(reference nerve_cl/federated/privacy.py) with the clip-and-noise step as two libnvq launches over the gradient bucket.

The rule is the reference's: every parameter's gradient is clipped on its own, ``g *= min(C / (|g| + 1e-6), 1)``, then
``g += N(0, 1) * noise_multiplier * C / batch_size``.  The reference loops over ~130 tensors with three launches and one host
comparison each; here the gradients of a HIP-backed network are one flat bucket whose slots are the tensors, and a step is
``nvq_dp_segment_norms`` + ``nvq_dp_clip_noise`` (csrc/federated.hip) with nothing read back.

Noise stream.  The parameters form *segments* (``_bucket.segments_of``: each bucketed network, then the loose rest); a segment is
laid out as its network's bucket, or - loose parameters, CPU modules - its parameters in order, each padded to a multiple of 4
floats.  Element i of segment j at step t (0-based) takes ``_philox.normals(seed, t * len(segments) + j, ...)[i]``: a function of
(seed, step, segment, element) only, the same on the device and on the CPU up to fp32 rounding of the normal itself.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import Segment, segments_of
from nerve_cl.federated import _philox

__all__ = ["PrivacyConfig", "compute_noise_multiplier", "DPOptimizer", "make_private", "get_privacy_spent"]


@dataclass
class PrivacyConfig:
    """epsilon / delta: the privacy budget; max_grad_norm: the per-tensor clipping bound C; noise_multiplier: sigma / C"""
    epsilon: float = 8.0
    delta: float = 1e-5
    max_grad_norm: float = 1.0
    noise_multiplier: float = 1.0


def compute_noise_multiplier(epsilon: float, delta: float, sample_rate: float, epochs: int) -> float:
    """the reference's simplified Gaussian-mechanism bound: sqrt(2 ln(1.25 / delta)) sqrt(epochs / sample_rate) / epsilon"""
    steps = epochs / sample_rate
    return math.sqrt(2 * math.log(1.25 / delta)) * math.sqrt(steps) / epsilon


def get_privacy_spent(steps: int, noise_multiplier: float, sample_rate: float, delta: float) -> float:
    """the reference's simplified accounting: steps q^2 / (2 sigma^2) (``delta`` does not enter it)"""
    return steps * sample_rate ** 2 / (2 * noise_multiplier ** 2)


def _padded_layout(numels: List[int]) -> "Tuple[List[int], int]":
    offs, off = [], 0
    for k in numels:
        offs.append(off)
        off += (k + 3) // 4 * 4
    return offs, off


class _Seg:
    """one segment of the DP step: its parameters, the padded layout, the device tables (built on first use per device)"""

    def __init__(self, sg: Segment):
        self.sg = sg
        self.params = [p for _, p in sg.named]
        if sg.net is not None:
            lay, self.total = sg.net._bucket_layout()
            self.offsets = [lay[n][0] for n in sg.net._param_names]
        else:
            self.offsets, self.total = _padded_layout([p.numel() for p in self.params])
        self.numels = [p.numel() for p in self.params]
        self.table: Optional[_nvq.DpTable] = None
        self.staging: Optional[torch.Tensor] = None

    def device_table(self, dev) -> "_nvq.DpTable":
        if self.table is None or self.table.sq.device != dev:
            self.table = _nvq.DpTable(self.offsets, self.numels, dev)
        return self.table


class DPOptimizer:
    """``DPOptimizer(optimizer, model, config, batch_size, sample_size, seed=None)``: the reference's wrapper.  ``step()`` clips
    and noises every gradient (see the module text), calls ``optimizer.step()`` and counts ``steps``; ``zero_grad()`` forwards.
    ``optimizer`` is any torch optimizer or ``nerve_cl.optim.BucketAdam`` / ``BucketAdamW``.  ``seed`` (None: drawn from
    ``random``) keys the noise; every step and every segment draws from a stream of its own."""

    def __init__(self, optimizer, model: nn.Module, config: PrivacyConfig, batch_size: int, sample_size: int,
                 seed: Optional[int] = None, *, _segments: "Optional[List[_Seg]]" = None):
        self.optimizer = optimizer
        self.model = model
        self.config = config
        self.batch_size = batch_size
        self.sample_rate = batch_size / sample_size
        self.noise_multiplier = config.noise_multiplier
        self.steps = 0
        self.seed = random.getrandbits(62) if seed is None else int(seed)
        if self.seed < 0:
            raise ValueError("seed is non-negative")
        # _segments: the segments of `model` with their device tables, kept by a caller that builds many wrappers (FederatedTrainer)
        self._segs = _segments if _segments is not None else [_Seg(sg) for sg in segments_of(model)]
        self.last_launches = 0                     # libnvq launches of the last step's clip-and-noise (a host integer)

    @property
    def noise_scale(self) -> float:
        return self.noise_multiplier * self.config.max_grad_norm / self.batch_size

    def noise_offset(self, segment: int, step: Optional[int] = None) -> int:
        """the ``offset`` of the stream that ``segment`` draws from at ``step`` (default: the step about to run)"""
        return (self.steps if step is None else step) * len(self._segs) + segment

    @torch.no_grad()
    def step(self) -> None:
        self.last_launches = 0
        for j, seg in enumerate(self._segs):
            if all(p.grad is None for p in seg.params):
                continue
            dev = seg.params[0].device
            if dev.type == "cuda":
                with _nvq.device_guard(dev):
                    self._device_segment(seg, dev, self.noise_offset(j))
            else:
                self._host_segment(seg, self.noise_offset(j))
        self.optimizer.step()
        self.steps += 1

    def _device_segment(self, seg: _Seg, dev, offset: int) -> None:
        C, scale = float(self.config.max_grad_norm), float(self.noise_scale)
        table = seg.device_table(dev)
        ws = _engine.workspace(dev)
        missing = [p.grad is None for p in seg.params]
        if seg.sg.aliased() and not any(missing):
            bucket = seg.sg.net._last_grad_bucket          # the gradients themselves: two launches, nothing copied
            _nvq.dp_segment_norms(bucket, table, ws)
            _nvq.dp_clip_noise(bucket, table, C, scale, self.seed, offset)
            self.last_launches += 2
            return
        # loose parameters, accumulated or partial gradients: the same two launches on a staging bucket in the padded layout
        if seg.staging is None or seg.staging.device != dev:
            seg.staging = torch.zeros(seg.total, dtype=torch.float32, device=dev)
        flat = seg.staging
        views = [flat[o:o + k].view(p.shape) for o, k, p in zip(seg.offsets, seg.numels, seg.params)]
        for v, p in zip(views, seg.params):
            if p.grad is not None:
                v.copy_(p.grad)
            else:
                v.zero_()
        _nvq.dp_segment_norms(flat, table, ws)
        _nvq.dp_clip_noise(flat, table, C, scale, self.seed, offset)
        self.last_launches += 2
        for v, p in zip(views, seg.params):
            if p.grad is not None:                         # a parameter without a gradient stays without one, as in the reference
                p.grad.copy_(v)

    def _host_segment(self, seg: _Seg, offset: int) -> None:
        C, scale = float(self.config.max_grad_norm), float(self.noise_scale)
        z = _philox.normals(self.seed, offset, seg.total) if scale != 0.0 else None
        for o, k, p in zip(seg.offsets, seg.numels, seg.params):
            g = p.grad
            if g is None:
                continue
            coef = min(C / (float(g.double().pow(2).sum().sqrt()) + 1e-6), 1.0)
            g.mul_(coef)
            if z is not None:
                noise = torch.from_numpy(np.ascontiguousarray(z[o:o + k])).to(g.dtype).view(g.shape)
                g.add_(noise, alpha=scale)

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.optimizer.zero_grad(set_to_none=set_to_none)


def make_private(model: nn.Module, optimizer, data_loader, config: PrivacyConfig):
    """(model, DPOptimizer, data_loader): the reference's behaviour without ``opacus`` - the simple per-tensor DP optimizer with the
    loader's batch size and the size of its dataset."""
    dp = DPOptimizer(optimizer, model, config, data_loader.batch_size, len(data_loader.dataset))
    return model, dp, data_loader
