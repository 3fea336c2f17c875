"""Averaged Gradient Episodic Memory (A-GEM, Chaudhry et al. 2019) on the flat gradient buckets.

The step's gradient ``g`` is compared with the gradient ``r`` of the same loss on a batch drawn from the episodic memory; when
they conflict (``g.r < 0``) the conflicting component is removed, ``g <- g - (g.r / r.r) r``.  On HIP tensors the three inner
products, the decision and the update are the kernels of csrc/bucket_ops.hip: per bucketed network one
``nvq_bucket_moments`` (two launches) and one ``nvq_bucket_project`` running on the network's gradient bucket in place, the
coefficient staying on the device - ``project()`` never synchronises with the host.  The walk over the segments and their
gradients is ``nerve_cl._bucket.grad_pairs``, which ``nerve_cl.ops.clip_grad_norm_`` (the same reduction followed by a scale) shares.

A module on the CPU takes the torch composition of the same formulas in float64, so the class also works on plain modules.
"""
from __future__ import annotations

from typing import Callable

import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import grad_pairs, refuse_loose_gradients, segments_of, sum_moments


class AGEM:
    """``AGEM(model, memory=None, ref_batch_size=8)``; in a training step::

        agem.compute_reference(loss_fn)       # r: gradient on a batch from the memory (False while it is empty)
        loss_fn(model(lr), hr).backward()     # g
        agem.project()                        # g <- g - (g.r / r.r) r  when g.r < 0
        optimizer.step()

    ``stats`` (float64, on the model's device) = [g.r, r.r, g.g, coefficient c, number of projections so far] of the last
    ``project()``.  Parameters without a gradient take no part in a projection (neither in the sums nor in the update).

    Data parallel (``nerve_cl.parallel``): ``g`` and ``r`` both leave the bucket hook rank-averaged, so every rank forms the
    same ``c`` without a further collective; a loose parameter that carries a gradient raises
    (``nerve_cl._bucket.refuse_loose_gradients``)."""

    def __init__(self, model: nn.Module, memory=None, ref_batch_size: int = 8, process_group=None):
        self.model, self.memory, self.ref_batch_size = model, memory, int(ref_batch_size)
        self.process_group = process_group
        self._segs = segments_of(model)
        first = next(model.parameters())
        self._dev = first.device
        self._hip = self._dev.type == "cuda"
        # the reference gradient: AGEM's own flat buffers in segment layout (bucket padding stays 0); float64 on the CPU, where
        # the parameters may be of any floating type
        rdtype = torch.float32 if self._hip else torch.float64
        self._ref = [torch.zeros(sg.numel(), dtype=rdtype, device=self._dev) for sg in self._segs]
        self._have_ref = False
        self.stats = torch.zeros(5, dtype=torch.float64, device=self._dev)

    # ------------------------------------------------------------------ reference gradient
    def capture_reference(self) -> None:
        """Copy the gradients now in place into the reference buffers (a parameter without a gradient: zeros)."""
        with torch.no_grad():
            for sg, ref in zip(self._segs, self._ref):
                if sg.net is None:
                    refuse_loose_gradients(sg.named, "AGEM.capture_reference", self.process_group)
                if self._hip and sg.aliased():
                    ref.copy_(sg.net._last_grad_bucket)          # a copy: the bucket itself belongs to the next zero_grad
                    continue
                views = sg.views(ref)
                for n, p in sg.named:
                    if p.grad is None:
                        views[n].zero_()
                    else:
                        views[n].copy_(p.grad)
        self._have_ref = True

    def _draw(self):
        if self.memory is None or len(self.memory) == 0:
            return None
        lr, hr, _ = self.memory.sample(batch_size=self.ref_batch_size, device=self._dev)
        return lr, hr

    def compute_reference(self, loss_fn: Callable, batch=None) -> bool:
        """zero_grad -> ``loss_fn(model(lr), hr).backward()`` -> ``capture_reference()`` -> zero_grad on ``batch = (lr, hr)``, or
        on ``ref_batch_size`` samples of the memory.  False (nothing captured) while the memory is empty."""
        if batch is None:
            batch = self._draw()
            if batch is None:
                return False
        lr, hr = batch[0], batch[1]
        self.model.zero_grad()
        loss_fn(self.model(lr), hr).backward()
        self.capture_reference()
        self.model.zero_grad()
        return True

    # ------------------------------------------------------------------ projection
    def project(self) -> None:
        """Between ``loss.backward()`` and ``optimizer.step()``.  Does nothing before a reference was captured."""
        if not self._have_ref:
            return
        pairs = grad_pairs(self._segs, self._ref, "AGEM.project", self.process_group)
        if not pairs:
            return
        if not self._hip:
            return self._project_torch(pairs)
        with _nvq.device_guard(self._dev):
            sum_moments(pairs, self.stats, _engine.workspace(self._dev), coefficient=True)
            for g, r, dst in pairs:
                _nvq.bucket_project(g, r, self.stats)
                if dst is not None:
                    dst.copy_(g.view(dst.shape))

    def _project_torch(self, pairs) -> None:
        """the same formulas in float64 (CPU modules)"""
        with torch.no_grad():
            gr = sum((g.double() * r.double()).sum() for g, r, _ in pairs)
            rr = sum((r.double() * r.double()).sum() for g, r, _ in pairs)
            gg = sum((g.double() * g.double()).sum() for g, r, _ in pairs)
            c = float(gr / rr) if bool(gr < 0) and bool(rr > 0) else 0.0
            self.stats[0], self.stats[1], self.stats[2], self.stats[3] = gr, rr, gg, c
            if c != 0.0:
                self.stats[4] += 1
                for g, r, dst in pairs:
                    out = g if dst is None else dst
                    out.copy_((g.double() - c * r.double()).view(out.shape))

    # ------------------------------------------------------------------ reports
    def cosine(self) -> torch.Tensor:
        """cos(g, r) of the last ``project()``: a 0-dim tensor on the model's device (0 where a norm is 0); no host read."""
        den = torch.sqrt(self.stats[1] * self.stats[2])
        return torch.where(den > 0, self.stats[0] / den, torch.zeros_like(den))

    def num_projections(self) -> int:
        """How many ``project()`` calls changed the gradient so far (this call reads from the device)."""
        return int(self.stats[4].item())
