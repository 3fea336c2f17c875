"""Averaged Gradient Episodic Memory (A-GEM, Chaudhry et al. 2019) on the flat gradient buckets.

The step's gradient ``g`` is compared with the gradient ``r`` of the same loss on a batch drawn from the episodic memory; when
they conflict (``g.r < 0``) the conflicting component is removed, ``g <- g - (g.r / r.r) r``.  On HIP tensors the three inner
products, the decision and the update are the kernels of csrc/bucket_ops.hip: per bucketed network one
``nvq_bucket_moments`` (two launches) and one ``nvq_bucket_project`` running on the network's gradient bucket in place, the
coefficient staying on the device - ``project()`` never synchronises with the host.  ``nerve_cl.ops.clip_grad_norm_`` is the
same reduction followed by a scale and shares the segment walk below.

A module on the CPU takes the torch composition of the same formulas in float64, so the class also works on plain modules.
"""
from __future__ import annotations

import weakref
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq, parallel
from nerve_cl.continual.ewc import SynapticIntelligence, _Segment, segments_of

_bucket_is_grad = SynapticIntelligence._bucket_is_grad


def _refuse_loose_gradients(sg: _Segment, what: str, group) -> None:
    """Data parallel: the bucket hook leaves the same averaged gradient on every rank, but nothing synchronises the gradient of
    a parameter outside the bucketed networks - the ranks would form different sums and drift apart."""
    if sg.net is None and parallel.world_size(group) > 1:
        for n, p in sg.named:
            if p.grad is not None:
                raise RuntimeError(f"{what}: parameter {n!r} lies outside the bucketed networks and carries a gradient; this "
                                   "package does not synchronise such gradients over the ranks, so every rank would compute "
                                   "a different result")


def grad_pairs(segs: "List[_Segment]", refs: "Optional[List[torch.Tensor]]", what: str, group=None) -> "List[Tuple]":
    """[(g, r, dst)]: the flat fp32 gradients the kernels update in place, each with its slice of the reference (None without
    ``refs``).  A bucketed network whose ``.grad`` tensors are the views of its last gradient bucket is ONE pair, the bucket
    itself; otherwise (loose parameters, gradients accumulated over several backwards) one pair per parameter that has a
    gradient.  ``dst`` is None, or the ``.grad`` a non-fp32 / non-contiguous gradient's working copy ``g`` is copied back to."""
    out = []
    for i, sg in enumerate(segs):
        _refuse_loose_gradients(sg, what, group)
        ref = refs[i] if refs is not None else None
        if sg.net is not None and _bucket_is_grad(sg):
            out.append((sg.net._last_grad_bucket, ref, None))
            continue
        views = sg.views(ref) if ref is not None else None
        for n, p in sg.named:
            if p.grad is None or p.numel() == 0:
                continue
            g = p.grad.detach()
            want = torch.float32 if g.is_cuda else g.dtype        # the kernels are fp32; the CPU composition takes any type
            inplace = g.dtype == want and g.is_contiguous()
            flat = g.view(-1) if inplace else g.to(want).contiguous().view(-1)
            out.append((flat, views[n].view(-1) if views is not None else None, None if inplace else g))
    return out


class AGEM:
    """``AGEM(model, memory=None, ref_batch_size=8)``; in a training step::

        agem.compute_reference(loss_fn)       # r: gradient on a batch from the memory (False while it is empty)
        loss_fn(model(lr), hr).backward()     # g
        agem.project()                        # g <- g - (g.r / r.r) r  when g.r < 0
        optimizer.step()

    ``stats`` (float64, on the model's device) = [g.r, r.r, g.g, coefficient c, number of projections so far] of the last
    ``project()``.  Parameters without a gradient take no part in a projection (neither in the sums nor in the update).

    Data parallel (``nerve_cl.parallel``): ``g`` and ``r`` both leave the bucket hook rank-averaged, so every rank forms the
    same ``c`` without a further collective; a loose parameter that carries a gradient raises (see above)."""

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
                _refuse_loose_gradients(sg, "AGEM.capture_reference", self.process_group)
                if self._hip and sg.net is not None and _bucket_is_grad(sg):
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
        ws = _engine.workspace(self._dev)
        last = len(pairs) - 1
        with _nvq.device_guard(self._dev):
            for k, (g, r, _) in enumerate(pairs):
                _nvq.bucket_moments(g, r, self.stats, ws, accumulate=k > 0, coefficient=k == last)
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


_clip_segments: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()      # module -> its segments (the walk costs > 1 ms)


def clip_grad_norm_(target, max_norm: float, refresh: bool = False) -> torch.Tensor:
    """``nerve_cl.ops.clip_grad_norm_`` (documented there)."""
    if isinstance(target, nn.Module):
        segs = None if refresh else _clip_segments.get(target)
        if segs is None:
            segs = _clip_segments[target] = segments_of(target)
        params = [p for sg in segs for _, p in sg.named]
    else:
        params = [target] if isinstance(target, torch.Tensor) else list(target)
        segs = [_Segment(None, [(str(i), p) for i, p in enumerate(params)])]
    grads = [p.grad for p in params if p.grad is not None]
    if not grads or not grads[0].is_cuda:
        return torch.nn.utils.clip_grad_norm_(params, max_norm)
    dev = grads[0].device
    pairs = grad_pairs(segs, None, "clip_grad_norm_")
    acc = torch.empty(5, dtype=torch.float64, device=dev)        # the first moments call writes the slots that are read
    norm = torch.empty((), dtype=torch.float32, device=dev)
    ws = _engine.workspace(dev)
    with _nvq.device_guard(dev):
        for k, (g, _, _) in enumerate(pairs):
            _nvq.bucket_moments(g, None, acc, ws, accumulate=k > 0)
        for g, _, dst in pairs:
            _nvq.bucket_clip(g, acc, float(max_norm), norm)
            if dst is not None:
                dst.copy_(g.view(dst.shape))
    return norm
