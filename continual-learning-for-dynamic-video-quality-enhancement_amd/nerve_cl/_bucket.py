"""Flat parameter / gradient buckets shared by the HIP-backed networks (SuperResolutionNet,
LightweightSuperResolution, FrameRecoveryNet).

Every such network is ONE autograd node whose backward writes all parameter gradients into one flat fp32 bucket
(16-byte aligned slots).  That bucket is

  * what a data-parallel run all-reduces (``nerve_cl.parallel`` installs ``_grad_bucket_hook``),
  * what ``EWC.compute_fisher`` squares and accumulates (``_last_grad_bucket``: no per-tensor ``cat``),
  * where the EWC penalty gradient ``lambda * F * (theta - theta*)`` is added by ONE kernel after the all-reduce
    (``_deferred_adds``, filled by the penalty's autograd node, drained by the network's backward) instead of 131
    ``AccumulateGrad`` additions (reference nerve_cl/continual/ewc.py:225-232 + experiments/train_continual.py:56-57).

For the last point the parameters themselves must be readable as one flat tensor in the same layout: ``flat_theta()``
re-homes every ``param.data`` as a view of one persistent buffer (checked by address on every call, rebuilt after
``.to()`` / ``deepcopy``; in-place optimizer and ``load_state_dict`` updates keep it valid).

Below the class is what the consumers of the gradient bucket share (EWC, SynapticIntelligence, AGEM, ``ops.clip_grad_norm_``,
``optim.BucketAdam``); ``BucketedNet.grad_alias_mask()`` is the one place that compares addresses.
"""
from __future__ import annotations

import weakref
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn

from nerve_cl import _nvq, parallel


class _Token:
    """lives exactly as long as the autograd node of one forward does"""
    __slots__ = ("__weakref__",)


_live_nets: "weakref.WeakSet" = weakref.WeakSet()     # every live BucketedNet: nerve_cl.optim finds a parameter's network here


class BucketedNet(nn.Module):
    """Mixin-style base: bucket layout, gradient bucket, flat parameter view, deferred bucket additions."""

    def __setstate__(self, state) -> None:
        super().__setstate__(state)
        _live_nets.add(self)                   # a deepcopy / unpickled network never ran _init_bucket

    def _init_bucket(self) -> None:
        _live_nets.add(self)
        self._param_names: List[str] = [n for n, _ in self.named_parameters()]
        self._grad_bucket_hook = None          # data-parallel all-reduce (nerve_cl.parallel)
        self._last_grad_bucket: Optional[torch.Tensor] = None
        self._theta_flat: Optional[torch.Tensor] = None
        self._layout: Optional[Tuple[Dict[str, Tuple[int, int]], int]] = None
        self._pending = None                   # weakref to the token of the latest forward-with-grad (see _mark_awaiting)
        self._deferred_adds: list = []         # (lam, star_flat, fisher_flat, scale_dev) to add into the next bucket

    # ------------------------------------------------------------------ caches of the module tree
    def _invalidate_module_caches(self) -> None:
        """A sub-module was added or replaced (``nn.SyncBatchNorm.convert_sync_batchnorm`` re-adds every child of the network
        with add_module): the cached parameter / buffer slots, the bucket layout, the parameter names, the backward plans and
        the synchronised-BatchNorm list are rebuilt on their next use."""
        d = self.__dict__
        for k in ("_slot_cache", "_sync_cache", "_plan_cache", "_alias_cache"):
            d.pop(k, None)
        if "_layout" in d:
            d["_layout"] = None
        if "_param_names" in d:
            d["_param_names"] = [n for n, _ in self.named_parameters()]

    def add_module(self, name: str, module: Optional[nn.Module]) -> None:
        super().add_module(name, module)
        self._invalidate_module_caches()

    def __setattr__(self, name: str, value) -> None:
        super().__setattr__(name, value)
        if isinstance(value, nn.Module):
            self._invalidate_module_caches()

    def _sync_bn_groups(self) -> Dict[str, object]:
        """{holder name: process group} of the BatchNorm holders that synchronise in this pass: the nn.SyncBatchNorm holders
        (nn.SyncBatchNorm.convert_sync_batchnorm, parallel.enable_data_parallel(sync_bn=True)), in a training pass, when
        torch.distributed is initialised and the holder's group (None = WORLD) has more than one rank; {} otherwise (the
        unsynchronised path).  The holders are found once per module tree (see _invalidate_module_caches)."""
        c = self.__dict__.get("_sync_cache")
        if c is None:
            c = [(n, m) for n, m in self.named_modules() if isinstance(m, nn.SyncBatchNorm)]
            self.__dict__["_sync_cache"] = c
        if not c or not self.training or not dist.is_available() or not dist.is_initialized():
            return {}
        world = dist.group.WORLD
        return {n: m.process_group if m.process_group is not None else world for n, m in c
                if dist.get_world_size(m.process_group) > 1}

    # ------------------------------------------------------------------ layout
    def _slots(self):
        """([(name, owner._parameters, key)], [(name, owner._buffers, key)]) in named_parameters() / named_buffers() order, built
        once.  Every forward and backward needs all ~180 tensors by name; walking the module tree for them (named_parameters +
        named_buffers, ~150 modules) cost 1 ms of the 4 ms continual-learning step.  The owner dicts are looked up per call, so
        a parameter or buffer that is REPLACED (load_state_dict(assign=True), module.to() with swapped tensors) is still
        found; a sub-module added or replaced through add_module / attribute assignment drops the cache."""
        c = self.__dict__.get("_slot_cache")
        if c is None:
            def locate(name: str, kind: str):
                path, _, key = name.rpartition(".")
                mod = self.get_submodule(path) if path else self
                return (name, getattr(mod, kind), key)
            c = ([locate(n, "_parameters") for n, _ in self.named_parameters()],
                 [locate(n, "_buffers") for n, _ in self.named_buffers()])
            self.__dict__["_slot_cache"] = c
        return c

    def _named_params(self):
        """list(self.named_parameters()) without the module-tree walk"""
        return [(n, d[k]) for n, d, k in self._slots()[0]]

    def _tensor_dict(self) -> Dict[str, torch.Tensor]:
        ps, bs = self._slots()
        d = {n: o[k].data for n, o, k in ps}
        for n, o, k in bs:
            d[n] = o[k]
        return d

    def _bucket_layout(self) -> "Tuple[Dict[str, Tuple[int, int]], int]":
        """{name: (offset, numel)} with 16-byte aligned offsets, total floats."""
        if self._layout is None:
            lay, off = {}, 0
            for n, p in self.named_parameters():
                lay[n] = (off, p.numel())
                off += (p.numel() + 3) // 4 * 4
            self._layout = (lay, off)
        return self._layout

    def _bucket_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        lay, _ = self._bucket_layout()
        shapes = {n: p.shape for n, p in self._named_params()}
        return {n: flat[o:o + k].view(shapes[n]) for n, (o, k) in lay.items()}

    def _new_grad_bucket(self):
        _, total = self._bucket_layout()
        dev = self._named_params()[0][1].device
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        return flat, self._bucket_views(flat)

    def grad_alias_mask(self) -> Optional[List[bool]]:
        """Per parameter, in bucket order: is its ``.grad`` the fp32 view of ``_last_grad_bucket`` at its slot (the plain
        zero_grad -> backward -> step loop; not after gradient accumulation)?  None without a usable bucket: none yet, or one on
        another device, of another size or type.  The bucket IS the gradients when ``mask is not None and all(mask)``."""
        bucket = self._last_grad_bucket
        if bucket is None:
            return None
        c = self.__dict__.get("_alias_cache")          # [(owner._parameters, key, byte offset of the slot)], see _slots()
        if c is None:
            c = [(d, k, 4 * o) for (_, d, k), (o, _) in zip(self._slots()[0], self._bucket_layout()[0].values())]
            self.__dict__["_alias_cache"] = c
        d0, k0, _ = c[0]
        f32 = torch.float32
        if bucket.device != d0[k0].device or bucket.numel() != self._bucket_layout()[1] or bucket.dtype != f32:
            return None
        base = bucket.data_ptr()                       # every step runs this loop: one .grad read per parameter
        return [(g := d[k].grad) is not None and g.data_ptr() == base + o and g.dtype is f32 for d, k, o in c]

    # ------------------------------------------------------------------ flat parameters
    def flat_theta(self) -> torch.Tensor:
        """All parameters as one flat fp32 tensor in bucket layout (padding = 0); the parameters are views of it."""
        lay, total = self._bucket_layout()
        flat = self._theta_flat
        named = self._named_params()
        dev = named[0][1].device
        ok = flat is not None and flat.device == dev
        if ok:
            base = flat.data_ptr()
            for n, p in named:
                if p.dtype != torch.float32 or p.data_ptr() != base + 4 * lay[n][0] or not p.is_contiguous():
                    ok = False
                    break
        if not ok:
            flat = torch.zeros(total, dtype=torch.float32, device=dev)
            with torch.no_grad():
                for n, p in named:
                    o, k = lay[n]
                    v = flat[o:o + k].view(p.shape)
                    v.copy_(p.data)
                    p.data = v
            self._theta_flat = flat
        return flat

    # ------------------------------------------------------------------ "is my backward still to come?"
    def _mark_awaiting(self, ctx) -> None:
        """Called by the network's autograd Function in forward when gradients are needed.  The token hangs on the node's
        ctx: if the graph is dropped without a backward (a validation forward outside no_grad), the token dies with it and
        the network stops 'awaiting' - a penalty gradient is then never parked for a backward that will not happen."""
        ctx._nvq_token = _Token()
        self._pending = weakref.ref(ctx._nvq_token)
        self._deferred_adds = []               # leftovers could only come from a pass that was abandoned half-way

    @property
    def _awaiting_backward(self) -> bool:
        return self._pending is not None and self._pending() is not None

    # ------------------------------------------------------------------ backward epilogue
    def _finish_bucket(self, flat: torch.Tensor) -> None:
        """Called by the network's backward once every gradient is in `flat`: data-parallel all-reduce, then the
        deferred penalty gradients (identical on every rank, hence after the reduce)."""
        hook = self._grad_bucket_hook
        if hook is not None:
            hook(flat)
        if self._deferred_adds:
            theta = self.flat_theta()
            for lam, star, fisher, scale in self._deferred_adds:
                _nvq.ewc_penalty_grad(theta, star, fisher, lam, scale, flat, True)
            self._deferred_adds = []
        self._pending = None
        self._last_grad_bucket = flat


class Segment:
    """One flat bucket of a module's trainable parameters: either all parameters of one bucketed network (``net`` set: Fisher /
    theta* / A-GEM's reference are stored in that network's gradient-bucket layout, so a kernel over the bucket needs no
    gather) or a plain concatenation of loose parameters (``net`` None: e.g. the engine's ``enhancement_strength``)."""

    def __init__(self, net: Optional[BucketedNet], named: "List[tuple]"):
        self.net, self.named = net, named          # named: [(full name, parameter)]
        self.names = [n for n, _ in named]

    def numel(self) -> int:
        if self.net is not None:
            return self.net._bucket_layout()[1]
        return sum(p.numel() for _, p in self.named)

    def views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self.net is None:
            parts = flat.split([p.numel() for _, p in self.named])
            return {n: v.view(p.shape) for (n, p), v in zip(self.named, parts)}
        local = self.net._bucket_views(flat)
        return {full: local[loc] for (full, _), loc in zip(self.named, self.net._param_names)}

    def theta(self) -> torch.Tensor:
        if self.net is not None:
            return self.net.flat_theta()           # persistent flat view of the parameters: no per-step cat
        return torch.cat([p.detach().reshape(-1).float() for _, p in self.named])

    def aliased(self) -> bool:
        """a bucketed network whose last gradient bucket IS its gradients (``grad_alias_mask``)"""
        mask = self.net.grad_alias_mask() if self.net is not None else None
        return mask is not None and all(mask)

    def grads(self) -> Optional[torch.Tensor]:
        """Flat gradient of the last backward in this segment's layout (None when nothing arrived)."""
        if self.aliased():
            return self.net._last_grad_bucket
        if all(p.grad is None for _, p in self.named):
            return None
        flat = torch.zeros(self.numel(), dtype=torch.float32, device=self.named[0][1].device)
        views = self.views(flat)
        for n, p in self.named:
            if p.grad is not None:
                views[n].copy_(p.grad.detach())
        return flat


def segments_of(model: nn.Module) -> "List[Segment]":
    """Split model.named_parameters() (requires_grad only, reference ewc.py:67-71) into bucketed networks + loose rest.  A
    network with a frozen parameter is no segment: its parameters are loose.  The walk costs > 1 ms: consumers keep the result."""
    owner: Dict[int, "tuple[BucketedNet, str]"] = {}
    for prefix, m in model.named_modules():
        if isinstance(m, BucketedNet) and all(p.requires_grad for p in m.parameters()):
            for p in m.parameters():
                owner.setdefault(id(p), (m, prefix))
    segs: "Dict[int, Segment]" = {}
    order: "List[Segment]" = []
    loose: "List[tuple]" = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        own = owner.get(id(p))
        if own is None:
            loose.append((name, p))
            continue
        net = own[0]
        if id(net) not in segs:
            segs[id(net)] = Segment(net, [])
            order.append(segs[id(net)])
        segs[id(net)].named.append((name, p))
    for sg in order:
        sg.names = [n for n, _ in sg.named]
        assert len(sg.named) == len(sg.net._param_names)
    if loose:
        order.append(Segment(None, loose))
    return order


def flat_grad(g: torch.Tensor) -> "Tuple[torch.Tensor, Optional[torch.Tensor]]":
    """(flat, dst): the gradient's own memory as ``view(-1)`` and None when it is contiguous and fp32 (on the CPU, where the
    torch compositions run: of any type), else a contiguous fp32 copy and ``g``, for a caller that changes the copy to write back."""
    g = g.detach()
    want = torch.float32 if g.is_cuda else g.dtype
    if g.dtype == want and g.is_contiguous():
        return g.view(-1), None
    return g.to(want).contiguous().view(-1), g


def refuse_loose_gradients(named, what: str, group=None) -> None:
    """``named``: the loose (name, parameter) pairs.  Data parallel: the bucket hook leaves the same averaged gradient on every
    rank, but nothing synchronises a gradient outside the bucketed networks - the ranks would form different sums and drift."""
    if parallel.world_size(group) > 1:
        for n, p in named:
            if p.grad is not None:
                raise RuntimeError(f"{what}: parameter {n!r} lies outside the bucketed networks and carries a gradient; this "
                                   "package does not synchronise such gradients over the ranks, so every rank would compute "
                                   "a different result")


def grad_pairs(segs: "List[Segment]", refs: "Optional[List[torch.Tensor]]", what: str, group=None) -> "List[Tuple]":
    """[(g, r, dst)]: the flat gradients the kernels update in place, each with its slice of the reference (None without
    ``refs``).  A bucketed network whose ``.grad`` tensors are the views of its last gradient bucket is ONE pair, the bucket
    itself; otherwise (loose parameters, gradients accumulated over several backwards) one pair per parameter that has a
    gradient, with ``flat_grad``'s ``dst``."""
    out = []
    for i, sg in enumerate(segs):
        if sg.net is None:
            refuse_loose_gradients(sg.named, what, group)
        ref = refs[i] if refs is not None else None
        if sg.aliased():
            out.append((sg.net._last_grad_bucket, ref, None))
            continue
        views = sg.views(ref) if ref is not None else None
        for n, p in sg.named:
            if p.grad is not None and p.numel():
                g, dst = flat_grad(p.grad)
                out.append((g, views[n].view(-1) if views is not None else None, dst))
    return out


def sum_moments(pairs, acc: torch.Tensor, ws: torch.Tensor, coefficient: bool = False) -> None:
    """acc[0..2] = g.r, r.r, g.g over ``pairs`` (``grad_pairs`` tuples, or bare flat gradients: g.g only), one ``nvq_bucket_moments``
    each, all but the first accumulating; ``coefficient``: the last one forms A-GEM's c in acc[3].  Under the caller's guard."""
    last = len(pairs) - 1
    for k, pair in enumerate(pairs):
        g, r = pair[:2] if isinstance(pair, tuple) else (pair, None)
        _nvq.bucket_moments(g, r, acc, ws, accumulate=k > 0, coefficient=coefficient and k == last)
