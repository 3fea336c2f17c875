"""Adam / AdamW on the flat parameter and gradient buckets: update, global-norm clipping and weight EMA in one launch.

Every HIP-backed network keeps its parameters as views of one flat fp32 buffer (``BucketedNet.flat_theta()``) and its backward
leaves every gradient in one flat bucket that ``.grad`` aliases.  ``BucketAdam`` / ``BucketAdamW`` keep ``exp_avg``, ``exp_avg_sq``
and, with ``ema_decay``, an exponential moving average of the weights as flat tensors in the same layout, and a step is ONE
``nvq_adam_step`` launch (csrc/optim.hip) per *run*: a maximal stretch of consecutive bucket slots whose
parameters share a param group and a step count and whose ``.grad`` is the bucket's view (``.data`` is the view of
``flat_theta()`` by construction: ``step()`` calls it first, and it re-homes a parameter that is not).  An all-trainable
network in one group is one launch; a frozen prefix costs one launch for the rest.  Loose parameters, gradients accumulated
over several backwards and non-contiguous gradients take the same kernel per tensor.

The update rule is exactly ``torch.optim.Adam`` / ``AdamW`` with ``amsgrad=False, maximize=False`` (single-tensor form: the bias
corrections are formed on the host in double from an integer step count), and ``state_dict()`` has torch's format: it loads into
``torch.optim.Adam`` / ``AdamW`` and theirs load here.

``max_grad_norm`` clips by the global 2-norm of the gradients this optimizer consumes at no extra pass over them: the squared norm
is reduced once (``nvq_bucket_moments``) and every update launch scales the gradient it reads by ``max_norm / (norm + 1e-6)`` when
that is below 1.  Unlike ``ops.clip_grad_norm_`` the ``.grad`` tensors themselves are left UNSCALED.  Nothing is read back to the
host; ``last_grad_norm`` is a 0-dim tensor on the device.

Parameters on the CPU take a torch composition of the same formulas in fp32 per tensor, so the classes work on plain modules.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.optim import Optimizer

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import BucketedNet, _live_nets, flat_grad, refuse_loose_gradients, sum_moments

__all__ = ["BucketAdam", "BucketAdamW", "Slot", "plan_runs"]


class Slot(NamedTuple):
    """One parameter of a bucketed network as the run planner sees it (bucket order)."""
    group: Optional[int]      # index of its param group; None: not this optimizer's parameter
    step: int                 # updates applied so far
    has_grad: bool            # .grad is not None
    fused: bool               # .grad is the gradient bucket's view at this slot (flat_theta() was just called: .data is its view)


def plan_runs(slots: "Sequence[Slot]") -> "Tuple[List[Tuple[int, int]], List[int]]":
    """-> (runs, singles).  ``runs``: [(first, last)] slot indices, inclusive, of the maximal stretches of consecutive slots that
    are this optimizer's, carry a gradient, are ``fused`` and share group and step count: one launch each, over the slots and the
    padding between them.  ``singles``: the remaining slots that carry a gradient (one launch per tensor).  A slot without a
    gradient, or of another owner, is in neither: it is not touched and its step count does not advance."""
    runs: "List[Tuple[int, int]]" = []
    singles: "List[int]" = []
    start = None
    for i, s in enumerate(slots):
        ok = s.group is not None and s.has_grad and s.fused
        if ok and start is not None and (slots[i - 1].group, slots[i - 1].step) == (s.group, s.step):
            continue
        if start is not None:
            runs.append((start, i - 1))
            start = None
        if ok:
            start = i
        elif s.group is not None and s.has_grad:
            singles.append(i)
    if start is not None:
        runs.append((start, len(slots) - 1))
    return runs, singles


class _NetState:
    """The optimizer's share of one bucketed network: flat state in the network's bucket layout."""

    def __init__(self, net: BucketedNet):
        self.net = net
        named = net._named_params()
        lay, self.total = net._bucket_layout()
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.offsets = [lay[n][0] for n in self.names]
        self.numels = [lay[n][1] for n in self.names]
        self.group_of: "List[Optional[int]]" = [None] * len(named)
        self.steps = [0] * len(named)                               # host copy of steps_t (the planner reads it)
        self.steps_t = torch.zeros(len(named), dtype=torch.float32)  # state[p]["step"] are its 0-dim views (CPU, as in torch)
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        self.ema: Optional[torch.Tensor] = None
        self.theta_ptr = 0

    def view(self, flat: torch.Tensor, i: int) -> torch.Tensor:
        o, k = self.offsets[i], self.numels[i]
        return flat[o:o + k].view(self.params[i].shape)

    def owned_ranges(self) -> "List[Tuple[int, int]]":
        """[lo, hi) float ranges of the maximal stretches of consecutive slots this optimizer owns"""
        out, start = [], None
        for i, g in enumerate(self.group_of):
            if g is not None and start is None:
                start = i
            if g is None and start is not None:
                out.append((self.offsets[start], self.offsets[i - 1] + self.numels[i - 1]))
                start = None
        if start is not None:
            out.append((self.offsets[start], self.offsets[-1] + self.numels[-1]))
        return out


_REFUSED = ("amsgrad", "maximize", "capturable", "foreach", "differentiable", "fused")


class BucketAdam(Optimizer):
    """``BucketAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, ema_decay=None)``.

    ``params``: what ``torch.optim.Adam`` takes - parameters, ``(name, parameter)`` pairs or param-group dicts with per-group
    ``lr`` / ``betas`` / ``eps`` / ``weight_decay``.  ``model`` (optional) only supplies the names ``ema_state_dict()`` uses when
    the parameters come without names.  ``amsgrad``, ``maximize``, ``capturable``, ``foreach``, ``differentiable``, ``fused`` and
    parameters that are not fp32 raise ``NotImplementedError``.

    ``last_launches``: update-kernel launches of the last ``step()`` (a host integer).  ``last_grad_norm`` (with
    ``max_grad_norm``): the global gradient norm of the last ``step()``, a 0-dim tensor on the parameters' device.

    EMA (``ema_decay``): starts as a copy of the parameters at construction and follows every update of a parameter,
    ``ema = ema_decay * ema + (1 - ema_decay) * theta_new``, inside the same launch.  Buffers (BatchNorm statistics) are not
    averaged.  ``ema_state_dict()``, ``swap_ema()``, ``copy_ema_to(module)``.

    Data parallel needs nothing: every rank holds the same bucket after the gradient hook; with ``max_grad_norm`` a loose
    parameter that carries a gradient raises as in ``ops.clip_grad_norm_``."""

    _decoupled_default = False

    def __init__(self, params, lr: float = 1e-3, betas: "Tuple[float, float]" = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: Optional[float] = None, max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None,
                 *, model: Optional[nn.Module] = None, process_group=None, amsgrad: bool = False, maximize: bool = False,
                 capturable: bool = False, foreach: Optional[bool] = None, differentiable: bool = False,
                 fused: Optional[bool] = None):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, foreach=foreach, differentiable=differentiable,
                     fused=fused)
        for k in _REFUSED:
            if given[k]:
                raise NotImplementedError(f"{type(self).__name__}: {k}={given[k]!r} is not implemented (the update runs as one "
                                          "libnvq kernel per run of parameters)")
        if weight_decay is None:
            weight_decay = 1e-2 if self._decoupled_default else 0.0
        lr = float(lr)
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid hyper-parameter: lr={lr}, betas={betas}, eps={eps}, weight_decay={weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"invalid ema_decay: {ema_decay}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.process_group = process_group
        self.last_launches = 0
        self._model = model
        self._nets: "List[_NetState]" = []
        self._loose: "List[Tuple[torch.Tensor, int]]" = []
        self._loose_ema: "Dict[torch.Tensor, torch.Tensor]" = {}
        self._acc: Optional[torch.Tensor] = None
        self._have_norm = False
        self._indexed = False
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._decoupled_default)
        super().__init__(params, defaults)
        self._index()

    # ------------------------------------------------------------------ which network owns which parameter
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if getattr(self, "_indexed", False):
            self._index()

    def _index(self) -> None:
        """Split the parameters into bucketed networks (every live ``BucketedNet`` that owns one of them, frozen neighbours or
        not) and loose ones; state that exists is kept."""
        group_of: "Dict[int, int]" = {}
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise NotImplementedError(f"{type(self).__name__}: a parameter of dtype {p.dtype} (only torch.float32 "
                                              "parameters are implemented)")
                if p.layout != torch.strided:
                    raise NotImplementedError(f"{type(self).__name__}: a parameter of layout {p.layout}")
                group_of[id(p)] = gi
        known = {id(ns.net): ns for ns in self._nets}
        nets: "List[_NetState]" = []
        taken = set()
        for net in sorted(_live_nets, key=id):
            named = net._named_params()
            if not any(id(p) in group_of and id(p) not in taken for _, p in named):
                continue
            ns = known.get(id(net))
            if ns is None or [id(p) for p in ns.params] != [id(p) for _, p in named]:
                ns = _NetState(net)
            ns.group_of = [group_of.get(id(p)) if id(p) not in taken else None for p in ns.params]
            taken.update(id(p) for p, g in zip(ns.params, ns.group_of) if g is not None)
            nets.append(ns)
        self._nets = nets
        self._loose = [(p, gi) for gi, group in enumerate(self.param_groups) for p in group["params"] if id(p) not in taken]
        if self.ema_decay is not None:
            with torch.no_grad():
                for ns in self._nets:
                    if ns.ema is None:
                        ns.ema = ns.net.flat_theta().detach().clone()
                for p, _ in self._loose:
                    if p not in self._loose_ema:
                        self._loose_ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
        self._indexed = True

    # ------------------------------------------------------------------ state
    def _home(self, ns: _NetState, flat: torch.Tensor) -> None:
        """The flat state lives where the parameters live; after the network re-homed its flat parameter buffer (``.to()``) the
        per-parameter views in ``self.state`` are rebuilt."""
        dev = flat.device
        if ns.m is None:
            ns.m = torch.zeros(ns.total, dtype=torch.float32, device=dev)
            ns.v = torch.zeros(ns.total, dtype=torch.float32, device=dev)
        elif ns.m.device != dev or ns.theta_ptr != flat.data_ptr():
            if ns.m.device != dev:
                ns.m, ns.v = ns.m.to(dev), ns.v.to(dev)
            for i, p in enumerate(ns.params):
                if ns.group_of[i] is not None and len(self.state.get(p, ())) != 0:
                    self._bind(ns, i)
        if ns.ema is not None and ns.ema.device != dev:
            ns.ema = ns.ema.to(dev)
        ns.theta_ptr = flat.data_ptr()

    def _bind(self, ns: _NetState, i: int) -> None:
        st = self.state[ns.params[i]]
        st["step"] = ns.steps_t[i]
        st["exp_avg"] = ns.view(ns.m, i)
        st["exp_avg_sq"] = ns.view(ns.v, i)

    def _loose_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    # ------------------------------------------------------------------ step
    def _collect(self) -> list:
        """[(theta, grad, exp_avg, exp_avg_sq, ema or None, group, step number)]: flat fp32 tensors, one entry per launch; the
        step counts are advanced here (``_refuse()`` has run).  A gradient that is not fp32 or not contiguous is read from
        ``flat_grad``'s copy; nothing is copied back, the update never writes the gradient."""
        work = []
        for ns in self._nets:
            net = ns.net
            flat = net.flat_theta()
            self._home(ns, flat)
            bucket = net._last_grad_bucket
            mask = net.grad_alias_mask() if flat.is_cuda else None        # the one-launch runs are the kernel's: GPU only
            mask = mask or [False] * len(ns.params)
            slots = [Slot(gi, step, gi is not None and (fused or p.grad is not None), fused)        # fused: .grad was just read
                     for p, gi, step, fused in zip(ns.params, ns.group_of, ns.steps, mask)]
            runs, singles = plan_runs(slots)
            for a, b in runs:
                lo, hi = ns.offsets[a], ns.offsets[b] + ns.numels[b]
                work.append((flat[lo:hi], bucket[lo:hi], ns.m[lo:hi], ns.v[lo:hi], ns.ema[lo:hi] if ns.ema is not None else None,
                             self.param_groups[slots[a].group], ns.steps[a] + 1))
                for i in range(a, b + 1):
                    if ns.steps[i] == 0 and len(self.state[ns.params[i]]) == 0:
                        self._bind(ns, i)
                    ns.steps[i] += 1
                ns.steps_t[a:b + 1] += 1
            for i in singles:
                p = ns.params[i]
                if p.numel() == 0:
                    continue
                lo, hi = ns.offsets[i], ns.offsets[i] + ns.numels[i]
                if len(self.state[p]) == 0:
                    self._bind(ns, i)
                ns.steps[i] += 1
                ns.steps_t[i] += 1
                work.append((flat[lo:hi], flat_grad(p.grad)[0], ns.m[lo:hi], ns.v[lo:hi],
                             ns.ema[lo:hi] if ns.ema is not None else None, self.param_groups[ns.group_of[i]], ns.steps[i]))
        for p, gi in self._loose:
            if p.grad is None or p.numel() == 0:
                continue
            st = self._loose_state(p)
            ema = self._loose_ema.get(p)
            if ema is not None and ema.device != p.device:
                ema = self._loose_ema[p] = ema.to(p.device)
            for k in ("exp_avg", "exp_avg_sq"):
                if st[k].device != p.device:
                    st[k] = st[k].to(p.device)
            st["step"] += 1
            work.append((p.data.view(-1), flat_grad(p.grad)[0], st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1),
                         ema.view(-1) if ema is not None else None, self.param_groups[gi], int(st["step"].item())))
        return work

    def _refuse(self) -> None:
        """Everything that can refuse a step, before any step count moves."""
        clip = self.max_grad_norm is not None
        devs = set()
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    if g.is_sparse:
                        raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                    if clip:
                        devs.add(g.device)
        for p, _ in self._loose:
            if p.grad is not None and not p.data.is_contiguous():
                raise NotImplementedError(f"{type(self).__name__}: a non-contiguous parameter outside the bucketed networks")
        if len(devs) > 1:
            raise NotImplementedError(f"{type(self).__name__}: max_grad_norm over parameters on several devices "
                                      f"{sorted(map(str, devs))}")
        if clip:                                          # the names are looked up only when there is something to refuse
            refuse_loose_gradients(((self._names().get(p, "?"), p) for p, _ in self._loose if p.grad is not None),
                                   f"{type(self).__name__}(max_grad_norm)", self.process_group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse()
        work = self._collect()
        self.last_launches = 0
        self._have_norm = False
        if not work:
            return loss
        devs = {w[0].device for w in work}
        acc = None
        if self.max_grad_norm is not None:
            acc = self._moments(work, next(iter(devs)))
            self._have_norm = True
        for theta, g, m, v, ema, group, t in work:
            beta1, beta2 = group["betas"]
            kw = dict(lr=float(group["lr"]), beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]),
                      weight_decay=float(group["weight_decay"]), decoupled=bool(group.get("decoupled_weight_decay", False)),
                      step=t, ema_decay=self.ema_decay if ema is not None else 0.0, acc=acc,
                      max_norm=self.max_grad_norm if acc is not None else 0.0)
            if theta.is_cuda:
                with _nvq.device_guard(theta.device):
                    _nvq.adam_step(theta, g, m, v, ema, **kw)
                self.last_launches += 1
            else:
                _adam_step_torch(theta, g, m, v, ema, **kw)
        return loss

    def _moments(self, work: list, dev: torch.device) -> torch.Tensor:
        """acc[2] = the squared global norm of the gradients of this step, chained over the launches' gradients"""
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros(5, dtype=torch.float64, device=dev)
        acc = self._acc
        if dev.type == "cuda":
            with _nvq.device_guard(dev):
                sum_moments([w[1] for w in work], acc, _engine.workspace(dev))
        else:
            acc[2] = sum((w[1].double() ** 2).sum() for w in work)
        return acc

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Global 2-norm of the gradients of the last ``step()`` before clipping (needs ``max_grad_norm``): a 0-dim fp32 tensor on
        the parameters' device, formed when asked for - the step itself reads nothing back.  None before the first step and
        after a step in which no parameter had a gradient."""
        if not self._have_norm:
            return None
        return self._acc[2].sqrt().to(torch.float32)

    # ------------------------------------------------------------------ state dict
    def _packed_params(self) -> "List[torch.Tensor]":
        return [p for group in self.param_groups for p in group["params"]]

    def _ema_of(self) -> "Dict[torch.Tensor, torch.Tensor]":
        out = {}
        for ns in self._nets:
            for i, p in enumerate(ns.params):
                if ns.group_of[i] is not None and ns.ema is not None:
                    out[p] = ns.view(ns.ema, i)
        out.update(self._loose_ema)
        return {p: out[p] for p in self._packed_params()}          # the order the parameters were given in

    def state_dict(self) -> dict:
        """``torch.optim.Adam``'s format (it loads there), plus - with ``ema_decay`` - the key ``"ema"``: the averages in the order
        of the packed parameter indices."""
        sd = super().state_dict()
        if self.ema_decay is not None:
            ema = self._ema_of()
            sd["ema"] = [ema[p] for p in self._packed_params()]
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        """Accepts a ``torch.optim.Adam`` / ``AdamW`` state dict and this class's own: the moments are copied into the flat
        tensors and ``self.state`` holds views of them again."""
        for group in state_dict["param_groups"]:
            for k in ("amsgrad", "maximize"):
                if group.get(k, False):
                    raise NotImplementedError(f"{type(self).__name__}: the state dict was written with {k}=True")
        super().load_state_dict({"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        for group in self.param_groups:
            group.update(foreach=None, fused=None, capturable=False, differentiable=False)
            group.setdefault("decoupled_weight_decay", self._decoupled_default)
        self._index()
        with torch.no_grad():
            for ns in self._nets:
                self._home(ns, ns.net.flat_theta())
                ns.m.zero_()
                ns.v.zero_()
                for i, p in enumerate(ns.params):
                    st = self.state.get(p)
                    ns.steps[i] = 0
                    if ns.group_of[i] is None or st is None or len(st) == 0:
                        continue
                    ns.steps[i] = int(round(float(st["step"])))
                    ns.view(ns.m, i).copy_(st["exp_avg"])
                    ns.view(ns.v, i).copy_(st["exp_avg_sq"])
                ns.steps_t = torch.tensor([float(s) for s in ns.steps], dtype=torch.float32)
                for i, p in enumerate(ns.params):
                    if ns.group_of[i] is not None and len(self.state.get(p, ())) != 0:
                        self._bind(ns, i)
            for p, _ in self._loose:
                st = self.state.get(p)
                if st is None or len(st) == 0:
                    continue
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
            saved = state_dict.get("ema")
            if saved is not None and self.ema_decay is not None:
                ema = self._ema_of()
                for p, e in zip(self._packed_params(), saved):
                    ema[p].copy_(e)

    # ------------------------------------------------------------------ EMA
    def _names(self) -> "Dict[torch.Tensor, str]":
        names: "Dict[torch.Tensor, str]" = {}
        for group in self.param_groups:
            for p, n in zip(group["params"], group.get("param_names") or ()):
                names[p] = n
        if self._model is not None:
            for n, p in self._model.named_parameters():
                names.setdefault(p, n)
        for ns in self._nets:
            for n, p, g in zip(ns.names, ns.params, ns.group_of):
                if g is not None:
                    names.setdefault(p, n)
        for i, p in enumerate(self._packed_params()):
            names.setdefault(p, f"param{i}")
        return names

    def _require_ema(self) -> None:
        if self.ema_decay is None:
            raise RuntimeError(f"{type(self).__name__} was built without ema_decay: there is no weight average")

    def ema_state_dict(self) -> "Dict[str, torch.Tensor]":
        """{parameter name: its average} for ``module.load_state_dict(..., strict=False)``.  The names are those the parameters
        were given with (``model.named_parameters()``), else those of ``model=``, else local to their bucketed network."""
        self._require_ema()
        names = self._names()
        return {names[p]: e for p, e in self._ema_of().items()}

    def _exchange(self) -> None:
        with torch.no_grad():
            for ns in self._nets:
                flat = ns.net.flat_theta()
                self._home(ns, flat)
                for lo, hi in ns.owned_ranges():
                    a, b = flat[lo:hi], ns.ema[lo:hi]
                    tmp = a.clone()
                    a.copy_(b)
                    b.copy_(tmp)
            for p, _ in self._loose:
                e = self._loose_ema[p]
                if e.device != p.device:
                    e = self._loose_ema[p] = e.to(p.device)
                tmp = p.data.clone()
                p.data.copy_(e)
                e.copy_(tmp)

    @contextlib.contextmanager
    def swap_ema(self):
        """``with opt.swap_ema(): evaluate(model)``: the parameters hold the averages inside the block and their own values
        again after it.  The contents are exchanged in place, so the parameters stay views of ``flat_theta()``."""
        self._require_ema()
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def copy_ema_to(self, module: nn.Module):
        """Load the averages into ``module`` (e.g. the teacher of ``ContinualDistillation``, a deepcopy of the model) by name;
        parameters and buffers the average does not cover keep their values."""
        with torch.no_grad():
            return module.load_state_dict({k: v.detach() for k, v in self.ema_state_dict().items()}, strict=False)


class BucketAdamW(BucketAdam):
    """``BucketAdam`` with decoupled weight decay (``torch.optim.AdamW``; ``weight_decay`` defaults to 1e-2)."""
    _decoupled_default = True


def _adam_step_torch(theta, g, m, v, ema, *, lr, beta1, beta2, eps, weight_decay, decoupled, step, ema_decay, acc, max_norm):
    """the formulas of nvq_adam_step in fp32 torch operations (parameters on the CPU)"""
    if acc is not None:
        coef = max_norm / (float(acc[2]) ** 0.5 + 1e-6)
        if coef < 1.0:
            g = g * coef
    if decoupled:
        theta.mul_(1.0 - lr * weight_decay)
    elif weight_decay != 0.0:
        g = g.add(theta, alpha=weight_decay)
    m.lerp_(g, 1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bias1 = 1.0 - beta1 ** step
    bias2_sqrt = (1.0 - beta2 ** step) ** 0.5
    denom = (v.sqrt() / bias2_sqrt).add_(eps)
    theta.addcdiv_(m, denom, value=-(lr / bias1))
    if ema is not None:
        ema.lerp_(theta, 1.0 - ema_decay)
