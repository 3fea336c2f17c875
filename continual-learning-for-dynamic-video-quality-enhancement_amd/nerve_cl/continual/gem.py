"""Gradient Episodic Memory (GEM, Lopez-Paz & Ranzato 2017) on the flat gradient buckets.

A-GEM (``agem.py``) averages the episodic memory into one reference gradient; GEM keeps one reference ``r_t`` per earlier task
and asks that the step's gradient ``g`` conflicts with none of them.  With ``q = R g`` and ``P = R R' + ridge I``: when some
``q_t < 0``, ``v = argmin 1/2 v'Pv + q'v`` subject to ``v >= margin`` and ``g <- g + R'v`` (``project2cone2`` of the authors'
code; ``margin`` is their "memory strength", ``eps`` their ridge).  ``eps_relative=True`` scales the ridge by ``max_t r_t.r_t``:
with gradients as small as this network's an absolute ridge can dominate ``P``.

On HIP tensors the Gram matrix of the references and ``g``, the quadratic program and the projection are the kernels of
csrc/gem.hip: per bucketed network one ``nvq_gem_gram`` (two launches, chained over the networks), then one
``nvq_gem_solve`` and one ``nvq_gem_project`` per network, on the network's gradient bucket in place.  The multipliers stay on the
device - ``project()`` never synchronises with the host.

A module on the CPU takes the same formulas and the same active-set rule in float64 (``solve_multipliers``), so the class also
works on plain modules.
"""
from __future__ import annotations

from typing import Callable, Dict, Hashable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import refuse_loose_gradients, segments_of

MAX_TASKS = _nvq.GEM_MAX_TASKS
MAX_ITER = 64                          # GEM_MAX_ITER of csrc/gem.hip
# stats slots
VIOLATED, ACTIVE, ITERATIONS, STATUS, PROJECTIONS, GG_BEFORE, GG_AFTER, MIN_COS = range(8)


def _free_solve(P: np.ndarray, c: np.ndarray, free: List[int]) -> Optional[np.ndarray]:
    """P_FF s = -c_F by Cholesky; None when a pivot is not positive"""
    try:
        L = np.linalg.cholesky(P[np.ix_(free, free)])
    except np.linalg.LinAlgError:
        return None
    y = np.linalg.solve(L, -c[free])
    return np.linalg.solve(L.T, y)


def solve_multipliers(gram, T: int, margin: float = 0.5, eps: float = 1e-3, eps_relative: bool = False,
                      projections: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """``(v, stats)`` as ``nvq_gem_solve`` leaves them (16 and 8 float64 values) from a 16 x 16 float64 Gram matrix whose index
    ``T`` stands for ``g``: the host form of the same primal active-set method (Lawson-Hanson on ``u = v - margin >= 0``: free
    the most violated multiplier, solve the free block by Cholesky, step back to the boundary when a free multiplier leaves)."""
    G = np.asarray(gram, dtype=np.float64).reshape(16, 16)
    v, stats = np.zeros(16), np.zeros(8)
    stats[PROJECTIONS] = projections
    gg = G[T, T]
    stats[GG_BEFORE] = stats[GG_AFTER] = gg
    if not np.isfinite(G[:T + 1, :T + 1]).all():
        stats[STATUS] = 2.0
        return v, stats
    if T == 0:
        return v, stats
    RR, q = G[:T, :T].copy(), G[:T, T].copy()
    rr = np.diag(RR).copy()
    den = np.sqrt(gg * rr)
    stats[MIN_COS] = np.where(den > 0, q / np.where(den > 0, den, 1.0), 0.0).min()
    stats[VIOLATED] = float((q < 0).sum())
    if stats[VIOLATED] == 0:
        return v, stats
    margin = float(np.float32(margin))
    eps = float(np.float32(eps))
    ridge = eps * rr.max() if eps_relative else eps
    P = RR + ridge * np.eye(T)
    c = q + margin * P.sum(axis=1)
    u = np.zeros(T)
    tol = 1e-13 * np.abs(c).max()
    free: List[int] = []
    it, status, running = 0, 0, True
    while running:
        w = P @ u + c
        bound = [i for i in range(T) if i not in free]
        if not bound:
            break
        pick = min(bound, key=lambda i: (w[i], i))
        if not w[pick] < -tol:
            break
        free = sorted(free + [pick])
        while True:
            if it == MAX_ITER:
                status, running = 1, False
                break
            it += 1
            s = _free_solve(P, c, free)
            if s is None:
                status, running = 1, False
                break
            neg = [k for k in range(len(free)) if not s[k] > 0]
            if not neg:
                u[free] = s
                break
            alphas = [max(u[free[k]] / (u[free[k]] - s[k]), 0.0) if u[free[k]] != s[k] else 0.0 for k in neg]
            a = min(alphas)
            leave = free[neg[alphas.index(a)]]
            u[free] = u[free] + a * (s - u[free])
            gone = [i for i in free if i == leave or not u[i] > 0]
            u[gone] = 0.0
            free = [i for i in free if i not in gone]
            if not free:
                break
    v[:T] = u + margin
    stats[ACTIVE] = float((u > 0).sum())
    stats[ITERATIONS], stats[STATUS] = float(it), float(status)
    stats[PROJECTIONS] += 1.0
    stats[GG_AFTER] = gg + 2.0 * (v[:T] @ q) + v[:T] @ (RR @ v[:T])
    return v, stats


class GEM:
    """``GEM(model, memory=None, ref_batch_size=8, margin=0.5, eps=1e-3, eps_relative=False, max_tasks=15)``; in a step::

        gem.compute_references(loss_fn)       # r_t: gradient on a batch of every earlier task drawn from the memory
        loss_fn(model(lr), hr).backward()     # g
        gem.project()                         # g <- g + R'v  when some g.r_t < 0
        optimizer.step()

    and ``gem.add_task(name)`` once a task's samples are in the memory under ``content_type=name``.

    ``stats`` (float64, on the model's device) = [number of g.r_t < 0, number of v_t > margin, solver iterations, status (0
    solved, 1 iteration cap reached, 2 non-finite input: no projection), projections so far, g.g before, g.g after, min_t cos(g,
    r_t)] of the last ``project()``; ``multipliers`` is ``v`` (16 float64, zeros when nothing was projected).

    Data parallel (``nerve_cl.parallel``): every reference pass and the task pass leave the bucket hook rank-averaged, so every
    rank forms the same Gram matrix in the same order and hence the same ``v``, with no further collective;
    ``compute_references`` is a collective step; a loose parameter that carries a gradient raises
    (``nerve_cl._bucket.refuse_loose_gradients``)."""

    def __init__(self, model: nn.Module, memory=None, ref_batch_size: int = 8, margin: float = 0.5, eps: float = 1e-3,
                 eps_relative: bool = False, max_tasks: int = MAX_TASKS, process_group=None):
        if not 1 <= int(max_tasks) <= MAX_TASKS:
            raise ValueError(f"max_tasks must be in [1, {MAX_TASKS}] (the references and g are the 16 rows of one tile), got {max_tasks}")
        if not margin >= 0 or not eps > 0:
            raise ValueError(f"margin must be >= 0 and eps > 0, got margin={margin}, eps={eps}")
        self.model, self.memory, self.ref_batch_size = model, memory, int(ref_batch_size)
        self.margin, self.eps, self.eps_relative = float(margin), float(eps), bool(eps_relative)
        self.max_tasks, self.process_group = int(max_tasks), process_group
        self._segs = segments_of(model)
        self._dev = next(model.parameters()).device
        self._hip = self._dev.type == "cuda"
        # one (max_tasks, numel) reference matrix per segment, in segment layout (bucket padding stays 0); float64 on the CPU,
        # where the parameters may be of any floating type
        rdtype = torch.float32 if self._hip else torch.float64
        self._ref = [torch.zeros(self.max_tasks, sg.numel(), dtype=rdtype, device=self._dev) for sg in self._segs]
        self._tasks: List[Hashable] = []
        self._captured: set = set()
        self.gram = torch.zeros(16, 16, dtype=torch.float64, device=self._dev)
        self.multipliers = torch.zeros(16, dtype=torch.float64, device=self._dev)
        self.stats = torch.zeros(8, dtype=torch.float64, device=self._dev)

    # ------------------------------------------------------------------ tasks
    @property
    def tasks(self) -> list:
        """the task ids in row order"""
        return list(self._tasks)

    def add_task(self, task: Hashable) -> int:
        """Register ``task`` (its reference stays zero until ``compute_references`` / ``capture_reference`` fills it); -> its row."""
        if task in self._tasks:
            return self._tasks.index(task)
        if len(self._tasks) >= self.max_tasks:
            raise ValueError(f"GEM keeps at most {self.max_tasks} tasks; {task!r} would be number {len(self._tasks) + 1}")
        self._tasks.append(task)
        return len(self._tasks) - 1

    def forget(self, task: Hashable) -> None:
        """Drop ``task``'s reference; the rows after it move up."""
        row = self._tasks.index(task)
        last = len(self._tasks) - 1
        with torch.no_grad():
            for ref in self._ref:
                if row < last:
                    ref[row:last] = ref[row + 1:last + 1].clone()
                ref[last].zero_()
        self._tasks.pop(row)
        self._captured.discard(task)

    # ------------------------------------------------------------------ reference gradients
    def capture_reference(self, task: Hashable) -> None:
        """Copy the gradients now in place into ``task``'s row (a parameter without a gradient: zeros).  A new id takes the next
        free row, a known id overwrites its own."""
        row = self.add_task(task)
        with torch.no_grad():
            for sg, ref in zip(self._segs, self._ref):
                if sg.net is None:
                    refuse_loose_gradients(sg.named, "GEM.capture_reference", self.process_group)
                if self._hip and sg.aliased():
                    ref[row].copy_(sg.net._last_grad_bucket)     # a copy: the bucket itself belongs to the next zero_grad
                    continue
                views = sg.views(ref[row])
                for n, p in sg.named:
                    if p.grad is None:
                        views[n].zero_()
                    else:
                        views[n].copy_(p.grad)
        self._captured.add(task)

    def _draw(self, task: Hashable):
        mem = self.memory
        if mem is None or len(mem) == 0:
            return None
        if hasattr(mem, "_by_type") and task not in mem._by_type():
            return None                                          # (sample() would fall back to all content types)
        lr, hr, metas = mem.sample(batch_size=self.ref_batch_size, device=self._dev, content_type=task)
        if lr.shape[0] == 0 or any(m.get("content_type", "unknown") != task for m in metas):
            return None
        return lr, hr

    def compute_references(self, loss_fn: Callable, batches: Optional[Dict] = None) -> int:
        """For every known task: zero_grad -> ``loss_fn(model(lr), hr).backward()`` -> ``capture_reference(task)`` -> zero_grad, on
        ``batches[task] = (lr, hr)`` or on ``ref_batch_size`` samples of the memory stored under ``content_type=task``.  A task
        without a batch / without samples is skipped and keeps its row.  -> the number of rows refreshed."""
        done = 0
        for task in list(self._tasks):
            batch = batches.get(task) if batches is not None else self._draw(task)
            if batch is None:
                continue
            self.model.zero_grad()
            loss_fn(self.model(batch[0]), batch[1]).backward()
            self.capture_reference(task)
            self.model.zero_grad()
            done += 1
        return done

    # ------------------------------------------------------------------ projection
    def _gradients(self, what: str):
        """[(flat g, reference matrix, segment or None)]: the bucket itself for an aliased network (written in place, None), else
        the segment's gradients gathered into one flat buffer as ``Segment.grads()`` does, with the segment to write back to"""
        out = []
        for sg, ref in zip(self._segs, self._ref):
            if sg.net is None:
                refuse_loose_gradients(sg.named, what, self.process_group)
            if self._hip:
                flat = sg.grads()                                # the bucket itself when .grad aliases it
                if flat is not None:
                    in_place = sg.net is not None and flat is sg.net._last_grad_bucket
                    out.append((flat, ref, None if in_place else sg))
                continue
            if all(p.grad is None for _, p in sg.named):
                continue
            flat = torch.zeros(sg.numel(), dtype=ref.dtype, device=self._dev)   # float64: Segment.grads() is fp32
            views = sg.views(flat)
            for n, p in sg.named:
                if p.grad is not None:
                    views[n].copy_(p.grad.detach())
            out.append((flat, ref, sg))
        return out

    @staticmethod
    def _write_back(flat: torch.Tensor, sg) -> None:
        views = sg.views(flat)
        for n, p in sg.named:
            if p.grad is not None:                               # a parameter without a gradient takes no part
                p.grad.copy_(views[n])

    def project(self) -> None:
        """Between ``loss.backward()`` and ``optimizer.step()``.  Does nothing before a reference was captured."""
        T = len(self._tasks)
        if not self._captured or T == 0:
            return
        with torch.no_grad():
            parts = self._gradients("GEM.project")
            if not parts:
                return
            if not self._hip:
                return self._project_host(parts, T)
            with _nvq.device_guard(self._dev):
                ws = _engine.workspace(self._dev)
                for k, (g, ref, _) in enumerate(parts):
                    _nvq.gem_gram(ref, T, g, self.gram, ws, accumulate=k > 0)
                _nvq.gem_solve(self.gram, T, self.margin, self.eps, self.eps_relative, self.multipliers, self.stats)
                for g, ref, sg in parts:
                    _nvq.gem_project(g, ref, T, self.multipliers)
                    if sg is not None:
                        self._write_back(g, sg)

    def _project_host(self, parts, T: int) -> None:
        """the same formulas in float64 (CPU modules)"""
        G = torch.zeros(16, 16, dtype=torch.float64)
        for g, ref, _ in parts:
            rows = torch.cat([ref[:T].double(), g.double().unsqueeze(0)])
            G[:T + 1, :T + 1] += rows @ rows.t()
        self.gram.copy_(G)
        v, stats = solve_multipliers(G.numpy(), T, self.margin, self.eps, self.eps_relative, float(self.stats[PROJECTIONS]))
        self.multipliers.copy_(torch.from_numpy(v))
        self.stats.copy_(torch.from_numpy(stats))
        if not v.any():
            return
        vt = self.multipliers[:T]
        for g, ref, sg in parts:
            g.add_(vt @ ref[:T].double())
            self._write_back(g, sg)

    # ------------------------------------------------------------------ reports
    def min_cosine(self) -> torch.Tensor:
        """min_t cos(g, r_t) of the last ``project()``: a 0-dim tensor on the model's device; no host read."""
        return self.stats[MIN_COS]

    def num_projections(self) -> int:
        """How many ``project()`` calls changed the gradient so far (this call reads from the device)."""
        return int(self.stats[PROJECTIONS].item())

    def status(self) -> int:
        """0 solved, 1 iteration cap reached, 2 non-finite input, of the last ``project()`` (this call reads from the device)."""
        return int(self.stats[STATUS].item())
