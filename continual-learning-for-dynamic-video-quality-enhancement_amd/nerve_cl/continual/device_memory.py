"""Device-resident replay memory: EpisodicMemory's interface with the samples in HBM.

The slot tables (capacity x LR, capacity x HR and the small per-slot tables) are device tensors; samples enter and leave
them through the libnvq replay kernels (csrc/replay.hip) and never visit the host.  Which sample is evicted and which
indices a draw returns is decided on the host with ``random.Random(seed)`` and the same calls in the same order as
``EpisodicMemory``, so for ``uniform`` / ``fifo`` / ``reservoir`` / ``stratified`` the same seed and call sequence give the
same stored set and the same ``sample()`` results.  ``importance`` / ``diversity`` read their one decision value per
``store`` from the device (two words).  On top of that the memory forms replay batches in place (``replay_batch``), takes
per-sample losses back as slot importances (``update_importance``) and draws weighted by them on the device.

Declared differences from the host class: every sample has the shapes of the first one; ``buffer`` is a read-only
snapshot; the weighted draw equals successive weighted sampling without replacement in distribution, not draw for draw."""
from __future__ import annotations

import random
import struct
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from nerve_cl import _nvq
from nerve_cl.continual.memory import EpisodicMemory, MemorySample

_LOAD_CHUNK = 32   # samples per launch when a file is loaded


class _Entry:
    __slots__ = ("slot", "metadata")

    def __init__(self, slot: int, metadata: Dict[str, Any]):
        self.slot, self.metadata = slot, metadata


class DeviceEpisodicMemory:
    """Bounded sample store in device memory with EpisodicMemory's public surface (``store``, ``sample``, ``len``,
    ``total_seen``, ``get_stats``, ``clear``, ``save``, ``load``, ``buffer``, ``STRATEGIES``) plus ``store_batch``,
    ``replay_batch``, ``update_importance`` and weighted sampling.  ``storage="bf16"`` halves the footprint: samples are
    rounded to bf16 (nearest even) when stored and widened exactly when read.  ``seed`` seeds the host planner and the
    device sampler's generator; with ``seed=None`` the planner is seeded by the OS and the device generator from the planner,
    so two unseeded memories (two ranks) draw different streams.  There is no CPU fallback."""

    STRATEGIES = EpisodicMemory.STRATEGIES

    def __init__(self, capacity: int = 1000, strategy: str = "reservoir", diversity_weight: float = 0.3,
                 seed: Optional[int] = None, device: Union[None, str, torch.device] = None, storage: str = "fp32",
                 recency_weight: float = 0.0):
        if strategy not in self.STRATEGIES:
            raise ValueError(f"unknown strategy {strategy!r}")
        if storage not in ("fp32", "bf16"):
            raise ValueError(f"storage must be 'fp32' or 'bf16', got {storage!r}")
        if not 0 < capacity <= 65536:
            raise ValueError(f"capacity must be in [1, 65536] (the one-workgroup sampler's limit), got {capacity}")
        if not 0.0 <= recency_weight <= 1.0:
            raise ValueError(f"recency_weight must be in [0, 1], got {recency_weight}")
        self.device = torch.device("cuda" if device is None else device)
        _nvq.require_replay_device(self.device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.strategy, self.diversity_weight = capacity, strategy, diversity_weight
        self.storage, self.recency_weight = storage, float(recency_weight)
        self._rng = random.Random(seed)
        # uniforms of the device sampler: seeded by `seed`, or (seed None) from the host generator, which the OS seeded -
        # a fresh torch.Generator would start every unseeded memory, in every process and on every rank, on the same stream
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed if seed is not None else self._rng.getrandbits(63))
        self._entries: List[_Entry] = []                       # logical order, as EpisodicMemory's list
        self._seen = 0
        self._type_ids: Dict[str, int] = {}
        self._lr = self._hr = None                             # allocated at the first store

    # ------------------------------------------------------------------------------------------------ tables
    def _allocate(self, lr_shape: Tuple[int, ...], hr_shape: Tuple[int, ...]) -> None:
        dt = torch.bfloat16 if self.storage == "bf16" else torch.float32
        dev, cap = self.device, self.capacity
        self._lr_shape, self._hr_shape = tuple(lr_shape), tuple(hr_shape)
        self._channels = lr_shape[0] if len(lr_shape) == 3 else 1
        self._lr = torch.empty((cap,) + self._lr_shape, dtype=dt, device=dev)
        self._hr = torch.empty((cap,) + self._hr_shape, dtype=dt, device=dev)
        self._means = torch.zeros((cap, self._channels), dtype=torch.float32, device=dev)
        self._importance = torch.zeros(cap, dtype=torch.float32, device=dev)
        self._time = torch.zeros(cap, dtype=torch.int32, device=dev)
        self._access = torch.zeros(cap, dtype=torch.int32, device=dev)
        self._type = torch.full((cap,), -1, dtype=torch.int32, device=dev)     # < 0: empty slot
        self._two = torch.zeros(2, dtype=torch.int32, device=dev)              # nvq_replay_nearest's answer
        self._cand_mean = torch.zeros((1, self._channels), dtype=torch.float32, device=dev)

    def _check_shapes(self, lr: torch.Tensor, hr: torch.Tensor) -> None:
        """lr / hr: (n, ...) batches"""
        if lr.numel() == 0 or hr.numel() == 0:
            raise ValueError("empty sample")
        if self._lr is None:
            self._allocate(tuple(lr.shape[1:]), tuple(hr.shape[1:]))
        if tuple(lr.shape[1:]) != self._lr_shape or tuple(hr.shape[1:]) != self._hr_shape:
            raise ValueError(f"DeviceEpisodicMemory holds samples of one shape: LR {self._lr_shape} / HR {self._hr_shape}, "
                             f"got LR {tuple(lr.shape[1:])} / HR {tuple(hr.shape[1:])}")

    def _on_device(self, t: torch.Tensor) -> torch.Tensor:
        """fp32, contiguous, on the memory's device (a device tensor is never copied to the host)"""
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _type_id(self, metadata: Dict[str, Any]) -> int:
        return self._type_ids.setdefault(metadata.get("content_type", "unknown"), len(self._type_ids))

    def _ints(self, rows: Sequence[Sequence]) -> torch.Tensor:
        """int32 rows of equal length, on the device with one copy"""
        return torch.tensor(rows, dtype=torch.int32).to(self.device, non_blocking=True)

    def _write(self, lr: torch.Tensor, hr: torch.Tensor, jobs: List[Tuple[int, int, float, int, int]]) -> None:
        """jobs: (row of lr / hr, slot, importance, time, type id); one launch.  A row without a job gets slot -1, which the
        kernel's workgroups skip: nothing of it is read or written."""
        if not jobs:
            return
        plan = [[-1] * lr.shape[0] for _ in range(4)]
        for row, slot, imp, time, tid in jobs:
            plan[0][row], plan[1][row], plan[2][row] = slot, time, tid
            plan[3][row] = struct.unpack("<i", struct.pack("<f", imp))[0]
        plan = self._ints(plan)
        with _nvq.device_guard(self.device):
            _nvq.replay_store(lr, hr, plan[0], plan[3].view(torch.float32), plan[1], plan[2], self._lr, self._hr,
                              self._means, self._importance, self._time, self._access, self._type)

    # ------------------------------------------------------------------------------------------------ host planner
    def __len__(self) -> int:
        return len(self._entries)

    @property
    def total_seen(self) -> int:
        return self._seen

    @staticmethod
    def _ctype(e: _Entry) -> str:
        return e.metadata.get("content_type", "unknown")

    def _by_type(self) -> Dict[str, List[int]]:
        groups: Dict[str, List[int]] = {}
        for i, e in enumerate(self._entries):
            groups.setdefault(self._ctype(e), []).append(i)
        return groups

    def _replace(self, pos: int, metadata: Dict[str, Any]) -> int:
        slot = self._entries[pos].slot
        self._entries[pos] = _Entry(slot, metadata)
        return slot

    def _reservoir(self, metadata: Dict[str, Any]) -> Optional[int]:
        if self._rng.random() < self.capacity / self._seen:
            return self._replace(self._rng.randrange(self.capacity), metadata)
        return None

    def _decision(self) -> Tuple[int, float]:
        """(slot, fp32 value) that nvq_replay_nearest left on the device: one copy of two words"""
        slot, bits = self._two.tolist()
        return slot, struct.unpack("<f", struct.pack("<i", bits))[0]

    def _plan(self, metadata: Dict[str, Any], importance: float, lr_row: Optional[torch.Tensor]) -> Optional[int]:
        """EpisodicMemory.store's decision for one newcomer (same generator calls): the physical slot, or None (rejected)"""
        self._seen += 1
        if len(self._entries) < self.capacity:
            slot = len(self._entries)          # slots fill in order; afterwards a newcomer takes its victim's slot
            self._entries.append(_Entry(slot, metadata))
            return slot
        if self.strategy == "reservoir":
            return self._reservoir(metadata)
        if self.strategy == "stratified":
            groups = self._by_type()
            biggest = max(groups, key=lambda k: len(groups[k]))
            if len(groups.get(metadata.get("content_type", "unknown"), [])) < len(groups[biggest]):
                return self._replace(self._rng.choice(groups[biggest]), metadata)
            return self._reservoir(metadata)
        if self.strategy == "importance":
            # logical position == physical slot here (nothing is ever popped), so the lowest slot is the host's first minimum
            with _nvq.device_guard(self.device):
                _nvq.replay_nearest(None, self._importance, self._type, self._two)
            slot, lowest = self._decision()
            imp32 = struct.unpack("<f", struct.pack("<f", importance))[0]
            return self._replace(slot, metadata) if slot >= 0 and imp32 > lowest else None
        if self.strategy == "diversity":
            with _nvq.device_guard(self.device):
                _nvq.replay_means(lr_row, self._cand_mean)
                _nvq.replay_nearest(self._cand_mean, self._means, self._type, self._two)
            slot, dist = self._decision()
            return self._replace(slot, metadata) if slot >= 0 and dist > struct.unpack("<f", struct.pack("<f", 0.1))[0] else None
        first = self._entries.pop(0)                                # 'uniform' / 'fifo': first in, first out
        self._entries.append(_Entry(first.slot, metadata))
        return first.slot

    # ------------------------------------------------------------------------------------------------ store
    def store(self, frame_lr: torch.Tensor, frame_hr: torch.Tensor, metadata: Optional[Dict[str, Any]] = None,
              importance: float = 1.0) -> bool:
        """EpisodicMemory.store with the sample kept on the device (CPU or GPU tensors; a GPU tensor stays there)."""
        lr, hr = self._on_device(frame_lr).unsqueeze(0), self._on_device(frame_hr).unsqueeze(0)
        self._check_shapes(lr, hr)
        metadata = metadata or {}
        slot = self._plan(metadata, float(importance), lr)
        if slot is None:
            return False
        self._write(lr, hr, [(0, slot, float(importance), self._seen, self._type_id(metadata))])
        return True

    def store_batch(self, lr: torch.Tensor, hr: torch.Tensor, content_type: Union[None, str, Sequence[str]] = None,
                    importance: Union[None, float, Sequence[float]] = None) -> List[bool]:
        """``store`` of the n samples of lr (n, ...) / hr (n, ...) in order, with one launch: the host plans the n slots
        first, and a sample the plan rejects (or that a later sample of the same batch evicts) is not in the launch.
        Returns what the n ``store`` calls would have returned.  (A full ``importance`` / ``diversity`` memory needs a device
        value per decision and stores sample by sample.)"""
        n = lr.shape[0]
        if hr.shape[0] != n:
            raise ValueError(f"store_batch: {n} LR samples and {hr.shape[0]} HR samples")
        types = list(content_type) if isinstance(content_type, (list, tuple)) else [content_type] * n
        imps = [1.0] * n if importance is None else \
            ([float(importance)] * n if isinstance(importance, (int, float)) else [float(v) for v in importance])
        if len(types) != n or len(imps) != n:
            raise ValueError("store_batch: one content type and one importance per sample")
        metas = [{} if t is None else {"content_type": t} for t in types]
        lr, hr = self._on_device(lr), self._on_device(hr)
        self._check_shapes(lr, hr)
        kept: List[bool] = []
        jobs: Dict[int, Tuple[int, int, float, int, int]] = {}
        for j in range(n):
            if self.strategy in ("importance", "diversity") and len(self._entries) >= self.capacity:
                self._write(lr, hr, list(jobs.values()))            # the decision reads what the batch has stored so far
                jobs = {}
            slot = self._plan(metas[j], imps[j], lr[j:j + 1])
            kept.append(slot is not None)
            if slot is not None:
                jobs.pop(slot, None)                                # an earlier sample of this batch, evicted again
                jobs[slot] = (j, slot, imps[j], self._seen, self._type_id(metas[j]))
        self._write(lr, hr, list(jobs.values()))
        return kept

    # ------------------------------------------------------------------------------------------------ draws
    def _spread(self, batch_size: int) -> List[int]:
        groups = self._by_type()
        per, rem = divmod(batch_size, len(groups))
        idx: List[int] = []
        for members in groups.values():
            n = min(per + (1 if rem > 0 else 0), len(members))
            rem -= 1
            idx.extend(self._rng.sample(members, n))
        return idx[:batch_size]

    def _host_draw(self, batch_size: int, content_type: Optional[str]) -> List[int]:
        """EpisodicMemory.sample's index plan (logical positions)"""
        batch_size = min(batch_size, len(self._entries))
        groups = self._by_type()
        if content_type is not None and content_type in groups:
            return self._rng.sample(groups[content_type], min(batch_size, len(groups[content_type])))
        return self._spread(batch_size)

    def _device_draw(self, k: int, content_type: Optional[str]) -> torch.Tensor:
        """k slot indices (int32, device; -1 where no eligible slot was left) from nvq_replay_sample_weighted"""
        if k > 256:
            raise ValueError(f"the device sampler draws at most 256 samples per call, got {k}")
        u = torch.rand(self.capacity, generator=self._gen, device=self.device, dtype=torch.float32).clamp_min_(1e-30)
        out = torch.empty(k, dtype=torch.int32, device=self.device)
        with _nvq.device_guard(self.device):
            _nvq.replay_sample_weighted(self._importance, self._time, self._type, self._seen, self.recency_weight,
                                        self._type_ids[content_type] if content_type is not None else -1, u, out)
        return out

    def _scope(self, n: int, content_type: Optional[str]) -> Tuple[int, Optional[str]]:
        """(samples a draw of n returns, the content type it is restricted to): EpisodicMemory.sample's rules - never more
        than is stored, and a content type that is not stored now means all samples"""
        if not self._entries:
            raise ValueError("Memory buffer is empty")
        n = min(n, len(self._entries))
        if content_type is not None:
            members = sum(1 for e in self._entries if self._ctype(e) == content_type)
            if members == 0:
                return n, None
            n = min(n, members)
        return n, content_type

    def _use_device_sampler(self, weighted: Optional[bool]) -> bool:
        return self.recency_weight > 0 if weighted is None else bool(weighted)

    def sample(self, batch_size: int = 32, content_type: Optional[str] = None, device: Optional[torch.device] = None,
               weighted: Optional[bool] = None):
        """(lr, hr, metadata) as EpisodicMemory.sample, the tensors on the memory's device (or moved to ``device``).

        ``weighted=True`` (or ``recency_weight > 0`` with ``weighted`` not given): the draw is the device sampler, with
        probability proportional to (1 - recency_weight) * importance + recency_weight / (1 + now - time stored), without
        replacement (Efraimidis-Spirakis keys from this memory's own device generator).  That equals successive weighted
        sampling without replacement in distribution; it does NOT reproduce StreamingEpisodicMemory draw for draw.  A
        content type of which nothing is stored means all samples, as in the host class."""
        k, content_type = self._scope(batch_size, content_type)
        if self._use_device_sampler(weighted):
            idx = self._device_draw(k, content_type)
            slots = [s for s in idx.tolist() if s >= 0]           # (the metadata costs this copy of k ints)
            idx = idx[:len(slots)]
            by_slot = {e.slot: e for e in self._entries}
            metas = [by_slot[s].metadata for s in slots]
        else:
            pos = self._host_draw(batch_size, content_type)
            slots = [self._entries[i].slot for i in pos]
            metas = [self._entries[i].metadata for i in pos]
            idx = self._ints([slots])[0]
        lr = torch.empty((len(slots),) + self._lr_shape, dtype=torch.float32, device=self.device)
        hr = torch.empty((len(slots),) + self._hr_shape, dtype=torch.float32, device=self.device)
        if slots:
            with _nvq.device_guard(self.device):
                _nvq.replay_gather(self._lr, self._hr, idx, lr, hr, 0, self._access)
        if device is not None and torch.device(device) != self.device:
            lr, hr = lr.to(device), hr.to(device)
        return lr, hr, metas

    def replay_batch(self, cur_lr: torch.Tensor, cur_hr: torch.Tensor, n: int, content_type: Optional[str] = None,
                     weighted: Optional[bool] = None):
        """(lr_batch, hr_batch, indices): the current batch in rows [0, B) and n replay samples (fewer if fewer are stored)
        gathered behind it by one launch, in one allocation per tensor.  ``indices`` (int32, device) are the slots of the
        replay rows, the handle ``update_importance`` takes.  With the device sampler (``weighted``, see ``sample``) the call
        makes no host synchronisation; a row whose draw found no slot with a positive weight is zero and has index -1.  A
        host-planned draw sends its indices up with one small non-blocking copy."""
        n, content_type = self._scope(n, content_type)
        B = cur_lr.shape[0]
        if tuple(cur_lr.shape[1:]) != self._lr_shape or tuple(cur_hr.shape[1:]) != self._hr_shape or cur_hr.shape[0] != B:
            raise ValueError(f"replay_batch: the current batch must be (B,) + LR {self._lr_shape} / HR {self._hr_shape}")
        if self._use_device_sampler(weighted):
            idx = self._device_draw(n, content_type)
        else:                                   # (an even spread over uneven content types can return fewer than n)
            idx = self._ints([[self._entries[i].slot for i in self._host_draw(n, content_type)]])[0]
        n = idx.numel()
        lr = torch.empty((B + n,) + self._lr_shape, dtype=torch.float32, device=self.device)
        hr = torch.empty((B + n,) + self._hr_shape, dtype=torch.float32, device=self.device)
        lr[:B].copy_(cur_lr.detach(), non_blocking=True)
        hr[:B].copy_(cur_hr.detach(), non_blocking=True)
        if idx.numel():
            with _nvq.device_guard(self.device):
                _nvq.replay_gather(self._lr, self._hr, idx, lr, hr, B, self._access)
        return lr, hr, idx

    def update_importance(self, indices, values: torch.Tensor, momentum: float = 0.0) -> None:
        """importance[indices[j]] = momentum * importance[indices[j]] + (1 - momentum) * values[j]: one launch, no host
        synchronisation.  ``values``: a (k,) fp32 device tensor, e.g. the replay rows of ``ops.l1_loss(...,
        reduction="none")``; non-finite values and indices of -1 are skipped.  ``indices``: the int32 device tensor
        ``replay_batch`` returned (distinct), or a list of slots, which is range-checked here."""
        if self._lr is None:
            raise ValueError("Memory buffer is empty")
        if not 0.0 <= momentum <= 1.0:
            raise ValueError(f"momentum must be in [0, 1], got {momentum}")
        if not isinstance(indices, torch.Tensor):
            indices = [int(i) for i in indices]
            if any(i < 0 or i >= self.capacity for i in indices):
                raise ValueError(f"update_importance: slot index outside [0, {self.capacity})")
            indices = self._ints([indices])[0]
        if indices.dtype != torch.int32 or indices.device != self.device:
            indices = indices.to(device=self.device, dtype=torch.int32)
        values = values.detach()
        if values.dtype != torch.float32 or values.device != self.device:
            values = values.to(device=self.device, dtype=torch.float32)
        if values.dim() != 1 or values.numel() != indices.numel():
            raise ValueError(f"update_importance: {indices.numel()} indices and values of shape {tuple(values.shape)}")
        if indices.numel() == 0:
            return
        with _nvq.device_guard(self.device):
            _nvq.replay_update_importance(self._importance, indices.contiguous(), values.contiguous(), float(momentum))

    # ------------------------------------------------------------------------------------------------ views
    def _rows(self, slots: List[int]):
        for s in slots:
            yield self._lr[s].float(), self._hr[s].float()       # fp32 storage: views; bf16: converted copies

    @property
    def buffer(self) -> List[MemorySample]:
        """A read-only SNAPSHOT of the stored samples in EpisodicMemory's order (not the live list of the host class):
        device views in fp32 storage, converted copies in bf16 storage; importances and access counts as of this call."""
        if not self._entries:
            return []
        imp, acc = self._importance.tolist(), self._access.tolist()
        return [MemorySample(lr, hr, e.metadata, imp[e.slot], acc[e.slot])
                for e, (lr, hr) in zip(self._entries, self._rows([e.slot for e in self._entries]))]

    def get_stats(self) -> Dict[str, Any]:
        return {"size": len(self), "capacity": self.capacity, "utilization": len(self) / self.capacity,
                "total_seen": self._seen, "content_distribution": {k: len(v) for k, v in self._by_type().items()},
                "strategy": self.strategy}

    def clear(self) -> None:
        self._entries, self._seen = [], 0
        if self._lr is not None:
            self._type.fill_(-1)

    def save(self, path: str) -> None:
        """EpisodicMemory's on-disk dictionary (tensors on the CPU): the file loads in either class."""
        imp = self._importance.tolist() if self._entries else []
        torch.save({"buffer": [(lr.cpu(), hr.cpu(), e.metadata, imp[e.slot])
                               for e, (lr, hr) in zip(self._entries, self._rows([e.slot for e in self._entries]))],
                    "total_seen": self._seen, "strategy": self.strategy, "capacity": self.capacity}, path)

    def load(self, path: str) -> None:
        """Replace the contents by a file either class wrote (bf16 storage rounds on load); access counts restart at 0."""
        blob = torch.load(path, weights_only=True)
        items = blob["buffer"]
        if len(items) > self.capacity:
            raise ValueError(f"{len(items)} stored samples do not fit a capacity of {self.capacity}")
        shapes = {(tuple(it[0].shape), tuple(it[1].shape)) for it in items}       # checked before anything is dropped
        if len(shapes) > 1 or (shapes and self._lr is not None and shapes != {(self._lr_shape, self._hr_shape)}):
            raise ValueError(f"DeviceEpisodicMemory holds samples of one shape"
                             + (f": LR {self._lr_shape} / HR {self._hr_shape}" if self._lr is not None else "")
                             + f", the file has {sorted(shapes)}")
        self.clear()
        self._seen = blob["total_seen"]
        t0 = self._seen - len(items)
        for c0 in range(0, len(items), _LOAD_CHUNK):
            chunk = items[c0:c0 + _LOAD_CHUNK]
            lr = self._on_device(torch.stack([it[0] for it in chunk]))
            hr = self._on_device(torch.stack([it[1] for it in chunk]))
            self._check_shapes(lr, hr)
            jobs = []
            for j, (_, _, meta, imp) in enumerate(chunk):
                self._entries.append(_Entry(c0 + j, meta))
                jobs.append((j, c0 + j, float(imp), t0 + c0 + j + 1, self._type_id(meta)))
            self._write(lr, hr, jobs)
