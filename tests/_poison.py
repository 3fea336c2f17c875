"""Poisoned buffers: the helper of the tests that assert *no result depends on memory the contract says nobody reads*.

`poisoned_allocations(monkeypatch)` wraps the four ways Python code obtains uninitialised memory - `torch.empty`,
`torch.empty_like`, `torch.empty_strided` and `Tensor.new_empty` - so that a tensor of a FLOATING dtype (fp32, bf16, fp64,
fp16) comes back filled with quiet NaN.  A program that is correct under `torch.empty` is correct under this wrapper, because
it may not read what it has not written: that is the whole argument for comparing a clean and a poisoned run bit by bit.
`poison_(t)` does the same to a tensor that already exists (the engine's cached workspaces, an explicitly passed `ws`, the
channels beside a slice, an overwritten destination).

What is deliberately NOT poisoned: integer, index and bool buffers - the warp gather's int32 hit list and counters, max-pool
index planes, one-bit ReLU masks, the CBAM arg-max plane, slot maps, replay-memory indices.  A NaN is only ever a value: the
worst a stray read of it can do is a wrong number, which is what these tests look for.  A stale *index* could send a kernel out
of bounds, and provoking a fault is not something a test may do on a shared GPU.  For the same reason a float tensor that a
kernel uses as a coordinate (the warp's flow field) is never poisoned as an input by the kernel tests.

`same_bits(a, b)` is equality of the raw bit patterns: NaN equals the same NaN, -0.0 differs from +0.0."""
from __future__ import annotations

import torch

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def is_poisonable(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_floating_point()


def poison_(t: torch.Tensor) -> torch.Tensor:
    """fill a floating tensor with quiet NaN in place (any other dtype is refused: see the module docstring)"""
    assert is_poisonable(t), f"only floating tensors are poisoned, not {t.dtype}"
    with torch.no_grad():
        t.fill_(float("nan"))
    return t


class Poison:
    """what `poisoned_allocations` returns: counters of what it poisoned and what it let through"""

    def __init__(self):
        self.tensors = self.bytes = self.untouched = 0

    def _seen(self, t):
        if is_poisonable(t):
            poison_(t)
            self.tensors += 1
            self.bytes += t.numel() * t.element_size()
        elif isinstance(t, torch.Tensor):
            self.untouched += 1
        return t


def poisoned_allocations(monkeypatch) -> Poison:
    """Until `monkeypatch` is undone (the end of the test, or `monkeypatch.undo()` / a `monkeypatch.context()` block), every
    floating tensor returned by torch.empty / empty_like / empty_strided / Tensor.new_empty holds NaN."""
    log = Poison()

    def wrap(fn):
        def poisoned(*args, **kwargs):
            return log._seen(fn(*args, **kwargs))
        poisoned.__name__ = getattr(fn, "__name__", "empty")
        poisoned.__wrapped__ = fn
        return poisoned

    for name in ("empty", "empty_like", "empty_strided"):
        monkeypatch.setattr(torch, name, wrap(getattr(torch, name)))
    monkeypatch.setattr(torch.Tensor, "new_empty", wrap(torch.Tensor.new_empty))
    return log


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    if t.dtype == torch.bool or not (t.is_floating_point() or t.is_complex()):
        return t.reshape(-1)
    return t.reshape(-1).view(_INT_VIEW[t.element_size()])


class BitCompare:
    """truthy when the two tensors have the same shape, dtype and raw bits; `index` is the first differing flat index and
    str() the message for an assert"""

    def __init__(self, a: torch.Tensor, b: torch.Tensor):
        self.index, self.why = None, ""
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
            self.ok, self.why = False, f"{a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
            return
        ba, bb = _bits(a), _bits(b.to(a.device))
        diff = ba != bb
        self.ok = not bool(diff.any())
        if not self.ok:
            self.index = int(diff.to(torch.uint8).argmax())       # (argmax of 0/1: the first 1)
            self.why = (f"{int(diff.sum())} of {diff.numel()} elements differ, the first at flat index {self.index}: "
                        f"{a.detach().contiguous().reshape(-1)[self.index].item()!r} against "
                        f"{b.detach().contiguous().reshape(-1)[self.index].item()!r}")

    def __bool__(self):
        return self.ok

    def __str__(self):
        return "same bits" if self.ok else self.why


def same_bits(a: torch.Tensor, b: torch.Tensor) -> BitCompare:
    return BitCompare(a, b)


def assert_same_bits(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    r = same_bits(a, b)
    assert r, f"{what}: {r}"
