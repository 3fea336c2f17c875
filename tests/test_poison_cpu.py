"""CPU: the poisoned-buffer helper (tests/_poison.py) proved on its own - every wrapped entry point poisons floating tensors
and leaves the others alone, a toy op that reads one element it never wrote is flagged while the same op without the read
passes, and `same_bits` is equality of bit patterns."""
import pytest
import torch

import _poison as P

FLOATS = [torch.float32, torch.bfloat16, torch.float64]
OTHERS = [torch.int32, torch.int64, torch.uint8, torch.bool]

# every wrapped entry point as (name, call(dtype) -> tensor)
ENTRY_POINTS = [
    ("torch.empty(shape)", lambda dt: torch.empty((3, 5), dtype=dt)),
    ("torch.empty(*sizes)", lambda dt: torch.empty(3, 5, dtype=dt)),
    ("torch.empty_like", lambda dt: torch.empty_like(torch.zeros(3, 5, dtype=dt))),
    ("torch.empty_like(dtype=)", lambda dt: torch.empty_like(torch.zeros(3, 5, dtype=torch.int16), dtype=dt)),
    ("torch.empty_strided", lambda dt: torch.empty_strided((3, 5), (8, 1), dtype=dt)),
    ("Tensor.new_empty", lambda dt: torch.zeros(2, dtype=dt).new_empty((3, 5))),
    ("Tensor.new_empty(dtype=)", lambda dt: torch.zeros(2, dtype=torch.int16).new_empty((3, 5), dtype=dt)),
]


def _all_nan(t):
    return bool(torch.isnan(t.double()).all())


@pytest.mark.parametrize("name,call", ENTRY_POINTS, ids=[e[0] for e in ENTRY_POINTS])
def test_every_entry_point_poisons_floats_and_only_floats(monkeypatch, name, call):
    log = P.poisoned_allocations(monkeypatch)
    for dt in FLOATS:
        t = call(dt)
        assert t.dtype == dt and tuple(t.shape) == (3, 5) and _all_nan(t), (name, dt)
    assert (log.tensors, log.untouched) == (len(FLOATS), 0)
    assert log.bytes == 15 * (4 + 2 + 8)
    for dt in OTHERS:
        t = call(dt)
        assert t.dtype == dt and tuple(t.shape) == (3, 5), (name, dt)
    # integer and index buffers pass through the wrapper without being written: the poisoned count did not move
    assert (log.tensors, log.untouched) == (len(FLOATS), len(OTHERS))
    monkeypatch.undo()
    assert torch.empty.__name__ == "empty" and not hasattr(torch.empty, "__wrapped__")
    assert not hasattr(torch.Tensor.new_empty, "__wrapped__")


def test_the_wrapper_is_seen_through_a_module_that_looks_torch_empty_up_at_call_time(monkeypatch):
    """nerve_cl._engine._new and nerve_cl._ops._new are `(torch.zeros if zero else torch.empty)(shape, ...)`: the attribute is
    read at every call, so the engine's allocations go through the wrapper; zero=True stays zero"""
    def _new(*shape, dtype=torch.float32, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype)
    P.poisoned_allocations(monkeypatch)
    assert _all_nan(_new(4, 4)) and _all_nan(_new(4, 4, dtype=torch.bfloat16))
    assert torch.equal(_new(4, 4, zero=True), torch.zeros(4, 4))
    assert _new(4, dtype=torch.int32).dtype == torch.int32


def test_poison_fills_floats_in_place_and_refuses_the_rest():
    for dt in FLOATS:
        t = torch.ones(7, dtype=dt)
        view = t[2:5]
        assert P.poison_(view) is view
        assert _all_nan(t[2:5]) and bool((t[:2] == 1).all()) and bool((t[5:] == 1).all())
    for dt in OTHERS:
        with pytest.raises(AssertionError):
            P.poison_(torch.ones(7, dtype=dt))


# ----------------------------------------------------------------------------- a seeded defect
def _toy_row_sums(x, read_the_pad):
    """row sums of x [R, 5] through a scratch buffer with a pixel stride of 8, as CatBuf's CATLD = 256 for CAT = 224: columns
    5 .. 7 are never written.  read_the_pad: the defect - the sum runs over 6 columns, one more than was written."""
    scratch = torch.empty(x.shape[0], 8)
    scratch[:, :5] = x
    return scratch[:, :6 if read_the_pad else 5].sum(dim=1)


def _clean_and_poisoned(monkeypatch, fn):
    """fn() on finite scratch memory (a fixed finite filler stands for whatever the allocator hands out: recycled CPU memory
    is not repeatable, and could even be an earlier test's NaN) and fn() on poisoned memory"""
    with monkeypatch.context() as m:
        real = torch.empty
        m.setattr(torch, "empty", lambda *a, **k: real(*a, **k).fill_(0))
        clean = fn()
    with monkeypatch.context() as m:
        P.poisoned_allocations(m)
        poisoned = fn()
    return clean, poisoned


def test_a_read_of_one_unwritten_element_is_flagged_and_its_absence_passes(monkeypatch):
    x = torch.arange(20.0).view(4, 5)
    clean, poisoned = _clean_and_poisoned(monkeypatch, lambda: _toy_row_sums(x, True))
    # on zeros the defect is invisible to a value check - this is what the suite could not see ...
    assert torch.equal(clean, x.sum(dim=1))
    # ... and on poisoned memory it is not
    r = P.same_bits(clean, poisoned)
    assert not r and r.index == 0 and "4 of 4" in str(r)
    with pytest.raises(AssertionError, match="row sums"):
        P.assert_same_bits(clean, poisoned, "row sums")
    clean, poisoned = _clean_and_poisoned(monkeypatch, lambda: _toy_row_sums(x, False))
    assert P.same_bits(clean, poisoned) and torch.equal(poisoned, x.sum(dim=1))


def test_a_multiplied_mask_is_flagged_and_a_select_passes(monkeypatch):
    """the halo / K-chunk form of the defect: an over-read that is masked by a multiplication with zero lets a NaN through,
    the same over-read masked by a select does not"""
    x, w = torch.arange(1.0, 6.0), torch.tensor([1.0, 1, 1, 1, 1, 0, 0, 0])

    def dot(select):
        buf = torch.empty(8)
        buf[:5] = x
        return (torch.where(w != 0, buf, torch.zeros(())) * w).sum() if select else (buf * w).sum()

    clean, poisoned = _clean_and_poisoned(monkeypatch, lambda: dot(False))
    assert clean.item() == 15.0 and not P.same_bits(clean, poisoned)
    clean, poisoned = _clean_and_poisoned(monkeypatch, lambda: dot(True))
    assert clean.item() == 15.0 and P.same_bits(clean, poisoned)


# ----------------------------------------------------------------------------- same_bits
def test_same_bits_is_equality_of_bit_patterns():
    nan = float("nan")
    a = torch.tensor([1.0, nan, 0.0, -2.5])
    assert P.same_bits(a, a.clone())                                    # NaN equals the same NaN
    assert not torch.equal(a, a.clone())                                # (which value equality denies)
    z = P.same_bits(torch.tensor([1.0, 0.0, 3.0]), torch.tensor([1.0, -0.0, 3.0]))
    assert not z and z.index == 1                                       # -0 differs from +0
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))      # (which value equality denies too)
    # a NaN of another payload is another bit pattern
    other = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert torch.isnan(other).all() and not P.same_bits(torch.tensor([nan]), other)
    # the first differing index, in flat order, whatever the shape
    b = torch.zeros(3, 4)
    c = b.clone()
    c[1, 2] = 1e-45
    c[2, 0] = 5.0
    r = P.same_bits(b, c)
    assert not r and r.index == 6 and "2 of 12" in str(r)
    # every storage type of the project; shape and dtype are part of the comparison
    for dt in FLOATS + [torch.int32, torch.bool]:
        t = torch.tensor([1, 0, 1, 1]).to(dt)
        assert P.same_bits(t, t.clone())
        u = t.clone()
        u[3] = 0
        assert P.same_bits(t, u).index == 3
    assert not P.same_bits(torch.zeros(4), torch.zeros(2, 2))
    assert not P.same_bits(torch.zeros(4), torch.zeros(4, dtype=torch.bfloat16))
    assert P.same_bits(torch.zeros(0), torch.zeros(0))
    # non-contiguous views compare by their logical elements
    m = torch.arange(12.0).view(3, 4)
    assert P.same_bits(m.t(), m.t().contiguous())
