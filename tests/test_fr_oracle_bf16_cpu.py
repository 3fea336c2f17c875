"""CPU: the bf16-emulating precision modes of oracle/fr_oracle.py.  The emulating convolution's forward and both gradients
equal float64 convolutions of explicitly bf16-rounded operands for every conv kind the oracle uses; the rounding is
round-to-nearest-even through float32; the default mode touches none of the emulation."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fr_oracle, synth

R = fr_oracle.bf16_round


def _f32(bits: int) -> float:
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32).item()


def test_bf16_round_is_round_to_nearest_even():
    one = 0x3F800000
    cases = [(one + 0x7FFF, one), (one + 0x8000, one), (one + 0x8001, one + 0x10000),     # below / tie to even / above
             (one + 0x18000, one + 0x20000), (one + 0x10000 + 0x7FFF, one + 0x10000)]       # tie from an odd neighbour: up
    for src, want in cases:
        for sign in (1.0, -1.0):
            got = R(torch.tensor([sign * _f32(src)], dtype=torch.float64)).to(torch.float32)
            assert got.item() == sign * _f32(want), (hex(src), got.item())
    # float64 -> float32 first: a float64 value just above a bf16 tie that float32 rounds onto the tie goes to even
    tie = _f32(one + 0x8000)
    assert R(torch.tensor([tie + 2.0 ** -40], dtype=torch.float64)).item() == 1.0
    # values, range and specials survive; the result is exactly representable in bf16
    x = torch.randn(4096, dtype=torch.float64) * 10.0 ** torch.randint(-30, 30, (4096,)).double()
    r = R(x)
    assert torch.equal(r, r.to(torch.bfloat16).to(torch.float64))
    assert ((r - x).abs() <= x.abs() * 2.0 ** -8).all()
    assert torch.isinf(R(torch.tensor([float("inf")], dtype=torch.float64))).all()


def test_bf16_round_is_not_truncation():
    x = torch.tensor([_f32(0x3F80C000)], dtype=torch.float64)            # 1 + 0.75 bf16 ulp
    assert R(x).item() == _f32(0x3F810000)
    assert R(x).item() != _f32(0x3F80C000 & ~0xFFFF)


CONVS = [  # (fn, x shape, w shape, kwargs)
    (F.conv2d, (2, 5, 9, 11), (7, 5, 3, 3), dict(padding=1)),
    (F.conv2d, (2, 6, 9, 11), (4, 6, 1, 1), dict(stride=2)),
    (F.conv2d, (2, 8, 9, 11), (8, 1, 3, 3), dict(padding=1, groups=8)),
    (F.conv3d, (2, 3, 4, 9, 11), (6, 3, 1, 3, 3), dict(padding=(0, 1, 1))),
    (F.conv3d, (2, 6, 4, 5, 7), (5, 6, 3, 1, 1), dict(padding=(1, 0, 0))),
    (F.conv_transpose2d, (2, 6, 5, 7), (6, 4, 4, 4), dict(stride=2, padding=1)),
]


@pytest.mark.parametrize("case", range(len(CONVS)))
def test_emulating_conv_equals_float64_conv_of_rounded_operands(case):
    fn, xs, ws, kw = CONVS[case]
    g = torch.Generator().manual_seed(case)
    x = torch.randn(xs, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(ws, generator=g, dtype=torch.float64).requires_grad_()
    y = fr_oracle.conv(fn, x, w, prec="bf16_operands", **kw)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xr, wr, dyr = R(x.detach()), R(w.detach()), R(dy)
    assert not torch.equal(xr, x.detach()) and not torch.equal(dyr, dy)     # the rounding does something here
    assert torch.equal(y.detach(), fn(xr, wr, None, **kw))
    xa, wa = xr.clone().requires_grad_(), wr.clone().requires_grad_()
    dx_ref, dw_ref = torch.autograd.grad(fn(xa, wa, None, **kw), (xa, wa), dyr)
    torch.testing.assert_close(x.grad, dx_ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(w.grad, dw_ref, rtol=1e-12, atol=1e-12)
    if fn is F.conv2d and kw.get("groups", 1) == 1:     # the closed-form gradients of torch.nn.grad
        torch.testing.assert_close(x.grad, torch.nn.grad.conv2d_input(xs, wr, dyr, **kw), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(w.grad, torch.nn.grad.conv2d_weight(xr, ws, dyr, **kw), rtol=1e-12, atol=1e-12)
    if fn is F.conv3d:
        torch.testing.assert_close(x.grad, torch.nn.grad.conv3d_input(xs, wr, dyr, **kw), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(w.grad, torch.nn.grad.conv3d_weight(xr, ws, dyr, **kw), rtol=1e-12, atol=1e-12)


def test_emulating_conv_exact_input_gradient_and_bias():
    """exact_dgrad (the fp32 head-conv input gradient): dx from the unrounded dy and w, dw still from rounded x and dy; the
    bias gradient is the sum of the unrounded dy"""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 4, 9, 11, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(6, 3, 1, 3, 3, generator=g, dtype=torch.float64).requires_grad_()
    y = fr_oracle.conv(F.conv3d, x, w, prec="bf16_storage", exact_dgrad=True, padding=(0, 1, 1))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    torch.testing.assert_close(x.grad, torch.nn.grad.conv3d_input(x.shape, w.detach(), dy, padding=(0, 1, 1)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(w.grad, torch.nn.grad.conv3d_weight(R(x.detach()), w.shape, R(dy), padding=(0, 1, 1)),
                               rtol=1e-12, atol=1e-12)
    b = torch.randn(4, generator=g, dtype=torch.float64).requires_grad_()
    x2 = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    y2 = fr_oracle.conv(F.conv2d, x2, torch.randn(4, 6, 1, 1, generator=g, dtype=torch.float64), b, "bf16_operands")
    dy2 = torch.randn(y2.shape, generator=g, dtype=torch.float64)
    y2.backward(dy2)
    torch.testing.assert_close(b.grad, dy2.sum(dim=(0, 2, 3)), rtol=1e-12, atol=1e-12)


def test_temporal_accumulation_rounds_each_pass():
    """the time-major (3,1,1) conv with bf16 storage: three passes, each rounded, in the HIP launch order"""
    g = torch.Generator().manual_seed(3)
    x = R(torch.randn(2, 5, 4, 3, 6, generator=g, dtype=torch.float64)).requires_grad_()
    w = torch.randn(6, 5, 3, 1, 1, generator=g, dtype=torch.float64).requires_grad_()
    y = fr_oracle._Bf16TemporalAccum.apply(x, w)
    wr, xr = R(w.detach()), x.detach()
    tap = lambda k, a: torch.einsum("oi,bithw->bothw", wr[:, :, k, 0, 0], a)   # noqa: E731
    T = x.shape[2]
    for t in range(T):
        v = R(tap(1, xr[:, :, t:t + 1]))
        if t >= 1:
            v = R(v + tap(0, xr[:, :, t - 1:t]))
        if t <= T - 2:
            v = R(v + tap(2, xr[:, :, t + 1:t + 2]))
        assert torch.equal(y.detach()[:, :, t:t + 1], v), t
    # not the singly rounded conv, though close to it
    one = R(F.conv3d(xr, wr, None, padding=(1, 0, 0)))
    assert not torch.equal(y.detach(), one)
    assert (y.detach() - one).norm() < 1e-2 * one.norm()
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xa, wa = xr.clone().requires_grad_(), wr.clone().requires_grad_()
    dx_ref, dw_ref = torch.autograd.grad(F.conv3d(xa, wa, None, padding=(1, 0, 0)), (xa, wa), R(dy))
    torch.testing.assert_close(w.grad, dw_ref, rtol=1e-12, atol=1e-12)
    assert not torch.equal(x.grad, R(dx_ref)) and (x.grad - dx_ref).norm() < 1e-2 * dx_ref.norm()


def _step(prec, time_major=False, train=True, base=16, H=64, W=64):
    sd = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN)
    P = {k: (v.double().clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    clip = synth.formula_clip(2, 3, H, W)
    xs = [clip[:, 0].double().requires_grad_(), clip[:, 1:].double().requires_grad_(),
          (0.05 + 0.9 * torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(1))).double().requires_grad_()]
    out = fr_oracle.frame_recovery_forward(P, *xs, train, prec=prec, time_major=time_major)
    F.mse_loss(out, synth.formula_target(2, H, W).double()).backward()
    return out.detach(), {k: v.grad for k, v in P.items() if v.grad is not None}, {k: v for k, v in P.items() if "running" in k}, \
        [x.grad for x in xs]


def _flat(r):
    out, grads, bufs, dx = r
    return [out] + list(grads.values()) + [b.detach() for b in bufs.values()] + dx


def test_default_mode_uses_no_emulation(monkeypatch):
    """prec=None runs the plain float64 graph: with every emulation entry point poisoned it still runs, bit-identical to an
    unpoisoned run"""
    ref = _flat(_step(None))

    def boom(*a, **k):
        raise AssertionError("emulation used in the default mode")
    for cls in (fr_oracle._Bf16Conv, fr_oracle._Bf16Store, fr_oracle._Bf16GradOnly, fr_oracle._Bf16TemporalAccum):
        monkeypatch.setattr(cls, "apply", boom)
    monkeypatch.setattr(fr_oracle, "bf16_round", boom)
    got = _flat(_step(None))
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    x, w = torch.randn(1, 4, 6, 6, dtype=torch.float64), torch.randn(3, 4, 3, 3, dtype=torch.float64)
    assert torch.equal(fr_oracle.conv(F.conv2d, x, w, None, None, padding=1), F.conv2d(x, w, None, padding=1))


@pytest.mark.parametrize("prec,time_major", [("bf16_operands", False), ("bf16_storage", False), ("bf16_storage", True)])
def test_emulating_modes_differ_from_default_and_from_each_other(prec, time_major):
    """every mode changes the result (its rounding points are reached) and stays a small perturbation of the forward pass"""
    plain = _step(None, train=False)
    got = _step(prec, time_major, train=False)
    d = (got[0] - plain[0]).abs().max().item()
    assert 0 < d < 5e-2, d
    if prec == "bf16_storage":
        other = _step("bf16_operands", train=False)
        assert not torch.equal(got[0], other[0])
        if time_major:
            assert not torch.equal(got[0], _step("bf16_storage", False, train=False)[0])


def test_bad_precision_is_refused():
    with pytest.raises(ValueError):
        _step("bf16")
