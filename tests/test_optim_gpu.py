"""GPU: nvq_adam_step (csrc/optim.hip) against the float64 recurrence within the derived bound of tests/optim_worker.py, and
nerve_cl.optim.BucketAdam / BucketAdamW on the product path: the engine's flat parameter and gradient buckets in place, frozen
layers, param groups, schedulers, accumulated gradients, state-dict exchange with torch.optim, clipping, weight EMA, HIP-graph
steps, two data-parallel ranks.

Class tests: a deepcopy of the engine under torch.optim.Adam / AdamW (fused=False) is fed the same gradients at every step, so the
two trajectories are compared step by step instead of diverging through the network; the bound is the theta bound with torch's
result in the place of the float64 one."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from optim_worker import AdamF64, theta_bound_against

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 12345.678
STRIDE_LOOP = 1_050_001          # > 1024 blocks x 256 threads x one quad: some thread takes a second trip, plus a one-float tail


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.detach().clone().view(torch.int32)


class _Buf:
    """n floats between two sentinels; offset 1: the floats start 4 bytes past a 16-byte boundary"""

    def __init__(self, values: torch.Tensor, offset: int):
        n = values.numel()
        self.start = 4 + offset
        self.full = torch.full((self.start + n + 1,), SENTINEL, dtype=torch.float32, device=_dev())
        self.t = self.full[self.start:self.start + n]
        self.t.copy_(values)
        assert n == 0 or self.t.data_ptr() % 16 == 4 * offset

    def intact(self) -> bool:
        s = torch.tensor(SENTINEL, dtype=torch.float32)
        return bool((self.full[:self.start].cpu() == s).all()) and bool(self.full[-1].cpu() == s)


def _inputs(n, seed, steps, grads="randn", s=1.0):
    gen = torch.Generator().manual_seed(seed)
    theta = 0.1 * torch.randn(n, generator=gen)
    if grads == "randn":
        gs = [torch.randn(n, generator=gen) * s for _ in range(steps)]
    else:                                           # random sign times U[0.5, 1.5]
        gs = [(torch.randint(0, 2, (n,), generator=gen) * 2 - 1) * (0.5 + torch.rand(n, generator=gen)) for _ in range(steps)]
    return theta, gs


def _run(theta, gs, offsets, *, ema=True, acc=None, max_norm=0.0, **hyper):
    """the kernel on fresh buffers at the given offsets (theta, grad, m, v, ema) -> the buffers after len(gs) steps"""
    from nerve_cl import _nvq
    n = theta.numel()
    zeros = torch.zeros(n)
    bt, bg, bm, bv, be = (_Buf(x, o) for x, o in zip((theta, zeros, zeros, zeros, theta), offsets))
    for k, g in enumerate(gs):
        bg.t.copy_(g)
        gbits = _bits(bg.t)
        _nvq.adam_step(bt.t, bg.t, bm.t, bv.t, be.t if ema else None, step=k + 1, ema_decay=0.9 if ema else 0.0, acc=acc,
                       max_norm=max_norm, **hyper)
        assert torch.equal(_bits(bg.t), gbits)                         # grad is never written
    torch.cuda.synchronize()
    for b in (bt, bg, bm, bv, be):
        assert b.intact()
    if not ema:
        assert torch.equal(be.t.cpu(), theta)
    return bt.t, bm.t, bv.t, be.t


HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, decoupled=True)


# ------------------------------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, STRIDE_LOOP])
def test_kernel_sizes_alignments_and_bounds(n):
    """two steps at every size: all buffers 16-byte aligned, all 4 bytes off, only grad 4 bytes off - the same bits, the
    sentinels on either side of every buffer intact, and within the bound of the float64 recurrence"""
    theta, gs = _inputs(n, 100 + n % 89, 2)
    aligned = _run(theta, gs, (0, 0, 0, 0, 0), **HYPER)
    shifted = _run(theta, gs, (1, 1, 1, 1, 1), **HYPER)
    grad_only = _run(theta, gs, (0, 1, 0, 0, 0), **HYPER)
    for a, b, c in zip(aligned, shifted, grad_only):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    ref = AdamF64(theta, 1e-3, weight_decay=1e-2, decoupled=True, ema_decay=0.9)
    for g in gs:
        ref.step(g)
    ref.check(*aligned, what=f"n={n}")


ACCURACY = [(dec, wd, lr, "randn", s) for dec, wd in ((False, 0.0), (True, 1e-2)) for lr in (1e-3, 1e-4) for s in (1e-3, 1.0)] \
    + [(False, 1e-2, lr, "sign", None) for lr in (1e-3, 1e-4)]


@pytest.mark.parametrize("decoupled,wd,lr,grads,s", ACCURACY)
def test_kernel_accuracy_after_ten_steps(decoupled, wd, lr, grads, s):
    """K = 10, theta_0 = 0.1 randn: no weight decay and AdamW(1e-2) on randn * s gradients, Adam with L2 decay 1e-2 on random sign
    times U[0.5, 1.5] (gradients near zero would make g + wd * theta cancel: ill-conditioned in any precision)"""
    theta, gs = _inputs(4099, 7, 10, grads, s if s is not None else 1.0)
    got = _run(theta, gs, (0, 0, 0, 0, 0), lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, decoupled=decoupled)
    ref = AdamF64(theta, lr, weight_decay=wd, decoupled=decoupled, ema_decay=0.9)
    for g in gs:
        ref.step(g)
    ref.check(*got, what=f"decoupled={decoupled} wd={wd} lr={lr} {grads} s={s}")


def test_kernel_without_an_ema_gives_the_same_bits():
    theta, gs = _inputs(4099, 11, 2)
    with_ema = _run(theta, gs, (0, 0, 0, 0, 0), **HYPER)
    without = _run(theta, gs, (0, 0, 0, 0, 0), ema=False, **HYPER)
    for a, b in zip(with_ema[:3], without[:3]):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(with_ema[3].cpu(), theta)


def test_kernel_clip_cases():
    theta, gs = _inputs(4099, 12, 2)
    plain = _run(theta, gs, (0, 0, 0, 0, 0), **HYPER)
    acc = torch.zeros(5, dtype=torch.float64, device=_dev())
    acc[2] = 16.0                                                       # norm 4
    clipped = _run(theta, gs, (1, 1, 1, 1, 1), acc=acc, max_norm=1.0, **HYPER)       # coef = 1 / (4 + 1e-6) < 1: scaled
    ref = AdamF64(theta, 1e-3, weight_decay=1e-2, decoupled=True, ema_decay=0.9)
    for g in gs:
        ref.step(g, max_norm=1.0, total_norm=4.0)
    ref.check(*clipped, what="clipped")
    assert not torch.equal(_bits(clipped[1]), _bits(plain[1]))
    for case, value, max_norm in (("coef >= 1", 16.0, 4.5), ("coef == 1 exactly is not < 1", 0.0, 1e-6), ("nan", float("nan"), 1.0)):
        acc[2] = value
        got = _run(theta, gs, (0, 0, 0, 0, 0), acc=acc, max_norm=max_norm, **HYPER)
        for a, b in zip(got, plain):
            assert torch.equal(_bits(a), _bits(b)), case


def test_kernel_on_nothing_and_refusals():
    from nerve_cl import _nvq
    e = torch.empty(0, device=_dev())
    _nvq.adam_step(e, e, e, e, None, step=1, **HYPER)                  # n == 0: success, no launch
    t = torch.zeros(4, 8, device=_dev())
    lib, (p, g, m, v) = _nvq.lib(), [_nvq.ptr(row) for row in t]
    tail = (1e-3, 0.9, 0.999, 0.1, 1e-3, 1e-8, 0.0, 0, 0.1, 0.03, 0.0, None, 0.0, None)
    assert lib.nvq_adam_step(p, g, m, v, None, 7, *tail) == 0
    assert lib.nvq_adam_step(None, g, m, v, None, 7, *tail) != 0       # NULL theta
    assert lib.nvq_adam_step(p, None, m, v, None, 7, *tail) != 0       # NULL grad
    assert lib.nvq_adam_step(p, g, m, v, None, -1, *tail) != 0         # negative n
    assert lib.nvq_adam_step(p, g + 2, m, v, None, 7, *tail) != 0      # not 4-byte aligned
    assert b"adam_step" in lib.nvq_last_error()
    torch.cuda.synchronize()
    assert not t.any()                                                  # zeros (bucket padding) stay exactly zero


# ------------------------------------------------------------------------------------------------- the product path

CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B, H, W = 2, 16, 24


def _engine(**extra):
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG, **extra))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    return eng.to(_dev()).train()


def _data():
    from oracle import synth
    x, y = synth.formula_clip(B, 3, H, W), synth.formula_target(B, 2 * H, 2 * W)
    return x.to(_dev()), y.to(_dev())


def _aliases_bucket(net) -> bool:
    lay, _ = net._bucket_layout()
    base = net._last_grad_bucket.data_ptr()
    return all(p.grad is None or p.grad.data_ptr() == base + 4 * lay[n][0] for n, p in net.named_parameters())


def _views_of_flat_theta(net) -> bool:
    lay, _ = net._bucket_layout()
    base = net.flat_theta().data_ptr()
    return all(p.data_ptr() == base + 4 * lay[n][0] for n, p in net.named_parameters())


def _backward(eng, x, y, backwards=1):
    for _ in range(backwards):
        F.mse_loss(eng(x)["enhanced"], y).backward()


def _share_grads(eng, twin):
    for p, q in zip(eng.parameters(), twin.parameters()):
        q.grad = None if p.grad is None else p.grad.detach().clone()


def _steps(eng, twin, opt, ref, x, y, steps, backwards=1, after=None):
    for _ in range(steps):
        opt.zero_grad()
        _backward(eng, x, y, backwards)
        _share_grads(eng, twin)
        opt.step()
        ref.step()
        if after is not None:
            after()


def _within_bound(eng, twin, start, steps, lr_of=lambda name: 1e-3):
    worst = 0.0
    for (n, p), q in zip(eng.named_parameters(), twin.parameters()):
        worst = max(worst, theta_bound_against(start[n], p, q, steps, lr_of(n)))
    print(f"largest difference to torch.optim / bound = {worst:.3f}")
    assert worst <= 1.0
    return worst


def _start(eng):
    return {n: p.detach().clone() for n, p in eng.named_parameters()}


def _padding_is_zero(net, *flats) -> bool:
    lay, total = net._bucket_layout()
    pad = torch.ones(total, dtype=torch.bool, device=_dev())
    for o, k in lay.values():
        pad[o:o + k] = False
    assert pad.any()
    return not any(bool(f[pad].any()) for f in flats)


def test_all_trainable_in_one_group_is_one_launch():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt, ref = BucketAdam(eng.parameters(), lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3, fused=False)
    launches = []
    _steps(eng, twin, opt, ref, x, y, 5, after=lambda: launches.append(opt.last_launches))
    assert launches == [1] * 5 and _aliases_bucket(eng.super_resolution)
    _within_bound(eng, twin, start, 5)
    assert any(not torch.equal(p, start[n]) for n, p in eng.named_parameters())
    ns = opt._nets[0]
    assert _padding_is_zero(eng.super_resolution, eng.super_resolution.flat_theta(), ns.m, ns.v)
    assert _views_of_flat_theta(eng.super_resolution)
    p = next(eng.super_resolution.parameters())
    assert int(opt.state[p]["step"]) == 5 and opt.state[p]["exp_avg"].shape == p.shape
    assert eng.enhancement_strength not in opt.state                    # no gradient reached it: skipped, no state


def test_frozen_prefix_is_never_touched_and_costs_one_launch():
    from nerve_cl.optim import BucketAdamW
    eng = _engine()
    for p in eng.super_resolution.feature_extractor.parameters():
        p.requires_grad_(False)
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt = BucketAdamW(eng.parameters(), lr=1e-3, weight_decay=0.1)
    ref = torch.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=0.1, fused=False)
    launches = []
    _steps(eng, twin, opt, ref, x, y, 3, after=lambda: launches.append(opt.last_launches))
    assert launches == [1] * 3
    for n, p in eng.super_resolution.feature_extractor.named_parameters():
        assert torch.equal(_bits(p), _bits(start["super_resolution.feature_extractor." + n])) and p not in opt.state
    _within_bound(eng, twin, start, 3)
    assert _padding_is_zero(eng.super_resolution, eng.super_resolution.flat_theta(), opt._nets[0].m, opt._nets[0].v)


def _two_groups(eng, lr):
    motion = list(eng.super_resolution.motion_estimator.parameters())
    ids = {id(p) for p in motion}
    return [{"params": [p for p in eng.parameters() if id(p) not in ids]}, {"params": motion, "lr": 0.25 * lr}]


def test_two_groups_and_a_scheduler():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt = BucketAdam(_two_groups(eng, 1e-3), lr=1e-3)
    ref = torch.optim.Adam(_two_groups(twin, 1e-3), lr=1e-3, fused=False)
    sa, sb = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5), torch.optim.lr_scheduler.StepLR(ref, 1, 0.5)
    launches = []

    def after():
        launches.append(opt.last_launches)
        sa.step()
        sb.step()
    _steps(eng, twin, opt, ref, x, y, 2, after=after)
    assert launches == [3, 3]                   # feature extractor | motion estimator at its own lr | everything behind it
    assert opt.param_groups[1]["lr"] == ref.param_groups[1]["lr"] == 0.25e-3 / 4
    _within_bound(eng, twin, start, 2, lambda n: 0.25e-3 if ".motion_estimator." in n else 1e-3)
    # the rates matter: Adam's first step moves an element by its lr, the second (lr halved) by at most about as much again
    moved = {True: 0.0, False: 0.0}
    for n, p in eng.super_resolution.named_parameters():
        key = n.startswith("motion_estimator.")
        moved[key] = max(moved[key], (p.detach() - start["super_resolution." + n]).abs().max().item())
    assert 0.2e-3 <= moved[True] <= 0.4e-3 and moved[False] >= 0.9e-3


def test_accumulated_gradients_take_the_per_tensor_path():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt, ref = BucketAdam(eng.parameters(), lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3, fused=False)
    _steps(eng, twin, opt, ref, x, y, 2, backwards=2)
    assert not _aliases_bucket(eng.super_resolution)
    assert opt.last_launches == sum(1 for p in eng.super_resolution.parameters() if p.numel())
    _within_bound(eng, twin, start, 2)
    assert _padding_is_zero(eng.super_resolution, eng.super_resolution.flat_theta(), opt._nets[0].m, opt._nets[0].v)


def test_a_parameter_without_a_gradient_is_skipped():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt, ref = BucketAdam(eng.parameters(), lr=1e-3, weight_decay=0.1), torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=0.1, fused=False)
    _steps(eng, twin, opt, ref, x, y, 1)
    names = [n for n, _ in eng.super_resolution.named_parameters()]
    skipped_name = names[len(names) // 2]
    skipped = dict(eng.super_resolution.named_parameters())[skipped_name]
    before = _bits(skipped)
    opt.zero_grad()
    _backward(eng, x, y)
    skipped.grad = None
    _share_grads(eng, twin)
    opt.step()
    ref.step()
    assert opt.last_launches == 2                                       # the slots in front of it and those behind it
    assert torch.equal(_bits(skipped), before) and int(opt.state[skipped]["step"]) == 1
    assert all(int(opt.state[p]["step"]) == 2 for n, p in eng.super_resolution.named_parameters() if n != skipped_name)
    _within_bound(eng, twin, start, 2)
    _steps(eng, twin, opt, ref, x, y, 1)                                # step counts 2 | 1 | 2 -> three runs, still torch's values
    assert opt.last_launches == 3
    _within_bound(eng, twin, start, 3)


def test_state_dict_travels_in_both_directions():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    opt, ref = BucketAdam(eng.parameters(), lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3, fused=False)
    _steps(eng, twin, opt, ref, x, y, 2)
    eng2, twin2 = copy.deepcopy(eng), copy.deepcopy(twin)
    opt2, ref2 = BucketAdam(eng2.parameters()), torch.optim.Adam(twin2.parameters(), fused=False)
    opt2.load_state_dict(copy.deepcopy(ref.state_dict()))               # torch's into this class (on the torch trajectory's weights)
    ref2.load_state_dict(copy.deepcopy(opt.state_dict()))               # this class's into torch
    with torch.no_grad():
        for p, q in zip(eng2.parameters(), twin.parameters()):
            p.copy_(q)
        for p, q in zip(twin2.parameters(), eng.parameters()):
            p.copy_(q)
    start, start2 = _start(twin), _start(eng)
    opt.zero_grad()
    _backward(eng, x, y)
    for other in (twin, eng2, twin2):
        _share_grads(eng, other)
    for o in (opt, ref, opt2, ref2):
        o.step()
    assert opt2.last_launches == len([p for p in eng2.super_resolution.parameters()])    # foreign gradients: per tensor
    _within_bound(eng2, twin, start, 1)                                 # torch state -> BucketAdam continues like torch
    _within_bound(eng, twin2, start2, 1)                                # BucketAdam state -> torch continues like BucketAdam
    p2 = next(eng2.super_resolution.parameters())
    assert int(opt2.state[p2]["step"]) == 3
    assert opt2.state[p2]["exp_avg"].data_ptr() == opt2._nets[0].m.data_ptr()       # views of the flat state again


def test_after_model_to_and_after_deepcopy_the_next_step_is_correct():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    opt, ref = BucketAdam(eng.parameters(), lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3, fused=False)
    _steps(eng, twin, opt, ref, x, y, 1)
    old = eng.super_resolution.flat_theta().data_ptr()
    eng.to("cpu")
    eng.to(_dev())                                                      # every parameter lives somewhere else now
    _steps(eng, twin, opt, ref, x, y, 1)
    assert opt.last_launches == 1 and _views_of_flat_theta(eng.super_resolution)
    assert eng.super_resolution.flat_theta().data_ptr() != old
    _within_bound(eng, twin, start, 2)
    eng2 = copy.deepcopy(eng)
    opt2 = BucketAdam(eng2.parameters(), lr=1e-3)
    assert opt2._nets[0].net is eng2.super_resolution
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    for e, o in ((eng, opt), (eng2, opt2)):
        o.zero_grad()
        _backward(e, x, y)
        o.step()
    assert opt2.last_launches == 1
    for p, q in zip(eng.parameters(), eng2.parameters()):
        assert torch.equal(_bits(p), _bits(q))
    _share_grads(eng, twin)
    ref.step()
    _within_bound(eng, twin, start, 3)


def test_max_grad_norm_equals_clip_grad_norm_then_a_plain_step():
    from nerve_cl import ops
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    twin = copy.deepcopy(eng)
    x, y = _data()
    start = _start(eng)
    _backward(eng, x, y)
    norm0 = torch.cat([p.grad.reshape(-1) for p in eng.parameters() if p.grad is not None]).double().norm().item()
    for max_norm, clips in ((0.5 * norm0, True), (1e3 * norm0, False)):
        opt, ref = BucketAdam(eng.parameters(), lr=1e-3, max_grad_norm=max_norm), BucketAdam(twin.parameters(), lr=1e-3)
        opt.zero_grad()
        _backward(eng, x, y)
        _share_grads(eng, twin)
        before = {n: _bits(p.grad) for n, p in eng.named_parameters() if p.grad is not None}
        want = torch.cat([p.grad.reshape(-1) for p in eng.parameters() if p.grad is not None]).double().norm().item()
        returned = ops.clip_grad_norm_(list(twin.parameters()), max_norm)
        opt.step()
        ref.step()
        assert opt.last_launches == 1
        norm = opt.last_grad_norm
        assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
        assert abs(norm.item() - returned.item()) <= 2.0 ** -23 * want and abs(norm.item() - want) <= 2.0 ** -23 * want
        for n, p in eng.named_parameters():                            # .grad is left unscaled
            assert p.grad is None or torch.equal(_bits(p.grad), before[n])
        scaled = any(not torch.equal(p.grad, q.grad) for p, q in zip(eng.parameters(), twin.parameters()) if p.grad is not None)
        assert scaled == clips
        _within_bound(eng, twin, start, 1)
        start = _start(twin)
        with torch.no_grad():
            for p, q in zip(eng.parameters(), twin.parameters()):
                p.copy_(q)


def test_ema_follows_the_float64_recurrence_and_swaps_in_place():
    from nerve_cl.optim import BucketAdam
    eng = _engine()
    x, y = _data()
    decay, steps = 0.75, 4
    opt = BucketAdam(eng.named_parameters(), lr=1e-3, ema_decay=decay)
    want = {n: p.detach().double().clone() for n, p in eng.named_parameters()}
    scale = {n: p.detach().double().abs() for n, p in eng.named_parameters()}
    for _ in range(steps):
        opt.zero_grad()
        _backward(eng, x, y)
        opt.step()
        for n, p in eng.named_parameters():
            if p.grad is not None:
                want[n] = decay * want[n] + (1 - decay) * p.detach().double()
                scale[n] = torch.maximum(scale[n], p.detach().double().abs())
    assert opt.last_launches == 1
    ema = opt.ema_state_dict()
    assert list(ema) == [n for n, _ in eng.named_parameters()]
    moved = False
    for n, p in eng.named_parameters():
        # one subtraction and one fma per step, on the fp32 thetas the recurrence was fed: 2^-23 max(|ema|, |theta|) each
        assert bool(((ema[n].double() - want[n]).abs() <= steps * 2.0 ** -23 * scale[n]).all()), n
        moved = moved or not torch.equal(ema[n], p)
    assert moved and _padding_is_zero(eng.super_resolution, opt._nets[0].ema)
    eng.eval()
    now = {n: _bits(p) for n, p in eng.named_parameters()}
    flat_ptr = eng.super_resolution.flat_theta().data_ptr()
    with torch.no_grad():
        out = eng(x)["enhanced"].clone()
        with opt.swap_ema():
            assert _views_of_flat_theta(eng.super_resolution) and eng.super_resolution.flat_theta().data_ptr() == flat_ptr
            for n, p in eng.named_parameters():
                assert bool(((p.double() - want[n]).abs() <= steps * 2.0 ** -23 * scale[n]).all())
            out_ema = eng(x)["enhanced"].clone()
        again = eng(x)["enhanced"]
    assert not torch.equal(out, out_ema) and torch.equal(out, again)
    assert all(torch.equal(_bits(p), now[n]) for n, p in eng.named_parameters())
    assert _views_of_flat_theta(eng.super_resolution) and eng.super_resolution.flat_theta().data_ptr() == flat_ptr
    fresh = _engine()
    res = fresh.load_state_dict(opt.ema_state_dict(), strict=False)
    assert not res.unexpected_keys
    assert all(torch.equal(p, ema[n]) for n, p in fresh.named_parameters())
    eng2 = copy.deepcopy(eng)                                           # its averages start as the weights, not as opt's averages
    opt2 = BucketAdam(eng2.named_parameters(), lr=1e-3, ema_decay=decay)
    assert not torch.equal(opt2._nets[0].ema, opt._nets[0].ema)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))               # the "ema" key: the averages land in the flat tensor
    assert torch.equal(opt2._nets[0].ema, opt._nets[0].ema) and torch.equal(opt2._nets[0].m, opt._nets[0].m)
    ref = torch.optim.Adam(copy.deepcopy(eng).parameters(), fused=False)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))                # torch ignores the key
    assert len(ref.state) == len(opt.state)
    teacher = copy.deepcopy(eng)
    opt.copy_ema_to(teacher)
    with torch.no_grad():
        assert torch.equal(teacher.eval()(x)["enhanced"], out_ema)


def test_hip_graph_steps_match_eager_steps_bit_for_bit():
    from nerve_cl.optim import BucketAdamW
    x, y = _data()
    results = []
    for graphs in (True, False):
        eng = _engine()
        eng.super_resolution.use_hip_graphs = graphs
        for _ in range(2):                                              # two eager warm-up calls, capture on the third
            eng.zero_grad()
            _backward(eng, x, y)
        opt = BucketAdamW(eng.parameters(), lr=1e-3, max_grad_norm=1e-3, ema_decay=0.9)
        for _ in range(3):
            opt.zero_grad()
            _backward(eng, x, y)
            opt.step()
            assert opt.last_launches == 1 and _aliases_bucket(eng.super_resolution)
        assert eng.super_resolution._step_graphs.replays == (3 if graphs else 0)
        ns = opt._nets[0]
        results.append([_bits(t) for t in (eng.super_resolution.flat_theta(), ns.m, ns.v, ns.ema)])
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- data parallel

def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_two_ranks_stay_bit_identical(tmp_path):
    out = tmp_path / "optim.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    # children are ordinary child processes of a launcher that never touches the GPU
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(HERE, "optim_worker.py"), str(out)], env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out, weights_only=True)
    assert got["launches"] == [1, 1, 1]
    for key in ("theta", "ema", "norm"):
        assert torch.equal(got[key][0].view(torch.int32), got[key][1].view(torch.int32)), key
    assert got["norm"][0] > 1e-3                                        # every step clipped
    import optim_worker as Wk
    start = Wk.make_engine().super_resolution
    lay, _ = start._bucket_layout()
    first = next(iter(lay))
    o, k = lay[first]
    assert not torch.equal(got["theta"][0][o:o + k], dict(start.named_parameters())[first].detach().reshape(-1))


# ------------------------------------------------------------------------------------------------- the scripts

def _script(args, cwd):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(600)
def test_train_continual_with_the_bucket_optimizer_clipping_and_ema(tmp_path):
    exp = os.path.join(os.path.dirname(HERE), "experiments")
    out = _script([os.path.join(exp, "train_continual.py"), "--strategy", "ewc", "--tasks", "2", "--samples", "16", "--epochs", "1",
                   "--features", "16", "--blocks", "1", "--clip-grad-norm", "1.0", "--ema-decay", "0.9"], tmp_path)
    assert "Registered task 1 for EWC protection" in out and "Training complete!" in out
    sd = torch.load(tmp_path / "checkpoints" / "continual_model.pt", weights_only=True)
    ema = torch.load(tmp_path / "checkpoints" / "continual_model_ema.pt", weights_only=True)
    assert list(sd) == list(ema)
    moved = [k for k in sd if sd[k].is_floating_point() and not torch.equal(sd[k], ema[k])]
    assert moved and all(".running_" not in k and "num_batches" not in k for k in moved)      # parameters only, and the weights are back


@pytest.mark.timeout(600)
def test_train_baseline_with_an_ema_validates_and_saves_the_average(tmp_path):
    exp = os.path.join(os.path.dirname(HERE), "experiments")
    _script([os.path.join(exp, "make_dummy_data.py"), "--out", "data", "--train", "32", "--val", "16", "--dist", "rand"], tmp_path)
    out = _script([os.path.join(exp, "train_baseline.py"), "--epochs", "1", "--batch-size", "16", "--ema-decay", "0.5"], tmp_path)
    assert "Epoch   1/1" in out and "Training complete!" in out
    ck = torch.load(tmp_path / "checkpoints" / "best_model.pt", weights_only=True)
    assert set(ck["optimizer_state_dict"]) == {"state", "param_groups", "ema"}
    names = [k for k in ck["model_state_dict"] if ".running_" not in k and "num_batches" not in k]
    assert len(ck["optimizer_state_dict"]["ema"]) == len(names)
    for k, e in zip(names, ck["optimizer_state_dict"]["ema"]):             # the saved weights are the average
        assert torch.equal(ck["model_state_dict"][k], e), k
