"""GPU: whole training steps on poisoned memory (tests/_poison.py; the helper is proved by tests/test_poison_cpu.py).

The invariant: no result depends on memory that the contract says nobody reads.  Production never runs on clean memory - the
engine's activations are `torch.empty`, the dense-block buffers have 32 never-written channels per pixel (CATLD = 256 for
CAT = 224), the workspaces always hold another layer's partial sums - and a stale finite value passes every value check.

Each case runs one eager training step (forward, loss, backward; graphs off) on a freshly built network
  * clean (twice: two clean runs must be bit-identical, the precondition of everything below, and finite), and
  * under `poisoned_allocations`, with `_engine.workspace` and the eight `workspace_slots` filled with NaN immediately before
    the step,
and then a SECOND step (another clip) on the same network objects, so that whatever a network caches is reused.  The output,
the loss, every parameter gradient, every input gradient and every BatchNorm running buffer of the poisoned run must have the
bits of the clean run.  Exact equality is a derivation, not a measurement: the compared paths have no float atomics (in csrc/
only motion.hip and drift.hip contain atomics or memsets; SuperResolutionNet therefore runs with deterministic = True, whose
warp gradient is the atomic-free one - the default warp gradient adds its far sources with float atomics and is not
bit-repeatable, it has a case of its own at the bound of the neighbouring kernel test), and poison sits only where nothing
may read.  Integer and index buffers are never poisoned (tests/_poison.py says why).

Geometries: the two smallest of each replay table - G3 and G2 of tests/test_sr_replay_gpu.py (24 x 40 and the odd 33 x 52),
and the 33 x 47 (base 16) and 40 x 72 (base 32) frames of tests/_fr_replay.py's cases F / H and E."""
import time

import pytest
import torch
import torch.nn.functional as F

import _poison as P
from _fr_replay import CASES as FR_TABLE
from oracle import synth
from test_fr_replay_gpu import frozen_in_case_I
from test_sr_replay_gpu import FLOW_GAIN, G2, G3

pytestmark = pytest.mark.gpu

# the bounds of tests/test_kernels_gpu.py::test_warp_forward_backward (max-normalised): the warp gradient at the features
# 5e-5, at the flow 2e-4.  Everything behind the non-deterministic warp gradient is compared at the wider of the two.
WARP_DFEAT_TOL, WARP_DFLOW_TOL = 5e-5, 2e-4

_FR = {c[0]: c for c in FR_TABLE}
FR_H = _FR["H"][1:6]          # base 16, T 2, B 2, 33 x 47
FR_E = _FR["E"][1:6]          # base 32, T 3, B 1, 40 x 72
assert FR_H == (16, 2, 2, 33, 47) and FR_E == (32, 3, 1, 40, 72) and _FR["F"][4:6] == (33, 47)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    t0 = time.perf_counter()
    yield
    print(f"\nPOISON-FILE tests/test_poison_networks_gpu.py wall {time.perf_counter() - t0:.1f} s")


# ----------------------------------------------------------------------------- the cached workspaces
def _cached_workspaces():
    from nerve_cl import _engine
    dev = torch.device("cuda", torch.cuda.current_device())
    _engine.workspace(dev)
    _engine.workspace_slots(dev, _engine._ReduceQueue.SLOTS)
    return list(_engine._ws_cache.values()) + [w for slots in _engine._ws_multi_cache.values() for w in slots]


def _fill_workspaces(poison: bool) -> int:
    """NaN (poisoned run) or zeros (clean run: whatever an earlier test left there is not part of a clean run) -> bytes"""
    n = 0
    for ws in _cached_workspaces():
        if poison:
            P.poison_(ws)
        else:
            ws.zero_()
        n += ws.numel() * ws.element_size()
    return n


# ----------------------------------------------------------------------------- the three networks
def _sr(geom, bf16, deterministic=True):
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    cin, s, Fc, NB, win, B, H, W = geom
    sd = synth.formula_state(cin, s, Fc, NB, win, gain=synth.GOLDEN_GAIN)
    for n in ("weight", "bias"):      # flows of a few pixels, as tests/test_sr_replay_gpu.py
        sd[f"motion_estimator.flow_net.6.{n}"] = sd[f"motion_estimator.flow_net.6.{n}"] * FLOW_GAIN
    net = SuperResolutionNet(cin, s, Fc, NB, win)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    net.use_hip_graphs = False
    net.deterministic = deterministic

    def batch(step):
        return ([synth.formula_clip(B, 2 * win + 1, H, W, seed=11 + step)], synth.formula_target(B, H * s, W * s, seed=23 + step))
    return net, batch


def _light(s, B, H, W):
    from nerve_cl import _nvq
    from nerve_cl.models import LightweightSuperResolution
    net = LightweightSuperResolution(s)
    net.load_state_dict(synth.formula_state_light(s, gain=synth.GOLDEN_GAIN), strict=True)
    net = net.cuda()
    net.math_mode, net.bf16_activations = _nvq.MATH_BF16, True

    def batch(step):
        return ([synth.formula_clip(B, 1, H, W, seed=11 + step)[:, 0].contiguous()], synth.formula_target(B, H * s, W * s, seed=23 + step))
    return net, batch


def _fr(geom, bf16_math, acts, tic, frozen=False):
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet
    base, T, B, H, W = geom
    net = FrameRecoveryNet(3, base, T)
    net.load_state_dict(synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN), strict=True)
    net = net.cuda()
    net.time_in_channels = tic
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16 if bf16_math else _nvq.MATH_F32), acts
    if frozen:
        for n, p in net.named_parameters():
            p.requires_grad_(not frozen_in_case_I(n))

    def batch(step):        # a clip and a soft mask in (0.05, 0.95), as tests/test_fr_replay_gpu.py
        clip = synth.formula_clip(B, T + 1, H, W, seed=5 + step)
        mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(5 + step))
        return ([clip[:, 0].contiguous(), clip[:, 1:].contiguous(), mask], synth.formula_target(B, H, W, seed=6 + step))
    return net, batch


# ----------------------------------------------------------------------------- one run = two steps on one network object
def _run(build, monkeypatch, poison: bool, train=True, steps=2):
    """-> ([{name: tensor} per step], poisoned bytes).  The network and its inputs are made on clean memory; only the steps
    themselves run under the wrapper."""
    net, batch = build()
    net.train(train)
    results, nbytes = [], 0
    for step in range(steps):
        xs, tgt = batch(step)
        xs = [x.cuda().requires_grad_(train) for x in xs]
        tgt = tgt.cuda()
        for p in net.parameters():
            p.grad = None
        with monkeypatch.context() as m:
            log = P.poisoned_allocations(m) if poison else None
            ws_bytes = _fill_workspaces(poison)
            if train:
                out = net(*xs)
                loss = F.mse_loss(out, tgt)
                loss.backward()
            else:
                with torch.no_grad():
                    out = net(*xs)
                loss = F.mse_loss(out, tgt)
            torch.cuda.synchronize()
            nbytes += (ws_bytes + log.bytes) if poison else 0
        r = {"out": out.detach().clone(), "loss": loss.detach().clone()}
        for n, p in net.named_parameters():
            if train and p.requires_grad:
                assert p.grad is not None, f"{n} has no gradient"
                r["grad:" + n] = p.grad.detach().clone()
            else:
                assert p.grad is None, f"{n} is not trained and has a gradient"
        for i, x in enumerate(xs):
            if train:
                assert x.grad is not None, f"input {i} has no gradient"
                r[f"dinput:{i}"] = x.grad.detach().clone()
        for n, b in net.named_buffers():
            r["buffer:" + n] = b.detach().clone()
        results.append(r)
    return results, nbytes


def _assert_finite(results, what):
    for step, r in enumerate(results):
        for k, v in r.items():
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), f"{what}, step {step}: {k} is not finite on clean memory"


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb)
        for k in ra:
            P.assert_same_bits(ra[k], rb[k], f"{what}, step {step}, {k}")


def _clean_pair(build, monkeypatch, name, **kw):
    clean, _ = _run(build, monkeypatch, False, **kw)
    again, _ = _run(build, monkeypatch, False, **kw)
    _assert_finite(clean, name)
    _assert_same(clean, again, f"{name}: two CLEAN runs differ (the precondition of the poisoned comparison)")
    return clean


TRAIN_CASES = [
    # SuperResolutionNet, deterministic mode
    ("sr-G3-fp32", lambda: _sr(G3, False), {}),
    ("sr-G2-fp32", lambda: _sr(G2, False), {}),                       # F = 64: fp32 CatBuf with CATLD 256 for CAT 224
    ("sr-G3-bf16", lambda: _sr(G3, True), {}),                        # slice-planar CatBuf
    ("sr-G2-bf16", lambda: _sr(G2, True), {}),
    ("sr-G2-bf16-interleaved", lambda: _sr(G2, True), {"NVQ_PLANAR": "0"}),   # bf16 CatBuf with the 32 padding channels
    # LightweightSuperResolution, the bf16 mode
    ("light-s2-24x40", lambda: _light(2, 2, 24, 40), {}),
    ("light-s3-33x52", lambda: _light(3, 1, 33, 52), {}),
    # FrameRecoveryNet
    ("fr-H-fp32-time-major", lambda: _fr(FR_H, False, False, False), {}),
    ("fr-H-fp32-time-in-channels", lambda: _fr(FR_H, False, False, True), {}),
    ("fr-H-bf16-time-in-channels", lambda: _fr(FR_H, True, True, True), {}),
    ("fr-H-bf16-time-major", lambda: _fr(FR_H, True, True, False), {}),
    ("fr-E-bf16-time-in-channels", lambda: _fr(FR_E, True, True, True), {}),
    ("fr-E-bf16math-fp32acts-time-major", lambda: _fr(FR_E, True, False, False), {}),
    ("fr-E-bf16-frozen-encoders", lambda: _fr(FR_E, True, True, True, frozen=True), {}),
]


@pytest.mark.parametrize("name,build,env", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_training_steps_do_not_depend_on_unwritten_memory(monkeypatch, name, build, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    clean = _clean_pair(build, monkeypatch, name)
    poisoned, nbytes = _run(build, monkeypatch, True)
    assert nbytes > 0
    print(f"\nPOISON network {name:36s} form eager-train-2-steps bytes {nbytes} compared {sum(len(r) for r in clean)}", end=" ")
    _assert_same(clean, poisoned, f"{name}: clean against poisoned")
    print("pass")


def test_a_seeded_missing_write_is_flagged(monkeypatch):
    """live on the GPU: the first BatchNorm statistics launch of the step is dropped, so the layer normalises with a `mean` /
    `invstd` that nobody wrote - the 'partial result that is read but not written' class.  On recycled clean memory that is some
    finite leftover and no value check need notice; here the comparison (or already its precondition) must fail."""
    from nerve_cl import _nvq
    real = _nvq.bn_stats
    dropped = []

    def bn_stats(*args, **kwargs):
        if not dropped or dropped[-1] != "armed":
            return real(*args, **kwargs)
        dropped[-1] = "dropped"

    monkeypatch.setattr(_nvq, "bn_stats", bn_stats)

    def build():
        net, batch = _sr(G3, False)
        dropped.append("armed")
        return net, batch

    with pytest.raises(AssertionError):
        clean = _clean_pair(build, monkeypatch, "seeded")
        poisoned, _ = _run(build, monkeypatch, True)
        _assert_same(clean, poisoned, "seeded: clean against poisoned")
    assert dropped.count("dropped") >= 1, "the seeded defect never ran: the exact-fp32 G3 step no longer calls nvq_bn_stats"
    print(f"\nPOISON network {'seeded: first nvq_bn_stats launch dropped':36s} form eager-train-2-steps bytes - flagged")


EVAL_CASES = [
    ("sr-G3-bf16-eval", lambda: _sr(G3, True)),
    ("sr-G2-fp32-eval", lambda: _sr(G2, False)),
    ("light-s2-24x40-eval", lambda: _light(2, 2, 24, 40)),
    ("fr-H-bf16-eval", lambda: _fr(FR_H, True, True, True)),
    ("fr-E-fp32-eval", lambda: _fr(FR_E, False, False, False)),
]


@pytest.mark.parametrize("name,build", EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_eval_forward_does_not_depend_on_unwritten_memory(monkeypatch, name, build):
    clean = _clean_pair(build, monkeypatch, name, train=False)
    poisoned, nbytes = _run(build, monkeypatch, True, train=False)
    assert nbytes > 0
    print(f"\nPOISON network {name:36s} form eval-no_grad-2-forwards bytes {nbytes} compared {sum(len(r) for r in clean)}", end=" ")
    _assert_same(clean, poisoned, f"{name}: clean against poisoned")
    # eval leaves the running statistics alone
    net, _ = build()
    for n, b in net.named_buffers():
        P.assert_same_bits(poisoned[-1]["buffer:" + n], b, f"{name}: buffer {n} moved in eval")
    print("pass")


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_default_warp_gradient_on_poisoned_memory_within_the_kernel_tests_bound(monkeypatch):
    """deterministic = False: the warp gradient's far sources are float atomics, so two runs are not bit-repeatable.  Run in the
    exact-fp32 mode, where the only difference between two runs is that summation order.  The forward (no atomics) stays
    bit-identical.  EVERY gradient - parameter and input gradients, on the feature side and on the flow side alike - is compared
    at the WIDER of the two bounds that tests/test_kernels_gpu.py::test_warp_forward_backward sets for the warp gradient (2e-4 of
    the tensor's largest magnitude, its bound at the flow; 5e-5 is its bound at the features).  Nothing here asserts how the
    launches behind the warp gradient carry its fp32 rounding on; one imported bound is applied to all of them."""
    build = lambda: _sr(G3, False, deterministic=False)   # noqa: E731
    clean, _ = _run(build, monkeypatch, False)
    _assert_finite(clean, "sr-G3-fp32-atomic-warp")
    poisoned, nbytes = _run(build, monkeypatch, True)
    worst = 0.0
    for step, (rc, rp) in enumerate(zip(clean, poisoned)):
        for k in rc:
            if k.startswith(("grad:", "dinput:")):
                e = _rel(rp[k], rc[k])
                worst = max(worst, e)
                assert e <= max(WARP_DFEAT_TOL, WARP_DFLOW_TOL), f"step {step}, {k}: {e:.2e}"
            else:
                P.assert_same_bits(rc[k], rp[k], f"step {step}, {k}")
    print(f"\nPOISON network {'sr-G3-fp32-atomic-warp':36s} form eager-train-2-steps bytes {nbytes} worst-rel {worst:.2e} pass")
