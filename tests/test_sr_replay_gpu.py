"""GPU: every launch of one SuperResolutionNet training step replayed in float64 on the HIP run's OWN stored operands
(tests/_sr_replay.py; the helper is proved on the CPU by tests/test_sr_replay_cpu.py).

The step runs eagerly with net.retain_backward_state (the `Saved` state stays on out.grad_fn) under _engine.DEBUG_CAPTURE (the
upstream gradient of every backward launch).  In the bf16 mode the stored operands are exactly representable and the masks are
the stored ones, so nothing flips and nothing chains: what is left per launch is fp32-vs-float64 accumulation and the rounding
of the stored result.  Bounds (tests/_sr_replay.py, none taken from a measured HIP value), max-normalised:
  bf16-stored result of one launch 5e-3; spanning n stored / inner bf16 roundings n * 5e-3 (n beside each such emit in the
  helper); fp32-stored forward 2e-5, gradient 2e-4; bits / amax / passmask equal to the mask of the stored activation.
Every parameter of net.named_parameters() is claimed by exactly one replayed launch - the motion_estimator.* gradients too.
Measured worst errors per launch class: profiles/sr_replay.txt."""
import pytest
import torch
import torch.nn.functional as F

import _sr_replay as R
from oracle import synth

pytestmark = pytest.mark.gpu
FLOW_GAIN = 20.0      # flows of 2.5 - 2.9 px instead of 0.13 px at these geometries (measured on the CPU float64 oracle)

#        in, s, F, NB, win, B,  H,  W
G1 = (3, 2, 64, 3, 1, 2, 45, 70)      # the benchmark's kernels: rdb_tail, planar, bf16 features, fused tail; first / middle / last block
G2 = (3, 4, 64, 1, 2, 1, 33, 52)      # T = 5 (Tp = 8, groups = 4 in the centre correlation gradient), s = 4
G3 = (3, 3, 32, 1, 1, 2, 24, 40)      # 32-channel variants, unfused lff, s = 3

CASES = [("G1-bf16", G1, True, {}), ("G2-bf16", G2, True, {}), ("G3-bf16", G3, True, {}),
         ("G1-bf16-interleaved-fp32feat", G1, True, {"NVQ_PLANAR": "0", "NVQ_BF16_FEATURES": "0"}),
         ("G1-fp32", G1, False, {}), ("G3-fp32", G3, False, {})]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


def _step(geom, bf16):
    """one eager training step -> (net, Saved, captures, out, dout)"""
    from nerve_cl import _engine, _nvq
    from nerve_cl.models import SuperResolutionNet
    cin, s, Fc, NB, win, B, H, W = geom
    T = 2 * win + 1
    sd = synth.formula_state(cin, s, Fc, NB, win, gain=synth.GOLDEN_GAIN)
    for n in ("weight", "bias"):
        sd[f"motion_estimator.flow_net.6.{n}"] = sd[f"motion_estimator.flow_net.6.{n}"] * FLOW_GAIN
    net = SuperResolutionNet(cin, s, Fc, NB, win)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    net.use_hip_graphs = False
    net.retain_backward_state = True
    x = synth.formula_clip(B, T, H, W).cuda()
    tgt = synth.formula_target(B, H * s, W * s).cuda()
    cap, seen = {}, {}
    _engine.DEBUG_CAPTURE = cap
    try:
        out = net(x)
        out.register_hook(lambda gr: seen.__setitem__("dout", gr.detach().clone()))
        F.mse_loss(out, tgt).backward()
        torch.cuda.synchronize()
    finally:
        _engine.DEBUG_CAPTURE = None
    return net, out.grad_fn.sv, cap, out, seen["dout"]


@pytest.mark.parametrize("name,geom,bf16,env", CASES, ids=[c[0] for c in CASES])
def test_every_launch_on_its_own_operands(monkeypatch, name, geom, bf16, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net, sv, cap, out, dout = _step(geom, bf16)
    S = R.read_state(net, sv, cap, out, dout)
    P = R.params64(net)
    q = R.bf16_round if bf16 else R.ident
    ck = R.Checker(S, bf16)
    R.walk_forward(S, P, q, ck)
    R.walk_backward(S, P, q, ck)
    flow = S["flow.4"].abs().max().item()
    print(f"\n  {name}: {len(ck.rows)} stored tensors of {len({r[0] for r in ck.rows})} launches, flow up to {flow:.2f} px")
    print(ck.report())
    for (cls, kind), worst in sorted(ck.worst_by_class().items()):
        print(f"  CLASS {name:30s} {cls:22s} bound {kind:6s} worst {worst:.2e}")
    assert flow > 1.0, "the scaled flow layer should move the warp away from the identity"
    names = sorted(n for n, _ in net.named_parameters())
    assert sorted(ck.claimed) == names, "every parameter gradient must be claimed by exactly one replayed launch"
    bad = ck.failures()
    assert not bad, "\n".join(f"launch {launch}, tensor {key}: rel {rel:.2e} (l2 {l2:.2e}) > {b:.1e}" for launch, key, rel, l2, b, _ in bad)
