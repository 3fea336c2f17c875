"""GPU: every op call of one FrameRecoveryNet training step replayed in float64 on the HIP run's OWN stored operands
(tests/_fr_replay.py; the helper is proved on the CPU by tests/test_fr_replay_cpu.py).

The step runs eagerly under `_fr_replay.Tape`, which records every `nerve_cl._ops` Function call with its arguments, output,
saved tensors, node-level gradients and the input-gradient sink around the ops that write to it.  Nothing chains: each op is
recomputed from what the kernel read, at the strides, channel paddings, storage types and T / B groupings the network hands
it, so what is left per op is fp32-vs-float64 accumulation and the roundings of that op.  Bounds (tests/_sr_replay.py, none taken
from a measured HIP value), max-normalised: a bf16-stored result 5e-3, n inner bf16 roundings (beside the plan that has any)
n * 5e-3 more, an fp32-stored forward result 2e-5, an fp32-stored gradient 2e-4; pooling selections, copies and padding channels
exact.  Every trained parameter of net.named_parameters() is claimed by exactly one taped op's gradient, which is also the
gradient the network delivers; the three input gradients are what the sink-writing ops left.  A taped op class without a replay
function fails the test.  Measured worst errors per op class: profiles/fr_replay.txt."""
import pytest
import torch
import torch.nn.functional as F

import _fr_replay as R
from oracle import synth

pytestmark = pytest.mark.gpu
B16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    assert (_nvq.MATH_F32, _nvq.MATH_BF16) == (R.MATH_F32, R.MATH_BF16)


def inputs(B, T, H, W, seed=5):
    """a clip and a soft mask in (0.05, 0.95), as tests/test_fr_bf16_emulated_gpu.py"""
    clip = synth.formula_clip(B, T + 1, H, W, seed=seed)
    mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed))
    return clip[:, 0].contiguous(), clip[:, 1:].contiguous(), mask, synth.formula_target(B, H, W, seed=seed + 1)


def frozen_in_case_I(name):
    return name.startswith(("spatial_encoder.", "temporal_encoder.", "fusion.refine.0.conv1.bn."))


def _step(case):
    from nerve_cl import _nvq, _ops
    from nerve_cl.models import FrameRecoveryNet
    name, base, T, B, H, W, bf16_math, acts, tic, train, frozen = case
    net = FrameRecoveryNet(3, base, T)
    net.load_state_dict(synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN), strict=True)
    net = net.cuda().train(train)
    net.time_in_channels = tic
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16 if bf16_math else _nvq.MATH_F32), acts
    if frozen:
        for n, p in net.named_parameters():
            p.requires_grad_(not frozen_in_case_I(n))
    frame, refs, mask, tgt = inputs(B, T, H, W)
    xs = [t.cuda().requires_grad_() for t in (frame, refs, mask)]
    with R.Tape(_ops) as tape:
        out = net(*xs)
        F.mse_loss(out, tgt.cuda()).backward()
        torch.cuda.synchronize()
    assert "apply" not in _ops.Conv.__dict__
    return net, xs, tape


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_every_op_call_on_its_own_operands(case):
    name, bf16_math = case[0], case[6]
    net, xs, tape = _step(case)
    trained = {p.data_ptr(): n for n, p in net.named_parameters() if p.requires_grad}
    ck = R.Checker(bf16_math, trained).check(tape.entries)
    ops = sorted({e["op"] for e in tape.entries})
    nbwd = sum("grad_inputs" in e for e in tape.entries)
    print(f"\n  {name}: {len(tape.entries)} op calls ({nbwd} with a backward), {len(ck.rows)} stored tensors; classes: {' '.join(ops)}")
    print(ck.report())
    for (cls, kind), worst in sorted(ck.worst_by_class().items()):
        print(f"  CLASS {name:3s} {cls:16s} bound {kind:7s} worst {worst:.2e}")
    if ck.shares:
        print(f"  largest share left out: {max(ck.shares.values()):.2e}")
    assert not ck.unknown, f"taped op classes without a replay function: {sorted(set(ck.unknown))}"
    assert sorted(ck.claimed) == sorted(trained.values()), "every trained parameter must be claimed by exactly one taped op's gradient"
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, ck.grads[n].view_as(p.grad)), f"{n}: the delivered gradient is not the op's"
        else:
            assert p.grad is None, f"{n} is frozen and has a gradient"
    if case[10]:
        # the BatchNorm whose affine is frozen behind a trained conv: no dgamma / dbeta launch (nvq_bn2_backward_ex), its dx compared
        ptr = dict(net.named_parameters())["fusion.refine.0.conv1.bn.weight"].data_ptr()
        e, = [x for x in tape.entries if x["op"] == "BatchNorm" and x["args"][1].data_ptr() == ptr]
        assert e["needs"][:3] == (True, False, False) and e["grad_inputs"][1] is None and e["grad_inputs"][2] is None
        assert any(launch == f"BatchNorm[{e['idx']}]" and key == "d.arg0" for launch, key, *_ in ck.rows)
    missing = ck.input_accounting(dict(zip(R.SINK_NAMES, (x.grad for x in xs))))
    assert not missing, missing
    assert all(x.grad is not None for x in xs)
    bad = ck.failures()
    assert not bad, "\n".join(f"op {launch}, tensor {key}: rel {rel:.2e} (l2 {l2:.2e}) > {b:.1e}" for launch, key, rel, l2, b, _ in bad)
    # and the check is live on the HIP run's own tensors: one element of the last conv's stored output and of its weight gradient
    # moved by twice the fp32 bounds is seen, there and nowhere else
    e = dict([x for x in tape.entries if x["op"] == "Conv" and "grad_inputs" in x][-1])
    e["out"], e["grad_inputs"] = e["out"].clone(), [None if g is None else g.clone() for g in e["grad_inputs"]]
    e["out"].view(-1)[0] += 2 * R.TOL_F32_FWD * e["out"].abs().max()
    e["grad_inputs"][1].view(-1)[3] += 2 * R.TOL_F32_GRAD * e["grad_inputs"][1].abs().max()
    seen = sorted(key for _, key, *_ in R.Checker(bf16_math, trained).check([e]).failures())
    assert seen == ["grad:decoder.final.0.weight", "out"], seen


# ----------------------------------------------------------------------------- the same machinery on single op calls
def T_(*shape):
    return torch.randn(*shape).bfloat16().float()


def _nhwc(x):
    """(N,C,H,W) -> fp32 [N,H,W,pad4(C)] on the device"""
    N, C, H, W = x.shape
    out = torch.zeros(N, H, W, (C + 3) // 4 * 4)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out.cuda()


def _op_calls():
    """the op calls of tests/test_ops_gpu.py::test_bf16_storage_variants_of_the_frame_recovery_ops: id -> (fn(ops, x, *params), x, C,
    params)"""
    from nerve_cl import _nvq
    MB = _nvq.MATH_BF16
    C = 64
    g, b = 1 + 0.2 * torch.randn(C), 0.1 * torch.randn(C)
    g230, b230 = 1 + 0.2 * torch.randn(230), 0.1 * torch.randn(230)
    stat = lambda c: (torch.zeros(c).cuda(), torch.ones(c).cuda())          # noqa: E731
    return {
        "bn_relu": (lambda o, x, g, b: o.BatchNorm.apply(x, g, b, None, *stat(C), True, True), T_(2, C, 9, 10), C, [g, b]),
        "bn_res_relu": (lambda o, x, g, b: o.BatchNorm.apply(x, g, b, x, *stat(C), True, True), T_(2, C, 9, 10), C, [g, b]),
        "bn_230": (lambda o, x, g, b: o.BatchNorm.apply(x, g, b, None, *stat(230), True, True), T_(2, 230, 6, 7), 230, [g230, b230]),
        "maxpool_3_2_1": (lambda o, x: o.MaxPool.apply(x, 3, 2, 1), F.relu(T_(2, C, 12, 14)), C, []),
        "maxpool_2_2_0": (lambda o, x: o.MaxPool.apply(x, 2, 2, 0), T_(2, C, 12, 14), C, []),
        "subsample2": (lambda o, x: o.Subsample2.apply(x), T_(2, C, 9, 12), C, []),
        "depth_to_space2": (lambda o, x: o.DepthToSpace2.apply(x), T_(2, C, 5, 6), C, []),
        "group_mean": (lambda o, x: o.GroupMean.apply(x, 2, C), T_(4, C, 5, 6), C, []),
        "dwconv": (lambda o, x, w: o.DwConv.apply(x, w), T_(2, C, 9, 10), C, [0.3 * torch.randn(C, 1, 3, 3)]),
        "conv3x3_64_230": (lambda o, x, w: o.Conv.apply(x, w, None, False, MB), T_(2, C, 9, 10), C, [torch.randn(230, C, 3, 3) / 24]),
        "conv1x1_230_128": (lambda o, x, w: o.Conv.apply(x, w, None, False, MB), T_(2, 230, 9, 10), 230, [torch.randn(128, 230, 1, 1) / 15]),
        "temporal_conv_T2_230": (lambda o, x, w: o.TemporalConv.apply(x, w, 2, MB), T_(4, 230, 5, 6), 230,
                                 [torch.randn(128, 230, 3, 1, 1) / 26]),
        "conv_transpose": (lambda o, x, w: o.ConvT.apply(x, w, MB), T_(2, C, 5, 6), C, [torch.randn(C, 32, 4, 4) / 16]),
        "temporal_conv_tc": (lambda o, x, w: o.TemporalConvTC.apply(x, w, 2, MB), T_(2, 2 * C, 5, 6), 2 * C,
                             [torch.randn(128, C, 3, 1, 1) / 14]),
        "spatial_conv_tc": (lambda o, x, w: o.SpatialConvTC.apply(x, w, 2, MB), T_(2, 2 * C, 5, 6), 2 * C, [torch.randn(128, C, 3, 3) / 24]),
        "group_mean_tc": (lambda o, x: o.GroupMeanTC.apply(x, 2, C), T_(2, 2 * C, 5, 6), 2 * C, []),
        "stem7": (None, T_(2, 4, 20, 24), 4, [torch.randn(16, 4, 7, 7) / 14]),
    }


OP_IDS = ["bn_relu", "bn_res_relu", "bn_230", "maxpool_3_2_1", "maxpool_2_2_0", "subsample2", "depth_to_space2", "group_mean", "dwconv",
          "conv3x3_64_230", "conv1x1_230_128", "temporal_conv_T2_230", "conv_transpose", "temporal_conv_tc", "spatial_conv_tc",
          "group_mean_tc", "stem7"]


@pytest.mark.parametrize("dt", [B16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("op", OP_IDS)
def test_single_op_calls_forward_dx_and_parameter_gradients(op, dt):
    """forward, dx and the weight / bias / gamma / beta gradients of each listed op call against float64, with bf16- and with
    fp32-stored activations (MATH_BF16 in the convolutions)"""
    from nerve_cl import _ops
    torch.manual_seed(12 + OP_IDS.index(op))
    calls = _op_calls()
    assert sorted(calls) == sorted(OP_IDS)
    fn, x, C, params = calls[op]
    ps = [p.cuda().requires_grad_(True) for p in params]
    names = {p.data_ptr(): f"param{i}" for i, p in enumerate(ps)}
    with R.Tape(_ops) as tape:
        if op == "stem7":
            y = _ops.Stem7.apply(_nhwc(x), ps[0], dt)
        else:
            leaf = _ops.Cast.apply(_nhwc(x), dt, C).detach().requires_grad_(True)
            y = fn(_ops, leaf, *ps)
        yf = _ops.Cast.apply(y, F32, y.shape[-1])
        yf.backward(torch.randn_like(yf).bfloat16().float())
        torch.cuda.synchronize()
    ck = R.Checker(True, names).check(tape.entries)
    print("\n" + ck.report())
    assert not ck.unknown, ck.unknown
    assert sorted(ck.claimed) == sorted(names.values())
    main = [e for e in tape.entries if e["op"] not in ("Cast",)]
    assert len(main) == 1 and "grad_inputs" in main[0]
    if op != "stem7":
        assert any(key == "d.arg0" and launch.startswith(main[0]["op"]) for launch, key, *_ in ck.rows), "dx was not compared"
    bad = ck.failures()
    assert not bad, "\n".join(f"op {launch}, tensor {key}: rel {rel:.2e} (l2 {l2:.2e}) > {b:.1e}" for launch, key, rel, l2, b, _ in bad)
