"""CPU: the per-op replay helper of FrameRecoveryNet (tests/_fr_replay.py) proved before the GPU tests trust it.

(1) Mirror: the replay functions chained in the network's op order into a whole float64 training step give
    oracle/fr_oracle.py's output, every parameter gradient, the three input gradients and the BatchNorm running-statistics
    updates back to 1e-10, in both temporal layouts, in train and eval, at every geometry of tests/test_fr_replay_gpu.py.
(2) Exclusion cap: on the mirror's own float64 values no tensor has more than NEAR_CAP of its elements left out.
(3) Detection: the taped mirror step is the clean state; one stored tensor of one op is perturbed by twice its bound in one
    element (plus one pooled-selection element and one padding-channel element) and the Checker must flag exactly that op
    and tensor.
(4) The tape on a toy Function: node-level gradients, forward-only entries with grad mode off, `apply` restored."""
import types

import pytest
import torch
import torch.nn.functional as F

import _fr_replay as R
from oracle import fr_oracle, synth

B16, F32 = torch.bfloat16, torch.float32


def inputs(B, T, H, W, seed=5):
    clip = synth.formula_clip(B, T + 1, H, W, seed=seed)
    mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed))
    return clip[:, 0].contiguous(), clip[:, 1:].contiguous(), mask, synth.formula_target(B, H, W, seed=seed + 1)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def oracle_step(sd, frame, refs, mask, tgt, train):
    P = {k: (v.detach().double().clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone())
         for k, v in sd.items()}
    before = {k: v.clone() for k, v in P.items() if "running" in k}
    xs = [t.double().clone().requires_grad_() for t in (frame, refs, mask)]
    out = fr_oracle.frame_recovery_forward(P, *xs, train, prec=None)
    F.mse_loss(out, tgt.double()).backward()
    return out.detach(), {k: v.grad for k, v in P.items() if v.grad is not None}, {k: P[k].detach() - v for k, v in before.items()}, \
        [x.grad for x in xs]


_STEPS = {}


def step(case):
    """the taped mirror step of a case, computed once per geometry / layout / mode"""
    name, base, T, B, H, W, bf16_math, acts, tic, train, frozen = case
    key = (base, T, B, H, W, acts, tic, train)
    if key not in _STEPS:
        sd = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN)
        data = inputs(B, T, H, W)
        _STEPS[key] = (sd, data, R.mirror_step(sd, *data, train, tic, B16 if acts else F32))
    return _STEPS[key]


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_chained_mirror_is_the_oracle_and_stays_within_the_exclusion_cap(case):
    sd, (frame, refs, mask, tgt), m = step(case)
    train = case[9]
    out, grads, bn, dx = oracle_step(sd, frame, refs, mask, tgt, train)
    errs = {"out": rel(m["out"], out)}
    assert sorted(m["grads"]) == sorted(grads)
    errs.update({"grad:" + n: rel(m["grads"][n], g) for n, g in grads.items()})
    errs.update({n: rel(getattr(m["sink"], n), g) for n, g in zip(R.SINK_NAMES, dx)})
    if train:
        errs.update({"bn:" + k: rel(m["bn"][k], v) for k, v in bn.items() if "running" in k and v.is_floating_point()})
    worst = max(errs, key=errs.get)
    print(f"\n  {case[0]}: {len(m['entries'])} op calls, worst {worst} {errs[worst]:.1e}")
    assert errs[worst] < R.TOL_F64, {k: v for k, v in errs.items() if v >= R.TOL_F64}
    # the clean state checks clean against itself, every parameter is claimed once, the inputs are accounted for, and the
    # conditions that leave elements out stay under the cap on the reference's own values
    ck = R.Checker(False, m["names"]).check(m["entries"])
    assert not ck.unknown and not ck.failures(), ck.failures()[:5]
    assert sorted(ck.claimed) == sorted(m["names"].values())
    assert not ck.input_accounting({n: getattr(m["sink"], n) for n in R.SINK_NAMES})
    assert ck.shares and max(ck.shares.values()) <= R.NEAR_CAP, max(ck.shares.items(), key=lambda kv: kv[1])
    print(f"  largest share left out: {max(ck.shares.values()):.2e}")


# ----------------------------------------------------------------------------- seeded defects
SMALL = ("F", 16, 1, 3, 33, 47, True, True, True, True, False)          # time-major ops
SMALL_TC = ("H-tc", 16, 2, 2, 33, 47, False, True, True, True, False)      # time-in-channels ops, bf16 paddings
OPS_TM = ["Cast", "Conv", "DwConv", "TemporalConv", "GroupMean", "ConvT", "Stem7", "BatchNorm", "MaxPool", "Subsample2", "Resize",
          "Cat2", "CBAMFn", "FusionMix", "Tanh", "MaskBlend"]
OPS_TC = ["SpatialConvTC", "TemporalConvTC", "GroupMeanTC"]


def _flagged(entries, names):
    ck = R.Checker(False, names).check(entries)
    return sorted({(launch, key.split(" ")[0]) for launch, key, *_ in ck.failures()})


def _bump(t, index, factor=2.0):
    """one element moved by factor x the float64 bound of its tensor"""
    t.view(-1)[index] += factor * R.TOL_F64 * t.abs().max().item()


@pytest.mark.parametrize("op", OPS_TM + OPS_TC)
@pytest.mark.parametrize("which", ["out", "grad"])
def test_a_seeded_defect_is_flagged_at_its_op_and_nowhere_else(op, which):
    sd, data, m = step(SMALL_TC if op in OPS_TC else SMALL)
    entries = [dict(e) for e in m["entries"]]
    # the last call of the class that ran backward (its operands are other ops' stored tensors, which must stay clean)
    e = [x for x in entries if x["op"] == op and "grad_inputs" in x][-1]
    launch = f"{op}[{e['idx']}]"
    if which == "out":
        # the stored output is the next op's operand: the defect is in a copy only this op's entry holds
        e["out"] = R.tag(e["out"].detach().clone(), R.layout_kind(e["out"]))
        _bump(e["out"], 0)
        want = [(launch, "out")]
    else:
        j = next(i for i, g in enumerate(e["grad_inputs"]) if g is not None)
        e["grad_inputs"] = [None if g is None else g.clone() for g in e["grad_inputs"]]
        _bump(e["grad_inputs"][j], 0)
        got = _flagged(entries, m["names"])
        assert len(got) == 1 and got[0][0] == launch and (got[0][1].startswith("grad:") or got[0][1].startswith("d.arg")), got
        return
    assert _flagged(entries, m["names"]) == want


def test_a_flipped_pool_selection_and_a_nonzero_padding_channel_are_flagged():
    sd, data, m = step(SMALL_TC)
    for kind in ("idx", "pad", "sink", "stat"):
        entries = [dict(e) for e in m["entries"]]
        if kind == "idx":
            e = [x for x in entries if x["op"] == "MaxPool" and "saved" in x][-1]
            idx = e["saved"][0].clone()
            idx.view(-1)[5] = (idx.view(-1)[5] + 1) % 4
            e["saved"] = (R.tag(idx, R.layout_kind(e["saved"][0])),)
            want = [(f"MaxPool[{e['idx']}]", "idx")]
        elif kind == "pad":
            # the 2-channel attention logits are stored in 4 channels: one padding element set
            e = [x for x in entries if x["op"] == "Conv" and x["args"][1].shape[0] == 2][-1]
            out = e["out"].detach().clone()
            assert out.shape[-1] == 4
            out[0, 0, 0, 3] = 1e-9
            e["out"] = R.tag(out, "fp32")
            want = [(f"Conv[{e['idx']}]", "pad:out")]
        elif kind == "sink":
            e = [x for x in entries if x["op"] == "Stem7"][-1]
            after = {k: v.clone() for k, v in e["sink_after"].items()}
            _bump(after["dmask"], 7)
            e["sink_after"] = after
            want = [(f"Stem7[{e['idx']}]", "sink.dmask")]
        else:
            e = [x for x in entries if x["op"] == "BatchNorm" and "saved" in x][3]
            b = tuple(t.clone() for t in e["buf_after"])
            _bump(b[1], 2)
            e["buf_after"] = b
            want = [(f"BatchNorm[{e['idx']}]", "running_var")]
        assert _flagged(entries, m["names"]) == want, kind


def test_an_unknown_op_class_and_a_missing_parameter_are_reported():
    sd, data, m = step(SMALL)
    entries = [dict(e) for e in m["entries"]]
    entries[3]["op"] = "BrandNewOp"
    ck = R.Checker(False, m["names"]).check(entries)
    assert ck.unknown == ["BrandNewOp"]
    assert sorted(ck.claimed) != sorted(m["names"].values())


def test_too_many_elements_left_out_is_a_failure_not_a_skip():
    sd, data, m = step(SMALL)
    entries = [dict(e) for e in m["entries"]]
    e = [x for x in entries if x["op"] == "BatchNorm" and x["args"][7] and x["args"][3] is not None and "grad_inputs" in x][-1]
    # a residual that cancels bn(x): pre is zero up to float64 rounding everywhere, every element is undecided
    a = list(e["args"])
    C = a[1].numel()
    xv, sh = R.dec(a[0], R.lay_of(a[0], C)), (1, -1, 1, 1)
    pre = (xv - e["saved"][4].view(sh)) * (e["saved"][5] * a[1].detach()).view(sh) + a[2].detach().view(sh)
    a[3] = R.enc(-pre, R.lay_of(a[3], C))
    e["args"] = tuple(a)
    ck = R.Checker(False, {}).check([e])
    assert any("left out" in key for _, key, *_ in ck.failures())


def test_operand_rounding_does_not_round_the_gradients():
    """MATH_BF16: the replayed kernel reads rounded operands; the gradients it writes are those of the rounded operands, not
    rounded again on the way back through the rounding"""
    torch.manual_seed(3)
    x, w, g = torch.randn(1, 8, 5, 6, dtype=torch.float64), torch.randn(4, 8, 3, 3, dtype=torch.float64), torch.randn(1, 4, 5, 6).double()
    xn = torch.zeros(1, 5, 6, 8, dtype=torch.float64)
    xn[:] = x.permute(0, 2, 3, 1)
    plan = R.PLANS["Conv"]((R.tag(xn, "fp32"), w, None, False, R.MATH_BF16))
    leaves = [x.clone().requires_grad_(), w.clone().requires_grad_()]
    dx, dw = torch.autograd.grad(plan.f(leaves, R.bf16_round, None), leaves, g)
    xq, wq, gq = (R.bf16_round(t).requires_grad_() for t in (x, w, g))
    dx0, dw0 = torch.autograd.grad(F.conv2d(xq, wq, None, padding=1), (xq, wq), gq.detach())
    assert rel(dx, dx0) < 1e-12 and rel(dw, dw0) < 1e-12


# ----------------------------------------------------------------------------- the tape
class Twice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        ctx.save_for_backward(x)
        ctx.k = k
        return x * k

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if ctx.k == 3:
            Twice.apply(g, 1)                    # a call with grad mode off: recorded as a forward-only entry
        return g * ctx.k, None


def test_tape_records_node_level_gradients_and_restores_apply():
    ns = types.SimpleNamespace(Twice=Twice, other=3)
    before = Twice.apply
    x = torch.arange(4.0, dtype=torch.float64).requires_grad_()
    with R.Tape(ns) as tp:
        assert list(tp.classes) == ["Twice"]
        y = ns.Twice.apply(x, 2)
        a, b = ns.Twice.apply(y, 3), ns.Twice.apply(y, 5)             # y is consumed twice
        (a.sum() + 2 * b.sum()).backward()
    assert "apply" not in Twice.__dict__ and Twice.apply == before
    e = tp.entries
    assert [(t["op"], t["args"][1]) for t in e] == [("Twice", 2), ("Twice", 3), ("Twice", 5), ("Twice", 1)]
    # node-level: each consumer's own gradient, not the sum that reaches y
    assert torch.equal(e[1]["grad_inputs"][0], torch.full((4,), 3.0, dtype=torch.float64))
    assert torch.equal(e[2]["grad_inputs"][0], torch.full((4,), 10.0, dtype=torch.float64))
    assert torch.equal(e[0]["grad_outputs"][0], torch.full((4,), 13.0, dtype=torch.float64))
    assert torch.equal(e[0]["saved"][0], x) and e[0]["needs"] == (True, False)
    assert "grad_inputs" not in e[3] and "saved" not in e[3] and not e[3]["grad_mode"]
    assert torch.equal(x.grad, torch.full((4,), 26.0, dtype=torch.float64))
