"""GPU: FrameRecoveryNet's bf16 mode (MATH_BF16, with and without bf16 activation storage) against the float64 oracle that
rounds the same operands and stored tensors to bf16 at the same points (oracle/fr_oracle.py, prec "bf16_operands" /
"bf16_storage").  Against that oracle the only differences left are fp32 against float64 accumulation and the bf16 rounding
boundaries those flip, so the network has to sit about as close to it as the fp32 mode sits to plain float64 - not the 0.5
relative L2 that separates the bf16 mode from plain float64 (tests/test_fr_input_grad_gpu.py BF16_BOUNDS).

Compared: the output, the loss, every parameter gradient (max-normalised error and relative L2 per tensor, and the relative L2
of the whole gradient), the three input gradients and, in training mode, the step's BatchNorm running-statistics updates.  Both
activation storage types and both temporal layouts at 128x160 in eval and in training mode, and the cfg4 geometry (270x480,
B=2, the bench's 25 % central mask) in the bench's default setting.  Eval mode is held to fixed bounds (measured values beside
them); training mode, chaotic in the rounding, to the distance of the same emulation evaluated in float32 (see FLOOR_FACTOR).
A failure names where the deviation starts: the first BatchNorm in forward order whose running-statistics update deviates, and
the first parameter group in backward order whose gradient does.

Conv forms reached (one kernel-traced training step, bf16 activations, time-in-channels): 128x160 and 270x480 launch the same
conv_bf16_kernel / wgrad_bf16_kernel instantiations, and neither reaches the 32x32x16 kernels (conv_m32 / wgrad_m32); the
8-row small-image tiles and the pixel-split count are launch arguments, chosen per shape inside those kernels.
"""
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import fr_oracle, synth

pytestmark = pytest.mark.gpu

# Eval mode (running statistics): bounds against the emulating oracle, measured MI355X value beside each (base 64, T 4, B 2,
# 128x160, bf16 activations, time-in-channels).  The plain float64 oracle is 10x-1000x farther: output 5.8e-4, whole gradient
# 6.4e-4, worst tensor 6.1e-2 / 3.9e-2, drefs 0.38.
EVAL = {"out": 1e-3,                 # 3.05e-4 max-normalised
        "loss": 2e-6,                # 4.8e-7
        "whole_l2": 2e-4,            # 4.1e-5
        "tensor_max": 4e-2,          # 1.1e-2 (spatial_encoder.stage3.2.conv1.bn.bias)
        "tensor_l2": 2e-2,           # 5.3e-3 (spatial_encoder.stage3.2.conv1.depthwise.weight)
        "inputs": (5e-4, 5e-2, 5e-4)}  # dframe 5.0e-5, drefs 2.2e-2, dmask 1.2e-4 (relative L2)
# drefs is the one tensor above 5e-3: the reference frames' gradient is a mean over four frames of nearly cancelling terms;
# the same emulation evaluated in float32 on the CPU sits 2.2e-2 from it too, and the exact fp32 mode 4e-3 from float64.

# Training mode (batch statistics): the step is chaotic in the rounding.  A bf16 rounding flipped by fp32 against float64
# accumulation moves a value by a whole bf16 step; where a BatchNorm channel's mean is large against its spread that step is a
# sizeable part of the normalised value, and the flips multiply from layer to layer.  The emulating oracle evaluated in float32
# on the CPU - the same rounding points, a different accumulation - is as far from itself in float64 as HIP is (128x160 bf16
# activations: whole gradient 5.8e-2 / HIP 6.0e-2, output 6.2e-2 / 6.7e-2, input gradients 0.35-0.39 / 0.35-0.41).  So in
# training mode HIP is held to that floor, measured in the test: each metric at most FLOOR_FACTOR x the float32 emulation's
# distance, + FLOOR_SLACK.  The running-statistics updates are not chaotic and keep a bound of their own.
FLOOR_FACTOR, FLOOR_SLACK = 3.0, 1e-3
BN_MAX = 1e-2                        # running-statistics update of one BatchNorm, max-normalised: 2.6e-3 (8.1e-4 at 270x480)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def fr_net(sd, base, T, train, tic, acts):
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet
    net = FrameRecoveryNet(3, base, T)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    net.time_in_channels = tic
    net.math_mode, net.bf16_activations = _nvq.MATH_BF16, acts
    return net


def inputs(B, T, H, W, central_mask=False, seed=5):
    """a clip and a soft mask in (0.05, 0.95), or the bench's mask: ones over the central quarter of the frame"""
    clip = synth.formula_clip(B, T + 1, H, W, seed=seed)
    if central_mask:
        mask = torch.zeros(B, 1, H, W)
        mask[:, :, H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 1.0
    else:
        mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed))
    return clip[:, 0].contiguous(), clip[:, 1:].contiguous(), mask, synth.formula_target(B, H, W, seed=seed + 1)


def hip_step(net, frame, refs, mask, tgt):
    """output, loss, parameter gradients, BatchNorm running-statistics updates, input gradients"""
    before = {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k}
    xs = [t.cuda().requires_grad_() for t in (frame, refs, mask)]
    out = net(*xs)
    loss = F.mse_loss(out, tgt.cuda())
    loss.backward()
    torch.cuda.synchronize()
    after = net.state_dict()
    return (out.detach().cpu(), loss.item(), {n: p.grad.cpu() for n, p in net.named_parameters()},
            {k: (after[k] - v).cpu() for k, v in before.items()}, [x.grad.cpu() for x in xs])


def oracle_step(sd, frame, refs, mask, tgt, train, prec, time_major, dt=torch.float64):
    """the same on the CPU, in float64 (or dt)"""
    P = {k: (v.detach().to(dt).clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone())
         for k, v in sd.items()}
    before = {k: v.clone() for k, v in P.items() if "running" in k}
    xs = [t.to(dt).clone().requires_grad_() for t in (frame, refs, mask)]
    out = fr_oracle.frame_recovery_forward(P, *xs, train, prec=prec, time_major=time_major)
    loss = F.mse_loss(out, tgt.to(dt))
    loss.backward()
    return (out.detach(), loss.item(), {k: v.grad for k, v in P.items() if v.grad is not None},
            {k: P[k].detach() - v for k, v in before.items()}, [x.grad for x in xs])


def bn_forward_order(sd):
    return [k[:-len("running_mean")] for k in sd if k.endswith("running_mean")]


def backward_groups(names):
    """parameter groups (layer prefixes) in backward order: decoder, fusion, then the encoders, each last layer first"""
    groups = []
    for n in reversed(names):
        g = n.rsplit(".", 1)[0]
        if g not in groups:
            groups.append(g)
    return groups


def metrics(a, b, train):
    """distances of step a from step b: output, loss, whole gradient, every tensor, input gradients, BatchNorm updates"""
    out, loss, grads, bn, dx = a
    o_out, o_loss, o_grads, o_bn, o_dx = b
    names = list(grads)
    per = {n: (rel(grads[n], o_grads[n]), rel_l2(grads[n], o_grads[n])) for n in names}
    m = {"out": rel(out, o_out), "loss": abs(loss - o_loss) / abs(o_loss), "per": per,
         "whole_l2": rel_l2(torch.cat([grads[n].reshape(-1).double() for n in names]),
                            torch.cat([o_grads[n].reshape(-1).double() for n in names])),
         "tensor_max": max(v[0] for v in per.values()), "tensor_l2": max(v[1] for v in per.values()),
         "inputs": [rel_l2(x, y) for x, y in zip(dx, o_dx)]}
    if train:
        m["bn"] = {pre: max(rel(bn[pre + s], o_bn[pre + s]) for s in ("running_mean", "running_var")) for pre in bn_forward_order(o_bn)}
    return m


def attribution(m, tensor_bound):
    """where the deviation starts: the first BatchNorm in forward order whose update deviates, the first parameter group in
    backward order with a tensor over its bound"""
    first_bn = next((f"{p} ({v:.2e})" for p, v in m.get("bn", {}).items() if v > BN_MAX), None)
    names = list(m["per"])
    first_grp = next((g for g in backward_groups(names)
                      if any(tensor_bound(n) for n in names if n.rsplit(".", 1)[0] == g)), None)
    return (f"forward: first deviating BatchNorm {first_bn or 'none'}; backward: first deviating parameter group "
            f"{first_grp or 'none'}")


def check(m, bounds, tensor_bounds):
    """failure messages; bounds: metric -> bound, inputs a 3-tuple; tensor_bounds: name -> (max bound, L2 bound)"""
    bad = [f"{k} {m[k]:.2e} > {bounds[k]:.2e}" for k in ("out", "loss", "whole_l2") if m[k] > bounds[k]]
    bad += [f"{n} {v:.2e} > {b:.2e}" for n, v, b in zip(("dframe", "drefs", "dmask"), m["inputs"], bounds["inputs"]) if v > b]
    bad += [f"{n} max {mx:.2e} L2 {l2:.2e} > {tensor_bounds(n)}" for n, (mx, l2) in m["per"].items()
            if mx > tensor_bounds(n)[0] or l2 > tensor_bounds(n)[1]]
    bad += [f"BatchNorm {p} update {v:.2e} > {BN_MAX}" for p, v in m.get("bn", {}).items() if v > BN_MAX]
    if not bad:
        return []
    over = lambda n: m["per"][n][0] > tensor_bounds(n)[0] or m["per"][n][1] > tensor_bounds(n)[1]   # noqa: E731
    return [attribution(m, over) + ": " + "; ".join(bad)]


def fmt(m):
    worst_max = max(m["per"].items(), key=lambda kv: kv[1][0])
    worst_l2 = max(m["per"].items(), key=lambda kv: kv[1][1])
    s = (f"out {m['out']:.2e} loss {m['loss']:.1e} whole L2 {m['whole_l2']:.2e} worst max {worst_max[0]} {worst_max[1][0]:.2e} "
         f"worst L2 {worst_l2[0]} {worst_l2[1][1]:.2e} inputs " + " ".join(f"{v:.2e}" for v in m["inputs"]))
    if "bn" in m:
        p = max(m["bn"], key=m["bn"].get)
        s += f" worst BN update {p} {m['bn'][p]:.2e}"
    return s


def run_case(H, W, train, tic, acts, central_mask=False, base=64, T=4, B=2):
    sd = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN)
    frame, refs, mask, tgt = inputs(B, T, H, W, central_mask)
    hip = hip_step(fr_net(sd, base, T, train, tic, acts), frame, refs, mask, tgt)
    prec = "bf16_storage" if acts else "bf16_operands"
    t0 = time.time()
    emu = oracle_step(sd, frame, refs, mask, tgt, train, prec, not tic)
    t_ora = time.time() - t0
    m = metrics(hip, emu, train)
    tag = f"{'train' if train else 'eval'} {'bf16_acts' if acts else 'fp32_acts'} {'tc' if tic else 'tm'} B{B} {H}x{W}"
    print(f"  FR bf16 vs emulating oracle, {tag} (oracle {t_ora:.1f} s): {fmt(m)}")
    print(f"    vs plain float64: {fmt(metrics(hip, oracle_step(sd, frame, refs, mask, tgt, train, None, False), train))}")
    if not train:
        bad = check(m, EVAL, lambda n: (EVAL["tensor_max"], EVAL["tensor_l2"]))
    else:
        floor = metrics(oracle_step(sd, frame, refs, mask, tgt, train, prec, not tic, torch.float32), emu, train)
        print(f"    floor (the emulation in float32): {fmt(floor)}")
        lim = lambda v: FLOOR_FACTOR * v + FLOOR_SLACK          # noqa: E731
        bounds = {k: lim(floor[k]) for k in ("out", "loss", "whole_l2")}
        bounds["inputs"] = tuple(lim(v) for v in floor["inputs"])
        # per tensor: the float32 emulation's distance for that tensor, or its median over all tensors when that is larger
        med = sorted(v[1] for v in floor["per"].values())[len(floor["per"]) // 2]
        bad = check(m, bounds, lambda n: (lim(max(floor["per"][n][0], med)), lim(max(floor["per"][n][1], med))))
    assert not bad, f"{tag}: {bad[0]}"


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tic", [True, False], ids=["tc", "tm"])
@pytest.mark.parametrize("acts", [True, False], ids=["bf16_acts", "fp32_acts"])
def test_fr_bf16_eval_vs_emulating_oracle(acts, tic):
    run_case(128, 160, False, tic, acts)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tic", [True, False], ids=["tc", "tm"])
@pytest.mark.parametrize("acts", [True, False], ids=["bf16_acts", "fp32_acts"])
def test_fr_bf16_train_vs_emulating_oracle(acts, tic):
    run_case(128, 160, True, tic, acts)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_fr_bf16_cfg4_size_vs_emulating_oracle(train):
    """the bench's default recovery setting (MATH_BF16, bf16 activations, time-in-channels) at 270x480 with B=2 and the bench's
    central mask: BatchNorm statistics over two full-size images, and the conv forms only 270x480 reaches"""
    run_case(270, 480, train, True, True, central_mask=True)
