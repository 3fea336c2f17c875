"""GPU: VALUE parity of the full-size training steps (reference nerve_cl/models/super_resolution.py:327-391) against a float64
evaluation of the same step.

tests/test_real_size_gpu.py compares values at 135x240 (B=1), where most launches fit in one pass of their grid, and
tests/test_full_size_gpu.py checks only properties (determinism, batch independence, linearity in dout) at 540x960.  A tile
walk that drops or double-counts a tile after its first pass (the persistent weight gradients, the correlation gradient's
(tile, frame group) steps, the weight-gradient pixel splits), an offset that wraps, or a BatchNorm sum over 4.1M pixels that
loses precision passes all of those.  Here the whole step runs at bench.py's sizes:

  cfg2: SuperResolutionNet(3, 2, 64, 8, 1), B=2 clips of 3 x 540x960 -> 1080x1920 (B=2: the BatchNorm statistics and the
        weight-gradient splits span two images);
  cfg4: SuperResolutionNet(3, 4, 64, 8, 2), B=2 clips of 5 x 270x480 -> 1080x1920;

in the exact-fp32 mode and in the benchmarked bf16 mode, train mode, MSE loss.  The yardstick is
oracle/sr_oracle.py:sr_forward_checkpointed in float64 on the GPU (torch's own fp64 kernels, no libnvq): every stage under
non-reentrant checkpointing, so that the ~75 GB of autograd state of a plain full-size oracle step are never held at once.

Every run prints the per-stage errors (forward: features, flows, aligned, aggregated, residual, fused; backward: the
gradients the HIP backward leaves in nerve_cl._engine.DEBUG_CAPTURE against the oracle's retained .grad) and names the first
stage that deviates; assertion messages carry the same attribution.  Inputs and weights are the closed-form ones of
oracle/synth.py."""
import gc
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import sr_oracle, synth

pytestmark = pytest.mark.gpu

Fc, NB = 64, 8
CFGS = {
    "cfg2": dict(scale=2, win=1, B=2, H=540, W=960, seed_x=41, seed_t=42),
    "cfg4": dict(scale=4, win=2, B=2, H=270, W=480, seed_x=43, seed_t=44),
}
PEAK_CAP = 64 << 30          # the oracle's GPU memory budget (the card is shared)
# a stage "deviates" when its relative L2 error against float64 exceeds this (exact-fp32 / bf16 mode)
STAGE_TOL = {False: 1e-3, True: 3e-2}


def _inputs(cfg):
    T = 2 * cfg["win"] + 1
    x = synth.formula_clip(cfg["B"], T, cfg["H"], cfg["W"], seed=cfg["seed_x"])
    tgt = synth.formula_target(cfg["B"], cfg["H"] * cfg["scale"], cfg["W"] * cfg["scale"], seed=cfg["seed_t"])
    return x, tgt


def _state(cfg):
    return synth.formula_state(3, cfg["scale"], Fc, NB, cfg["win"], gain=synth.GOLDEN_GAIN)


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _oracle_step(cfg):
    """float64 training step on the GPU; everything it returns lives on the CPU (stage tensors as float32: they only serve
    the attribution)"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    x, tgt = _inputs(cfg)
    ora = sr_oracle.OracleSR(3, cfg["scale"], Fc, NB, cfg["win"])
    ora.load_named(_state(cfg))
    ora = ora.double().cuda().train()
    P = ora.P()
    _free()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, inter = sr_oracle.sr_forward_checkpointed(P, x.double().cuda(), training=True)
    T = len(inter["features"])
    c = T // 2
    stages = _stage_list(inter, c)
    for _, v in stages:
        v.retain_grad()
    bufs = {n: P[n].detach().cpu().clone() for n in ora._bufs}      # after the forward (the recompute updates them again)
    loss = F.mse_loss(out, tgt.double().cuda())
    loss.backward()
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    res = {
        "out": out.detach().cpu(), "loss": loss.item(),
        "grads": {n: P[n].grad.detach().cpu() for n in ora._names},
        "bufs": bufs,
        "fwd": {k: v.detach().float().cpu() for k, v in stages},
        "bwd": {k: v.grad.detach().float().cpu() for k, v in stages},
        "peak": peak, "secs": secs,
    }
    print(f"\n  float64 oracle step ({cfg['B']} x {T} x {cfg['H']}x{cfg['W']}, checkpointed, GPU): {secs:.1f} s, "
          f"peak {peak / 2**30:.1f} GiB (model + inputs {base / 2**30:.2f} GiB)")
    del out, inter, stages, loss, P, ora
    _free()
    return res


def _stage_list(inter, c):
    """(name, tensor) of the stage tensors in forward order, NCHW as the oracle holds them (the centre frame's `aligned` IS its
    features: not listed twice)"""
    T = len(inter["features"])
    rows = [(f"features[{t}]", inter["features"][t]) for t in range(T)]
    rows += [(f"flow[{t}]", inter["flows"][t]) for t in range(T) if t != c]
    rows += [(f"aligned[{t}]", inter["aligned"][t]) for t in range(T) if t != c]
    rows += [("aggregated", inter["aggregated"]), ("residual", inter["residual"]), ("fused", inter["fused"])]
    return rows


def _nchw(t, c=None, off=0):
    c = t.shape[-1] - off if c is None else c
    return t[..., off:off + c].permute(0, 3, 1, 2).float().cpu()


def _hip_step(cfg, bf16):
    """one training step of the HIP path, the stage tensors and gradients in the oracle's layout"""
    from nerve_cl import _engine, _nvq
    from nerve_cl.models import SuperResolutionNet
    x, tgt = _inputs(cfg)
    net = SuperResolutionNet(3, cfg["scale"], Fc, NB, cfg["win"])
    net.load_state_dict(_state(cfg), strict=True)
    net = net.cuda().train()
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    B, T = cfg["B"], 2 * cfg["win"] + 1
    c = T // 2
    slots = [c] + [t for t in range(T) if t != c]        # the engine's frame order of batched per-frame tensors
    cap = {}
    _engine.DEBUG_CAPTURE = cap
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, inter = net(x.cuda(), return_intermediate=True)
        loss = F.mse_loss(out, tgt.cuda())
        loss.backward()
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
    finally:
        _engine.DEBUG_CAPTURE = None
    fwd, bwd = {}, {}
    for t in range(T):
        fwd[f"features[{t}]"] = inter["features"][t].float().cpu()
    for j in range(1, T):
        t = slots[j]
        fwd[f"flow[{t}]"] = _nchw(cap["flow"][(j - 1) * B:j * B], 2)
        fwd[f"aligned[{t}]"] = inter["aligned"][t].float().cpu()
        bwd[f"aligned[{t}]"] = _nchw(cap["daligned"], Fc, t * Fc)
        bwd[f"flow[{t}]"] = _nchw(cap["dflow"][(j - 1) * B:j * B], 2)
    for j, t in enumerate(slots):
        bwd[f"features[{t}]"] = _nchw(cap["dfeat_all"][j * B:(j + 1) * B])
    fwd["aggregated"] = inter["aggregated"].float().cpu()
    fwd["residual"], fwd["fused"] = _nchw(cap["residual"]), _nchw(cap["fused"])
    bwd["aggregated"], bwd["residual"], bwd["fused"] = _nchw(cap["dagg"]), _nchw(cap["dres"]), _nchw(cap["dfused"])
    res = {
        "out": out.detach().double().cpu(), "loss": loss.item(),
        "grads": {n: p.grad.detach().double().cpu() for n, p in net.named_parameters()},
        "bufs": {k: v.detach().cpu() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k},
        "fwd": fwd, "bwd": bwd, "secs": secs,
    }
    del out, inter, loss, cap, net
    _free()
    return res


def _err(a, b):
    """(relative L2, max-normalised element error) of a against the yardstick b"""
    a, b = a.double(), b.double()
    d = a - b
    return (d.norm() / b.norm().clamp_min(1e-300)).item(), (d.abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _dout(out, tgt):
    """the loss gradient at the network's output, behind the clamp (zero where the output sits on a rail)"""
    return 2.0 / out.numel() * (out - tgt) * ((out > 0) & (out < 1))


def _attribution(hip, ora, tgt, bf16):
    """Per-stage error table, forward order (frames -> output), then backward order (output -> frames), and the first stage
    that DEVIATES: its relative L2 error exceeds STAGE_TOL and 4x the largest error of the stages before it - an error that
    is only carried along from an earlier stage is not new.  The backward starts from the output gradient behind the clamp,
    which is a function of the output alone: where an output sits within rounding of a rail, its mask differs between the
    two evaluations (a handful of pixels in fp32 mode, ~0.6 % in bf16 mode), so that stage sets the level the backward
    stages are measured against instead of being flagged itself.  A defect in a weight-gradient kernel leaves every stage
    clean: the parameter gradients then carry it alone."""
    tol = STAGE_TOL[bf16]
    names = list(ora["fwd"])
    tgt = tgt.double()
    rails = ((hip["out"] > 0) & (hip["out"] < 1)) != ((ora["out"] > 0) & (ora["out"] < 1))
    # the backward runs from the output towards the frames: out, fused, residual, aggregated, aligned, flow, features
    order = [(f, hip["fwd"][f], ora["fwd"][f]) for f in names] + [("out", hip["out"], ora["out"]),
                                                                  ("d out", _dout(hip["out"], tgt), _dout(ora["out"], tgt))]
    order += [(f"d {f}", hip["bwd"][f], ora["bwd"][f]) for f in reversed(names)]
    rows, first, carried = [], None, 0.0
    for label, a, b in order:
        l2, mx = _err(a, b)
        rows.append(f"{label:>18}: L2 {l2:.2e}  max {mx:.2e}")
        if first is None and label != "d out" and l2 > tol and l2 > 4 * carried:
            first = label
        carried = max(carried, l2)
    return ("stage errors vs float64 (" + ("bf16" if bf16 else "fp32") + " mode):\n    " + "\n    ".join(rows) +
            f"\n  outputs on a clamp rail in one evaluation only: {int(rails.sum())} of {rails.numel()}"
            f"\n  first stage that deviates (L2 over {tol:g} and over 4x the stages before it): "
            f"{first or 'none (a parameter-gradient error then comes from a weight-gradient kernel)'}")


_ORACLE = {}


@pytest.fixture(scope="module")
def oracle():
    """the float64 step of each geometry, computed once for both modes and held on the CPU"""
    def get(name):
        if name not in _ORACLE:
            _ORACLE.clear()                                   # (one geometry's CPU copies at a time)
            _free()
            _ORACLE[name] = _oracle_step(CFGS[name])
        return _ORACLE[name]
    yield get
    _ORACLE.clear()


def _check_fp32(name, oracle):
    ora = oracle(name)
    assert ora["peak"] < PEAK_CAP, f"float64 oracle peak {ora['peak'] / 2**30:.1f} GiB"
    hip = _hip_step(CFGS[name], False)
    att = _attribution(hip, ora, _inputs(CFGS[name])[1], False)
    out_err = (hip["out"] - ora["out"]).abs().max().item()
    loss_rel = abs(hip["loss"] - ora["loss"]) / ora["loss"]
    rows, over, bad, num, den = [], [], [], 0.0, 0.0
    for n, r in ora["grads"].items():
        g = hip["grads"][n]
        l2, mx = _err(g, r)
        num += float(((g - r) ** 2).sum())
        den += float((r ** 2).sum())
        rows.append((max(l2, mx), n, l2, mx))
        if l2 >= 1e-3 or mx >= 1e-3:
            over.append(f"{n}: L2 {l2:.2e} max {mx:.2e}")
        if l2 >= 1e-2 or mx >= 2e-2:
            bad.append(f"{n}: L2 {l2:.2e} max {mx:.2e}")
    glob = (num / den) ** 0.5
    buf_err = {n: _err(hip["bufs"][n], ora["bufs"][n])[1] for n in ora["bufs"]}
    rows.sort(reverse=True)
    print(f"\n  {name} fp32 mode: HIP step {hip['secs']:.2f} s; output max abs err {out_err:.2e}; loss {hip['loss']:.8f} vs "
          f"{ora['loss']:.8f} (rel {loss_rel:.2e}); whole-gradient rel L2 {glob:.2e}; worst BN buffer {max(buf_err.values()):.2e}")
    print("  worst gradients (L2, max-normalised):")
    for _, n, l2, mx in rows[:8]:
        print(f"    {n}: L2 {l2:.2e} max {mx:.2e}")
    print("  tensors over 1e-3:", over or "none")
    print("  " + att)
    assert out_err < 1e-3, att
    assert loss_rel < 1e-5, att
    for n, e in buf_err.items():
        assert e < 1e-3, (n, e, att)
    assert glob < 1e-4, (glob, att)
    assert not bad, (bad, att)
    assert len(over) <= 3, (over, att)


def _check_bf16(name, oracle):
    ora = oracle(name)
    hip = _hip_step(CFGS[name], True)
    att = _attribution(hip, ora, _inputs(CFGS[name])[1], True)
    psnr = sr_oracle.compute_psnr(hip["out"], ora["out"])
    loss_rel = abs(hip["loss"] - ora["loss"]) / ora["loss"]
    cos_min, at, flow_min, dot, na, nb = 1.0, None, 1.0, 0.0, 0.0, 0.0
    worst_l2 = []
    for n, r in ora["grads"].items():
        a, b = hip["grads"][n].reshape(-1), r.reshape(-1)
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))
        dot += float(a @ b); na += float(a @ a); nb += float(b @ b)
        worst_l2.append((_err(a, b)[0], n))
        if "motion_estimator" in n:
            flow_min = min(flow_min, cos)
        elif cos < cos_min:
            cos_min, at = cos, n
    whole = dot / (na * nb) ** 0.5
    whole_l2 = (sum(float(((hip["grads"][n] - r) ** 2).sum()) for n, r in ora["grads"].items()) / nb) ** 0.5
    worst_l2.sort(reverse=True)
    print(f"\n  {name} bf16 mode: HIP step {hip['secs']:.2f} s; PSNR vs float64 {psnr:.1f} dB; loss {hip['loss']:.6f} vs "
          f"{ora['loss']:.6f} (rel {loss_rel:.2e}); min non-flow gradient cosine {cos_min:.5f} at {at} (flow net "
          f"{flow_min:.4f}); whole-gradient cosine {whole:.6f}, rel L2 {whole_l2:.2e}")
    print("  worst gradients (rel L2):", ", ".join(f"{n} {e:.2e}" for e, n in worst_l2[:6]))
    print("  " + att)
    assert psnr > 41.0, (psnr, att)
    assert loss_rel < 2e-3, (loss_rel, att)
    assert cos_min > 0.98, (cos_min, at, att)
    assert whole > 0.995, (whole, att)
    # (measured 2.9e-3 at both geometries.  bf16 weight-gradient pixel splits that skip their last tile at full size give
    # 5.3e-2 at cfg2 while every cosine above still passes: this bound, not the cosines, catches a dropped tile)
    assert whole_l2 < 1e-2, (whole_l2, att)


@pytest.mark.timeout(2400)
def test_cfg2_full_size_training_step_fp32_vs_float64(oracle):
    _check_fp32("cfg2", oracle)


@pytest.mark.timeout(1200)
def test_cfg2_full_size_training_step_benchmarked_bf16_mode_vs_float64(oracle):
    _check_bf16("cfg2", oracle)


@pytest.mark.timeout(1800)
def test_cfg4_sr_full_size_training_step_fp32_vs_float64(oracle):
    _check_fp32("cfg4", oracle)


@pytest.mark.timeout(1200)
def test_cfg4_sr_full_size_training_step_benchmarked_bf16_mode_vs_float64(oracle):
    _check_bf16("cfg4", oracle)
