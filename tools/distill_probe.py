"""Time the distillation losses (csrc/distill.hip) against what they replace (profiles/distillation.txt).
usage: python tools/distill_probe.py [--mode time|kernels|step] [--iters 20] [--rounds 3]
  time    : forward + backward, fused and composed forms alternated, device events around `iters` calls, `rounds` rounds:
              distill_loss folded (alpha, 2 - alpha) against the three MSE nodes it replaces, alpha * ops.mse_loss(s, t) +
              (1 - alpha) * ops.mse_loss(s, y) + ops.mse_loss(s, y), at 8 x 3 x 128 x 128 and 8 x 3 x 1080 x 1920;
              cosine_feature_loss against its torch-op composition at 8 x 64 x 64 x 64 and 8 x 64 x 540 x 960, with the
              algorithmic bytes (forward 2 N reads; backward 2 N reads + N writes when its second sweep over the channels is
              served from cache, 4 N + N when it is not) and the share of the 8 TB/s HBM peak;
              then the two cosine launches alone (forward, backward) for the second-sweep question
  kernels : a few calls of every fused op and nothing else, for `rocprofv3 --kernel-trace --stats`
  step    : one `train_continual.py --strategy distill` step at the script's default size (16 x 3 x 64 x 64 -> 128 x 128, F = 64,
            8 blocks, bf16, graphs auto), teacher registered: fold_task on / off, feature distillation off / 0.1"""
import argparse
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd"))
from nerve_cl import _engine, _nvq, ops  # noqa: E402

HBM_PEAK = 8e12
ALPHA = 0.5


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # us per call


def alternate(fns, iters, rounds):
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(timed(fn, iters))
    return times


def torch_cosine(s, t, eps=1e-8):
    a, b, ab = (s * s).sum(1), (t * t).sum(1), (s * t).sum(1)
    return (1 - ab / (a.clamp_min(eps * eps).sqrt() * b.clamp_min(eps * eps).sqrt())).mean()


def fb(fn, s, *rest):
    def run():
        s.grad = None
        fn(s, *rest).backward()
    return run


def fmt(ts):
    return " ".join(f"{t:9.1f}" for t in ts)


def distill_rows(dev, gen, shape, args):
    y = torch.rand(shape, device=dev, generator=gen)
    t = y + 0.1 * torch.randn(shape, device=dev, generator=gen)
    s = (t + 0.05 * torch.randn(shape, device=dev, generator=gen)).requires_grad_(True)
    n = s.numel()
    fused = fb(lambda a, b, c: ops._distill_weighted(a, b, c, ALPHA, 2 - ALPHA)[0], s, t, y)
    composed = fb(lambda a, b, c: ALPHA * ops.mse_loss(a, b) + (1 - ALPHA) * ops.mse_loss(a, c) + ops.mse_loss(a, c), s, t, y)
    if args.mode == "kernels":
        for _ in range(3):
            fused()
        return
    fused()
    g1 = s.grad.clone()
    composed()
    err = ((s.grad - g1).abs().max() / g1.abs().max()).item()
    tf, tc = alternate((fused, composed), args.iters, args.rounds)
    nbytes = (3 + 3 + 1) * 4 * n            # forward reads s, t, y; backward reads them again and writes ds
    bf, bc = min(tf), min(tc)
    print(f"distill fwd+bwd {'x'.join(map(str, shape)):>16s} fused {fmt(tf)} | three ops.mse_loss nodes {fmt(tc)} | composed / fused "
          f"{bc / bf:5.2f}x | {nbytes / 1e6:7.1f} MB -> {nbytes / bf / 1e6:5.2f} TB/s = {nbytes / (bf * 1e-6) / HBM_PEAK:4.2f} of peak"
          f" | ds fused vs composed {err:.1e} of max", flush=True)


def cosine_rows(dev, gen, shape, args):
    s = torch.randn(shape, device=dev, generator=gen).requires_grad_(True)
    t = torch.randn(shape, device=dev, generator=gen)
    n = s.numel()
    fused, composed = fb(ops.cosine_feature_loss, s, t), fb(torch_cosine, s, t)
    sd, ds = s.detach(), torch.empty_like(s)
    out, go = torch.empty(1, device=dev), torch.ones(1, device=dev)
    ws = _engine.workspace(dev)
    k_fwd = lambda: _nvq.cosine_distill_forward(sd, t, 1e-8, False, out, ws)          # noqa: E731
    k_bwd = lambda: _nvq.cosine_distill_backward(sd, t, 1e-8, go, False, ds)           # noqa: E731
    if args.mode == "kernels":
        for _ in range(3):
            fused()
        return
    tf, tc, t1, t2 = alternate((fused, composed, k_fwd, k_bwd), args.iters, args.rounds)
    bf, bc, b1, b2 = min(tf), min(tc), min(t1), min(t2)
    lo, hi = (2 + 3) * 4 * n, (2 + 5) * 4 * n
    name = "x".join(map(str, shape))
    print(f"cosine fwd+bwd {name:>16s} fused {fmt(tf)} | torch ops {fmt(tc)} | torch / fused {bc / bf:5.2f}x | "
          f"{lo / 1e6:7.1f} MB -> {lo / bf / 1e6:5.2f} TB/s = {lo / (bf * 1e-6) / HBM_PEAK:4.2f} of peak "
          f"({hi / 1e6:.1f} MB with the second sweep from HBM: {hi / (bf * 1e-6) / HBM_PEAK:4.2f})", flush=True)
    print(f"  launches alone {name:>14s} forward (2 launches) {fmt(t1)} = {8 * n / b1 / 1e6:5.2f} TB/s of its 2 N reads | backward "
          f"(1 launch) {fmt(t2)} = {12 * n / b2 / 1e6:5.2f} TB/s counting 2 N reads + N writes, {20 * n / b2 / 1e6:5.2f} TB/s "
          f"counting 4 N reads + N writes | backward / forward {b2 / b1:4.2f}x (1.5x if the second sweep is free, 2.5x if it is "
          f"a second HBM read)", flush=True)


def step_rows(dev, args):
    sys.path.insert(0, os.path.join(REPO, "experiments"))
    import train_continual as tc
    from nerve_cl.continual import ContinualDistillation
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    torch.manual_seed(0)
    lr, hr = tc.create_task_data("sports", 16)
    lr, hr = lr.to(dev), hr.to(dev)
    print("step of train_continual.py --strategy distill: 16 x 3 x 64 x 64 -> 128 x 128, F = 64, 8 blocks, bf16, graphs auto, "
          f"teacher registered; {args.iters} steps per timing, {args.rounds} alternated rounds (us per step)")
    steps = {}
    for feature_weight in (0.0, 0.1):
        for fold in (True, False):
            model = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, super_resolution_enabled=True)).to(dev)
            tc.configure_precision(model, "bf16", "auto")
            model.train()
            cd = ContinualDistillation(tc._SRClipAdapter(model.super_resolution), alpha=ALPHA, feature_weight=feature_weight,
                                       fold_task=fold)
            cd.register_task()
            opt = tc.make_optimizer(torch.optim.Adam, model.parameters(), lr=1e-4)
            crit = ops.MSELoss()

            def step(cd=cd, opt=opt, crit=crit):
                opt.zero_grad()
                cd.compute_loss(lr, hr, crit)["total"].backward()
                opt.step()
            steps[(feature_weight, fold)] = step
    keys = list(steps)
    for _ in range(4):                      # past the graph warm-up and capture of every variant
        for k in keys:
            steps[k]()
    times = alternate([steps[k] for k in keys], args.iters, args.rounds)
    for k, t in zip(keys, times):
        print(f"  feature_weight {k[0]:3.1f} fold_task {str(k[1]):5s} {fmt(t)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "kernels", "step"], default="time")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda", 0)
    if args.mode == "step":
        return step_rows(dev, args)
    gen = torch.Generator(device=dev).manual_seed(1234)
    if args.mode == "time":
        print(f"fp32, {args.iters} calls per timing, {args.rounds} alternated rounds (us per call)")
    for shape in ((8, 3, 128, 128), (8, 3, 1080, 1920)):
        distill_rows(dev, gen, shape, args)
    for shape in ((8, 64, 64, 64), (8, 64, 540, 960)):
        cosine_rows(dev, gen, shape, args)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
