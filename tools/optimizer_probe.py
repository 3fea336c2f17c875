"""Time the flat-bucket optimizer (nerve_cl.optim, csrc/optim.hip) against what it replaces
(profiles/bucket_optimizer.txt).
usage: python tools/optimizer_probe.py [--mode optimizer|step] [--iters 50] [--rounds 5]
  optimizer : on the default SR engine (F = 64, 8 blocks, 131 parameter tensors) after a step's real backward, so that .grad
              aliases the gradient bucket: `iters` optimizer calls per timing, the forms alternated over `rounds` rounds.  Two
              clocks per form: "host" = the host clock around the calls without a synchronise (what the step's host thread pays to
              enqueue the update), "loop" = device events around the same calls (the larger of host and device time per call).
                torch           experiments/_common.make_optimizer(torch.optim.Adam): torch's fused Adam over the tensor lists
                bucket          BucketAdam: one nvq_adam_step launch
                torch + clip    ops.clip_grad_norm_(engine) in front of torch's step (three launches that rewrite the gradient)
                bucket + clip   BucketAdam(max_grad_norm): nvq_bucket_moments (two launches) + the one update launch
                bucket + clip + ema   the same with ema_decay
              max_norm is half the gradient norm at first and the norm of a clipped gradient after, so every call clips.
  step      : one train_continual.py EWC step at the continual-learning frame size (8 clips of 3 x 64 x 64 -> 128 x 128, F = 64,
              8 blocks, bf16, graphs auto, loss = mse + penalty after a registered task) with each of the forms above; host clock
              around `iters` synchronised steps"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd"))
sys.path.insert(0, os.path.join(REPO, "experiments"))
from nerve_cl import ops  # noqa: E402
from nerve_cl.continual import EWC  # noqa: E402
from nerve_cl.models import EnhancementConfig, EnhancementEngine  # noqa: E402

FORMS = ("torch", "bucket", "torch + clip", "bucket + clip", "bucket + clip + ema")


def make(form, model, max_norm):
    """-> (optimizer, clip or None): the optimizer of `form` and the separate clipping call it needs in front of step()"""
    import train_continual as tc
    impl = "bucket" if form.startswith("bucket") else "torch"
    kw = {}
    if impl == "bucket":
        kw = dict(max_grad_norm=max_norm if "clip" in form else None, ema_decay=0.999 if "ema" in form else None)
    opt = tc.make_optimizer(torch.optim.Adam, model.parameters(), impl, lr=1e-4, **kw)
    clip = (lambda: ops.clip_grad_norm_(model, max_norm)) if form == "torch + clip" else None
    return opt, clip


def launches(opt, form):
    if not form.startswith("bucket"):
        return "torch's own"
    return f"{opt.last_launches} update" + (" + 2 norm" if "clip" in form else "")


def timed_calls(fn, iters):
    """-> (host us per call without a synchronise, device-event us per call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) / iters * 1e6
    b.record()
    torch.cuda.synchronize()
    return host, a.elapsed_time(b) / iters * 1e3


def fmt(ts):
    return " ".join(f"{t:8.1f}" for t in ts)


def optimizer_rows(dev, args):
    torch.manual_seed(0)
    model = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, super_resolution_enabled=True)).to(dev).train()
    net = model.super_resolution
    x = torch.randn(2, 3, 3, 32, 32, device=dev)
    y = torch.randn(2, 3, 64, 64, device=dev)
    model.zero_grad()
    ops.mse_loss(model(x)["enhanced"], y).backward()
    bucket = net._last_grad_bucket
    max_norm = 0.5 * bucket.norm().item()
    print(f"optimizer call on the default SR engine: {bucket.numel()} floats in the bucket ({4 * bucket.numel() / 1e6:.1f} MB), "
          f"{len(list(net.parameters()))} parameter tensors; {args.iters} calls per timing, {args.rounds} alternated rounds (us per call)")
    calls, opts = [], []
    for form in FORMS:
        opt, clip = make(form, model, max_norm)
        opts.append(opt)

        def call(opt=opt, clip=clip):
            if clip is not None:
                clip()
            opt.step()
        calls.append(call)
    for _ in range(3):
        for c in calls:
            c()
    host = [[] for _ in FORMS]
    loop = [[] for _ in FORMS]
    for _ in range(args.rounds):
        for h, l, c in zip(host, loop, calls):
            a, b = timed_calls(c, args.iters)
            h.append(a)
            l.append(b)
    for form, opt, h, l in zip(FORMS, opts, host, loop):
        print(f"  {form:20s} host {fmt(h)}   loop {fmt(l)}   launches: {launches(opt, form)}", flush=True)
    best = {f: (min(h), min(l)) for f, h, l in zip(FORMS, host, loop)}
    for a, b in (("torch", "bucket"), ("torch + clip", "bucket + clip")):
        print(f"  best of each, {a} / {b}: host {best[a][0] / best[b][0]:.2f}x, loop {best[a][1] / best[b][1]:.2f}x")


def step_rows(dev, args):
    import train_continual as tc
    torch.manual_seed(0)
    lr, hr = tc.create_task_data("sports", 64)
    lr, hr = lr.to(dev), hr.to(dev)
    batch = 8
    loader = [(lr[i:i + batch], hr[i:i + batch]) for i in range(0, 64, batch)]
    print(f"EWC step of train_continual.py: {batch} x 3 x 64 x 64 -> 128 x 128, F = 64, 8 blocks, bf16, graphs auto, loss = mse + penalty; "
          f"{args.iters} steps per timing, {args.rounds} alternated rounds (us per step, host clock, synchronised)")
    steps, opts = [], []
    for form in FORMS:
        torch.manual_seed(0)
        model = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, super_resolution_enabled=True)).to(dev)
        tc.configure_precision(model, "bf16", "auto")
        ewc = EWC(tc._ClipAdapter(model), ewc_lambda=5000)
        opt, clip = make(form, model, 1.0)
        opts.append(opt)
        crit = ops.MSELoss()

        def step(a, b, model=model, ewc=ewc, opt=opt, clip=clip, crit=crit):
            opt.zero_grad()
            out = model(a.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]
            (crit(out, b) + ewc.penalty()).backward()
            if clip is not None:
                clip()
            opt.step()
        model.train()
        for a, b in loader[:3]:
            step(a, b)
        ewc.register_task(0, loader[:2])
        model.train()
        for a, b in loader:                     # past the graph warm-up and capture
            step(a, b)
        steps.append(step)
    times = [[] for _ in FORMS]
    for _ in range(args.rounds):
        for t, step in zip(times, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.iters):
                step(*loader[i % len(loader)])
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / args.iters * 1e6)
    for form, opt, t in zip(FORMS, opts, times):
        print(f"  {form:20s} {fmt(t)}   launches: {launches(opt, form)}", flush=True)
    best = {f: min(t) for f, t in zip(FORMS, times)}
    print(f"  best of each: torch / bucket {best['torch'] / best['bucket']:.3f}x, torch + clip / bucket + clip "
          f"{best['torch + clip'] / best['bucket + clip']:.3f}x, bucket + clip + ema / bucket + clip "
          f"{best['bucket + clip + ema'] / best['bucket + clip']:.3f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["optimizer", "step"], default="optimizer")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda", 0)
    (step_rows if args.mode == "step" else optimizer_rows)(dev, args)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
