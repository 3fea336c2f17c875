#!/usr/bin/env python3
"""Timings behind profiles/device_memory.txt: DeviceEpisodicMemory against the host EpisodicMemory at the cfg2 sample size
(3x540x960 LR, 3x1080x1920 HR), HIP events, median over --reps repetitions after --warmup.

    python tools/device_memory_probe.py [--reps 20] [--warmup 3] [--small]

Bytes are counted as bytes read plus bytes written by the kernel; the fraction is of the 8 TB/s HBM peak."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")]

from nerve_cl import _nvq  # noqa: E402
from nerve_cl.continual import DeviceEpisodicMemory, EpisodicMemory  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps, warmup):
    """median ms of fn() between two events (the device is idle when each repetition starts)"""
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def line(label, ms, nbytes=None):
    med, lo, hi = ms
    s = f"{label:<58s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})"
    if nbytes:
        rate = nbytes / (med * 1e-3)
        s += f"  {nbytes / 1e6:8.1f} MB  {rate / 1e12:5.2f} TB/s = {rate / PEAK:4.2f} of peak"
    print(s, flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="64x64 / 128x128 samples (a dry run of the script)")
    args = ap.parse_args()
    lr_shape, hr_shape = ((3, 64, 64), (3, 128, 128)) if args.small else ((3, 540, 960), (3, 1080, 1920))
    n = 8
    g = torch.Generator().manual_seed(0)
    lr, hr = torch.rand((n,) + lr_shape, generator=g).cuda(), torch.rand((n,) + hr_shape, generator=g).cuda()
    cur_lr, cur_hr = torch.rand((n,) + lr_shape, generator=g).cuda(), torch.rand((n,) + hr_shape, generator=g).cuda()
    per = lr[0].numel() + hr[0].numel()
    print(f"# {torch.cuda.get_device_name(0)}; sample = LR {lr_shape} + HR {hr_shape} = {per * 4 / 1e6:.1f} MB in fp32; "
          f"{n} replay samples behind a batch of {n}; {args.reps} repetitions after {args.warmup} warm-up")

    host = EpisodicMemory(capacity=n, strategy="fifo", seed=0)

    def host_store():
        for j in range(n):
            host.store(lr[j], hr[j], {"content_type": "movie"})
    t_host_store = line(f"host: {n} x EpisodicMemory.store from GPU tensors", timed(host_store, args.reps, args.warmup))

    def host_replay():
        r_lr, r_hr, _ = host.sample(n, device="cuda")
        return torch.cat([cur_lr, r_lr]), torch.cat([cur_hr, r_hr])
    t_host = line(f"host: sample({n}, device='cuda') + 2 x torch.cat", timed(host_replay, args.reps, args.warmup))

    for storage, esz in (("fp32", 4), ("bf16", 2)):
        mem = DeviceEpisodicMemory(capacity=n, strategy="fifo", seed=0, device="cuda", storage=storage)
        t = line(f"device[{storage}]: store_batch of {n} (copy + mean kernels)",
                 timed(lambda: mem.store_batch(lr, hr, content_type="movie"), args.reps, args.warmup),
                 n * (per * (4 + esz) + lr[0].numel() * 4))
        print(f"    -> {t_host_store / t:.1f} x the host stores")
        t = line(f"device[{storage}]: replay_batch (empty + 2 copies + gather)",
                 timed(lambda: mem.replay_batch(cur_lr, cur_hr, n), args.reps, args.warmup))
        print(f"    -> {t_host / t:.1f} x the host path")
        out_lr, out_hr = torch.empty((2 * n,) + lr_shape, device="cuda"), torch.empty((2 * n,) + hr_shape, device="cuda")
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        line(f"device[{storage}]: nvq_replay_gather alone, {n} samples",
             timed(lambda: _nvq.replay_gather(mem._lr, mem._hr, idx, out_lr, out_hr, n, mem._access), args.reps, args.warmup),
             n * per * (4 + esz))
        t = line(f"device[{storage}]: replay_batch(weighted=True) + update_importance",
                 timed(lambda: mem.update_importance(mem.replay_batch(cur_lr, cur_hr, n, weighted=True)[2],
                                                     torch.ones(n, device="cuda"), 0.9), args.reps, args.warmup))
        del mem, out_lr, out_hr
        torch.cuda.empty_cache()

    for cap in (1000, 65536):
        imp, tm = torch.rand(cap, device="cuda") + 0.1, torch.randint(1, 100, (cap,), dtype=torch.int32, device="cuda")
        tid, u = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.rand(cap, device="cuda").clamp_min_(1e-30)
        out = torch.empty(8, dtype=torch.int32, device="cuda")
        line(f"nvq_replay_sample_weighted capacity {cap}, k = 8",
             timed(lambda: _nvq.replay_sample_weighted(imp, tm, tid, 100, 0.2, -1, u, out), args.reps, args.warmup))


if __name__ == "__main__":
    main()
