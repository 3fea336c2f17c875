#!/usr/bin/env python3
"""Timings and accuracy of the drift kernels for profiles/drift.txt.

    python tools/drift_probe.py            # on the MI355X

Times ``DriftDetector.detect_device`` (MMD and PSI), ``frame_descriptor`` and, next to them, the host route the reference takes:
the window copied to the host and the biased RBF-MMD formula of its ``_mmd_test`` in float64 numpy (restated here; numpy threads as
the environment sets them).  Device timings: events around ``calls`` back-to-back calls after a warm-up, ``rounds`` rounds, every
round printed; the host route is wall time per call, the device-to-host copy included."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")]

from nerve_cl import drift  # noqa: E402


def device_us(fn, calls: int, rounds: int):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return out


def host_us(fn, calls: int, rounds: int):
    fn()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return out


def numpy_mmd(ref_dev: torch.Tensor, cur_dev: torch.Tensor) -> float:
    """the reference's route: both windows to the host, then its formula (all rows: the sets have at most 500)"""
    x = ref_dev.cpu().numpy().astype(np.float64)
    y = cur_dev.cpu().numpy().astype(np.float64)
    gamma = 1.0 / x.shape[1]

    def k(a, b):
        d = np.sum(a ** 2, axis=1, keepdims=True) + np.sum(b ** 2, axis=1, keepdims=True).T - 2 * a @ b.T
        return np.exp(-gamma * d)
    return k(x, x).mean() + k(y, y).mean() - 2 * k(x, y).mean()


def row(label: str, values) -> None:
    print(f"  {label:66s}" + "".join(f"{v:10.1f}" for v in values))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"us per call, {args.rounds} rounds of {args.calls} calls; numpy threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}")
    for n, d in ((500, 384), (500, 12288)):
        ref = torch.randn(n, d, generator=g).to(dev)
        cur = (torch.randn(n, d, generator=g) + 0.1).to(dev)
        print(f"windows of {n} x {d}")
        for method in ("mmd", "psi"):
            det = drift.DriftDetector(method=method)
            det.set_reference(ref)
            row(f"DriftDetector('{method}').detect_device", device_us(lambda: det.detect_device(cur), args.calls, args.rounds))
            row(f"DriftDetector('{method}').detect (one host copy)", host_us(lambda: det.detect(cur), args.calls, args.rounds))
        det = drift.DriftDetector(method="mmd")
        det.set_reference(ref)
        got, want = det.detect(cur).score, numpy_mmd(ref, cur)
        row("numpy route: two device-to-host copies + float64 formula", host_us(lambda: numpy_mmd(ref, cur), max(args.calls // 40, 2), args.rounds))
        print(f"    mmd {got:.12f} (device) {want:.12f} (numpy), {abs(got - want):.2e} apart")
    for shape in ((8, 3, 64, 64), (200, 3, 64, 64)):
        x = torch.randn(*shape, generator=g).to(dev)
        row(f"frame_descriptor {shape}, grid 8 x 8", device_us(lambda: drift.frame_descriptor(x), args.calls, args.rounds))
        row(f"torch composition {shape} (adaptive_avg_pool2d of x and x^2, fp32)",
            device_us(lambda: _torch_descriptor(x), args.calls, args.rounds))


def _torch_descriptor(x: torch.Tensor) -> torch.Tensor:
    import torch.nn.functional as F
    mean = F.adaptive_avg_pool2d(x, (8, 8))
    var = (F.adaptive_avg_pool2d(x * x, (8, 8)) - mean * mean).clamp_min(0)
    return torch.cat([mean.flatten(1), var.sqrt().flatten(1)], 1)


if __name__ == "__main__":
    main()
