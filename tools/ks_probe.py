#!/usr/bin/env python3
"""Timings of the Kolmogorov-Smirnov drift route for profiles/ks.txt.

    python tools/ks_probe.py            # on the MI355X

Times ``KSDriftDetector.detect_device`` (the sort of the current window, the statistic, the p-values and the decision; the
reference was sorted in ``set_reference``) and its three launches on their own, and, where scipy is importable, the host route
the reference takes: the window copied to the host and ``scipy.stats.ks_2samp`` per feature.  Device timings: events around
``calls`` back-to-back calls after a warm-up, ``rounds`` rounds, every round and the median printed; the host route is wall time
per call, the device-to-host copy included."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")]

from nerve_cl import _nvq, drift  # noqa: E402


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


def row(label: str, values) -> None:
    print(f"  {label:66s}" + "".join(f"{v:11.1f}" for v in values) + f"   median {statistics.median(values):.1f}")


def scipy_route(ref_dev: torch.Tensor, cur_dev: torch.Tensor) -> float:
    """the reference's route: both windows to the host, then its loop over the features"""
    from scipy import stats
    x = ref_dev.cpu().numpy().astype(np.float64)
    y = cur_dev.cpu().numpy().astype(np.float64)
    return min(stats.ks_2samp(x[:, i], y[:, i])[1] for i in range(x.shape[1])) * x.shape[1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    print(f"us per call, {args.rounds} rounds of {args.calls} calls")
    for n1, n2, d in ((1000, 1000, 384), (1000, 999, 384)):
        ref = torch.randn(n1, d, generator=g).to(dev)
        cur = (torch.randn(n2, d, generator=g) + 0.05).to(dev)
        print(f"reference {n1} x {d}, window {n2} x {d}")
        det = drift.KSDriftDetector()
        det.set_reference(ref)
        row("KSDriftDetector.detect_device", device_us(lambda: det.detect_device(cur), args.calls, args.rounds))
        row("KSDriftDetector.detect (one host copy)", host_us(lambda: det.detect(cur), args.calls, args.rounds))
        cs = torch.empty(d, n2, device=dev)
        h = torch.empty(d, dtype=torch.int32, device=dev)
        stat = torch.empty(d, dtype=torch.float64, device=dev)
        p = torch.empty(d, dtype=torch.float64, device=dev)
        row("  nvq_sort_columns (window)", device_us(lambda: _nvq.sort_columns(cur, None, cs), args.calls, args.rounds))
        row("  nvq_ks_statistic", device_us(lambda: _nvq.ks_statistic(det._ref_sorted, cs, h, stat), args.calls, args.rounds))
        row("  nvq_ks_pvalue", device_us(lambda: _nvq.ks_pvalue(h, n1, n2, p), args.calls, args.rounds))
        r = det.detect(cur)
        print(f"    score {r.score:.12g}, h in [{int(h.min())}, {int(h.max())}]")
        if have_scipy:
            row("scipy route: two device-to-host copies + ks_2samp per feature", host_us(lambda: scipy_route(ref, cur), 1, 3))
            want = scipy_route(ref, cur)
            print(f"    score {want:.12g} (scipy), {abs(r.score - want) / want:.2e} relative apart")
        else:
            print("    scipy is not importable here: no host route timed")


if __name__ == "__main__":
    main()
