#!/usr/bin/env python3
"""Writes tests/golden/drift_*.npz: fixed-seed float32 inputs and what the reference's mlops/drift/detector.py answers on them.

    python tools/make_drift_fixtures.py --reference /path/to/reference/checkout

The reference module is loaded by path and only here: no test imports it, the tests read the recorded numbers.  Its detector
is numpy on whatever dtype it is handed, so it gets the float64 widening of the stored float32 inputs (what nerve_cl.drift
computes on).  Only equal-sized sets of at most 500 rows are recorded: there the reference's subsample is a permutation of both
sets and cannot move the score beyond rounding.  A fixture whose reference score lies within 20 % of its threshold is refused
(the tests assert the decision of every fixture).  Without scipy the reference's import of scipy.stats is satisfied by an empty
stand-in: only its KS path, which is not recorded, uses it."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
MARGIN = 0.2

# name -> (sample shape, mean offset of the current set, seed)
CASES = {
    "same_64x384": ((64, 384), 0.0, 11),
    "shift_64x384": ((64, 384), 0.75, 12),
    "same_clips_48x3x8x8": ((48, 3, 8, 8), 0.0, 13),
    "shift_clips_48x3x8x8": ((48, 3, 8, 8), 1.0, 14),
    "shift_100x48": ((100, 48), 1.0, 15),
}
# the performance monitor: baseline, threshold, window and a metric sequence that crosses the threshold and recovers; the
# values are multiples of 1/8, exact in fp32
MONITOR = dict(baseline=32.0, threshold=0.1, window=4,
               metrics=[32.0, 31.5, 31.0, 30.0, 29.0, 28.0, 27.5, 27.0, 26.5, 26.0, 30.0, 32.0, 33.0, 33.5, 34.0])


def load_reference(root: str):
    try:
        import scipy.stats  # noqa: F401
    except ImportError:
        scipy = types.ModuleType("scipy")
        scipy.stats = types.ModuleType("scipy.stats")
        sys.modules.setdefault("scipy", scipy)
        sys.modules.setdefault("scipy.stats", scipy.stats)
    path = os.path.join(root, "mlops", "drift", "detector.py")
    spec = importlib.util.spec_from_file_location("reference_drift_detector", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod                 # dataclasses looks the module up while the class is built
    spec.loader.exec_module(mod)
    return mod


def check_margin(name: str, method: str, score: float, threshold: float) -> None:
    if abs(score - threshold) < MARGIN * threshold:
        raise SystemExit(f"{name}: reference {method} score {score:.6g} is within {MARGIN:.0%} of its threshold {threshold}: "
                         "choose another offset")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    args = ap.parse_args()
    ref_mod = load_reference(args.reference)
    os.makedirs(GOLDEN, exist_ok=True)
    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("drift_"))
    for name, (shape, offset, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        ref = rng.standard_normal(shape).astype(np.float32)
        cur = (rng.standard_normal(shape) + offset).astype(np.float32)
        out = {"ref": ref, "cur": cur, "offset": np.float64(offset)}
        for method in ("mmd", "psi"):
            det = ref_mod.DriftDetector(method=method, threshold=0.05)
            det.set_reference(ref.astype(np.float64))
            np.random.seed(seed)                                        # the reference draws its permutation from the global RNG
            res = det.detect(cur.astype(np.float64))
            check_margin(name, method, float(res.score), float(res.threshold))
            out[f"{method}_score"] = np.float64(res.score)
            out[f"{method}_drift"] = np.bool_(res.is_drift)
            out[f"{method}_threshold"] = np.float64(res.threshold)
            print(f"{name:24s} {method}: score {float(res.score):.6f} drift {bool(res.is_drift)}")
        path = os.path.join(GOLDEN, f"drift_{name}.npz")
        np.savez(path, **out)
        if os.path.getsize(path) > limit:
            raise SystemExit(f"{path}: {os.path.getsize(path)} bytes, more than the largest existing fixture ({limit})")
    mon = ref_mod.ModelDriftMonitor(metric_threshold=MONITOR["threshold"], window_size=MONITOR["window"])
    mon.set_baseline(MONITOR["baseline"])
    flags = [bool(mon.update(m)) for m in MONITOR["metrics"]]
    if not (any(flags) and not all(flags) and not flags[-1]):
        raise SystemExit("monitor sequence does not cross the threshold and recover")
    np.savez(os.path.join(GOLDEN, "drift_monitor.npz"), baseline=np.float64(MONITOR["baseline"]),
             threshold=np.float64(MONITOR["threshold"]), window=np.int64(MONITOR["window"]),
             metrics=np.asarray(MONITOR["metrics"], dtype=np.float64), flags=np.asarray(flags))
    print("monitor flags:", "".join("1" if f else "0" for f in flags))


if __name__ == "__main__":
    main()
