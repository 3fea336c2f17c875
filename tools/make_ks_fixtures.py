#!/usr/bin/env python3
"""Writes tests/golden/ks_*.npz: fixed-seed float32 inputs and what the reference's mlops/drift/detector.py answers on them with
method="ks" (scipy.stats.ks_2samp per feature, Bonferroni-corrected minimum).

    python tools/make_ks_fixtures.py --reference /path/to/reference/checkout

The reference module is loaded by path and only here; it needs scipy, which no test and no part of nerve_cl imports: the tests
read the recorded numbers.  The detector gets the float64 widening of the stored float32 inputs (what nerve_cl.drift computes
on).  Next to the reference's p_values, score and decision the file holds scipy's per-feature two-sided statistic, which the
reference computes and drops.  A fixture whose reference score lies within 20 % of the threshold is refused (the tests assert the
decision of every fixture), and so is a file larger than the largest existing non-drift fixture."""
import argparse
import os

import numpy as np
from scipy import stats

from make_drift_fixtures import GOLDEN, check_margin, load_reference

THRESHOLD = 0.05

# name -> (reference shape, current shape, mean offset of the current set, rounding step or None, seed)
CASES = {
    "same_64v64x24": ((64, 24), (64, 24), 0.0, None, 21),
    "shift_64v48x24": ((64, 24), (48, 24), 0.75, None, 22),
    "ties_100v37x12": ((100, 12), (37, 12), 0.5, 0.25, 23),
    "clips_48v40x3x8x8": ((48, 3, 8, 8), (40, 3, 8, 8), 1.0, None, 24),
    "window_1000v999x4": ((1000, 4), (999, 4), 0.2, None, 25),
    "same_1000v999x4": ((1000, 4), (999, 4), 0.0, None, 26),
}


def make_inputs(ref_shape, cur_shape, offset, step, seed):
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal(ref_shape)
    cur = rng.standard_normal(cur_shape) + offset
    if step is not None:                                                # ties: multiples of the step, and both signs of zero
        ref, cur = np.round(ref / step) * step, np.round(cur / step) * step
        ref, cur = ref.astype(np.float32), cur.astype(np.float32)
        ref[ref == 0] = np.where(rng.random(int((ref == 0).sum())) < 0.5, -0.0, 0.0)
        cur[cur == 0] = np.where(rng.random(int((cur == 0).sum())) < 0.5, -0.0, 0.0)
        zeros = np.concatenate([ref[ref == 0], cur[cur == 0]])
        if not (np.signbit(zeros).any() and not np.signbit(zeros).all()):
            raise SystemExit("ties case: both signs of zero must be present; choose another seed")
    return ref.astype(np.float32), cur.astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    args = ap.parse_args()
    ref_mod = load_reference(args.reference)
    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith(("drift_", "ks_")))
    for name, (ref_shape, cur_shape, offset, step, seed) in CASES.items():
        ref, cur = make_inputs(ref_shape, cur_shape, offset, step, seed)
        det = ref_mod.DriftDetector(method="ks", threshold=THRESHOLD)
        det.set_reference(ref.astype(np.float64))
        res = det.detect(cur.astype(np.float64))
        check_margin(name, "ks", float(res.score), float(res.threshold))
        r2, c2 = ref.reshape(len(ref), -1).astype(np.float64), cur.reshape(len(cur), -1).astype(np.float64)
        statistic = np.array([stats.ks_2samp(r2[:, i], c2[:, i]).statistic for i in range(r2.shape[1])], dtype=np.float64)
        path = os.path.join(GOLDEN, f"ks_{name}.npz")
        np.savez(path, ref=ref, cur=cur, p_values=np.asarray(res.details["p_values"], dtype=np.float64), statistic=statistic,
                 score=np.float64(res.score), is_drift=np.bool_(res.is_drift), threshold=np.float64(res.threshold))
        size = os.path.getsize(path)
        if size > limit:
            raise SystemExit(f"{path}: {size} bytes, more than the largest existing fixture ({limit})")
        print(f"{name:22s} score {float(res.score):.6g} drift {bool(res.is_drift)} min p {min(res.details['p_values']):.3g} {size} bytes")


if __name__ == "__main__":
    main()
