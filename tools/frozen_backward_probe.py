"""Time a SuperResolutionNet training step (forward + MSE + backward) for the freeze patterns of DESIGN.md section 13, at cfg2
(540 x 960, 8 clips, F 64, 8 blocks, T 3, bf16 math and activations as bench.py runs it) and at a 64 x 64 cfg5-like step
(8 clips, same net).  Per pattern: wall time per step (synchronised host timer, alternating rounds) and, from one step under
the kernel timer of bench.py, the timed kernel time split into weight-gradient kernels (wgrad_*) and the rest.
--pkg DIR imports nerve_cl from another tree (e.g. the parent commit's) so that the same patterns can be timed there.
usage: python tools/frozen_backward_probe.py [--iters 5] [--rounds 2] [--sizes cfg2,small] [--pkg DIR]"""
import argparse
import os
import re
import sys
import time

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

PATTERNS = {
    # name: (frozen-parameter predicate, frames need a gradient)
    "P1 all trainable": (lambda n: False, False),
    "P2 extractor+motion frozen": (lambda n: n.startswith(("feature_extractor.", "motion_estimator.")), False),
    "P3 only gff+upsampler": (lambda n: not n.startswith(("gff.", "upsampler.")), False),
    "P4 all frozen, frames grad": (lambda n: True, True),
    "P5 residual blocks frozen": (lambda n: n.startswith("residual_blocks."), False),
    "P6 extractor BN affine frozen": (lambda n: re.match(r"feature_extractor\.body\.\d\.bn\.", n) is not None, False),
}
SIZES = {"cfg2": (8, 540, 960), "small": (8, 64, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", default="cfg2,small")
    ap.add_argument("--pkg", default=os.path.join(HERE, "..", "continual-learning-for-dynamic-video-quality-enhancement_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda")
    print(f"tree: {os.path.abspath(args.pkg)}")
    for size in args.sizes.split(","):
        B, H, W = SIZES[size]
        torch.manual_seed(0)
        net = SuperResolutionNet(3, 2, 64, 8, 1).to(dev).train()
        net.math_mode, net.bf16_activations = _nvq.MATH_BF16, True
        g = torch.Generator(device=dev).manual_seed(1234)
        x = torch.rand(B, 3, 3, H, W, device=dev, generator=g)
        tgt = torch.rand(B, 3, 2 * H, 2 * W, device=dev, generator=g)

        def step(pattern):
            frozen, frames_grad = PATTERNS[pattern]
            for n, p in net.named_parameters():
                p.requires_grad_(not frozen(n))
                p.grad = None
            F.mse_loss(net(x.detach().requires_grad_(frames_grad)), tgt).backward()

        for p in PATTERNS:
            step(p)
        times = {p: [] for p in PATTERNS}
        for _ in range(args.rounds):
            for p in PATTERNS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    step(p)
                torch.cuda.synchronize()
                times[p].append((time.perf_counter() - t0) / args.iters * 1e3)
        split = {}
        for p in PATTERNS:
            _nvq.TIMER = _nvq.KernelTimer()
            step(p)
            torch.cuda.synchronize()
            s = _nvq.TIMER.summary()
            _nvq.TIMER = None
            tot = sum(d["ms_total"] for d in s.values())
            wg = sum(d["ms_total"] for k, d in s.items() if k.startswith("wgrad"))
            split[p] = (tot, wg, sum(d["launches"] for d in s.values()))
        print(f"\n{size}: {B} x {H} x {W}, T 3, F 64, 8 blocks, bf16 (ms / step, {args.rounds} alternating rounds of {args.iters}; "
              f"timed kernels of one step)")
        print(f"  {'pattern':32s} {'step ms (min)':>14s}  rounds          {'timed ms':>9s} {'wgrad ms':>9s} {'launches':>8s}")
        for p in PATTERNS:
            tot, wg, n = split[p]
            print(f"  {p:32s} {min(times[p]):14.2f}  " + " ".join(f"{t:7.2f}" for t in times[p]) +
                  f"  {tot:9.2f} {wg:9.2f} {n:8d}")


if __name__ == "__main__":
    main()
