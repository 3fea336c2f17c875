"""Time a FrameRecoveryNet training step (forward + MSE + backward) at the cfg4 geometry - base 64, 8 clips of 270 x 480, four
reference frames, the 25 % mask of bench.py --recovery, bf16 math and activations as bench.py runs it - without and with
the gradient of the three image inputs (corrupted frame, reference frames, mask), alternating the two variants.  Also
prints the bytes and FLOPs the three input-gradient kernels need at this geometry.
usage: python tools/fr_input_grad_probe.py [--iters 10] [--rounds 3] [--math bf16|f32]
Under rocprofv3 --kernel-trace --stats the kernel times come from the trace (stem7_dgrad_kernel, mask_blend_bwd_ex_kernel,
head_dgrad_kernel)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "continual-learning-for-dynamic-video-quality-enhancement_amd"))
from nerve_cl import _nvq  # noqa: E402
from nerve_cl.models import FrameRecoveryNet  # noqa: E402

B, T, H, W, BASE = 8, 4, 270, 480, 64


def cost(math: str):
    """algorithmic bytes / FLOPs of the input-gradient kernels at this geometry (dy / g in the storage type of the step)"""
    act = 2 if math == "bf16" else 4
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    mid = 32                                                   # conv1.spatial width, max(23, 32)
    return {
        "stem7_dgrad": dict(bytes=B * OH * OW * BASE * act + B * H * W * 4 * 4 * 2,          # dy + (r+w of dframe, dmask)
                            flops=2 * B * OH * OW * BASE * 4 * 49),
        "mask_blend_bwd_ex": dict(bytes=B * H * W * 4 * (3 + 3 + 4 + 1 + 4 + 3 + 1),        # dout frame rec m | drec dframe dm
                                  flops=B * H * W * 3 * 5),
        "head_dgrad (refs)": dict(bytes=B * T * H * W * mid * act + B * T * 3 * H * W * 4,
                                  flops=2 * B * T * H * W * mid * 3 * 9),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--math", choices=["bf16", "f32"], default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = FrameRecoveryNet(3, BASE, 2).to(dev).train()
    net.math_mode = _nvq.MATH_BF16 if args.math == "bf16" else _nvq.MATH_F32
    net.bf16_activations = args.math == "bf16"
    g = torch.Generator(device=dev).manual_seed(1234)
    frame = torch.rand(B, 3, H, W, device=dev, generator=g)
    refs = torch.rand(B, T, 3, H, W, device=dev, generator=g)
    tgt = torch.rand(B, 3, H, W, device=dev, generator=g)
    mask = torch.zeros(B, 1, H, W, device=dev)
    mask[:, :, H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 1.0

    def step(want: bool):
        net.zero_grad(set_to_none=True)
        xs = [t.detach().requires_grad_(want) for t in (frame, refs, mask)]
        torch.nn.functional.mse_loss(net(*xs), tgt).backward()

    times = {False: [], True: []}
    for want in (False, True):
        step(want)
    for _ in range(args.rounds):
        for want in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step(want)
            torch.cuda.synchronize()
            times[want].append((time.perf_counter() - t0) / args.iters * 1e3)
    print(f"FrameRecoveryNet train step, base {BASE}, {B} x {H} x {W}, T {T}, math {args.math} (ms / step, {args.rounds} "
          f"alternating rounds of {args.iters}):")
    for want in (False, True):
        label = "with input gradients   " if want else "without input gradients"
        print(f"  {label}: " + ", ".join(f"{t:.2f}" for t in times[want]) + f"  (min {min(times[want]):.2f})")
    print("input-gradient kernels, algorithmic cost at this geometry:")
    for name, c in cost(args.math).items():
        print(f"  {name}: {c['bytes'] / 1e6:.1f} MB, {c['flops'] / 1e9:.2f} GFLOP")


if __name__ == "__main__":
    main()
