"""Time a FrameRecoveryNet training step (forward + MSE + backward) with parts of the network frozen (requires_grad False), at the
cfg4 geometry - base 64, 8 clips of 270 x 480, four reference frames, the 25 % mask of bench.py --recovery, bf16 math and
activations as bench.py runs it.  The patterns are alternated on one box, round by round.
usage: python tools/fr_frozen_probe.py [--iters 10] [--rounds 3] [--math bf16|f32] [--patterns all,enc_frozen,...]
A tree without frozen-layer support runs only `all` and `all_frozen_inputs` (the others fail there).
Under rocprofv3 --kernel-trace --stats, --patterns enc_frozen --rounds 1 gives the kernels of that pattern alone."""
import argparse
import os
import re
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "continual-learning-for-dynamic-video-quality-enhancement_amd"))
from nerve_cl import _nvq  # noqa: E402
from nerve_cl.models import FrameRecoveryNet  # noqa: E402

B, T, H, W, BASE = 8, 4, 270, 480, 64
# the BatchNorm affines: stem.1, the stage-entry '.1', ResidualBlock conv1.bn / conv2.2, TemporalConv3D spatial.1 / temporal.1,
# decoder upK.1
BN = re.compile(r"(\.stem\.1|\.stage\d\.0\.1|\.conv1\.bn|\.conv2\.2|\.spatial\.1|\.temporal\.1|\.up\d\.1)\.(weight|bias)$")

PATTERNS = {
    # name: (frozen-parameter predicate, train mode, image inputs need a gradient, description)
    "all": (lambda n: False, True, False, "all trainable"),
    "enc_frozen": (lambda n: n.startswith(("spatial_encoder.", "temporal_encoder.")), True, False,
                   "spatial_encoder + temporal_encoder frozen"),
    "decoder_only": (lambda n: not n.startswith("decoder."), True, False, "only decoder.* trained"),
    "decoder_frozen": (lambda n: n.startswith("decoder."), True, False, "decoder.* frozen, encoders + fusion trained"),
    "bn_affine": (lambda n: BN.search(n) is not None, True, False, "BatchNorm affine frozen"),
    "final_only_eval": (lambda n: not n.startswith("decoder.final."), False, False, "only decoder.final.* trained, eval mode"),
    "all_frozen_inputs": (lambda n: True, True, True, "all frozen, frame / refs / mask gradients"),
    # (not run by default) the one-pass eval BatchNorm backward of a frozen decoder against the all-trainable eval step
    "all_eval": (lambda n: False, False, False, "all trainable, eval mode"),
    "decoder_frozen_eval": (lambda n: n.startswith("decoder."), False, False, "decoder.* frozen, eval mode"),
}
DEFAULT = ("all", "enc_frozen", "decoder_only", "decoder_frozen", "bn_affine", "final_only_eval", "all_frozen_inputs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--math", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--patterns", default=",".join(DEFAULT))
    args = ap.parse_args()
    names = args.patterns.split(",")
    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = FrameRecoveryNet(3, BASE, 2).to(dev)
    net.math_mode = _nvq.MATH_BF16 if args.math == "bf16" else _nvq.MATH_F32
    net.bf16_activations = args.math == "bf16"
    g = torch.Generator(device=dev).manual_seed(1234)
    frame = torch.rand(B, 3, H, W, device=dev, generator=g)
    refs = torch.rand(B, T, 3, H, W, device=dev, generator=g)
    tgt = torch.rand(B, 3, H, W, device=dev, generator=g)
    mask = torch.zeros(B, 1, H, W, device=dev)
    mask[:, :, H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 1.0

    def setup(name):
        frozen, train, _, _ = PATTERNS[name]
        net.train(train)
        for n, p in net.named_parameters():
            p.requires_grad_(not frozen(n))

    def step(name):
        want = PATTERNS[name][2]
        net.zero_grad(set_to_none=True)
        xs = [t.detach().requires_grad_(want) for t in (frame, refs, mask)]
        torch.nn.functional.mse_loss(net(*xs), tgt).backward()

    times = {n: [] for n in names}
    for n in names:
        setup(n)
        step(n)
    for _ in range(args.rounds):
        for n in names:
            setup(n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step(n)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / args.iters * 1e3)
    print(f"FrameRecoveryNet step, base {BASE}, {B} x {H} x {W}, T {T}, math {args.math} (ms / step, {args.rounds} alternating "
          f"rounds of {args.iters}):")
    for n in names:
        frozen = PATTERNS[n][0]
        nfrozen = sum(p.numel() for k, p in net.named_parameters() if frozen(k))
        print(f"  {n:19s} {PATTERNS[n][3]:46s} " + " ".join(f"{t:7.2f}" for t in times[n]) + f"  (min {min(times[n]):.2f}; "
              f"{nfrozen / sum(p.numel() for p in net.parameters()) * 100:.1f} % of the parameters frozen)")


if __name__ == "__main__":
    main()
