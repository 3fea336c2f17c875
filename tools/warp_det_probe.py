"""Time the overwrite-mode warp backward in its two forms - the atomic one (nvq_warp_backward: far sources scattered with float
atomics) and the deterministic one (nvq_warp_backward_ex, NVQ_WARP_DETERMINISTIC: far sources binned and gathered) - at the
cfg2 shape 8 x 540 x 960 x 64 (bf16 feat and dout, as the bf16 step stores them) for fp32 and bf16 dfeat, on four motion
fields: no far source (~1 px), 20 % of the sources 5 - 8 px away, 60 % up to 30 px away, and a contracting far flow (every
16 x 16 block collapsed onto one point 6 px beyond its centre).  Also reports the largest |difference| between the forms.
usage: python tools/warp_det_probe.py [--iters 10] [--out FILE]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "continual-learning-for-dynamic-video-quality-enhancement_amd"))
from nerve_cl import _nvq as K  # noqa: E402
from dwpw_probe import timed  # noqa: E402

N, H, W, C = 8, 540, 960, 64


def flows(dev):
    g = torch.Generator(device=dev).manual_seed(3)
    base = torch.randn(N, H, W, 4, device=dev, generator=g) * 0.5
    out = {"0 % far (~1 px)": torch.randn(N, H, W, 4, device=dev, generator=g) * 1.2}
    for name, frac, rmin, rmax in (("20 % far (5-8 px)", 0.2, 5.0, 8.0), ("60 % far (4.5-30 px)", 0.6, 4.5, 30.0)):
        far = torch.rand(N, H, W, 1, device=dev, generator=g) < frac
        ang = torch.rand(N, H, W, 1, device=dev, generator=g) * 2 * math.pi
        r = rmin + (rmax - rmin) * torch.rand(N, H, W, 1, device=dev, generator=g)
        f = base.clone()
        f[..., 0:1] += torch.where(far, r * torch.cos(ang), torch.zeros((), device=dev))
        f[..., 1:2] += torch.where(far, r * torch.sin(ang), torch.zeros((), device=dev))
        out[name] = f
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    f = base.clone() * 0.01
    f[..., 0] += (torch.div(xs, 16, rounding_mode="floor") * 16 + 8 + 6.3) - xs
    f[..., 1] += (torch.div(ys, 16, rounding_mode="floor") * 16 + 8 + 6.6) - ys
    out["contracting far (16x16 -> 1 point)"] = f
    return out


def far_fraction(f):
    ys = torch.arange(H, device=f.device, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=f.device, dtype=torch.float32).view(1, 1, W)
    ox = torch.floor(xs + f[..., 0]) - xs
    oy = torch.floor(ys + f[..., 1]) - ys
    return ((ox < -4) | (ox > 3) | (oy < -4) | (oy > 3)).float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    feat = torch.randn(N, H, W, C, device=dev).bfloat16()
    dout = torch.randn(N, H, W, 3 * C, device=dev).bfloat16()
    dflow = torch.empty(N, H, W, 4, device=dev)
    lines = [f"warp backward, overwrite mode, {N} x {H} x {W} x {C}, bf16 feat / dout; ms per call (mean of {a.iters}, "
             "records and workspace from the caching allocator)",
             f"{'motion field':38s} {'far':>6s} {'dfeat':>6s} {'atomic':>8s} {'determ.':>8s} {'ratio':>6s} {'max|diff|':>10s}"]
    for name, fl in flows(dev).items():
        frac = far_fraction(fl)
        for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            d0 = torch.empty(N, H, W, C, device=dev, dtype=dt)
            d1 = torch.empty(N, H, W, C, device=dev, dtype=dt)
            ms0 = timed(lambda: K.warp_backward(K.Sl(dout, C, 2 * C), K.Sl(feat), fl, K.Sl(d0), dflow, overwrite=True), a.iters)
            ms1 = timed(lambda: K.warp_backward(K.Sl(dout, C, 2 * C), K.Sl(feat), fl, K.Sl(d1), dflow, overwrite=True,
                                                deterministic=True), a.iters)
            diff = (d0.float() - d1.float()).abs().max().item()
            lines.append(f"{name:38s} {frac * 100:5.1f}% {dname:>6s} {ms0:8.3f} {ms1:8.3f} {ms1 / ms0:6.2f} {diff:10.3e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
