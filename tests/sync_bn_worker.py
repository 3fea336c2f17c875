"""Rank body of tests/test_sync_bn_gpu.py (launched with torch.distributed.run, 2 ranks sharing the one GPU of the box, gloo
as the transport because RCCL refuses two ranks on one device).  Every case converts its network with
enable_data_parallel(sync_bn=True), runs one training step on this rank's shard and saves what the parent compares with a
single process over the concatenated batch."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WORLD = 2
CASES = ("sr_f32", "sr_bf16", "light", "fr", "unequal", "late")


def make_net(case: str):
    """the unconverted network of a case, on the CPU, identical in every process"""
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet, LightweightSuperResolution, SuperResolutionNet
    from oracle import synth
    torch.manual_seed(0)
    if case in ("sr_f32", "unequal", "late"):
        net = SuperResolutionNet(3, 2, 16, 1, 1)
        net.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
        net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    elif case == "sr_bf16":
        # F = 64 in the bf16 mode: the fused dwpw forward / pw_bn backward kernels
        net = SuperResolutionNet(3, 2, 64, 1, 1)
        net.math_mode, net.bf16_activations = _nvq.MATH_BF16, True
    elif case == "light":
        net = LightweightSuperResolution(2)
        net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    else:
        net = FrameRecoveryNet(3, 16, 2)
        net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    net.use_hip_graphs = False
    return net


def shard_sizes(case: str):
    return (1, 2) if case == "unequal" else (2, 2)


def data(case: str):
    """(inputs, target) of the global batch; rank 1's shard is scaled and offset, so that per-rank statistics are far off"""
    g = torch.Generator().manual_seed(7)
    n0, n1 = shard_sizes(case)
    n = n0 + n1
    if case == "fr":
        H = W = 32
        frame = torch.rand(n, 3, H, W, generator=g)
        refs = torch.rand(n, 2, 3, H, W, generator=g)
        frame[n0:] = frame[n0:] * 3.0 + 0.5
        refs[n0:] = refs[n0:] * 3.0 + 0.5
        mask = (torch.rand(n, 1, H, W, generator=g) > 0.3).float()      # corrupted pixels: the recovered frame is blended in there
        return (frame, refs, mask), torch.rand(n, 3, H, W, generator=g)
    H, W = 16, 24
    if case == "light":
        x = torch.rand(n, 3, H, W, generator=g)
    else:
        x = torch.rand(n, 3, 3, H, W, generator=g)
    x[n0:] = x[n0:] * 3.0 + 0.5
    return (x,), torch.rand(n, 3, 2 * H, 2 * W, generator=g)


def run(net, inputs):
    """forward of a case's network on (already on-device) inputs"""
    return net(*inputs)


def bn_state(net):
    return {n: t.detach().clone().cpu() for n, t in net.state_dict().items()
            if n.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def main():
    out_path = sys.argv[1]
    from nerve_cl import parallel
    rank, world, _ = parallel.init_from_env("gloo")
    assert world == WORLD
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {}
    for case in CASES:
        net = make_net(case).to(dev)
        n0, n1 = shard_sizes(case)
        lo, hi = (0, n0) if rank == 0 else (n0, n0 + n1)
        inputs, tgt = data(case)
        xs = [t[lo:hi].to(dev).requires_grad_(case != "unequal") for t in inputs]
        y = tgt[lo:hi].to(dev)
        if case == "late":
            # a first (eval-mode) forward builds the engine's caches; the conversion afterwards must still be noticed
            net.eval()
            with torch.no_grad():
                run(net, xs)
        net = parallel.enable_data_parallel(net, sync_bn=True)
        assert sum(isinstance(m, torch.nn.SyncBatchNorm) for m in net.modules()) > 0
        net.train()
        r = {}
        if case == "unequal":
            with torch.no_grad():
                out = run(net, xs)
        else:
            out = run(net, xs)
            F.mse_loss(out, y).backward()
            r["bucket"] = net._last_grad_bucket.detach().cpu()
            r["dx"] = xs[0].grad.detach().cpu()
        r["out"] = out.detach().cpu()
        r["bn"] = bn_state(net)
        res[case] = r
        torch.cuda.synchronize()
    torch.save(res, out_path + f".{rank}")
    parallel.barrier()


if __name__ == "__main__":
    main()
