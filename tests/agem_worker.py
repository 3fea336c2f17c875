"""Rank body of tests/test_agem_gpu.py::test_two_ranks_project_to_the_same_gradient (launched with torch.distributed.run, 2 ranks
sharing the one GPU of the box, gloo as the transport because RCCL refuses two ranks on one device).  Drives the PRODUCT path:
enable_data_parallel -> a reference gradient on this rank's shard -> a conflicting step -> AGEM.project()."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B_PER_RANK, H, W = 2, 16, 24


def make_engine():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    return eng


def data(world: int):
    from oracle import synth
    n = B_PER_RANK * world
    return synth.formula_clip(n, 3, H, W), synth.formula_target(n, 2 * H, 2 * W)


def loss(eng, x, y, sign):
    """+1: the loss L whose gradient is the reference; -1: -L plus half of another loss - conflicting, but not simply -r"""
    out = eng(x)["enhanced"]
    if sign > 0:
        return F.mse_loss(out, y)
    return -F.mse_loss(out, y) + 0.5 * F.mse_loss(out, 0.5 * y.flip(0))


def main():
    out_path = sys.argv[1]
    from nerve_cl import parallel
    from nerve_cl.continual import AGEM
    rank, world, local = parallel.init_from_env("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = make_engine().to(dev)
    if rank == 1:                                   # replicas start different; enable_data_parallel must fix that
        with torch.no_grad():
            for p in eng.parameters():
                p.mul_(1.5)
    parallel.enable_data_parallel(eng)
    x, y = data(world)
    mine = slice(B_PER_RANK * rank, B_PER_RANK * (rank + 1))
    xs, ys = x[mine].to(dev), y[mine].to(dev)
    agem = AGEM(eng)
    eng.train()
    eng.zero_grad()
    loss(eng, xs, ys, +1.0).backward()              # the bucket hook leaves the rank mean: the same r on both ranks
    agem.capture_reference()
    eng.zero_grad()
    loss(eng, xs, ys, -1.0).backward()
    agem.project()
    grads = torch.cat([p.grad.reshape(-1) for p in eng.super_resolution.parameters()]).cpu()
    gathered = [torch.empty_like(grads) for _ in range(world)]
    torch.distributed.all_gather(gathered, grads)
    counts = [None] * world
    torch.distributed.all_gather_object(counts, agem.num_projections())
    # a loose parameter that carries a gradient is refused: nothing synchronises it over the ranks
    eng.enhancement_strength.grad = torch.ones_like(eng.enhancement_strength)
    try:
        agem.project()
        refused = False
    except RuntimeError as e:
        refused = "enhancement_strength" in str(e)
    assert refused
    if rank == 0:
        torch.save({"grads_rank0": gathered[0], "grads_rank1": gathered[1], "projections": counts}, out_path)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
