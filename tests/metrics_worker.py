"""Rank body of tests/test_metrics_gpu.py::test_quality_meter_two_ranks (launched with torch.distributed.run, 2 ranks sharing
the one GPU of the box, gloo as the transport because RCCL refuses two ranks on one device).  Each rank feeds its shard of the
data to a QualityMeter in two unequal batches, calls all_reduce once and saves what compute() returns."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SHARDS = ((0, 3), (3, 8))


def data():
    g = torch.Generator().manual_seed(21)
    y = torch.rand(8, 3, 36, 52, generator=g)
    x = (y + 0.05 * torch.randn(y.shape, generator=g)).clamp(0, 1)
    return x, y


def main():
    out_path = sys.argv[1]
    from nerve_cl import metrics, parallel
    rank, world, _ = parallel.init_from_env("gloo")
    assert world == 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    x, y = data()
    lo, hi = SHARDS[rank]
    x, y = x[lo:hi].to(dev), y[lo:hi].to(dev)
    m = metrics.QualityMeter()
    m.update(x[:1], y[:1])
    m.update(x[1:], y[1:])
    m.all_reduce()
    res = m.compute()
    torch.cuda.synchronize()
    torch.save(res, out_path + f".{rank}")
    parallel.barrier()


if __name__ == "__main__":
    main()
