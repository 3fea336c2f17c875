"""`bench.py --dump-outputs DIR`: what the last timed step computed, as DIR/<name>.npy.

CPU part: dump_outputs() writes float32 arrays (float64 for a 0-d one), keeps the total within DUMP_BYTES and samples a large
array at the same positions every time.  GPU part (`-m gpu`): two runs of a tiny benchmark with the same arguments dump the
same output, loss and gradients (to float rounding), and the result line reports the requested number of timed steps and
ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bench_launch import REPO, _load_bench


def test_dump_writes_float_arrays_within_the_budget(tmp_path):
    bench = _load_bench()
    g = torch.Generator().manual_seed(0)
    big = torch.rand(bench.DUMP_BYTES // 4 + 12345, generator=g)          # alone larger than the whole budget
    small = torch.rand(3, 5, generator=g, dtype=torch.float64)
    half = torch.rand(7, generator=g).to(torch.bfloat16)
    arrays = {"big": big, "small": small, "half": half, "loss": torch.tensor(0.25)}
    n = bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert sum(a.nbytes for a in got.values()) == n <= bench.DUMP_BYTES
    assert got["loss"].dtype == np.float64 and got["loss"].shape == () and got["loss"] == 0.25
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], small.float().numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], half.float().numpy())
    assert got["big"].dtype == np.float32 and got["big"].ndim == 1 and got["big"].size < big.numel()
    assert np.isin(got["big"], big.numpy()).all()                           # a sample of the elements, not something else
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), got["big"])  # the same positions on every run


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_runs_with_the_same_arguments_dump_the_same_results(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    lines, dumps = [], []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch", "2", "--height", "32", "--width", "48", "--features", "16", "--blocks", "1",
                            "--no-cpu-baseline", "--dump-outputs", str(tmp_path / run)],
                           env=env, capture_output=True, text=True, timeout=420)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert abs(line["value"] - 2 * 1000.0 / line["ms_per_step"]) <= 1e-6 * line["value"]
    a, b = dumps
    assert set(a) == set(b) == {"output", "loss", "grads"}
    assert a["output"].shape == (2, 3, 64, 96) and a["output"].dtype == np.float32
    assert a["loss"].dtype == np.float64 and a["loss"] == np.float32(lines[0]["config"]["final_loss"])
    assert a["grads"].dtype == np.float32 and np.isfinite(a["grads"]).all() and np.abs(a["grads"]).max() > 0
    for k in a:                     # same inputs; the warp backward's far-source scatter may add in another order
        assert a[k].shape == b[k].shape and np.abs(a[k] - b[k]).max() <= 1e-4 * np.abs(a[k]).max(), k
