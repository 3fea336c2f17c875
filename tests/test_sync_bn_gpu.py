"""nn.SyncBatchNorm through the HIP networks: two ranks share the box's one GPU (gloo transport; RCCL wants one device per
rank), convert their networks with enable_data_parallel(sync_bn=True) and run tests/sync_bn_worker.py.  The parent runs the
unconverted network in one process over the concatenated batch: the synchronised step must reproduce it (gradient bucket,
every BatchNorm's running statistics, the rank's output slice, W times the rank's slice of the frames' gradient), and the
per-rank-statistics step (plain data parallelism) must miss it by far, so that the comparison discriminates."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sync_bn_worker as W  # noqa: E402

# fp32 cases: the tolerance of tests/test_dp_gpu.py.  bf16 case: activations are stored as bf16, and a statistic that differs
# in its last fp32 bit (sums added in another order) can move a stored activation by one bf16 step (2^-8 relative).
TOL = {"sr_f32": 1e-5, "sr_bf16": 2e-3, "light": 1e-5, "fr": 1e-5, "unequal": 1e-5, "late": 1e-5}


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("syncbn") / "res.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    # children are ordinary child processes of a launcher that never touches the GPU
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(HERE, "sync_bn_worker.py"), out], env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [torch.load(out + f".{k}", weights_only=True) for k in range(W.WORLD)]


def _single(case: str, rows=None, backward: bool = True):
    """the unconverted network in one process over the global batch (rows: a slice of it = one rank's plain-DP step)"""
    dev = torch.device("cuda", 0)
    net = W.make_net(case).to(dev).train()
    inputs, tgt = W.data(case)
    if rows is not None:
        inputs, tgt = [t[rows] for t in inputs], tgt[rows]
    xs = [t.to(dev).requires_grad_(backward) for t in inputs]
    if not backward:
        with torch.no_grad():
            out = W.run(net, xs)
        return {"out": out.cpu(), "bn": W.bn_state(net)}
    out = W.run(net, xs)
    F.mse_loss(out, tgt.to(dev)).backward()
    return {"out": out.detach().cpu(), "bn": W.bn_state(net), "bucket": net._last_grad_bucket.cpu(), "dx": xs[0].grad.cpu()}


def _check_bn(case, got, ref, tol):
    assert set(got[0]["bn"]) == set(ref["bn"]) and len(ref["bn"]) > 0
    for n, want in ref["bn"].items():
        a, b = got[0]["bn"][n], got[1]["bn"][n]
        assert torch.equal(a, b), f"{case}: {n} differs between the ranks"
        if n.endswith("num_batches_tracked"):
            assert torch.equal(a, want), (case, n, a, want)
        else:
            assert _rel(a, want) <= tol, f"{case}: {n} off by {_rel(a, want):.3e}"


def _bounds(case, r):
    n0, n1 = W.shard_sizes(case)
    return (0, n0) if r == 0 else (n0, n0 + n1)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["sr_f32", "sr_bf16", "light", "fr", "late"])
def test_sync_bn_step_matches_single_process(ranks, case):
    tol = TOL[case]
    got = [ranks[r][case] for r in range(W.WORLD)]
    ref = _single(case)
    # the gradient bucket (after the bucket all-reduce, identical on the ranks)
    for r in range(W.WORLD):
        e = _rel(got[r]["bucket"], ref["bucket"])
        assert e <= tol, f"{case}: rank {r} bucket off by {e:.3e}"
    _check_bn(case, got, ref, tol)
    for r in range(W.WORLD):
        lo, hi = _bounds(case, r)
        e = _rel(got[r]["out"], ref["out"][lo:hi])
        assert e <= tol, f"{case}: rank {r} output off by {e:.3e}"
        # the frames' gradient stays per rank: the gradient of the sum of the ranks' losses = W x the global-batch mean loss
        e = _rel(got[r]["dx"], W.WORLD * ref["dx"][lo:hi])
        assert e <= tol, f"{case}: rank {r} frames' gradient off by {e:.3e}"
    # plain data parallelism (each rank normalises with its own shard's statistics) misses the target by far
    local = [_single(case, slice(*_bounds(case, r))) for r in range(W.WORLD)]
    miss = _rel((local[0]["bucket"] + local[1]["bucket"]) / 2, ref["bucket"])
    assert miss > 100 * tol, f"{case}: the per-rank-statistics step is only {miss:.3e} off: the test does not discriminate"


@pytest.mark.timeout(900)
def test_sync_bn_unequal_shards_global_count(ranks):
    """rank 0 holds 1 clip, rank 1 holds 2: the count is global too (running statistics use the global unbiased variance)"""
    case = "unequal"
    tol = TOL[case]
    got = [ranks[r][case] for r in range(W.WORLD)]
    ref = _single(case, backward=False)
    _check_bn(case, got, ref, tol)
    for r in range(W.WORLD):
        lo, hi = _bounds(case, r)
        assert _rel(got[r]["out"], ref["out"][lo:hi]) <= tol
    # as if every rank had counted only its own pixels (or the ranks had the same count): far off
    local = _single(case, slice(0, 1), backward=False)
    name = next(n for n in ref["bn"] if n.endswith("running_var"))
    assert _rel(local["bn"][name], ref["bn"][name]) > 100 * tol
