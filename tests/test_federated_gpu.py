"""GPU: csrc/federated.hip (client-update norms, the aggregation pass, per-slot DP clip-and-noise, the Philox normals) against
float64 written here (tests/_federated_oracle.py), then DPOptimizer, FederatedTrainer and experiments/train_federated.py on the
device.

Bounds.  Sums of squares: exact differences and products in double, summed in double: 1e-10 of the sum of the terms (as
tests/test_agem_gpu.py).  Aggregate without noise: the float64 chain is rounded to fp32 once: 1 ulp of the float64 value.  Normals:
fp32 logf / sincospif / sqrtf against float64: 2e-5 absolute per unit of standard deviation.  DP step: the coefficient, the product
and the fma are one fp32 rounding each (2^-24 relative), asserted at 1e-6 |g coef|, plus the noise bound."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _federated_oracle as oracle  # noqa: E402
from test_federated_cpu import GOLDEN, golden_model  # noqa: E402

SECOND_TRIP = (1 << 20) + 1031          # 1024 blocks x 256 threads x one quad = 2^20 floats per trip: a second trip and a tail


def _dev():
    return torch.device("cuda", 0)


def _ws():
    from nerve_cl import _engine
    return _engine.workspace(_dev())


def _matrix(K, n, stride, seed, shift=0, base=True):
    """clients [K][stride] (as a view `shift` floats into its allocation), base [n] or None; values from a seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(K, n, generator=g)
    buf = torch.zeros(shift + K * stride + 4, device=_dev())
    clients = buf[shift:shift + K * stride].view(K, stride)
    clients[:, :n] = vals.to(_dev())
    b = None
    if base:
        bbuf = torch.zeros(shift + n, device=_dev())
        b = bbuf[shift:]
        b.copy_((vals.mean(0) + 0.1 * torch.randn(n, generator=g)).to(_dev()))
    if shift:
        assert clients.data_ptr() % 16 == 4 * shift
    return clients, b


def _sq(clients, n, base):
    from nerve_cl import _nvq
    sq = torch.zeros(clients.shape[0], dtype=torch.float64, device=_dev())
    _nvq.fed_delta_norms(clients, n, base, sq, _ws())
    return sq


def _pad4(n):
    return (n + 3) // 4 * 4


NORM_CASES = [(n, K, padded, has_base) for n in (1, 3, 4, 5, 1023) for K in (1, 2, 5, 64) for padded in (False, True)
              for has_base in (False, True) if (K in (2, 64) or (padded and has_base))]
NORM_CASES += [(SECOND_TRIP, 2, False, True), (SECOND_TRIP, 5, True, False)]


# ------------------------------------------------------------------------------------------------ client-update norms
@pytest.mark.parametrize("n,K,padded,has_base", NORM_CASES)
def test_delta_norms_against_float64(n, K, padded, has_base):
    stride = _pad4(n) if padded else n
    clients, base = _matrix(K, n, stride, 1000 + n % 89 + K, base=has_base)
    sq = _sq(clients, n, base)
    d = clients[:, :n].double() - (base.double() if has_base else 0.0)
    want = (d * d).sum(1)
    assert ((sq - want).abs() <= 1e-10 * want).all(), (sq, want)
    assert torch.equal(sq.view(torch.int64), _sq(clients, n, base).view(torch.int64))          # the same bits on every call
    shifted, sbase = _matrix(K, n, stride, 1000 + n % 89 + K, shift=1, base=has_base)            # only 4-byte aligned
    assert torch.equal(sq.view(torch.int64), _sq(shifted, n, sbase).view(torch.int64))


def test_delta_norms_refuse_a_short_workspace_and_bad_counts():
    from nerve_cl import _nvq
    clients, base = _matrix(2, 5000, 5000, 1)
    sq = torch.zeros(2, dtype=torch.float64, device=_dev())
    assert _nvq.fed_workspace_bytes(2, 5000) == 5 * 2 * 8
    with pytest.raises(RuntimeError, match="workspace"):
        _nvq.fed_delta_norms(clients, 5000, base, sq, torch.zeros(8, device=_dev()))
    rc = _nvq.lib().nvq_fed_delta_norms(clients.data_ptr(), 5000, 65, None, 5000, sq.data_ptr(), _ws().data_ptr(), 1 << 20, None)
    assert rc == -1


# ------------------------------------------------------------------------------------------------ aggregate, no noise
def _aggregate(clients, n, base, weights, sq=None, out=None, **kw):
    from nerve_cl import _nvq
    w = torch.tensor(weights, dtype=torch.float64).to(_dev())
    if out is None:
        out = torch.full((n,), float("nan"), device=_dev())
    _nvq.fed_aggregate(clients, n, base, w, sq, out, **kw)
    return out


def _within_ulps(got, want, ulps=1):
    w32 = want.abs().to(torch.float32)
    ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
    return bool(((got.double() - want).abs() <= ulps * ulp).all())


def _want_aggregate(clients, n, base, weights, clip=None, lr=1.0):
    x = clients[:, :n].double()
    b = base.double() if base is not None else torch.zeros(n, dtype=torch.float64, device=_dev())
    w = torch.tensor(weights, dtype=torch.float64, device=_dev())
    d = x - b
    c = w / w.sum()
    if clip is not None:
        c = c * torch.clamp(clip / (d.pow(2).sum(1).sqrt() + 1e-6), max=1.0)
    return b + lr * (c.view(-1, 1) * d).sum(0)


AGG_CASES = [(n, K, padded) for n in (1, 3, 4, 5, 1023) for K in (1, 2, 5, 64) for padded in (False, True)
             if K in (2, 5) or padded] + [(SECOND_TRIP, 2, False), (SECOND_TRIP, 5, True)]


@pytest.mark.parametrize("n,K,padded", AGG_CASES)
def test_fedavg_and_server_step_within_one_ulp(n, K, padded):
    stride = _pad4(n) if padded else n
    clients, base = _matrix(K, n, stride, 2000 + n % 89 + K)
    weights = [float(3 + (7 * k) % 5) for k in range(K)]
    if K > 1:
        weights[1] = 0.0                                               # a client without samples
    got = _aggregate(clients, n, None, weights)
    assert _within_ulps(got, _want_aggregate(clients, n, None, weights))
    for lr in (1.0, 0.5):
        got = _aggregate(clients, n, base, weights, server_lr=lr)
        assert _within_ulps(got, _want_aggregate(clients, n, base, weights, lr=lr)), lr
    shifted, sbase = _matrix(K, n, stride, 2000 + n % 89 + K, shift=1)
    assert torch.equal(_aggregate(shifted, n, sbase, weights, server_lr=0.5).view(torch.int32), got.view(torch.int32))
    aliased = base.clone()                                             # out may be base
    _aggregate(clients, n, aliased, weights, out=aliased, server_lr=0.5)
    assert torch.equal(aliased.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("n,padded", [(5, False), (1023, True), (1023, False)])
def test_clipped_updates(n, padded):
    stride = _pad4(n) if padded else n
    clients, base = _matrix(3, n, stride, 31)
    with torch.no_grad():
        clients[0, :n] = base + 5.0 * torch.randn(n, device=_dev())     # far above the bound
        clients[1, :n] = base + 1e-3 * torch.randn(n, device=_dev())    # below it
        clients[2, :n] = base                                           # unchanged: norm 0, coefficient 1
    sq = _sq(clients, n, base)
    assert sq[2] == 0 and sq[0].sqrt() > 1.0 > sq[1].sqrt()
    weights = [2.0, 3.0, 4.0]
    for lr in (1.0, 0.5):
        got = _aggregate(clients, n, base, weights, sq=sq, clip_norm=1.0, server_lr=lr)
        assert _within_ulps(got, _want_aggregate(clients, n, base, weights, clip=1.0, lr=lr)), lr
    aliased = base.clone()
    _aggregate(clients, n, aliased, weights, sq=sq, out=aliased, clip_norm=1.0, server_lr=0.5)
    assert torch.equal(aliased.view(torch.int32), got.view(torch.int32))


# ------------------------------------------------------------------------------------------------ aggregate, noise
def test_noise_is_the_philox_stream():
    n, seed, offset, std = (1 << 20) + 3, (1 << 40) + 77, (1 << 33) + 5, 1.0
    g = torch.Generator().manual_seed(4)
    base = (0.1 * torch.randn(n, generator=g)).to(_dev())
    outs = {}
    for K in (2, 5):
        clients = base.repeat(K, 1).contiguous()
        outs[K] = _aggregate(clients, n, base, [1.0] * K, noise_std=std, seed=seed, offset=offset)
    z = torch.from_numpy(oracle.normals(seed, offset, n)).to(_dev())
    err = ((outs[2].double() - base.double()) - std * z).abs().max().item()
    print(f"noise: max |out - base - std z| = {err:.3e}")
    assert err <= 2e-5 * std, err
    again = _aggregate(base.repeat(2, 1).contiguous(), n, base, [1.0, 1.0], noise_std=std, seed=seed, offset=offset)
    assert torch.equal(outs[2].view(torch.int32), again.view(torch.int32))                      # across calls
    assert torch.equal(outs[2].view(torch.int32), outs[5].view(torch.int32))                    # across K
    buf = torch.zeros(2 * n + 8, device=_dev())
    shifted = buf[1:1 + 2 * n].view(2, n)
    shifted.copy_(base.repeat(2, 1))
    sbase = torch.zeros(n + 1, device=_dev())[1:]
    sbase.copy_(base)
    sout = torch.zeros(n + 1, device=_dev())[1:]
    _aggregate(shifted, n, sbase, [1.0, 1.0], out=sout, noise_std=std, seed=seed, offset=offset)
    assert torch.equal(outs[2].view(torch.int32), sout.clone().view(torch.int32))               # across an alignment shift
    other = _aggregate(base.repeat(2, 1).contiguous(), n, base, [1.0, 1.0], noise_std=std, seed=seed, offset=offset + 1)
    assert (other != outs[2]).float().mean() > 0.99                                             # a new offset: new draws
    small = _aggregate(base[:7].repeat(2, 1).contiguous(), 7, base[:7], [1.0, 1.0], noise_std=std, seed=seed, offset=offset)
    assert torch.equal(small.view(torch.int32), outs[2][:7].clone().view(torch.int32))          # and independent of n (the tail too)


# ------------------------------------------------------------------------------------------------ per-slot DP kernels
def _sr_numels():
    from nerve_cl.models import SuperResolutionNet
    return [p.numel() for p in SuperResolutionNet(num_features=16, num_residual_blocks=1).parameters()]


TABLES = {"one": [1], "three": [3], "four": [4], "mixed": [5, 1, 7], "wide": [1, 147456, 2], "sr16": None}


def _bucket(numels, seed, C):
    """a bucket in the padded layout: slot s has norm 3 C (s even) or C / 2 (s odd); padding zero"""
    offs, total = oracle.padded_layout(numels)
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(total, dtype=torch.float64)
    for s, (o, k) in enumerate(zip(offs, numels)):
        v = torch.randn(k, generator=g, dtype=torch.float64)
        flat[o:o + k] = v / v.norm() * (3 * C if s % 2 == 0 else C / 2)
    return flat.float().to(_dev()), offs, total


@pytest.mark.parametrize("name", list(TABLES))
def test_dp_segment_norms_and_clip_noise(name):
    from nerve_cl import _nvq
    numels = TABLES[name] or _sr_numels()
    C, scale, seed, offset = 0.7, 0.05, 123456789, 3
    g, offs, total = _bucket(numels, 5, C)
    g0 = g.clone()
    table = _nvq.DpTable(offs, numels, _dev())
    _nvq.dp_segment_norms(g, table, _ws())
    want_sq = torch.stack([g0[o:o + k].double().pow(2).sum() for o, k in zip(offs, numels)])
    assert ((table.sq - want_sq).abs() <= 1e-10 * want_sq).all()
    assert torch.equal(g, g0)
    pad = torch.ones(total, dtype=torch.bool, device=_dev())
    for o, k in zip(offs, numels):
        pad[o:o + k] = False
    # noise_scale = 0: a slot under the bound keeps its bits, one above it is scaled
    _nvq.dp_clip_noise(g, table, C, 0.0, seed, offset)
    coef = torch.clamp(C / (want_sq.sqrt() + 1e-6), max=1.0)
    for s, (o, k) in enumerate(zip(offs, numels)):
        if coef[s] == 1.0:
            assert torch.equal(g[o:o + k].view(torch.int32), g0[o:o + k].view(torch.int32)), s
        else:
            want = g0[o:o + k].double() * coef[s]
            assert ((g[o:o + k].double() - want).abs() <= 1e-6 * want.abs()).all(), s
    assert (g[pad] == 0).all()
    # with noise
    g = g0.clone()
    _nvq.dp_clip_noise(g, table, C, scale, seed, offset)
    z = torch.from_numpy(oracle.normals(seed, offset, total)).to(_dev())
    worst = 0.0
    for s, (o, k) in enumerate(zip(offs, numels)):
        clipped = g0[o:o + k].double() * coef[s]
        err = (g[o:o + k].double() - (clipped + scale * z[o:o + k])).abs() - 1e-6 * clipped.abs()
        worst = max(worst, err.max().item())
    print(f"{name}: worst excess over the rounding term {worst:.3e} (noise bound {2e-5 * scale:.1e})")
    assert worst <= 2e-5 * scale
    assert (g[pad] == 0).all() and bool(pad.any()) == any(k % 4 for k in numels)
    again = g0.clone()
    _nvq.dp_clip_noise(again, table, C, scale, seed, offset)
    assert torch.equal(g.view(torch.int32), again.view(torch.int32))


def test_dp_kernels_refuse_a_misaligned_bucket():
    from nerve_cl import _nvq
    numels = [5, 1, 7]
    offs, total = oracle.padded_layout(numels)
    table = _nvq.DpTable(offs, numels, _dev())
    g = torch.zeros(total + 4, device=_dev())[1:1 + total]
    with pytest.raises(RuntimeError, match="16-byte"):
        _nvq.dp_segment_norms(g, table, _ws())
    with pytest.raises(RuntimeError, match="16-byte"):
        _nvq.dp_clip_noise(g, table, 1.0, 0.0, 0, 0)
    with pytest.raises(ValueError):
        _nvq.DpTable([0, 6], [5, 1], _dev())                            # a slot that does not start on a quad


# ------------------------------------------------------------------------------------------------ DPOptimizer
def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_dp_optimizer_on_the_device_matches_the_reference_values():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig
    f = np.load(GOLDEN)
    model = golden_model(f).to(_dev())
    cfg = PrivacyConfig(max_grad_norm=float(f["max_grad_norm"]), noise_multiplier=0.0)
    dp = DPOptimizer(torch.optim.SGD(model.parameters(), lr=float(f["sgd_lr"])), model, cfg, int(f["batch_size"]), 60, seed=1)
    for n, p in model.named_parameters():                               # the recorded gradients: only the DP step is under test
        p.grad = torch.from_numpy(f["g/" + n]).to(_dev())
    grads = {n: p.grad for n, p in model.named_parameters()}
    dp.step()
    assert dp.steps == 1 and dp.last_launches == 2
    for n, p in model.named_parameters():
        assert _rel(grads[n].cpu().numpy(), f["clipped/" + n]) <= 1e-6, n
        assert _rel(p.detach().cpu().numpy(), f["w1/" + n]) <= 1e-6, n


def test_dp_optimizer_device_and_cpu_draw_the_same_noise():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig
    f = np.load(GOLDEN)
    C, B = float(f["max_grad_norm"]), int(f["batch_size"])
    got = {}
    for dev in (torch.device("cpu"), _dev()):
        model = golden_model(f).to(dev)
        dp = DPOptimizer(torch.optim.SGD(model.parameters(), lr=0.0), model, PrivacyConfig(max_grad_norm=C, noise_multiplier=2.0),
                         B, 60, seed=4242)
        for _ in range(2):                                              # lr = 0: two steps on the recorded gradients
            for n, p in model.named_parameters():
                p.grad = torch.from_numpy(f["g/" + n]).to(dev)
            dp.step()
        got[dev.type] = {n: p.grad.cpu().double() for n, p in model.named_parameters()}
    scale = 2.0 * C / B
    for n, a in got["cpu"].items():
        b = got["cuda"][n]
        assert ((a - b).abs() <= 2e-6 * a.abs() + 2e-5 * scale).all(), n


def _sr_net():
    from nerve_cl.models import SuperResolutionNet
    torch.manual_seed(3)
    net = SuperResolutionNet(num_features=16, num_residual_blocks=1).to(_dev()).train()
    net.deterministic = True
    return net


def _clips(count, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(count, 3, 3, 16, 16, generator=g) + shift).to(_dev()), (torch.rand(count, 3, 32, 32, generator=g) + shift).to(_dev())


def test_dp_optimizer_takes_the_gradient_bucket_in_two_launches():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig
    net = _sr_net()
    C, B, seed = 1e-3, 4, 99
    dp = DPOptimizer(torch.optim.SGD(net.parameters(), lr=0.0), net, PrivacyConfig(max_grad_norm=C, noise_multiplier=1.0), B, 8, seed=seed)
    x, y = _clips(B, 1)
    dp.zero_grad()
    nn.functional.mse_loss(net(x), y).backward()
    bucket = net._last_grad_bucket
    before = bucket.clone()
    dp.step()
    assert dp.last_launches == 2 and net._last_grad_bucket is bucket
    lay, total = net._bucket_layout()
    z = torch.from_numpy(oracle.normals(seed, 0, total)).to(_dev())
    pad = torch.ones(total, dtype=torch.bool, device=_dev())
    clipped_any = False
    for n, p in net.named_parameters():
        o, k = lay[n]
        pad[o:o + k] = False
        g0 = before[o:o + k].double()
        coef = min(C / (g0.pow(2).sum().sqrt().item() + 1e-6), 1.0)
        clipped_any |= coef < 1.0
        want = g0 * coef + C / B * z[o:o + k]
        assert ((p.grad.reshape(-1).double() - want).abs() <= 1e-6 * (g0 * coef).abs() + 2e-5 * C / B).all(), n
    assert clipped_any and (bucket[pad] == 0).all()


# ------------------------------------------------------------------------------------------------ FederatedTrainer
def test_trainer_round_on_the_device():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    start = copy.deepcopy(net)
    data = {c: _clips(8, 10 + c, 0.05 * c) for c in range(3)}
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8)
    for c, d in data.items():
        tr.set_client_data(c, d)
    theta_ptr = net.flat_theta().data_ptr()
    out = tr.train_round()
    assert out["round"] == 1 and out["clients"] == 3 and out["samples"] == 24 and np.isfinite(out["train_loss"])
    assert net.flat_theta().data_ptr() == theta_ptr                                 # never re-homed
    states, thetas = [], []
    for c in tr.last_selected:
        m = copy.deepcopy(start).train()
        m.deterministic = True
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True)
        xs, ys = data[c]
        for i in range(0, 8, 4):
            opt.zero_grad()
            nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4]).backward()
            opt.step()
        states.append({k: v.clone() for k, v in m.state_dict().items()})
        thetas.append(m.flat_theta().clone())
    w = torch.full((3,), 8.0, dtype=torch.float64, device=_dev())
    want = (torch.stack(thetas).double() * w.view(3, 1)).sum(0) / w.sum()
    assert (torch.stack(thetas)[0] != start.flat_theta()).any()
    assert _within_ulps(net.flat_theta(), want)
    seen_int = False
    for k, v in net.state_dict().items():
        stack = torch.stack([s[k] for s in states]).double()
        mean = (stack * w.view(3, *([1] * (stack.dim() - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert _within_ulps(v, mean), k
        else:
            seen_int = True
            assert torch.equal(v, mean.trunc().to(v.dtype)), k
    assert seen_int


def test_trainer_round_reads_nothing_back():
    from nerve_cl.federated import FederatedTrainer, PrivacyConfig
    net = _sr_net()
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=2, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                          privacy=PrivacyConfig(noise_multiplier=0.1), update_clip=1.0, update_noise=1e-4, server_lr=0.5)
    for c in range(3):
        tr.set_client_data(c, _clips(8, 20 + c))
    tr.train_round()                                                    # warm-up: code objects loaded, buffers and tables built
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = tr.train_round_device()
        try:
            out["train_loss"].item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if not control_raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this PyTorch build: the check would be vacuous")
    assert out["round"] == 2 and np.isfinite(out["train_loss"].item()) and torch.isfinite(net.flat_theta()).all()


# ------------------------------------------------------------------------------------------------ the script
@pytest.mark.parametrize("extra", [[], ["--dp-enabled", "--update-clip", "1.0", "--update-noise", "0.01"]])
def test_train_federated_script(tmp_path, extra):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_federated.py"),
           "--num-clients", "3", "--clients-per-round", "2", "--num-rounds", "2", "--local-epochs", "1", "--samples", "8",
           "--features", "16", "--blocks", "1"] + extra
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rounds = [ln for ln in r.stdout.splitlines() if ln.startswith("Round ")]
    assert len(rounds) == 2 and rounds[1].startswith("Round 2: 2 clients, 16 samples"), r.stdout
    for ln in rounds:
        assert np.isfinite(float(ln.split("loss")[1].split()[0].strip(":="))), ln
