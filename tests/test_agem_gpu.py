"""GPU: the flat-bucket kernels of csrc/bucket_ops.hip (moments, A-GEM projection, global-norm clipping) against float64
torch on copies of the same device data, and AGEM / ops.clip_grad_norm_ on the product path: the engine's gradient bucket in
place, HIP-graph steps, accumulated gradients, two bucketed networks, a device memory, two data-parallel ranks.

Bounds.  Moments: the products are exact in double and summed in double, so |got - want| <= n 2^-53 sum|g_i r_i|, rounded up to
1e-10 sum|g_i r_i| for every n here.  Projection: c is rounded to fp32 once and the update is one fma, 2 * 2^-24 (|g_i| + |c r_i|)
per element, asserted with a factor-2 margin; summed against r that bounds the remaining |g'.r| by 4 * 2^-24 |g||r| (asserted at
8).  Clipping: one rounding of the coefficient and one of the product."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS24 = 2.0 ** -24
SECOND_TRIP = 1024 * 256 * 4 + 5        # 1024 blocks x 256 threads x one quad: some thread takes a second trip, plus a tail
SIZES = [1, 3, 255, 256, 257, 1025, SECOND_TRIP]


def _dev():
    return torch.device("cuda", 0)


def _acc():
    return torch.zeros(5, dtype=torch.float64, device=_dev())


def _ws():
    from nerve_cl import _engine
    return _engine.workspace(_dev())


def _pair(n, seed, offset=0, conflict=False):
    """g, r of n floats; offset 1: views that start 4 bytes into their allocation (not 16-byte aligned)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g = torch.randn(n + offset, generator=gen).to(_dev())[offset:]
    noise = torch.randn(n + offset, generator=gen).to(_dev())[offset:]
    r = torch.empty(n + offset, device=_dev())[offset:]
    r.copy_(-g * (0.5 + noise.abs()) if conflict else noise)            # conflict: g.r = -sum g_i^2 (0.5 + |noise_i|) < 0 for every n
    if offset:
        assert g.data_ptr() % 16 == 4 and r.data_ptr() % 16 == 4
    return g, r


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _check_moments(acc, g, r):
    gd = g.double()
    rd = r.double() if r is not None else torch.zeros_like(gd)
    for slot, (a, b) in enumerate(((gd, rd), (rd, rd), (gd, gd))):
        want, scale = (a * b).sum().item(), (a * b).abs().sum().item()
        got = acc[slot].item()
        assert abs(got - want) <= 1e-10 * scale, (slot, got, want, scale)


# ------------------------------------------------------------------------------------------------- moments

@pytest.mark.parametrize("n", SIZES)
def test_moments_against_float64(n):
    from nerve_cl import _nvq
    g, r = _pair(n, 100 + n % 97)
    acc = _acc()
    _nvq.bucket_moments(g, r, acc, _ws())
    _check_moments(acc, g, r)
    assert acc[3] == 0 and acc[4] == 0
    again = _acc()
    _nvq.bucket_moments(g, r, again, _ws())
    assert torch.equal(_bits_f64(acc), _bits_f64(again))                # no atomics, a fixed grid: the same bits


def _bits_f64(t):
    return t.detach().clone().view(torch.int64)


@pytest.mark.parametrize("n", [257, 1025, SECOND_TRIP])
def test_moments_on_pointers_that_are_only_4_byte_aligned(n):
    from nerve_cl import _nvq
    g, r = _pair(n, 7, offset=1)
    acc = _acc()
    _nvq.bucket_moments(g, r, acc, _ws())
    _check_moments(acc, g, r)
    aligned = _acc()                                                    # the same values at 16-byte aligned addresses: same bits
    _nvq.bucket_moments(g.clone(), r.clone(), aligned, _ws())
    assert torch.equal(_bits_f64(acc), _bits_f64(aligned))


def test_two_chained_segments_equal_their_concatenation():
    from nerve_cl import _nvq
    g, r = _pair(1025 + 4099, 11)
    acc = _acc()
    _nvq.bucket_moments(g[:1025], r[:1025], acc, _ws())
    _nvq.bucket_moments(g[1025:], r[1025:], acc, _ws(), accumulate=True)      # starts 4 bytes past a 16-byte boundary
    _check_moments(acc, g, r)


def test_moments_without_a_reference_give_the_squared_norm_only():
    from nerve_cl import _nvq
    g, _ = _pair(1025, 12)
    acc = _acc()
    acc[:2] = 7.0
    _nvq.bucket_moments(g, None, acc, _ws())
    _check_moments(acc, g, None)
    assert acc[0] == 0 and acc[1] == 0
    _nvq.bucket_moments(g, None, acc, _ws(), accumulate=True)
    assert abs(acc[2].item() - 2 * (g.double() ** 2).sum().item()) <= 1e-10 * 2 * (g.double() ** 2).sum().item()


# ------------------------------------------------------------------------------------------------- projection

def _check_projection(g0, r, g1, c):
    gd, rd = g0.double(), r.double()
    want = gd - c * rd
    err = (g1.double() - want).abs()
    bound = 4 * EPS24 * (gd.abs() + (c * rd).abs())
    assert bool((err <= bound).all()), (err - bound).max().item()
    assert abs((g1.double() * rd).sum().item()) <= 8 * EPS24 * (gd.norm() * rd.norm()).item()


@pytest.mark.parametrize("n,offset", [(3, 0), (257, 0), (1025, 1), (SECOND_TRIP, 0), (SECOND_TRIP, 1)])
def test_projection_of_a_conflicting_gradient(n, offset):
    from nerve_cl import _nvq
    g, r = _pair(n, 21, offset, conflict=True)
    g0 = g.clone()
    acc = _acc()
    _nvq.bucket_moments(g, r, acc, _ws(), coefficient=True)
    _nvq.bucket_project(g, r, acc)
    gr, rr = (g0.double() * r.double()).sum().item(), (r.double() ** 2).sum().item()
    assert gr < 0
    c = acc[3].item()
    assert abs(c - gr / rr) <= 1e-9 * abs(gr / rr) and acc[4] == 1
    _check_projection(g0, r, g, gr / rr)


@pytest.mark.parametrize("case", ["agree", "zero_reference", "nan"])
def test_projection_leaves_the_gradient_bit_identical_without_a_conflict(case):
    from nerve_cl import _nvq
    g, r = _pair(1029, 22, conflict=True)
    if case == "agree":
        r = g.clone() + 0.1 * r
        assert (g.double() * r.double()).sum() >= 0
    elif case == "zero_reference":
        r = torch.zeros_like(g)
    else:
        g[517] = float("nan")
    before = _bits(g)
    acc = _acc()
    _nvq.bucket_moments(g, r, acc, _ws(), coefficient=True)
    _nvq.bucket_project(g, r, acc)
    assert torch.equal(_bits(g), before)
    assert acc[3] == 0 and acc[4] == 0


def test_the_counter_counts_only_the_conflicting_calls():
    from nerve_cl import _nvq
    acc = _acc()
    for conflict in (True, False, True, False, False):
        g, r = _pair(300, 23, conflict=True)
        if not conflict:
            r = g.clone()
        _nvq.bucket_moments(g, r, acc, _ws(), coefficient=True)
        _nvq.bucket_project(g, r, acc)
        assert (acc[3].item() != 0) == conflict
    assert acc[4] == 2


# ------------------------------------------------------------------------------------------------- clipping

@pytest.mark.parametrize("n,offset", [(3, 0), (1025, 1), (SECOND_TRIP, 0)])
def test_clip_kernel(n, offset):
    from nerve_cl import _nvq
    g, _ = _pair(n, 31, offset)
    g0 = g.clone()
    norm64 = g0.double().norm().item()
    acc = _acc()
    out = torch.zeros((), dtype=torch.float32, device=_dev())
    _nvq.bucket_moments(g, None, acc, _ws())
    _nvq.bucket_clip(g, acc, 2.0 * norm64, out)                         # max_norm above the norm: untouched
    assert torch.equal(_bits(g), _bits(g0))
    assert abs(out.item() - norm64) <= 2.0 ** -23 * norm64
    max_norm = 0.25 * norm64
    _nvq.bucket_clip(g, acc, max_norm, out)
    want = g0.double() * (max_norm / (norm64 + 1e-6))
    assert bool(((g.double() - want).abs() <= 4 * EPS24 * g0.double().abs()).all())
    assert abs(out.item() - norm64) <= 2.0 ** -23 * norm64


# ------------------------------------------------------------------------------------------------- the product path

CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B, H, W = 2, 16, 24


def _engine(**extra):
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG, **extra))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    return eng.to(_dev()).train()


def _data():
    from oracle import synth
    x, y = synth.formula_clip(B, 3, H, W), synth.formula_target(B, 2 * H, 2 * W)
    return x.to(_dev()), y.to(_dev())


def _flat_grads(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])


def _aliases_bucket(net) -> bool:
    lay, _ = net._bucket_layout()
    base = net._last_grad_bucket.data_ptr()
    return all(p.grad is not None and p.grad.data_ptr() == base + 4 * lay[n][0] for n, p in net.named_parameters())


def _conflict_step(eng, agem, x, y, sign, mix=0.0, backwards=1):
    """capture r = grad L, then g = grad(sign * L + mix * L2) (`backwards` times, accumulating); -> (g, r) clones before project"""
    def loss():
        return F.mse_loss(eng(x)["enhanced"], y)
    eng.zero_grad()
    loss().backward()
    agem.capture_reference()
    eng.zero_grad()
    for _ in range(backwards):
        out = eng(x)["enhanced"]
        (sign * F.mse_loss(out, y) + mix * F.mse_loss(out, y.flip(0) * 0.5)).backward()
    g = _flat_grads(eng).clone()
    r = torch.cat([ref[o:o + k] for sg, ref in zip(agem._segs, agem._ref) if sg.net is not None
                   for o, k in sg.net._bucket_layout()[0].values()]).clone()
    return g, r


@pytest.mark.parametrize("mix", [0.0, 0.5], ids=["minus_L", "minus_L_plus_other"])
def test_agem_projects_the_engines_bucket_in_place_and_the_step_uses_it(mix):
    from nerve_cl.continual import AGEM
    eng = _engine()
    x, y = _data()
    agem = AGEM(eng)
    opt = torch.optim.SGD(eng.parameters(), lr=0.1)
    g, r = _conflict_step(eng, agem, x, y, -1.0, mix)
    assert _aliases_bucket(eng.super_resolution)
    agem.project()
    gr, rr = (g.double() * r.double()).sum().item(), (r.double() ** 2).sum().item()
    assert gr < 0 and agem.num_projections() == 1
    assert abs(agem.stats[3].item() - gr / rr) <= 1e-9 * abs(gr / rr)
    assert _aliases_bucket(eng.super_resolution)                        # still the bucket's views: projected in place
    g1 = _flat_grads(eng)
    _check_projection(g, r, g1, gr / rr)
    assert torch.equal(g1, torch.cat([eng.super_resolution._last_grad_bucket[o:o + k]
                                      for o, k in eng.super_resolution._bucket_layout()[0].values()]))
    before = torch.cat([p.detach().reshape(-1) for p in eng.super_resolution.parameters()]).clone()
    opt.step()
    after = torch.cat([p.detach().reshape(-1) for p in eng.super_resolution.parameters()])
    want = before.double() - 0.1 * g1.double()
    assert bool(((after.double() - want).abs() <= 4 * EPS24 * (before.double().abs() + 0.1 * g1.double().abs())).all())
    if mix:
        assert (after != before).any()
    cos = agem.cosine()
    assert cos.is_cuda and cos.dim() == 0 and abs(cos.item() - gr / (g.double().norm() * r.double().norm()).item()) <= 1e-9


def test_agem_leaves_an_agreeing_gradient_bit_identical():
    from nerve_cl.continual import AGEM
    eng = _engine()
    x, y = _data()
    agem = AGEM(eng)
    g, r = _conflict_step(eng, agem, x, y, +1.0)
    agem.project()
    assert torch.equal(_bits(_flat_grads(eng)), _bits(g))
    assert agem.stats[0] > 0 and agem.stats[3] == 0 and agem.num_projections() == 0


def test_agem_with_hip_graph_steps():
    from nerve_cl.continual import AGEM
    eng = _engine()
    eng.super_resolution.use_hip_graphs = True
    x, y = _data()
    for _ in range(3):                                                  # two eager warm-up calls, capture on the third
        eng.zero_grad()
        F.mse_loss(eng(x)["enhanced"], y).backward()
    agem = AGEM(eng)
    replays = eng.super_resolution._step_graphs.replays
    g, r = _conflict_step(eng, agem, x, y, -1.0, 0.5)
    assert eng.super_resolution._step_graphs.replays >= replays + 2
    assert _aliases_bucket(eng.super_resolution)
    agem.project()
    gr, rr = (g.double() * r.double()).sum().item(), (r.double() ** 2).sum().item()
    assert gr < 0 and agem.num_projections() == 1
    _check_projection(g, r, _flat_grads(eng), gr / rr)


def test_agem_on_accumulated_gradients_goes_per_tensor():
    from nerve_cl.continual import AGEM
    eng = _engine()
    x, y = _data()
    agem = AGEM(eng)
    g, r = _conflict_step(eng, agem, x, y, -1.0, 0.5, backwards=2)
    assert not _aliases_bucket(eng.super_resolution)
    agem.project()
    gr, rr = (g.double() * r.double()).sum().item(), (r.double() ** 2).sum().item()
    assert gr < 0 and agem.num_projections() == 1
    _check_projection(g, r, _flat_grads(eng), gr / rr)


def test_agem_forms_one_coefficient_over_two_bucketed_networks():
    from nerve_cl.continual import AGEM
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=True, recovery_base_channels=16, recovery_temporal_window=1,
                                              **CFG))
    eng.frame_recovery.load_state_dict(synth.formula_state_fr(3, 16, gain=synth.GOLDEN_GAIN))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    eng = eng.to(_dev()).train()
    x = synth.formula_clip(B, 3, 32, 32).to(_dev())
    y = synth.formula_target(B, 64, 64).to(_dev())
    mask = torch.zeros(B, 1, 32, 32, device=_dev())
    mask[:, :, 8:24, 4:20] = 1.0

    def loss(sign):
        res = eng(x, corruption_mask=mask)
        return sign * F.mse_loss(res["enhanced"], y) + 0.3 * sign * F.mse_loss(res["recovered"], x[:, 1] * 0.5)

    agem = AGEM(eng)
    nets = [sg.net for sg in agem._segs if sg.net is not None]
    assert len(nets) == 2
    eng.zero_grad()
    loss(1.0).backward()
    agem.capture_reference()
    eng.zero_grad()
    loss(-1.0).backward()
    assert all(_aliases_bucket(n) for n in nets)
    gs = [n._last_grad_bucket.clone() for n in nets]
    rs = [ref.clone() for sg, ref in zip(agem._segs, agem._ref) if sg.net is not None]
    assert all(r.abs().max() > 0 for r in rs)
    agem.project()
    g, r = torch.cat(gs), torch.cat(rs)
    gr, rr = (g.double() * r.double()).sum().item(), (r.double() ** 2).sum().item()
    assert gr < 0
    assert abs(agem.stats[3].item() - gr / rr) <= 1e-9 * abs(gr / rr)    # one c from the sums over both networks
    _check_projection(g, r, torch.cat([n._last_grad_bucket for n in nets]), gr / rr)


class _Clip(nn.Module):
    """(B,C,H,W) frames -> the engine on the repeated-frame clip -> 'enhanced'"""

    def __init__(self, eng):
        super().__init__()
        self.engine = eng

    def forward(self, x):
        return self.engine(x.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]


def test_compute_reference_draws_from_a_device_memory():
    from nerve_cl import ops
    from nerve_cl.continual import AGEM, DeviceEpisodicMemory
    eng = _engine()
    model = _Clip(eng)
    mem = DeviceEpisodicMemory(capacity=8, strategy="stratified", device=_dev(), seed=0)
    agem = AGEM(model, mem, ref_batch_size=2)
    assert agem.compute_reference(ops.MSELoss()) is False
    x, y = _data()
    mem.store_batch(torch.cat([x[:, 0], x[:, 1]]), torch.cat([y, y * 0.5]), content_type="movie")
    assert len(mem) == 4
    assert agem.compute_reference(ops.MSELoss()) is True
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    assert agem._ref[0].abs().max() > 0


def test_ops_clip_grad_norm_on_the_engine_and_on_a_parameter_list():
    from nerve_cl import ops
    eng = _engine()
    x, y = _data()
    for target in ("module", "parameters"):
        eng.zero_grad()
        F.mse_loss(eng(x)["enhanced"], y).backward()
        g0 = _flat_grads(eng).clone()
        norm64 = g0.double().norm().item()
        arg = eng if target == "module" else [p for p in eng.parameters()]
        got = ops.clip_grad_norm_(arg, 10.0 * norm64)
        assert got.is_cuda and got.dim() == 0 and abs(got.item() - norm64) <= 2.0 ** -23 * norm64
        assert torch.equal(_bits(_flat_grads(eng)), _bits(g0))
        got = ops.clip_grad_norm_(arg, 0.5 * norm64)
        want = g0.double() * (0.5 * norm64 / (norm64 + 1e-6))
        assert bool(((_flat_grads(eng).double() - want).abs() <= 4 * EPS24 * g0.double().abs()).all())
        assert abs(got.item() - norm64) <= 2.0 ** -23 * norm64
        assert _aliases_bucket(eng.super_resolution)


# ------------------------------------------------------------------------------------------------- data parallel

def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_two_ranks_project_to_the_same_gradient(tmp_path):
    out = tmp_path / "agem.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    # children are ordinary child processes of a launcher that never touches the GPU
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(HERE, "agem_worker.py"), str(out)], env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out, weights_only=True)
    assert torch.equal(got["grads_rank0"], got["grads_rank1"])         # the same c on both ranks, no extra collective
    assert got["projections"] == [1, 1]

    sys.path.insert(0, HERE)
    import agem_worker as Wk
    dev = _dev()
    x, y = Wk.data(2)
    x, y = x.to(dev), y.to(dev)
    b = Wk.B_PER_RANK
    state0 = {k: v.clone() for k, v in Wk.make_engine().state_dict().items()}

    def rank_mean_bucket(sign):
        buckets = []
        for k in range(2):                                              # every rank starts from rank 0's broadcast state
            eng = Wk.make_engine()
            eng.load_state_dict(state0)
            eng = eng.to(dev).train()
            Wk.loss(eng, x[b * k:b * k + b], y[b * k:b * k + b], sign).backward()
            buckets.append(eng.super_resolution._last_grad_bucket.clone())
        lay = eng.super_resolution._bucket_layout()[0]
        mean = (buckets[0] + buckets[1]) / 2
        return torch.cat([mean[o:o + n] for o, n in lay.values()]).double()

    rr_, gg_ = rank_mean_bucket(+1.0), rank_mean_bucket(-1.0)
    c = (gg_ * rr_).sum() / (rr_ * rr_).sum()
    assert c < 0
    want = gg_ - c * rr_
    assert (got["grads_rank0"].to(dev).double() - want).abs().max() <= 1e-5 * want.abs().max()
