"""GPU: csrc/fedopt.hip (nvq_fed_server_opt, nvq_fed_prox_grad) against the float64 oracle of tests/_fedopt_oracle.py, then
ServerOptimizer, FederatedTrainer(server_optimizer=..., prox_mu=...) and experiments/train_federated.py on the device.

One criterion for values: test_federated_gpu._within_ulps(got, want_float64, 1).  The kernel rounds a double chain to fp32 once
per stored value; the float64 oracle differs from it by double rounding only (~1e-15 relative), so by at most one fp32 ulp.  Every
round is teacher-forced: the oracle starts from the m and v the device holds.  Yogi's sign(v - D^2) is discontinuous, so its cases
first assert on the oracle that every element is further than 1e-9 (relative) from v = D^2."""
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
import _fedopt_oracle as oracle  # noqa: E402
from test_federated_gpu import SECOND_TRIP, _aggregate, _clips, _dev, _matrix, _pad4, _sq, _sr_net, _within_ulps  # noqa: E402

LR, BETAS, TAU = 0.1, (0.9, 0.99), 1e-3
SENTINEL = 12345.0
RULE_ID = {r: i for i, r in enumerate(oracle.RULES)}


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _vec(values, shift=0):
    """``values`` (n floats, or None: NaN) as a view `shift` floats into an allocation that ends in four sentinel floats"""
    n = values.numel() if isinstance(values, torch.Tensor) else int(values)
    buf = torch.full((shift + n + 4,), SENTINEL, device=_dev())
    view = buf[shift:shift + n]
    if isinstance(values, torch.Tensor):
        view.copy_(values)
    else:
        view.fill_(float("nan"))
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return buf, view


def _intact(*bufs):
    return all(bool((b[-4:] == SENTINEL).all()) for b in bufs)


def _call(clients, n, base, weights, rule, m, v, out, sq=None, lr=LR, betas=BETAS, tau=TAU, **kw):
    from nerve_cl import _nvq
    w = torch.tensor(weights, dtype=torch.float64).to(_dev())
    _nvq.fed_server_opt(clients, n, base, w, sq, RULE_ID[rule], m, v, out, server_lr=lr, beta1=betas[0], beta2=betas[1], tau=tau, **kw)


def _bits(t):
    return t.clone().view(torch.int32)


def _two_rounds(rule, n, K, padded):
    stride = _pad4(n) if padded else n
    weights = [float(k + 1) for k in range(K)]
    m0, v0 = oracle.initial_state(rule, n, TAU)
    mbuf, m = _vec(m0)
    vbuf, v = _vec(v0) if v0 is not None else (None, None)
    base = None
    for rnd in range(2):
        seed = 3000 + 100 * rnd + n % 89 + K
        clients, b0 = _matrix(K, n, stride, seed)
        base = b0 if base is None else base
        m_prev, v_prev = m.clone(), None if v is None else v.clone()
        D = oracle.pseudo_gradient(clients[:, :n], base, weights)
        if rule == "fedyogi":
            assert oracle.yogi_margin(D, v_prev) > 1e-9
        want, m1, v1 = oracle.server_step(rule, D, base, m_prev, v_prev, LR, BETAS, TAU)
        obuf, out = _vec(n)
        _call(clients, n, base, weights, rule, m, v, out)
        assert _within_ulps(out, _t64(want)), (rnd, "out")
        assert _within_ulps(m, _t64(m1)), (rnd, "m")
        assert v is None or _within_ulps(v, _t64(v1)), (rnd, "v")
        assert _intact(obuf, mbuf) and (vbuf is None or _intact(vbuf))
        # only 4-byte aligned (the scalar path): the same bits
        shifted, _ = _matrix(K, n, stride, seed, shift=1)
        sb, sbase = _vec(base, 1)
        smb, sm = _vec(m_prev, 1)
        svb, sv = _vec(v_prev, 1) if v_prev is not None else (None, None)
        sob, sout = _vec(n, 1)
        _call(shifted, n, sbase, weights, rule, sm, sv, sout)
        assert torch.equal(_bits(sout), _bits(out)) and torch.equal(_bits(sm), _bits(m)), rnd
        assert sv is None or torch.equal(_bits(sv), _bits(v)), rnd
        assert _intact(sob, smb, sb) and (svb is None or _intact(svb))
        # out may be base
        ab, aliased = _vec(base)
        _, am = _vec(m_prev)
        _, av = _vec(v_prev) if v_prev is not None else (None, None)
        _call(clients, n, aliased, weights, rule, am, av, aliased)
        assert torch.equal(_bits(aliased), _bits(out)) and torch.equal(_bits(am), _bits(m)) and _intact(ab), rnd
        assert av is None or torch.equal(_bits(av), _bits(v)), rnd
        base = out.clone()
    assert (m != 0).any()


@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
@pytest.mark.parametrize("rule", oracle.RULES)
def test_server_opt_against_float64(rule, n, K):
    for padded in (False, True):
        _two_rounds(rule, n, K, padded)


@pytest.mark.parametrize("rule,K,padded", [("fedadam", 2, False), ("fedyogi", 5, True)])
def test_server_opt_second_grid_trip_and_tail(rule, K, padded):
    _two_rounds(rule, SECOND_TRIP, K, padded)


@pytest.mark.parametrize("n", [5, 1023])
def test_fedavgm_without_momentum_has_the_bits_of_fed_aggregate(n):
    K, stride = 5, _pad4(n)
    clients, base = _matrix(K, n, stride, 77)
    with torch.no_grad():
        clients[0, :n] = base + 5.0 * torch.randn(n, device=_dev())     # far above the clip bound
    weights = [float(k + 1) for k in range(K)]
    sq = _sq(clients, n, base)
    mbuf, m = _vec(torch.zeros(n))
    for rnd in range(2):                                                # the second call: m is the first update, not zero
        kw = dict(sq=sq, clip_norm=1.0, noise_std=0.05, seed=(1 << 40) + 9, offset=(1 << 33) + rnd)
        want = _aggregate(clients, n, base, weights, server_lr=0.5, **kw)
        obuf, out = _vec(n)
        _call(clients, n, base, weights, "fedavgm", m, None, out, lr=0.5, betas=(0.0, 0.99), **kw)
        assert torch.equal(_bits(out), _bits(want)), rnd
        assert _intact(obuf, mbuf) and (m != 0).any()


@pytest.mark.parametrize("rule", oracle.RULES[1:])
def test_adaptive_rule_with_noise(rule):
    """out - out_plain = noise_std z: the project's normals bound (2e-5 noise_std absolute, tests/test_federated_gpu.py) plus the one
    rounding of the final fmaf, an ulp of the larger of out and out_plain; the noise never reaches m and v."""
    from nerve_cl.federated import _philox
    n, K, std, seed, offset = 1023, 2, 0.05, (1 << 40) + 77, (1 << 33) + 5
    clients, base = _matrix(K, n, n, 55)
    weights = [1.0, 2.0]
    got = {}
    for noise in (0.0, std):
        m0, v0 = oracle.initial_state(rule, n, TAU)
        mbuf, m = _vec(m0)
        vbuf, v = _vec(v0)
        obuf, out = _vec(n)
        _call(clients, n, base, weights, rule, m, v, out, noise_std=noise, seed=seed, offset=offset)
        assert _intact(mbuf, vbuf, obuf)
        got[noise] = (out.clone(), m.clone(), v.clone())
    plain, noisy = got[0.0][0], got[std][0]
    z = _t64(_philox.normals(seed, offset, n))
    big = torch.maximum(plain.abs(), noisy.abs())
    ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
    err = ((noisy.double() - plain.double()) - std * z).abs()
    print(f"{rule}: max |out - out_plain - std z| = {err.max().item():.3e}")
    assert (err <= 2e-5 * std + ulp).all()
    assert (noisy != plain).float().mean() > 0.99
    assert torch.equal(_bits(got[0.0][1]), _bits(got[std][1])) and torch.equal(_bits(got[0.0][2]), _bits(got[std][2]))


def test_robust_rule_then_the_single_row_step():
    from nerve_cl.federated import ServerOptimizer, aggregate_flat_median
    n, K = 1023, 5
    opt = ServerOptimizer("fedyogi", lr=LR, betas=BETAS, tau=TAU)
    base = None
    for rnd in range(2):
        clients, b0 = _matrix(K, n, n, 900 + rnd)
        base = b0 if base is None else base
        agg = aggregate_flat_median(clients, base=base)
        m, v = (opt.m.clone(), opt.v.clone()) if opt.m is not None else oracle.initial_state("fedyogi", n, TAU)
        D = oracle.pseudo_gradient(agg[None], base, [1.0])              # the pseudo-gradient of the fp32 aggregate
        assert oracle.yogi_margin(D, v) > 1e-9
        want, m1, v1 = oracle.server_step("fedyogi", D, base, m, v, LR, BETAS, TAU)
        out = opt.step(agg[None], [1.0], base)
        assert _within_ulps(out, _t64(want)) and _within_ulps(opt.m, _t64(m1)) and _within_ulps(opt.v, _t64(v1)), rnd
        base = out


# ------------------------------------------------------------------------------------------------ the FedProx gradient
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, SECOND_TRIP])
def test_prox_grad_against_float64(n):
    from nerve_cl import _nvq
    g = torch.Generator().manual_seed(600 + n % 89)
    grad0, theta0, anchor0 = (torch.randn(n, generator=g) for _ in range(3))
    mu = 0.01
    want = _t64(oracle.prox_grad(grad0, theta0, anchor0, mu))
    got = {}
    for shift in (0, 1):
        gb, grad = _vec(grad0, shift)
        tb, theta = _vec(theta0, shift)
        ab, anchor = _vec(anchor0, shift)
        _nvq.fed_prox_grad(grad, theta, anchor, 0.0)
        assert torch.equal(_bits(grad), _bits(grad0.to(_dev())))        # mu = 0: the same bits
        _nvq.fed_prox_grad(grad, theta, anchor, mu)
        assert _within_ulps(grad, want), shift
        assert torch.equal(theta.cpu(), theta0) and torch.equal(anchor.cpu(), anchor0) and _intact(gb, tb, ab)
        got[shift] = grad.clone()
    assert torch.equal(_bits(got[0]), _bits(got[1]))


def test_prox_grad_where_the_terms_cancel():
    """g ~ -mu (theta - anchor): fp32 arithmetic is not within an ulp of the exact value here, the kernel's double fma is"""
    from nerve_cl import _nvq
    n, mu = 1023, 0.01
    g = torch.Generator().manual_seed(8)
    theta0, anchor0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    grad0 = (-(oracle.f32(mu) * (theta0.double() - anchor0.double()))).float()
    want = oracle.prox_grad(grad0, theta0, anchor0, mu, exact=True)
    assert np.abs(want).max() < 1e-8 and (want != 0).any()
    _, grad = _vec(grad0)
    _nvq.fed_prox_grad(grad, theta0.to(_dev()), anchor0.to(_dev()), mu)
    assert _within_ulps(grad, _t64(want))


# ------------------------------------------------------------------------------------------------ refusals
def test_binding_refusals():
    from nerve_cl import _nvq
    n = 8
    dev = _dev()
    w = torch.ones(65, dtype=torch.float64, device=dev)
    base, m, v, out = (torch.zeros(n, device=dev) for _ in range(4))
    good = torch.zeros(2, n, device=dev)

    def call(clients=good, base=base, rule=2, m=m, v=v, out=out, **kw):
        _nvq.fed_server_opt(clients, n, base, w, None, rule, m, v, out, **kw)

    call()                                                              # the arguments the refusals vary are fine
    call(rule=0, v=None)                                                # fedavgm needs no v
    for bad in (dict(clients=torch.zeros(2, n, device=dev)[:0]), dict(clients=torch.zeros(65, n, device=dev)), dict(base=None),
                dict(m=None), dict(v=None), dict(v=None, rule=1), dict(v=None, rule=3), dict(rule=4), dict(rule=-1),
                dict(beta1=1.0), dict(beta2=1.0), dict(tau=0.0), dict(tau=0.0, rule=3), dict(noise_std=-1.0)):
        with pytest.raises(RuntimeError, match="nvq_fed_server_opt"):
            call(**bad)
    call(rule=0, v=None, tau=0.0)                                       # tau belongs to the adaptive rules
    for K in (0, 65):                                                   # the library's own check of K, with a good pointer
        rc = _nvq.lib().nvq_fed_server_opt(good.data_ptr(), n, K, base.data_ptr(), w.data_ptr(), None, 0.0, 2, 1.0, 0.9, 0.99, 1e-3,
                                           m.data_ptr(), v.data_ptr(), 0.0, 0, 0, n, out.data_ptr(), None)
        assert rc == -1 and f"fed_server_opt: K = {K}" in _nvq.lib().nvq_last_error().decode()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(clients=torch.zeros(2, n))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(m=torch.zeros(n))
    with pytest.raises(RuntimeError, match="nvq_fed_prox_grad"):
        _nvq.fed_prox_grad(out, base, m, -1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _nvq.fed_prox_grad(torch.zeros(n), base, m, 0.1)
    torch.cuda.synchronize()
    assert not base.any() and not out.any()                             # zeros in, zeros out: D = 0


# ------------------------------------------------------------------------------------------------ FederatedTrainer
def _hand_train(start, data):
    m = copy.deepcopy(start).train()
    m.deterministic = True
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True)
    xs, ys = data
    for i in range(0, len(xs), 4):
        opt.zero_grad()
        nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4]).backward()
        opt.step()
    return m


def test_trainer_fedadam_on_the_device():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    data = {c: _clips(8, 10 + c, 0.05 * c) for c in range(3)}
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                          server_optimizer="fedadam", server_lr=1e-3, server_betas=BETAS, server_tau=TAU)
    for c, d in data.items():
        tr.set_client_data(c, d)
    theta_ptr = net.flat_theta().data_ptr()
    n = net.flat_theta().numel()
    w = [8.0, 8.0, 8.0]
    for rnd in range(2):
        start = copy.deepcopy(net)
        if rnd == 0:
            m, v = oracle.initial_state("fedadam", n, TAU)
        else:
            m, v = tr._server_opts[0].m.clone(), tr._server_opts[0].v.clone()
        out = tr.train_round()
        assert out["round"] == rnd + 1 and out["clients"] == 3 and np.isfinite(out["train_loss"])
        assert net.flat_theta().data_ptr() == theta_ptr                 # never re-homed
        copies = [_hand_train(start, data[c]) for c in tr.last_selected]
        thetas = torch.stack([c.flat_theta() for c in copies])
        base = start.flat_theta()
        assert (thetas[0] != base).any()
        D = oracle.pseudo_gradient(thetas, base, w)
        want, m1, v1 = oracle.server_step("fedadam", D, base, m, v, 1e-3, BETAS, TAU)
        assert _within_ulps(net.flat_theta(), _t64(want)), rnd
        assert _within_ulps(tr._server_opts[0].m, _t64(m1)) and _within_ulps(tr._server_opts[0].v, _t64(v1)), rnd
        assert (net.flat_theta() != base).any()
        params = {k for k, _ in net.named_parameters()}
        states = [c.state_dict() for c in copies]
        seen_float = seen_int = False
        for k, val in net.state_dict().items():                         # the BatchNorm statistics: the plain mean
            if k in params:
                continue
            mean = torch.stack([s[k] for s in states]).double().mean(0)
            if val.is_floating_point():
                seen_float = True
                assert _within_ulps(val, mean), k
            else:
                seen_int = True
                assert torch.equal(val, mean.trunc().to(val.dtype)), k
        assert seen_float and seen_int
    assert len(tr.server_state_dict()["states"]) == 1


def test_trainer_fedadam_on_a_plain_module_on_the_device():
    """no HIP-backed network: the parameters' columns of the packed matrix (a strided view, a base inside a vector) take
    nvq_fed_server_opt, the statistics behind them the plain rule"""
    from nerve_cl.federated import FederatedTrainer
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(5, 7), nn.BatchNorm1d(7), nn.ReLU(), nn.Linear(7, 3)).to(_dev())
    start = copy.deepcopy(model)
    g = torch.Generator().manual_seed(11)
    data = {c: (torch.randn(8, 5, generator=g).to(_dev()) + 0.1 * c, torch.randn(8, 3, generator=g).to(_dev())) for c in range(3)}
    tr = FederatedTrainer(model, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-2, batch_size=4, seed=5,
                          server_optimizer="fedadam", server_lr=1e-2, server_betas=BETAS, server_tau=TAU)
    for c, d in data.items():
        tr.set_client_data(c, d)
    tr.train_round()
    states = []
    for c in tr.last_selected:
        m = copy.deepcopy(start).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-2, fused=True)
        xs, ys = data[c]
        for i in range(0, len(xs), 4):
            opt.zero_grad()
            nn.MSELoss()(m(xs[i:i + 4]), ys[i:i + 4]).backward()
            opt.step()
        states.append(m.state_dict())
    params = dict(model.named_parameters())
    assert tr._plan["n_params"] == sum((p.numel() + 3) // 4 * 4 for p in params.values()) and not tr._plan["nets"]
    for k, val in model.state_dict().items():
        stack = torch.stack([s[k].reshape(-1) for s in states])
        if k in params:
            base = start.state_dict()[k].reshape(-1)
            m0, v0 = oracle.initial_state("fedadam", base.numel(), TAU)
            D = oracle.pseudo_gradient(stack, base, [8.0, 8.0, 8.0])
            want, _, _ = oracle.server_step("fedadam", D, base, m0, v0, 1e-2, BETAS, TAU)
            assert _within_ulps(val.reshape(-1), _t64(want)), k
        elif val.is_floating_point():
            assert _within_ulps(val.reshape(-1), stack.double().mean(0)), k
        else:
            assert int(val) == int(stack.double().mean(0).trunc()), k


def test_trainer_prox_takes_one_launch_on_the_gradient_bucket(monkeypatch):
    """Trajectories are not compared (AdamW amplifies ulp differences): what the trainer hands to nvq_fed_prox_grad is."""
    from nerve_cl import _nvq
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    mu = 0.01
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=2, local_epochs=1, lr=1e-3, batch_size=4, seed=8, prox_mu=mu)
    for c in range(3):
        tr.set_client_data(c, _clips(8, 10 + c, 0.05 * c))
    start = net.flat_theta().clone()
    real, calls = _nvq.fed_prox_grad, []

    def recorder(grad, theta, anchor, mu_):
        before = (grad.clone(), theta.clone(), anchor.clone())
        real(grad, theta, anchor, mu_)
        calls.append(dict(grad_is_bucket=grad is net._last_grad_bucket, theta_is_flat=theta.data_ptr() == net.flat_theta().data_ptr(),
                          before=before, after=grad.clone(), mu=mu_))

    monkeypatch.setattr(_nvq, "fed_prox_grad", recorder)
    tr.train_round()
    assert len(calls) == 2 * 2                                          # 2 clients x 8 samples / batch 4: one per local step
    moved = False
    for c in calls:
        g0, th, an = c["before"]
        assert c["grad_is_bucket"] and c["theta_is_flat"] and c["mu"] == mu
        assert torch.equal(_bits(an), _bits(start))                     # the round-start weights
        moved |= bool((th != an).any())
        assert _within_ulps(c["after"], _t64(oracle.prox_grad(g0, th, an, mu)))
    assert moved                                                        # the second local step pulls back: theta has left the anchor


def test_trainer_round_with_both_options_reads_nothing_back():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=2, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                          server_optimizer="fedyogi", server_lr=1e-3, prox_mu=0.01, update_clip=1.0, update_noise=1e-4)
    for c in range(3):
        tr.set_client_data(c, _clips(8, 20 + c))
    tr.train_round()                                                    # warm-up: code objects loaded, buffers and state built
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


def test_trainer_robust_rule_with_a_server_optimizer_runs_on_the_device():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                          aggregator="median", server_optimizer="fedavgm", server_betas=(0.0, 0.99), update_noise=1e-4)
    ref_net = _sr_net()
    ref = FederatedTrainer(ref_net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                           aggregator="median", update_noise=1e-4)
    for c in range(3):
        tr.set_client_data(c, _clips(8, 10 + c, 0.05 * c))
        ref.set_client_data(c, _clips(8, 10 + c, 0.05 * c))
    tr.train_round()
    ref.train_round()
    # Momentum 0 towards the fp32 median agg from the snapshot: (float)(base + (agg - base)) plus the round's draw, where the plain
    # round writes agg plus the same draw.  agg - base is exact in double unless the exponents lie 29 bits apart, and then the
    # sum rounds back to agg: the same bits; one rounding, one ulp of the larger value, covers the rest.
    a, b = net.flat_theta(), ref_net.flat_theta()
    big = torch.maximum(a.abs(), b.abs())
    ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
    assert ((a.double() - b.double()).abs() <= ulp).all() and torch.isfinite(a).all()
    assert (a != _sr_net().flat_theta()).any()
    for (k, x), y in zip(net.state_dict().items(), ref_net.state_dict().values()):
        if k not in dict(net.named_parameters()):
            assert torch.equal(x, y), k                                 # statistics: the rule alone, as without the option


# ------------------------------------------------------------------------------------------------ the script
def test_train_federated_script_with_server_opt_and_prox(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_federated.py"),
           "--num-clients", "3", "--clients-per-round", "2", "--num-rounds", "2", "--local-epochs", "1", "--samples", "8",
           "--features", "16", "--blocks", "1", "--server-opt", "fedadam", "--server-lr", "1e-3", "--prox-mu", "0.01"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rounds = [ln for ln in r.stdout.splitlines() if ln.startswith("Round ")]
    assert len(rounds) == 2 and rounds[1].startswith("Round 2: 2 clients, 16 samples"), r.stdout
    for ln in rounds:
        assert np.isfinite(float(ln.split("loss")[1].split()[0].strip(":="))), ln
