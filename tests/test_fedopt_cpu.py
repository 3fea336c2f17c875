"""CPU: nerve_cl.federated.fedopt (ServerOptimizer, prox_grad_) and FederatedTrainer's server_optimizer / prox_mu on CPU tensors
against the float64 oracle of tests/_fedopt_oracle.py.  One criterion for values: within one fp32 ulp of the float64 value (the
stored values are a float64 chain rounded once).  Every round is teacher-forced from the state the code under test holds."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _fedopt_oracle as oracle  # noqa: E402

LR, BETAS, TAU = 0.1, (0.9, 0.99), 1e-3


def _matrix(K, n, seed):
    """the generator of test_federated_gpu._matrix on the CPU: randn rows, base = their mean + 0.1 randn; weights 1 .. K"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(K, n, generator=g)
    base = vals.mean(0) + 0.1 * torch.randn(n, generator=g)
    return vals, base, [float(k + 1) for k in range(K)]


def _state(opt, rule, n):
    if opt.m is None:
        return oracle.initial_state(rule, n, TAU)
    return opt.m.clone(), None if opt.v is None else opt.v.clone()


@pytest.mark.parametrize("clip", [None, 2.0])
@pytest.mark.parametrize("n,K", [(5, 2), (1023, 5)])
@pytest.mark.parametrize("rule", oracle.RULES)
def test_server_optimizer_on_cpu_tensors(rule, n, K, clip):
    from nerve_cl.federated import ServerOptimizer
    opt = ServerOptimizer(rule, lr=LR, betas=BETAS, tau=TAU)
    base = None
    for rnd in range(2):
        clients, b0, weights = _matrix(K, n, 100 * rnd + n % 89 + K)
        base = b0 if base is None else base                          # round 2 starts from round 1's result
        m, v = _state(opt, rule, n)
        D = oracle.pseudo_gradient(clients, base, weights, clip)
        if rule == "fedyogi":
            assert oracle.yogi_margin(D, v) > 1e-9
        want, m1, v1 = oracle.server_step(rule, D, base, m, v, LR, BETAS, TAU)
        out = opt.step(clients, weights, base, clip_norm=clip)
        assert out.dtype == torch.float32 and out is not base
        assert oracle.within_ulps(out, want), (rule, rnd)
        assert oracle.within_ulps(opt.m, m1), (rule, rnd)
        if rule == "fedavgm":
            assert opt.v is None
        else:
            assert oracle.within_ulps(opt.v, v1), (rule, rnd)
        base = out
    assert (opt.m != 0).any()


def test_adaptive_state_starts_at_tau_squared():
    from nerve_cl.federated import ServerOptimizer
    clients, base, weights = _matrix(2, 5, 1)
    opt = ServerOptimizer("fedadam", lr=LR, tau=TAU)
    opt.step(base.repeat(2, 1), weights, base)                        # D = 0: v' = beta2 v, out = base
    assert oracle.within_ulps(opt.v, np.full(5, oracle.f32(0.99) * float(np.float32(oracle.f32(TAU) ** 2))))


@pytest.mark.parametrize("clip", [None, 2.0])
@pytest.mark.parametrize("lr", [1.0, 0.5])
def test_fedavgm_without_momentum_is_aggregate_flat_to_the_bit(lr, clip):
    from nerve_cl.federated import ServerOptimizer, aggregate_flat
    clients, base, weights = _matrix(5, 1023, 9)
    opt = ServerOptimizer("fedavgm", lr=lr, betas=(0.0, 0.99))
    for rnd in range(2):                                              # the second round: m is not zero any more
        kw = dict(clip_norm=clip, noise_std=0.01, seed=77, offset=rnd)
        got = opt.step(clients, weights, base, **kw)
        want = aggregate_flat(clients, weights, base=base, server_lr=lr, **kw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rnd
        base = got


@pytest.mark.parametrize("rule", oracle.RULES)
def test_state_dict_round_trip_continues_the_trajectory(rule):
    from nerve_cl.federated import ServerOptimizer
    rounds = [_matrix(3, 37, 40 + r) for r in range(3)]

    def run(opt, base, rs):
        for clients, _, weights in rs:
            base = opt.step(clients, weights, base)
        return base

    a = ServerOptimizer(rule, lr=LR, betas=(0.8, 0.95), tau=2e-3)
    full = run(a, rounds[0][1], rounds)
    b = ServerOptimizer(rule, lr=LR, betas=(0.8, 0.95), tau=2e-3)
    mid = run(b, rounds[0][1], rounds[:1])
    state = b.state_dict()
    assert state["rule"] == rule and state["betas"] == (0.8, 0.95) and state["tau"] == 2e-3 and state["lr"] == LR
    assert state["m"] is not b.m and torch.equal(state["m"], b.m) and (state["v"] is None) == (rule == "fedavgm")
    c = ServerOptimizer("fedavgm")                                    # everything comes from the state
    c.load_state_dict(state)
    b.m.zero_()                                                       # the loaded state is a copy
    got = run(c, mid, rounds[1:])
    assert torch.equal(got.view(torch.int32), full.view(torch.int32))
    assert torch.equal(c.m, a.m) and (rule == "fedavgm" or torch.equal(c.v, a.v))


def test_prox_grad_on_cpu_tensors():
    from nerve_cl.federated import prox_grad_
    g = torch.Generator().manual_seed(3)
    n, mu = 1023, 0.01
    grad, theta, anchor = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    theta0, anchor0 = theta.clone(), anchor.clone()
    want = oracle.prox_grad(grad, theta, anchor, mu)
    ret = prox_grad_(grad, theta, anchor, mu)
    assert ret is grad and oracle.within_ulps(grad, want)
    assert torch.equal(theta, theta0) and torch.equal(anchor, anchor0)
    before = grad.clone()
    prox_grad_(grad, theta, anchor, 0.0)
    assert torch.equal(grad.view(torch.int32), before.view(torch.int32))
    shaped = torch.zeros(3, 4)                                        # a parameter's shape is fine on the CPU
    prox_grad_(shaped, torch.ones(3, 4), torch.zeros(3, 4), 0.5)
    assert torch.equal(shaped, torch.full((3, 4), 0.5))


# ------------------------------------------------------------------------------------------------ the trainer
def _small_net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.BatchNorm1d(7), nn.ReLU(), nn.Linear(7, 3))


def _client_data():
    g = torch.Generator().manual_seed(11)
    return {c: (torch.randn(6 + 2 * c, 5, generator=g) + 0.1 * c, torch.randn(6 + 2 * c, 3, generator=g)) for c in range(4)}


def _trainer(model, **kw):
    from nerve_cl.federated import FederatedTrainer
    tr = FederatedTrainer(model, num_clients=4, clients_per_round=3, local_epochs=2, lr=1e-2, batch_size=4, seed=5, **kw)
    for c, d in _client_data().items():
        tr.set_client_data(c, d)
    return tr


def _hand_trained(start, selected, mu=0.0):
    """the clients' state dicts after local training from ``start``, the way the trainer trains them (FedProx by autograd)"""
    data, states = _client_data(), []
    anchor = [p.detach().clone() for p in start.parameters()]
    for c in selected:
        m = copy.deepcopy(start).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
        xs, ys = data[c]
        for _ in range(2):
            for i in range(0, len(xs), 4):
                opt.zero_grad()
                loss = nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4])
                if mu:
                    loss = loss + 0.5 * mu * sum((p - a).pow(2).sum() for p, a in zip(m.parameters(), anchor))
                loss.backward()
                opt.step()
        states.append(m.state_dict())
    return states, np.array([len(data[c][0]) for c in selected], dtype=np.float64)


def _check_statistics(model, states, w):
    for k, v in model.state_dict().items():
        if k in dict(model.named_parameters()):
            continue
        stack = np.stack([s[k].double().numpy() for s in states])
        mean = (stack * w.reshape(-1, *([1] * (stack.ndim - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert oracle.within_ulps(v, mean), k                     # running_mean / running_var: the plain weighted mean
        else:
            assert int(v) == int(np.trunc(mean)), k                   # num_batches_tracked: the truncated mean


def test_trainer_fedadam_steps_parameters_and_averages_statistics():
    model = _small_net()
    start = copy.deepcopy(model)
    tr = _trainer(model, server_optimizer="fedadam", server_lr=1e-2, server_betas=BETAS, server_tau=TAU)
    out = tr.train_round()
    assert out["round"] == 1 and out["clients"] == 3 and np.isfinite(out["train_loss"])
    states, w = _hand_trained(start, tr.last_selected)
    params = dict(model.named_parameters())
    for k, p in params.items():
        clients = torch.stack([s[k].reshape(-1) for s in states])
        base = start.state_dict()[k].reshape(-1)
        m, v = oracle.initial_state("fedadam", base.numel(), TAU)
        D = oracle.pseudo_gradient(clients, base, w)
        want, _, _ = oracle.server_step("fedadam", D, base, m, v, 1e-2, BETAS, TAU)
        assert (np.abs(want - oracle.np64(base)) > 1e-3).any(), k     # an Adam step: about server_lr per coordinate
        assert oracle.within_ulps(p.detach().reshape(-1), want), k
    _check_statistics(model, states, w)
    # parameters first, each at a multiple of 4 floats; the server state covers exactly them
    plan, sd = tr._plan, model.state_dict()
    n_params = sum((p.numel() + 3) // 4 * 4 for p in params.values())
    assert plan["n_params"] == n_params
    assert [t.data_ptr() for t in plan["pack"].tensors] == ([sd[k].data_ptr() for k in params] +
                                                            [t.data_ptr() for k, t in sd.items() if k not in params and t.is_floating_point()])
    state = tr.server_state_dict()
    assert state["server_optimizer"] == "fedadam" and len(state["states"]) == 1 and state["states"][0]["m"].numel() == n_params
    # the state continues in another trainer: the second round is the same to the bit
    other = _small_net()
    other.load_state_dict(model.state_dict())
    tr2 = _trainer(other, server_optimizer="fedadam", server_lr=1e-2, server_betas=BETAS, server_tau=TAU)
    tr2.load_server_state_dict(state)
    tr2._rng.setstate(tr._rng.getstate())
    tr2.global_round = tr.global_round
    tr.train_round()
    tr2.train_round()
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))


def test_trainer_without_server_optimizer_packs_in_state_dict_order():
    model = _small_net()
    tr = _trainer(model)
    tr.train_round()
    sd = model.state_dict()
    assert tr._plan["n_params"] == 0 and tr.server_state_dict()["states"] == []
    assert [t.data_ptr() for t in tr._plan["pack"].tensors] == [t.data_ptr() for t in sd.values() if t.is_floating_point()]


def test_trainer_robust_rule_then_the_single_row_server_step():
    model = _small_net()
    start = copy.deepcopy(model)
    tr = _trainer(model, aggregator="median", server_optimizer="fedyogi", server_lr=1e-2, server_betas=BETAS, server_tau=TAU)
    tr.train_round()
    states, w = _hand_trained(start, tr.last_selected)
    for k, p in model.named_parameters():
        base = start.state_dict()[k].reshape(-1)
        b = oracle.np64(base)
        med = np.median(np.stack([oracle.np64(s[k].reshape(-1)) for s in states]), axis=0)
        agg = (b + (med - b)).astype(np.float32)                      # the rule alone, rounded to fp32: what the kernel steps towards
        m, v = oracle.initial_state("fedyogi", base.numel(), TAU)
        D = oracle.pseudo_gradient(agg[None], base, [1.0])
        assert oracle.yogi_margin(D, v) > 1e-9
        want, _, _ = oracle.server_step("fedyogi", D, base, m, v, 1e-2, BETAS, TAU)
        assert oracle.within_ulps(p.detach().reshape(-1), want), k


def test_trainer_prox_mu_is_the_proximal_term():
    """prox_mu on a CPU module is one add_ per parameter: the round equals clients trained with mu / 2 |theta - theta_round|^2 in
    their loss.  Autograd forms that gradient in fp32 in another order: a few ulps (1e-7 relative) of a gradient change an AdamW
    step of lr = 1e-2 by about 1e-9, so 1e-4, a hundredth of one step, is far above rounding and far below a missing or doubled
    term, which moves the weights by more than 1e-3 (asserted on the round without the term)."""
    mu = 0.5
    model = _small_net()
    start = copy.deepcopy(model)
    tr = _trainer(model, prox_mu=mu)
    tr.train_round()
    states, w = _hand_trained(start, tr.last_selected, mu)
    plain, _ = _hand_trained(start, tr.last_selected, 0.0)

    def mean(sts, k):
        return sum(wk * s[k].double() for wk, s in zip(w, sts)) / w.sum()

    gap = 0.0
    for k, p in model.named_parameters():
        assert (p.detach().double() - mean(states, k)).abs().max() <= 1e-4, k
        gap = max(gap, float((p.detach().double() - mean(plain, k)).abs().max()))
    assert gap > 1e-3


def test_trainer_defaults_are_bit_identical_to_no_options():
    a, b = _small_net(), _small_net()
    ta, tb = _trainer(a), _trainer(b, server_optimizer=None, prox_mu=0.0)
    for _ in range(2):
        ta.train_round()
        tb.train_round()
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def test_refusals():
    from nerve_cl.federated import SERVER_OPTIMIZERS, FederatedTrainer, ServerOptimizer, prox_grad_
    assert SERVER_OPTIMIZERS == ("fedavgm", "fedadagrad", "fedadam", "fedyogi")
    for kw in (dict(rule="adam"), dict(rule="fedadam", betas=(1.0, 0.99)), dict(rule="fedadam", betas=(0.9, -0.1)),
               dict(rule="fedadam", betas=(0.9,)), dict(rule="fedyogi", tau=0.0), dict(rule="fedyogi", tau=-1.0)):
        with pytest.raises(ValueError):
            ServerOptimizer(**kw)
    for kw in (dict(server_optimizer="adam"), dict(server_optimizer="fedadam", server_betas=(0.9, 1.0)),
               dict(server_optimizer="fedyogi", server_tau=0.0), dict(prox_mu=-0.1), dict(prox_mu=float("nan"))):
        with pytest.raises(ValueError):
            FederatedTrainer(_small_net(), **kw)
    with pytest.raises(NotImplementedError):
        FederatedTrainer(_small_net(), server_optimizer="fedadam", num_clusters=2)
    with pytest.raises(ValueError):
        prox_grad_(torch.zeros(4), torch.zeros(4), torch.zeros(4), -1.0)
    opt = ServerOptimizer("fedadam")
    clients, base, weights = _matrix(2, 5, 1)
    with pytest.raises(ValueError):
        opt.step(clients, weights, None)                              # the server step starts from the round's weights
    opt.step(clients, weights, base)
    with pytest.raises(ValueError):
        opt.step(clients[:, :4].contiguous(), weights, base[:4])      # another size than the state


def test_abi_declares_the_fedopt_symbols():
    from nerve_cl import _nvq
    header = open(os.path.join(os.path.dirname(HERE), "include", "nvq.h")).read()
    for name in ("nvq_fed_server_opt", "nvq_fed_prox_grad"):
        assert name + "(" in header and name in _nvq.SIGNATURES, name
    for k, name in enumerate(("AVGM", "ADAGRAD", "ADAM", "YOGI")):
        assert f"#define NVQ_FED_OPT_{name} {k}" in header and getattr(_nvq, "FED_OPT_" + name) == k
