"""CPU: nerve_cl.federated without a GPU - the host Philox stream against the Random123 known answers, the privacy formulas and
the per-tensor DP step against values recorded from the reference (tests/golden/federated_privacy.npz, written by
tools/make_federated_fixtures.py), FedAvg against the float64 formula, and FederatedTrainer on a plain module against
independently trained deep copies."""
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
import _federated_oracle as oracle  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "federated_privacy.npz")


def _hex(words):
    return " ".join("%08x" % int(np.asarray(w).reshape(-1)[0]) for w in words)


def _h(s):
    return [int(x, 16) for x in s.split()]


KAT = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("counter,key,want", KAT)
def test_oracle_reproduces_the_random123_known_answers(counter, key, want):
    assert _hex(oracle.philox(_h(counter), _h(key))) == want


def test_oracle_normals_are_standard_normal():
    n = 1 << 20
    z = oracle.normals(20240607, 3, n)
    assert np.isfinite(z).all()
    assert abs(z.mean()) <= 6 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 6 * np.sqrt(2 / n), z.var()


# ------------------------------------------------------------------------------------------------ the package against it
@pytest.mark.parametrize("counter,key,want", KAT)
def test_package_philox_known_answers(counter, key, want):
    from nerve_cl.federated import _philox
    assert _hex(_philox.philox4x32_10(np.array(_h(counter)), np.array(_h(key)))) == want


@pytest.mark.parametrize("seed,offset,n", [(0, 0, 1), (5, 7, 6), ((1 << 61) + 12345, (1 << 40) + 9, 1025)])
def test_package_normals_equal_the_oracle(seed, offset, n):
    from nerve_cl.federated import _philox
    assert np.array_equal(_philox.normals(seed, offset, n), oracle.normals(seed, offset, n))
    assert np.array_equal(_philox.normals(seed, offset, 3, first=2), oracle.normals(seed, offset, 5)[2:])


def test_privacy_formulas_match_the_reference_values():
    from nerve_cl.federated import PrivacyConfig, compute_noise_multiplier, get_privacy_spent
    f = np.load(GOLDEN)
    for (e, d, q, n), want in zip(f["noise_args"], f["noise_values"]):
        assert compute_noise_multiplier(e, d, q, int(n)) == pytest.approx(want, rel=1e-12)
    for (s, m, q, d), want in zip(f["spent_args"], f["spent_values"]):
        assert get_privacy_spent(int(s), m, q, d) == pytest.approx(want, rel=1e-12)
    c = PrivacyConfig()
    assert (c.epsilon, c.delta, c.max_grad_norm, c.noise_multiplier) == (8.0, 1e-5, 1.0, 1.0)


def golden_model(f):
    """the small model of tools/make_federated_fixtures.py with the recorded initial weights"""
    model = nn.Sequential(nn.Conv2d(3, 5, 3, padding=1), nn.ReLU(), nn.Conv2d(5, 3, 3, padding=1, bias=False), nn.Flatten(),
                          nn.Linear(3 * 6 * 6, 7))
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(f["w0/" + n]))
    return model


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_dp_optimizer_without_noise_reproduces_the_reference_clipping():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig
    f = np.load(GOLDEN)
    model = golden_model(f)
    cfg = PrivacyConfig(max_grad_norm=float(f["max_grad_norm"]), noise_multiplier=0.0)
    dp = DPOptimizer(torch.optim.SGD(model.parameters(), lr=float(f["sgd_lr"])), model, cfg, int(f["batch_size"]), 60, seed=1)
    dp.zero_grad()
    nn.functional.mse_loss(model(torch.from_numpy(f["x"])), torch.from_numpy(f["y"])).backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    for n, g in grads.items():
        assert _rel(g.numpy(), f["g/" + n]) <= 1e-6, n
    dp.step()
    assert dp.steps == 1 and dp.sample_rate == int(f["batch_size"]) / 60
    for n, p in model.named_parameters():
        assert _rel(grads[n].numpy(), f["clipped/" + n]) <= 1e-6, n
        assert _rel(p.detach().numpy(), f["w1/" + n]) <= 1e-6, n


def test_dp_optimizer_noise_is_the_oracle_stream():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig
    f = np.load(GOLDEN)
    model = golden_model(f)
    C, B, seed = float(f["max_grad_norm"]), int(f["batch_size"]), 991
    cfg = PrivacyConfig(max_grad_norm=C, noise_multiplier=1.5)
    dp = DPOptimizer(torch.optim.SGD(model.parameters(), lr=0.0), model, cfg, B, 60, seed=seed)
    names = [n for n, _ in model.named_parameters()]
    offs, total = oracle.padded_layout([int(np.prod(f["g/" + n].shape)) for n in names])
    for step in range(2):                                     # offset = the step count: fresh noise every step
        dp.zero_grad()
        nn.functional.mse_loss(model(torch.from_numpy(f["x"])), torch.from_numpy(f["y"])).backward()
        dp.step()
        z = oracle.normals(seed, step, total)
        for (n, p), o in zip(model.named_parameters(), offs):
            want = f["clipped/" + n].astype(np.float64) + 1.5 * C / B * z[o:o + p.numel()].reshape(p.shape)
            assert np.abs(p.grad.numpy() - want).max() <= 1e-6 * np.abs(want).max() + 1e-7, (step, n)


def test_make_private_is_the_simple_optimizer():
    from nerve_cl.federated import DPOptimizer, PrivacyConfig, make_private
    model = nn.Linear(3, 2)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.zeros(10, 3), torch.zeros(10, 2)), batch_size=5)
    m, dp, ld = make_private(model, opt, loader, PrivacyConfig())
    assert m is model and ld is loader and isinstance(dp, DPOptimizer) and dp.optimizer is opt
    assert dp.batch_size == 5 and dp.sample_rate == 0.5 and dp.steps == 0


# ------------------------------------------------------------------------------------------------ aggregation
def _rows(K, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(K, n, generator=g), torch.randn(n, generator=g)


def test_aggregate_flat_cpu_against_the_formula():
    from nerve_cl.federated import aggregate_flat
    x, base = _rows(4, 37, 3)
    x[2] = base                                                # an unchanged client: norm 0, coefficient 1
    x[3] = base + 10.0                                         # far above the bound
    w = [3.0, 0.0, 5.0, 2.0]
    got = aggregate_flat(x, w)
    assert got.dtype == torch.float32
    assert np.abs(got.numpy() - oracle.aggregate(x.numpy(), w)).max() <= 1e-6
    poisoned = x.clone()
    poisoned[1] = 1e6                                          # a zero-weight client contributes nothing
    assert torch.equal(aggregate_flat(poisoned, w), got)
    for lr in (1.0, 0.5):
        got = aggregate_flat(x, w, base=base, clip_norm=1.0, server_lr=lr)
        want = oracle.aggregate(x.numpy(), w, base.numpy(), 1.0, lr)
        assert (np.abs(got.numpy() - want) <= oracle.ulp32(want)).all()
    noisy = aggregate_flat(x, w, base=base, noise_std=0.25, seed=9, offset=4)
    plain = aggregate_flat(x, w, base=base)
    assert np.abs((noisy - plain).numpy() - 0.25 * oracle.normals(9, 4, 37)).max() <= 1e-6
    out = base.clone()
    assert aggregate_flat(x, w, base=out, clip_norm=1.0, out=out) is out            # out may be base
    assert torch.equal(out, aggregate_flat(x, w, base=base, clip_norm=1.0))


def test_all_zero_weights_raise():
    from nerve_cl.federated import aggregate_flat, fedavg
    x, _ = _rows(2, 8, 1)
    with pytest.raises(ValueError):
        aggregate_flat(x, [0.0, 0.0])
    with pytest.raises(ValueError):
        fedavg([{"w": x[0]}, {"w": x[1]}], [0, 0])


def test_fedavg_state_dicts_and_integer_buffers():
    from nerve_cl.federated import fedavg
    torch.manual_seed(0)
    nets = [nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4)) for _ in range(3)]
    for i, net in enumerate(nets):
        net[1].num_batches_tracked.fill_([7, 2, 4][i])
    counts = [1, 2, 4]
    avg = fedavg([n.state_dict() for n in nets], counts)
    assert list(avg) == list(nets[0].state_dict())
    w = np.array(counts, dtype=np.float64)
    for k, v in avg.items():
        stack = np.stack([n.state_dict()[k].double().numpy() for n in nets])
        want = (stack * w.reshape(-1, *([1] * (stack.ndim - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert v.dtype == torch.float32 and (np.abs(v.numpy() - want) <= oracle.ulp32(want)).all(), k
        else:
            assert v.dtype == torch.int64 and int(v) == int(np.trunc(want)) == 3, k      # (7 + 4 + 16) / 7 = 3.857 -> 3


def test_get_and_set_parameters_round_trip():
    from nerve_cl.federated import get_parameters, set_parameters
    torch.manual_seed(1)
    a, b = (nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4)) for _ in range(2))
    a[1].num_batches_tracked.fill_(5)
    params = get_parameters(a)
    assert all(isinstance(p, np.ndarray) for p in params) and len(params) == len(a.state_dict())
    ptrs = [p.data_ptr() for p in b.parameters()]
    set_parameters(b, params)
    assert [p.data_ptr() for p in b.parameters()] == ptrs                           # copied in place
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(va, vb), k
    with pytest.raises(ValueError):
        set_parameters(b, params[:-1])


def test_weighted_average_and_server_without_flwr():
    from nerve_cl.federated import start_server, weighted_average
    assert weighted_average([(1, {"loss": 4.0}), (3, {"loss": 0.0})]) == {"loss": 1.0}
    try:
        import flwr  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="flwr"):
            start_server(nn.Linear(1, 1))


def test_client_works_without_flwr():
    from nerve_cl.federated import VideoEnhancementClient, create_client, get_parameters
    torch.manual_seed(2)
    model = nn.Linear(4, 2)
    client = create_client(0, model, (torch.randn(12, 4), torch.randn(12, 2)), (torch.randn(6, 4), torch.randn(6, 2)),
                           local_epochs=2, learning_rate=1e-2)
    assert isinstance(client, VideoEnhancementClient)
    start = get_parameters(model)
    params, seen, metrics = client.fit(start, {})
    assert seen == 24 and np.isfinite(metrics["train_loss"]) and any((a != b).any() for a, b in zip(params, start))
    loss, n, m = client.evaluate(params, {})
    assert n == 6 and m["val_loss"] == loss and np.isfinite(loss)


# ------------------------------------------------------------------------------------------------ the trainer
def _small_net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.BatchNorm1d(7), nn.ReLU(), nn.Linear(7, 3))


def _client_data():
    g = torch.Generator().manual_seed(11)
    return {c: (torch.randn(6 + 2 * c, 5, generator=g) + 0.1 * c, torch.randn(6 + 2 * c, 3, generator=g)) for c in range(4)}


def _trainer(model, **kw):
    from nerve_cl.federated import FederatedTrainer
    tr = FederatedTrainer(model, num_clients=4, clients_per_round=3, local_epochs=2, lr=1e-2, batch_size=4, **kw)
    for c, d in _client_data().items():
        tr.set_client_data(c, d)
    return tr


def test_trainer_round_equals_the_mean_of_independently_trained_copies():
    model = _small_net()
    start = copy.deepcopy(model)
    tr = _trainer(model, seed=5)
    out = tr.train_round()
    sel = tr.last_selected
    data = _client_data()
    assert set(out) >= {"round", "clients", "samples", "train_loss"}
    assert out["round"] == 1 and out["clients"] == 3 and out["samples"] == sum(len(data[c][0]) for c in sel)
    assert np.isfinite(out["train_loss"]) and len(set(sel)) == 3 and tr.global_round == 1
    states = []
    for c in sel:
        m = copy.deepcopy(start).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
        xs, ys = data[c]
        for _ in range(2):
            for i in range(0, len(xs), 4):
                opt.zero_grad()
                nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4]).backward()
                opt.step()
        states.append(m.state_dict())
    w = np.array([len(data[c][0]) for c in sel], dtype=np.float64)
    for k, v in model.state_dict().items():
        stack = np.stack([s[k].double().numpy() for s in states])
        want = (stack * w.reshape(-1, *([1] * (stack.ndim - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert (np.abs(v.numpy() - want) <= oracle.ulp32(want)).all(), k
        else:
            assert int(v) == int(np.trunc(want)), k


def test_trainer_seed_fixes_selection_and_weights():
    runs = []
    for _ in range(2):
        model = _small_net()
        from nerve_cl.federated import PrivacyConfig
        tr = _trainer(model, seed=77, privacy=PrivacyConfig(noise_multiplier=0.5), update_clip=0.5, update_noise=0.01, server_lr=0.5)
        outs = [tr.train_round() for _ in range(2)]
        runs.append((list(tr.last_selected), outs, [v.clone() for v in model.state_dict().values()]))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert runs[0][1][1]["round"] == 2


def test_abi_declares_the_federated_symbols():
    from nerve_cl import _nvq
    header = open(os.path.join(os.path.dirname(HERE), "include", "nvq.h")).read()
    for name in ("nvq_fed_workspace_bytes", "nvq_fed_delta_norms", "nvq_fed_aggregate", "nvq_dp_segment_norms", "nvq_dp_clip_noise"):
        assert name + "(" in header and name in _nvq.SIGNATURES, name
    import nerve_cl
    assert nerve_cl.FederatedTrainer is nerve_cl.federated.FederatedTrainer
