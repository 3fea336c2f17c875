"""CPU: nerve_cl.federated.robust without a GPU - the ABI of csrc/robust.hip, the float64 torch compositions of the trimmed mean,
the median and Krum against plain numpy (np.sort, slice, mean, np.median), every refusal, and FederatedTrainer rounds with each
aggregator on a plain module."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _federated_oracle as oracle  # noqa: E402
from test_federated_cpu import _client_data, _small_net  # noqa: E402

ROBUST = ("median", "trimmed_mean", "krum", "multi_krum")


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_the_robust_symbols():
    from nerve_cl import _nvq
    header = open(os.path.join(os.path.dirname(HERE), "include", "nvq.h")).read()
    for name in ("nvq_fed_trimmed_aggregate", "nvq_fed_krum_select"):
        assert name + "(" in header and name in _nvq.SIGNATURES, name
    assert "#define NVQ_FED_TRIM_MEDIAN 64" in header and _nvq.FED_TRIM_MEDIAN == 64 >= (_nvq.FED_MAX_CLIENTS - 1) // 2
    import nerve_cl.federated as fed
    for name in ("aggregate_flat_trimmed", "aggregate_flat_median", "krum_select", "krum_aggregate_flat", "KrumResult"):
        assert name in fed.__all__ and hasattr(fed, name), name


# ------------------------------------------------------------------------------------------------ numpy yardsticks
def np_trimmed(x, trim, live=None, base=None, lr=1.0):
    """float64: base + lr * mean(np.sort(live rows)[t : m - t] - base), t = min(trim, (m - 1) // 2)"""
    x = np.asarray(x, dtype=np.float32)
    if live is not None:
        x = x[list(live)]
    m = len(x)
    t = min(trim, (m - 1) // 2)
    b = np.zeros(x.shape[1]) if base is None else np.asarray(base, dtype=np.float64)
    d = np.sort(x, axis=0).astype(np.float64)[t:m - t] - b
    return b + lr * d.mean(0)


def np_krum(G, f, q, live=None):
    """(scores, order, weights) of Krum from a float64 Gram matrix"""
    K = len(G)
    live = list(range(K)) if live is None else list(live)
    m = len(live)
    c = min(max(m - f - 2, 1), m - 1)
    diag = np.diag(G)
    with np.errstate(invalid="ignore"):
        D = np.maximum(diag[:, None] + diag[None, :] - 2 * G, 0.0)
    D[np.isnan(diag[:, None] + diag[None, :] - 2 * G)] = np.inf
    scores = np.full(K, np.inf)
    for i in live:
        scores[i] = np.sort(D[i, [j for j in live if j != i]])[:c].sum()
    ranked = sorted(live, key=lambda i: (np.isnan(scores[i]), scores[i], i))
    order = ranked + [k for k in range(K) if k not in live]
    w = np.zeros(K)
    w[ranked[:min(q, m)]] = 1.0
    return scores, np.array(order), w


def _rows(K, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(K, n, generator=g), torch.randn(n, generator=g)


# ------------------------------------------------------------------------------------------------ the compositions
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_trimmed_mean_cpu_against_numpy(K):
    from nerve_cl.federated import aggregate_flat_trimmed
    x, base = _rows(K, 37, 40 + K)
    for trim in (0, 1, (K - 1) // 2, 64):
        got = aggregate_flat_trimmed(x, trim)
        assert got.dtype == torch.float32
        want = np_trimmed(x.numpy(), trim)
        assert (np.abs(got.numpy() - want) <= oracle.ulp32(want)).all(), trim
        for lr in (1.0, 0.5):
            got = aggregate_flat_trimmed(x, trim, base=base, server_lr=lr)
            want = np_trimmed(x.numpy(), trim, base=base.numpy(), lr=lr)
            assert (np.abs(got.numpy() - want) <= oracle.ulp32(want)).all(), (trim, lr)
    out = base.clone()
    assert aggregate_flat_trimmed(x, 1, base=out, out=out) is out                  # out may be base
    assert torch.equal(out, aggregate_flat_trimmed(x, 1, base=base))


@pytest.mark.parametrize("K", [1, 3, 4, 7, 10])
def test_median_cpu_is_numpys(K):
    from nerve_cl.federated import aggregate_flat_median
    x, _ = _rows(K, 41, 50 + K)
    got = aggregate_flat_median(x).numpy()
    want = np.median(x.numpy().astype(np.float64), axis=0)
    if K % 2:
        assert np.array_equal(got, np.median(x.numpy(), axis=0))                   # the middle value itself
    assert (np.abs(got - want) <= oracle.ulp32(want)).all()


def test_live_rows_and_nan_order_cpu():
    from nerve_cl.federated import aggregate_flat, aggregate_flat_trimmed
    x, _ = _rows(5, 16, 7)
    poisoned = x.clone()
    poisoned[1] = float("nan")
    w = [2.0, 0.0, 3.0, 1.0, 4.0]
    got = aggregate_flat_trimmed(poisoned, 0, weights=w)                           # the zero-weight NaN row is not read
    assert torch.isfinite(got).all() and torch.equal(got, aggregate_flat_trimmed(x[[0, 2, 3, 4]], 0))
    assert torch.isnan(aggregate_flat(poisoned, w)).all()                          # FedAvg: 0 * NaN
    want = np_trimmed(poisoned.numpy(), 1)                                         # live: the NaN sorts last and is trimmed
    got = aggregate_flat_trimmed(poisoned, 1)
    assert np.isfinite(want).all() and (np.abs(got.numpy() - want) <= oracle.ulp32(want)).all()
    neg = poisoned.clone()
    neg[1] = torch.tensor(np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0])          # a NaN with the sign bit set
    assert torch.equal(aggregate_flat_trimmed(neg, 1), got)
    noisy = aggregate_flat_trimmed(x, 1, noise_std=0.25, seed=9, offset=4)
    assert np.abs((noisy - aggregate_flat_trimmed(x, 1)).numpy() - 0.25 * oracle.normals(9, 4, 16)).max() <= 1e-6


@pytest.mark.parametrize("K,f,q", [(3, 0, 1), (5, 1, 1), (5, 1, 4), (9, 3, 6), (9, 0, 9)])
def test_krum_cpu_against_numpy(K, f, q):
    from nerve_cl.federated import krum_aggregate_flat, krum_select, update_gram
    g = torch.Generator().manual_seed(60 + K + f)
    x = 0.05 * torch.randn(K, 33, generator=g) + 1.0
    for k in range(f):
        x[2 * k] = 20.0 * torch.randn(33, generator=g)                              # f far outliers
    base = torch.full((33,), 1.0)
    G = update_gram(x, base)
    res = krum_select(G, f, q)
    scores, order, w = np_krum(G.numpy(), f, q)
    assert np.allclose(res.scores.numpy(), scores, rtol=1e-12, atol=0)
    assert np.array_equal(res.order.numpy(), order) and np.array_equal(res.weights.numpy(), w)
    assert res.order.dtype == torch.int32 and res.weights.dtype == torch.float64
    assert not any(w[2 * k] for k in range(f))                                      # no outlier is chosen
    got = krum_aggregate_flat(x, f, q, base=base, server_lr=0.5)
    want = np_trimmed(x.numpy(), 0, live=np.flatnonzero(w), base=base.numpy(), lr=0.5)
    assert (np.abs(got.numpy() - want) <= oracle.ulp32(want)).all()
    live = [k for k in range(K) if k != 1]                                          # a zero-weight row of NaN is never chosen
    if len(live) >= f + 3:
        y = x.clone()
        y[1] = float("nan")
        wts = [0.0 if k == 1 else 2.0 for k in range(K)]
        res = krum_select(update_gram(y, base), f, q, weights=wts)
        scores, order, w = np_krum(update_gram(x, base).numpy(), f, q, live=live)
        assert np.array_equal(res.order.numpy(), order) and np.array_equal(res.weights.numpy(), w) and res.weights[1] == 0
        assert np.isinf(res.scores[1].item()) and np.isfinite(res.scores.numpy()[live]).all()
        assert torch.isfinite(krum_aggregate_flat(y, f, q, base=base, weights=wts)).all()


def test_krum_nan_row_is_never_selected_cpu():
    from nerve_cl.federated import krum_select, update_gram
    x, _ = _rows(6, 20, 3)
    x[4] = float("nan")
    res = krum_select(update_gram(x), 1, 5)
    assert res.weights[4] == 0 and res.order[-1] == 4 and res.weights.sum() == 5
    assert np.isfinite(res.scores.numpy()[[0, 1, 2, 3, 5]]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_errors():
    from nerve_cl.federated import (FederatedTrainer, aggregate_flat_median, aggregate_flat_trimmed, krum_aggregate_flat,
                                    krum_select, update_gram)
    x, base = _rows(4, 8, 1)
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(x, -1)
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(x.double(), 0)
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(torch.zeros(65, 4), 0)
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(x, 0, weights=[0.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        aggregate_flat_median(x, weights=[0.0, -1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(x, 0, weights=[1.0, 1.0])
    with pytest.raises(ValueError):
        aggregate_flat_trimmed(x, 0, base=base[:3])
    G = update_gram(x)
    with pytest.raises(ValueError):
        krum_select(G, 2)                                                          # m = 4 < f + 3
    with pytest.raises(ValueError):
        krum_select(G, 0, weights=[1.0, 1.0, 0.0, 0.0])                            # m = 2 < 3
    with pytest.raises(ValueError):
        krum_select(G, 0, weights=[0.0] * 4)
    with pytest.raises(ValueError):
        krum_select(G, -1)
    with pytest.raises(ValueError):
        krum_select(G, 0, 0)
    with pytest.raises(ValueError):
        krum_select(G.float(), 0)
    with pytest.raises(ValueError):
        krum_aggregate_flat(x, 2)
    net = _small_net()
    with pytest.raises(ValueError):
        FederatedTrainer(net, aggregator="mean")
    with pytest.raises(ValueError):
        FederatedTrainer(net, aggregator="trimmed_mean", trim_ratio=-0.1)
    with pytest.raises(ValueError):
        FederatedTrainer(net, aggregator="krum", num_byzantine=-1)
    with pytest.raises(ValueError):
        FederatedTrainer(net, aggregator="multi_krum", num_selected=0)
    for agg in ROBUST:
        with pytest.raises(NotImplementedError):
            FederatedTrainer(net, aggregator=agg, update_clip=1.0)
        with pytest.raises(NotImplementedError):
            FederatedTrainer(net, aggregator=agg, num_clusters=2)


def _trainer(model, **kw):
    from nerve_cl.federated import FederatedTrainer
    kw.setdefault("clients_per_round", 4)
    tr = FederatedTrainer(model, num_clients=4, local_epochs=2, lr=1e-2, batch_size=4, **kw)
    for c, d in _client_data().items():
        tr.set_client_data(c, d)
    return tr


def test_trainer_refuses_a_round_it_cannot_aggregate():
    model = _small_net()
    before = [v.clone() for v in model.state_dict().values()]
    for kw in (dict(aggregator="trimmed_mean", trim_ratio=0.5), dict(aggregator="krum", num_byzantine=2),
               dict(aggregator="multi_krum", clients_per_round=2)):
        with pytest.raises(ValueError):
            _trainer(model, seed=1, **kw).train_round()
    assert all(torch.equal(a, b) for a, b in zip(before, model.state_dict().values()))          # raised before any client trained


# ------------------------------------------------------------------------------------------------ the trainer
def _state(model):
    return [v.clone() for v in model.state_dict().values()]


def test_fedavg_aggregator_is_todays_trainer_bit_for_bit():
    from nerve_cl.federated import PrivacyConfig
    kw = dict(seed=77, privacy=PrivacyConfig(noise_multiplier=0.5), update_clip=0.5, update_noise=0.01, server_lr=0.5,
              clients_per_round=3)
    runs = []
    for extra in ({}, {"aggregator": "fedavg"}, {"aggregator": "fedavg", "after_client": None, "trim_ratio": 0.3, "num_byzantine": 1}):
        model = _small_net()
        tr = _trainer(model, **kw, **extra)
        outs = [tr.train_round() for _ in range(2)]
        runs.append((list(tr.last_selected), outs, _state(model)))
    for other in runs[1:]:
        assert other[0] == runs[0][0] and other[1] == runs[0][1]
        assert all(torch.equal(a, b) for a, b in zip(runs[0][2], other[2]))
    assert "selected_weights" not in runs[0][1][0]


@pytest.mark.parametrize("agg", ROBUST)
def test_trainer_round_per_aggregator_is_reproducible(agg):
    runs = []
    for _ in range(2):
        model = _small_net()
        tr = _trainer(model, seed=5, aggregator=agg, trim_ratio=0.25, num_byzantine=1, update_noise=0.01, server_lr=0.5)
        outs = [tr.train_round() for _ in range(2)]
        runs.append((list(tr.last_selected), outs, _state(model)))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert all(torch.isfinite(v.double()).all() for v in runs[0][2])
    out = runs[0][1][1]
    assert out["round"] == 2 and out["clients"] == 4 and np.isfinite(out["train_loss"])
    if agg in ("krum", "multi_krum"):
        sel = out["selected_weights"]
        assert isinstance(sel, list) and len(sel) == 4 and set(sel) <= {0.0, 1.0} and sum(sel) == (1 if agg == "krum" else 3)
    else:
        assert "selected_weights" not in out


def _rows_after_training(seed, hook):
    """the float state of every client after its local training in a first round with this seed, in the order of last_selected"""
    seen = []

    def record(cid, model):
        hook(cid, model)
        seen.append(torch.cat([v.detach().reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()]).clone())

    tr = _trainer(_small_net(), seed=seed, after_client=record)
    tr.train_round()
    return tr.last_selected, torch.stack(seen)


@pytest.mark.parametrize("kind", ["nan", "flip"])
def test_trainer_median_and_krum_hold_against_a_poisoned_client(kind):
    start = torch.cat([v.reshape(-1).float() for v in _small_net().state_dict().values() if v.is_floating_point()])
    calls = []

    def poison(cid, model, calls=calls):
        calls.append(cid)
        if cid != 2:
            return
        off = 0
        for v in model.state_dict().values():
            if v.is_floating_point():
                g = start[off:off + v.numel()].view(v.shape)
                v.copy_(torch.full_like(v, float("nan")) if kind == "nan" else g - 10.0 * (v - g))
                off += v.numel()

    selected, rows = _rows_after_training(5, poison)
    assert sorted(selected) == [0, 1, 2, 3] and calls == selected
    honest = rows[[k for k, c in enumerate(selected) if c != 2]]
    lo, hi = honest.min(0).values, honest.max(0).values
    results = {}
    for agg in ("fedavg", "median", "krum"):
        model = _small_net()
        tr = _trainer(model, seed=5, aggregator=agg, num_byzantine=1, after_client=poison)
        out = tr.train_round()
        assert tr.last_selected == selected
        results[agg] = torch.cat([v.reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()])
        if agg == "krum":
            assert out["selected_weights"][selected.index(2)] == 0.0 and sum(out["selected_weights"]) == 1.0
    for agg in ("median", "krum"):
        assert torch.isfinite(results[agg]).all(), agg
        assert ((results[agg] >= lo) & (results[agg] <= hi)).all(), agg             # inside the honest clients' range
    bad = results["fedavg"]
    assert torch.isnan(bad).any() or ((bad < lo) | (bad > hi)).any()                # the poison is real
