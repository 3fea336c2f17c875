"""CPU: nerve_cl.federated.compression (compress_updates_, topk_count, wire_bytes) and FederatedTrainer's compression on CPU tensors
against the float64 oracle of tests/_compress_oracle.py.  One criterion for values: equality (every step of the contract is a
single correctly rounded operation, so there is nothing to tolerate); -0 equals +0 and NaN stands exactly where the oracle's does."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _compress_oracle as oracle  # noqa: E402

LEVELS = (0, 1, 127, 32767)


def k_values(n):
    """none, 1, 2, n // 2, n - 1, n, n + 5, without the values below 1 and without repeats"""
    out = [None]
    for k in (1, 2, n // 2, n - 1, n, n + 5):
        if k >= 1 and k not in out:
            out.append(k)
    return out


def make_case(K, n, seed, rows=None):
    """clients, base and a residual matrix of `rows` rows (default K) as float32 numpy arrays from a seeded generator"""
    g = np.random.default_rng(seed)
    clients = g.standard_normal((K, n)).astype(np.float32)
    base = (clients.mean(0) + 0.1 * g.standard_normal(n)).astype(np.float32)
    residual = (0.3 * g.standard_normal((rows or K, n))).astype(np.float32)
    return clients, base, residual


@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_cpu_path_equals_the_oracle(n, K):
    from nerve_cl.federated import compress_updates_
    clients, base, residual = make_case(K, n, 1000 * K + n)
    case = 0
    for k in k_values(n):
        for levels in LEVELS:
            case += 1                                                   # residual x base: two of the four per (k, levels), in turn
            for has_res, has_base in (((True, True), (False, False)) if case % 2 else ((True, False), (False, True))):
                b = base if has_base else None
                want_x, want_e, want_kept = oracle.compress(clients, b, k, levels, residual if has_res else None, seed=7, offset=3 + case)
                x, e = torch.from_numpy(clients.copy()), torch.from_numpy(residual.copy()) if has_res else None
                kept = compress_updates_(x, None if b is None else torch.from_numpy(b), k=k, levels=levels, residual=e, seed=7,
                                         offset=3 + case)
                what = (n, K, k, levels, has_res, has_base)
                assert kept.dtype == torch.int32 and kept.tolist() == want_kept.tolist(), what
                assert oracle.same(x.numpy(), want_x), what
                if has_res:
                    assert oracle.same(e.numpy(), want_e), what
                if k is not None and k < n:
                    assert (want_kept >= k).all() and (want_kept == k).all(), what     # continuous draws: no ties
                else:
                    assert (want_kept == n).all(), what


def test_cpu_path_slots_strides_ties_and_special_values():
    from nerve_cl.federated import compress_updates_
    K, n, M = 3, 37, 5
    clients, base, residual = make_case(K, n, 5, rows=M)
    base = np.round(base * 4) / 4                                       # multiples of 1/4: row 0's update is exact, so it has ties
    clients[0] = np.random.default_rng(1).choice(np.array([0, 0.5, -0.5, 1, -1, 2, -2], dtype=np.float32), n) + base
    residual[4] = 0
    clients[1, 4], clients[2, 9], clients[2, 11] = np.nan, np.inf, -np.inf
    slots = [4, 0, 2]
    want_x, want_e, want_kept = oracle.compress(clients, base, 7, 127, residual, slots, seed=1, offset=2)
    wide = torch.zeros(K, n + 3)
    wide[:, :n] = torch.from_numpy(clients)
    x, e = wide[:, :n], torch.from_numpy(residual.copy())
    kept = compress_updates_(x, torch.from_numpy(base), k=7, levels=127, residual=e, slots=slots, seed=1, offset=2)
    assert kept.tolist() == want_kept.tolist() and oracle.same(x.numpy(), want_x) and oracle.same(e.numpy(), want_e)
    assert (wide[:, n:] == 0).all()
    assert np.array_equal(e.numpy()[[1, 3]].view(np.uint32), residual[[1, 3]].view(np.uint32))     # rows no slot names
    assert np.isnan(x.numpy()[1, 4]) and e[0, 4] == 0 and e[2, 9] == 0 and e[2, 11] == 0
    assert kept[0] > 7 and kept[1] == 7 and kept[2] == 7                 # ties are kept; NaN and the infinities are kept first
    assert torch.isnan(x[1, 4]) and torch.isinf(x[2, [9, 11]]).all()


def test_argument_errors():
    from nerve_cl.federated import compress_updates_
    x, res = torch.zeros(2, 8), torch.zeros(3, 8)
    for kw in (dict(k=0), dict(k=-1), dict(k=1.5), dict(levels=-1), dict(levels=32768), dict(slots=[0, 1]),
               dict(residual=res, slots=[0, 0]), dict(residual=res, slots=[0, 3]), dict(residual=res, slots=[0, -1]),
               dict(residual=res, slots=[0]), dict(residual=res.double()), dict(residual=torch.zeros(3, 7)),
               dict(residual=torch.zeros(1, 8)), dict(seed=-1), dict(offset=-1)):
        with pytest.raises(ValueError):
            compress_updates_(x.clone(), **kw)
    with pytest.raises(ValueError):
        compress_updates_(torch.zeros(2, 8, dtype=torch.float64), k=1)
    with pytest.raises(ValueError):
        compress_updates_(torch.zeros(8), k=1)
    with pytest.raises(ValueError):
        compress_updates_(x.clone(), torch.zeros(7), k=1)
    kept = compress_updates_(x.clone())                                 # the valid no-op
    assert kept.tolist() == [8, 8]


def test_topk_count_and_wire_bytes():
    from nerve_cl.federated import topk_count, wire_bytes
    assert [topk_count(n, r) for n, r in ((1000, 0.01), (1001, 0.01), (5, 0.01), (7, 1.0), (16, 0.5))] == [10, 11, 1, 7, 8]
    for r in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            topk_count(10, r)
    assert wire_bytes(1000, 10, 0) == 10 * 8
    assert wire_bytes(1000, 10, 127) == 10 * 5                          # 255 values: 8 bits
    assert wire_bytes(1000, 10, 128) == 10 * 6                          # 257 values: 9 bits, two bytes
    assert wire_bytes(1000, 10, 32767) == 10 * 6
    assert wire_bytes(1000, 1000, 127) == 1000 + 4
    assert wire_bytes(1001, 1001, 1) == 251 + 4                         # 3 values: 2 bits
    assert wire_bytes(1000, 1000, 0) == 4000
    assert "model" in wire_bytes.__doc__ and "not a measurement" in wire_bytes.__doc__
    with pytest.raises(ValueError):
        wire_bytes(10, 11, 0)


def test_names_are_declared():
    import nerve_cl.federated as fed
    from nerve_cl import _nvq
    for name in ("compress_updates_", "topk_count", "wire_bytes", "COMPRESSIONS"):
        assert name in fed.__all__ and hasattr(fed, name)
    assert fed.COMPRESSIONS == ("topk", "quant", "topk_quant")
    header = open(os.path.join(REPO, "include", "nvq.h")).read()
    for sym in ("nvq_fed_compress_workspace_bytes", "nvq_fed_compress"):
        assert sym in _nvq.SIGNATURES and f" {sym}(" in header
    assert len(_nvq.SIGNATURES["nvq_fed_compress"][1]) == 16


# ------------------------------------------------------------------------------------------------ properties of the contract
def test_quantiser_is_unbiased():
    """levels = 3, n = 64, R = 4000 streams: floor(t + u) deviates from t by at most one level and has mean t, so the mean of R
    draws lies within 5 standard errors of at most scale / (2 levels) each of the input"""
    from nerve_cl.federated import compress_updates_
    n, levels, R, rows = 64, 3, 4000, 50
    x = np.random.default_rng(11).standard_normal(n).astype(np.float32)
    scale = float(np.abs(x).max())
    total = np.zeros(n)
    for i in range(R // rows):
        m = torch.from_numpy(np.tile(x, (rows, 1)))
        compress_updates_(m, levels=levels, seed=5, offset=i * rows)
        total += m.double().numpy().sum(0)
    dev = np.abs(total / R - x.astype(np.float64)).max()
    bound = 5 * scale / (2 * levels * np.sqrt(R))
    print(f"largest deviation of the mean {dev:.4g}, bound {bound:.4g}")
    assert dev <= bound


@pytest.mark.parametrize("levels", [0, 127, 1])
def test_error_feedback_telescopes(levels):
    """over T rounds sum_t (x'_t - b) + e_T = sum_t (x_t - b) up to two fp32 roundings per round, that of a and that of e'"""
    from nerve_cl.federated import compress_updates_
    n, k, T = 1023, 50, 20
    g = np.random.default_rng(3)
    b = g.standard_normal(n).astype(np.float32)
    e = torch.zeros(1, n)
    sent, meant, big = np.zeros(n), np.zeros(n), 0.0
    for t in range(T):
        x = (b + 0.1 * g.standard_normal(n)).astype(np.float32)
        meant += x.astype(np.float64) - b
        a = (x.astype(np.float64) - b) + e[0].double().numpy()
        m = torch.from_numpy(x.copy()).view(1, n)
        kept = compress_updates_(m, torch.from_numpy(b), k=k, levels=levels, residual=e, seed=9, offset=t)
        assert kept.tolist() == [k]
        sent += m[0].double().numpy() - b
        big = max(big, np.abs(a).max(), e.abs().max().item())
    err = np.abs(sent + e[0].double().numpy() - meant).max()
    bound = T * 2.0 ** -23 * big
    print(f"levels {levels}: telescoping error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ FederatedTrainer
def _model():
    torch.manual_seed(2)
    return nn.Sequential(nn.Linear(6, 9), nn.BatchNorm1d(9), nn.ReLU(), nn.Linear(9, 3))


def _data(c):
    g = torch.Generator().manual_seed(40 + c)
    return torch.randn(8, 6, generator=g) + 0.2 * c, torch.randn(8, 3, generator=g)


def _row(state, model):
    """the floating tensors of a state dict as the trainer packs them under compression: parameters first, every tensor at a
    multiple of 4 floats; returns (row, n_params)"""
    params = dict(model.named_parameters())
    names = [k for k, v in state.items() if v.is_floating_point()]
    names = [k for k in names if k in params] + [k for k in names if k not in params]
    parts, n_params = [], 0
    for k in names:
        v = state[k].detach().reshape(-1).float()
        parts.append(torch.cat([v, torch.zeros(-v.numel() % 4)]))
        if k in params:
            n_params += parts[-1].numel()
    return torch.cat(parts), n_params


def _trainer(model, captured=None, **kw):
    from nerve_cl.federated import FederatedTrainer

    def hook(cid, m):
        captured.append((cid, {k: v.clone() for k, v in m.state_dict().items()}))

    tr = FederatedTrainer(model, num_clients=4, clients_per_round=3, local_epochs=1, lr=1e-2, batch_size=4, seed=6,
                          after_client=hook if captured is not None else None, **kw)
    for c in range(4):
        tr.set_client_data(c, _data(c))
    return tr


def test_trainer_without_compression_is_unchanged():
    plain, off = _model(), _model()
    a = _trainer(plain).train_round()
    b = _trainer(off, compression=None, compress_ratio=0.5, compress_levels=3, error_feedback=False).train_round()
    assert "kept" not in a and "kept" not in b and a == b
    for x, y in zip(plain.state_dict().values(), off.state_dict().values()):
        assert torch.equal(x, y)


def test_trainer_topk_on_a_plain_module():
    from nerve_cl.federated import topk_count
    model, captured = _model(), []
    start = copy.deepcopy(model.state_dict())
    tr = _trainer(model, captured, compression="topk", compress_ratio=0.25)
    snap, n_p = _row(start, model)
    k = topk_count(n_p, 0.25)
    residual = np.zeros((4, n_p), dtype=np.float32)
    for rnd in range(2):
        del captured[:]
        out = tr.train_round()
        rows, K = tr._plan["rest_rows"], len(captured)
        assert [c for c, _ in captured] == tr.last_selected and tr._plan["n_params"] == n_p and K == 3
        sent = torch.stack([_row(s, model)[0] for _, s in captured])
        slots = [tr._residual_slot[c] for c in tr.last_selected]
        want, residual, want_kept = oracle.compress(sent[:, :n_p].numpy(), snap[:n_p].numpy(), k, 0, residual, slots,
                                                    seed=tr._compress_seed, offset=rnd * 64)
        assert out["kept"] == [want_kept.tolist()] and (want_kept >= k).all()
        for r in range(K):
            changed = int((rows[r, :n_p] != snap[:n_p]).sum())
            assert changed == out["kept"][0][r], (rnd, r)                # exactly the kept parameter columns moved
            assert torch.equal(rows[r, n_p:], sent[r, n_p:])             # the statistics are what the client sent
        assert oracle.same(rows[:K, :n_p].numpy(), want)
        state = tr.compression_state_dict()
        assert oracle.same(state["residuals"][0].numpy(), residual) and state["slots"] == tr._residual_slot
        snap, _ = _row(model.state_dict(), model)
        assert np.allclose(snap[:n_p].numpy(), want.astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)   # FedAvg of the compressed rows
    assert len(set(tr._residual_slot.values())) == len(tr._residual_slot) and (residual != 0).any()
    other = _trainer(_model(), compression="topk", compress_ratio=0.25)
    other.load_compression_state_dict(state)
    assert torch.equal(other.compression_state_dict()["residuals"][0], state["residuals"][0])
    with pytest.raises(ValueError):
        _trainer(_model(), compression="quant").load_compression_state_dict(state)


@pytest.mark.parametrize("kw", [dict(compression="quant", compress_levels=7), dict(compression="topk_quant", compress_ratio=0.5),
                                dict(compression="topk", error_feedback=False, aggregator="median"),
                                dict(compression="topk_quant", server_optimizer="fedadam", server_lr=1e-2, update_clip=1.0)])
def test_trainer_modes_compose_with_the_other_options(kw):
    model = _model()
    tr = _trainer(model, **kw)
    for _ in range(2):
        out = tr.train_round()
        assert len(out["kept"]) == 1 and len(out["kept"][0]) == 3 and np.isfinite(out["train_loss"])
    assert all(torch.isfinite(v).all() for v in model.state_dict().values() if v.is_floating_point())
    assert (tr.compression_state_dict()["residuals"] == []) == (not kw.get("error_feedback", True))


def test_trainer_argument_errors():
    from nerve_cl.federated import FederatedTrainer
    for kw in (dict(compression="gzip"), dict(compression="topk", compress_ratio=0.0), dict(compression="topk", compress_ratio=1.5),
               dict(compression="quant", compress_levels=0), dict(compression="quant", compress_levels=32768)):
        with pytest.raises(ValueError):
            FederatedTrainer(_model(), **kw)
    with pytest.raises(NotImplementedError):
        FederatedTrainer(_model(), compression="topk", num_clusters=2)


def test_compression_seed_leaves_the_other_streams_alone():
    a, b = _trainer(_model()), _trainer(_model(), compression="topk")
    assert a._noise_seed == b._noise_seed and a._rng.getrandbits(62) == b._rng.getrandbits(62)
    assert b._compress_seed not in (0, b._noise_seed)
