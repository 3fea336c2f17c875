"""GPU: nvq_fed_compress (csrc/compress.hip) and FederatedTrainer's compression on the device against the float64 oracle of
tests/_compress_oracle.py.  One criterion for values: equality, as in tests/test_compress_cpu.py (-0 equals +0, NaN exactly where
the oracle has NaN); the kept counts and the residual rows are compared in the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _compress_oracle as oracle  # noqa: E402
from test_compress_cpu import LEVELS, k_values, make_case  # noqa: E402
from test_federated_gpu import _clips, _dev, _pad4, _sr_net  # noqa: E402

SENTINEL = 12345.0


def _n3():
    """The smallest n that is no multiple of 4 and spans three workgroups of the passes: a workgroup takes
    _nvq.FED_COMPRESS_BLOCK_FLOATS = 8192 floats (2048 quads) of a row before the grid grows, so 2 * 8192 + 4 + 1 = 16389."""
    from nerve_cl import _nvq
    return 2 * _nvq.FED_COMPRESS_BLOCK_FLOATS + 5


def _mat(values, stride=None, shift=0):
    """``values`` [R, n] as a [R, n] view with row stride ``stride``, `shift` floats into an allocation filled with the sentinel
    (the padding columns and the four floats behind the matrix keep it); returns (allocation, view)"""
    R, n = values.shape
    stride = stride or n
    buf = torch.full((shift + R * stride + 4,), SENTINEL, device=_dev())
    view = buf[shift:shift + R * stride].view(R, stride)[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(_dev()))
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return buf, view


def _intact(buf, view, shift=0):
    """the sentinels before, between and behind the rows of _mat's matrix"""
    R, n = view.shape
    stride = (buf.numel() - shift - 4) // R
    body = buf[shift:shift + R * stride].view(R, stride)
    return bool((buf[:shift] == SENTINEL).all() and (buf[-4:] == SENTINEL).all() and (body[:, n:] == SENTINEL).all())


def _np(t):
    return t.cpu().numpy()


def _run(clients, base, k, levels, residual=None, slots=None, seed=7, offset=3, stride=None, shift=0):
    """one compress_updates_ on device copies of the numpy operands; returns (x', e' or None, kept) as numpy and whether every
    sentinel survived"""
    from nerve_cl.federated import compress_updates_
    n = clients.shape[1]
    xb, x = _mat(clients, stride, shift)
    bb, b = _mat(base.reshape(1, n), None, shift) if base is not None else (None, None)
    eb, e = _mat(residual, stride, shift) if residual is not None else (None, None)
    kept = compress_updates_(x, None if b is None else b[0], k=k, levels=levels, residual=e, slots=slots, seed=seed, offset=offset)
    assert kept.dtype == torch.int32 and kept.device == x.device
    ok = _intact(xb, x, shift) and (bb is None or _intact(bb, b, shift)) and (eb is None or _intact(eb, e, shift))
    return _np(x), None if e is None else _np(e), _np(kept), ok


@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, "N3"])
def test_kernel_equals_the_oracle(n, K):
    """Every k of {none, 1, 2, n // 2, n - 1, n, n + 5} with every level count of {0, 1, 127, 32767} (at N3 = 16389, see _n3, the
    levels take turns over the k), residual and base present or not in turn, the residual rows in place or permuted into a larger
    matrix, a padded row stride (16-byte loads) or the plain one (scalar loads when n is no multiple of 4) in turn."""
    big = n == "N3"
    n = _n3() if big else n
    M = K + 3
    clients, base, residual = make_case(K, n, 1000 * K + n, rows=M)
    perm = [int(s) for s in np.random.default_rng(K).permutation(M)[:K]]
    case = 0
    for i, k in enumerate(k_values(n)):
        for levels in ((LEVELS[i % 4],) if big else LEVELS):
            case += 1
            for has_res, has_base in (((True, True), (False, False)) if case % 2 else ((True, False), (False, True))):
                slots = perm if has_res and case % 4 < 2 else None
                stride = _pad4(n) if (case // 2) % 2 else None
                b, e = base if has_base else None, residual if has_res else None
                want_x, want_e, want_kept = oracle.compress(clients, b, k, levels, e, slots)
                x, e1, kept, ok = _run(clients, b, k, levels, e, slots, 0, 0, stride)
                what = (n, K, k, levels, has_res, has_base, slots is not None, stride)
                assert ok, what
                assert kept.tolist() == want_kept.tolist(), what
                assert oracle.same(x, want_x), what
                if has_res:
                    assert oracle.same(e1, want_e), what
                    untouched = sorted(set(range(M)) - set(slots if slots is not None else range(K)))
                    assert np.array_equal(e1[untouched].view(np.uint32), residual[untouched].view(np.uint32)), what


def test_ties_and_special_values():
    n, k = 261, 40
    g = np.random.default_rng(4)
    symbols = np.array([0, 0.5, -0.5, 1, -1, 2, -2], dtype=np.float32)
    rows = [g.choice(symbols, n),                                        # the threshold is tied
            np.zeros(n, dtype=np.float32),                               # all zero: nothing to scale by
            np.where(g.random(n) < 0.1, g.standard_normal(n), 0.0),      # more zeros than n - k: the threshold is the key 0
            g.standard_normal(n) * 1e-41,                                # denormals
            g.standard_normal(n), g.standard_normal(n),
            g.choice(symbols, n) * np.float32(1e-45)]                    # tied denormals: 0 and +-1 ulp
    clients = np.stack(rows).astype(np.float32)
    clients[4, 17] = np.nan
    clients[5, 3], clients[5, 200] = np.inf, -np.inf
    assert (np.abs(clients[3]) < 1.2e-38).all() and (clients[3] != 0).any() and (clients[2] == 0).sum() > n - k
    residual = np.zeros_like(clients)
    for levels in (0, 127):
        want_x, want_e, want_kept = oracle.compress(clients, None, k, levels, residual, None, 7, 3)
        x, e, kept, ok = _run(clients, None, k, levels, residual)
        assert ok and kept.tolist() == want_kept.tolist()
        assert oracle.same(x, want_x) and oracle.same(e, want_e)
        assert kept[0] > k and kept[1] == n and kept[2] == n and kept[3] == k and kept[4] == k and kept[5] == k and kept[6] > k
        assert np.isnan(x[4, 17]) and e[4, 17] == 0 and np.isnan(x[4]).sum() == 1
        assert x[5, 3] == np.inf and x[5, 200] == -np.inf and e[5, 3] == 0 and e[5, 200] == 0
        kept_rows = (x != 0)
        assert np.array_equal(x[4][kept_rows[4]], clients[4][kept_rows[4]], equal_nan=True)      # NaN and inf rows: not quantised
        assert np.array_equal(x[5][kept_rows[5]], clients[5][kept_rows[5]]) and (x[1] == 0).all()
    # with a base next to the special values
    base = g.standard_normal(n).astype(np.float32)
    want_x, want_e, want_kept = oracle.compress(clients, base, k, 127, residual, None, 7, 3)
    x, e, kept, ok = _run(clients, base, k, 127, residual)
    assert ok and kept.tolist() == want_kept.tolist() and oracle.same(x, want_x) and oracle.same(e, want_e)


@pytest.mark.parametrize("k,levels", [(None, 127), (300, 0), (300, 127), (None, 0)])
def test_layout_changes_nothing_and_calls_repeat(k, levels):
    K, n = 5, 4101                                                      # two workgroups and a one-float tail
    clients, base, residual = make_case(K, n, 77)
    ref = _run(clients, base, k, levels, residual)
    assert ref[3]
    for stride, shift in ((_pad4(n), 0), (None, 1), (_pad4(n) + 4, 1), (None, 0)):    # the last one: a second call, fresh copies
        got = _run(clients, base, k, levels, residual, stride=stride, shift=shift)
        assert got[3], (stride, shift)
        for a, b in zip(ref[:3], got[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (stride, shift)
    want_x, want_e, want_kept = oracle.compress(clients, base, k, levels, residual, None, 7, 3)
    assert oracle.same(ref[0], want_x) and oracle.same(ref[1], want_e) and ref[2].tolist() == want_kept.tolist()


def test_refusals_come_without_a_launch():
    from nerve_cl import _nvq
    K, n = 3, 1023
    clients, base, residual = make_case(K, n, 9)
    xb, x = _mat(clients)
    eb, e = _mat(residual)
    kept = torch.full((K,), -7, dtype=torch.int32, device=_dev())
    ws = torch.zeros(_nvq.fed_compress_workspace_bytes(K, n) // 4, dtype=torch.float32, device=_dev())
    assert ws.numel() > 0 and _nvq.fed_compress_workspace_bytes(0, n) == 0
    lib = _nvq.lib()

    def call(K_=K, k=10, levels=127, ws_bytes=ws.numel() * 4, stride=n, res_stride=n, seed=0):
        return lib.nvq_fed_compress(x.data_ptr(), stride, K_, None, n, k, levels, e.data_ptr(), res_stride, None, seed, 0,
                                    kept.data_ptr(), ws.data_ptr(), ws_bytes, _nvq.stream())

    with torch.cuda.device(_dev()):
        assert call(ws_bytes=ws.numel() * 4 - 4) == -3                  # NVQ_EWORKSPACE
        assert call(ws_bytes=0) == -3
        for kw in (dict(K_=0), dict(K_=65), dict(k=-1), dict(levels=-1), dict(levels=32768), dict(stride=n - 1),
                   dict(res_stride=n - 1), dict(seed=-1)):
            assert call(**kw) == -1, kw                                 # NVQ_EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(_np(x).view(np.uint32), clients.view(np.uint32)) and (kept == -7).all() and (ws == 0).all()
        assert np.array_equal(_np(e).view(np.uint32), residual.view(np.uint32))
        # k = 0, levels = 0, no residual: valid, nothing changes, kept = n; no workspace is needed
        assert lib.nvq_fed_compress(x.data_ptr(), n, K, None, n, 0, 0, None, 0, None, 0, 0, kept.data_ptr(), None, 0, _nvq.stream()) == 0
        torch.cuda.synchronize()
        assert kept.tolist() == [n] * K and np.array_equal(_np(x).view(np.uint32), clients.view(np.uint32))
        assert call() == 0
        torch.cuda.synchronize()
    want_x, want_e, want_kept = oracle.compress(clients, None, 10, 127, residual)
    assert oracle.same(_np(x), want_x) and oracle.same(_np(e), want_e) and kept.tolist() == want_kept.tolist()
    assert _intact(xb, x) and _intact(eb, e)
    with pytest.raises(RuntimeError):
        _nvq.fed_compress(x, n, None, 10, 127, e, None, kept, ws[:8])


# ------------------------------------------------------------------------------------------------ FederatedTrainer
def _trainer(net, captured=None, **kw):
    from nerve_cl.federated import FederatedTrainer

    def hook(cid, model):
        captured.append((cid, model.flat_theta().clone()))

    kw.setdefault("clients_per_round", 2)
    tr = FederatedTrainer(net, num_clients=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                          after_client=hook if captured is not None else None, **kw)
    for c in range(3):
        tr.set_client_data(c, _clips(8, 10 + c, 0.05 * c))
    return tr


def test_trainer_rounds_equal_the_oracle_on_the_captured_rows():
    """Teacher-forced: every round's rows are the captured client weights, its residual what the device held before the round.  Two
    of three clients per round, so round 2 selects a client of round 1 again and starts from its residual."""
    from nerve_cl.federated import aggregate_flat, topk_count
    net, captured = _sr_net(), []
    tr = _trainer(net, captured, compression="topk_quant", compress_ratio=0.05, compress_levels=127)
    n = net.flat_theta().numel()
    k = topk_count(n, 0.05)
    seen = []
    for rnd in range(2):
        del captured[:]
        snap = net.flat_theta().clone()
        before = _np(tr._residuals[0]) if tr._residuals is not None else np.zeros((3, n), dtype=np.float32)
        out = tr.train_round()
        assert [c for c, _ in captured] == tr.last_selected and len(captured) == 2
        slots = [tr._residual_slot[c] for c in tr.last_selected]
        rows = np.stack([_np(t) for _, t in captured])
        want, residual, kept = oracle.compress(rows, _np(snap), k, 127, before, slots, seed=tr._compress_seed, offset=rnd * 2 * 64)
        assert out["kept"] == [kept.tolist()] and (kept >= k).all()
        assert oracle.same(_np(tr._plan["rows"][0][:2]), want)
        assert oracle.same(_np(tr._residuals[0]), residual)
        model = aggregate_flat(torch.from_numpy(want).to(_dev()), [8.0, 8.0])
        assert torch.equal(net.flat_theta().view(torch.int32), model.view(torch.int32))
        if rnd == 1:
            again = [c for c in tr.last_selected if c in seen]
            assert again and all((before[tr._residual_slot[c]] != 0).any() for c in again)     # round 1 left them a residual
        seen += tr.last_selected
    assert torch.isfinite(net.flat_theta()).all()


@pytest.mark.parametrize("kw", [dict(aggregator="median", clients_per_round=3), dict(server_optimizer="fedadam", server_lr=1e-3)])
def test_trainer_compression_composes_with_the_other_rules(kw):
    net = _sr_net()
    start = net.flat_theta().clone()
    tr = _trainer(net, compression="topk_quant", compress_ratio=0.05, **kw)
    out = tr.train_round()
    assert len(out["kept"]) == 1 and np.isfinite(out["train_loss"])
    assert torch.isfinite(net.flat_theta()).all() and (net.flat_theta() != start).any()


def test_trainer_without_compression_never_calls_the_kernel(monkeypatch):
    from nerve_cl import _nvq
    real, calls = _nvq.fed_compress, []

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(_nvq, "fed_compress", counting)
    out = _trainer(_sr_net(), compression=None).train_round()
    assert "kept" not in out and not calls
    out = _trainer(_sr_net(), compression="topk").train_round()
    assert len(out["kept"]) == 1 and len(calls) == 1                    # one network: one nvq_fed_compress per round


# ------------------------------------------------------------------------------------------------ the script
def test_train_federated_script_with_compression(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_federated.py"),
           "--num-clients", "3", "--clients-per-round", "2", "--num-rounds", "2", "--local-epochs", "1", "--samples", "8",
           "--features", "16", "--blocks", "1", "--compress", "topk_quant"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rounds = [ln for ln in r.stdout.splitlines() if ln.startswith("Round ")]
    assert len(rounds) == 2 and rounds[1].startswith("Round 2: 2 clients, 16 samples"), r.stdout
    for ln in rounds:
        assert np.isfinite(float(ln.split("loss")[1].split()[0].strip(":="))), ln
    sent = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("  compressed updates:")]
    assert len(sent) == 2, r.stdout
    for words in sent:
        share, wire = float(words[3]), float(words[8])
        assert 0.01 <= share < 0.0105 and 0.0 < wire < 0.02, words       # 1 % kept; 5 of 4 bytes per kept coordinate
