"""GPU: csrc/robust.hip (the trimmed-mean / median pass and the Krum selection) against float64 numpy written here, then
nerve_cl.federated.robust and FederatedTrainer with the robust aggregators on the device.

Bounds.  Trimmed mean without noise: the float64 chain (differences, the sum in sorted order, one division, one fma) is rounded to
fp32 once: 1 ulp of the float64 value, the bound tests/test_federated_gpu.py derives.  The median of an odd number of rows with no
base and server_lr = 1 is one of the inputs: bit-equal.  The envelope min_honest <= out <= max_honest is a theorem of the trimmed
mean with trim >= the number of replaced rows (a mean of values inside an interval, rounded monotonically): asserted exactly.
Noise: fp32 logf / sincospif / sqrtf against float64, 2e-5 absolute per unit of standard deviation, as the existing noise test.
Krum: a distance is G_ii + G_jj - 2 G_ij of Gram entries that carry the Gram bound of the existing tests, 4e-10 of the sum of the
G_ii + G_jj terms of a score; the inputs are chosen (and checked) so that the scores which decide the selection are farther apart."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _federated_oracle as oracle  # noqa: E402
from test_federated_cpu import GOLDEN, golden_model  # noqa: E402
from test_federated_gpu import SECOND_TRIP, _clips, _dev, _matrix, _pad4, _sr_net, _within_ulps  # noqa: E402

MEDIAN = 64
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)          # both sides of every boundary of the instantiations (8, 16, 32, 64 rows)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _trimmed(clients, n, base, weights, trim, out=None, **kw):
    from nerve_cl import _nvq
    w = None if weights is None else torch.tensor(weights, dtype=torch.float64).to(_dev())
    if out is None:
        out = torch.full((n,), float("nan"), device=_dev())
    _nvq.fed_trimmed_aggregate(clients, n, base, w, trim, out, **kw)
    return out


def _want(clients, n, base, trim, lr=1.0, live=None):
    """float64 numpy: base + lr * (sum of (np.sort(live rows) - base)[t : m - t] in that order) / (m - 2 t), as a device tensor"""
    x = clients[:, :n].cpu().numpy()
    if live is not None:
        x = x[list(live)]
    m = len(x)
    t = min(trim, (m - 1) // 2)
    b = np.zeros(n) if base is None else base.cpu().numpy().astype(np.float64)
    s = np.sort(x, axis=0)
    a = np.zeros(n)
    for j in range(t, m - t):
        a = a + (s[j].astype(np.float64) - b)
    return torch.from_numpy(b + lr * (a / (m - 2 * t))).to(_dev())


# ------------------------------------------------------------------------------------------------ trimmed mean
TRIM_CASES = [(n, K, padded) for n in (1, 3, 4, 5, 1023) for K in KS for padded in (False, True) if n % 4 or not padded]


@pytest.mark.parametrize("n,K,padded", TRIM_CASES)
def test_trimmed_mean_within_one_ulp(n, K, padded):
    from nerve_cl.federated import aggregate_flat
    stride = _pad4(n) if padded else n
    seed = 3000 + n % 89 + K
    clients, base = _matrix(K, n, stride, seed)
    shifted, sbase = _matrix(K, n, stride, seed, shift=1)                          # only 4-byte aligned
    for trim in sorted({0, 1, (K - 1) // 2}):
        for b, sb in ((None, None), (base, sbase)):
            for lr in (1.0, 0.5):
                got = _trimmed(clients, n, b, None, trim, server_lr=lr)
                assert _within_ulps(got, _want(clients, n, b, trim, lr)), (trim, b is not None, lr)
                assert torch.equal(_bits(got), _bits(_trimmed(clients, n, b, None, trim, server_lr=lr)))            # a second call
                assert torch.equal(_bits(got), _bits(_trimmed(shifted, n, sb, None, trim, server_lr=lr)))           # another alignment
        aliased = base.clone()                                                     # out may be base
        _trimmed(clients, n, aliased, None, trim, out=aliased, server_lr=0.5)
        assert torch.equal(_bits(aliased), _bits(got)), trim
    mean = aggregate_flat(clients[:, :n], [2.0] * K)                               # trim = 0, equal weights: FedAvg
    assert _within_ulps(_trimmed(clients, n, None, None, 0), mean.double())
    assert _within_ulps(_trimmed(clients, n, None, [2.0] * K, 0), mean.double())


@pytest.mark.parametrize("K,padded", [(1, False), (9, True), (17, False), (33, True)])      # the smallest K of each instantiation
def test_trimmed_mean_second_trip(K, padded):
    n = SECOND_TRIP
    stride = _pad4(n) if padded else n
    clients, base = _matrix(K, n, stride, 3100 + K)
    trim = min(1, (K - 1) // 2)
    got = _trimmed(clients, n, base, None, trim, server_lr=0.5)
    assert _within_ulps(got, _want(clients, n, base, trim, 0.5))
    shifted, sbase = _matrix(K, n, stride, 3100 + K, shift=1)
    assert torch.equal(_bits(got), _bits(_trimmed(shifted, n, sbase, None, trim, server_lr=0.5)))


# ------------------------------------------------------------------------------------------------ median
@pytest.mark.parametrize("K", KS)
def test_median_is_numpys(K):
    from nerve_cl.federated import aggregate_flat_median
    n = 1023
    clients, _ = _matrix(K, n, n, 3200 + K, base=False)
    got = aggregate_flat_median(clients)
    x = clients.cpu().numpy()
    if K % 2:
        assert np.array_equal(got.cpu().numpy().view(np.int32), np.median(x, axis=0).view(np.int32))     # the middle value, bit for bit
    else:
        assert _within_ulps(got, torch.from_numpy(np.median(x.astype(np.float64), axis=0)).to(_dev()))
    assert torch.equal(_bits(got), _bits(_trimmed(clients, n, None, None, (K - 1) // 2)))                # any trim >= (K - 1) / 2


# ------------------------------------------------------------------------------------------------ order semantics
def _small(seed, K=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(K, 8, generator=g)


def _nan(sign_bit):
    return float(np.array([0xFFC00000 if sign_bit else 0x7FC00000], dtype=np.uint32).view(np.float32)[0])


def test_ties_and_signed_zeros():
    x = _small(1)
    x[:, 2] = 0.37                                                                 # a column of equal values
    x[:, 5] = torch.tensor([0.0, -0.0, -0.0, 0.0, -0.0])                           # both zeros, in either order
    x[:, 6] = torch.tensor([1.5, -0.0, 0.0, 1.5, -2.0])
    clients = x.to(_dev())
    for trim in (0, 1, 2):
        got = _trimmed(clients, 8, None, None, trim)
        assert _within_ulps(got, _want(clients, 8, None, trim)), trim
        assert got[2].item() == np.float32(0.37) and got[5].item() == 0.0
    assert _trimmed(clients, 8, None, None, 2)[6].item() == 0.0                    # the median of {-2, -0, +0, 1.5, 1.5}


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), _nan(0), _nan(1)])
def test_a_row_of_inf_or_nan_is_trimmed(value):
    x = _small(2)
    x[3] = value
    clients = x.to(_dev())
    got = _trimmed(clients, 8, None, None, 1)
    want = _want(clients, 8, None, 1)                                              # np.sort: -inf first, +inf and then NaN last
    assert torch.isfinite(want).all() and torch.isfinite(got).all() and _within_ulps(got, want)
    base = (0.1 * _small(3)[0]).to(_dev())
    assert _within_ulps(_trimmed(clients, 8, base, None, 1, server_lr=0.5), _want(clients, 8, base, 1, 0.5))
    assert _within_ulps(_trimmed(clients, 8, None, None, MEDIAN), _want(clients, 8, None, MEDIAN))
    if value != value:                                                             # without trimming the NaN is in the mean
        assert torch.isnan(_trimmed(clients, 8, None, None, 0)).all()


def test_rows_that_are_not_live_are_never_read():
    from nerve_cl.federated import aggregate_flat, aggregate_flat_trimmed
    x = _small(4)
    x[1] = float("nan")
    clients = x.to(_dev())
    w = [2.0, 0.0, 3.0, 1.0, 4.0]
    got = _trimmed(clients, 8, None, w, 0)
    assert torch.isfinite(got).all() and _within_ulps(got, _want(clients, 8, None, 0, live=[0, 2, 3, 4]))
    assert torch.isnan(aggregate_flat(clients, w)).all()                           # the weighted mean: 0 * NaN
    y = _small(5)
    y[0], y[2] = float("nan"), 1e30
    clients = y.to(_dev())
    alone = y[[1, 3, 4]].contiguous().to(_dev())
    base = (0.1 * _small(6)[0]).to(_dev())
    for trim in (0, 1, MEDIAN):
        for b, lr in ((None, 1.0), (base, 0.5)):
            got = _trimmed(clients, 8, b, [0.0, 0.5, 0.0, 0.5, 0.5], trim, server_lr=lr)
            assert torch.equal(_bits(got), _bits(_trimmed(alone, 8, b, None, trim, server_lr=lr))), (trim, lr)
    out = aggregate_flat_trimmed(clients, 1, weights=torch.tensor([0.0, 1.0, 0.0, 2.0, 3.0], dtype=torch.float64, device=_dev()))
    assert torch.equal(_bits(out), _bits(_trimmed(alone, 8, None, None, 1)))       # device weights are used as they are
    none = _trimmed(clients, 8, base, [0.0] * 5, 1, server_lr=0.5)                 # m = 0 (only reachable with device weights): a = 0
    assert torch.equal(_bits(none), _bits(base))


# ------------------------------------------------------------------------------------------------ envelope
@pytest.mark.parametrize("K,b", [(5, 1), (9, 2), (17, 5), (33, 5), (64, 20)])
def test_envelope_of_the_honest_rows(K, b):
    n = 1023
    clients, _ = _matrix(K, n, n, 3300 + K, base=False)
    honest = clients[b:].clone()
    with torch.no_grad():
        for k in range(b):
            kind = k % 4
            if kind == 0:
                clients[k] = 1e30 * torch.sign(clients[k])                         # huge
            elif kind == 1:
                clients[k] = float("nan")
            elif kind == 2:
                clients[k] = -10.0 * honest.mean(0)                                # the sign-flipped, scaled mean
            else:
                clients[k] = float("-inf")
    lo, hi = honest.min(0).values, honest.max(0).values
    for trim in sorted({b, b + 1, (K - 1) // 2, MEDIAN}):
        got = _trimmed(clients, n, None, None, trim)
        assert bool(((got >= lo) & (got <= hi)).all()), trim


# ------------------------------------------------------------------------------------------------ noise
def test_noise_is_the_philox_stream_of_the_aggregate():
    from nerve_cl import _nvq
    n, seed, offset, std = 4099, (1 << 40) + 77, (1 << 33) + 5, 1.0
    g = torch.Generator().manual_seed(4)
    base = (0.1 * torch.randn(n, generator=g)).to(_dev())
    z = torch.from_numpy(oracle.normals(seed, offset, n)).to(_dev())
    outs = {}
    for K in (2, 5, 9, 17, 33):                                                    # every instantiation
        clients = base.repeat(K, 1).contiguous()                                   # every d = 0: v = base exactly
        outs[K] = _trimmed(clients, n, base, None, 1, noise_std=std, seed=seed, offset=offset)
        assert torch.equal(_bits(outs[K]), _bits(outs[2])), K                      # independent of K
    err = ((outs[2].double() - base.double()) - std * z).abs().max().item()
    print(f"noise: max |out - base - std z| = {err:.3e}")
    assert err <= 2e-5 * std, err
    fed = torch.empty(n, device=_dev())                                            # the same stream as nvq_fed_aggregate
    _nvq.fed_aggregate(base.repeat(2, 1).contiguous(), n, base, torch.ones(2, dtype=torch.float64, device=_dev()), None, fed,
                       noise_std=std, seed=seed, offset=offset)
    assert torch.equal(_bits(fed), _bits(outs[2]))
    buf = torch.zeros(2 * n + 8, device=_dev())
    shifted = buf[1:1 + 2 * n].view(2, n)
    shifted.copy_(base.repeat(2, 1))
    sbase = torch.zeros(n + 1, device=_dev())[1:]
    sbase.copy_(base)
    sout = torch.zeros(n + 1, device=_dev())[1:]
    _trimmed(shifted, n, sbase, None, 1, out=sout, noise_std=std, seed=seed, offset=offset)
    assert torch.equal(_bits(outs[2]), _bits(sout.clone()))                        # independent of the alignment
    other = _trimmed(base.repeat(2, 1).contiguous(), n, base, None, 1, noise_std=std, seed=seed, offset=offset + 1)
    assert (other != outs[2]).float().mean() > 0.99                                # a new offset: new draws
    x = _matrix(5, n, n, 9)[0]                                                     # and on real updates: fmaf(std, z, v)
    v = _trimmed(x, n, base, None, 1, server_lr=0.5)
    got = _trimmed(x, n, base, None, 1, server_lr=0.5, noise_std=0.25, seed=seed, offset=offset)
    want = v.double() + 0.25 * z
    ulp = (torch.nextafter(want.abs().float(), torch.full_like(v, float("inf"))) - want.abs().float()).double()
    assert ((got.double() - want).abs() <= 2e-5 * 0.25 + ulp).all()


# ------------------------------------------------------------------------------------------------ Krum
def _krum_oracle(x, base, f, q, live):
    """float64 numpy on the rows themselves: (scores, order, weights, per-score bound 4e-10 * sum of the G_ii + G_jj terms, c).
    D_ij is formed from the difference of the two updates, so D is symmetric bit for bit, as the device's is (its Gram is)."""
    K = len(x)
    u = x.astype(np.float64) - base.astype(np.float64)
    with np.errstate(invalid="ignore"):
        diag = (u * u).sum(1)
        D = np.array([[((u[i] - u[j]) ** 2).sum() for j in range(K)] for i in range(K)])
    D = np.where(np.isnan(D), np.inf, D)
    m = len(live)
    c = min(max(m - f - 2, 1), m - 1)
    scores, bound = np.full(K, np.inf), np.zeros(K)
    for i in live:
        others = np.array([j for j in live if j != i], dtype=np.int64)
        near = others[np.argsort(D[i, others], kind="stable")[:c]]
        scores[i] = np.sort(D[i, near]).sum() if c else 0.0
        bound[i] = 4e-10 * np.nansum(diag[i] + diag[near]) if c else 0.0
    ranked = sorted(live, key=lambda i: (np.isnan(scores[i]), scores[i], i))
    w = np.zeros(K)
    w[ranked[:min(q, m)]] = 1.0
    return scores, ranked + [k for k in range(K) if k not in live], w, bound, c


def _krum_rows(K, f, seed, n=257):
    """honest rows: one tight cluster around the base; rows 1, 3, ..: f far outliers"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    x = base + 0.01 * torch.randn(K, n, generator=g)
    out = [2 * k + 1 for k in range(f)]
    for k in out:
        x[k] = base + 5.0 * torch.randn(n, generator=g)
    return x, base, out


def _select(x, base, f, q, weights):
    """nvq_fed_krum_select itself on the device Gram: the library clamps c for any m, where the Python function refuses m < f + 3"""
    from nerve_cl import _nvq
    from nerve_cl.federated import KrumResult, update_gram
    K = len(x)
    w = None if weights is None else torch.tensor(weights, dtype=torch.float64).to(_dev())
    res = KrumResult(torch.empty(K, dtype=torch.float64, device=_dev()), torch.empty(K, dtype=torch.float64, device=_dev()),
                     torch.empty(K, dtype=torch.int32, device=_dev()))
    _nvq.fed_krum_select(update_gram(x.to(_dev()), base.to(_dev())), K, w, f, q, *res)
    return res


KRUM_CASES = sorted({(K, f, q, dead) for K in (3, 5, 64) for f in (0, 1, (K - 3) // 2) for q in (1, K - f) for dead in (False, True)
                     if K > 3 or not dead})


@pytest.mark.parametrize("K,f,q,dead", KRUM_CASES)
def test_krum_selection_against_float64(K, f, q, dead):
    x, base, outliers = _krum_rows(K, f, 3400 + 7 * K + f)
    weights, live = None, list(range(K))
    if dead:                                                                       # rows without samples: one honest, one of NaN
        gone = [0, K - 1]
        x[K - 1] = float("nan")
        weights = [0.0 if k in gone else 1.0 + k % 3 for k in range(K)]
        live = [k for k in range(K) if k not in gone]
    scores, order, w, bound, c = _krum_oracle(x.numpy(), base.numpy(), f, q, live)
    m = len(live)
    top = min(q, m)
    # A condition on the inputs, not on the kernel: neighbours among the scores that decide the first `top` places are farther apart than their two bounds.
    # With c = 1 a score is the distance to the nearest row, and two rows that are each other's nearest have the same score, D_ij =
    # D_ji, whatever the inputs (K = 3 always has such a pair in front): an exact tie on the device too, since its Gram matrix is
    # symmetric bit for bit, and the index decides it.
    decisive = order[:min(top + 1, m)]
    assert all(scores[j] - scores[i] > bound[i] + bound[j] or (c == 1 and scores[i] == scores[j])
               for i, j in zip(decisive, decisive[1:])), "the inputs do not separate the scores"
    res = _select(x, base, f, q, weights)
    assert res.order.dtype == torch.int32 and res.order[:top].tolist() == order[:top]
    assert sorted(res.order.tolist()) == list(range(K)) and res.order[m:].tolist() == order[m:]
    assert res.weights.tolist() == w.tolist()
    got = res.scores.cpu().numpy()
    assert np.isinf(got[[k for k in range(K) if k not in live]]).all()
    assert (np.abs(got[live] - scores[live]) <= bound[live]).all(), np.abs(got[live] - scores[live]).max()
    if top <= m - len([o for o in outliers if o in live]):                         # enough honest rows: no outlier among the chosen
        assert not any(w[k] for k in outliers)
    again = _select(x, base, f, q, weights)
    assert torch.equal(res.scores.view(torch.int64), again.scores.view(torch.int64)) and torch.equal(res.order, again.order)


def test_krum_never_selects_a_live_row_of_nan():
    x, base, _ = _krum_rows(5, 0, 77)
    x[2] = float("nan")
    res = _select(x, base, 1, 4, None)
    assert res.weights.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0] and res.order[-1].item() == 2
    s = res.scores.cpu().numpy()
    assert np.isfinite(s[[0, 1, 3, 4]]).all() and np.isinf(s[2])
    scores, order, w, bound, _ = _krum_oracle(x.numpy(), base.numpy(), 1, 4, list(range(5)))
    assert res.order.tolist() == order and (np.abs(s[[0, 1, 3, 4]] - scores[[0, 1, 3, 4]]) <= bound[[0, 1, 3, 4]]).all()


def test_krum_with_one_or_two_live_rows():
    x, base, _ = _krum_rows(3, 0, 78)
    res = _select(x, base, 0, 1, None)
    assert res.weights.sum().item() == 1.0
    from nerve_cl import _nvq
    from nerve_cl.federated import update_gram
    gram = update_gram(x.to(_dev()), base.to(_dev()))
    out = [torch.empty(3, dtype=torch.float64, device=_dev()), torch.empty(3, dtype=torch.float64, device=_dev()),
           torch.empty(3, dtype=torch.int32, device=_dev())]
    _nvq.fed_krum_select(gram, 3, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).to(_dev()), 0, 2, *out)
    assert out[0].tolist() == [0.0, 1.0, 0.0] and out[2].tolist() == [1, 0, 2]    # m = 1: selected, score 0
    assert out[1][1].item() == 0.0 and np.isinf(out[1][[0, 2]].cpu().numpy()).all()
    _nvq.fed_krum_select(gram, 3, torch.tensor([2.0, 0.0, 1.0], dtype=torch.float64).to(_dev()), 0, 1, *out)
    d = (x[0].double() - x[2].double()).pow(2).sum().item()                        # m = 2: c = 1, both scores are D_02; index decides
    assert out[0].tolist() == [1.0, 0.0, 0.0] and out[2].tolist() == [0, 2, 1]
    assert abs(out[1][0].item() - d) <= 1e-9 * d and out[1][0].item() == out[1][2].item()
    rc = _nvq.lib().nvq_fed_krum_select(gram.data_ptr(), 65, None, 0, 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None)
    assert rc == -1
    rc = _nvq.lib().nvq_fed_trimmed_aggregate(gram.data_ptr(), 8, 65, None, None, 0, 1.0, 0.0, 0, 0, 8, out[0].data_ptr(), None)
    assert rc == -1


def test_krum_aggregate_is_the_mean_of_the_selected_rows():
    from nerve_cl.federated import krum_aggregate_flat
    K, f = 9, 2
    x, base, outliers = _krum_rows(K, f, 79, n=1023)
    clients, b = x.to(_dev()), base.to(_dev())
    for q in (1, K - f):
        scores, order, w, _, _ = _krum_oracle(x.numpy(), base.numpy(), f, q, list(range(K)))
        chosen = [int(k) for k in np.flatnonzero(w)]
        assert not set(chosen) & set(outliers)
        got = krum_aggregate_flat(clients, f, q, base=b, server_lr=0.5)
        assert _within_ulps(got, _want(clients, 1023, b, 0, 0.5, live=chosen)), q
        assert torch.equal(_bits(got), _bits(_trimmed(clients[chosen].contiguous(), 1023, b, None, 0, server_lr=0.5)))
    poisoned = clients.clone()
    poisoned[4] = float("nan")
    wts = [0.0 if k == 4 else 1.0 for k in range(K)]
    got = krum_aggregate_flat(poisoned, f, K - 1 - f, base=b, weights=wts)
    assert torch.isfinite(got).all()


# ------------------------------------------------------------------------------------------------ no synchronisation
def _no_sync(fn):
    """run fn under set_sync_debug_mode("error"); the control .item() must raise, or the check would be vacuous"""
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fn()
        try:
            torch.zeros((), device=_dev()).item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert control_raised, "torch.cuda.set_sync_debug_mode('error') does not flag .item() on this PyTorch build"
    return out


def test_robust_functions_read_nothing_back():
    from nerve_cl.federated import aggregate_flat_median, aggregate_flat_trimmed, krum_aggregate_flat, krum_select, update_gram
    clients, base = _matrix(9, 5000, 5000, 11)
    w = torch.tensor([1.0, 0.0, 2.0, 1.0, 1.0, 3.0, 1.0, 1.0, 1.0], dtype=torch.float64).to(_dev())
    krum_aggregate_flat(clients, 2, 3, base=base)                                  # warm-up: code objects, the Gram workspace
    aggregate_flat_median(clients, base=base)
    torch.cuda.synchronize()

    def run():
        a = krum_aggregate_flat(clients, 2, 3, base=base, weights=w, server_lr=0.5, noise_std=0.1, seed=3, offset=1)
        b = aggregate_flat_median(clients, weights=w, base=base)
        c = aggregate_flat_trimmed(clients, 2, out=torch.empty(5000, device=_dev()))
        d = krum_select(update_gram(clients, base), 1, 2)
        return a, b, c, d
    a, b, c, d = _no_sync(run)
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.isfinite(c).all() and d.weights.sum().item() == 2.0


@pytest.mark.parametrize("agg", ["median", "trimmed_mean", "krum", "multi_krum"])
def test_trainer_round_with_a_robust_aggregator_reads_nothing_back(agg):
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8, aggregator=agg,
                          trim_ratio=0.34, update_noise=1e-4, server_lr=0.5)
    for c in range(3):
        tr.set_client_data(c, _clips(4, 20 + c))
    tr.train_round()                                                               # warm-up: code objects loaded, buffers built
    out = _no_sync(tr.train_round_device)
    assert out["round"] == 2 and np.isfinite(out["train_loss"].item()) and torch.isfinite(net.flat_theta()).all()
    if agg in ("krum", "multi_krum"):
        sel = out["selected_weights"]
        assert sel.is_cuda and sel.dtype == torch.float64 and sel.sum().item() == (1.0 if agg == "krum" else 3.0)
    else:
        assert "selected_weights" not in out


def test_trainer_median_on_the_flat_buffer_is_the_median_of_the_rows():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    rows = []
    tr = FederatedTrainer(net, num_clients=3, clients_per_round=3, local_epochs=1, lr=1e-3, batch_size=4, seed=8, aggregator="median",
                          after_client=lambda cid, model: rows.append(model.flat_theta().clone()))
    for c in range(3):
        tr.set_client_data(c, _clips(4, 30 + c, 0.05 * c))
    tr.train_round()
    want = torch.stack(rows).median(0).values                                      # three rows: the middle one, bit for bit
    assert len(rows) == 3 and (rows[0] != rows[1]).any() and torch.equal(_bits(net.flat_theta()), _bits(want))


# ------------------------------------------------------------------------------------------------ the trainer against a poisoned client
def _golden_data():
    g = torch.Generator().manual_seed(21)
    return {c: ((torch.randn(8, 3, 6, 6, generator=g) + 0.1 * c).to(_dev()), torch.randn(8, 7, generator=g).to(_dev())) for c in range(4)}


def _float_state(model):
    return torch.cat([v.detach().reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()])


def _poisoned_round(agg, kind, data):
    """one round of 4 clients on the small golden model, client 2 poisoned through after_client; (weights after the round, the
    clients' rows as the hook left them, the order of the clients, the round dict)"""
    from nerve_cl.federated import FederatedTrainer
    model = golden_model(np.load(GOLDEN)).to(_dev())
    start = _float_state(model).clone()
    rows = []

    def hook(cid, m):
        if cid == 2:
            off = 0
            for v in m.state_dict().values():
                if v.is_floating_point():
                    g = start[off:off + v.numel()].view(v.shape)
                    v.copy_(torch.full_like(v, float("nan")) if kind == "nan" else g - 10.0 * (v - g))
                    off += v.numel()
        rows.append(_float_state(m).clone())

    tr = FederatedTrainer(model, num_clients=4, clients_per_round=4, local_epochs=2, lr=1e-2, batch_size=4, seed=5, aggregator=agg,
                          num_byzantine=1, after_client=hook)
    for c, d in data.items():
        tr.set_client_data(c, d)
    out = tr.train_round()
    return _float_state(model).clone(), torch.stack(rows), list(tr.last_selected), out


@pytest.mark.parametrize("kind", ["nan", "flip"])
def test_trainer_median_and_krum_hold_against_a_poisoned_client(kind):
    data = _golden_data()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        runs = {agg: _poisoned_round(agg, kind, data) for agg in ("fedavg", "median", "krum")}
        again = _poisoned_round("median", kind, data)
    finally:
        torch.backends.cudnn.deterministic = det
    for agg, (theta, rows, selected, out) in runs.items():
        honest = rows[[k for k, c in enumerate(selected) if c != 2]]               # the rows of this very round, from the hook
        lo, hi = honest.min(0).values, honest.max(0).values
        inside = bool(((theta >= lo) & (theta <= hi)).all())
        if agg == "fedavg":
            assert bool(torch.isnan(theta).any()) or not inside                    # the poison is real
        else:
            assert bool(torch.isfinite(theta).all()) and inside, agg
        if agg == "krum":
            sel = out["selected_weights"]
            assert sel[selected.index(2)] == 0.0 and sum(sel) == 1.0
            assert torch.equal(_bits(theta), _bits(rows[sel.index(1.0)]))          # Krum's model is the chosen client's
    from nerve_cl.federated import krum_select, update_gram
    x, base, _ = _krum_rows(5, 1, 80)                                              # the Python function: the same selection
    res = krum_select(update_gram(x.to(_dev()), base.to(_dev())), 1, 2, weights=[1.0, 1.0, 1.0, 1.0, 1.0])
    assert res.weights.tolist() == _select(x, base, 1, 2, None).weights.tolist() and res.weights[1].item() == 0.0
    assert again[2] == runs["median"][2] and torch.equal(_bits(again[0]), _bits(runs["median"][0]))      # same seed, same bits


# ------------------------------------------------------------------------------------------------ the script
def test_train_federated_script_with_a_poisoned_client(tmp_path):
    import subprocess
    repo = os.path.dirname(HERE)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(repo, "experiments", "train_federated.py"),
           "--num-clients", "3", "--clients-per-round", "3", "--num-rounds", "2", "--local-epochs", "1", "--samples", "4",
           "--features", "16", "--blocks", "1", "--aggregator", "median", "--poison", "1", "--poison-kind", "nan"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rounds = [ln for ln in r.stdout.splitlines() if ln.startswith("Round ")]
    evals = [float(ln.split()[-1]) for ln in r.stdout.splitlines() if ln.startswith("  evaluation loss")]
    assert len(rounds) == 2 and len(evals) == 2 and np.isfinite(evals).all(), r.stdout
