"""GPU: csrc/cluster.hip (the update Gram on the fp64 matrix cores, kernel k-means on the Gram, one aggregation pass for C cluster
models) against float64 numpy written here, then the clustered FederatedTrainer on the smallest SuperResolutionNet.

Bounds.  Gram: the device adds n products of exact float64 differences in another order than the oracle; the standard bound for a
reordered sum of n products is n 2^-52 (|U| |U|^T) elementwise (Higham, Accuracy and Stability, 3.1), nothing measured.  k-means:
the oracle runs the identical algorithm on the explicit vectors; the inputs are built (and asserted) so that at every decision of
the oracle the best and the second-best candidate differ by more than 1e-6 relative, far above the Gram bound, so labels, counts
and sweeps are equal exactly.  Inertia: each d(k, c) is a sum of Gram entries of magnitude <= max G_kk with total weight 4, so
its error is <= 4 n 2^-52 max G_kk; with n = 4099, G_kk ~ 4.5e3 and d ~ 2.8e2 that is 6e-11 relative: asserted at 1e-9.
Aggregation: bit for bit nvq_fed_aggregate on the gathered member rows.  Trainer: the one-ulp bound of tests/test_federated_gpu.py."""
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
from test_clustering_cpu import lloyd_oracle  # noqa: E402

PAST_THE_CAP = 1024 * 1024 + 1031       # more than 1024 blocks x 256 threads x one quad: a second trip and a tail


def _dev():
    return torch.device("cuda", 0)


def _ws():
    from nerve_cl import _engine
    return _engine.workspace(_dev())


def _place(vals, stride, shift=0):
    """vals [K, n] (CPU) as a [K][stride] device matrix, a view `shift` floats into its allocation"""
    K, n = vals.shape
    buf = torch.zeros(shift + K * stride + 4, device=_dev())
    m = buf[shift:shift + K * stride].view(K, stride)
    m[:, :n] = vals.to(_dev())
    if shift:
        assert m.data_ptr() % 16 == 4 * shift
    return m


def _place_vec(v, shift=0):
    buf = torch.zeros(shift + v.numel() + 4, device=_dev())
    out = buf[shift:shift + v.numel()]
    out.copy_(v.to(_dev()))
    return out


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ------------------------------------------------------------------------------------------------ the update Gram
def _gram(clients, n, base):
    from nerve_cl import _nvq
    from nerve_cl.federated.clustering import _gram_workspace
    K = clients.shape[0]
    g = torch.full((K, K), float("nan"), dtype=torch.float64, device=_dev())
    _nvq.fed_update_gram(clients, n, base, g, _gram_workspace(_dev(), K, n))
    return g


def _check_gram(K, n, seed):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(seed)
    vals = torch.randn(K, n, generator=gen)
    bvals = vals.mean(0) + 0.1 * torch.randn(n, generator=gen)
    for has_base in (False, True):
        stride = n if (K + n + has_base) % 2 else (n + 3) // 4 * 4 + 4           # stride == n and stride > n both occur
        clients = _place(vals, stride)
        base = _place_vec(bvals) if has_base else None
        g = _gram(clients, n, base)
        u = vals.double().numpy() - (bvals.double().numpy() if has_base else 0.0)
        ref, bound = u @ u.T, n * 2.0 ** -52 * (np.abs(u) @ np.abs(u).T)
        got = g.cpu().numpy()
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= bound).all(), (K, n, has_base, np.abs(got - ref).max(), bound.min())
        assert torch.equal(_bits(g), _bits(g.t()))                                 # symmetric bit for bit
        assert torch.equal(_bits(g), _bits(_gram(clients, n, base)))               # the same bits on every call
        shifted = _place(vals, stride, shift=1)                                    # only 4-byte aligned: the scalar form
        sbase = _place_vec(bvals, shift=1) if has_base else None
        assert torch.equal(_bits(g), _bits(_gram(shifted, n, sbase)))
        odd = _place(vals, (n + 3) // 4 * 4 + 1)                                   # aligned, stride % 4 != 0: the scalar form too
        assert torch.equal(_bits(g), _bits(_gram(odd, n, base)))
        sq = torch.zeros(K, dtype=torch.float64, device=_dev())
        _nvq.fed_delta_norms(clients, n, base, sq, _ws())
        assert (np.abs(np.diag(got) - sq.cpu().numpy()) <= np.diag(bound)).all()


@pytest.mark.parametrize("n", [1, 3, 4, 7, 1023, 4101])
@pytest.mark.parametrize("K", [1, 2, 5, 16, 17, 33, 64])
def test_update_gram_against_float64(K, n):
    _check_gram(K, n, 100 * K + n % 97)


def test_update_gram_past_the_block_cap():
    _check_gram(3, PAST_THE_CAP, 7)


def test_update_gram_refuses_a_short_workspace_and_bad_counts():
    from nerve_cl import _nvq
    clients = _place(torch.zeros(17, 5000), 5000)
    g = torch.zeros(17, 17, dtype=torch.float64, device=_dev())
    assert _nvq.fed_gram_workspace_bytes(17, 5000) == 5 * 3 * 256 * 8              # 5 blocks, 3 tiles of the 2 x 2 grid
    assert _nvq.fed_gram_workspace_bytes(64, 1) == 10 * 256 * 8 and _nvq.fed_gram_workspace_bytes(65, 1) == 0
    with pytest.raises(RuntimeError, match="workspace"):
        _nvq.fed_update_gram(clients, 5000, None, g, torch.zeros(8, device=_dev()))
    rc = _nvq.lib().nvq_fed_update_gram(clients.data_ptr(), 5000, 65, None, 5000, g.data_ptr(), _ws().data_ptr(), 1 << 20, None)
    assert rc == -1


def test_update_similarity_is_the_cosine_and_zero_for_a_zero_update():
    from nerve_cl.federated import update_similarity
    gen = torch.Generator().manual_seed(5)
    vals = torch.randn(4, 1031, generator=gen)
    base = vals[2].clone()                                                         # client 2 did not move
    s = update_similarity(vals.to(_dev()), base.to(_dev())).cpu().numpy()
    u = (vals.double() - base.double()).numpy()                                   # the difference is formed in double
    norm = np.sqrt((u * u).sum(1))
    want = np.where(np.outer(norm, norm) > 0, (u @ u.T) / np.where(np.outer(norm, norm) > 0, np.outer(norm, norm), 1.0), 0.0)
    assert np.isfinite(s).all() and (s[2] == 0).all() and (s[:, 2] == 0).all()
    assert np.abs(s - want).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ k-means on the Gram
def _groups(groups, per, n, noise, seed):
    gen = torch.Generator().manual_seed(seed)
    dirs = torch.randn(groups, n, generator=gen)
    rows = [dirs[g] + noise * torch.randn(n, generator=gen) for g in range(groups) for _ in range(per)]
    return torch.stack(rows)


def _compare(vals, C, init, max_iter, margin=1e-6, inertia_rel=1e-9):
    from nerve_cl.federated import cluster_updates
    u = vals.double().numpy()
    want = lloyd_oracle(u, C, init, max_iter)
    assert want["margin"] > margin, want["margin"]                                 # a condition on the inputs, not a tolerance
    res = cluster_updates(vals.to(_dev()), C, init=init, max_iter=max_iter)
    assert all(t.is_cuda for t in res)
    assert res.labels.dtype == torch.int32 and res.counts.dtype == torch.int32 and res.inertia.dtype == torch.float64
    assert res.labels.cpu().tolist() == want["labels"].tolist()
    assert res.counts.cpu().tolist() == want["counts"].tolist()
    assert int(res.n_iter) == want["n_iter"]
    n, gmax = u.shape[1], float((u * u).sum(1).max())
    # 1e-9 relative, as for the three groups; only an inertia of exactly zero (every row its own centroid, duplicate rows) has no
    # relative bound and takes the absolute Gram bound on a sum of K distances instead
    slack = len(u) * 4 * n * 2.0 ** -52 * gmax if want["inertia"] == 0.0 else 0.0
    assert abs(float(res.inertia) - want["inertia"]) <= inertia_rel * want["inertia"] + slack, (float(res.inertia), want["inertia"])
    return res, want


@pytest.mark.parametrize("init", [None, [0, 4, 8], [0, 1, 2], [11, 3, 5]])
def test_kmeans_three_groups_of_four(init):
    vals = _groups(3, 4, 4099, 0.3, 21)
    res, want = _compare(vals, 3, init, 50)
    if init == [0, 1, 2]:                                                          # every seed in the first group: several sweeps,
        assert want["n_iter"] >= 2                                                 # and a local optimum that is not the three groups
    else:
        lab = want["labels"]
        assert sorted(want["counts"].tolist()) == [4, 4, 4] and want["n_iter"] >= 1
        assert all(len(set(lab[4 * g:4 * g + 4].tolist())) == 1 for g in range(3))
    u = vals.double().numpy()
    n, gmax = u.shape[1], float((u * u).sum(1).max())
    assert 12 * 4 * n * 2.0 ** -52 * gmax <= 1e-9 * want["inertia"]                # the derivation in the module docstring holds
    assert abs(float(res.inertia) - want["inertia"]) <= 1e-9 * want["inertia"]


def test_kmeans_stops_at_max_iter():
    vals = _groups(3, 4, 4099, 0.3, 21)
    full = lloyd_oracle(vals.double().numpy(), 3, [0, 1, 2], 50)
    assert full["n_iter"] >= 2                                                     # so that fewer sweeps are another answer
    res0, _ = _compare(vals, 3, [0, 1, 2], 0)
    assert int(res0.n_iter) == 0
    res1, _ = _compare(vals, 3, [0, 1, 2], 1)
    assert int(res1.n_iter) == 1


def test_kmeans_one_cluster_and_one_cluster_per_row():
    vals = _groups(5, 1, 259, 0.3, 4)
    res, _ = _compare(vals, 1, None, 50)
    assert res.labels.cpu().tolist() == [0] * 5 and res.counts.cpu().tolist() == [5] and int(res.n_iter) == 1
    res, want = _compare(vals, 5, None, 50)
    assert sorted(res.labels.cpu().tolist()) == [0, 1, 2, 3, 4] and res.counts.cpu().tolist() == [1] * 5
    assert want["inertia"] == 0.0


def test_kmeans_duplicate_rows_and_empty_clusters():
    gen = torch.Generator().manual_seed(9)
    a, b = torch.randn(131, generator=gen), 2.0 * torch.randn(131, generator=gen)
    vals = torch.stack([a, a, b, b, a])
    res, _ = _compare(vals, 2, [0, 1], 50)                                         # both seeds are the row a: every tie goes to cluster 0
    assert res.labels.cpu().tolist() == [0] * 5 and res.counts.cpu().tolist() == [5, 0]
    res, _ = _compare(vals, 2, None, 50)                                           # farthest-first: b (the larger), then the first a
    assert res.labels.cpu().tolist() == [1, 1, 0, 0, 1] and res.counts.cpu().tolist() == [2, 3]
    res, _ = _compare(vals, 3, None, 50)                                           # more clusters than distinct rows: one stays empty
    assert res.labels.cpu().tolist() == [1, 1, 0, 0, 1] and res.counts.cpu().tolist() == [2, 3, 0]
    assert np.isfinite(float(res.inertia)) and abs(float(res.inertia)) <= 1e-9


def test_kmeans_sixty_four_rows_in_eight_clusters():
    vals = _groups(8, 8, 259, 0.3, 13)
    res, want = _compare(vals, 8, None, 50)
    assert res.counts.cpu().tolist() == [8] * 8
    _compare(vals, 8, list(range(8)), 50)                                          # every seed in the first group


def test_kmeans_refuses_bad_counts():
    from nerve_cl import _nvq
    g = torch.eye(4, dtype=torch.float64, device=_dev())
    out = [torch.zeros(8, dtype=torch.int32, device=_dev()) for _ in range(3)]
    inertia = torch.zeros(1, dtype=torch.float64, device=_dev())
    for K, C in ((4, 5), (4, 0), (65, 2), (16, 9)):
        rc = _nvq.lib().nvq_cluster_gram_kmeans(g.data_ptr(), K, C, None, 5, out[0].data_ptr(), out[1].data_ptr(), inertia.data_ptr(),
                                                out[2].data_ptr(), None)
        assert rc == -1, (K, C)


# ------------------------------------------------------------------------------------------------ clustered aggregation
def _fed_aggregate(rows, n, base, w, sq, **kw):
    from nerve_cl import _nvq
    out = torch.full((n,), float("nan"), device=_dev())
    _nvq.fed_aggregate(rows, n, base, w, sq, out, **kw)
    return out


def _clusters(clients, n, labels, C, bases, w, sq, out=None, **kw):
    from nerve_cl import _nvq
    if out is None:
        out = torch.full((C, n), float("nan"), device=_dev())
    _nvq.fed_aggregate_clusters(clients, n, labels, C, bases, w, sq, out, **kw)
    return out


@pytest.mark.parametrize("n", [3, 4, 7, 4101])
@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_cluster_rows_equal_fed_aggregate_on_the_members(C, K, n):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(1000 * C + 10 * K + n % 7)
    vals = torch.randn(K, n, generator=gen)
    shared_v = vals.mean(0) + 0.1 * torch.randn(n, generator=gen)
    per_v = shared_v.view(1, n) + 0.1 * torch.randn(C, n, generator=gen)
    host = [(3 * k + k // 5) % C for k in range(K)]
    if K >= 5:
        host[3] = C                                                               # outside [0, C): left out of every cluster
        host[1] = -1
    clients = _place(vals, n if n % 2 else n + 4)
    labels = torch.tensor(host, dtype=torch.int32, device=_dev())
    w = torch.tensor([float(3 + (7 * k) % 5) for k in range(K)], dtype=torch.float64, device=_dev())
    shared, per = _place_vec(shared_v), _place(per_v, n + 4)
    sq = torch.zeros(K, dtype=torch.float64, device=_dev())
    _nvq.fed_delta_norms(clients, n, shared, sq, _ws())
    clip = float(sq.sqrt().median())                                               # about half the clients are clipped
    seed, offset = (1 << 40) + 77, (1 << 33) + 5
    noisy = dict(server_lr=0.5, noise_std=0.25, seed=seed, offset=offset)
    cases = [("none", None, None, {}), ("none", None, None, noisy), ("shared", shared, None, dict(server_lr=0.5)),
             ("shared", shared, sq, dict(clip_norm=clip, **noisy)), ("per", per, None, {}), ("per", per, None, noisy)]
    seen_empty = False
    for mode, bases, s, kw in cases:
        got = _clusters(clients, n, labels, C, bases, w, s, **kw)
        assert torch.isfinite(got).all()
        for c in range(C):
            members = [k for k in range(K) if host[k] == c]
            base_c = None if bases is None else (bases if mode == "shared" else per[c, :n].clone())
            kw_c = dict(kw, offset=kw["offset"] + c) if "offset" in kw else kw
            if members:
                idx = torch.tensor(members, device=_dev())
                want = _fed_aggregate(clients[idx][:, :n].contiguous(), n, base_c, w[idx], None if s is None else s[idx], **kw_c)
            else:
                seen_empty = True
                zero = base_c if base_c is not None else torch.zeros(n, device=_dev())
                if not kw.get("noise_std"):
                    want = zero                                                    # an empty cluster: its base exactly
                else:
                    want = _fed_aggregate(zero.view(1, n).clone(), n, base_c, torch.ones(1, dtype=torch.float64, device=_dev()), None,
                                          **{k: v for k, v in kw_c.items() if k != "clip_norm"})
            assert torch.equal(_bits(got[c]), _bits(want)), (mode, kw, c, members)
        if mode == "per":                                                          # out may be bases: an in-place step
            inplace = per.clone()
            assert inplace.data_ptr() % 16 == 0
            _clusters(clients, n, labels, C, inplace, w, None, out=inplace, **kw)
            assert torch.equal(_bits(inplace[:, :n]), _bits(got))
        sclients = _place(vals, n + 1 if (n + 1) % 4 else n + 2, shift=1)         # only 4-byte aligned: the scalar form
        sbases = None if bases is None else (_place_vec(shared_v, shift=1) if mode == "shared" else _place(per_v, n + 1, shift=1))
        assert torch.equal(_bits(_clusters(sclients, n, labels, C, sbases, w, s, **kw)), _bits(got)), (mode, kw)
    assert seen_empty == (len({h for h in host if 0 <= h < C}) < C)


def test_aggregate_clusters_refuses_clip_with_per_cluster_bases_and_bad_counts():
    from nerve_cl import _nvq
    from nerve_cl.federated import aggregate_flat_clustered
    clients = torch.zeros(4, 16, device=_dev())
    labels = torch.zeros(4, dtype=torch.int32, device=_dev())
    w = torch.ones(4, dtype=torch.float64, device=_dev())
    bases, out = torch.zeros(2, 16, device=_dev()), torch.zeros(2, 16, device=_dev())
    with pytest.raises(RuntimeError, match="shared base"):
        _nvq.fed_aggregate_clusters(clients, 16, labels, 2, bases, w, w, out, clip_norm=1.0)
    with pytest.raises(ValueError, match="shared base"):
        aggregate_flat_clustered(clients, w, labels, 2, bases=bases, clip_norm=1.0)
    rc = _nvq.lib().nvq_fed_aggregate_clusters(clients.data_ptr(), 16, 4, labels.data_ptr(), 9, None, 0, w.data_ptr(), None, 0.0, 1.0,
                                               0.0, 0, 0, 16, out.data_ptr(), 16, None)
    assert rc == -1


def test_aggregate_flat_clustered_device_and_cpu_agree():
    from nerve_cl.federated import aggregate_flat_clustered
    gen = torch.Generator().manual_seed(3)
    x, base = torch.randn(6, 1031, generator=gen), torch.randn(1031, generator=gen)
    labels, w = [0, 2, 0, 2, 2, 5], [1.0, 2.0, 3.0, 4.0, 0.0, 9.0]
    kw = dict(clip_norm=20.0, server_lr=0.5, noise_std=0.1, seed=11, offset=4)
    cpu = aggregate_flat_clustered(x, w, labels, 3, bases=base, **kw)
    gpu = aggregate_flat_clustered(x.to(_dev()), w, labels, 3, bases=base.to(_dev()), **kw)
    assert gpu.is_cuda and gpu.shape == (3, 1031)
    assert (cpu - gpu.cpu()).abs().max() <= 1e-6 + 2e-5 * 0.1                        # fp32 rounding of the value plus the noise bound


# ------------------------------------------------------------------------------------------------ the trainer
def _sr_net():
    from nerve_cl.models import SuperResolutionNet
    torch.manual_seed(3)
    net = SuperResolutionNet(num_features=16, num_residual_blocks=1).to(_dev()).train()
    net.deterministic = True
    return net


def _group_clips(count, seed, group):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(count, 3, 3, 16, 16, generator=g)
    y = 0.1 * torch.rand(count, 3, 32, 32, generator=g) + (1.5 if group == 0 else -0.5)   # opposite sides of the net's first output
    return x.to(_dev()), y.to(_dev())


def _within_ulps(got, want, ulps=1):
    w32 = want.abs().to(torch.float32)
    ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
    return bool(((got.double() - want).abs() <= ulps * ulp).all())


def _train_copy(start, data):
    m = copy.deepcopy(start).train()
    m.deterministic = True
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True)
    xs, ys = data
    for i in range(0, len(xs), 4):
        opt.zero_grad()
        nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4]).backward()
        opt.step()
    return m


def _check_state(net, models, weights):
    w = torch.tensor(weights, dtype=torch.float64, device=_dev())
    for k, v in net.state_dict().items():
        stack = torch.stack([m.state_dict()[k] for m in models]).double()
        mean = (stack * w.view(-1, *([1] * (stack.dim() - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert _within_ulps(v, mean), k
        else:
            assert torch.equal(v, mean.trunc().to(v.dtype)), k


def test_clustered_trainer_on_the_device():
    from nerve_cl.federated import FederatedTrainer
    net = _sr_net()
    start = copy.deepcopy(net)
    counts = [4, 8, 4, 8, 4, 4]
    data = {c: _group_clips(counts[c], 40 + c, 0 if c < 3 else 1) for c in range(6)}
    tr = FederatedTrainer(net, num_clients=6, clients_per_round=6, local_epochs=1, lr=1e-3, batch_size=4, seed=8, num_clusters=2,
                          cluster_after=0)
    for c, d in data.items():
        tr.set_client_data(c, d)
    theta_ptr = net.flat_theta().data_ptr()
    out = tr.train_round()
    assert out["round"] == 1 and out["clients"] == 6 and out["samples"] == 32 and out["clusters"] == [3, 3]
    assert net.flat_theta().data_ptr() == theta_ptr
    lab = tr.client_cluster
    assert lab[0] == lab[1] == lab[2] != lab[3] == lab[4] == lab[5]
    assert len(tr.cluster_models) == 1 and tuple(tr.cluster_models[0].shape) == (2, net.flat_theta().numel())
    trained = {c: _train_copy(start, data[c]) for c in range(6)}
    groups = {lab[0]: [0, 1, 2], lab[3]: [3, 4, 5]}
    mean_theta = net.flat_theta().clone()
    cw = [float(sum(counts[c] for c in groups[g])) for g in range(2)]
    want_mean = (tr.cluster_models[0].double() * torch.tensor(cw, dtype=torch.float64, device=_dev()).view(2, 1)).sum(0) / sum(cw)
    assert _within_ulps(mean_theta, want_mean)                                     # the model: the weighted mean of the cluster models
    starts = {}
    for g, members in groups.items():
        tr.load_cluster(g)
        w = [float(counts[c]) for c in members]
        thetas = torch.stack([trained[c].flat_theta() for c in members]).double()
        want = (thetas * torch.tensor(w, dtype=torch.float64, device=_dev()).view(-1, 1)).sum(0) / sum(w)
        assert _within_ulps(tr.cluster_models[0][g], want) and torch.equal(net.flat_theta(), tr.cluster_models[0][g])
        _check_state(net, [trained[c] for c in members], w)
        starts[g] = copy.deepcopy(net)
    assert (tr.cluster_models[0][0] != tr.cluster_models[0][1]).any()
    # a second round with every client: a FedAvg step per group from the cluster models
    out = tr.train_round()
    assert out["round"] == 2 and sorted(tr.last_selected) == list(range(6)) and out["clusters"] == [3, 3]
    for g, members in groups.items():
        again = [_train_copy(starts[g], data[c]) for c in members]
        tr.load_cluster(g)
        _check_state(net, again, [float(counts[c]) for c in members])


def test_one_cluster_is_the_unclustered_trainer_on_the_device():
    from nerve_cl.federated import FederatedTrainer
    thetas = []
    for kw in ({}, {"num_clusters": 1, "cluster_after": 1}):
        net = _sr_net()
        tr = FederatedTrainer(net, num_clients=3, clients_per_round=2, local_epochs=1, lr=1e-3, batch_size=4, seed=8, **kw)
        for c in range(3):
            tr.set_client_data(c, _group_clips(4, 60 + c, c % 2))
        outs = [tr.train_round() for _ in range(2)]
        assert "clusters" not in outs[0]
        thetas.append(net.flat_theta().clone())
    assert torch.equal(_bits(thetas[0]), _bits(thetas[1]))


def test_clustering_and_a_clustered_round_read_nothing_back():
    from nerve_cl.federated import FederatedTrainer, aggregate_flat_clustered, cluster_updates
    vals = _groups(3, 4, 4099, 0.3, 21).to(_dev())
    base = torch.zeros(4099, device=_dev())
    w = torch.ones(12, dtype=torch.float64, device=_dev())
    init = torch.tensor([0, 4, 8], dtype=torch.int32, device=_dev())
    net = _sr_net()
    tr = FederatedTrainer(net, num_clients=4, clients_per_round=2, local_epochs=1, lr=1e-3, batch_size=4, seed=8, num_clusters=2,
                          update_noise=1e-4, server_lr=0.5)
    for c in range(4):
        tr.set_client_data(c, _group_clips(4, 80 + c, c % 2))
    tr.train_round()                                                               # the split round: it reads the labels once
    tr.train_round()                                                               # warm-up of the clustered round's buffers
    cluster_updates(vals, 3, base=base)                                            # warm-up: code objects loaded, workspace built
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = cluster_updates(vals, 3, base=base)
        res2 = cluster_updates(vals, 3, base=base, init=init, max_iter=5)
        models = aggregate_flat_clustered(vals, w, res.labels, 3, bases=base, clip_norm=1.0, noise_std=0.1, seed=3)
        out = tr.train_round_device()
        try:
            res.n_iter.item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert control_raised, "torch.cuda.set_sync_debug_mode('error') does not flag .item(): the check would be vacuous"
    assert res.counts.cpu().tolist() == [4, 4, 4] and res2.counts.cpu().tolist() == [4, 4, 4] and torch.isfinite(models).all()
    assert out["round"] == 3 and out["clusters"] == tr.cluster_sizes() and np.isfinite(out["train_loss"].item())
    assert torch.isfinite(net.flat_theta()).all() and torch.isfinite(tr.cluster_models[0]).all()


# ------------------------------------------------------------------------------------------------ the script
def test_train_federated_script_with_clusters(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_federated.py"),
           "--num-clients", "4", "--clients-per-round", "2", "--num-rounds", "3", "--local-epochs", "1", "--samples", "8",
           "--features", "16", "--blocks", "1", "--clusters", "2", "--cluster-after", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rounds = [ln for ln in lines if ln.startswith("Round ")]
    assert len(rounds) == 3 and rounds[0].startswith("Round 1: 2 clients") and rounds[1].startswith("Round 2: 4 clients, 32 samples")
    split = [ln for ln in lines if "clusters after the split" in ln]
    assert len(split) == 1 and lines.index(split[0]) == lines.index(rounds[1]) + 1
    sizes = [int(v) for v in split[0].split("sizes [")[1].split("]")[0].split(",")]
    assert len(sizes) == 2 and sum(sizes) == 4
    per = [ln for ln in lines if ln.startswith("Cluster ")]
    assert len(per) == 2
    for ln in per:
        assert ln.endswith("empty") or np.isfinite(float(ln.split("eval loss")[1])), ln
