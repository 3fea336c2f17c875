"""CPU: nerve_cl.federated.clustering without a GPU - the float64 composition of aggregate_flat_clustered against the written
formula, the reference's UserClustering behaviour (feature encoding, assignment before the first fit, get_cluster and
get_cluster_stats), the host Lloyd's algorithm against the oracle of this file (and against scikit-learn where it imports), the
clustered FederatedTrainer on a plain module against independently trained copies, and the ABI declarations.

The oracles of tests/test_clustering_gpu.py live here too: short numpy float64 functions on the explicit vectors."""
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


# ------------------------------------------------------------------------------------------------ oracles
def _gap(best, second):
    """relative gap between the best and the second-best candidate; an exact tie (duplicate rows: the device sees bit-identical
    Gram rows and both sides resolve it by the index rule) does not count"""
    if not np.isfinite(second) or second == best:
        return np.inf
    return abs(second - best) / max(abs(second), abs(best))


def farthest_first_oracle(u, C):
    """seeds: the row with the largest norm, then the row that maximises its minimum distance to the seeds so far; ties to the
    lowest index.  Returns (seeds, the smallest relative gap between the chosen row and the runner-up)."""
    sq = (u * u).sum(1)
    order = np.sort(sq)[::-1]
    margin = _gap(order[0], order[1]) if len(u) > 1 else np.inf
    seeds = [int(np.argmax(sq))]
    mind = np.full(len(u), np.inf)
    for _ in range(1, C):
        mind = np.minimum(mind, ((u - u[seeds[-1]]) ** 2).sum(1))
        order = np.sort(mind)[::-1]
        if len(u) > 1:
            margin = min(margin, _gap(order[0], order[1]))
        seeds.append(int(np.argmax(mind)))
    return seeds, margin


def lloyd_oracle(u, C, init=None, max_iter=50):
    """Lloyd's algorithm on the rows of u with the rules of DESIGN.md section 25: unweighted means, ties to the lowest cluster,
    an empty cluster stays empty (distance +inf), stop when no label changes or after max_iter sweeps.  ``margin``: the smallest
    relative gap between the best and the second-best candidate over every decision taken."""
    u = np.asarray(u, dtype=np.float64)
    K = len(u)
    margin = np.inf
    if init is None:
        init, margin = farthest_first_oracle(u, C)

    def assign(centers, live):
        nonlocal margin
        d = ((u[:, None, :] - centers[None, :, :]) ** 2).sum(-1)
        d[:, ~live] = np.inf
        for k in range(K):
            s = np.sort(d[k])
            if C > 1:
                margin = min(margin, _gap(s[0], s[1]))
        return d.argmin(1), d

    def stats(labels):
        counts = np.bincount(labels, minlength=C)
        centers = np.zeros((C, u.shape[1]))
        for c in range(C):
            if counts[c]:
                centers[c] = u[labels == c].mean(0)
        return counts, centers

    labels, _ = assign(u[np.asarray(init)], np.ones(C, dtype=bool))
    n_iter = 0
    while n_iter < max_iter:
        counts, centers = stats(labels)
        new, _ = assign(centers, counts > 0)
        n_iter += 1
        changed = bool((new != labels).any())
        labels = new
        if not changed:
            break
    counts, centers = stats(labels)
    inertia = float(((u - centers[labels]) ** 2).sum(1).sum())
    return {"labels": labels, "counts": counts, "inertia": inertia, "n_iter": n_iter, "margin": margin}


def _same_partition(a, b):
    pairs = set(zip(list(a), list(b)))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


def _blobs(groups, per, d, noise, seed):
    rng = np.random.RandomState(seed)
    centers = 4.0 * rng.randn(groups, d)
    return np.concatenate([centers[g] + noise * rng.randn(per, d) for g in range(groups)])


# ------------------------------------------------------------------------------------------------ aggregation
def test_aggregate_flat_clustered_cpu_against_the_formula():
    from nerve_cl.federated import aggregate_flat, aggregate_flat_clustered
    g = torch.Generator().manual_seed(3)
    x, base = torch.randn(7, 37, generator=g), torch.randn(37, generator=g)
    per = base.view(1, 37) + 0.1 * torch.randn(3, 37, generator=g)
    x[4] = base + 10.0                                        # far above the clip bound
    labels = [0, 2, 0, 2, 2, 7, -1]                           # cluster 1 is empty; clients 5 and 6 belong to no cluster
    w = [3.0, 0.0, 5.0, 2.0, 1.0, 4.0, 4.0]
    members = {0: [0, 2], 1: [], 2: [1, 3, 4]}
    got = aggregate_flat_clustered(x, w, labels, 3)
    assert got.dtype == torch.float32 and got.shape == (3, 37)
    for c, m in members.items():
        want = oracle.aggregate(x[m].numpy(), [w[k] for k in m]) if m else np.zeros(37)
        assert (np.abs(got[c].numpy() - want) <= oracle.ulp32(want)).all(), c
    for lr in (1.0, 0.5):
        got = aggregate_flat_clustered(x, w, labels, 3, bases=base, clip_norm=1.0, server_lr=lr)
        for c, m in members.items():
            want = oracle.aggregate(x[m].numpy(), [w[k] for k in m], base.numpy(), 1.0, lr) if m else base.double().numpy()
            assert (np.abs(got[c].numpy() - want) <= oracle.ulp32(want)).all(), (c, lr)
        assert torch.equal(got[1], base)                      # the empty cluster: its base exactly
    got = aggregate_flat_clustered(x, w, labels, 3, bases=per, server_lr=0.5)
    for c, m in members.items():
        want = oracle.aggregate(x[m].numpy(), [w[k] for k in m], per[c].numpy(), None, 0.5) if m else per[c].double().numpy()
        assert (np.abs(got[c].numpy() - want) <= oracle.ulp32(want)).all(), c
    for c, m in members.items():                             # and the package's own single-model form on the gathered rows
        if m:
            assert torch.equal(got[c], aggregate_flat(x[m], [w[k] for k in m], base=per[c], server_lr=0.5))
    noisy = aggregate_flat_clustered(x, w, labels, 3, bases=per, server_lr=0.5, noise_std=0.25, seed=9, offset=4)
    for c in range(3):
        assert np.abs((noisy[c] - got[c]).numpy() - 0.25 * oracle.normals(9, 4 + c, 37)).max() <= 1e-6, c
    out = per.clone()
    assert aggregate_flat_clustered(x, w, labels, 3, bases=out, server_lr=0.5, out=out) is out        # out may be bases
    assert torch.equal(out, got)
    with pytest.raises(ValueError, match="shared base"):
        aggregate_flat_clustered(x, w, labels, 3, bases=per, clip_norm=1.0)
    with pytest.raises(ValueError):
        aggregate_flat_clustered(x, w[:-1], labels, 3)


def test_update_gram_similarity_and_cluster_updates_on_cpu_tensors():
    from nerve_cl.federated import ClusterResult, cluster_updates, update_gram, update_similarity
    rng = np.random.RandomState(2)
    dirs = rng.randn(3, 203)
    u = np.concatenate([dirs[g] + 0.3 * rng.randn(4, 203) for g in range(3)]).astype(np.float32)
    base = rng.randn(203).astype(np.float32)
    x = torch.from_numpy(u + base)
    d = x.double().numpy() - base.astype(np.float64)
    g = update_gram(x, torch.from_numpy(base))
    assert g.dtype == torch.float64 and np.abs(g.numpy() - d @ d.T).max() <= 1e-9
    x0 = torch.cat([x, torch.from_numpy(base).view(1, -1)])   # a client that did not move
    s = update_similarity(x0, torch.from_numpy(base)).numpy()
    assert np.isfinite(s).all() and (s[12] == 0).all() and np.abs(np.diag(s)[:12] - 1.0).max() <= 1e-12
    for init in (None, [0, 1, 2]):
        want = lloyd_oracle(d, 3, init, 50)
        assert want["margin"] > 1e-6
        res = cluster_updates(x, 3, base=torch.from_numpy(base), init=init)
        assert isinstance(res, ClusterResult) and res.labels.dtype == torch.int32
        assert res.labels.tolist() == want["labels"].tolist() and res.counts.tolist() == want["counts"].tolist()
        assert int(res.n_iter) == want["n_iter"] and float(res.inertia) == pytest.approx(want["inertia"], rel=1e-12)
    with pytest.raises(ValueError):
        cluster_updates(x, 13)
    with pytest.raises(ValueError):
        cluster_updates(x, 2, init=[1, 1])


# ------------------------------------------------------------------------------------------------ the reference's names
def _profile(uid, **kw):
    from nerve_cl.federated import UserProfile
    base = dict(content_preferences={"sports": 2.0, "news": 0.5, "cooking": 9.0}, quality_preference=0.75, network_pattern="cellular",
                device_tier="mid")
    base.update(kw)
    return UserProfile(user_id=uid, **base)


def test_extract_features_is_the_reference_encoding():
    from nerve_cl.federated import UserClustering, UserProfile
    uc = UserClustering(num_clusters=3)
    f = uc._extract_features(_profile("u"))
    assert f.dtype == np.float64 and f.tolist() == [2.0, 0.0, 0.0, 0.5, 0.0, 0.75, 1.0, 0.5]
    f = uc._extract_features(UserProfile("v", {"music": 1.5, "animation": 0.25, "movie": 3.0}, 0.0, "wifi", "high"))
    assert f.tolist() == [0.0, 0.25, 3.0, 0.0, 1.5, 0.0, 0.0, 1.0]
    f = uc._extract_features(UserProfile("w", {}, 1.0, "satellite", "unknown"))        # unknown codes: 0.5
    assert f.tolist() == [0.0] * 5 + [1.0, 0.5, 0.5]
    assert uc._extract_features(_profile("x", network_pattern="mixed", device_tier="low")).tolist()[6:] == [0.5, 0.0]
    assert _profile("y").update_vector is None


def test_assignment_before_the_first_fit_and_lookups():
    from nerve_cl.federated import UserClustering
    uc = UserClustering(num_clusters=3)
    assert (uc.num_clusters, uc.method, uc.update_frequency) == (3, "kmeans", 10) and uc.clusterer is None
    assert uc.clusters == {0: [], 1: [], 2: []} and uc.cluster_models == {}
    got = [uc.register_user(_profile(f"u{i}", quality_preference=i / 4)) for i in range(5)]
    assert got == [1, 2, 0, 1, 2]                               # len(users) % num_clusters, counted after the insertion
    assert uc.clusters == {0: ["u2"], 1: ["u0", "u3"], 2: ["u1", "u4"]}
    assert uc.get_cluster("u3") == 1 and uc.get_cluster("u2") == 0 and uc.get_cluster("nobody") == 0
    stats = uc.get_cluster_stats()
    assert set(stats) == {0, 1, 2} and stats[1]["size"] == 2 and stats[1]["avg_quality_pref"] == pytest.approx((0 + 0.75) / 2)
    assert stats[1]["content_mix"] == "cooking"
    few = UserClustering(num_clusters=4)
    few.register_user(_profile("a"))
    few.update_clusters()                                       # fewer users than clusters: nothing happens
    assert few.clusterer is None and few.get_cluster_stats() == {1: {"size": 1, "avg_quality_pref": 0.75, "content_mix": "cooking"}}
    empty = UserClustering(num_clusters=2)
    empty.register_user(_profile("b", content_preferences={}))
    assert empty.get_cluster_stats()[1]["content_mix"] == "unknown"


def _populate(uc, seed=0):
    rng = np.random.RandomState(seed)
    kinds = [dict(content_preferences={"sports": 8.0}, quality_preference=0.9, network_pattern="wifi", device_tier="high"),
             dict(content_preferences={"news": 8.0}, quality_preference=0.1, network_pattern="cellular", device_tier="low"),
             dict(content_preferences={"music": 8.0, "movie": 4.0}, quality_preference=0.5, network_pattern="mixed", device_tier="mid")]
    truth = {}
    for i in range(18):
        k = dict(kinds[i % 3])
        k["content_preferences"] = {ct: v + 0.2 * rng.rand() for ct, v in k["content_preferences"].items()}
        uc.register_user(_profile(f"u{i}", **k))
        truth[f"u{i}"] = i % 3
    return truth


def test_update_clusters_groups_the_profiles_and_predicts_new_users():
    from nerve_cl.federated import UserClustering
    uc = UserClustering(num_clusters=3)
    truth = _populate(uc)
    uc.update_clusters()
    assert uc.clusterer is not None and uc.clusterer.cluster_centers_.shape == (3, 8)
    assert sorted(len(v) for v in uc.clusters.values()) == [6, 6, 6]
    assert _same_partition([truth[u] for u in truth], [uc.get_cluster(u) for u in truth])
    feats = np.array([uc._extract_features(uc.users[u]) for u in uc.users])
    want = lloyd_oracle(feats, 3, init=None, max_iter=300)     # another start, the same partition on separated data
    assert _same_partition(want["labels"], uc.clusterer.labels_)
    again = UserClustering(num_clusters=3)
    _populate(again)
    again.update_clusters()
    assert again.clusters == uc.clusters                        # seeded: the same fit every time
    new = uc.register_user(_profile("late", content_preferences={"news": 8.1}, quality_preference=0.1, network_pattern="cellular",
                                    device_tier="low"))
    assert new == uc.get_cluster("u1") and "late" in uc.clusters[new]
    stats = uc.get_cluster_stats()
    assert stats[uc.get_cluster("u0")]["content_mix"] == "sports" and stats[new]["size"] == 7


def test_host_lloyd_follows_the_rules():
    from nerve_cl.federated.clustering import _lloyd
    x = _blobs(4, 6, 5, 0.3, 1)
    for init in ([0, 1, 2, 3], [0, 6, 12, 18], [23, 2, 9, 14]):
        want = lloyd_oracle(x, 4, init, 300)
        labels, counts, inertia, n_iter, centers = _lloyd(x, 4, init=init)
        assert labels.tolist() == want["labels"].tolist() and counts.tolist() == want["counts"].tolist() and n_iter == want["n_iter"]
        assert inertia == pytest.approx(want["inertia"], rel=1e-12)
    a, b = x[0], x[7]
    dup = np.stack([a, a, b, b, a])
    labels, counts, inertia, n_iter, _ = _lloyd(dup, 2, init=[0, 1])        # both seeds are the row a: ties go to cluster 0
    assert labels.tolist() == [0] * 5 and counts.tolist() == [5, 0] and np.isfinite(inertia)
    labels, counts, _, n_iter, _ = _lloyd(x, 4, init=[0, 1, 2, 3], max_iter=0)
    assert n_iter == 0 and labels.tolist() == lloyd_oracle(x, 4, [0, 1, 2, 3], 0)["labels"].tolist()


def test_update_clusters_agrees_with_scikit_learn_on_separated_blobs():
    cluster = pytest.importorskip("sklearn.cluster")
    from nerve_cl.federated.clustering import _lloyd
    x = _blobs(4, 10, 8, 0.2, 5)
    labels, counts, _, _, _ = _lloyd(x, 4, seed=42)
    theirs = cluster.KMeans(n_clusters=4, random_state=42, n_init=10).fit_predict(x)
    assert _same_partition(labels, theirs) and sorted(counts.tolist()) == [10] * 4


def test_user_clustering_by_update_fills_the_clusters():
    from nerve_cl.federated import UserClustering
    rng = np.random.RandomState(4)
    dirs = rng.randn(2, 301)
    u = np.concatenate([dirs[g] + 0.2 * rng.randn(3, 301) for g in range(2)]).astype(np.float32)
    base = rng.randn(301).astype(np.float32)
    uc = UserClustering(num_clusters=2)
    ids = [f"u{i}" for i in range(6)]
    res = uc.cluster_updates(ids, torch.from_numpy(u + base), torch.from_numpy(base))
    assert sorted(sorted(v) for v in uc.clusters.values()) == [["u0", "u1", "u2"], ["u3", "u4", "u5"]]
    assert res.counts.tolist() == [3, 3] and uc.get_cluster("u4") == uc.get_cluster("u5") != uc.get_cluster("u0")


# ------------------------------------------------------------------------------------------------ the trainer
def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.BatchNorm1d(7), nn.ReLU(), nn.Linear(7, 3))


COUNTS = [6, 8, 6, 10, 6, 8]


def _data():
    g = torch.Generator().manual_seed(11)
    out = {}
    for c in range(6):
        x = torch.randn(COUNTS[c], 5, generator=g)
        y = (2.0 if c < 3 else -2.0) + 0.1 * torch.randn(COUNTS[c], 3, generator=g)   # two groups with opposite targets
        out[c] = (x, y)
    return out


def _trainer(model, **kw):
    from nerve_cl.federated import FederatedTrainer
    tr = FederatedTrainer(model, num_clients=6, clients_per_round=6, local_epochs=2, lr=1e-2, batch_size=4, **kw)
    for c, d in _data().items():
        tr.set_client_data(c, d)
    return tr


def _train_copy(start, data):
    m = copy.deepcopy(start).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    xs, ys = data
    for _ in range(2):
        for i in range(0, len(xs), 4):
            opt.zero_grad()
            nn.functional.mse_loss(m(xs[i:i + 4]), ys[i:i + 4]).backward()
            opt.step()
    return m


def _check_state(model, copies, w):
    w = np.array(w, dtype=np.float64)
    for k, v in model.state_dict().items():
        stack = np.stack([m.state_dict()[k].double().numpy() for m in copies])
        want = (stack * w.reshape(-1, *([1] * (stack.ndim - 1)))).sum(0) / w.sum()
        if v.is_floating_point():
            assert (np.abs(v.numpy() - want) <= oracle.ulp32(want)).all(), k
        else:
            assert int(v) == int(np.trunc(want)), k


def test_clustered_trainer_equals_per_group_fedavg_of_independent_copies():
    model = _net()
    start = copy.deepcopy(model)
    tr = _trainer(model, seed=5, num_clusters=2, cluster_after=0)
    data = _data()
    out = tr.train_round()
    assert out["round"] == 1 and out["clients"] == 6 and out["samples"] == sum(COUNTS) and out["clusters"] == [3, 3]
    lab = tr.client_cluster
    assert lab[0] == lab[1] == lab[2] != lab[3] == lab[4] == lab[5]
    groups = {lab[0]: [0, 1, 2], lab[3]: [3, 4, 5]}
    trained = {c: _train_copy(start, data[c]) for c in range(6)}
    mean_state = {k: v.clone() for k, v in model.state_dict().items()}
    starts, cluster_states = {}, {}
    for g, members in groups.items():
        tr.load_cluster(g)
        _check_state(model, [trained[c] for c in members], [COUNTS[c] for c in members])
        starts[g] = copy.deepcopy(model)
        cluster_states[g] = {k: v.clone() for k, v in model.state_dict().items()}
    cw = np.array([sum(COUNTS[c] for c in groups[g]) for g in range(2)], dtype=np.float64)
    for k, v in mean_state.items():                             # the model: the weighted mean of the cluster models
        if v.is_floating_point():
            want = sum(cw[g] * cluster_states[g][k].double().numpy() for g in range(2)) / cw.sum()
            assert (np.abs(v.numpy() - want) <= oracle.ulp32(want)).all(), k
    out = tr.train_round()                                      # every client again: one FedAvg step per group from its cluster model
    assert out["round"] == 2 and sorted(tr.last_selected) == list(range(6))
    for g, members in groups.items():
        again = [_train_copy(starts[g], data[c]) for c in members]
        tr.load_cluster(g)
        _check_state(model, again, [COUNTS[c] for c in members])


def test_plain_rounds_come_first_with_cluster_after():
    model = _net()
    tr = _trainer(model, seed=5, num_clusters=2, cluster_after=1)
    out = tr.train_round()
    assert out["clusters"] == [0, 0] and tr.cluster_models is None and tr.client_cluster == {}
    with pytest.raises(RuntimeError):
        tr.load_cluster(0)
    out = tr.train_round()
    assert out["clusters"] == [3, 3] and out["clients"] == 6


def test_members_without_samples_and_late_clients():
    model = _net()
    tr = _trainer(model, seed=5, num_clusters=2, cluster_after=0)
    tr.train_round()
    lab = tr.client_cluster
    g = lab[3]                                                  # from now on the second group's clients hold no samples
    for c in (3, 4, 5):
        x, y = tr.client_data[c]
        tr.set_client_data(c, (x[:0], y[:0]))
    tr.load_cluster(g)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    out = tr.train_round()
    assert out["clients"] == 6 and out["samples"] == sum(COUNTS[:3])
    tr.load_cluster(g)                                          # no division by W_c = 0: the cluster kept its model
    for k, v in model.state_dict().items():
        assert torch.isfinite(v.double()).all() and torch.equal(v, before[k]), k
    tr.load_mean()
    assert all(torch.isfinite(v.double()).all() for v in model.state_dict().values())
    tr.set_client_data(6, _data()[0])                           # data that arrives after the split: no cluster, no re-clustering
    tr.clients_per_round = 7                                    # every client is selected, the late one among them
    with pytest.raises(ValueError, match="after the split"):
        tr.train_round()


def test_one_cluster_reproduces_the_unclustered_trainer_bit_for_bit():
    states = []
    for kw in ({}, {"num_clusters": 1, "cluster_after": 1}):
        model = _net()
        tr = _trainer(model, seed=77, update_clip=0.5, update_noise=0.01, server_lr=0.5, **kw)
        tr.clients_per_round = 3
        outs = [tr.train_round() for _ in range(2)]
        assert all("clusters" not in o for o in outs)
        states.append([v.clone() for v in model.state_dict().values()])
    assert all(torch.equal(a, b) for a, b in zip(*states))


def test_constructor_refuses_clip_and_too_many_clients_with_clusters():
    from nerve_cl.federated import FederatedTrainer
    with pytest.raises(NotImplementedError, match="update_clip"):
        FederatedTrainer(_net(), num_clients=4, clients_per_round=2, num_clusters=2, update_clip=1.0)
    with pytest.raises(ValueError, match="num_clients"):
        FederatedTrainer(_net(), num_clients=65, clients_per_round=2, num_clusters=2)
    with pytest.raises(ValueError, match="num_clusters"):
        FederatedTrainer(_net(), num_clients=4, clients_per_round=2, num_clusters=9)
    FederatedTrainer(_net(), num_clients=65, clients_per_round=2)                   # fine without clusters
    tr = FederatedTrainer(_net(), num_clients=2, clients_per_round=2, num_clusters=2)
    for c, d in _data().items():
        tr.set_client_data(c, d)
    with pytest.raises(ValueError, match="num_clients"):                            # six clients with data, rows for two
        tr.train_round()
    FederatedTrainer(_net(), num_clients=64, clients_per_round=2, num_clusters=2)


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_clustering_symbols():
    from nerve_cl import _nvq
    header = open(os.path.join(os.path.dirname(HERE), "include", "nvq.h")).read()
    for name in ("nvq_fed_gram_workspace_bytes", "nvq_fed_update_gram", "nvq_cluster_gram_kmeans", "nvq_fed_aggregate_clusters"):
        assert name + "(" in header and name in _nvq.SIGNATURES, name
    import nerve_cl.federated as fed
    for name in ("UserProfile", "UserClustering", "ClusterResult", "update_gram", "update_similarity", "cluster_updates",
                 "aggregate_flat_clustered"):
        assert name in fed.__all__ and hasattr(fed, name), name
