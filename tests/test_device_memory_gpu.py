"""GPU: nerve_cl.continual.DeviceEpisodicMemory and the libnvq replay kernels (csrc/replay.hip).

The oracle for the host-planned strategies is the repository's own EpisodicMemory (pinned to the reference by
tests/test_continual_cpu.py): same seed, same calls, bit-identical results in fp32 storage.  bf16 storage is checked against
``x.to(torch.bfloat16)``, the weighted sampler against a numpy float64 evaluation of the same keys (exact) and against the
enumerated successive-sampling inclusion probabilities (distribution)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(REPO, "experiments")
TYPES = ("sports", "animation", "news")


def _mems(strategy, capacity, seed, **kw):
    from nerve_cl.continual import DeviceEpisodicMemory, EpisodicMemory
    return DeviceEpisodicMemory(capacity=capacity, strategy=strategy, seed=seed, device="cuda", **kw), \
        EpisodicMemory(capacity=capacity, strategy=strategy, seed=seed)


def _assert_same_state(dev, host):
    assert len(dev) == len(host) and dev.total_seen == host.total_seen and dev.get_stats() == host.get_stats()
    snap = dev.buffer
    assert len(snap) == len(host.buffer)
    for a, b in zip(snap, host.buffer):
        assert a.frame_lr.is_cuda and torch.equal(a.frame_lr.cpu(), b.frame_lr) and torch.equal(a.frame_hr.cpu(), b.frame_hr)
        assert a.metadata == b.metadata and a.importance == b.importance and a.access_count == b.access_count


# ------------------------------------------------------------------------------------------------ 1. equivalence
@pytest.mark.parametrize("strategy", ["uniform", "fifo", "reservoir", "stratified"])
@pytest.mark.parametrize("lr_shape,hr_shape", [((3, 8, 8), (3, 16, 16)), ((3, 5, 7), (3, 10, 14))])
def test_same_seed_same_results_as_the_host_class(strategy, lr_shape, hr_shape):
    """(3, 5, 7) / (3, 10, 14): rows of 105 / 420 elements - 105 is no multiple of 4: the scalar instantiation"""
    dev, host = _mems(strategy, 7, 11)
    g = torch.Generator().manual_seed(5)
    draws = 0
    for i in range(24):
        meta = {"content_type": TYPES[(i * i + i // 3) % 3], "i": i} if i != 4 else {"i": i}
        lr, hr = torch.rand(lr_shape, generator=g), torch.rand(hr_shape, generator=g)
        src = (lr.cuda(), hr.cuda()) if i % 2 else (lr, hr)                 # GPU and CPU sources
        assert dev.store(*src, meta, 0.5 + 0.25 * (i % 3)) == host.store(lr, hr, meta, 0.5 + 0.25 * (i % 3))
        requests = []
        if i == 2:
            requests.append((5, None))                                      # larger than the fill
        if i % 5 == 4:
            requests.append((4, None))
        if i % 7 == 6:
            requests.append((3, TYPES[i % 3]))
        if i == 15:
            requests += [(2, "documentary"), (50, None)]
        for k, ct in requests:
            a, b = dev.sample(k, content_type=ct), host.sample(k, content_type=ct)
            assert a[0].is_cuda and a[0].dtype == torch.float32
            assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1]) and a[2] == b[2]
            draws += 1
        _assert_same_state(dev, host)
    assert draws >= 8 and len(host) == 7 and host.total_seen == 24
    with pytest.raises(AttributeError):
        dev.buffer = []
    with pytest.raises(ValueError, match="one shape"):
        dev.store(torch.zeros(3, 9, 9), torch.zeros(hr_shape))


# ------------------------------------------------------------------------------------------------ 2. bf16 storage
def _bf16_cases(n):
    """fp32 values that exercise the rounding: ties to even both ways, a carry into the next exponent, subnormals,
    the largest finite value (rounds to inf), inf, and one NaN"""
    special = torch.from_numpy(np.array([0x3f808000, 0x3f818000, 0x3f80ffff, 0x3fffffff, 0x00000001, 0x00008000, 0x00018000,
                                         0x007fffff, 0x80000001, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00001,
                                         0x3f800000, 0x80000000], dtype=np.uint32).view(np.float32))
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(n, generator=g) - 0.5) * 8
    x[:special.numel()] = special
    return x


@pytest.mark.parametrize("lr_shape,hr_shape", [((3, 8, 8), (3, 16, 16)), ((3, 5, 7), (3, 10, 14))])
def test_bf16_storage_rounds_like_torch(lr_shape, hr_shape):
    from nerve_cl.continual import DeviceEpisodicMemory
    mem = DeviceEpisodicMemory(capacity=4, strategy="fifo", seed=0, device="cuda", storage="bf16")
    nl, nh = int(np.prod(lr_shape)), int(np.prod(hr_shape))
    stored = {}
    for i in range(4):
        lr, hr = _bf16_cases(nl).roll(7 * i).reshape(lr_shape), _bf16_cases(nh).roll(3 * i).reshape(hr_shape)
        mem.store(lr.cuda() if i % 2 else lr, hr, {"i": i})
        stored[i] = (lr, hr)
    a_lr, a_hr, metas = mem.sample(4)
    assert sorted(m["i"] for m in metas) == [0, 1, 2, 3]
    for row, m in enumerate(metas):
        for got, src in ((a_lr[row].cpu(), stored[m["i"]][0]), (a_hr[row].cpu(), stored[m["i"]][1])):
            want = src.to(torch.bfloat16).to(torch.float32)
            assert torch.isnan(src).any() and torch.isinf(want).sum() > torch.isinf(src).sum()   # the cases are really there
            assert torch.equal(torch.isnan(got), torch.isnan(want))                               # NaN positions, not payloads
            ok = ~torch.isnan(want)
            assert torch.equal(got[ok].view(torch.int32), want[ok].view(torch.int32))             # bit for bit (incl. -0, subnormals)
    assert mem._lr.dtype == torch.bfloat16 and mem._hr.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------ 3. batches
def _pattern(n, shape, salt):
    """arange-derived values, all distinct per (sample, position): a misplaced row or chunk changes the tensor"""
    per = int(np.prod(shape))
    i = torch.arange(n * per, dtype=torch.float64).reshape((n,) + tuple(shape))
    return ((i * 0.6180339887 + salt) % 1.0).float() + (i // per).float()


@pytest.mark.parametrize("strategy", ["fifo", "stratified"])
def test_store_batch_equals_store_calls(strategy):
    from nerve_cl.continual import DeviceEpisodicMemory
    one = DeviceEpisodicMemory(capacity=5, strategy=strategy, seed=3, device="cuda")
    many = DeviceEpisodicMemory(capacity=5, strategy=strategy, seed=3, device="cuda")
    for b in range(3):
        lr, hr = _pattern(6, (3, 8, 8), b).cuda(), _pattern(6, (3, 16, 16), b + 0.5).cuda()
        types = [TYPES[(j * j + b) % 3] for j in range(6)]
        kept = many.store_batch(lr, hr, content_type=types, importance=[0.5 + j for j in range(6)])
        assert kept == [one.store(lr[j], hr[j], {"content_type": types[j]}, 0.5 + j) for j in range(6)]
        for x, y in zip(many.buffer, one.buffer):
            assert torch.equal(x.frame_lr, y.frame_lr) and torch.equal(x.frame_hr, y.frame_hr)
            assert x.metadata == y.metadata and x.importance == y.importance and x.access_count == 0
        assert torch.equal(many._time, one._time) and torch.equal(many._means, one._means)
        assert torch.equal(many._type, one._type)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_replay_batch_equals_cat_of_sample(storage):
    from nerve_cl.continual import DeviceEpisodicMemory
    a = DeviceEpisodicMemory(capacity=6, strategy="reservoir", seed=21, device="cuda", storage=storage)
    b = DeviceEpisodicMemory(capacity=6, strategy="reservoir", seed=21, device="cuda", storage=storage)
    lr, hr = _pattern(9, (3, 6, 10), 0.1).cuda(), _pattern(9, (3, 12, 20), 0.2).cuda()
    for m in (a, b):
        m.store_batch(lr, hr, content_type=[TYPES[j % 3] for j in range(9)])
    wide_lr, wide_hr = _pattern(4, (3, 6, 20), 0.3).cuda(), _pattern(4, (3, 12, 40), 0.4).cuda()
    cur_lr, cur_hr = wide_lr[:, :, :, ::2], wide_hr[:, :, :, 1::2]          # non-contiguous views
    assert not cur_lr.is_contiguous()
    for n, ct in ((3, None), (2, "animation"), (40, None)):
        got_lr, got_hr, idx = a.replay_batch(cur_lr, cur_hr, n, content_type=ct)
        r_lr, r_hr, _ = b.sample(n, content_type=ct)
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.numel() == r_lr.shape[0]
        assert torch.equal(got_lr, torch.cat([cur_lr, r_lr])) and torch.equal(got_hr, torch.cat([cur_hr, r_hr]))
        assert torch.equal(a._access, b._access)


@pytest.mark.timeout(600)
def test_full_size_samples_land_where_they_belong():
    """2 samples of 3x540x960 / 3x1080x1920 (the cfg2 sizes): store_batch, then replay_batch behind a 1-sample batch"""
    from nerve_cl.continual import DeviceEpisodicMemory
    lr_shape, hr_shape = (3, 540, 960), (3, 1080, 1920)
    lr, hr = _pattern(3, lr_shape, 0.25).cuda(), _pattern(3, hr_shape, 0.75).cuda()
    for storage in ("fp32", "bf16"):
        a = DeviceEpisodicMemory(capacity=2, strategy="fifo", seed=4, device="cuda", storage=storage)
        b = DeviceEpisodicMemory(capacity=2, strategy="fifo", seed=4, device="cuda", storage=storage)
        a.store_batch(lr[:2], hr[:2], content_type="movie")
        b.store(lr[0], hr[0], {"content_type": "movie"})
        b.store(lr[1], hr[1], {"content_type": "movie"})
        got_lr, got_hr, idx = a.replay_batch(lr[2:], hr[2:], 2)
        r_lr, r_hr, _ = b.sample(2)
        assert torch.equal(got_lr, torch.cat([lr[2:], r_lr])) and torch.equal(got_hr, torch.cat([hr[2:], r_hr]))
        slots = idx.tolist()
        assert sorted(slots) == [0, 1]
        for row, s in enumerate(slots):
            want_lr, want_hr = lr[s], hr[s]
            if storage == "bf16":
                want_lr, want_hr = want_lr.to(torch.bfloat16).float(), want_hr.to(torch.bfloat16).float()
            assert torch.equal(got_lr[1 + row], want_lr) and torch.equal(got_hr[1 + row], want_hr)
        del a, b, got_lr, got_hr, r_lr, r_hr
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 4. sampler, exact
def sampler_case(name):
    """(importance, time, type_id, now, recency_weight, type_filter, uniforms, k) of one exact-sampler case, on the CPU"""
    g = torch.Generator().manual_seed({"few": 1, "nonpositive": 2, "all": 3, "duplicates": 4}[name])
    cap = 48
    imp = torch.rand(cap, generator=g) * 1.8 + 0.2
    time = torch.randint(1, 60, (cap,), generator=g, dtype=torch.int32)
    tid = torch.randint(0, 3, (cap,), generator=g, dtype=torch.int32)
    tid[torch.randperm(cap, generator=g)[:6]] = -1                              # empty slots
    u = torch.rand(cap, generator=g).clamp_(1e-6, 1 - 1e-6)
    now, rw, filt, k = 60, 0.3, -1, 8
    if name == "few":
        tid[tid == 2] = 0
        tid[torch.tensor([5, 17, 30])] = 2
        filt = 2                                                                # 3 eligible slots < k
    elif name == "nonpositive":
        rw = 0.0
        imp[::3] = 0.0
        imp[1::5] = -0.5                                                        # never drawn
    elif name == "all":
        filt = 1
        k = int((tid == 1).sum())                                               # k == number of eligible slots
        assert 0 < k <= 256
    elif name == "duplicates":
        rw = 0.0
        imp[:] = 0.75                                                           # equal weights: the uniforms separate the keys
    return imp, time, tid, now, rw, filt, u, k


def sampler_reference(imp, time, tid, now, rw, filt, u, k):
    """numpy float64: (expected indices padded with -1, sorted eligible keys)"""
    w = (1.0 - float(np.float32(rw))) * imp.double().numpy() + float(np.float32(rw)) / (1.0 + now - time.double().numpy())
    ok = (tid.numpy() >= 0) & (w > 0)
    if filt >= 0:
        ok &= tid.numpy() == filt
    key = np.where(ok, np.log(u.double().numpy()) / np.where(ok, w, 1.0), -np.inf)
    order = sorted(np.nonzero(ok)[0].tolist(), key=lambda i: (-key[i], i))
    picks = order[:k]
    return picks + [-1] * (k - len(picks)), [key[i] for i in order]


def assert_well_conditioned(keys, k):
    """adjacent keys among the first k + 1 differ by more than 1e-4 relative: fp32 log / divide cannot reorder them"""
    head = keys[:k + 1]
    for a, b in zip(head, head[1:]):
        assert abs(a - b) > 1e-4 * max(abs(a), abs(b)), (a, b)


@pytest.mark.parametrize("name", ["few", "nonpositive", "all", "duplicates"])
def test_weighted_sampler_matches_float64_keys(name):
    from nerve_cl import _nvq
    imp, time, tid, now, rw, filt, u, k = sampler_case(name)
    want, keys = sampler_reference(imp, time, tid, now, rw, filt, u, k)
    assert_well_conditioned(keys, k)
    if name == "few":
        assert want.count(-1) == k - 3
    if name == "nonpositive":
        assert (imp <= 0).sum() >= 20 and all(imp[i] > 0 for i in want if i >= 0)
    if name == "all":
        assert -1 not in want and len(keys) == k
    out = torch.full((k,), -7, dtype=torch.int32, device="cuda")
    _nvq.replay_sample_weighted(imp.cuda(), time.cuda(), tid.cuda(), now, rw, filt, u.cuda(), out)
    assert out.tolist() == want
    got = [i for i in out.tolist() if i >= 0]
    assert len(set(got)) == len(got)


def large_sampler_case(cap):
    g = torch.Generator().manual_seed(cap)
    imp = torch.rand(cap, generator=g) * 1.8 + 0.2
    imp[::7] = 0.0
    time = torch.randint(1, 500, (cap,), generator=g, dtype=torch.int32)
    tid = torch.randint(0, 3, (cap,), generator=g, dtype=torch.int32)
    tid[torch.randperm(cap, generator=g)[:cap // 10]] = -1
    u = torch.rand(cap, generator=g).clamp_(1e-6, 1 - 1e-6)
    return imp, time, tid, 500, 0.25, 1, u, 12


@pytest.mark.parametrize("cap", [1000, 5000, 65536])
def test_weighted_sampler_matches_float64_keys_at_large_capacities(cap):
    """every thread of the one workgroup holds several slots' keys (up to 64 at capacity 65536)"""
    from nerve_cl import _nvq
    case = large_sampler_case(cap)
    want, keys = sampler_reference(*case)
    assert_well_conditioned(keys, case[-1])
    assert -1 not in want
    out = torch.full((case[-1],), -7, dtype=torch.int32, device="cuda")
    imp, time, tid, now, rw, filt, u, k = case
    _nvq.replay_sample_weighted(imp.cuda(), time.cuda(), tid.cuda(), now, rw, filt, u.cuda(), out)
    assert out.tolist() == want


def test_kernel_limits_are_refused_with_an_error_code():
    """out-of-contract sizes never reach a launch: NVQ_EINVAL (-1) and a message"""
    from nerve_cl import _nvq
    lib = _nvq.lib()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = _nvq.ptr
    assert lib.nvq_replay_sample_weighted(p(t), p(i), p(i), 64, 0, 0.0, -1, p(t), 257, p(i), None) == -1
    assert b"k <= 256" in lib.nvq_last_error()
    assert lib.nvq_replay_sample_weighted(p(t), p(i), p(i), 65537, 0, 0.0, -1, p(t), 4, p(i), None) == -1
    assert lib.nvq_replay_gather(p(t), p(t), 0, 4, 16, 16, p(i), 2, p(t), p(t), -1, p(i), None) == -1
    assert b"row0" in lib.nvq_last_error()
    assert lib.nvq_replay_update_importance(p(t), 0, p(i), p(t), 4, 0.5, None) == -1
    assert lib.nvq_replay_nearest(None, p(t), p(i), 32, 2, p(i), p(t), None) == -1
    from nerve_cl.continual import DeviceEpisodicMemory
    mem = DeviceEpisodicMemory(capacity=3, device="cuda")
    mem.store(torch.zeros(3, 4, 4), torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="outside"):
        mem.update_importance([3], torch.ones(1, device="cuda"))
    with pytest.raises(ValueError, match="outside"):
        _nvq.replay_gather(mem._lr, mem._hr, torch.zeros(2, dtype=torch.int32, device="cuda"),
                           torch.zeros(2, 3, 4, 4, device="cuda"), torch.zeros(2, 3, 8, 8, device="cuda"), 1, mem._access)


# ------------------------------------------------------------------------------------------------ 5. sampler, distribution
def inclusion_probabilities(w, k=2):
    """exact inclusion probability of every item under successive weighted sampling without replacement (k = 2), by
    enumerating the ordered pairs"""
    assert k == 2
    W = float(sum(w))
    p = [0.0] * len(w)
    for i, j in itertools.permutations(range(len(w)), 2):
        pr = w[i] / W * w[j] / (W - w[i])
        p[i] += pr
        p[j] += pr
    return p


def assert_inclusion(counts, N, w):
    p = inclusion_probabilities(w)
    assert abs(sum(p) - 2.0) < 1e-12
    bound = [4.0 * (q * (1 - q) / N) ** 0.5 for q in p]
    assert bound[0] < abs(p[0] - 1 / 3) and bound[-1] < abs(p[-1] - 1 / 3)       # N tells slots 1 and 6 from uniform
    for c, q, b in zip(counts, p, bound):
        assert abs(c / N - q) <= b, (counts, p, bound)


def test_inclusion_bound_holds_for_a_numpy_sampler_of_the_same_scheme():
    """(runs without the kernels: the statistical assertion itself, on Efraimidis-Spirakis keys drawn with numpy)"""
    w = np.arange(1.0, 7.0)
    rng = np.random.default_rng(2024)
    N = 4000
    keys = np.log(rng.random((N, 6))) / w
    top2 = np.argsort(-keys, axis=1)[:, :2]
    assert_inclusion(np.bincount(top2.ravel(), minlength=6).tolist(), N, w.tolist())


def test_weighted_sampler_distribution():
    from nerve_cl.continual import DeviceEpisodicMemory
    mem = DeviceEpisodicMemory(capacity=6, strategy="fifo", seed=1234, device="cuda")
    for i in range(6):
        mem.store(torch.full((3, 4, 4), float(i)), torch.full((3, 8, 8), float(i)), {"i": i}, importance=float(i + 1))
    N = 4000
    counts = [0] * 6
    for _ in range(N):
        lr, _, metas = mem.sample(2, weighted=True)
        assert len(metas) == 2 and metas[0]["i"] != metas[1]["i"]
        for m in metas:
            counts[m["i"]] += 1
    assert lr[0, 0, 0, 0].item() == float(metas[0]["i"])
    assert_inclusion(counts, N, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert int(mem._access.sum()) == 2 * N


# ------------------------------------------------------------------------------------------------ 6. update_importance
def test_update_importance_formula_and_eviction():
    from nerve_cl.continual import DeviceEpisodicMemory
    mem = DeviceEpisodicMemory(capacity=5, strategy="importance", seed=0, device="cuda")
    for i in range(5):
        mem.store(torch.full((3, 4, 4), float(i)), torch.full((3, 8, 8), float(i)), {"i": i}, importance=1.0 + 0.125 * i)
    before = mem._importance.clone()
    idx = torch.tensor([3, 1, 4], dtype=torch.int32, device="cuda")
    vals = torch.tensor([0.3337, float("nan"), 2.718281], dtype=torch.float32, device="cuda")
    mem.update_importance(idx, vals, momentum=0.9)
    m = torch.tensor(0.9, dtype=torch.float32, device="cuda")
    one_minus = torch.tensor(1.0, dtype=torch.float32, device="cuda") - m
    want = before.clone()
    for j, s in ((0, 3), (2, 4)):
        want[s] = m * before[s] + one_minus * vals[j]           # two rounded products, one rounded sum, all fp32
    assert torch.equal(mem._importance, want)                   # slots 0, 2 untouched; slot 1 (NaN) unchanged
    assert mem._importance[1].item() == 1.125
    # momentum 0 overwrites; the lowered slot is the one the next accepted store evicts
    mem.update_importance(torch.tensor([2], dtype=torch.int32, device="cuda"), torch.tensor([0.0625], device="cuda"))
    assert mem._importance[2].item() == 0.0625
    assert mem.store(torch.full((3, 4, 4), 9.0), torch.full((3, 8, 8), 9.0), {"i": 9}, importance=0.5) is True
    assert [s.metadata["i"] for s in mem.buffer] == [0, 1, 9, 3, 4] and mem.buffer[2].importance == 0.5
    assert mem.buffer[2].frame_lr[0, 0, 0].item() == 9.0
    assert mem.store(torch.full((3, 4, 4), 8.0), torch.full((3, 8, 8), 8.0), {"i": 8}, importance=0.25) is False   # below the minimum
    # the host class makes the same decisions when told the same importances
    from nerve_cl.continual import EpisodicMemory
    host = EpisodicMemory(capacity=5, strategy="importance", seed=0)
    for i in range(5):
        host.store(torch.zeros(3, 4, 4), torch.zeros(3, 8, 8), {"i": i}, importance=1.0 + 0.125 * i)
    host.buffer[2].importance = 0.0625
    assert host.store(torch.zeros(3, 4, 4), torch.zeros(3, 8, 8), {"i": 9}, importance=0.5) is True
    assert [s.metadata["i"] for s in host.buffer] == [0, 1, 9, 3, 4]


def test_update_importance_takes_per_sample_losses_of_a_real_step():
    from nerve_cl import ops
    from nerve_cl.continual import DeviceEpisodicMemory
    from nerve_cl.models import SuperResolutionNet
    torch.manual_seed(0)
    net = SuperResolutionNet(3, 2, 16, 1, 1).cuda().train()
    g = torch.Generator().manual_seed(3)
    mem = DeviceEpisodicMemory(capacity=6, strategy="reservoir", seed=2, device="cuda")
    mem.store_batch(torch.rand(6, 3, 16, 16, generator=g).cuda(), torch.rand(6, 3, 32, 32, generator=g).cuda(), content_type="sports")
    cur_lr, cur_hr = torch.rand(2, 3, 16, 16, generator=g).cuda(), torch.rand(2, 3, 32, 32, generator=g).cuda()
    lr, hr, idx = mem.replay_batch(cur_lr, cur_hr, 3, weighted=True)
    out = net(lr.unsqueeze(1).expand(-1, 3, -1, -1, -1).contiguous())
    values = ops.l1_loss(out, hr, reduction="none")
    assert values.shape == (5,) and values.dtype == torch.float32
    values.mean().backward()
    before = mem._importance.clone()
    mem.update_importance(idx, values.detach()[2:], momentum=0.0)          # exactly what the loss returned, sliced
    slots = idx.tolist()
    assert len(set(slots)) == 3 and min(slots) >= 0
    for j, s in enumerate(slots):
        assert mem._importance[s].item() == values[2 + j].item() and torch.isfinite(values[2 + j])
    rest = [s for s in range(6) if s not in slots]
    assert torch.equal(mem._importance[rest], before[rest])
    assert all(p.grad is not None for p in net.parameters())


# ------------------------------------------------------------------------------------------------ 7. diversity
def _diversity_sequence():
    """(lr, hr) samples whose LR mean colours are placed by hand: 4 that fill the memory, then newcomers that sit 0.02-0.05
    (rejected) or 0.2-0.6 (accepted, replacing their nearest neighbour) from their nearest stored neighbour"""
    g = torch.Generator().manual_seed(17)
    centres = [(0.2, 0.2, 0.2), (0.8, 0.2, 0.2), (0.2, 0.8, 0.2), (0.2, 0.2, 0.8),          # fill
               (0.22, 0.21, 0.2), (0.45, 0.4, 0.55), (0.8, 0.24, 0.2), (0.2, 0.5, 0.8), (0.52, 0.5, 0.47), (0.9, 0.9, 0.9),
               (0.2, 0.83, 0.2), (0.2, 0.2, 0.35)]
    out = []
    for c in centres:
        noise = torch.rand(3, 8, 8, generator=g) * 0.1
        noise -= noise.mean(dim=(1, 2), keepdim=True)
        out.append((noise + torch.tensor(c).view(3, 1, 1), torch.rand(3, 16, 16, generator=g)))
    return out


def test_diversity_decisions_and_mean_table():
    from nerve_cl.continual import DeviceEpisodicMemory, EpisodicMemory
    seq = _diversity_sequence()
    # float64 replay of the decisions, asserting the margins first
    stored, decisions = [], []
    for lr, _ in seq:
        m = lr.double().mean(dim=(1, 2))
        if len(stored) < 4:
            stored.append(m)
            decisions.append(True)
            continue
        d = sorted((float(torch.norm(s - m)), i) for i, s in enumerate(stored))
        assert not 0.09 <= d[0][0] <= 0.11, d[0]                       # away from the 0.1 threshold
        assert d[1][0] - d[0][0] > 1e-3, d[:2]                          # the nearest neighbour is unique
        decisions.append(d[0][0] > 0.1)
        if decisions[-1]:
            stored[d[0][1]] = m
    assert decisions.count(False) >= 3 and decisions[4:].count(True) >= 3
    tables = []
    for _ in range(2):
        dev = DeviceEpisodicMemory(capacity=4, strategy="diversity", seed=0, device="cuda")
        host = EpisodicMemory(capacity=4, strategy="diversity", seed=0)
        got = [dev.store(lr.cuda(), hr.cuda(), {"i": i}) for i, (lr, hr) in enumerate(seq)]
        assert got == [host.store(lr, hr, {"i": i}) for i, (lr, hr) in enumerate(seq)] == decisions
        _assert_same_state(dev, host)
        tables.append(dev._means.clone())
        want = torch.stack([s.frame_lr.double().mean(dim=(1, 2)) for s in host.buffer])
        assert (dev._means.cpu().double() - want).abs().max().item() <= 1e-6
    assert torch.equal(tables[0], tables[1])                            # the same bits in two runs


# ------------------------------------------------------------------------------------------------ 8. no host sync
def test_replay_and_update_make_no_host_sync():
    from nerve_cl.continual import DeviceEpisodicMemory
    mem = DeviceEpisodicMemory(capacity=8, strategy="reservoir", seed=5, device="cuda")
    g = torch.Generator().manual_seed(1)
    mem.store_batch(torch.rand(8, 3, 8, 8, generator=g), torch.rand(8, 3, 16, 16, generator=g), content_type="news")
    cur_lr, cur_hr = torch.rand(4, 3, 8, 8, generator=g).cuda(), torch.rand(4, 3, 16, 16, generator=g).cuda()
    values = torch.rand(3, generator=g).cuda()
    mem.replay_batch(cur_lr, cur_hr, 3, weighted=True)                  # warm-up: code objects loaded, generator created
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        lr, hr, idx = mem.replay_batch(cur_lr, cur_hr, 3, content_type="news", weighted=True)
        mem.update_importance(idx, values, momentum=0.9)
        try:
            values.sum().item()
        except RuntimeError:
            control_raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if not control_raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this PyTorch build: the check would be vacuous")
    assert lr.shape == (7, 3, 8, 8) and hr.shape == (7, 3, 16, 16) and len(set(idx.tolist())) == 3


# ------------------------------------------------------------------------------------------------ 9. save / load
def test_files_load_in_either_class(tmp_path):
    dev, host = _mems("reservoir", 5, 7)
    g = torch.Generator().manual_seed(2)
    for i in range(9):
        lr, hr = torch.rand(3, 8, 8, generator=g), torch.rand(3, 16, 16, generator=g)
        meta = {"content_type": TYPES[i % 3], "i": i}
        assert dev.store(lr.cuda(), hr.cuda(), meta, 0.25 * (i + 1)) == host.store(lr, hr, meta, 0.25 * (i + 1))
    dev.save(str(tmp_path / "dev.pt"))
    host.save(str(tmp_path / "host.pt"))
    a, b = torch.load(tmp_path / "dev.pt", weights_only=True), torch.load(tmp_path / "host.pt", weights_only=True)
    assert a["total_seen"] == b["total_seen"] == 9 and a["strategy"] == b["strategy"] and a["capacity"] == b["capacity"]
    for x, y in zip(a["buffer"], b["buffer"]):
        assert not x[0].is_cuda and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3]
    from nerve_cl.continual import DeviceEpisodicMemory, EpisodicMemory
    dev2 = DeviceEpisodicMemory(capacity=5, strategy="reservoir", seed=1, device="cuda")
    dev2.load(str(tmp_path / "host.pt"))                              # host file -> device class
    host2 = EpisodicMemory(capacity=5, strategy="reservoir", seed=1)
    host2.load(str(tmp_path / "dev.pt"))                              # device file -> host class
    _assert_same_state(dev2, host2)
    _assert_same_state(dev2, host)
    assert [s.access_count for s in dev2.buffer] == [0] * 5
    lo = DeviceEpisodicMemory(capacity=5, strategy="reservoir", seed=1, device="cuda", storage="bf16")
    lo.load(str(tmp_path / "host.pt"))                                # rounds on load
    for s, h in zip(lo.buffer, host.buffer):
        assert torch.equal(s.frame_lr.cpu(), h.frame_lr.to(torch.bfloat16).float()) and s.importance == h.importance


# ------------------------------------------------------------------------------------------------ 10. the script
def _run(args, cwd):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(600)
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_train_continual_with_the_device_memory(tmp_path, storage):
    """--memory-size 40 as in tests/test_harness_gpu.py: 2 tasks x 24 samples fill a capacity of 40 (the default capacity of
    200 would print 48)"""
    out = _run([os.path.join(EXP, "train_continual.py"), "--strategy", "replay", "--device-memory", "--prioritized", "--tasks", "2",
                "--samples", "24", "--epochs", "2", "--features", "16", "--blocks", "1", "--memory-size", "40",
                "--memory-storage", storage], tmp_path)
    assert "=== Training on Task 1: animation ===" in out and "Memory size: 40" in out and "Training complete!" in out
    losses = [float(line.split("Loss=")[1].split()[0]) for line in out.splitlines() if "Loss=" in line]
    assert len(losses) == 4 and all(np.isfinite(v) for v in losses)
