"""GPU: the kernels of csrc/gem.hip (Gram, quadratic program, projection) against float64 numpy and the enumeration oracle of
tests/_gem_oracle.py, and GEM on the product path: the engine's gradient bucket in place, accumulated gradients, two bucketed
networks, HIP-graph steps, a device memory holding two content types, two data-parallel ranks.

Bounds.  Gram: every product is exact in double and n of them are summed in double: |got - want| <= n 2^-52 (|A| |A|')
entrywise, the bound tests/test_clustering_gpu.py uses for the same kind of sum.  Solve: the Cholesky forward-error bound
max|v - v_oracle| <= 8 T^2 cond(P) 2^-53 max|v_oracle|, cond(P) computed here in float64 from the same bits the device gets.
Projection: the sum is formed in double and rounded once to fp32, |g1 - want| <= 2^-24 |want|, asserted at a factor 2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _gem_oracle as O  # noqa: E402

EPS24, EPS52, EPS53 = 2.0 ** -24, 2.0 ** -52, 2.0 ** -53
# One block of the Gram kernel (n <= 1024) holds 4 waves, a wave takes 4 groups of 4 quads per trip: 256 floats per block and
# trip.  Wave 0 takes a second trip once there are more than 16 groups, i.e. more than 64 quads: n = 260.
N2 = 260 + 5
SIZES = [1, 3, 255, 257, 1025, N2]
TS = [1, 2, 15]


def _dev():
    return torch.device("cuda", 0)


def _ws():
    from nerve_cl import _engine
    return _engine.workspace(_dev())


def _gram_buf(fill=0.0):
    return torch.full((16, 16), fill, dtype=torch.float64, device=_dev())


def _place(a: np.ndarray, offset: int, stride=None) -> torch.Tensor:
    """a ([n] or [T][n] fp32) on the device; offset 1: a view that starts 4 bytes into its allocation; stride: the row stride"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dim() == 1:
        buf = torch.zeros(a.numel() + offset, device=_dev())
        v = buf[offset:]
        v.copy_(a)
    else:
        T, n = a.shape
        stride = n if stride is None else stride
        buf = torch.full((T * stride + offset,), 7.0, device=_dev())      # the gaps between rows hold 7: they must not be read
        v = buf[offset:].view(T, stride)[:, :n]
        v.copy_(a)
    if offset:
        assert v.data_ptr() % 16 == 4
    return v


def _inputs(kind, T, n, seed):
    return O._rows(kind, T, n, seed)


def _bits64(t):
    return t.detach().clone().view(torch.int64)


def _bits32(t):
    return t.detach().clone().contiguous().view(torch.int32)


def _gram(R, g, T, accumulate=False, gram=None):
    from nerve_cl import _nvq
    gram = _gram_buf(3.0) if gram is None else gram           # stale contents must be overwritten
    _nvq.gem_gram(R, T, g, gram, _ws(), accumulate=accumulate)
    return gram


def _check_gram(got: torch.Tensor, R: np.ndarray, g: np.ndarray, n: int):
    T = R.shape[0]
    A = np.concatenate([R.astype(np.float64), g.astype(np.float64)[None]])
    want = np.zeros((16, 16))
    want[:T + 1, :T + 1] = A @ A.T
    bound = np.zeros((16, 16))
    bound[:T + 1, :T + 1] = n * EPS52 * (np.abs(A) @ np.abs(A).T)
    err = np.abs(got.cpu().numpy() - want)
    assert (err <= bound).all(), (err - bound).max()
    assert torch.equal(_bits64(got), _bits64(got.t().contiguous()))       # symmetric bit for bit
    outside = got.clone()
    outside[:T + 1, :T + 1] = 0
    assert not outside.any()


# ------------------------------------------------------------------------------------------------- Gram

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", SIZES)
def test_gram_against_float64(n, T):
    R, g = _inputs("random", T, n, 10 + T)
    dR, dg = _place(R, 0), _place(g, 0)
    got = _gram(dR, dg, T)
    _check_gram(got, R, g, n)
    again = _gram(dR, dg, T)
    assert torch.equal(_bits64(got), _bits64(again))                     # no atomics, a fixed grid: the same bits


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", [3, 257, 1025, N2])
def test_gram_does_not_depend_on_alignment_or_stride(n, T):
    R, g = _inputs("random", T, n, 20 + T)
    aligned = _gram(_place(R, 0), _place(g, 0), T)
    _check_gram(aligned, R, g, n)
    shifted = _gram(_place(R, 1, stride=(n + 3) // 4 * 4 + 8), _place(g, 1), T)    # rows 4 bytes off, stride > n
    assert torch.equal(_bits64(aligned), _bits64(shifted))
    odd = _gram(_place(R, 0, stride=n + 5), _place(g, 0), T)                      # a stride that is no multiple of 4
    assert torch.equal(_bits64(aligned), _bits64(odd))


@pytest.mark.parametrize("T", [2, 15])
def test_two_chained_segments_equal_their_concatenation(T):
    n1, n2 = 1025, N2
    R, g = _inputs("random", T, n1 + n2, 30 + T)
    gram = _gram(_place(R[:, :n1], 0), _place(g[:n1], 0), T)
    _gram(_place(R[:, n1:], 1, stride=n2 + 7), _place(g[n1:], 1), T, accumulate=True, gram=gram)
    _check_gram(gram, R, g, n1 + n2)


def test_gram_uses_only_the_first_T_rows_of_a_larger_matrix():
    R, g = _inputs("random", 15, 257, 33)
    dR = _place(R, 0)
    dR[2:] = float("nan")                                                 # rows past T are not read
    got = _gram(dR, _place(g, 0), 2)
    _check_gram(got, R[:2], g, 257)


# ------------------------------------------------------------------------------------------------- solve

def _solve(G: np.ndarray, T, margin, eps=1e-3, eps_relative=False, stats=None):
    from nerve_cl import _nvq
    gram = torch.from_numpy(G).to(_dev())                                 # a host-made upload: the oracle sees the same bits
    v = torch.full((16,), 9.0, dtype=torch.float64, device=_dev())
    stats = torch.zeros(8, dtype=torch.float64, device=_dev()) if stats is None else stats
    _nvq.gem_solve(gram, T, margin, eps, eps_relative, v, stats)
    return v.cpu().numpy(), stats.cpu().numpy()


def _check_solve(G, T, margin, eps_relative=False):
    ridge = O.ridge_of(G[:T, :T], O.EPS_F32, eps_relative)
    P, q = G[:T, :T] + ridge * np.eye(T), G[:T, T]
    v, st = _solve(G, T, margin, eps_relative=eps_relative)
    if not (q < 0).any():
        assert not v.any() and st[4] == 0 and st[3] == 0 and st[0] == 0
        return v
    want, free = O.certified(P, q, margin)
    err, bound = np.abs(v[:T] - want).max(), 8 * T * T * np.linalg.cond(P) * EPS53 * np.abs(want).max()
    print(f"T={T} margin={margin} cond={np.linalg.cond(P):.1f} active={len(free)} iterations={st[2]:.0f} err={err:.3e} bound={bound:.3e}")
    assert st[3] == 0 and st[0] == (q < 0).sum() and st[1] == len(free) and st[4] == 1
    assert 4 * st[2] <= 64                                                # the cap is at least 4 x what the cases need
    assert err <= bound and not v[T:].any()
    ex = O.expected_stats(G, T, margin, want)
    for slot in (5, 6, 7):
        assert abs(st[slot] - ex[slot]) <= 1e-12 * abs(ex[slot]), (slot, st[slot], ex[slot])
    return v


@pytest.mark.parametrize("margin", O.MARGINS)
@pytest.mark.parametrize("name", list(O.CASES))
def test_solve_on_the_six_cases(name, margin):
    R, g = O.case(name)
    _check_solve(O.gram_of(R, g), R.shape[0], margin)


@pytest.mark.parametrize("T", [1, 3, 6, 15])
def test_solve_on_problems_that_bind_freed_multipliers(T):
    for seed in O.RANDOM_SEEDS[T]:
        for margin in O.MARGINS:
            _check_solve(O.random_problem(T, seed), T, margin)


def test_solve_with_a_relative_ridge():
    R, g = O.case("conflict_T6")
    G = O.gram_of(R * np.float32(1e-3), g * np.float32(1e-3))             # small gradients: eps = 1e-3 would dominate P
    v_rel = _check_solve(G, 6, 0.0, eps_relative=True)
    v_abs = _check_solve(G, 6, 0.0, eps_relative=False)
    assert np.abs(v_rel - v_abs).max() > 0.1 * np.abs(v_rel).max()


def test_solve_refuses_non_finite_input_and_counts_only_projections():
    R, g = O.case("conflict_T6")
    G = O.gram_of(R, g)
    stats = torch.zeros(8, dtype=torch.float64, device=_dev())
    _solve(G, 6, 0.5, stats=stats)
    assert stats[4] == 1
    for bad in (float("nan"), float("inf")):
        H = G.copy()
        H[2, 4] = H[4, 2] = bad
        v, st = _solve(H, 6, 0.5, stats=stats)
        assert not v.any() and st[3] == 2 and st[4] == 1
    H = G.copy()
    H[9, 9] = float("nan")                                                # outside (T + 1)^2: not used
    v, st = _solve(H, 6, 0.5, stats=stats)
    assert v.any() and st[3] == 0 and st[4] == 2
    R, g = O.case("agree_T8")
    v, st = _solve(O.gram_of(R, g), 8, 0.5, stats=stats)
    assert not v.any() and st[3] == 0 and st[0] == 0 and st[4] == 2       # no q_t < 0: the counter stays
    v, st = _solve(G, 0, 0.5, stats=stats)
    assert not v.any() and st[3] == 0 and st[4] == 2 and st[5] == G[0, 0]


# ------------------------------------------------------------------------------------------------- project

def _check_projection(g0: np.ndarray, R: np.ndarray, v: np.ndarray, g1: torch.Tensor, slack=None):
    T = R.shape[0]
    want = g0.astype(np.float64) + v[:T] @ R.astype(np.float64)
    err = np.abs(g1.cpu().numpy().astype(np.float64) - want)
    bound = 2 * EPS24 * np.abs(want) + (0.0 if slack is None else slack)
    assert (err <= bound).all(), (err - bound).max()
    return want


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", SIZES)
def test_chain_gram_solve_project(n, T):
    """the three kernels in a row at margin 0, the device's own v read back; afterwards no reference is opposed"""
    from nerve_cl import _nvq
    R, g = _inputs("conflict", T, n, 40 + T)
    dR, dg = _place(R, 0), _place(g, 0)
    gram = _gram(dR, dg, T)
    v = torch.zeros(16, dtype=torch.float64, device=_dev())
    stats = torch.zeros(8, dtype=torch.float64, device=_dev())
    _nvq.gem_solve(gram, T, 0.0, 1e-3, False, v, stats)
    assert stats[3] == 0 and stats[0] >= 1 and stats[4] == 1
    _nvq.gem_project(dg, dR, T, v)
    vh = v.cpu().numpy()
    _check_projection(g, R, vh, dg)
    g1, Rd = dg.cpu().numpy().astype(np.float64), R.astype(np.float64)
    for t in range(T):
        floor = -O.EPS_F32 * vh[t] - EPS24 * np.linalg.norm(Rd[t]) * np.linalg.norm(g1) - n * EPS52 * (np.abs(Rd[t]) @ np.abs(g1))
        assert Rd[t] @ g1 >= floor, (t, Rd[t] @ g1, floor)
    gg_after = stats[6].item()
    assert abs(gg_after - g1 @ g1) <= 8 * EPS24 * (g1 @ g1) + 1e-13 * stats[5].item()               # the Gram's forecast of |g'|^2 (g' itself is rounded)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", [3, 257, 1025, N2])
def test_projection_does_not_depend_on_alignment(n, T):
    from nerve_cl import _nvq
    R, g = _inputs("random", T, n, 50 + T)
    v = torch.zeros(16, dtype=torch.float64, device=_dev())
    v[:T] = torch.linspace(0.5, 1.75, T, dtype=torch.float64)
    a = _place(g, 0)
    _nvq.gem_project(a, _place(R, 0), T, v)
    _check_projection(g, R, v.cpu().numpy(), a)
    b = _place(g, 1)
    _nvq.gem_project(b, _place(R, 1, stride=(n + 3) // 4 * 4 + 4), T, v)
    assert torch.equal(_bits32(a), _bits32(b))
    c = _place(g, 0)
    _nvq.gem_project(c, _place(R, 0, stride=n + 3), T, v)
    assert torch.equal(_bits32(a), _bits32(c))


@pytest.mark.parametrize("n", [3, 1025, N2])
def test_projection_with_zero_multipliers(n):
    from nerve_cl import _nvq
    R, g = _inputs("random", 15, n, 60)
    dg = _place(g, 0)
    before = _bits32(dg)
    dR = _place(R, 0)
    dR[:] = float("nan")                                                  # v == 0: no row is read, g is not written
    v = torch.zeros(16, dtype=torch.float64, device=_dev())
    _nvq.gem_project(dg, dR, 15, v)
    assert torch.equal(_bits32(dg), before)
    dR.copy_(torch.from_numpy(R))
    dR[1] = float("nan")                                                  # rows with v_t == 0 may hold anything
    dR[14] = float("nan")
    v[0], v[7] = 0.75, -0.25
    _nvq.gem_project(dg, dR, 15, v)
    want = _check_projection(g, np.where(np.isnan(dR.cpu().numpy()), 0, R), v.cpu().numpy(), dg)
    assert np.isfinite(want).all() and (dg.cpu().numpy() != g).any()


# ------------------------------------------------------------------------------------------------- the product path

CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B, H, W = 2, 16, 24


def _engine(**extra):
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG, **extra))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    return eng.to(_dev()).train()


def _data():
    from oracle import synth
    x, y = synth.formula_clip(B, 3, H, W), synth.formula_target(B, 2 * H, 2 * W)
    return x.to(_dev()), y.to(_dev())


def _flat_grads(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])


def _aliases_bucket(net) -> bool:
    lay, _ = net._bucket_layout()
    base = net._last_grad_bucket.data_ptr()
    return all(p.grad is not None and p.grad.data_ptr() == base + 4 * lay[n][0] for n, p in net.named_parameters())


def _task_loss(eng, x, y, kind):
    out = eng(x)["enhanced"]
    L = F.mse_loss(out, y)
    if kind == "+L":
        return L
    if kind == "-L":
        return -L
    return -L + 0.5 * F.mse_loss(out, y.flip(0) * 0.5)                    # "-L+0.5L2"


def _three_references(eng, gem, x, y):
    for kind in ("+L", "-L", "-L+0.5L2"):
        eng.zero_grad()
        _task_loss(eng, x, y, kind).backward()
        gem.capture_reference(kind)
    eng.zero_grad()


def _expect_from_device_gram(gem, T, g0: torch.Tensor, refs: torch.Tensor, g1: torch.Tensor, margin=0.5, eps_relative=False):
    """the oracle's projection from the device's own Gram matrix; -> v of the oracle"""
    G = gem.gram.cpu().numpy()
    ridge = O.ridge_of(G[:T, :T], O.EPS_F32, eps_relative)
    P, q = G[:T, :T] + ridge * np.eye(T), G[:T, T]
    assert (q < 0).any()
    want_v, free = O.certified(P, q, margin)
    v = gem.multipliers.cpu().numpy()
    dv = 8 * T * T * np.linalg.cond(P) * EPS53 * np.abs(want_v).max()
    assert np.abs(v[:T] - want_v).max() <= dv and gem.status() == 0
    Rn = refs.cpu().numpy()
    v16 = np.zeros(16)
    v16[:T] = want_v
    _check_projection(g0.cpu().numpy(), Rn, v16, g1, slack=dv * np.abs(Rn.astype(np.float64)).sum(0))
    return want_v


def _ref_rows(gem, T):
    """the references restricted to the parameters' own floats, in _flat_grads order"""
    cols = []
    for sg, ref in zip(gem._segs, gem._ref):
        if sg.net is not None:
            cols += [ref[:T, o:o + k] for o, k in sg.net._bucket_layout()[0].values()]
        else:                                                             # loose parameters count only when they carry a gradient
            views = sg.views(ref[0])
            cols += [ref[:T, views[n].storage_offset() - ref.storage_offset():][:, :p.numel()] for n, p in sg.named if p.grad is not None]
    return torch.cat(cols, dim=1)


@pytest.mark.parametrize("eps_relative", [False, True], ids=["eps_absolute", "eps_relative"])
def test_gem_projects_the_engines_bucket_in_place_and_the_step_uses_it(eps_relative):
    from nerve_cl.continual import GEM
    eng = _engine()
    x, y = _data()
    gem = GEM(eng, eps_relative=eps_relative)
    opt = torch.optim.SGD(eng.parameters(), lr=0.1)
    _three_references(eng, gem, x, y)
    assert gem.tasks == ["+L", "-L", "-L+0.5L2"]
    _task_loss(eng, x, y, "+L").backward()
    assert _aliases_bucket(eng.super_resolution)
    g0 = _flat_grads(eng).clone()
    gem.project()
    assert _aliases_bucket(eng.super_resolution)                          # still the bucket's views: projected in place
    g1 = _flat_grads(eng)
    _expect_from_device_gram(gem, 3, g0, _ref_rows(gem, 3), g1, eps_relative=eps_relative)
    assert gem.num_projections() == 1 and gem.stats[0] == 2
    cos = gem.min_cosine()
    assert cos.is_cuda and cos.dim() == 0 and -1.0 - 1e-9 <= cos.item() < 0
    before = torch.cat([p.detach().reshape(-1) for p in eng.super_resolution.parameters()]).clone()
    opt.step()
    after = torch.cat([p.detach().reshape(-1) for p in eng.super_resolution.parameters()])
    want = before.double() - 0.1 * g1.double()
    assert bool(((after.double() - want).abs() <= 4 * EPS24 * (before.double().abs() + 0.1 * g1.double().abs())).all())
    assert (after != before).any()


def test_gem_leaves_an_agreeing_gradient_bit_identical():
    from nerve_cl.continual import GEM
    eng = _engine()
    x, y = _data()
    gem = GEM(eng)
    for name in ("a", "b"):
        eng.zero_grad()
        _task_loss(eng, x, y, "+L").backward()
        gem.capture_reference(name)
    eng.zero_grad()
    _task_loss(eng, x, y, "+L").backward()
    g0 = _flat_grads(eng).clone()
    gem.project()
    assert torch.equal(_bits32(_flat_grads(eng)), _bits32(g0))
    assert gem.num_projections() == 0 and gem.status() == 0 and not gem.multipliers.any() and gem.stats[0] == 0
    assert abs(gem.min_cosine().item() - 1.0) <= 1e-9


def test_gem_on_accumulated_gradients_takes_the_gathered_path():
    from nerve_cl.continual import GEM
    eng = _engine()
    x, y = _data()
    gem = GEM(eng)
    _three_references(eng, gem, x, y)
    for _ in range(2):
        _task_loss(eng, x, y, "+L").backward()
    assert not _aliases_bucket(eng.super_resolution)
    g0 = _flat_grads(eng).clone()
    gem.project()
    _expect_from_device_gram(gem, 3, g0, _ref_rows(gem, 3), _flat_grads(eng))
    assert gem.num_projections() == 1


def test_gem_forms_one_gram_over_two_bucketed_networks():
    from nerve_cl.continual import GEM
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=True, recovery_base_channels=16, recovery_temporal_window=1,
                                              **CFG))
    eng.frame_recovery.load_state_dict(synth.formula_state_fr(3, 16, gain=synth.GOLDEN_GAIN))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    eng = eng.to(_dev()).train()
    x = synth.formula_clip(B, 3, 32, 32).to(_dev())
    y = synth.formula_target(B, 64, 64).to(_dev())
    mask = torch.zeros(B, 1, 32, 32, device=_dev())
    mask[:, :, 8:24, 4:20] = 1.0

    def loss(sign, other):
        res = eng(x, corruption_mask=mask)
        return (sign * F.mse_loss(res["enhanced"], y) + 0.3 * sign * F.mse_loss(res["recovered"], x[:, 1] * 0.5)
                + other * F.mse_loss(res["enhanced"], y.flip(0) * 0.5))

    gem = GEM(eng)
    nets = [sg.net for sg in gem._segs if sg.net is not None]
    assert len(nets) == 2
    for name, (sign, other) in {"a": (-1.0, 0.0), "b": (-1.0, 0.5)}.items():
        eng.zero_grad()
        loss(sign, other).backward()
        gem.capture_reference(name)
    eng.zero_grad()
    loss(1.0, 0.0).backward()
    assert all(_aliases_bucket(n) for n in nets)
    g0 = torch.cat([n._last_grad_bucket.clone() for n in nets])
    refs = torch.cat([ref[:2] for sg, ref in zip(gem._segs, gem._ref) if sg.net is not None], dim=1)
    assert all(ref[:2].abs().max() > 0 for ref in gem._ref[:2])
    gem.project()
    _check_gram(gem.gram, refs.cpu().numpy(), g0.cpu().numpy(), g0.numel())         # one Gram from the sums over both networks
    _expect_from_device_gram(gem, 2, g0, refs, torch.cat([n._last_grad_bucket for n in nets]))


class _Enhanced(torch.nn.Module):
    """clip -> the engine -> 'enhanced': the module GEM's own reference passes call"""

    def __init__(self, eng):
        super().__init__()
        self.engine = eng

    def forward(self, clip):
        return self.engine(clip)["enhanced"]


def _minus_mse(out, tgt):
    return -F.mse_loss(out, tgt)


def test_gem_with_hip_graph_steps():
    from nerve_cl.continual import GEM
    eng = _engine()
    eng.super_resolution.use_hip_graphs = True
    x, y = _data()
    for _ in range(3):                                                  # two eager warm-up calls, capture on the third
        eng.zero_grad()
        F.mse_loss(eng(x)["enhanced"], y).backward()
    gem = GEM(_Enhanced(eng))
    for name in ("a", "b", "c"):
        gem.add_task(name)
    replays = eng.super_resolution._step_graphs.replays
    assert gem.compute_references(_minus_mse, batches={"a": (x, y), "b": (x, y * 0.5), "c": (x, y.flip(0))}) == 3
    assert eng.super_resolution._step_graphs.replays >= replays + 3      # the reference passes share the step's graph entry
    eng.zero_grad()
    F.mse_loss(eng(x)["enhanced"], y).backward()
    assert _aliases_bucket(eng.super_resolution)
    g0 = _flat_grads(eng).clone()
    gem.project()
    _expect_from_device_gram(gem, 3, g0, _ref_rows(gem, 3), _flat_grads(eng))


class _Clip(torch.nn.Module):
    """(B,C,H,W) frames -> the engine on the repeated-frame clip -> 'enhanced'"""

    def __init__(self, eng):
        super().__init__()
        self.engine = eng

    def forward(self, x):
        return self.engine(x.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]


def test_compute_references_draws_per_content_type_from_a_device_memory():
    from nerve_cl import ops
    from nerve_cl.continual import GEM, DeviceEpisodicMemory
    eng = _engine()
    model = _Clip(eng)
    mem = DeviceEpisodicMemory(capacity=8, strategy="stratified", device=_dev(), seed=0)
    gem = GEM(model, mem, ref_batch_size=2)
    for name in ("movie", "sports", "news"):
        gem.add_task(name)
    assert gem.compute_references(ops.MSELoss()) == 0                     # an empty memory
    x, y = _data()
    mem.store_batch(x[:, 0], y, content_type="movie")
    mem.store_batch(x[:, 1], y * 0.5, content_type="news")
    assert len(mem) == 4
    assert gem.compute_references(ops.MSELoss()) == 2                     # nothing of 'sports' is stored: its row stays
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    ref = gem._ref[0]
    assert ref[0].abs().max() > 0 and not ref[1].any() and ref[2].abs().max() > 0 and not torch.equal(ref[0], ref[2])
    eng.zero_grad()                                                       # row 0 is the gradient on the two 'movie' samples
    ops.MSELoss()(model(x[:, 0]), y).backward()
    want = eng.super_resolution._last_grad_bucket
    assert (ref[0] - want).abs().max() <= 1e-5 * want.abs().max()


# ------------------------------------------------------------------------------------------------- data parallel

def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_two_ranks_project_to_the_same_gradient(tmp_path):
    out = tmp_path / "gem.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    # children are ordinary child processes of a launcher that never touches the GPU
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(HERE, "gem_worker.py"), str(out)], env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out, weights_only=True)
    assert torch.equal(got["bucket_rank0"].view(torch.int32), got["bucket_rank1"].view(torch.int32))
    assert torch.equal(got["v_rank0"], got["v_rank1"]) and got["v_rank0"][:2].min() >= 0.5
    assert got["projections"] == [1, 1] and got["status"] == [0, 0]
    assert not torch.equal(got["bucket_rank0"], got["unprojected_rank0"])
