"""CPU: GEM on a plain module (its float64 composition against the enumeration oracle of tests/_gem_oracle.py), the task table,
the memory draw per content type, the package's host solver against the oracle, the declarations and the script's flags.  No
kernel runs here."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import nerve_cl.continual
from nerve_cl import _nvq
from nerve_cl.continual import GEM, EpisodicMemory
from nerve_cl.continual import gem as gem_mod

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _gem_oracle as O  # noqa: E402


def _net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3)).double()


def _numel(net):
    return sum(p.numel() for p in net.parameters())


def _set_grads(net, flat):
    off = 0
    for p in net.parameters():
        p.grad = flat[off:off + p.numel()].view(p.shape).clone()
        off += p.numel()


def _grads(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def _three_tasks(net, kind, **kw):
    """GEM with the references of tasks 'a', 'b', 'c' and the gradient g in place -> (gem, R [3][n], g)"""
    n = _numel(net)
    gen = torch.Generator().manual_seed(11)
    g = torch.randn(n, dtype=torch.float64, generator=gen)
    noise = torch.randn(3, n, dtype=torch.float64, generator=gen)
    if kind == "agree":
        R = g + 0.3 * noise
    elif kind == "one":                                   # only 'b' conflicts
        R = torch.stack([g + 0.3 * noise[0], -g + 0.3 * noise[1], 0.5 * g + noise[2]])
    else:                                                 # all three conflict, with different strength
        R = torch.stack([-g + 0.5 * noise[0], -0.5 * g + 0.8 * noise[1], -2.0 * g + 0.3 * noise[2]])
    gem = GEM(net, **kw)
    for name, r in zip("abc", R):
        _set_grads(net, r)
        gem.capture_reference(name)
    _set_grads(net, g)
    return gem, R, g


def _oracle(R, g, margin, eps=O.EPS_F32, eps_relative=False):
    RR, q = (R @ R.t()).numpy(), (R @ g).numpy()
    ridge = O.ridge_of(RR, eps, eps_relative)
    v, free = O.certified(RR + ridge * np.eye(len(q)), q, margin)
    return v, free, ridge


def test_gem_is_exported_next_to_agem():
    assert "GEM" in nerve_cl.continual.__all__ and nerve_cl.continual.GEM is GEM
    assert "AGEM" in nerve_cl.continual.__all__


def test_an_agreeing_gradient_stays_bit_identical():
    net = _net()
    gem, R, g = _three_tasks(net, "agree")
    assert bool(((R @ g) > 0).all())
    gem.project()
    assert torch.equal(_grads(net), g)
    assert gem.num_projections() == 0 and gem.status() == 0 and not gem.multipliers.any()
    assert gem.stats[gem_mod.VIOLATED] == 0 and gem.stats[gem_mod.GG_AFTER] == gem.stats[gem_mod.GG_BEFORE]
    want = ((R @ g) / (R.norm(dim=1) * g.norm())).min()
    assert gem.min_cosine().dim() == 0 and abs(float(gem.min_cosine()) - float(want)) <= 1e-12


def test_nothing_happens_before_a_reference_exists():
    net = _net()
    gem = GEM(net)
    g = torch.randn(_numel(net), dtype=torch.float64)
    _set_grads(net, g)
    gem.project()
    gem.add_task("a")                                     # registered, never filled
    gem.project()
    assert torch.equal(_grads(net), g) and gem.num_projections() == 0


@pytest.mark.parametrize("kind,margin,violated", [("one", 0.5, 1), ("one", 0.0, 1), ("several", 0.5, 3), ("several", 0.0, 3)])
def test_projection_equals_the_oracles(kind, margin, violated):
    net = _net()
    gem, R, g = _three_tasks(net, kind, margin=margin)
    v, free, _ = _oracle(R, g, margin)
    assert int(((R @ g) < 0).sum()) == violated
    gem.project()
    got_v = gem.multipliers.numpy()
    assert np.abs(got_v[:3] - v).max() <= 1e-12 * np.abs(v).max() and not got_v[3:].any()
    want = g + torch.from_numpy(v) @ R
    assert (_grads(net) - want).abs().max() <= 1e-12 * want.abs().max()
    st = gem.stats
    assert st.dtype == torch.float64 and st.shape == (8,)
    assert st[gem_mod.VIOLATED] == violated and st[gem_mod.ACTIVE] == len(free) and st[gem_mod.STATUS] == 0
    assert 4 * st[gem_mod.ITERATIONS] <= gem_mod.MAX_ITER
    assert gem.num_projections() == 1
    assert abs(float(st[gem_mod.GG_BEFORE]) - float(g @ g)) <= 1e-12 * float(g @ g)
    assert abs(float(st[gem_mod.GG_AFTER]) - float(want @ want)) <= 1e-12 * float(want @ want)
    if margin == 0.0 and kind == "several":
        assert len(free) >= 2                             # several active constraints


@pytest.mark.parametrize("kind", ["one", "several"])
def test_at_margin_zero_no_task_is_opposed_after_the_projection(kind):
    net = _net()
    gem, R, g = _three_tasks(net, kind, margin=0.0)
    gem.project()
    g1, v = _grads(net), gem.multipliers[:3]
    ridge = O.EPS_F32
    for t in range(3):
        assert float(R[t] @ g1) >= -ridge * float(v[t]) - 1e-12 * float(R[t].norm() * g1.norm()), t


def test_eps_relative_scales_the_ridge_by_the_largest_reference():
    net = _net()
    gem, R, g = _three_tasks(net, "several", margin=0.0, eps=0.05, eps_relative=True)
    eps = float(np.float32(0.05))
    v_rel, _, ridge = _oracle(R, g, 0.0, eps, True)
    assert abs(ridge - eps * float((R * R).sum(1).max())) <= 1e-15 * ridge
    v_abs, _, _ = _oracle(R, g, 0.0, eps, False)
    assert np.abs(v_rel - v_abs).max() > 1e-3 * np.abs(v_abs).max()          # the two ridges give different answers here
    gem.project()
    assert np.abs(gem.multipliers.numpy()[:3] - v_rel).max() <= 1e-12 * np.abs(v_rel).max()


def test_a_nan_reference_means_no_projection_and_status_2():
    net = _net()
    gem, R, g = _three_tasks(net, "several")
    bad = R[1].clone()
    bad[5] = float("nan")
    _set_grads(net, bad)
    gem.capture_reference("b")
    _set_grads(net, g)
    gem.project()
    assert torch.equal(_grads(net), g)
    assert gem.status() == 2 and not gem.multipliers.any() and gem.num_projections() == 0


def test_task_table_limit_overwrite_and_forget():
    net = _net()
    n = _numel(net)
    gem = GEM(net)
    for t in range(15):
        _set_grads(net, torch.full((n,), float(t + 1), dtype=torch.float64))
        gem.capture_reference(("task", t))
    assert gem.tasks == [("task", t) for t in range(15)]
    with pytest.raises(ValueError):
        gem.capture_reference("the sixteenth")
    with pytest.raises(ValueError):
        gem.add_task("the sixteenth")
    _set_grads(net, torch.full((n,), -7.0, dtype=torch.float64))
    gem.capture_reference(("task", 3))                    # a known id overwrites its own row
    assert len(gem.tasks) == 15 and bool((gem._ref[0][3] == -7.0).all())
    gem.forget(("task", 1))
    assert gem.tasks == [("task", t) for t in range(15) if t != 1]
    want = [1.0, 3.0, -7.0] + [float(t + 1) for t in range(4, 15)] + [0.0]
    assert gem._ref[0][:, 0].tolist() == want and gem._ref[0][:, -1].tolist() == want
    gem.capture_reference("the sixteenth")                # a row is free again
    assert gem.tasks[-1] == "the sixteenth"
    with pytest.raises(ValueError):
        GEM(net, max_tasks=16)


def test_compute_references_draws_per_content_type_and_skips_absent_tasks():
    net = _net().float()
    mem = EpisodicMemory(capacity=16)
    torch.manual_seed(8)
    for k in range(8):
        mem.store(torch.randn(5), torch.randn(3), {"content_type": "sports" if k % 2 else "news"})
    gem = GEM(net, mem, ref_batch_size=3)
    assert gem.compute_references(nn.MSELoss()) == 0      # no task known yet
    for name in ("sports", "animation", "news"):
        gem.add_task(name)
    assert gem.compute_references(nn.MSELoss()) == 2      # nothing of 'animation' is stored: skipped
    assert all(p.grad is None or not p.grad.any() for p in net.parameters())
    ref = gem._ref[0]
    assert ref[0].abs().max() > 0 and not ref[1].any() and ref[2].abs().max() > 0
    assert not torch.equal(ref[0], ref[2])
    x, y = torch.randn(4, 5), torch.randn(4, 3)
    assert gem.compute_references(nn.MSELoss(), batches={"animation": (x, y)}) == 1
    net.zero_grad()
    nn.functional.mse_loss(net(x), y).backward()
    assert torch.equal(gem._ref[0][1].float(), _grads(net))
    assert GEM(net).compute_references(nn.MSELoss()) == 0  # no memory at all


@pytest.mark.parametrize("T", [1, 3, 6, 15])
def test_the_host_solver_against_the_oracle(T):
    worst_iter, shrank = 0, False
    for seed in O.RANDOM_SEEDS[T]:
        G = O.random_problem(T, seed)
        for margin in O.MARGINS:
            P, q = G[:T, :T] + O.EPS_F32 * np.eye(T), G[:T, T]
            v, free = O.certified(P, q, margin)
            got, st = gem_mod.solve_multipliers(G, T, margin, 1e-3)
            bound = 8 * T * T * np.linalg.cond(P) * 2.0 ** -53 * np.abs(v).max()
            assert np.abs(got[:T] - v).max() <= bound, (seed, margin)
            assert st[gem_mod.STATUS] == 0 and st[gem_mod.ACTIVE] == len(free) and st[gem_mod.VIOLATED] == (q < 0).sum()
            worst_iter = max(worst_iter, int(st[gem_mod.ITERATIONS]))
            shrank |= st[gem_mod.ITERATIONS] > len(free)
    assert 4 * worst_iter <= gem_mod.MAX_ITER
    if T >= 3:
        assert shrank                                     # some problem made the method bind a multiplier it had freed


@pytest.mark.parametrize("name", list(O.CASES))
def test_the_host_solver_on_the_shared_cases(name):
    R, g = O.case(name)
    T = R.shape[0]
    G = O.gram_of(R, g)
    for margin in O.MARGINS:
        P, q = G[:T, :T] + O.EPS_F32 * np.eye(T), G[:T, T]
        got, st = gem_mod.solve_multipliers(G, T, margin, 1e-3)
        if not (q < 0).any():
            assert not got.any() and st[gem_mod.PROJECTIONS] == 0
            continue
        v, free = O.certified(P, q, margin)
        assert np.abs(got[:T] - v).max() <= 8 * T * T * np.linalg.cond(P) * 2.0 ** -53 * np.abs(v).max()
        assert st[gem_mod.ACTIVE] == len(free) and 4 * st[gem_mod.ITERATIONS] <= gem_mod.MAX_ITER


def test_the_new_symbols_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "nvq.h")).read()
    for name in ("nvq_gem_gram", "nvq_gem_solve", "nvq_gem_project"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _nvq.SIGNATURES
    assert not re.search(r"nvq_gem_\w+\([^)]*\bdouble\s+\w", text)          # no double by value through the ABI
    assert _nvq.GEM_MAX_TASKS == 15 and gem_mod.MAX_TASKS == 15


def test_the_script_accepts_the_gem_strategy():
    sys.path.insert(0, os.path.join(REPO, "experiments"))               # (the scripts import their sibling _common.py)
    spec = importlib.util.spec_from_file_location("train_continual_script_gem", os.path.join(REPO, "experiments", "train_continual.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    d = parser.parse_args([])
    assert d.gem_ref_batch == 8 and d.gem_margin == 0.5 and d.gem_eps == 1e-3 and d.gem_eps_relative is False and d.gem_refresh == 1
    a = parser.parse_args(["--strategy", "gem", "--gem-ref-batch", "4", "--gem-margin", "0", "--gem-eps", "0.01", "--gem-eps-relative",
                           "--gem-refresh", "5", "--clip-grad-norm", "1.0"])
    assert a.strategy == "gem" and a.gem_ref_batch == 4 and a.gem_margin == 0.0 and a.gem_eps == 0.01 and a.gem_eps_relative
    assert a.gem_refresh == 5 and callable(mod.train_with_gem)
