"""CPU: AGEM on a plain module (its float64 torch composition against the formula restated here), the empty-memory and
no-reference cases, ops.clip_grad_norm_ on CPU parameters, the script's flags and the package export.  No kernel runs here."""
import importlib.util
import os
import sys

import pytest
import torch
import torch.nn as nn

import nerve_cl.continual
from nerve_cl import ops
from nerve_cl.continual import AGEM, EpisodicMemory

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3)).double()


def _set_grads(net, flat):
    off = 0
    for p in net.parameters():
        p.grad = flat[off:off + p.numel()].view(p.shape).clone()
        off += p.numel()


def _grads(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def _numel(net):
    return sum(p.numel() for p in net.parameters())


def test_agem_is_exported():
    assert "AGEM" in nerve_cl.continual.__all__ and nerve_cl.continual.AGEM is AGEM


def test_conflicting_gradient_is_projected_as_the_float64_formula_says():
    net = _net()
    torch.manual_seed(4)
    g = torch.randn(_numel(net), dtype=torch.float64)
    r = -g + 0.3 * torch.randn_like(g)
    agem = AGEM(net)
    _set_grads(net, r)
    agem.capture_reference()
    _set_grads(net, g)
    agem.project()
    gr, rr = (g * r).sum(), (r * r).sum()
    assert gr < 0
    want = g - gr / rr * r
    got = _grads(net)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    assert abs(float(got @ r)) <= 1e-12 * float(g.norm() * r.norm())
    st = agem.stats
    assert st.dtype == torch.float64 and st.shape == (5,)
    for have, ref in zip(st[:4].tolist(), (gr, rr, (g * g).sum(), gr / rr)):
        assert abs(have - float(ref)) <= 1e-12 * abs(float(ref))
    assert agem.num_projections() == 1
    cos = agem.cosine()
    assert cos.dim() == 0 and abs(float(cos) - float(gr / (g.norm() * r.norm()))) <= 1e-12


def test_agreeing_gradient_stays_bit_identical():
    net = _net()
    torch.manual_seed(5)
    g = torch.randn(_numel(net), dtype=torch.float64)
    agem = AGEM(net)
    _set_grads(net, g)
    agem.capture_reference()                     # r = g
    agem.project()
    assert torch.equal(_grads(net), g)
    assert agem.stats[3] == 0 and agem.num_projections() == 0


def test_no_reference_and_zero_reference_change_nothing():
    net = _net()
    torch.manual_seed(6)
    g = torch.randn(_numel(net), dtype=torch.float64)
    agem = AGEM(net)
    _set_grads(net, g)
    agem.project()                               # nothing captured yet
    assert torch.equal(_grads(net), g)
    _set_grads(net, torch.zeros_like(g))
    agem.capture_reference()                     # r == 0: r.r == 0, no division
    _set_grads(net, g)
    agem.project()
    got = _grads(net)
    assert torch.equal(got, g) and not torch.isnan(got).any()
    assert not torch.isnan(agem.stats).any() and agem.num_projections() == 0


def test_the_reference_is_a_copy_and_float32_modules_work():
    net = _net().float()
    torch.manual_seed(7)
    g = torch.randn(_numel(net))
    r = -g + 0.3 * torch.randn_like(g)
    agem = AGEM(net)
    _set_grads(net, r)
    agem.capture_reference()
    for p in net.parameters():                   # the captured reference must not follow later writes to .grad
        p.grad.zero_()
    _set_grads(net, g)
    agem.project()
    gd, rd = g.double(), r.double()
    want = gd - (gd * rd).sum() / (rd * rd).sum() * rd
    got = _grads(net)
    assert got.dtype == torch.float32
    assert (got.double() - want).abs().max() <= 2.0 ** -23 * want.abs().max()


def test_compute_reference_with_an_empty_memory_returns_false():
    net = _net()
    agem = AGEM(net, EpisodicMemory(capacity=8), ref_batch_size=4)
    assert agem.compute_reference(nn.MSELoss()) is False
    assert all(p.grad is None for p in net.parameters())
    assert AGEM(net).compute_reference(nn.MSELoss()) is False          # no memory at all


def test_compute_reference_draws_from_the_memory_and_leaves_no_gradient():
    net = _net().float()
    mem = EpisodicMemory(capacity=8)
    torch.manual_seed(8)
    for _ in range(6):
        mem.store(torch.randn(5), torch.randn(3))
    agem = AGEM(net, mem, ref_batch_size=4)
    assert agem.compute_reference(nn.MSELoss()) is True
    assert all(p.grad is None or not p.grad.any() for p in net.parameters())
    assert any(r.abs().max() > 0 for r in agem._ref)
    x, y = torch.randn(4, 5), torch.randn(4, 3)
    assert agem.compute_reference(nn.MSELoss(), batch=(x, y)) is True
    net.zero_grad()
    nn.functional.mse_loss(net(x), y).backward()
    assert torch.equal(torch.cat([r for r in agem._ref]).float(), _grads(net))


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_clip_grad_norm_on_cpu_parameters_is_torchs(max_norm):
    a, b = _net().float(), _net().float()
    torch.manual_seed(9)
    g = torch.randn(_numel(a))
    _set_grads(a, g)
    _set_grads(b, g)
    want = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
    got = ops.clip_grad_norm_(a, max_norm)
    assert torch.equal(got, want) and torch.equal(_grads(a), _grads(b))
    _set_grads(a, g)
    got = ops.clip_grad_norm_(a.parameters(), max_norm)                 # an iterable of parameters, as torch takes
    assert torch.equal(got, want) and torch.equal(_grads(a), _grads(b))


def test_the_script_accepts_the_agem_strategy_and_the_clip_flag():
    sys.path.insert(0, os.path.join(REPO, "experiments"))               # (the scripts import their sibling _common.py)
    spec = importlib.util.spec_from_file_location("train_continual_script", os.path.join(REPO, "experiments", "train_continual.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    d = parser.parse_args([])
    assert d.strategy == "ewc" and d.agem_ref_batch == 8 and d.clip_grad_norm is None
    a = parser.parse_args(["--strategy", "agem", "--agem-ref-batch", "4", "--clip-grad-norm", "1.0"])
    assert a.strategy == "agem" and a.agem_ref_batch == 4 and a.clip_grad_norm == 1.0
    assert callable(mod.train_with_agem)
