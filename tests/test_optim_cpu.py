"""CPU: nerve_cl.optim without a kernel - the run planner on hand-made layouts, the refusals, the state-dict format and its
exchange with torch.optim, the torch composition of the update rule (parameters on the CPU) against torch.optim.Adam / AdamW and
against the float64 recurrence within the derived bound (tests/optim_worker.py), and experiments/_common.make_optimizer."""
import copy
import importlib.util
import os

import pytest
import torch
import torch.nn as nn

from optim_worker import AdamF64, theta_bound_against

from nerve_cl.optim import BucketAdam, BucketAdamW, Slot, plan_runs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10


# ------------------------------------------------------------------------------------------------- the run planner

def _slots(spec):
    """spec: one (group, step, has_grad, fused) per slot"""
    return [Slot(*s) for s in spec]


def test_an_all_trainable_network_in_one_group_is_one_run():
    assert plan_runs(_slots([(0, 3, True, True)] * 7)) == ([(0, 6)], [])


def test_a_group_boundary_splits_the_run():
    slots = _slots([(0, 1, True, True)] * 2 + [(1, 1, True, True)] * 3 + [(0, 1, True, True)])
    assert plan_runs(slots) == ([(0, 1), (2, 4), (5, 5)], [])


def test_a_step_count_mismatch_splits_the_run():
    slots = _slots([(0, 4, True, True), (0, 4, True, True), (0, 2, True, True), (0, 4, True, True)])
    assert plan_runs(slots) == ([(0, 1), (2, 2), (3, 3)], [])


def test_a_slot_whose_gradient_does_not_alias_the_bucket_goes_alone_and_splits_the_run():
    slots = _slots([(0, 1, True, True), (0, 1, True, False), (0, 1, True, True), (0, 1, True, True)])
    assert plan_runs(slots) == ([(0, 0), (2, 3)], [1])


def test_a_frozen_prefix_costs_one_run_for_the_rest_and_a_missing_gradient_is_skipped():
    frozen = [(None, 0, False, False)] * 3
    assert plan_runs(_slots(frozen + [(0, 1, True, True)] * 4)) == ([(3, 6)], [])
    # this optimizer's parameter without a gradient: neither a run nor a single
    assert plan_runs(_slots([(0, 1, True, True), (0, 1, False, False), (0, 1, True, True)])) == ([(0, 0), (2, 2)], [])


def test_all_frozen_plans_nothing():
    assert plan_runs(_slots([(None, 0, False, False)] * 5)) == ([], [])
    assert plan_runs([]) == ([], [])


# ------------------------------------------------------------------------------------------------- refusals

def _mlp():
    torch.manual_seed(3)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3))


@pytest.mark.parametrize("option", ["amsgrad", "maximize", "capturable", "foreach"])
def test_unimplemented_options_raise_and_name_the_option(option):
    with pytest.raises(NotImplementedError, match=option):
        BucketAdam(_mlp().parameters(), **{option: True})


def test_a_parameter_that_is_not_fp32_raises():
    with pytest.raises(NotImplementedError, match="float64"):
        BucketAdamW(_mlp().double().parameters())
    with pytest.raises(NotImplementedError, match="bfloat16"):
        BucketAdam(_mlp().bfloat16().parameters())


def test_defaults_are_torchs():
    net = _mlp()
    for cls, ref in ((BucketAdam, torch.optim.Adam), (BucketAdamW, torch.optim.AdamW)):
        a, b = cls(net.parameters()).param_groups[0], ref(net.parameters()).param_groups[0]
        for k in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay"):
            assert a[k] == b[k], (cls.__name__, k)
    with pytest.raises(RuntimeError, match="ema_decay"):
        BucketAdam(net.parameters()).ema_state_dict()


# ------------------------------------------------------------------------------------------------- the update rule

def _feed(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


CASES = [(cls, wd, lr, s) for cls, wd in ((BucketAdam, 0.0), (BucketAdamW, 1e-2)) for lr in (1e-3, 1e-4) for s in (1e-3, 1.0)] \
    + [(BucketAdam, 1e-2, lr, None) for lr in (1e-3, 1e-4)]


@pytest.mark.parametrize("cls,wd,lr,s", CASES)
def test_cpu_composition_against_torch_and_float64(cls, wd, lr, s):
    """theta_0 = 0.1 randn, K = 10; gradients randn * s, or (Adam with L2 decay) random sign times U[0.5, 1.5]"""
    gen = torch.Generator().manual_seed(7)
    p = nn.Parameter(0.1 * torch.randn(4099, generator=gen))
    q = nn.Parameter(p.detach().clone())
    mine = cls([p], lr=lr, weight_decay=wd, ema_decay=0.9)
    ref = (torch.optim.AdamW if cls is BucketAdamW else torch.optim.Adam)([q], lr=lr, weight_decay=wd)
    f64 = AdamF64(p, lr, weight_decay=wd, decoupled=cls is BucketAdamW, ema_decay=0.9)
    for _ in range(K):
        if s is None:
            g = (torch.randint(0, 2, (4099,), generator=gen) * 2 - 1) * (0.5 + torch.rand(4099, generator=gen))
        else:
            g = torch.randn(4099, generator=gen) * s
        _feed([p, q], [g, g])
        mine.step()
        ref.step()
        f64.step(g)
    st = mine.state[p]
    f64.check(p, st["exp_avg"], st["exp_avg_sq"], mine.ema_state_dict()["param0"], what=f"{cls.__name__} wd={wd} lr={lr} s={s}")
    share = theta_bound_against(f64.theta0, p, q, K, lr)
    print(f"against torch.optim: largest difference / bound = {share:.3f}")
    assert share <= 1.0
    assert int(st["step"]) == K


def test_clipping_on_the_cpu_leaves_the_gradient_unscaled():
    gen = torch.Generator().manual_seed(8)
    ps = [nn.Parameter(0.1 * torch.randn(33, generator=gen)), nn.Parameter(0.1 * torch.randn(5, 4, generator=gen))]
    opt = BucketAdam(ps, lr=1e-3, max_grad_norm=0.5)
    refs = [AdamF64(p, 1e-3) for p in ps]
    for _ in range(3):
        gs = [torch.randn_like(p) for p in ps]
        _feed(ps, gs)
        opt.step()
        total = torch.cat([g.reshape(-1) for g in gs]).double().norm()
        for r, g in zip(refs, gs):
            r.step(g.reshape(-1), max_norm=0.5, total_norm=total)
        assert all(torch.equal(p.grad, g) for p, g in zip(ps, gs))
        assert abs(opt.last_grad_norm.item() - total.item()) <= 2.0 ** -22 * total.item()
    for r, p in zip(refs, ps):
        r.check(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], what="clipped")


def test_last_grad_norm_is_none_without_work_and_refusals_leave_the_step_counts_alone():
    ps = [nn.Parameter(torch.ones(3)), nn.Parameter(torch.ones(2, 2).t())]      # the second is not contiguous
    opt = BucketAdam(ps, max_grad_norm=1.0)
    assert opt.last_grad_norm is None
    _feed(ps, [torch.ones(3), None])
    opt.step()
    assert opt.last_grad_norm.item() == pytest.approx(3 ** 0.5)
    _feed(ps, [torch.ones(3), torch.ones(2, 2)])
    with pytest.raises(NotImplementedError, match="non-contiguous"):
        opt.step()
    assert int(opt.state[ps[0]]["step"]) == 1 and ps[1] not in opt.state    # refused before anything moved
    _feed(ps, [None, None])
    opt.step()
    assert opt.last_grad_norm is None and int(opt.state[ps[0]]["step"]) == 1


def test_a_parameter_without_a_gradient_is_skipped_and_its_step_does_not_advance():
    net = _mlp()
    ps = list(net.parameters())
    opt = BucketAdam(ps, lr=1e-2, weight_decay=0.1)
    _feed(ps, [torch.ones_like(p) for p in ps])
    opt.step()
    before = ps[1].detach().clone()
    _feed(ps, [torch.ones_like(ps[0]), None, torch.ones_like(ps[2]), torch.ones_like(ps[3])])
    opt.step()
    assert torch.equal(ps[1], before)                                   # weight decay included
    assert [int(opt.state[p]["step"]) for p in ps] == [2, 1, 2, 2]


def test_param_groups_and_a_scheduler():
    net, twin = _mlp(), _mlp()
    groups = lambda m: [{"params": m[0].parameters()}, {"params": m[2].parameters(), "lr": 2.5e-4, "weight_decay": 1e-3}]  # noqa: E731
    a, b = BucketAdam(groups(net), lr=1e-3), torch.optim.Adam(groups(twin), lr=1e-3)
    sa, sb = torch.optim.lr_scheduler.StepLR(a, 1, 0.5), torch.optim.lr_scheduler.StepLR(b, 1, 0.5)
    for k in range(3):
        gs = [torch.randn_like(p) for p in net.parameters()]
        _feed(net.parameters(), gs)
        _feed(twin.parameters(), gs)
        a.step(), b.step(), sa.step(), sb.step()
    assert a.param_groups[1]["lr"] == b.param_groups[1]["lr"] == 2.5e-4 / 8
    for p, q in zip(net.parameters(), twin.parameters()):
        assert torch.equal(p, q)        # the same fp32 operations in the same order on the CPU


# ------------------------------------------------------------------------------------------------- state dict

def _three_steps(cls, ref_cls, **kw):
    net, twin = _mlp(), _mlp()
    a, b = cls(net.parameters(), lr=1e-3, **kw), ref_cls(twin.parameters(), lr=1e-3, **kw)
    for _ in range(3):
        gs = [torch.randn_like(p) for p in net.parameters()]
        _feed(net.parameters(), gs)
        _feed(twin.parameters(), gs)
        a.step(), b.step()
    return net, twin, a, b


def test_state_dict_has_torchs_format():
    net, twin, a, b = _three_steps(BucketAdam, torch.optim.Adam, weight_decay=1e-2)
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) == {"state", "param_groups"}
    assert set(sa["state"]) == set(sb["state"]) == {0, 1, 2, 3}
    for i in sa["state"]:
        assert set(sa["state"][i]) == set(sb["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        x, y = sa["state"][i]["step"], sb["state"][i]["step"]
        assert x.dtype == y.dtype and x.shape == y.shape == () and x.device == y.device and x == y == 3
        for k in ("exp_avg", "exp_avg_sq"):
            assert sa["state"][i][k].shape == sb["state"][i][k].shape and torch.equal(sa["state"][i][k], sb["state"][i][k])
    assert set(sa["param_groups"][0]) == set(sb["param_groups"][0])
    assert sa["param_groups"][0]["params"] == sb["param_groups"][0]["params"] == [0, 1, 2, 3]
    with_ema = BucketAdam(net.parameters(), ema_decay=0.5).state_dict()
    assert set(with_ema) == {"state", "param_groups", "ema"} and len(with_ema["ema"]) == 4


@pytest.mark.parametrize("cls,ref_cls", [(BucketAdam, torch.optim.Adam), (BucketAdamW, torch.optim.AdamW)])
def test_state_dict_travels_in_both_directions(cls, ref_cls):
    net, twin, a, b = _three_steps(cls, ref_cls, weight_decay=1e-2)
    net2, twin2 = copy.deepcopy(net), copy.deepcopy(twin)
    a2, b2 = cls(net2.parameters()), ref_cls(twin2.parameters())
    a2.load_state_dict(copy.deepcopy(b.state_dict()))                   # torch's -> this class
    b2.load_state_dict(copy.deepcopy(a.state_dict()))                   # this class's -> torch
    assert a2.param_groups[0]["lr"] == 1e-3 and a2.param_groups[0]["weight_decay"] == 1e-2
    gs = [torch.randn_like(p) for p in net.parameters()]
    for m, o in ((net, a), (twin, b), (net2, a2), (twin2, b2)):
        _feed(m.parameters(), gs)
        o.step()
    for p, q, p2, q2 in zip(net.parameters(), twin.parameters(), net2.parameters(), twin2.parameters()):
        assert torch.equal(p, q) and torch.equal(p2, q) and torch.equal(q2, q)
    assert all(int(a2.state[p]["step"]) == 4 for p in net2.parameters())


def test_a_state_dict_with_averages_loads_into_torch_and_into_its_own_class():
    net = _mlp()
    a = BucketAdam(net.parameters(), lr=1e-3, ema_decay=0.75)
    for _ in range(3):
        _feed(net.parameters(), [torch.randn_like(p) for p in net.parameters()])
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert len(sd["ema"]) == 4 and all(not torch.equal(e, p) for e, p in zip(sd["ema"], net.parameters()))
    twin = copy.deepcopy(net)
    b = torch.optim.Adam(twin.parameters())
    b.load_state_dict(copy.deepcopy(sd))                                # torch ignores the extra top-level key
    for p, q in zip(net.parameters(), twin.parameters()):
        assert int(b.state[q]["step"]) == 3
        assert torch.equal(b.state[q]["exp_avg"], a.state[p]["exp_avg"]) and torch.equal(b.state[q]["exp_avg_sq"], a.state[p]["exp_avg_sq"])
    net2 = copy.deepcopy(net)
    a2 = BucketAdam(net2.parameters(), ema_decay=0.75)                   # its averages start as the weights ...
    a2.load_state_dict(copy.deepcopy(sd))                               # ... and are the saved ones after the load
    assert all(torch.equal(x, y) for x, y in zip(a2.ema_state_dict().values(), sd["ema"]))
    gs = [torch.randn_like(p) for p in net.parameters()]
    for m, o in ((net, a), (twin, b), (net2, a2)):
        _feed(m.parameters(), gs)
        o.step()
    for p, q, p2 in zip(net.parameters(), twin.parameters(), net2.parameters()):
        assert torch.equal(p, q) and torch.equal(p, p2)
    assert all(torch.equal(x, y) for x, y in zip(a2.ema_state_dict().values(), a.ema_state_dict().values()))


def test_a_state_dict_written_with_amsgrad_is_refused():
    net = _mlp()
    sd = torch.optim.Adam(net.parameters(), amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError, match="amsgrad"):
        BucketAdam(net.parameters()).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------- EMA

def test_ema_swap_and_copy_on_a_plain_module():
    net = _mlp()
    opt = BucketAdam(net.named_parameters(), lr=1e-2, ema_decay=0.75)
    start = [p.detach().clone() for p in net.parameters()]
    want = [p.detach().double().clone() for p in net.parameters()]
    for _ in range(4):
        _feed(net.parameters(), [torch.randn_like(p) for p in net.parameters()])
        opt.step()
        want = [0.75 * w + 0.25 * p.detach().double() for w, p in zip(want, net.parameters())]
    ema = opt.ema_state_dict()
    assert list(ema) == [n for n, _ in net.named_parameters()]
    for (n, p), w, s in zip(net.named_parameters(), want, start):
        assert (ema[n].double() - w).abs().max() <= 4 * 2.0 ** -23 * w.abs().max() and not torch.equal(ema[n], p)
    now = [p.detach().clone() for p in net.parameters()]
    with opt.swap_ema():
        for (n, p), w in zip(net.named_parameters(), want):
            assert (p.double() - w).abs().max() <= 4 * 2.0 ** -23 * w.abs().max()
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), now))
    teacher = _mlp()
    res = opt.copy_ema_to(teacher)
    assert not res.unexpected_keys and not res.missing_keys
    assert all(torch.equal(p, ema[n]) for n, p in teacher.named_parameters())


def test_a_bucketed_network_on_the_cpu_keeps_flat_state_with_zero_padding():
    from nerve_cl.models import SuperResolutionNet
    torch.manual_seed(0)
    net = SuperResolutionNet(3, 2, 16, 1, 1)
    for p in net.feature_extractor.parameters():
        p.requires_grad_(False)
    opt = BucketAdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3, ema_decay=0.9)
    assert len(opt._nets) == 1 and opt._nets[0].net is net and not opt._loose
    frozen = [p.detach().clone() for p in net.feature_extractor.parameters()]
    for _ in range(2):
        for p in net.parameters():
            p.grad = torch.randn_like(p) if p.requires_grad else None
        opt.step()
    assert opt.last_launches == 0                                       # no kernel on the CPU
    ns = opt._nets[0]
    lay, total = net._bucket_layout()
    pad = torch.ones(total, dtype=torch.bool)
    for o, k in lay.values():
        pad[o:o + k] = False
    assert pad.any()
    for flat in (net.flat_theta(), ns.m, ns.v, ns.ema):
        assert not flat[pad].any()
    assert all(torch.equal(p, f) for p, f in zip(net.feature_extractor.parameters(), frozen))
    assert all(p not in opt.state for p in net.feature_extractor.parameters())
    name, p = [(n, q) for n, q in net.named_parameters() if q.requires_grad][-1]
    assert opt.state[p]["exp_avg"].data_ptr() == ns.m.data_ptr() + 4 * lay[name][0]
    twin = copy.deepcopy(net)                                           # a deepcopy is found as a network of its own
    assert [n.net for n in BucketAdam(twin.parameters())._nets] == [twin]


# ------------------------------------------------------------------------------------------------- the scripts

def _common():
    spec = importlib.util.spec_from_file_location("experiments_common_for_optim", os.path.join(REPO, "experiments", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_make_optimizer_torch_is_todays_path_and_bucket_maps_the_classes():
    common = _common()
    net = _mlp()
    for impl in ((), ("torch",)):
        opt = common.make_optimizer(torch.optim.AdamW, net.parameters(), *impl, lr=3e-4, weight_decay=1e-5)
        assert type(opt) is torch.optim.AdamW
        g = opt.param_groups[0]
        assert g["lr"] == 3e-4 and g["weight_decay"] == 1e-5 and g["fused"] is None       # fused only for fp32 GPU parameters
        assert [id(p) for p in g["params"]] == [id(p) for p in net.parameters()]
    assert type(common.make_optimizer(torch.optim.Adam, net.parameters(), "bucket", lr=1e-4)) is BucketAdam
    opt = common.make_optimizer(torch.optim.AdamW, net.parameters(), "bucket", lr=1e-4, ema_decay=0.99, max_grad_norm=1.0)
    assert type(opt) is BucketAdamW and opt.ema_decay == 0.99 and opt.max_grad_norm == 1.0
    with pytest.raises(NotImplementedError, match="SGD"):
        common.make_optimizer(torch.optim.SGD, net.parameters(), "bucket", lr=1e-4)


@pytest.mark.parametrize("script", ["train_baseline", "train_continual"])
def test_the_scripts_take_the_optimizer_flags(script):
    spec = importlib.util.spec_from_file_location(f"{script}_for_optim", os.path.join(REPO, "experiments", f"{script}.py"))
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.path.insert(0, os.path.join(REPO, "experiments"))
    spec.loader.exec_module(mod)
    common = _common()
    args = mod.build_parser().parse_args([])
    assert args.optimizer_impl == "torch" and args.ema_decay is None and common.optimizer_impl(args) == "torch"
    args = mod.build_parser().parse_args(["--ema-decay", "0.999"])
    assert common.optimizer_impl(args) == "bucket"
    assert common.optimizer_impl(mod.build_parser().parse_args(["--optimizer-impl", "bucket"])) == "bucket"
