"""GPU: the distillation kernels (csrc/distill.hip) behind nerve_cl.ops.distill_loss / cosine_feature_loss, the
ContinualDistillation strategy on a small SuperResolutionNet, and experiments/train_continual.py --strategy distill.

Every yardstick is the formula written here with torch ops in float64 (autograd for the gradients), never nerve_cl code and
never F.cosine_similarity.  Bounds: 2e-5 is the project's fp32-kernel bound: relative on the three rows
of the distill kernel (MSE values), absolute on the cosine values (they lie in [0, 2]), and relative to the gradient's largest
element on every gradient.  Where the exact gradient cancels (near-equal features) the bound is 4 x the error of the same
formula run by torch in fp32 plus 2e-5 of the max, capped at 1e-3 of the max - the rule tests/test_metrics_gpu.py uses for
SSIM.  With C = 1 the exact gradient is zero and |ds_p| <= 1e-6 |go| / (N |s_p|): a few ulp of the two cancelling terms.
Every figure is printed before it is asserted.
"""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5
UP = (0.5, 1.0, -2.0)                    # per-sample upstream gradients
UP_MEAN = 1.5                            # upstream gradient of a mean-reduced value


def dev():
    return torch.device("cuda", 0)


def upstream(B, per_sample):
    return torch.tensor(UP[:B] if per_sample else [UP_MEAN], dtype=torch.float64, device=dev())


def max_rel(got, ref):
    """largest error of `got` relative to the largest element of `ref`"""
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ============================================================================================================== distill kernel

DISTILL_SHAPES = {1: (1,), 105: (3, 5, 7), 3 * 128 * 128: (3, 128, 128)}       # per -> a sample's shape
WEIGHTS = [("alpha", 0.0), ("alpha", 0.3), ("alpha", 1.0), ("folded", (0.3, 1.7))]


@functools.lru_cache(maxsize=None)
def distill_inputs(per, B):
    g = torch.Generator().manual_seed(1000 + per + B)
    shape = (B, *DISTILL_SHAPES[per])
    y = torch.rand(shape, generator=g)
    t = y + 0.1 * torch.randn(shape, generator=g)
    s = t + 0.05 * torch.randn(shape, generator=g)
    return s.to(dev()), t.to(dev()), y.to(dev())


def distill_ref(s, t, y, wt, wy, per_sample, up):
    """float64: (value, d, m, d(sum up * value) / ds)"""
    sr = s.double().requires_grad_(True)
    dims = tuple(range(1, s.dim())) if per_sample else tuple(range(s.dim()))
    d = ((sr - t.double()) ** 2).mean(dim=dims)
    m = ((sr - y.double()) ** 2).mean(dim=dims) if y is not None else torch.zeros_like(d)
    v = wt * d + wy * m
    (v.reshape(-1) * up).sum().backward()
    return v.detach(), d.detach(), m.detach(), sr.grad


@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no-target"])
@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", list(DISTILL_SHAPES))
def test_distill_value_terms_and_gradient(per, B, reduction, with_target):
    from nerve_cl import ops
    s, t, y = distill_inputs(per, B)
    y = y if with_target else None
    per_sample = reduction == "none"
    up = upstream(B, per_sample)
    for kind, w in WEIGHTS:
        if kind == "alpha":
            wt, wy = (w, 1.0 - w) if with_target else (1.0, 0.0)
        else:
            wt, wy = w if with_target else (w[0], 0.0)
        sr = s.clone().requires_grad_(True)
        if kind == "alpha":
            v, d, m = ops.distill_loss(sr, t, y, alpha=w, reduction=reduction, return_terms=True)
        else:
            v, d, m = ops._distill_weighted(sr, t, y, w[0], w[1], reduction)
        assert v.shape == ((B,) if per_sample else ()) and d.shape == v.shape and m.shape == v.shape
        assert v.requires_grad and not d.requires_grad and not m.requires_grad
        (v.reshape(-1).double() * up).sum().backward()
        rv, rd, rm, rg = distill_ref(s, t, y, wt, wy, per_sample, up)
        for name, got, ref in (("value", v, rv), ("d", d, rd), ("m", m, rm)):
            err = (got.detach().double().reshape(-1) - ref.reshape(-1)).abs()
            tol = BOUND * ref.reshape(-1).abs()
            print(f"per={per} B={B} {reduction} target={with_target} {kind}={w} {name}: err/|ref| "
                  f"{(err / ref.reshape(-1).abs().clamp_min(1e-300)).max().item():.3e}")
            assert bool((err <= tol).all()), (name, got, ref)
        gerr = max_rel(sr.grad, rg)
        print(f"per={per} B={B} {reduction} target={with_target} {kind}={w} ds: {gerr:.3e} of max")
        assert sr.grad.shape == s.shape and gerr <= BOUND


def test_distill_misaligned_slice_equals_its_clone():
    from nerve_cl import ops
    g = torch.Generator().manual_seed(7)
    big = [torch.randn(3, 105, generator=g).to(dev()) for _ in range(3)]
    sl = [b[1:2] for b in big]                               # contiguous, 420 bytes into the allocation: not 16-byte aligned
    assert all(x.is_contiguous() and x.data_ptr() % 16 != 0 for x in sl)
    res = []
    for s, t, y in (sl, [x.clone() for x in sl]):
        sr = s.detach().requires_grad_(True)
        out = ops.distill_loss(sr, t, y, alpha=0.3, reduction="none", return_terms=True)
        out[0].sum().backward()
        res.append((*out, sr.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_distill_two_calls_are_bit_identical():
    from nerve_cl import ops
    s, t, y = distill_inputs(3 * 128 * 128, 3)
    res = []
    for _ in range(2):
        sr = s.clone().requires_grad_(True)
        out = ops.distill_loss(sr, t, y, alpha=0.3, reduction="none", return_terms=True)
        (out[0] * torch.tensor(UP, device=dev())).sum().backward()
        res.append((*out, sr.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# =============================================================================================================== cosine kernel

COSINE_SHAPES = [(3, 3, 5, 7), (2, 16, 16, 16), (2, 64, 64, 64), (1, 64, 9, 13)]
C1_SHAPES = [(2, 1, 1, 1), (3, 1, 9, 13)]
EPS_CLAMP = 1e-2


def cosine_formula(s, t, eps):
    """(B, H, W) map v_p = 1 - ab / (max(sqrt a, eps) max(sqrt b, eps)) in the dtype of s (differentiable in s).  The clamp is
    written as sqrt(max(a, eps^2)): the same value, and a zero gradient (not 0 * inf) where it is active."""
    a, b, ab = (s * s).sum(1), (t * t).sum(1), (s * t).sum(1)
    ns, nt = a.clamp_min(eps * eps).sqrt(), b.clamp_min(eps * eps).sqrt()
    return 1 - ab / (ns * nt)


def cosine_ref(s, t, eps, per_sample, up, dtype=torch.float64, device=None):
    """(value (B,) or (1,), d(sum up * value) / ds) by torch ops in `dtype`"""
    device = device or s.device
    sr = s.detach().to(device, dtype).requires_grad_(True)
    v = cosine_formula(sr, t.to(device, dtype), eps)
    v = v.mean(dim=(1, 2)) if per_sample else v.mean().reshape(1)
    (v * up.to(device, dtype)).sum().backward()
    return v.detach().to(s.device), sr.grad.to(s.device)


def directions(shape, g):
    """unit vectors over the channel axis"""
    v = torch.randn(shape, generator=g)
    return v / (v * v).sum(1, keepdim=True).sqrt()


@functools.lru_cache(maxsize=None)
def cosine_inputs(shape, case):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2000 + C * H + W + len(case))
    if case == "random":
        s, t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    elif case == "clamp":
        # norms in [0.5, 2] (50 x above eps = 1e-2) except about 30 % of the positions of each tensor, in [0.5e-3, 1e-3] (10 x
        # below): every norm is at least 10 x away from eps
        out = []
        for _ in range(2):
            r = 0.5 + 1.5 * torch.rand(B, 1, H, W, generator=g)
            small = torch.rand(B, 1, H, W, generator=g) < 0.3
            r = torch.where(small, 1e-3 * (0.5 + 0.5 * torch.rand(B, 1, H, W, generator=g)), r)
            out.append(directions(shape, g) * r)
        s, t = out
    elif case == "near":
        s = torch.randn(shape, generator=g)
        t = s + 1e-2 * torch.randn(shape, generator=g)
    else:                                                   # "c1": |s| >= 0.1
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        s = sign * (0.1 + 0.9 * torch.rand(shape, generator=g))
        t = torch.randn(shape, generator=g)
        t = torch.where(t.abs() < 0.05, torch.full_like(t, 0.05), t)
    return s.to(dev()), t.to(dev())


def run_cosine(s, t, eps, reduction, up):
    from nerve_cl import ops
    sr = s.clone().requires_grad_(True)
    v = ops.cosine_feature_loss(sr, t, eps=eps, reduction=reduction)
    assert v.shape == ((s.shape[0],) if reduction == "none" else ())
    (v.reshape(-1).double() * up).sum().backward()
    assert sr.grad.shape == s.shape
    return v.detach().reshape(-1), sr.grad


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("shape", COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_random(shape, reduction):
    s, t = cosine_inputs(shape, "random")
    up = upstream(shape[0], reduction == "none")
    v, g = run_cosine(s, t, 1e-8, reduction, up)
    rv, rg = cosine_ref(s, t, 1e-8, reduction == "none", up)
    verr, gerr = (v.double() - rv).abs().max().item(), max_rel(g, rg)
    print(f"{shape} {reduction} random: value {rv.tolist()} err {verr:.3e}, ds {gerr:.3e} of max")
    assert verr <= BOUND and gerr <= BOUND


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("shape", COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_clamp(shape, reduction):
    s, t = cosine_inputs(shape, "clamp")
    for x in (s, t):                                        # every norm at least 10 x away from eps
        n = (x.double() ** 2).sum(1).sqrt()
        assert bool(((n >= 10 * EPS_CLAMP) | (n <= EPS_CLAMP / 10)).all())
    up = upstream(shape[0], reduction == "none")
    v, g = run_cosine(s, t, EPS_CLAMP, reduction, up)
    rv, rg = cosine_ref(s, t, EPS_CLAMP, reduction == "none", up)
    verr = (v.double() - rv).abs().max().item()
    print(f"{shape} {reduction} clamp: value {rv.tolist()} err {verr:.3e}")
    assert verr <= BOUND
    # clamped positions' gradients are ~30 x larger and would hide the others: each set against its own max
    clamped = ((s.double() ** 2).sum(1, keepdim=True).sqrt() <= EPS_CLAMP).expand_as(s)
    assert bool(clamped.any()) and bool((~clamped).any())
    for name, mask in (("clamped", clamped), ("unclamped", ~clamped)):
        gerr = max_rel(g[mask], rg[mask])
        print(f"{shape} {reduction} clamp: ds over {name} positions {gerr:.3e} of their max {rg[mask].abs().max().item():.3e}")
        assert gerr <= BOUND


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("shape", COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_near_equal(shape, reduction):
    s, t = cosine_inputs(shape, "near")
    up = upstream(shape[0], reduction == "none")
    v, g = run_cosine(s, t, 1e-8, reduction, up)
    rv, rg = cosine_ref(s, t, 1e-8, reduction == "none", up)
    _, g32 = cosine_ref(s, t, 1e-8, reduction == "none", up, dtype=torch.float32, device=torch.device("cpu"))
    verr, gerr, err32 = (v.double() - rv).abs().max().item(), max_rel(g, rg), max_rel(g32, rg)
    bound = min(4 * err32 + BOUND, 1e-3)
    print(f"{shape} {reduction} near-equal: value {rv.tolist()} err {verr:.3e}, ds {gerr:.3e} of max "
          f"(fp32 torch {err32:.3e}, bound {bound:.3e})")
    assert verr <= BOUND * 1 and gerr <= bound


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("shape", C1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_single_channel(shape, reduction):
    """C = 1: v_p = 1 - sign(s t) and the exact gradient is zero; the kernel's two terms cancel to a few ulp"""
    s, t = cosine_inputs(shape, "c1")
    B, _, H, W = shape
    per_sample = reduction == "none"
    up = upstream(B, per_sample)
    v, g = run_cosine(s, t, 1e-8, reduction, up)
    rv, _ = cosine_ref(s, t, 1e-8, per_sample, up)
    verr = (v.double() - rv).abs().max().item()
    go = up.abs().reshape(-1, 1, 1, 1) if per_sample else up.abs().reshape(1, 1, 1, 1)
    N = H * W if per_sample else B * H * W
    limit = 1e-6 * go / (N * s.double().abs())
    worst = (g.double().abs() / limit).max().item()
    print(f"{shape} {reduction} C=1: value {rv.tolist()} err {verr:.3e}, worst |ds| / limit {worst:.3e}")
    assert verr <= BOUND and bool((g.double().abs() <= limit).all())


@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_cosine_list_is_the_mean_of_its_entries(reduction):
    from nerve_cl import ops
    pairs = [cosine_inputs((2, 16, 16, 16), "random"), cosine_inputs((2, 64, 64, 64), "near"),
             cosine_inputs((2, 64, 64, 64), "random")]
    up = upstream(2, reduction == "none")
    ss = [s.clone().requires_grad_(True) for s, _ in pairs]
    ts = [t for _, t in pairs]
    v = ops.cosine_feature_loss(ss, ts, reduction=reduction)
    (v.reshape(-1).double() * up).sum().backward()
    single = [run_cosine(s, t, 1e-8, reduction, up) for s, t in pairs]
    want = sum(x[0] for x in single) / len(pairs)
    assert (v.detach().reshape(-1) - want).abs().max().item() <= 1e-6
    for sr, (_, g) in zip(ss, single):
        assert max_rel(sr.grad, g.double() / len(pairs)) <= 1e-6


def test_cosine_two_calls_are_bit_identical():
    s, t = cosine_inputs((2, 64, 64, 64), "random")
    up = upstream(2, True)
    a, b = run_cosine(s, t, 1e-8, "none", up), run_cosine(s, t, 1e-8, "none", up)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ================================================================================================================== whole path

ALPHA, FEATURE_WEIGHT, KEYS = 0.5, 0.5, ("features", "aggregated")


def torch_parts(out, inter, t_out, t_inter, y):
    """task, distill, feature of the issue's formulas from the network's outputs and intermediates, in float64"""
    o, t, yd = out.double(), t_out.double(), y.double()
    m, d = ((o - yd) ** 2).mean(), ((o - t) ** 2).mean()

    def cos(a, b):
        return cosine_formula(a.double(), b.double(), 1e-8).mean()

    feature = sum(cos(a, b) for a, b in zip(inter["features"], t_inter["features"])) / len(inter["features"]) \
        + cos(inter["aggregated"], t_inter["aggregated"])
    return m, ALPHA * d + (1 - ALPHA) * m, feature


def grads_of(net, total):
    net.zero_grad(set_to_none=True)
    total.backward()
    return {n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().clone() for n, p in net.named_parameters()}


def compare_grads(tag, got, ref, bound=1e-3):
    worst = 0.0
    for n, r in ref.items():
        if r.norm() == 0:
            assert got[n].norm() == 0, n
            continue
        e = ((got[n] - r).norm() / r.norm()).item()
        worst = max(worst, e)
        assert e <= bound, (tag, n, e)
    print(f"{tag}: worst per-tensor relative L2 of the parameter gradients {worst:.3e}")


def test_continual_distillation_on_the_sr_network():
    from nerve_cl import ops
    from nerve_cl.continual import ContinualDistillation
    from nerve_cl.models import SuperResolutionNet
    torch.manual_seed(0)
    net = SuperResolutionNet(3, 2, 16, 1, 1).to(dev()).train()          # fp32 math, eager (the defaults)
    x = torch.rand(2, 3, 3, 16, 16, device=dev())
    y = torch.rand(2, 3, 32, 32, device=dev())
    crit = ops.MSELoss()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    cd = ContinualDistillation(net, alpha=ALPHA, feature_weight=FEATURE_WEIGHT, feature_keys=KEYS)
    for register in (True, False):          # one step, the teacher, one more step: the student has left its teacher
        opt.zero_grad()
        cd.compute_loss(x, y, crit)["total"].backward()
        opt.step()
        if register:
            cd.register_task()

    losses = cd.compute_loss(x, y, crit)
    assert set(losses) == {"task", "distill", "total", "feature"} and all(v.requires_grad for v in losses.values())
    got = grads_of(net, losses["total"])

    with torch.no_grad():
        t_out, t_inter = cd.teacher(x, return_intermediate=True)
    out, inter = net(x, return_intermediate=True)
    task, distill, feature = torch_parts(out, inter, t_out, t_inter, y)
    total = task + distill + FEATURE_WEIGHT * feature
    ref = grads_of(net, total)
    for name, ref_v in (("task", task), ("distill", distill), ("feature", feature), ("total", total)):
        g, r = losses[name].item(), ref_v.item()
        print(f"{name}: {g:.8f} vs float64 torch ops {r:.8f}")
        assert abs(g - r) <= BOUND * max(abs(r), 1.0 if name in ("feature", "total") else 0.0)
    assert distill.item() > 0 and feature.item() > 0
    compare_grads("unfolded vs torch-op losses", got, ref)

    folded = ContinualDistillation(net, alpha=ALPHA, feature_weight=FEATURE_WEIGHT, feature_keys=KEYS, fold_task=True)
    folded.teacher = cd.teacher
    fl = folded.compute_loss(x, y, crit)
    assert fl["total"].requires_grad and not fl["task"].requires_grad and not fl["distill"].requires_grad
    for name in ("task", "distill", "feature", "total"):
        g, r = fl[name].item(), losses[name].item()
        print(f"folded {name}: {g:.8f} vs unfolded {r:.8f}")
        assert abs(g - r) <= BOUND * max(abs(r), 1.0 if name in ("feature", "total") else 0.0)
    compare_grads("folded vs unfolded", grads_of(net, fl["total"]), got)
    with pytest.raises(ValueError, match="fold_task"):
        folded.compute_loss(x, y, ops.L1Loss())


# ====================================================================================================================== script

@pytest.mark.parametrize("extra", [[], ["--precision", "fp32", "--graphs", "off"]], ids=["default", "fp32-eager"])
def test_train_continual_distill_strategy(extra, tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "experiments", "train_continual.py"),
           "--strategy", "distill", "--tasks", "2", "--samples", "16", "--epochs", "1", "--features", "16", "--blocks", "1",
           "--feature-distill", "0.1", *extra]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    task1 = r.stdout.split("Training on Task 1")[1]
    m = re.search(r"Distill=([0-9.eE+-]+) Feature=([0-9.eE+-]+)", task1)
    assert m and float(m.group(1)) > 0
    assert "Training complete!" in r.stdout
