"""GPU: the multi-scale SSIM kernels (csrc/quality.hip) behind nerve_cl.ops.ms_ssim_loss and nerve_cl.metrics.ms_ssim.

The yardstick is the definition written here with torch ops in float64 (shifted-slice blurs, F.avg_pool2d, relu, pow; autograd
for the gradient), never the code under test.  Bounds of the value-and-gradient cases: the kernels' value error and the
relative L2 error of dx against float64 are each at most 4 x the error that the SAME formula has when torch runs it in fp32
(whose E[x^2] - mu^2 cancels; the kernels centre their moments), and under the fixed ceilings of 2e-5 on the value and 2e-4 on dx, so that
an ill-conditioned yardstick cannot hide a wrong kernel.  Every figure is printed before it is asserted.

Inputs: target = rand, pred = clamp(target + 0.05 randn, 0, 1), seeded.  At every shape used here the smallest per-plane mean
is above 0.98, so the clamp of the definition is inactive except in the test that aims at it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STANDARD = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
VALUE_CAP, GRAD_CAP = 2e-5, 2e-4


def dev():
    return torch.device("cuda", 0)


def std_weights(M):
    head = STANDARD[:M]
    return tuple(w / sum(head) for w in head) if M < 5 else STANDARD


# ------------------------------------------------------------------------------------------------ the definition, any dtype

def taps(dtype):
    """11 Gaussian taps, sigma 1.5, normalised to sum 1 in fp32"""
    d = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(d * d) / (2 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def blur(t, g):
    """valid separable 11-tap filter along W then H, as shifted slices (any dtype, differentiable)"""
    W = t.shape[-1]
    h = sum(g[k] * t[..., k:W - 10 + k] for k in range(11))
    H = t.shape[-2]
    return sum(g[k] * h[..., k:H - 10 + k, :] for k in range(11))


def ms_ssim_ref(x, y, weights, L=1.0, dtype=torch.float64):
    """per-sample MS-SSIM (B,) by torch ops in `dtype`"""
    x, y = x.to(dtype), y.to(dtype)
    g = taps(dtype).to(x.device)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    v = None
    for j, w in enumerate(weights):
        mx, my = blur(x, g), blur(y, g)
        sxx, syy, sxy = blur(x * x, g) - mx * mx, blur(y * y, g) - my * my, blur(x * y, g) - mx * my
        m = (2 * sxy + c2) / (sxx + syy + c2)
        if j == len(weights) - 1:
            m = m * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        term = torch.relu(m.mean(dim=(2, 3))) ** w                       # (B, C)
        v = term if v is None else v * term
        if j < len(weights) - 1:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return v.mean(dim=1)


def ref_with_grad(x, y, weights, up, L, dtype):
    """(per-sample MS-SSIM, d(sum_b up_b * (1 - ms_b)) / dx) in `dtype`"""
    xr = x.detach().to(dtype).requires_grad_(True)
    s = ms_ssim_ref(xr, y, weights, L, dtype)
    ((1 - s) * up.to(dtype)).sum().backward()
    return s.detach(), xr.grad.detach()


def images(shape, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g)
    x = (y + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return x.to(dev()), y.to(dev())


def rel_l2(a, ref):
    return ((a.double() - ref.double()).norm() / ref.double().norm()).item()


CASES = [((2, 3, 23, 27), 2), ((2, 1, 45, 47), 3), ((2, 3, 64, 128), 3), ((1, 1, 100, 200), 3), ((1, 3, 177, 181), 5),
         ((1, 3, 176, 176), 5)]


@functools.lru_cache(maxsize=None)
def reference(shape, M):
    """inputs and the float64 / fp32 torch results of one case, computed once and shared (nothing modifies them)"""
    B = shape[0]
    x, y = images(shape, 100 + shape[2] + M)
    w = std_weights(M)
    up = (0.5 + torch.rand(B, generator=torch.Generator().manual_seed(5))).to(dev())      # per-sample upstream gradients
    mean = torch.full((B,), 1.0 / B, device=dev())
    r = {"x": x, "y": y, "w": w, "up": up}
    for name, dtype in (("64", torch.float64), ("32", torch.float32)):
        r["ms" + name], r["g_none" + name] = ref_with_grad(x, y, w, up, 1.0, dtype)
        _, r["g_mean" + name] = ref_with_grad(x, y, w, mean, 1.0, dtype)
    return r


# ------------------------------------------------------------------------------------- 1. value and gradient against float64

@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("shape,M", CASES, ids=[f"{'x'.join(map(str, s))}-M{m}" for s, m in CASES])
def test_value_and_gradient(shape, M, reduction):
    from nerve_cl import metrics, ops
    r = reference(shape, M)
    x, y, w = r["x"], r["y"], r["w"]
    weights = None if M == 5 else w                       # five scales: the default argument is the standard tuple
    ms64, ms32 = r["ms64"], r["ms32"]
    assert ms64.min().item() > 0.9                        # the clamp is inactive here
    xr = x.clone().requires_grad_(True)
    loss = ops.ms_ssim_loss(xr, y, weights=weights, reduction=reduction)
    val = metrics.ms_ssim(x, y, weights=weights, reduction=reduction)
    if reduction == "none":
        assert loss.shape == val.shape == (shape[0],)
        (loss * r["up"]).sum().backward()
        want, want32 = ms64, ms32.double()
        want_l32 = (1 - ms32).double()
    else:
        assert loss.shape == val.shape == ()
        loss.backward()
        want, want32 = ms64.mean(), ms32.mean().double()
        want_l32 = (1 - ms32.mean()).double()
    g64, g32 = r["g_" + reduction + "64"], r["g_" + reduction + "32"]
    e_v, e_v32 = (val.double() - want).abs().max().item(), (want32 - want).abs().max().item()
    e_l, e_l32 = (loss.detach().double() - (1 - want)).abs().max().item(), (want_l32 - (1 - want)).abs().max().item()
    e_g, e_g32 = rel_l2(xr.grad, g64), rel_l2(g32, g64)
    print(f"ms_ssim {shape} M={M} {reduction}: MS-SSIM {ms64.tolist()} | value err kernel {e_v:.3e} fp32 torch {e_v32:.3e} | "
          f"loss err kernel {e_l:.3e} fp32 torch {e_l32:.3e} | dx rel L2 kernel {e_g:.3e} fp32 torch {e_g32:.3e}")
    assert torch.isfinite(xr.grad).all()
    assert e_v <= VALUE_CAP and e_l <= VALUE_CAP and e_g <= GRAD_CAP
    assert e_v <= 4 * e_v32
    assert e_l <= 4 * e_l32
    assert e_g <= 4 * e_g32


# ------------------------------------------------------------------------------------------ 2. one scale is the windowed SSIM

def test_one_scale_is_the_existing_ssim():
    from nerve_cl import metrics, ops
    x, y = images((2, 3, 37, 70), 21)
    up = torch.tensor([0.7, 1.3], device=dev())
    for reduction in ("none", "mean"):
        a = metrics.ms_ssim(x, y, weights=[1.0], reduction=reduction)
        b = metrics.ssim(x, y, reduction=reduction)
        assert a.shape == b.shape
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        la = ops.ms_ssim_loss(xa, y, weights=[1.0], reduction=reduction)
        lb = ops.ssim_loss(xb, y, reduction=reduction)
        (la * up).sum().backward()
        (lb * up).sum().backward()
        dv, dl, dg = (a - b).abs().max().item(), (la - lb).abs().max().item(), (xa.grad - xb.grad).abs().max().item()
        print(f"one scale {reduction}: value diff {dv:.3e} loss diff {dl:.3e} dx max diff {dg:.3e} (dx max {xb.grad.abs().max().item():.3e})")
        assert dv <= 1e-6 and dl <= 1e-6 and dg <= 1e-6
        assert xb.grad.abs().max().item() > 1e-5           # the comparison of the gradients is not one of zeros


# ------------------------------------------------------------------------------------------------------- 3. pooling alone

@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 64, 128), (1, 23, 27), (2, 3, 10, 12)], ids=str)
def test_pair_pooling_is_avg_pool2d(shape):
    from nerve_cl import _nvq
    g = torch.Generator().manual_seed(31)
    x, y = torch.rand(shape, generator=g).to(dev()), torch.rand(shape, generator=g).to(dev())
    out = (*shape[:-2], shape[-2] // 2, shape[-1] // 2)
    px, py = torch.full(out, float("nan"), device=dev()), torch.full(out, float("nan"), device=dev())
    _nvq.avgpool2_pair(x, y, px, py)
    for got, src in ((px, x), (py, y)):
        want = F.avg_pool2d(src.reshape(-1, 1, *shape[-2:]), 2).reshape(out)
        assert torch.isfinite(got).all()
        ulps = (got.view(torch.int32) - want.view(torch.int32)).abs().max().item()     # positive floats: ordered as integers
        assert ulps <= 1, ulps
        want64 = F.avg_pool2d(src.double().reshape(-1, 1, *shape[-2:]), 2).reshape(out)
        assert (got.double() - want64).abs().max().item() <= 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- 4. clamp

def test_a_clamped_term_gives_zero_and_a_zero_gradient():
    from nerve_cl import metrics, ops
    _, y = images((1, 3, 23, 27), 41)
    x = 1 - y
    w = std_weights(2)
    assert ms_ssim_ref(x, y, w).item() == 0.0             # the cs means are negative: float64 clamps them too
    for reduction in ("none", "mean"):
        assert metrics.ms_ssim(x, y, weights=w, reduction=reduction).abs().max().item() == 0.0
        xr = x.clone().requires_grad_(True)
        loss = ops.ms_ssim_loss(xr, y, weights=w, reduction=reduction)
        assert (loss == 1.0).all()
        loss.sum().backward()
        assert torch.isfinite(xr.grad).all()
        assert (xr.grad == 0).all()


# ---------------------------------------------------------------------------------------------------- 5. identical inputs

def test_identical_inputs():
    from nerve_cl import metrics, ops
    shape, M = (2, 3, 64, 128), 3
    r = reference(shape, M)
    y = r["y"]
    val = metrics.ms_ssim(y, y, weights=r["w"], reduction="none")
    assert (val - 1).abs().max().item() <= 1e-6
    xr = y.clone().requires_grad_(True)
    ops.ms_ssim_loss(xr, y, weights=r["w"]).backward()
    norm, ref_norm = xr.grad.double().norm().item(), r["g_mean64"].norm().item()
    print(f"identical inputs: value {val.tolist()} | dx norm {norm:.3e} against {ref_norm:.3e} of the perturbed prediction")
    assert torch.isfinite(xr.grad).all() and norm < 1e-4 * ref_norm


# --------------------------------------------------------------------------------------------------------- 6. determinism

def test_ms_ssim_is_deterministic():
    from nerve_cl import ops
    x, y = images((2, 3, 64, 128), 61)
    w = std_weights(3)

    def run():
        xr = x.clone().requires_grad_(True)
        v = ops.ms_ssim_loss(xr, y, weights=w, reduction="none")
        v.sum().backward()
        return v.detach().clone(), xr.grad.clone()

    first, second = run(), run()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        third = run()
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


# ---------------------------------------------------------------------------------------------------------------- 7. views

def test_views_give_the_result_of_their_contiguous_copies():
    from nerve_cl import metrics, ops
    w = std_weights(2)
    bx, by = images((2, 1, 23, 27), 71)                   # x[1:2] starts 621 floats in: contiguous, not 16-byte aligned
    wx, wy = images((2, 2, 24, 31), 72)                   # [..., 1:] is not contiguous
    for name, (vx, vy) in {"misaligned": (bx[1:2], by[1:2]), "strided": (wx[..., 1:], wy[..., 1:])}.items():
        if name == "misaligned":
            assert vx.is_contiguous() and vx.data_ptr() % 16 != 0
        else:
            assert not vx.is_contiguous()
        cx, cy = vx.clone(memory_format=torch.contiguous_format), vy.clone(memory_format=torch.contiguous_format)
        assert cx.is_contiguous() and cx.data_ptr() % 16 == 0
        assert torch.equal(metrics.ms_ssim(vx, vy, weights=w, reduction="none"), metrics.ms_ssim(cx, cy, weights=w, reduction="none"))
        base = (bx if name == "misaligned" else wx).clone().requires_grad_(True)
        view = base[1:2] if name == "misaligned" else base[..., 1:]
        leaf = cx.clone().requires_grad_(True)
        lv, lc = ops.ms_ssim_loss(view, vy, weights=w), ops.ms_ssim_loss(leaf, cy, weights=w)
        lv.backward()
        lc.backward()
        got = base.grad[1:2] if name == "misaligned" else base.grad[..., 1:]
        assert torch.equal(lv, lc) and torch.equal(got, leaf.grad), name
        assert leaf.grad.abs().max().item() > 0


def test_shapes_must_agree():
    from nerve_cl import ops
    a = torch.rand(2, 3, 44, 48, device=dev())
    with pytest.raises(RuntimeError, match="shapes differ"):
        ops.ms_ssim_loss(a, a[:1], weights=[0.5, 0.5])


# ------------------------------------------------------------------------------------------------------------- 8. training

@pytest.mark.parametrize("kind", ["ms_ssim", "ms_ssim_l1"])
def test_three_adamw_steps_lower_the_loss(kind):
    from nerve_cl import ops
    x, y = images((1, 3, 44, 89), 81)
    w = std_weights(3)
    fn = {"ms_ssim": ops.ms_ssim_loss, "ms_ssim_l1": ops.ms_ssim_l1_loss}[kind]
    img = x.clone().requires_grad_(True)
    opt = torch.optim.AdamW([img], lr=5e-3, weight_decay=0.0, fused=True)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = fn(img, y, weights=w)
        loss.backward()
        assert torch.isfinite(img.grad).all()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(fn(img, y, weights=w).item())
    print(f"{kind}: {losses}")
    assert all(b < a for a, b in zip(losses, losses[1:]))


def test_the_mix_is_the_sum_of_its_parts():
    from nerve_cl import ops
    x, y = images((2, 3, 44, 89), 82)
    w = std_weights(3)
    for reduction in ("none", "mean"):
        mix = ops.ms_ssim_l1_loss(x, y, weights=w, reduction=reduction)
        parts = 0.84 * ops.ms_ssim_loss(x, y, weights=w, reduction=reduction) + 0.16 * ops.l1_loss(x, y, reduction=reduction)
        assert mix.shape == parts.shape and (mix - parts).abs().max().item() <= 1e-6
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ops.ms_ssim_l1_loss(xa, y, alpha=0.5, weights=w).backward()
    (0.5 * ops.ms_ssim_loss(xb, y, weights=w) + 0.5 * ops.l1_loss(xb, y)).backward()
    assert (xa.grad - xb.grad).abs().max().item() <= 1e-6 * xb.grad.abs().max().item() + 1e-12
    m = ops.MSSSIMLoss(weights=w, reduction="none")(x, y)
    assert torch.equal(m, ops.ms_ssim_loss(x, y, weights=w, reduction="none"))
