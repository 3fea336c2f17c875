"""GPU: the deterministic warp backward (nvq_warp_backward_ex with NVQ_WARP_DETERMINISTIC) and the deterministic training
mode of SuperResolutionNet.

The kernel is checked against float64 autograd of the oracle's grid_sample warp, evaluated at the coordinates the kernel
itself computes in fp32 (so that a floor at a cell border cannot pick a different cell than the kernel's):
  * fp32 dfeat: rel < 5e-5 of the reference's max magnitude;
  * bf16 dfeat: EVERY element within  half a bf16 ulp of (|ref| + E)  +  E,  E = (k + 4) * 2^-24 * T,
    where k is the largest number of addends any destination receives and T the element's sum of |addend| before the
    weight: the bound of one fp32 sum of k products (plus a few ulps of the weights) rounded once to bf16.  The atomic
    form rounds after every far addend and breaks it when many far sources land on one pixel."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle import sr_oracle, synth

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    return _nvq


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def to_nhwc(x, ld=None, coff=0, dtype=torch.float32):
    n, c, h, w = x.shape
    buf = torch.zeros((n, h, w, ld or c), dtype=dtype)
    buf[..., coff:coff + c] = x.permute(0, 2, 3, 1).to(dtype)
    return buf.cuda()


def from_nhwc(buf, c=None, coff=0):
    c = buf.shape[-1] - coff if c is None else c
    return buf[..., coff:coff + c].permute(0, 3, 1, 2).double().cpu()


# ----------------------------------------------------------------------------- motion fields
def make_flow(case, N, H, W):
    g = torch.Generator().manual_seed(11)
    base = 0.5 * rnd(N, 2, H, W, seed=2)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    if case == "half_px":
        return base
    if case in ("far20", "far60"):
        frac, rmin, rmax = (0.2, 5.0, 8.0) if case == "far20" else (0.6, 4.5, 30.0)
        far = torch.rand(N, 1, H, W, generator=g) < frac
        ang = torch.rand(N, 1, H, W, generator=g) * 6.2831853
        r = rmin + (rmax - rmin) * torch.rand(N, 1, H, W, generator=g)   # up to 30 px: many leave the frame
        return base + torch.where(far, r, torch.zeros(())) * torch.cat([torch.cos(ang), torch.sin(ang)], 1)
    fl = base.clone()
    if case == "region_onto_point":
        # a 9 x 9 region moved >= 6 px onto one point (far: one bin, 81 addends on 4 pixels) and a 7 x 7 region contracted
        # onto a nearby point (near: more window sources per pixel than the hit list holds)
        ty, tx = H - 3.63, W - 4.29
        fl[:, 0, 1:10, 1:10] = tx - xs[..., 1:10]
        fl[:, 1, 1:10, 1:10] = ty - ys[:, 1:10]
        cy, cx = 5.31, W - 9.72
        ry, rx = slice(2, 9), slice(W - 13, W - 6)
        fl[:, 0, ry, rx] = cx - xs[..., rx] + 0.01 * base[:, 0, ry, rx]
        fl[:, 1, ry, rx] = cy - ys[:, ry] + 0.01 * base[:, 1, ry, rx]
        return fl
    if case == "all_onto_pixel":
        ty, tx = H / 2 + 0.37, W / 2 + 0.41
        fl[:, 0] = tx - xs + 0.001 * base[:, 0]
        fl[:, 1] = ty - ys + 0.001 * base[:, 1]
        return fl
    raise ValueError(case)


CASES = ["half_px", "far20", "far60", "region_onto_point", "all_onto_pixel"]


def kernel_coords(flow):
    """The sampling coordinates as the kernel computes them in fp32 (warp_geom), as a float64 flow for the oracle."""
    N, _, H, W = flow.shape
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    ix = ((2.0 * (xs + flow[:, 0]) / float(W - 1) - 1.0 + 1.0) / 2.0) * float(W - 1)
    iy = ((2.0 * (ys + flow[:, 1]) / float(H - 1) - 1.0 + 1.0) / 2.0) * float(H - 1)
    return torch.stack([ix.double() - xs.double(), iy.double() - ys.double()], 1)


def addend_stats(flow64, dy64):
    """Per destination element: T = sum of |dout| over its addends; k = the largest addend count of any destination."""
    N, C, H, W = dy64.shape
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    ix, iy = xs + flow64[:, 0], ys + flow64[:, 1]
    x0, y0 = ix.floor(), iy.floor()
    T = torch.zeros(N, H * W, C, dtype=torch.float64)
    cnt = torch.zeros(N, H * W, dtype=torch.float64)
    src = dy64.abs().permute(0, 2, 3, 1).reshape(N, H * W, C)
    for dy_, dx_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cx, cy = x0 + dx_, y0 + dy_
        w = (1 - (ix - cx).abs()) * (1 - (iy - cy).abs())
        ok = ((cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (w > 0)).reshape(N, H * W)
        dst = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long().reshape(N, H * W)
        for n in range(N):
            T[n].index_add_(0, dst[n][ok[n]], src[n][ok[n]])
            cnt[n].index_add_(0, dst[n][ok[n]], torch.ones(int(ok[n].sum()), dtype=torch.float64))
    return T.view(N, H, W, C).permute(0, 3, 1, 2), int(cnt.max().item())


def bf16_ulp(a):
    """ulp of bf16 at magnitude |a| (8 significant bits); subnormal range floored at the smallest normal's ulp."""
    e = torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def bf16_violations(got, ref, T, k):
    E = (k + 4) * U32 * T
    bound = 0.5 * bf16_ulp(ref.abs() + E) + E
    return int(((got - ref).abs() > bound).sum().item())


class Setup:
    def __init__(self, C, N, H, W, case, dout_bf16):
        self.C, self.N, self.H, self.W = C, N, H, W
        self.feat = rnd(N, C, H, W)
        self.flow = make_flow(case, N, H, W)
        dy = rnd(N, C, H, W, seed=4)
        if dout_bf16:
            dy = dy.bfloat16().float()                 # the kernel reads bf16: the reference gets the same values
        self.dy = dy
        flow64 = kernel_coords(self.flow)
        f64 = self.feat.double().requires_grad_()
        sr_oracle.warp(f64, flow64).backward(dy.double())
        self.ref = f64.grad
        self.T, self.k = addend_stats(flow64, dy.double())

    def run(self, K, feat_bf16, dout_bf16, dfeat_bf16, deterministic, images=None):
        C = self.C
        fd = torch.bfloat16 if feat_bf16 else torch.float32
        dd = torch.bfloat16 if dout_bf16 else torch.float32
        fb = to_nhwc(self.feat, dtype=fd)
        flb = to_nhwc(self.flow, 4)
        dal = to_nhwc(self.dy, 3 * C, 2 * C, dtype=dd)
        lo, hi = images or (0, self.N)
        dfeat = torch.full((hi - lo, self.H, self.W, C), float("nan"), device="cuda",
                           dtype=torch.bfloat16 if dfeat_bf16 else torch.float32)
        dflow = torch.full((hi - lo, self.H, self.W, 4), float("nan"), device="cuda")
        kw = {"deterministic": True} if deterministic else {}
        K.warp_backward(K.Sl(dal, C, 2 * C).images(lo, hi), K.Sl(fb).images(lo, hi), flb[lo:hi], K.Sl(dfeat), dflow,
                        overwrite=True, **kw)
        torch.cuda.synchronize()
        return dfeat, dflow


COMBOS = [(f, d, o) for f in (False, True) for d in (False, True) for o in (False, True)]


# ----------------------------------------------------------------------------- 1. kernel against float64
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("C", [16, 32, 64, 128])
def test_deterministic_warp_backward_against_float64(K, C, case):
    N, H, W = (2, 21, 45) if C <= 64 else (1, 19, 37)
    setups = {d: Setup(C, N, H, W, case, d) for d in (False, True)}
    for feat_bf16, dout_bf16, dfeat_bf16 in COMBOS:
        s = setups[dout_bf16]
        dfeat, dflow = s.run(K, feat_bf16, dout_bf16, dfeat_bf16, True)
        got = from_nhwc(dfeat)
        combo = (case, C, feat_bf16, dout_bf16, dfeat_bf16)
        assert torch.isfinite(got).all(), combo
        if dfeat_bf16:
            assert bf16_violations(got, s.ref, s.T, s.k) == 0, combo
        else:
            assert rel(got, s.ref) < 5e-5, combo
        _, dflow_atomic = s.run(K, feat_bf16, dout_bf16, dfeat_bf16, False)
        assert torch.equal(dflow, dflow_atomic), combo


def test_far_sources_are_present_in_the_far_cases():
    """The motion fields above do what their names say (checked on the kernel's own classification rule)."""
    N, H, W = 2, 21, 45
    for case, lo, hi in (("half_px", 0.0, 0.0), ("far20", 0.15, 0.25), ("far60", 0.4, 0.65)):
        fl = kernel_coords(make_flow(case, N, H, W))
        xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
        ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
        ox = (xs + fl[:, 0]).floor() - xs
        oy = (ys + fl[:, 1]).floor() - ys
        far = ((ox < -4) | (ox > 3) | (oy < -4) | (oy > 3)).double().mean().item()
        assert lo <= far <= hi, (case, far)


# ----------------------------------------------------------------------------- 2. near flows: nothing changes
@pytest.mark.parametrize("C", [16, 64, 128])
def test_near_flows_match_the_existing_form_bit_for_bit(K, C):
    s = Setup(C, 2, 21, 45, "half_px", False)
    for feat_bf16 in (False, True):
        for dout_bf16 in (False, True):
            d1, f1 = s.run(K, feat_bf16, dout_bf16, False, True)
            d0, f0 = s.run(K, feat_bf16, dout_bf16, False, False)
            assert torch.equal(d1, d0) and torch.equal(f1, f0), (feat_bf16, dout_bf16)


# ----------------------------------------------------------------------------- 3. reproducible, batch-independent
@pytest.mark.parametrize("case", ["far60", "all_onto_pixel"])
@pytest.mark.parametrize("dfeat_bf16", [False, True])
def test_reproducible_and_independent_of_the_batch(K, case, dfeat_bf16):
    s = Setup(64, 2, 21, 45, case, True)
    runs = [s.run(K, True, True, dfeat_bf16, True) for _ in range(3)]
    for d, f in runs[1:]:
        assert torch.equal(d, runs[0][0]) and torch.equal(f, runs[0][1])
    d1, f1 = s.run(K, True, True, dfeat_bf16, True, images=(1, 2))
    assert torch.equal(d1, runs[0][0][1:2]) and torch.equal(f1, runs[0][1][1:2])


def test_deterministic_mode_refuses_the_other_forms(K):
    s = Setup(16, 1, 9, 33, "far20", False)
    fb, flb, dal = to_nhwc(s.feat), to_nhwc(s.flow, 4), to_nhwc(s.dy)
    dfeat, dflow = torch.zeros_like(fb), torch.empty(1, 9, 33, 4, device="cuda")
    with pytest.raises(RuntimeError, match="deterministic mode exists for the gather form"):
        K.warp_backward(K.Sl(dal), K.Sl(fb), flb, K.Sl(dfeat), dflow, deterministic=True)                 # accumulate
    with pytest.raises(RuntimeError, match="deterministic mode exists for the gather form"):
        K.warp_backward(K.Sl(dal), K.Sl(fb), flb, K.Sl(dfeat), dflow, gather=False, overwrite=True, deterministic=True)


def test_warp_features_follows_the_torch_switch(K):
    from nerve_cl.models.super_resolution import warp_features
    s = Setup(32, 2, 21, 45, "far60", False)
    outs = []
    for det in (True, None):
        ctx = _torch_deterministic() if det is None else contextlib.nullcontext()
        with ctx:
            f = s.feat.cuda().requires_grad_()
            fl = s.flow.cuda().requires_grad_()
            warp_features(f, fl, deterministic=det).backward(s.dy.cuda())
            outs.append((f.grad.clone(), fl.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rel(outs[0][0], s.ref) < 5e-5


# ----------------------------------------------------------------------------- 4. whole training step
@contextlib.contextmanager
def _torch_deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


FC, NB, WIN, S, B, H, W = 16, 2, 1, 2, 2, 48, 80


def _far_net(bf16: bool):
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    sd = synth.formula_state(3, S, FC, NB, WIN, gain=synth.GOLDEN_GAIN)
    sd["motion_estimator.flow_net.6.bias"] = torch.zeros(2)
    net = SuperResolutionNet(3, S, FC, NB, WIN)
    net.load_state_dict(sd)
    net.math_mode = _nvq.MATH_BF16 if bf16 else _nvq.MATH_F32
    net.bf16_activations = bf16
    net = net.cuda().train()
    # the last flow conv scaled to ~1 px of spread (few sampling positions within rounding distance of a cell border, where
    # the flow gradient jumps) and its x bias at 4 px minus the median: about half of the sources land 4 px or more away
    x = synth.formula_clip(B, 2 * WIN + 1, H, W).cuda()
    with torch.no_grad():
        fx = net.motion_estimator(net.feature_extractor(x[:, 1]), net.feature_extractor(x[:, 0]))[:, 0].float()
    k = 1.0 / fx.std().clamp_min(1e-6).item()
    sd["motion_estimator.flow_net.6.weight"] = sd["motion_estimator.flow_net.6.weight"] * k
    sd["motion_estimator.flow_net.6.bias"] = torch.tensor([4.0 - k * fx.median().item(), -0.3])
    P = dict(net.named_parameters())
    with torch.no_grad():
        for n in ("weight", "bias"):
            P["motion_estimator.flow_net.6." + n].copy_(sd["motion_estimator.flow_net.6." + n])
    return net, sd


def _far_fraction(net, x):
    with torch.no_grad():
        f1 = net.feature_extractor(x[:, 1].cuda())
        f2 = net.feature_extractor(x[:, 0].cuda())
        flow = net.motion_estimator(f1, f2).double().cpu()
    _, _, h, w = flow.shape
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    ox = (xs + flow[:, 0]).floor() - xs
    oy = (ys + flow[:, 1]).floor() - ys
    inside = (xs + flow[:, 0] > -1) & (xs + flow[:, 0] < w) & (ys + flow[:, 1] > -1) & (ys + flow[:, 1] < h)
    return (((ox < -4) | (ox > 3) | (oy < -4) | (oy > 3)) & inside).double().mean().item()


def _step(net, x, tgt):
    net.zero_grad(set_to_none=True)
    out = net(x)
    F.mse_loss(out, tgt).backward()
    return out.detach().clone(), torch.cat([p.grad.flatten() for p in net.parameters()]).clone()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("how", ["attribute", "torch_switch"])
def test_training_step_is_bit_reproducible_with_far_motion(K, bf16, how):
    net, sd = _far_net(bf16)
    x = synth.formula_clip(B, 2 * WIN + 1, H, W).cuda()
    tgt = synth.formula_target(B, H * S, W * S).cuda()
    frac = _far_fraction(net, x)
    assert 0.2 <= frac <= 0.8, frac
    if how == "attribute":
        net.deterministic = True
        ctx = contextlib.nullcontext
    else:
        assert net.deterministic is None
        ctx = _torch_deterministic
    with ctx():
        o1, g1 = _step(net, x, tgt)
        o2, g2 = _step(net, x, tgt)
        assert torch.equal(o1, o2) and torch.equal(g1, g2)
        assert torch.isfinite(o1).all() and torch.isfinite(g1).all()
        # HIP-graph replay (captured on the third call of the shape, replayed on the fourth) == eager
        net.use_hip_graphs = True
        for _ in range(4):
            og, gg = _step(net, x, tgt)
        net.use_hip_graphs = False
        assert net._step_graphs.replays >= 2
        assert torch.equal(og, o1) and torch.equal(gg, g1)
    if not bf16:
        # against the oracle: with motion this far the existing (atomic) form itself is off the parity bound of
        # tests/test_sr_parity_gpu.py (up to ~1e-2 on the attention convs: the network's sensitivity at cell borders, not the
        # warp's summation), so the deterministic form is held to that bound or to the existing form's own distance, and to
        # 1e-3 of the existing form's gradients
        net.deterministic = False
        oa, ga = _step(net, x, tgt)
        ora = sr_oracle.OracleSR(3, S, FC, NB, WIN)
        ora.load_named(sd)
        ora.train()
        o_ref = ora(x.cpu())
        F.mse_loss(o_ref, tgt.cpu()).backward()
        onamed = ora.named()
        assert rel(o1, o_ref.detach()) < 1e-3 and rel(o1, oa) < 1e-5
        off = 0
        for n, p in net.named_parameters():
            k = p.numel()
            gd, gat = g1[off:off + k].view_as(p), ga[off:off + k].view_as(p)
            assert rel(gd, onamed[n].grad) <= max(1e-3, 1.01 * rel(gat, onamed[n].grad) + 1e-5), n
            assert rel(gd, gat) < 1e-3, n
            off += k


def test_training_step_with_ewc_and_fused_adam_under_the_torch_switch(K):
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "experiments"))
    from _common import make_optimizer
    from nerve_cl.continual import EWC
    x = synth.formula_clip(B, 2 * WIN + 1, H, W).cuda()
    tgt = synth.formula_target(B, H * S, W * S).cuda()
    results = []
    for _ in range(2):
        net, _ = _far_net(False)
        with _torch_deterministic():
            ewc = EWC(net, ewc_lambda=100.0)
            ewc.register_task(0, [(x, tgt)])                 # the Fisher pass: a backward too
            opt = make_optimizer(torch.optim.Adam, net.parameters(), lr=1e-3)
            for _ in range(2):
                opt.zero_grad(set_to_none=True)
                loss = F.mse_loss(net(x), tgt) + ewc.penalty()
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
        results.append(torch.cat([p.detach().flatten() for p in net.parameters()]))
    assert torch.isfinite(results[0]).all()
    assert torch.equal(results[0], results[1])


# ----------------------------------------------------------------------------- 5. default path unchanged
def test_default_mode_calls_the_existing_export(K, monkeypatch):
    lib = K.lib()
    calls = {"nvq_warp_backward": 0, "nvq_warp_backward_ex": 0}
    for name in calls:
        orig = getattr(lib, name)

        def spy(*a, _orig=orig, _name=name):
            calls[_name] += 1
            return _orig(*a)
        monkeypatch.setattr(lib, name, spy)
    net, _ = _far_net(False)
    x = synth.formula_clip(B, 2 * WIN + 1, H, W).cuda()
    tgt = synth.formula_target(B, H * S, W * S).cuda()
    assert not torch.are_deterministic_algorithms_enabled() and net.deterministic is None
    _step(net, x, tgt)
    assert calls["nvq_warp_backward"] > 0 and calls["nvq_warp_backward_ex"] == 0
    net.deterministic = True
    calls.update({k: 0 for k in calls})
    _step(net, x, tgt)
    assert calls["nvq_warp_backward_ex"] > 0 and calls["nvq_warp_backward"] == 0
