"""GPU: frozen layers in SuperResolutionNet / LightweightSuperResolution.  With some parameters frozen
(requires_grad False) the backward forms only the planned gradients, and each of them - and the frames' gradient - is
bit-identical to the all-trainable backward's; frozen .grad stays None.  Also: which kernels run (launch audit), the _ex entry
points against their full forms, HIP graphs with requires_grad toggled between steps, the data-parallel bucket, determinism."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


PATTERNS = {
    # name: (frozen-parameter predicate, frames need a gradient)
    "P1": (lambda n: False, True),
    "P2": (lambda n: n.startswith(("feature_extractor.", "motion_estimator.")), False),
    "P3": (lambda n: not n.startswith(("gff.", "upsampler.")), True),
    "P4": (lambda n: True, True),
    "P5": (lambda n: n.startswith("residual_blocks."), True),
    "P6": (lambda n: re.match(r"feature_extractor\.body\.\d\.bn\.", n) is not None, True),
    "motion_frozen": (lambda n: n.startswith("motion_estimator."), False),
}


def make_net(bf16, train, Fc=64, NB=2, win=1, s=2):
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    sd = synth.formula_state(3, s, Fc, NB, win, gain=synth.GOLDEN_GAIN)
    net = SuperResolutionNet(3, s, Fc, NB, win)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    net.deterministic = True
    return net


def step(net, x, tgt, pattern):
    frozen, frames_grad = PATTERNS[pattern]
    for n, p in net.named_parameters():
        p.requires_grad_(not frozen(n))
        p.grad = None
    xg = x.clone().requires_grad_(frames_grad)
    out = net(xg)
    F.mse_loss(out, tgt).backward()
    return {n: (p.grad.clone() if p.grad is not None else None) for n, p in net.named_parameters()}, xg.grad


def clip(B=2, T=3, H=24, W=40, s=2):
    return synth.formula_clip(B, T, H, W).cuda(), synth.formula_target(B, H * s, W * s).cuda()


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pattern", ["P2", "P3", "P4", "P5", "P6", "motion_frozen"])
def test_bit_identical_to_all_trainable(pattern, bf16, train):
    net = make_net(bf16, train)
    x, tgt = clip()
    ref, ref_dx = step(net, x, tgt, "P1")
    got, got_dx = step(net, x, tgt, pattern)
    frozen, frames_grad = PATTERNS[pattern]
    for n, g in got.items():
        if frozen(n):
            assert g is None, n
        else:
            assert g is not None and bits_equal(g, ref[n]), n
    if frames_grad:
        assert bits_equal(got_dx, ref_dx)
    else:
        assert got_dx is None


def test_light_bit_identical():
    from nerve_cl import _nvq
    from nerve_cl.models import LightweightSuperResolution
    net = LightweightSuperResolution(2)
    net.load_state_dict(synth.formula_state_light(2, gain=synth.GOLDEN_GAIN), strict=True)
    net = net.cuda().train()
    net.math_mode, net.bf16_activations = _nvq.MATH_BF16, True
    x = synth.formula_clip(2, 1, 24, 40)[:, 0].cuda()
    tgt = synth.formula_target(2, 48, 80).cuda()

    def run(frozen, xgrad):
        for n, p in net.named_parameters():
            p.requires_grad_(not frozen(n))
            p.grad = None
        xg = x.clone().requires_grad_(xgrad)
        F.mse_loss(net(xg), tgt).backward()
        return {n: p.grad for n, p in net.named_parameters()}, xg.grad
    ref, rdx = run(lambda n: False, True)
    for frozen in (lambda n: n.startswith(("net.2.", "net.3.")), lambda n: True, lambda n: not n.startswith("net.6.")):
        got, gdx = run(frozen, True)
        assert bits_equal(gdx, rdx)
        for n, g in got.items():
            assert (g is None) if frozen(n) else bits_equal(g, ref[n]), n


# ------------------------------------------------------------------ launch audit
WGRAD_ONLY = ("conv_wgrad", "head_wgrad", "dwconv_wgrad", "wgrad_reduce_batch")


def audit(monkeypatch, pattern, bf16=True):
    from nerve_cl import _nvq
    calls = {}
    wgrad_side = []

    def wrap(name):
        orig = getattr(_nvq, name)

        def f(*a, **kw):
            if name != "wgrad_reduce_batch" or a[0]:         # (an empty reduce queue launches nothing)
                calls[name] = calls.get(name, 0) + 1
            side = {"pw_bn_backward": lambda: a[13] is not None or a[11] is not None or a[12] is not None,
                    "dwconv_backward": lambda: a[5] is not None,
                    "cbam_bwd_spatial_conv": lambda: a[4] is not None,
                    "cbam_bwd_channel": lambda: a[11] is not None or a[12] is not None}.get(name)
            if side is not None and side():
                wgrad_side.append(name)
            return orig(*a, **kw)
        monkeypatch.setattr(_nvq, name, f)
    for name in ("correlation_backward", "warp_backward", "pw_bn_backward", "dwconv_backward", "head_wgrad", "head_dgrad",
                 "conv_wgrad", "dwconv_wgrad", "wgrad_reduce_batch", "cbam_bwd_spatial_conv", "cbam_bwd_channel",
                 "bn_relu_backward"):
        wrap(name)
    net = make_net(bf16, True)
    x, tgt = clip()
    step(net, x, tgt, pattern)
    return calls, wgrad_side


def test_launch_audit_p2(monkeypatch):
    calls, _ = audit(monkeypatch, "P2")
    for name in ("correlation_backward", "warp_backward", "pw_bn_backward", "dwconv_backward", "head_wgrad", "head_dgrad",
                 "dwconv_wgrad", "bn_relu_backward"):
        assert calls.get(name, 0) == 0, (name, calls)
    assert calls.get("conv_wgrad", 0) > 0


def test_launch_audit_p4(monkeypatch):
    calls, side = audit(monkeypatch, "P4")
    for name in WGRAD_ONLY:
        assert calls.get(name, 0) == 0, (name, calls)
    assert side == []
    assert calls.get("head_dgrad", 0) == 1 and calls.get("pw_bn_backward", 0) == 3


# ------------------------------------------------------------------ the _ex kernels against their full forms
def _intercept(monkeypatch, fname, index, sentinel):
    """replace the weight-gradient pointer argument of lib().<fname> by the sentinel's address"""
    from nerve_cl import _nvq
    lib = _nvq.lib()
    orig = getattr(lib, fname)
    seen = []

    def f(*a):
        a = list(a)
        a[index] = ctypes.c_void_p(sentinel.data_ptr())
        seen.append(a[-2])
        return orig(*a)
    monkeypatch.setattr(lib, fname, f)
    return seen


def nan_like(t):
    return torch.full_like(t, float("nan"))


@pytest.mark.parametrize("dy_bf16", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_pw_bn_backward_ex(monkeypatch, dy_bf16, training):
    from nerve_cl import _engine, _nvq
    g = torch.Generator().manual_seed(1)
    N, H, W, T = 6, 19, 45, 3
    dev = "cuda"
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    dy = r(N, H, W, 64).to(torch.bfloat16 if dy_bf16 else torch.float32)
    p, d = r(N, H, W, 64).bfloat16(), r(N, H, W, 64).bfloat16()
    mean, invstd = r(T, 64) * 0.1, r(T, 64).abs() + 0.5
    gamma, beta, wt = r(64), r(64) * 0.1, r(64, 64, 1, 1) * 0.1
    ws = _engine.workspace(torch.device(dev))
    dd0, dg0, db0, dw0 = torch.empty_like(p), torch.empty(64, device=dev), torch.empty(64, device=dev), torch.empty(64, 64, 1, 1, device=dev)
    _nvq.pw_bn_backward(dy, p, d, N // T, mean, invstd, gamma, beta, training, wt, dd0, dg0, db0, dw0, ws)
    # frozen BatchNorm affine, trained pointwise weight: dd and dweight unchanged
    dd1, dw1 = torch.empty_like(p), torch.empty_like(dw0)
    _nvq.pw_bn_backward(dy, p, d, N // T, mean, invstd, gamma, beta, training, wt, dd1, None, None, dw1, ws)
    assert torch.equal(dd1.view(torch.int16), dd0.view(torch.int16)) and bits_equal(dw1, dw0)
    # NVQ_NO_WGRAD: dd alone, a NaN dweight sentinel is not touched
    sent = nan_like(dw0)
    seen = _intercept(monkeypatch, "nvq_pw_bn_backward_ex", 21, sent)
    dd2 = torch.empty_like(p)
    _nvq.pw_bn_backward(dy, p, d, N // T, mean, invstd, gamma, beta, training, wt, dd2, None, None, None, ws)
    torch.cuda.synchronize()
    assert seen == [_nvq.NO_WGRAD]
    assert torch.equal(dd2.view(torch.int16), dd0.view(torch.int16))
    assert torch.isnan(sent).all()


@pytest.mark.parametrize("with_bn", [True, False])
def test_dwconv_backward_ex(monkeypatch, with_bn):
    from nerve_cl import _engine, _nvq
    g = torch.Generator().manual_seed(2)
    N, H, W, T = 6, 21, 70, 3
    dev = "cuda"
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, dy = r(N, H, W, 64).bfloat16(), r(N, H, W, 64).bfloat16()
    wt = r(64, 1, 3, 3)
    bn = (r(T, 64) * 0.1, r(T, 64).abs() + 0.5, r(64), r(64) * 0.1, N // T) if with_bn else None
    ws = _engine.workspace(torch.device(dev))
    dx0, dw0 = torch.empty_like(x), torch.empty(64, 1, 3, 3, device=dev)
    _nvq.dwconv_backward(x, bn, dy, wt, dx0, dw0, ws)
    sent = nan_like(dw0)
    seen = _intercept(monkeypatch, "nvq_dwconv_backward_ex", 12, sent)
    dx1 = torch.empty_like(x)
    _nvq.dwconv_backward(x, bn, dy, wt, dx1, None, ws)
    torch.cuda.synchronize()
    assert seen == [_nvq.NO_WGRAD]
    assert torch.equal(dx1.view(torch.int16), dx0.view(torch.int16))
    assert torch.isnan(sent).all()


@pytest.mark.parametrize("form", ["epilogue", "bn + epilogue", "bn + sums"])
def test_dwconv_backward_ex_other_forms(form):
    """NVQ_NO_WGRAD with the add / mask epilogue (without and with the BatchNorm input) and with the BatchNorm-backward sums:
    dw_bwd_kernel<., ., ., false> forms 1, 3 and 4 give the bits of the forms with the weight gradient"""
    from nerve_cl import _engine, _nvq
    g = torch.Generator().manual_seed(4)
    N, H, W, T = 6, 21, 70, 3
    dev = "cuda"
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, dy = r(N, H, W, 64).bfloat16(), r(N, H, W, 64).bfloat16()
    wt = r(64, 1, 3, 3)
    bn = (r(T, 64) * 0.1, r(T, 64).abs() + 0.5, r(64), r(64) * 0.1, N // T) if form != "epilogue" else None
    kw = [dict(), dict()]
    if form == "bn + sums":
        for k in kw:
            k.update(bn_sums=torch.zeros(T, 2, 64, device=dev), bn_dgamma=torch.zeros(64, device=dev),
                     bn_dbeta=torch.zeros(64, device=dev))
    else:
        add, mask = r(N, H, W, 64), r(N, H, W, 64).bfloat16()
        for k in kw:
            k.update(add=add, mask=mask)
    ws = _engine.workspace(torch.device(dev))
    dx0, dw0, dx1 = torch.empty_like(x), torch.empty(64, 1, 3, 3, device=dev), torch.empty_like(x)
    _nvq.dwconv_backward(x, bn, dy, wt, dx0, dw0, ws, **kw[0])
    _nvq.dwconv_backward(x, bn, dy, wt, dx1, None, ws, **kw[1])
    assert torch.equal(dx1.view(torch.int16), dx0.view(torch.int16))
    for name in kw[0]:
        if name.startswith("bn_"):
            assert bits_equal(kw[1][name], kw[0][name]) and kw[0][name].abs().max().item() > 0, name


def test_cbam_ex(monkeypatch):
    from nerve_cl import _engine, _nvq
    g = torch.Generator().manual_seed(3)
    B, H, W, Fc = 3, 37, 53, 64
    R = Fc // 16
    dev = "cuda"
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    ws = _engine.workspace(torch.device(dev))
    dpre, sm, w7 = r(B, H, W), r(B, H, W, 2), r(1, 2, 7, 7)
    dsm0, dw70 = torch.empty(B, H, W, 2, device=dev), torch.empty(1, 2, 7, 7, device=dev)
    _nvq.cbam_bwd_spatial_conv(dpre, sm, w7, dsm0, dw70, ws)
    nblk = _nvq.tsum_blocks(H, W)
    dca, w1, w2 = r(B, nblk, Fc), r(R, Fc) * 0.2, r(Fc, R) * 0.2
    gap, hid, ca = r(B, Fc), r(B, R).relu(), torch.rand(B, Fc, generator=g).to(dev)
    dgap0, d10, d20 = torch.empty(B, Fc, device=dev), torch.empty(R, Fc, device=dev), torch.empty(Fc, R, device=dev)
    _nvq.cbam_bwd_channel(dca, nblk, Fc, R, B, H * W, w1, w2, gap, hid, ca, d10, d20, dgap0)
    s7 = nan_like(dw70)
    seen7 = _intercept(monkeypatch, "nvq_cbam_bwd_spatial_conv_ex", 7, s7)
    dsm1 = torch.empty_like(dsm0)
    _nvq.cbam_bwd_spatial_conv(dpre, sm, w7, dsm1, None, ws)
    s1, s2 = nan_like(d10), nan_like(d20)
    from nerve_cl import _nvq as K
    lib = K.lib()
    orig = lib.nvq_cbam_bwd_channel_ex

    def chan(*a):
        a = list(a)
        a[11], a[12] = ctypes.c_void_p(s1.data_ptr()), ctypes.c_void_p(s2.data_ptr())
        return orig(*a)
    monkeypatch.setattr(lib, "nvq_cbam_bwd_channel_ex", chan)
    dgap1 = torch.empty_like(dgap0)
    _nvq.cbam_bwd_channel(dca, nblk, Fc, R, B, H * W, w1, w2, gap, hid, ca, None, None, dgap1)
    torch.cuda.synchronize()
    assert seen7 == [_nvq.NO_WGRAD]
    assert bits_equal(dsm1, dsm0) and bits_equal(dgap1, dgap0)
    assert torch.isnan(s7).all() and torch.isnan(s1).all() and torch.isnan(s2).all()


# ------------------------------------------------------------------ graphs, data parallelism, determinism
def test_graphs_requires_grad_toggle():
    x, tgt = clip(8, 3, 64, 64)
    eager = make_net(True, True)
    graphed = make_net(True, True)
    graphed.use_hip_graphs = True
    for pattern, entries in (("P1", 1), ("P2", 2), ("P3", 3), ("P2", 3), ("P1", 3)):
        frozen = PATTERNS[pattern][0]
        for _ in range(4):
            for n, p in graphed.named_parameters():
                p.requires_grad_(not frozen(n))
                p.grad = None
            F.mse_loss(graphed(x), tgt).backward()
        got = {n: p.grad for n, p in graphed.named_parameters()}
        for n, p in eager.named_parameters():
            p.requires_grad_(not frozen(n))
            p.grad = None
        F.mse_loss(eager(x), tgt).backward()
        for n, p in eager.named_parameters():
            if frozen(n):
                assert got[n] is None, (pattern, n)
            else:
                assert bits_equal(got[n], p.grad), (pattern, n)
        # a new need mask captures an entry of its own; a mask seen before replays its entry
        assert len(graphed._step_graphs.entries) == entries, pattern
    assert graphed._step_graphs.replays > 0


def test_bucket_hook_sees_only_trained_data():
    net = make_net(True, True)
    x, tgt = clip()
    seen = []
    net._grad_bucket_hook = lambda flat: seen.append(flat.clone())
    grads, _ = step(net, x, tgt, "P3")
    assert len(seen) == 1
    lay, total = net._bucket_layout()
    flat = seen[0]
    mask = torch.zeros(total, dtype=torch.bool, device=flat.device)
    for n, (o, k) in lay.items():
        if grads[n] is not None:
            mask[o:o + k] = True
            assert bits_equal(flat[o:o + k], grads[n].reshape(-1)), n
    assert torch.count_nonzero(flat[~mask]).item() == 0         # frozen slots and padding: zeros, never stale memory
    seen.clear()
    step(net, x, tgt, "P4")
    assert seen == []


def test_deterministic_p2():
    net = make_net(True, True)
    x, tgt = clip()
    a, _ = step(net, x, tgt, "P2")
    b, _ = step(net, x, tgt, "P2")
    for n in a:
        assert (a[n] is None and b[n] is None) or bits_equal(a[n], b[n]), n
