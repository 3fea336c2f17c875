"""GPU: the gradient w.r.t. the input frames of SuperResolutionNet, LightweightSuperResolution and the EnhancementEngine blend
(reference: plain nn.Modules, autograd reaches lr_frames through every layer), against CPU autograd through the pure-torch
oracle on the closed-form weights and clips of oracle/synth.py.  Also the two kernels behind it (nvq_head_dgrad,
nvq_bicubic_adjoint) on their own, determinism, the eager-only rule for HIP graphs, and that parameter gradients do not
depend on whether the input gradient was requested.
Tolerances: fp32 at 1e-3 of the reference tensor's max magnitude per frame (the REL of test_sr_parity_gpu.py); the bf16
throughput mode by relative L2 against a float64 oracle (bounds below, with the measured values beside them)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fr_oracle, sr_oracle, synth

pytestmark = pytest.mark.gpu
REL = 1e-3


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


def sr_pair(Fc, N, win, s, train, bf16=False):
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    sd = synth.formula_state(3, s, Fc, N, win, gain=synth.GOLDEN_GAIN)
    net = SuperResolutionNet(3, s, Fc, N, win)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    ora = sr_oracle.OracleSR(3, s, Fc, N, win)
    ora.load_named(sd)
    ora.train(train)
    return net, ora


def light_pair(s, train, bf16=False):
    from nerve_cl import _nvq
    from nerve_cl.models import LightweightSuperResolution
    sd = synth.formula_state_light(s, gain=synth.GOLDEN_GAIN)
    net = LightweightSuperResolution(s)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    P = {k: v.clone() for k, v in sd.items()}
    return net, P


def sr_input_grad(net, x, tgt, **kw):
    xg = x.cuda().requires_grad_()
    out = net(xg, **kw)
    out = out[0] if isinstance(out, tuple) else out
    F.mse_loss(out, tgt.cuda()).backward()
    return xg.grad


def oracle_input_grad(fwd, x, tgt):
    xo = x.clone().requires_grad_()
    F.mse_loss(fwd(xo), tgt.to(xo.dtype)).backward()
    return xo.grad


# ------------------------------------------------------------------ (1) SR net, exact-fp32 mode
@pytest.mark.parametrize("s,T,H,W,train", [
    (2, 3, 24, 40, True), (2, 5, 37, 53, False), (3, 3, 37, 53, True), (3, 5, 20, 28, False),
    (4, 3, 37, 53, False), (4, 5, 16, 24, True)])
def test_sr_input_grad_fp32_vs_oracle(s, T, H, W, train):
    win = T // 2
    net, ora = sr_pair(32, 2, win, s, train)
    x = synth.formula_clip(2, T, H, W)
    tgt = synth.formula_target(2, H * s, W * s)
    g = sr_input_grad(net, x, tgt)
    assert g is not None and g.shape == x.shape
    og = oracle_input_grad(ora, x, tgt)
    errs = [rel(g[:, t], og[:, t]) for t in range(T)]
    print(f"  SR fp32 s{s} T{T} {H}x{W} {'train' if train else 'eval'}: per-frame rel {['%.1e' % e for e in errs]}")
    assert max(errs) < REL, errs


def test_sr_input_grad_frozen_parameters_and_intermediates():
    """frozen parameters (input gradient only), return_intermediate=False, against return_intermediate=True with trainable
    parameters: the same input gradient, bit for bit"""
    x = synth.formula_clip(2, 3, 37, 53)
    tgt = synth.formula_target(2, 74, 106)
    net, ora = sr_pair(32, 2, 1, 2, True)
    g_inter = sr_input_grad(net, x, tgt, return_intermediate=True)
    net, _ = sr_pair(32, 2, 1, 2, True)
    for p in net.parameters():
        p.requires_grad_(False)
    g_frozen = sr_input_grad(net, x, tgt, return_intermediate=False)
    assert all(p.grad is None for p in net.parameters())
    assert torch.equal(g_inter, g_frozen)
    og = oracle_input_grad(ora, x, tgt)
    assert max(rel(g_frozen[:, t], og[:, t]) for t in range(3)) < REL
    # autograd.grad with respect to the frames alone
    net, _ = sr_pair(32, 2, 1, 2, True)
    xg = x.cuda().requires_grad_()
    (gx,) = torch.autograd.grad(F.mse_loss(net(xg), tgt.cuda()), xg)
    assert torch.equal(gx, g_inter)


def test_sr_input_grad_through_a_cast_and_a_preprocessing_stage():
    """the frames' gradient chains through the dtype cast / copy forward() makes and a trained stage in front of the net"""
    net, ora = sr_pair(16, 1, 1, 2, True)
    x = synth.formula_clip(1, 3, 24, 32)
    tgt = synth.formula_target(1, 48, 64)
    gain = torch.tensor(0.9, device="cuda", requires_grad=True)
    xd = x.double().cuda().requires_grad_()                  # float64 input: cast inside forward()
    F.mse_loss(net(xd * gain), tgt.cuda()).backward()
    xo = x.double().clone().requires_grad_()
    go = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    F.mse_loss(ora((xo * go).float()), tgt).backward()
    assert xd.grad is not None and xd.grad.dtype == torch.float64
    assert max(rel(xd.grad[:, t], xo.grad[:, t]) for t in range(3)) < REL
    assert abs(gain.grad.item() - go.grad.item()) < REL * abs(go.grad.item())


# ------------------------------------------------------------------ (2) SR net, bf16 throughput mode
# HIP-bf16 relative L2 distance of the input gradient from the float64 oracle: at most 4x the fp32 oracle's own distance plus
# this cap.  Measured on MI355X (fp32 oracle's own distance in brackets): 64x64 F32 N4 1.93e-1 (5.4e-6), 135x240 F64 N8
# 2.24e-1 (2.3e-4).  That is the bf16 mode's usual gradient accuracy (its parameter gradients sit at cosine ~0.98 to the
# oracle, test_real_size_gpu.py), not the new kernels': both take their bf16 operands at 1e-5 in test_head_dgrad_kernel,
# and the exact-fp32 mode gives the same input gradient to ~1e-5.
BF16_CAP = {(64, 32, 4): 0.30, (240, 64, 8): 0.33}


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("H,W,Fc,N", [(64, 64, 32, 4), (135, 240, 64, 8)])
def test_sr_input_grad_bf16_vs_float64(H, W, Fc, N):
    s, B = 2, 1
    net, ora = sr_pair(Fc, N, 1, s, True, bf16=True)
    x = synth.formula_clip(B, 3, H, W, seed=13)
    tgt = synth.formula_target(B, H * s, W * s, seed=14)
    g = sr_input_grad(net, x, tgt)
    og32 = oracle_input_grad(ora, x, tgt)
    og64 = oracle_input_grad(ora.double(), x.double(), tgt)
    e_hip, e_ora = rel_l2(g, og64), rel_l2(og32, og64)
    cap = BF16_CAP[(W, Fc, N)]
    print(f"  SR bf16 {H}x{W} F{Fc} N{N}: input-grad rel L2 vs float64: HIP {e_hip:.2e}, fp32 oracle {e_ora:.2e}")
    assert e_hip <= 4 * e_ora + cap


# ------------------------------------------------------------------ (3) LightweightSuperResolution
@pytest.mark.parametrize("s,H,W,train", [(2, 37, 53, True), (3, 24, 40, False), (4, 37, 53, True), (2, 16, 16, False)])
def test_light_input_grad_fp32_vs_oracle(s, H, W, train):
    net, P = light_pair(s, train)
    x = synth.formula_clip(2, 1, H, W)[:, 0].contiguous()
    tgt = synth.formula_target(2, H * s, W * s)
    g = sr_input_grad(net, x, tgt)
    og = oracle_input_grad(lambda v: sr_oracle.light_forward(P, v, train), x, tgt)
    e = rel(g, og)
    print(f"  light fp32 s{s} {H}x{W}: rel {e:.1e}")
    assert e < REL


LIGHT_BF16_CAP = 0.40          # measured on MI355X: 2.65e-1 (fp32 oracle 3.6e-3)


def test_light_input_grad_bf16_vs_float64():
    net, P = light_pair(2, True, bf16=True)
    x = synth.formula_clip(2, 1, 64, 64)[:, 0].contiguous()
    tgt = synth.formula_target(2, 128, 128)
    g = sr_input_grad(net, x, tgt)
    og32 = oracle_input_grad(lambda v: sr_oracle.light_forward(P, v, True), x, tgt)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    og64 = oracle_input_grad(lambda v: sr_oracle.light_forward(P64, v, True), x.double(), tgt)
    e_hip, e_ora = rel_l2(g, og64), rel_l2(og32, og64)
    print(f"  light bf16 64x64: input-grad rel L2 vs float64: HIP {e_hip:.2e}, fp32 oracle {e_ora:.2e}")
    assert e_hip <= 4 * e_ora + LIGHT_BF16_CAP


# ------------------------------------------------------------------ (4) the strength < 1 blend
def test_engine_blend_input_grad():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    s, Fc, N = 2, 32, 2
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, scale_factor=s, sr_num_features=Fc,
                                              sr_num_residual_blocks=N))
    sd = synth.formula_state(3, s, Fc, N, 1, gain=synth.GOLDEN_GAIN)
    eng.super_resolution.load_state_dict(sd, strict=True)
    eng = eng.cuda().train()
    x = synth.formula_clip(2, 3, 37, 53)
    tgt = synth.formula_target(2, 74, 106)
    xg = x.cuda().requires_grad_()
    res = eng(xg, enhancement_strength=0.5)
    F.mse_loss(res["enhanced"], tgt.cuda()).backward()
    P = {k: v.clone() for k, v in sd.items()}
    xo = x.clone().requires_grad_()
    o = 0.5 * sr_oracle.sr_forward(P, xo, True) + 0.5 * sr_oracle.bicubic_up(xo[:, 1], s)
    F.mse_loss(o, tgt).backward()
    errs = [rel(xg.grad[:, t], xo.grad[:, t]) for t in range(3)]
    print(f"  blend: per-frame rel {['%.1e' % e for e in errs]}")
    assert max(errs) < REL, errs
    # strength < 1 with frames that need no gradient: nothing changes for them
    res = eng(x.cuda(), enhancement_strength=0.5)
    F.mse_loss(res["enhanced"], tgt.cuda()).backward()


# ------------------------------------------------------------------ (5) engine training through the lightweight net
def test_engine_trains_frame_recovery_through_lightweight_sr():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    base, s, B, T, H, W = 16, 2, 2, 5, 32, 48
    eng = EnhancementEngine(EnhancementConfig(use_lightweight_sr=True, recovery_base_channels=base, scale_factor=s))
    sd_fr = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN)
    sd_l = synth.formula_state_light(s, gain=synth.GOLDEN_GAIN)
    eng.frame_recovery.load_state_dict(sd_fr, strict=True)
    eng.super_resolution.load_state_dict(sd_l, strict=True)
    eng = eng.cuda().train()
    clip = synth.formula_clip(B, T, H, W)
    mask = torch.zeros(B, 1, H, W)
    mask[:, :, 8:24, 12:36] = 1.0
    tgt = synth.formula_target(B, H * s, W * s)
    res = eng(clip.cuda(), corruption_mask=mask.cuda())
    assert set(res) == {"recovered", "super_resolved", "enhanced"}
    F.mse_loss(res["enhanced"], tgt.cuda()).backward()
    Pfr = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd_fr.items()}
    Pl = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd_l.items()}
    refs = clip[:, [0, 1, 3, 4]]

    def chain(Pf, Pli, dt):
        rec = fr_oracle.frame_recovery_forward(Pf, clip[:, 2].to(dt), refs.to(dt), mask.to(dt), True)
        F.mse_loss(sr_oracle.light_forward(Pli, rec, True), tgt.to(dt)).backward()

    chain(Pfr, Pl, torch.float32)
    # float64 oracle: attributes a tensor over 1e-3 of the fp32 oracle (the rule of test_real_size_gpu.py: HIP at most 4x as far
    # from float64 as the fp32 CPU oracle itself, + 2e-5)
    d64 = lambda sd: {k: (v.double().requires_grad_(v.is_floating_point() and "running" not in k) if v.is_floating_point()
                          else v.clone()) for k, v in sd.items()}
    Pfr64, Pl64 = d64(sd_fr), d64(sd_l)
    chain(Pfr64, Pl64, torch.float64)
    worst, n_fr, listed = 0.0, 0, []
    for mod, P32, P64 in ((eng.frame_recovery, Pfr, Pfr64), (eng.super_resolution, Pl, Pl64)):
        for n, p in mod.named_parameters():
            assert p.grad is not None, n
            e = rel(p.grad, P32[n].grad)
            worst = max(worst, e)
            if e >= REL:
                t = P64[n].grad
                hip, ora = rel(p.grad, t), rel(P32[n].grad, t)
                listed.append((n, f"{e:.1e}", f"{hip:.1e}", f"{ora:.1e}"))
                assert hip <= 4 * ora + 2e-5, (n, e, hip, ora)
            n_fr += mod is eng.frame_recovery
    print(f"  engine: {n_fr} frame_recovery gradients, worst rel {worst:.1e}; attributed with float64 "
          f"(name, vs fp32, HIP vs f64, fp32 oracle vs f64): {listed}")
    # (this chain is ill-conditioned in fp32: BatchNorm over 32x48 images; the fp32 CPU oracle itself sits ~1e-2 from float64
    # on most frame_recovery tensors, so most of them are attributed rather than compared at 1e-3)
    assert n_fr == 117


# ------------------------------------------------------------------ (6) the kernels
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_bicubic_adjoint_kernel(s, masked):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(s)
    for H in (2, 3, 17, 135):
        for W in (2, 3, 17, 135):
            B, C, T, tc = 2, 3, 3, 1
            g = torch.randn(B, C, H * s, W * s, generator=gen)
            pm = (torch.rand(B, C, H * s, W * s, generator=gen) > 0.3).to(torch.uint8) if masked else None
            # fp32, like the forward: the tap weights are the fp32 ones (a float64 evaluation moves the s = 3 taps by 1e-6)
            xr = torch.zeros(B, C, H, W, requires_grad=True)
            up = F.interpolate(xr, scale_factor=float(s), mode="bicubic", align_corners=False)
            (ref,) = torch.autograd.grad(up, xr, g * (pm.float() if masked else 1.0))
            base = torch.randn(B, T, C, H, W, generator=gen)
            d = base.clone().cuda()
            _nvq.bicubic_adjoint(g.cuda(), pm.cuda() if masked else None, s, tc, 0.75, d)
            dd = d.cpu()
            assert torch.equal(dd[:, 0], base[:, 0]) and torch.equal(dd[:, 2], base[:, 2])    # other frames untouched
            e = rel(dd[:, tc], 0.75 * ref)
            assert e <= 1e-5, (H, W, e)
            d2 = d.clone()
            _nvq.bicubic_adjoint(g.cuda(), pm.cuda() if masked else None, s, tc, 0.75, d2, accumulate=True)
            assert rel(d2[:, tc].cpu() - dd[:, tc], dd[:, tc]) <= 1e-5
            d3 = base.clone().cuda()
            _nvq.bicubic_adjoint(g.cuda(), pm.cuda() if masked else None, s, tc, 0.75, d3)
            assert torch.equal(d3, d)                                                       # deterministic


@pytest.mark.parametrize("form", ["bf16_premasked", "fp32_dout2", "fp32_nodout2"])
@pytest.mark.parametrize("Fc", [16, 32, 64])
@pytest.mark.parametrize("Cin", [1, 3])
def test_head_dgrad_kernel(Cin, Fc, form):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(Cin * 100 + Fc)
    B, T, H, W = 2, 3, 19, 45
    slots = [1, 0, 2]
    NI = len(slots) * B
    ld = Fc + 16 if form == "fp32_dout2" else Fc
    w = torch.randn(Fc, Cin, 3, 3, generator=gen)
    dout = torch.randn(NI, H, W, ld, generator=gen)
    if form == "bf16_premasked":
        dout = dout.to(torch.bfloat16)
        act, dout2 = None, None
        gm = dout.float()[..., :Fc]
    else:
        act = torch.randn(NI, H, W, Fc, generator=gen).to(torch.bfloat16 if Fc == 32 else torch.float32)
        dout2 = torch.randn(NI, H, W, Fc, generator=gen) if form == "fp32_dout2" else None
        gm = dout[..., :Fc] + (dout2 if dout2 is not None else 0.0)
        gm = gm * (act.float() > 0)
    din = torch.nn.grad.conv2d_input((NI, Cin, H, W), w.double(), gm.permute(0, 3, 1, 2).double(), padding=1)
    ref = torch.empty(B, T, Cin, H, W, dtype=torch.float64)
    for j, t in enumerate(slots):
        ref[:, t] = din[j * B:(j + 1) * B]
    out = torch.full((B, T, Cin, H, W), float("nan"), device="cuda")
    c = lambda t: t.cuda() if t is not None else None
    _nvq.head_dgrad(c(dout), w.cuda(), B, slots, out, act=c(act), dout2=c(dout2))
    e = rel(out, ref)
    assert e <= 1e-5, e
    again = torch.ones_like(out)
    _nvq.head_dgrad(c(dout), w.cuda(), B, slots, again, act=c(act), dout2=c(dout2), accumulate=True)
    assert rel(again - 1.0, ref) <= 1e-5
    out2 = torch.empty_like(out)
    _nvq.head_dgrad(c(dout), w.cuda(), B, slots, out2, act=c(act), dout2=c(dout2))
    assert torch.equal(out, out2)


@pytest.mark.parametrize("bf16", [False, True])
def test_sr_input_grad_deterministic(bf16):
    x = synth.formula_clip(2, 3, 48, 64)
    tgt = synth.formula_target(2, 96, 128)
    grads = []
    for _ in range(2):
        net, _ = sr_pair(64, 2, 1, 2, True, bf16=bf16)
        net.deterministic = True
        grads.append(sr_input_grad(net, x, tgt))
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------------ (7) unchanged behaviour
@pytest.mark.parametrize("bf16", [False, True])
def test_parameter_grads_do_not_depend_on_the_input_grad(bf16):
    x = synth.formula_clip(2, 3, 48, 64)
    tgt = synth.formula_target(2, 96, 128)
    runs = []
    for want in (False, True):
        net, _ = sr_pair(64, 2, 1, 2, True, bf16=bf16)
        net.deterministic = True
        xc = x.cuda().requires_grad_(want)
        F.mse_loss(net(xc), tgt.cuda()).backward()
        assert (xc.grad is not None) == want
        runs.append({n: p.grad.clone() for n, p in net.named_parameters()})
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n


def test_hip_graphs_step_runs_eagerly_when_frames_need_grad():
    x = synth.formula_clip(2, 3, 24, 32)
    tgt = synth.formula_target(2, 48, 64)
    net, _ = sr_pair(32, 1, 1, 2, True)
    net.deterministic = True
    ref = sr_input_grad(net, x, tgt)
    net.use_hip_graphs = True
    for _ in range(4):                                        # past the graph warm-up: still no graph for this step
        g = sr_input_grad(net, x, tgt)
        assert torch.equal(g, ref)
    assert len(net._step_graphs.entries) == 0
