"""GPU: the gradient w.r.t. FrameRecoveryNet's image inputs (corrupted frame, reference frames, corruption mask; reference:
a plain nn.Module, autograd reaches all three), against CPU autograd through the pure-torch oracle (oracle/fr_oracle.py) on
the closed-form weights of oracle/synth.py.  Also the three kernels behind it (nvq_stem7_dgrad, nvq_mask_blend_backward_ex,
nvq_head_dgrad_tc) on their own, frozen parameters, determinism, that parameter gradients do not depend on whether the
input gradient was requested, and the EnhancementEngine's clip gradient through the recovery branch.
Tolerances: fp32 at 1e-3 of the reference tensor's max magnitude.  Where BatchNorm in training mode makes the step
ill-conditioned in fp32, the tensor is attributed with float64: the rule of test_real_size_gpu.py (HIP at most 4x as far
from float64 as the fp32 oracle, + 2e-5), or - where the CPU oracle happens to be much closer to float64 than the HIP
network's own parameter gradients are - HIP's input gradient no farther from float64 (relative L2) than twice the weight
gradient of the layer it leaves through (stem / conv1.spatial), which the existing parity tests accept; a relative-L2 cap of
1e-2 always.  The bf16 mode by relative L2 and cosine against float64 (bounds below, measured values beside them)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fr_oracle, sr_oracle, synth

pytestmark = pytest.mark.gpu
REL = 1e-3
L2_CAP = 1e-2


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def cosine(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


def fr_net(base, T, train, tic=True, bf16=None):
    """bf16: None = exact fp32, else bf16 MFMA operands with bf16_activations = bf16"""
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet
    sd = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN)
    net = FrameRecoveryNet(3, base, T)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    net.time_in_channels = tic
    if bf16 is None:
        net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    else:
        net.math_mode, net.bf16_activations = _nvq.MATH_BF16, bf16
    return net, sd


def soft_inputs(B, T, H, W, seed=5):
    """a clip, and a soft mask with values in (0.05, 0.95) (exercises the blend and dmask everywhere)"""
    clip = synth.formula_clip(B, T + 1, H, W, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=gen)
    return clip[:, 0].contiguous(), clip[:, 1:].contiguous(), mask, synth.formula_target(B, H, W, seed=seed + 1)


def hip_input_grads(net, frame, refs, mask, tgt, want=(True, True, True)):
    xs = [t.cuda().requires_grad_(w) for t, w in zip((frame, refs, mask), want)]
    out = net(*xs)
    F.mse_loss(out, tgt.cuda()).backward()
    return [x.grad for x in xs]


def oracle_input_grads(sd, frame, refs, mask, tgt, train, dt=torch.float32, params=None):
    """the oracle's gradients of (frame, refs, mask); params (a dict): also receives the parameter gradients"""
    P = _d(sd, dt)
    xs = [t.to(dt).clone().requires_grad_() for t in (frame, refs, mask)]
    F.mse_loss(fr_oracle.frame_recovery_forward(P, *xs, train), tgt.to(dt)).backward()
    if params is not None:
        params.update({k: v.grad for k, v in P.items() if v.grad is not None})
    return [x.grad for x in xs]


def check_vs_oracle(name, hip, o32, o64_fn, layer_l2_fn=None):
    """1e-3 of the fp32 oracle's max, or (ill-conditioned fp32) the float64 attribution rule (module docstring); returns a
    note.  layer_l2_fn: relative L2 distance from float64 of HIP's weight gradient of the layer the input enters."""
    e = rel(hip, o32)
    if e < REL:
        return f"{name} {e:.1e}"
    o64 = o64_fn()
    h64, r64, l2 = rel(hip, o64), rel(o32, o64), rel_l2(hip, o64)
    note = f"{name} {e:.1e} (f64: HIP {h64:.1e}, fp32 oracle {r64:.1e}, L2 {l2:.1e}"
    ok = h64 <= 4 * r64 + 2e-5
    if not ok and layer_l2_fn is not None:
        w_l2 = layer_l2_fn()
        note += f", layer weight grad L2 {w_l2:.1e}"
        ok = l2 <= 2 * w_l2 + 2e-5
    assert ok and l2 < L2_CAP, note
    return note + ")"


LAYER = {"dframe": "spatial_encoder.stem.0.weight", "drefs": "temporal_encoder.conv1.spatial.0.weight",
         "dmask": "spatial_encoder.stem.0.weight"}


# ------------------------------------------------------------------ (1) exact-fp32 mode against the oracle
CASES = [  # (time_in_channels, train, T, base, H, W)
    (True, True, 2, 16, 128, 160), (True, False, 4, 64, 50, 70), (False, True, 4, 16, 50, 70),
    (False, False, 2, 64, 128, 160), (True, True, 1, 64, 128, 160), (False, True, 1, 16, 50, 70),
    (True, True, 4, 64, 128, 160), (False, False, 1, 16, 128, 160), (True, False, 2, 16, 50, 70)]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("tic,train,T,base,H,W", CASES)
def test_fr_input_grad_fp32_vs_oracle(tic, train, T, base, H, W):
    net, sd = fr_net(base, T, train, tic)
    frame, refs, mask, tgt = soft_inputs(2, T, H, W)
    g = hip_input_grads(net, frame, refs, mask, tgt)
    assert all(x is not None for x in g)
    assert g[0].shape == frame.shape and g[1].shape == refs.shape and g[2].shape == mask.shape
    o32 = oracle_input_grads(sd, frame, refs, mask, tgt, train)
    o64, p64 = [], {}
    hip_w = {n: p.grad for n, p in net.named_parameters()}

    def f64(i):
        def get():
            if not o64:
                o64.extend(oracle_input_grads(sd, frame, refs, mask, tgt, train, torch.float64, p64))
            return o64[i]
        return get

    def layer_l2(n):
        return lambda: rel_l2(hip_w[LAYER[n]], p64[LAYER[n]])

    notes = [check_vs_oracle(n, g[i], o32[i], f64(i), layer_l2(n)) for i, n in enumerate(("dframe", "drefs", "dmask"))]
    print(f"  FR fp32 {'tc' if tic else 'tm'} {'train' if train else 'eval'} T{T} base{base} {H}x{W}: {notes}")


def test_fr_input_grad_each_input_alone_and_no_mask():
    """only one input needing a gradient at a time gives that input's gradient of the all-inputs run, bit for bit;
    corruption_mask=None is zeros with no gradient"""
    frame, refs, mask, tgt = soft_inputs(1, 2, 64, 96)
    net, _ = fr_net(16, 2, True)
    full = hip_input_grads(net, frame, refs, mask, tgt)
    for i in range(3):
        net, _ = fr_net(16, 2, True)
        want = tuple(j == i for j in range(3))
        g = hip_input_grads(net, frame, refs, mask, tgt, want)
        assert torch.equal(g[i], full[i]), i
        assert all(g[j] is None for j in range(3) if j != i)
    net, sd = fr_net(16, 2, False)
    fc, rc = frame.cuda().requires_grad_(), refs.cuda().requires_grad_()
    F.mse_loss(net(fc, rc), tgt.cuda()).backward()
    P = {k: v.clone() for k, v in sd.items()}
    fo, ro = frame.clone().requires_grad_(), refs.clone().requires_grad_()
    F.mse_loss(fr_oracle.frame_recovery_forward(P, fo, ro, None, False), tgt).backward()
    assert rel(fc.grad, fo.grad) < REL and rel(rc.grad, ro.grad) < REL


# ------------------------------------------------------------------ (2) bf16 mode
# relative L2 / cosine of the HIP-bf16 input gradient against float64.  Measured on MI355X (base 64, T 4, 128x160, train;
# time-in-channels / time-major): bf16 activations dframe 0.580 / 0.581 (cosine 0.837 / 0.838), drefs 0.559 (0.844),
# dmask 0.567 (0.846); fp32 activations dframe 0.398 / 0.394 (0.921 / 0.923), drefs 0.429 / 0.432 (0.908 / 0.907),
# dmask 0.387 / 0.382 (0.926 / 0.928).  That distance is the rounding, not a kernel defect: against the float64 oracle that
# rounds the same operands and stored tensors to bf16 (oracle/fr_oracle.py prec, tests/test_fr_bf16_emulated_gpu.py) the eval
# step agrees to 4e-5 whole-gradient L2, and in this training step the same emulation evaluated in float32 on the CPU lies as
# far (0.35-0.39 on these three) from itself in float64 as the HIP network does: with batch statistics the step is chaotic in
# the bf16 rounding, so no tighter bound holds in training mode at this size.
BF16_BOUNDS = {True: (0.70, 0.78), False: (0.52, 0.86)}    # bf16_activations: (max rel L2, min cosine)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("tic", [True, False], ids=["tc", "tm"])
@pytest.mark.parametrize("acts", [True, False], ids=["bf16_acts", "fp32_acts"])
def test_fr_input_grad_bf16_vs_float64(acts, tic):
    net, sd = fr_net(64, 4, True, tic, bf16=acts)
    frame, refs, mask, tgt = soft_inputs(2, 4, 128, 160)
    g = hip_input_grads(net, frame, refs, mask, tgt)
    o64 = oracle_input_grads(sd, frame, refs, mask, tgt, True, torch.float64)
    notes = []
    for i, n in enumerate(("dframe", "drefs", "dmask")):
        l2, cs = rel_l2(g[i], o64[i]), cosine(g[i], o64[i])
        notes.append(f"{n} L2 {l2:.2e} cos {cs:.4f}")
        mx, mn = BF16_BOUNDS[acts]
        assert l2 <= mx and cs >= mn, (n, l2, cs)
    print(f"  FR bf16 acts={acts} {'tc' if tic else 'tm'}: {notes}")


# ------------------------------------------------------------------ (3) the kernels
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Co", [16, 32, 64])
def test_stem7_dgrad_kernel(Co, bf16):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(Co + bf16)
    for N, H, W in ((2, 37, 53), (1, 9, 33), (3, 50, 70), (1, 64, 32)):
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        ld = Co + 8 if Co == 32 else Co                       # a padded row for one width
        w = torch.randn(Co, 4, 7, 7, generator=gen)
        dy = torch.randn(N, OH, OW, ld, generator=gen)
        if bf16:
            dy = dy.to(torch.bfloat16)
        g = dy.double()[..., :Co].permute(0, 3, 1, 2)
        ref = torch.nn.grad.conv2d_input((N, 4, H, W), w.double(), g, stride=2, padding=3)
        base_f, base_m = torch.randn(N, 3, H, W, generator=gen), torch.randn(N, 1, H, W, generator=gen)
        for acc in (False, True):
            for which in ("both", "frame", "mask"):
                df = base_f.clone().cuda() if which != "mask" else None
                dm = base_m.clone().cuda() if which != "frame" else None
                _nvq.stem7_dgrad(dy.cuda(), w.cuda(), df, dm, H, W, accumulate=acc)
                if df is not None:
                    got = df.cpu().double() - (base_f.double() if acc else 0.0)
                    assert rel(got, ref[:, :3]) <= 1e-5, (N, H, W, acc, which)
                if dm is not None:
                    got = dm.cpu().double() - (base_m.double() if acc else 0.0)
                    assert rel(got, ref[:, 3:]) <= 1e-5, (N, H, W, acc, which)
        again = torch.empty(N, 3, H, W, device="cuda")
        again2 = torch.empty(N, 3, H, W, device="cuda")
        _nvq.stem7_dgrad(dy.cuda(), w.cuda(), again, None, H, W)
        _nvq.stem7_dgrad(dy.cuda(), w.cuda(), again2, None, H, W)
        assert torch.equal(again, again2)                     # deterministic


@pytest.mark.parametrize("ld", [4, 8])
def test_mask_blend_backward_ex_kernel(ld):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(ld)
    N, C, H, W = 2, 3, 19, 45
    dout, frame = torch.randn(N, C, H, W, generator=gen), torch.randn(N, C, H, W, generator=gen)
    rec, mask = torch.randn(N, H, W, ld, generator=gen), torch.rand(N, 1, H, W, generator=gen)
    recn = rec[..., :C].permute(0, 3, 1, 2)
    want_rec = torch.zeros(N, H, W, ld)
    want_rec[..., :C] = (dout * mask).permute(0, 2, 3, 1)
    want_f = dout * (1 - mask)
    want_m = (dout.double() * (recn.double() - frame.double())).sum(1, keepdim=True)
    c = lambda t: t.cuda()
    for wf, wm in ((True, True), (True, False), (False, True), (False, False)):
        drec = torch.full((N, H, W, ld), float("nan"), device="cuda")
        df = torch.full((N, C, H, W), float("nan"), device="cuda") if wf else None
        dm = torch.full((N, 1, H, W), float("nan"), device="cuda") if wm else None
        _nvq.mask_blend_backward_ex(c(dout), c(frame), c(rec), c(mask), drec, df, dm)
        assert torch.equal(drec.cpu(), want_rec)
        if wf:
            assert torch.equal(df.cpu(), want_f)
        if wm:
            assert rel(dm, want_m) <= 1e-6
    # drec is what nvq_mask_blend_backward writes
    drec2 = torch.empty(N, H, W, ld, device="cuda")
    from nerve_cl._nvq import check, lib, ptr, stream
    dout_d, mask_d = c(dout), c(mask)                         # (held: a freed temporary's block would be reused)
    check(lib().nvq_mask_blend_backward(ptr(dout_d), ptr(mask_d), N, C, H, W, ptr(drec2), ld, stream()), "blend")
    assert torch.equal(drec2.cpu(), want_rec)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [2, 3, 4, 5])
def test_head_dgrad_tc_kernel(T, bf16):
    from nerve_cl import _nvq
    gen = torch.Generator().manual_seed(T * 10 + bf16)
    B, H, W, Fc, Cp = 2, 19, 45, 32, 32
    w = torch.randn(Fc, 3, 3, 3, generator=gen)
    g = torch.randn(B, H, W, T * Cp, generator=gen)
    if bf16:
        g = g.to(torch.bfloat16)
    ref = torch.empty(B, T, 3, H, W, dtype=torch.float64)
    for t in range(T):
        gt = g.double()[..., t * Cp:t * Cp + Fc].permute(0, 3, 1, 2)
        ref[:, t] = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), gt, padding=1)
    out = torch.full((B, T, 3, H, W), float("nan"), device="cuda")
    _nvq.head_dgrad_tc(g.cuda(), w.cuda(), B, list(range(T)), [t * Cp for t in range(T)], 0, out)
    assert rel(out, ref) <= 1e-5
    again = torch.ones_like(out)
    _nvq.head_dgrad_tc(g.cuda(), w.cuda(), B, list(range(T)), [t * Cp for t in range(T)], 0, again, accumulate=True)
    assert rel(again - 1.0, ref) <= 1e-5
    # the time-major form (slot_images = B, offsets 0) is nvq_head_dgrad's pre-masked form, bit for bit
    gtm = torch.cat([g[..., t * Cp:(t + 1) * Cp] for t in range(T)], 0).contiguous().cuda()
    a, b = torch.empty_like(out), torch.empty_like(out)
    _nvq.head_dgrad(gtm, w.cuda(), B, list(range(T)), a)
    _nvq.head_dgrad_tc(gtm, w.cuda(), B, list(range(T)), [0] * T, B, b)
    assert torch.equal(a, b)
    assert rel(a, ref) <= 1e-5


# ------------------------------------------------------------------ (4) frozen parameters, (5) determinism
@pytest.mark.parametrize("tic", [True, False], ids=["tc", "tm"])
def test_fr_input_grad_frozen_parameters(tic):
    frame, refs, mask, tgt = soft_inputs(2, 2, 64, 96)
    net, _ = fr_net(16, 2, True, tic)
    ref = hip_input_grads(net, frame, refs, mask, tgt)
    net, _ = fr_net(16, 2, True, tic)
    for p in net.parameters():
        p.requires_grad_(False)
    net._last_grad_bucket = None
    got = hip_input_grads(net, frame, refs, mask, tgt)
    assert all(p.grad is None for p in net.parameters())
    assert net._last_grad_bucket is None                      # no bucket was finished
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # autograd.grad with respect to the inputs alone
    net, _ = fr_net(16, 2, True, tic)
    for p in net.parameters():
        p.requires_grad_(False)
    xs = [t.cuda().requires_grad_() for t in (frame, refs, mask)]
    gx = torch.autograd.grad(F.mse_loss(net(*xs), tgt.cuda()), xs)
    for a, b in zip(gx, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tic", [True, False], ids=["tc", "tm"])
@pytest.mark.parametrize("bf16", [None, True], ids=["fp32", "bf16"])
def test_fr_input_grad_deterministic_and_param_grads_unchanged(bf16, tic):
    frame, refs, mask, tgt = soft_inputs(2, 4, 96, 128)
    runs = []
    for want in (True, True, False):
        net, _ = fr_net(32, 4, True, tic, bf16=bf16)
        g = hip_input_grads(net, frame, refs, mask, tgt, (want,) * 3)
        assert all((x is not None) == want for x in g)
        runs.append((g, {n: p.grad.clone() for n, p in net.named_parameters()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[2][1][n]), n
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


# ------------------------------------------------------------------ (6) the engine's clip gradient
def _d(sd, dt):
    return {k: (v.detach().to(dt).clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone())
            for k, v in sd.items()}


def test_engine_clip_grad_through_recovery_and_lightweight_sr():
    from nerve_cl import _nvq
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    base, s, B, T, H, W = 16, 2, 2, 5, 64, 96
    eng = EnhancementEngine(EnhancementConfig(use_lightweight_sr=True, recovery_base_channels=base, scale_factor=s))
    sd_fr, sd_l = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN), synth.formula_state_light(s, gain=synth.GOLDEN_GAIN)
    eng.frame_recovery.load_state_dict(sd_fr, strict=True)
    eng.super_resolution.load_state_dict(sd_l, strict=True)
    # eval mode (running statistics): training mode through this chain at this size is the ill-conditioned case of
    # test_engine_trains_frame_recovery_through_lightweight_sr; the temporal-SR test below runs in training mode
    eng = eng.cuda().eval()
    for m in (eng.frame_recovery, eng.super_resolution):
        m.math_mode, m.bf16_activations = _nvq.MATH_F32, False
    clip = synth.formula_clip(B, T, H, W)
    mask = torch.zeros(B, 1, H, W)
    mask[:, :, 16:48, 24:72] = 1.0
    tgt = synth.formula_target(B, H * s, W * s)
    cg = clip.cuda().requires_grad_()
    F.mse_loss(eng(cg, corruption_mask=mask.cuda())["enhanced"], tgt.cuda()).backward()

    def chain(dt):
        Pf, Pl = _d(sd_fr, dt), _d(sd_l, dt)
        c = clip.to(dt).clone().requires_grad_()
        rec = fr_oracle.frame_recovery_forward(Pf, c[:, 2], c[:, [0, 1, 3, 4]], mask.to(dt), False)
        F.mse_loss(sr_oracle.light_forward(Pl, rec, False), tgt.to(dt)).backward()
        return c.grad

    o32 = chain(torch.float32)
    note = check_vs_oracle("clip", cg.grad, o32, lambda: chain(torch.float64))
    # every frame gets a share: the centre through the blend / stem, the others through the temporal encoder
    assert all(cg.grad[:, t].abs().max() > 0 for t in range(T))
    print(f"  engine FR + light SR: {note}")


def test_engine_clip_grad_through_recovery_and_temporal_sr_blend():
    from nerve_cl import _nvq
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    base, s, Fc, N, win, B, H, W = 16, 2, 32, 2, 1, 2, 64, 96
    eng = EnhancementEngine(EnhancementConfig(recovery_base_channels=base, scale_factor=s, sr_num_features=Fc,
                                              sr_num_residual_blocks=N, sr_temporal_window=win, recovery_temporal_window=win))
    sd_fr, sd_sr = synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN), synth.formula_state(3, s, Fc, N, win,
                                                                                               gain=synth.GOLDEN_GAIN)
    eng.frame_recovery.load_state_dict(sd_fr, strict=True)
    eng.super_resolution.load_state_dict(sd_sr, strict=True)
    eng = eng.cuda().train()
    for m in (eng.frame_recovery, eng.super_resolution):
        m.math_mode, m.bf16_activations = _nvq.MATH_F32, False
    T, tc, strength = 3, 1, 0.7
    clip = synth.formula_clip(B, T, H, W)
    mask = torch.zeros(B, 1, H, W)
    mask[:, :, 16:48, 24:72] = 1.0
    tgt = synth.formula_target(B, H * s, W * s)
    cg = clip.cuda().requires_grad_()
    res = eng(cg, corruption_mask=mask.cuda(), enhancement_strength=strength)
    (F.mse_loss(res["enhanced"], tgt.cuda()) + F.mse_loss(res["recovered"], cg[:, tc].detach())).backward()

    def chain(dt):
        Pf, Ps = _d(sd_fr, dt), _d(sd_sr, dt)
        c = clip.to(dt).clone().requires_grad_()
        rec = fr_oracle.frame_recovery_forward(Pf, c[:, tc], c[:, [0, 2]], mask.to(dt), True)
        o = strength * sr_oracle.sr_forward(Ps, c, True) + (1 - strength) * sr_oracle.bicubic_up(c[:, tc], s)
        (F.mse_loss(o, tgt.to(dt)) + F.mse_loss(rec, clip.to(dt)[:, tc])).backward()
        return c.grad

    o32 = chain(torch.float32)
    note = check_vs_oracle("clip", cg.grad, o32, lambda: chain(torch.float64))
    print(f"  engine FR + temporal SR blend: {note}")
