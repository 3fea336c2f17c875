"""GPU: frozen layers in FrameRecoveryNet.  With some parameters frozen (requires_grad False) a
training step runs; frozen .grad stays None; every trained gradient, the output, the BatchNorm running statistics and the
image inputs' gradients are bit-identical to the all-trainable step's.  Also: which launches the backward makes (launch
audit), nvq_bn2_backward_ex against nvq_bn2_backward and torch, the EnhancementEngine, the data-parallel bucket,
determinism and a stand-alone ResidualBlock."""
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu

BASE, B, T, H, W = 16, 2, 2, 64, 96


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(a.dtype)
    return torch.equal(a.view(iv), b.view(iv)) if iv is not None else torch.equal(a, b)


def _is_bn(n):
    # the BatchNorm affines of FrameRecoveryNet: stem.1, the stage-entry '.1', ResidualBlock conv1.bn / conv2.2,
    # TemporalConv3D spatial.1 / temporal.1, decoder upK.1
    return re.search(r"(\.stem\.1|\.stage\d\.0\.1|\.conv1\.bn|\.conv2\.2|\.spatial\.1|\.temporal\.1|\.up\d\.1)\.(weight|bias)$",
                     n) is not None


PATTERNS = {
    # name: (frozen-parameter predicate, image inputs need a gradient)
    "all_trainable": (lambda n: False, False),
    "encoders_frozen": (lambda n: n.startswith(("spatial_encoder.", "temporal_encoder.")), False),
    "decoder_only": (lambda n: not n.startswith("decoder."), False),
    "decoder_frozen": (lambda n: n.startswith("decoder."), False),
    "bn_affine_frozen": (_is_bn, False),
    "final_only": (lambda n: not n.startswith("decoder.final."), False),
    "fusion_only": (lambda n: not n.startswith("fusion."), False),
    "one_bn_bias": (lambda n: n == "fusion.refine.0.conv2.2.bias", False),
    "all_frozen_inputs": (lambda n: True, True),
}


def make_net(train, bf16, tic):
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet
    net = FrameRecoveryNet(3, BASE, T)
    net.load_state_dict(synth.formula_state_fr(3, BASE, gain=synth.GOLDEN_GAIN), strict=True)
    net = net.cuda().train(train)
    net.time_in_channels = tic
    net.math_mode, net.bf16_activations = (_nvq.MATH_BF16, True) if bf16 else (_nvq.MATH_F32, False)
    return net


def inputs(seed=5):
    clip = synth.formula_clip(B, T + 1, H, W, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    mask = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=gen)
    tgt = synth.formula_target(B, H, W, seed=seed + 1)
    return clip[:, 0].contiguous().cuda(), clip[:, 1:].contiguous().cuda(), mask.cuda(), tgt.cuda()


def step(net, data, frozen, want=(False, False, False)):
    """one forward + MSE + backward with `frozen` parameters frozen; returns (grads, output, buffers, input grads)"""
    frame, refs, mask, tgt = data
    for n, p in net.named_parameters():
        p.requires_grad_(not frozen(n))
        p.grad = None
    xs = [t.clone().requires_grad_(w) for t, w in zip((frame, refs, mask), want)]
    out = net(*xs)
    F.mse_loss(out, tgt).backward()
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in net.named_parameters()}
    bufs = {n: b.clone() for n, b in net.named_buffers()}
    return grads, out.detach().clone(), bufs, [x.grad for x in xs]


def check_against_reference(got, ref, frozen):
    grads, out, bufs, dins = got
    rgrads, rout, rbufs, rdins = ref
    for n, g in grads.items():
        if frozen(n):
            assert g is None, n
        else:
            assert g is not None and bits_equal(g, rgrads[n]), n
    assert bits_equal(out, rout)
    for n, b in bufs.items():
        assert bits_equal(b, rbufs[n]), n


# ------------------------------------------------------------------ (1) partial freezing trains, bit for bit
@pytest.mark.parametrize("tic", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pattern", [p for p in PATTERNS if p != "all_trainable"])
def test_partial_freezing_bit_identical(pattern, train, bf16, tic):
    frozen, with_inputs = PATTERNS[pattern]
    want = (with_inputs,) * 3
    data = inputs()
    ref = step(make_net(train, bf16, tic), data, lambda n: False, want)
    got = step(make_net(train, bf16, tic), data, frozen, want)
    check_against_reference(got, ref, frozen)
    if with_inputs:
        for a, b in zip(got[3], ref[3]):
            assert bits_equal(a, b)


def test_requires_grad_toggled_between_steps():
    net = make_net(True, True, True)
    data = inputs()
    for pattern in ("encoders_frozen", "all_trainable", "decoder_only", "encoders_frozen"):
        frozen = PATTERNS[pattern][0]
        grads = step(net, data, frozen)[0]
        for n, g in grads.items():
            assert (g is None) == frozen(n), (pattern, n)


# ------------------------------------------------------------------ (2) input gradients behind a frozen encoder
@pytest.mark.parametrize("tic", [True, False])
@pytest.mark.parametrize("train,bf16", [(True, False), (False, True)])
def test_input_grads_with_frozen_encoders(tic, train, bf16):
    frozen = PATTERNS["encoders_frozen"][0]
    data = inputs(seed=9)
    ref = step(make_net(train, bf16, tic), data, lambda n: False, (True, True, True))
    got = step(make_net(train, bf16, tic), data, frozen, (True, True, True))
    check_against_reference(got, ref, frozen)
    for a, b in zip(got[3], ref[3]):                          # dframe, drefs, dmask
        assert a is not None and bits_equal(a, b)


# ------------------------------------------------------------------ (3) launch audit
_OWNED = {"Conv": 1, "DwConv": 1, "SpatialConvTC": 1, "TemporalConvTC": 1, "CBAMFn": 1, "BatchNorm": 1}
_FIXED = {"Stem7": "spatial_encoder", "TemporalConv": "temporal_encoder", "ConvT": "decoder"}


def audit(monkeypatch, net, data, frozen):
    """run one step; returns (ops, launches): the op backwards that ran as (class, owner parameter name), and the launches as
    (name, owner, detail).  The owner of an op is the parameter it saved (or its network part when it saves none)."""
    from nerve_cl import _nvq, _ops
    by_ptr = {p.data_ptr(): n for n, p in net.named_parameters()}
    ops, launches, cur = [], [], [None]

    for cls_name in list(_OWNED) + list(_FIXED):
        cls = getattr(_ops, cls_name)
        orig = cls.backward

        def bwd(ctx, *grads, _orig=orig, _name=cls_name):
            if _name in _FIXED:
                owner = _FIXED[_name]
            else:
                owner = by_ptr.get(ctx.saved_tensors[_OWNED[_name]].data_ptr(), "?")
            ops.append((_name, owner))
            prev, cur[0] = cur[0], owner
            try:
                return _orig(ctx, *grads)
            finally:
                cur[0] = prev
        monkeypatch.setattr(cls, "backward", staticmethod(bwd))

    def wrap_py(name):
        orig = getattr(_nvq, name)

        def f(*a, **kw):
            launches.append((name, cur[0], None))
            return orig(*a, **kw)
        monkeypatch.setattr(_nvq, name, f)
    for name in ("conv_wgrad", "dwconv_wgrad"):
        wrap_py(name)

    def cbam_side(name, idx):
        orig = getattr(_nvq, name)

        def f(*a, **kw):
            launches.append((name, cur[0], "wgrad" if any(a[i] is not None for i in idx) else "no_wgrad"))
            return orig(*a, **kw)
        monkeypatch.setattr(_nvq, name, f)
    cbam_side("cbam_bwd_spatial_conv", (4,))
    cbam_side("cbam_bwd_channel", (11, 12))

    lib = _nvq.lib()

    def wrap_lib(name, detail=None):
        orig = getattr(lib, name)

        def f(*a):
            launches.append((name, cur[0], detail(a) if detail else None))
            return orig(*a)
        monkeypatch.setattr(lib, name, f)
    # (training, dgamma, dbeta, flags) of the BatchNorm backwards
    wrap_lib("nvq_bn2_backward", lambda a: (a[13], a[18] is not None, a[19] is not None, 0))
    wrap_lib("nvq_bn2_backward_ex", lambda a: (a[13], a[18] is not None, a[19] is not None, a[23]))
    for name in ("nvq_stem7_wgrad", "nvq_convt_unpack_grad", "nvq_tconv_grad_combine", "nvq_tconv_relayout", "nvq_stem7_dgrad"):
        wrap_lib(name)
    step(net, data, frozen)
    torch.cuda.synchronize()
    return ops, launches


def _enc(owner):
    return owner is not None and owner.startswith(("spatial_encoder", "temporal_encoder"))


@pytest.mark.parametrize("tic", [True, False])
def test_launch_audit_encoders_frozen(monkeypatch, tic):
    net = make_net(True, True, tic)
    ops, launches = audit(monkeypatch, net, inputs(), PATTERNS["encoders_frozen"][0])
    assert ops and not [o for o in ops if _enc(o[1])], ops         # no encoder op's backward runs at all
    assert not [l for l in launches if _enc(l[1])], launches
    assert not [l for l in launches if l[0] in ("nvq_stem7_wgrad", "nvq_stem7_dgrad", "nvq_tconv_grad_combine")]
    # the trained part still forms its weight gradients
    assert any(l[0] == "conv_wgrad" and l[1].startswith("decoder.") for l in launches)
    assert any(l[0] == "conv_wgrad" and l[1].startswith("fusion.") for l in launches)


def test_launch_audit_decoder_frozen_eval(monkeypatch):
    from nerve_cl import _nvq
    net = make_net(False, True, True)
    ops, launches = audit(monkeypatch, net, inputs(), PATTERNS["decoder_frozen"][0])
    dec_bn = [l for l in launches if l[0].startswith("nvq_bn2_backward") and l[1].startswith("decoder.")]
    assert len(dec_bn) == 4
    for name, _, (training, dg, db, flags) in dec_bn:
        # the one-pass eval form: no partial, no final launch
        assert name == "nvq_bn2_backward_ex" and flags == _nvq.NO_WGRAD and training == 0 and not dg and not db
    assert not [l for l in launches if l[1] == "decoder" and l[0] == "conv_wgrad"]
    assert not [l for l in launches if l[1] is not None and l[1].startswith("decoder.") and l[0] == "conv_wgrad"]
    assert not [l for l in launches if l[0] == "nvq_convt_unpack_grad"]
    assert sum(1 for o in ops if o[0] == "ConvT") == 4             # their input gradients still run
    # the trained encoders and fusion: full forms
    other_bn = [l for l in launches if l[0].startswith("nvq_bn2_backward") and not l[1].startswith("decoder.")]
    assert other_bn and all(l[0] == "nvq_bn2_backward" for l in other_bn)


@pytest.mark.parametrize("tic", [True, False])
def test_launch_audit_nothing_frozen(monkeypatch, tic):
    net = make_net(True, True, tic)
    ops, launches = audit(monkeypatch, net, inputs(), PATTERNS["all_trainable"][0])
    n_bn = sum(isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)) for m in net.modules())
    bn = [l for l in launches if l[0].startswith("nvq_bn2_backward")]
    assert len(bn) == n_bn
    assert all(l[0] == "nvq_bn2_backward" and l[2][1] and l[2][2] for l in bn)
    # one weight-gradient launch set per parameterised op
    per_op = {}
    for name, owner, _ in launches:
        if name in ("conv_wgrad", "dwconv_wgrad", "nvq_stem7_wgrad", "nvq_convt_unpack_grad"):
            per_op[owner] = per_op.get(owner, 0) + 1
    for cls, owner in ops:
        if cls != "BatchNorm" and cls != "CBAMFn":
            assert per_op.get(owner, 0) >= 1, (cls, owner)
    assert sum(1 for l in launches if l[0] == "nvq_stem7_wgrad") == 1
    assert sum(1 for l in launches if l[0] == "nvq_convt_unpack_grad") == 4
    assert [l[2] for l in launches if l[0].startswith("cbam_bwd_")] == ["wgrad"] * 4   # two CBAMs x (spatial, channel)
    assert sum(1 for o in ops if o[0] == "Conv" and o[1] == "decoder.final.0.weight") == 1


# ------------------------------------------------------------------ (4) nvq_bn2_backward_ex against nvq_bn2_backward
def _bn2_backward(fn, flags, dy, x, mean, invstd, gamma, beta, res, relu, training, dgamma, dbeta, ws):
    from nerve_cl import _nvq
    from nerve_cl._nvq import ptr, stream
    N, Hh, Ww, ld = x.shape
    C = gamma.numel()
    dx = torch.full_like(x, float("nan"))
    dres = torch.full_like(res, float("nan")) if res is not None else None
    args = (ptr(dy), dy.shape[-1], ptr(x), ld, C, N * Hh * Ww, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(res),
            res.shape[-1] if res is not None else 0, int(relu), int(training), ptr(dx), ld, ptr(dres),
            dres.shape[-1] if dres is not None else 0, ptr(dgamma), ptr(dbeta), ptr(ws),
            ws.numel() * 4 if ws is not None else 0, int(x.dtype == torch.bfloat16))
    lib = _nvq.lib()
    if fn == "full":
        _nvq.check(lib.nvq_bn2_backward(*args, stream()), "nvq_bn2_backward")
    else:
        _nvq.check(lib.nvq_bn2_backward_ex(*args, flags, stream()), "nvq_bn2_backward_ex")
    torch.cuda.synchronize()
    return dx, dres


def _bn_case(bf16, C=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    N, Hh, Ww = 3, 17, 29
    ld = (C + 7) // 8 * 8 if bf16 else (C + 3) // 4 * 4
    dt = torch.bfloat16 if bf16 else torch.float32

    def act():
        t = torch.zeros(N, Hh, Ww, ld)
        t[..., :C] = torch.randn(N, Hh, Ww, C, generator=g)
        return t.to(dt).cuda()
    x, dy, res = act(), act(), act()
    mean = (torch.randn(C, generator=g) * 0.1).cuda()
    invstd = (torch.rand(C, generator=g) + 0.5).cuda()
    gamma, beta = torch.randn(C, generator=g).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    return x, dy, res, mean, invstd, gamma, beta


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, True), (True, False)])
def test_bn2_backward_ex_bits(bf16, training, with_res, relu):
    from nerve_cl import _engine, _nvq
    x, dy, res, mean, invstd, gamma, beta = _bn_case(bf16)
    res = res if with_res else None
    C = gamma.numel()
    ws = _engine.workspace(torch.device("cuda"))
    dg0, db0 = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx0, dres0 = _bn2_backward("full", 0, dy, x, mean, invstd, gamma, beta, res, relu, training, dg0, db0, ws)

    def same(a, b):
        return (a is None and b is None) or bits_equal(a, b)
    # flags 0 with both affine outputs: exactly the full form
    dg, db = torch.empty_like(dg0), torch.empty_like(db0)
    dx, dres = _bn2_backward("ex", 0, dy, x, mean, invstd, gamma, beta, res, relu, training, dg, db, ws)
    assert same(dx, dx0) and same(dres, dres0) and bits_equal(dg, dg0) and bits_equal(db, db0)
    # one affine output NULL (flags 0): the other one unchanged
    dg = torch.empty_like(dg0)
    dx, dres = _bn2_backward("ex", 0, dy, x, mean, invstd, gamma, beta, res, relu, training, dg, None, ws)
    assert same(dx, dx0) and same(dres, dres0) and bits_equal(dg, dg0)
    db = torch.empty_like(db0)
    dx, dres = _bn2_backward("ex", 0, dy, x, mean, invstd, gamma, beta, res, relu, training, None, db, ws)
    assert same(dx, dx0) and same(dres, dres0) and bits_equal(db, db0)
    # both NULL, with and without NVQ_NO_WGRAD (with the flag, given buffers stay untouched)
    dx, dres = _bn2_backward("ex", 0, dy, x, mean, invstd, gamma, beta, res, relu, training, None, None, ws)
    assert same(dx, dx0) and same(dres, dres0)
    sg, sb = torch.full_like(dg0, float("nan")), torch.full_like(db0, float("nan"))
    dx, dres = _bn2_backward("ex", _nvq.NO_WGRAD, dy, x, mean, invstd, gamma, beta, res, relu, training, sg, sb, ws)
    assert same(dx, dx0) and same(dres, dres0)
    assert torch.isnan(sg).all() and torch.isnan(sb).all()
    if not training:
        # the eval one-pass form needs no workspace at all
        dx, dres = _bn2_backward("ex", _nvq.NO_WGRAD, dy, x, mean, invstd, gamma, beta, res, relu, training, None, None, None)
        assert same(dx, dx0) and same(dres, dres0)


@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, True)])
def test_bn2_backward_ex_eval_vs_torch(with_res, relu):
    """eval NO_WGRAD form, fp32: dx (and dres) against autograd of F.batch_norm (+ res) (+ ReLU) at 1e-6"""
    from nerve_cl import _nvq
    x, dy, res, _, _, gamma, beta = _bn_case(False, C=40, seed=3)
    C = gamma.numel()
    rmean = (torch.randn(C, generator=torch.Generator().manual_seed(4)) * 0.1).cuda()
    rvar = (torch.rand(C, generator=torch.Generator().manual_seed(5)) + 0.5).cuda()
    mean, invstd = rmean.clone(), 1.0 / torch.sqrt(rvar + 1e-5)
    res = res if with_res else None
    dx, dres = _bn2_backward("ex", _nvq.NO_WGRAD, dy, x, mean, invstd, gamma, beta, res, relu, False, None, None, None)
    xr = x[..., :C].double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    rr = res[..., :C].double().permute(0, 3, 1, 2).contiguous().requires_grad_() if with_res else None
    y = F.batch_norm(xr, rmean.double(), rvar.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    if with_res:
        y = y + rr
    pre = y.detach()
    if relu:
        y = torch.relu(y)
    y.backward(dy[..., :C].double().permute(0, 3, 1, 2))
    # (elements whose ReLU input is within 1e-4 of 0 may take the other side in fp32: left out)
    clear = (pre.abs() > 1e-4).permute(0, 2, 3, 1) if relu else torch.ones_like(dx[..., :C], dtype=torch.bool)
    assert clear.float().mean().item() > 0.99
    ref = xr.grad.permute(0, 2, 3, 1)
    scale = ref.abs().max().item()
    assert (dx[..., :C].double() - ref)[clear].abs().max().item() <= 1e-6 * scale
    assert torch.count_nonzero(dx[..., C:]).item() == 0
    if with_res:
        rref = rr.grad.permute(0, 2, 3, 1)
        assert (dres[..., :C].double() - rref)[clear].abs().max().item() <= 1e-6 * max(rref.abs().max().item(), 1e-30)


# ------------------------------------------------------------------ (5) the engine
def test_engine_encoders_frozen():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    base, s, Bn, Tn, Hn, Wn, Fc, NB = 16, 2, 2, 5, 64, 96, 32, 2

    def engine():
        eng = EnhancementEngine(EnhancementConfig(recovery_base_channels=base, scale_factor=s, sr_num_features=Fc,
                                                  sr_num_residual_blocks=NB))
        eng.frame_recovery.load_state_dict(synth.formula_state_fr(3, base, gain=synth.GOLDEN_GAIN), strict=True)
        eng.super_resolution.load_state_dict(synth.formula_state(3, s, Fc, NB, 1, gain=synth.GOLDEN_GAIN), strict=True)
        eng = eng.cuda().train()
        eng.super_resolution.deterministic = True
        return eng
    clip = synth.formula_clip(Bn, Tn, Hn, Wn).cuda()
    mask = torch.zeros(Bn, 1, Hn, Wn, device="cuda")
    mask[:, :, 16:48, 24:72] = 1.0
    tgt_sr = synth.formula_target(Bn, Hn * s, Wn * s).cuda()
    tgt_fr = synth.formula_target(Bn, Hn, Wn, seed=7).cuda()

    def run(frozen):
        eng = engine()
        for n, p in eng.named_parameters():
            p.requires_grad_(not frozen(n))
        r = eng(clip, corruption_mask=mask)
        (F.mse_loss(r["enhanced"], tgt_sr) + F.mse_loss(r["recovered"], tgt_fr)).backward()
        return {n: p.grad for n, p in eng.named_parameters()}
    ref = run(lambda n: False)
    frozen = lambda n: n.startswith(("frame_recovery.spatial_encoder.", "frame_recovery.temporal_encoder."))  # noqa: E731
    got = run(frozen)
    assert ref["frame_recovery.decoder.final.0.weight"] is not None
    for n, g in got.items():
        if frozen(n) or ref[n] is None:                           # (enhancement_strength: no blend at strength 1)
            assert g is None, n
        else:
            assert g is not None and bits_equal(g, ref[n]), n


# ------------------------------------------------------------------ (6) data-parallel bucket, (7) determinism
def test_bucket_hook_frozen_slots_zero():
    net = make_net(True, True, True)
    seen = []
    net._grad_bucket_hook = lambda flat: seen.append(flat.clone())
    frozen = PATTERNS["encoders_frozen"][0]
    grads = step(net, inputs(), frozen)[0]
    assert len(seen) == 1
    lay, total = net._bucket_layout()
    flat = seen[0]
    mask = torch.zeros(total, dtype=torch.bool, device=flat.device)
    for n, (o, k) in lay.items():
        if frozen(n):
            assert grads[n] is None
        else:
            mask[o:o + k] = True
            assert bits_equal(flat[o:o + k], grads[n].reshape(-1)), n
    assert torch.count_nonzero(flat[~mask]).item() == 0         # frozen slots and padding: zeros, never stale memory
    seen.clear()
    step(net, inputs(), lambda n: True, (True, False, False))
    assert seen == []                                            # nothing trained: no bucket, no hook


@pytest.mark.parametrize("bf16", [False, True])
def test_deterministic_encoders_frozen(bf16):
    frozen = PATTERNS["encoders_frozen"][0]
    data = inputs()
    a = step(make_net(True, bf16, True), data, frozen)
    b = step(make_net(True, bf16, True), data, frozen)
    check_against_reference(a, b, frozen)


# ------------------------------------------------------------------ (8) a stand-alone layer module
def test_residual_block_frozen_depthwise():
    from nerve_cl.models.layers import ResidualBlock
    torch.manual_seed(0)
    blk = ResidualBlock(32).cuda().train()
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.randn(2, 32, 20, 28, device="cuda")
    tgt = torch.randn(2, 32, 20, 28, device="cuda")

    def run(frozen):
        blk.load_state_dict(state)
        for n, p in blk.named_parameters():
            p.requires_grad_(not frozen(n))
            p.grad = None
        xg = x.clone().requires_grad_()
        F.mse_loss(blk(xg), tgt).backward()
        return {n: p.grad for n, p in blk.named_parameters()}, xg.grad
    ref, rdx = run(lambda n: False)
    for frozen in (lambda n: n == "conv1.depthwise.weight", lambda n: n.endswith("depthwise.weight") or ".bn." in n):
        got, gdx = run(frozen)
        assert bits_equal(gdx, rdx)
        for n, g in got.items():
            assert (g is None) if frozen(n) else bits_equal(g, ref[n]), n
