"""GPU: gradients through SuperResolutionNet.forward(x, return_intermediate=True)'s `features`, `aligned` and `aggregated`
(reference super_resolution.py:327-391: those tensors are part of the autograd graph, a loss on them trains the network).
Against CPU autograd through the pure-torch oracle on the closed-form weights and clips of oracle/synth.py; also the two
kernels behind it (nvq_gather_nchw, nvq_inject_nchw) on their own.
Tolerances as in test_input_grad_gpu.py: fp32 at 1e-3 of the reference tensor's max magnitude (per parameter, per frame);
the bf16 throughput mode against a float64 oracle by gradient cosine (flow net apart) and relative L2."""
import pytest
import torch
import torch.nn.functional as F

from oracle import sr_oracle, synth

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


def flat(inter):
    """the intermediates in the order features[0 .. T-1], aligned[0 .. T-1], aggregated"""
    return list(inter["features"]) + list(inter["aligned"]) + [inter["aggregated"]]


def weights(T, B, Fc, H, W, seed=5):
    """fixed weights W_k of the intermediates' loss terms <W_k, inter_k>, of the size of the mse term's output gradient"""
    n = B * Fc * H * W
    return [torch.from_numpy(synth.hash01(n, seed + k).reshape(B, Fc, H, W)).float().sub(0.5).mul(4.0 / n)
            for k in range(2 * T + 1)]


def make_loss(Ws, use_out=True, which=None):
    """mse(out, tgt) (use_out) + sum of <W_k, inter_k> over the intermediates `which` (indices into flat(); None: all)"""
    def loss(out, inter, tgt):
        total = F.mse_loss(out, tgt.to(out)) if use_out else 0.0
        for k, t in enumerate(flat(inter)):
            if which is None or k in which:
                total = total + (Ws[k].to(t) * t).sum()
        return total
    return loss


def hip_grads(net, x, tgt, loss, frames_grad=True):
    xg = x.cuda().requires_grad_(frames_grad)
    out, inter = net(xg, return_intermediate=True)
    loss(out, inter, tgt.cuda()).backward()
    return {n: p.grad for n, p in net.named_parameters() if p.requires_grad}, xg.grad


def oracle_grads(ora, x, tgt, loss):
    xo = x.clone().requires_grad_()
    out, inter = ora(xo, return_intermediate=True)
    loss(out, inter, tgt).backward()
    named = ora.named()
    grads = {n: (named[n].grad if named[n].grad is not None else torch.zeros_like(named[n])) for n in ora._names}
    return grads, xo.grad


def float64_of(ora, x, tgt, loss):
    """the same gradients from the oracle in float64 (after the fp32 pass: the oracle's gradients are cleared first)"""
    def run():
        ora.zero_grad(set_to_none=True)
        return oracle_grads(ora.double(), x.double(), tgt, loss)
    return run


def check_fp32(g, gx, og, ogx, T, what, f64=None):
    """Every gradient within REL (max-normalised) of the fp32 oracle - or, for a tensor that is not, ATTRIBUTED with the float64
    oracle as in test_real_size_gpu.py: the HIP gradient at most 4x as far from the float64 gradient as the fp32 CPU oracle
    itself is (+ 2e-5), and within 5e-2 of the fp32 oracle.  In training mode a loss on the features reaches the BatchNorm
    backward, whose mean subtraction cancels most of that gradient: a few small tensors (BatchNorm biases, the first flow conv's
    bias, a frame's gradient) are then ill-conditioned in fp32, and an ordering or slot defect would put the HIP gradient far
    from float64 where the CPU oracle is close."""
    rows = [(n, g[n], og[n]) for n in g] + ([(f"frames[{t}]", gx[:, t], ogx[:, t]) for t in range(T)] if gx is not None else [])
    errs = {n: rel(a, b) for n, a, b in rows}
    worst = max(errs, key=errs.get) if errs else None
    print(f"  {what}: worst rel {errs.get(worst, 0.0):.1e} ({worst})")
    over = [(n, a) for n, a, _ in rows if errs[n] >= REL]
    if not over:
        return
    assert f64 is not None, (worst, errs[worst])
    og64, ogx64 = f64()
    failed = []
    for n, a in over:
        ref = ogx64[:, int(n[7:-1])] if n.startswith("frames[") else og64[n]
        r = ogx[:, int(n[7:-1])] if n.startswith("frames[") else og[n]
        hip_e, ora_e = rel(a, ref), rel(r, ref)
        row = f"{n}: vs fp32 oracle {errs[n]:.2e}; vs float64: HIP {hip_e:.2e}, CPU fp32 {ora_e:.2e}"
        print("    attributed", row)
        if not (hip_e <= 4 * ora_e + 2e-5 and errs[n] < 5e-2):
            failed.append(row)
    assert not failed, failed


# ------------------------------------------------------------------ (1) the kernels on their own
@pytest.mark.parametrize("Fc", [16, 32, 64, 128])
@pytest.mark.parametrize("H,W", [(37, 53), (16, 24), (20, 26)])
def test_gather_kernel_bit_exact(Fc, H, W):
    from nerve_cl import _nvq
    from nerve_cl._nvq import Sl
    N = 3
    g = torch.Generator().manual_seed(Fc + H)
    srcs = [torch.randn(N, H, W, Fc, generator=g),                          # compact fp32
            torch.randn(N, H, W, 3 * Fc, generator=g),                      # fp32, ld > F, channel offset
            torch.randn(N, H, W, Fc + 16, generator=g).bfloat16(),          # bf16, ld > F, offset 8
            torch.randn(N, H, W, 2 * Fc, generator=g).bfloat16()]           # bf16, offset F
    sls = [Sl(srcs[0].cuda()), Sl(srcs[1].cuda(), Fc, 2 * Fc), Sl(srcs[2].cuda(), Fc, 8), Sl(srcs[3].cuda(), Fc, Fc)]
    outs = [torch.full((N, Fc, H, W), float("nan"), device="cuda") for _ in sls]
    _nvq.gather_nchw(list(zip(sls, outs)))
    for sl, o in zip(sls, outs):
        ref = sl.t[..., sl.coff:sl.coff + Fc].permute(0, 3, 1, 2).contiguous().float()
        assert torch.equal(o, ref)


@pytest.mark.parametrize("Fc", [16, 32, 64, 128])
@pytest.mark.parametrize("H,W", [(37, 53), (16, 24)])
def test_inject_kernel_sums_in_order(Fc, H, W):
    from nerve_cl import _nvq
    from nerve_cl._nvq import Sl
    N = 2
    g = torch.Generator().manual_seed(7 * Fc + W)
    d32 = torch.randn(N, H, W, 2 * Fc, generator=g).cuda()
    d16 = torch.randn(N, H, W, Fc + 8, generator=g).bfloat16().cuda()
    s = [torch.randn(N, Fc, H, W, generator=g).cuda() for _ in range(3)]
    # fp32 slice at offset F: ((dst + s0) + s1); bf16 slice at offset 8: (dst + s2), None skipped; all in one launch
    runs = []
    for _ in range(2):
        a, b = d32.clone(), d16.clone()
        _nvq.inject_nchw([(Sl(a, Fc, Fc), [s[0], None, s[1]]), (Sl(b, Fc, 8), [None, s[2]])])
        runs.append((a, b))
    nhwc = lambda t: t.permute(0, 2, 3, 1)   # noqa: E731
    want32 = d32.clone()
    want32[..., Fc:] = (d32[..., Fc:] + nhwc(s[0])) + nhwc(s[1])
    want16 = d16.clone()
    want16[..., 8:8 + Fc] = (d16[..., 8:8 + Fc].float() + nhwc(s[2])).bfloat16()       # summed in fp32, rounded once
    assert torch.equal(runs[0][0], want32) and torch.equal(runs[0][1], want16)
    assert torch.equal(runs[1][0], runs[0][0]) and torch.equal(runs[1][1], runs[0][1])
    # only null sources: nothing changes
    a = d32.clone()
    _nvq.inject_nchw([(Sl(a, Fc, 0), [None, None])])
    assert torch.equal(a, d32)


# ------------------------------------------------------------------ (2) exact-fp32 mode, every gradient
# (The sizes avoid 24x32 and 24x40 with these weights and clips: there the HIP forward already sits on a ReLU / warp-cell
# boundary the CPU oracle does not, and a loss on `out` alone is up to 1.5e-2 (24x32, attention.0.weight) and 1.8e-4 (24x40,
# flow_net.0) from the float64 gradient where the fp32 CPU oracle is within 1e-6 - with or without this feature.)
@pytest.mark.parametrize("s,T,H,W,train", [
    (2, 3, 19, 26, True), (2, 5, 37, 53, False), (3, 3, 37, 53, True), (3, 5, 20, 28, False),
    (4, 3, 37, 53, False), (4, 5, 17, 23, True)])
def test_fp32_combined_loss_vs_oracle(s, T, H, W, train):
    B, Fc = 2, 32
    net, ora = sr_pair(Fc, 2, T // 2, s, train)
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W))
    g, gx = hip_grads(net, x, tgt, loss)
    og, ogx = oracle_grads(ora, x, tgt, loss)
    check_fp32(g, gx, og, ogx, T, f"fp32 s{s} T{T} {H}x{W} {'train' if train else 'eval'}", float64_of(ora, x, tgt, loss))


@pytest.mark.parametrize("win,NB", [(0, 2), (1, 0), (0, 0)])
def test_fp32_single_frame_and_no_dense_blocks(win, NB):
    """T = 1 (no motion path) and no dense blocks (the gff input gradient is the aggregated features' gradient)"""
    B, Fc, s, H, W = 2, 32, 2, 21, 30
    T = 2 * win + 1
    net, ora = sr_pair(Fc, NB, win, s, True)
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W))
    g, gx = hip_grads(net, x, tgt, loss)
    og, ogx = oracle_grads(ora, x, tgt, loss)
    check_fp32(g, gx, og, ogx, T, f"fp32 T{T} NB{NB}", float64_of(ora, x, tgt, loss))


# ------------------------------------------------------------------ (3) one intermediate at a time (no output gradient)
@pytest.mark.parametrize("name", ["features_c", "features_other", "aligned_c", "aligned_other", "aggregated"])
@pytest.mark.parametrize("T", [3, 5])
def test_fp32_one_intermediate(name, T):
    B, Fc, s, H, W = 2, 32, 2, 19, 26
    c = T // 2
    k = {"features_c": c, "features_other": 0, "aligned_c": T + c, "aligned_other": T + T - 1, "aggregated": 2 * T}[name]
    net, ora = sr_pair(Fc, 2, T // 2, s, True)
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W), use_out=False, which={k})
    g, gx = hip_grads(net, x, tgt, loss)
    og, ogx = oracle_grads(ora, x, tgt, loss)
    check_fp32(g, gx, og, ogx, T, f"fp32 {name} T{T}", float64_of(ora, x, tgt, loss))


# ------------------------------------------------------------------ (4) bf16 throughput mode against float64
@pytest.fixture(scope="module")
def bf16_case():
    B, T, Fc, NB, s, H, W = 1, 3, 32, 2, 2, 64, 64
    x = synth.formula_clip(B, T, H, W, seed=13)
    tgt = synth.formula_target(B, H * s, W * s, seed=14)
    loss = make_loss(weights(T, B, Fc, H, W))
    _, ora = sr_pair(Fc, NB, 1, s, True)
    og32, ogx32 = oracle_grads(ora, x, tgt, loss)
    _, ora = sr_pair(Fc, NB, 1, s, True)
    og64, ogx64 = oracle_grads(ora.double(), x.double(), tgt, loss)
    return dict(x=x, tgt=tgt, loss=loss, args=(Fc, NB, 1, s, True), og32=og32, ogx32=ogx32, og64=og64, ogx64=ogx64)


def cosines(g, og):
    cos_min, at, dot, na, nb = 1.0, None, 0.0, 0.0, 0.0
    for n in g:
        a, b = g[n].detach().double().cpu().reshape(-1), og[n].double().reshape(-1)
        dot += float(a @ b); na += float(a @ a); nb += float(b @ b)
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))
        if "motion_estimator" not in n and cos < cos_min:
            cos_min, at = cos, n
    return cos_min, at, dot / max(na * nb, 1e-300) ** 0.5


BF16_FRAMES_CAP = 0.30     # the cap of test_input_grad_gpu.py's 64x64 bf16 case


@pytest.mark.parametrize("flag", ["NVQ_BF16_FEATURES", "NVQ_BF16_FEATURE_GRAD", "NVQ_BF16_CBAM", "NVQ_PLANAR"])
@pytest.mark.parametrize("value", ["0", "1"])
def test_bf16_combined_loss_vs_float64(bf16_case, monkeypatch, flag, value):
    monkeypatch.setenv(flag, value)
    d = bf16_case
    net, _ = sr_pair(*d["args"], bf16=True)
    g, gx = hip_grads(net, d["x"], d["tgt"], d["loss"])
    cos_min, at, whole = cosines(g, d["og64"])
    e_hip, e_ora = rel_l2(gx, d["ogx64"]), rel_l2(d["ogx32"], d["ogx64"])
    print(f"  bf16 {flag}={value}: min non-flow gradient cosine {cos_min:.5f} at {at}, whole {whole:.6f}; frames rel L2 "
          f"{e_hip:.2e} (fp32 oracle {e_ora:.2e})")
    assert cos_min > 0.98 and whole > 0.995
    assert e_hip <= 4 * e_ora + BF16_FRAMES_CAP


# ------------------------------------------------------------------ (5) no change when the intermediates get no gradient
@pytest.mark.parametrize("bf16", [False, True])
def test_unused_intermediates_change_nothing(bf16):
    x = synth.formula_clip(2, 3, 37, 53)
    tgt = synth.formula_target(2, 74, 106)
    runs = []
    for want in (False, True):
        net, _ = sr_pair(32, 2, 1, 2, True, bf16=bf16)
        net.deterministic = True
        xg = x.cuda().requires_grad_()
        res = net(xg, return_intermediate=want)
        out = res[0] if want else res
        if want:
            assert all(t.requires_grad and t.dtype == torch.float32 for t in flat(res[1]))
        F.mse_loss(out, tgt.cuda()).backward()
        runs.append(({n: p.grad.clone() for n, p in net.named_parameters()}, xg.grad.clone()))
    for n in runs[0][0]:
        assert torch.equal(runs[0][0][n], runs[1][0][n]), n
    assert torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ (6) frozen layers and frames
def test_only_feature_extractor_trained_loss_on_aggregated():
    B, T, Fc, s, H, W = 2, 3, 32, 2, 23, 31
    net, ora = sr_pair(Fc, 2, 1, s, True)
    for n, p in net.named_parameters():
        p.requires_grad_(n.startswith("feature_extractor."))
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W), use_out=False, which={2 * T})
    g, gx = hip_grads(net, x, tgt, loss, frames_grad=False)
    assert gx is None and set(g) == {n for n, _ in net.named_parameters() if n.startswith("feature_extractor.")}
    assert all(p.grad is None for n, p in net.named_parameters() if not n.startswith("feature_extractor."))
    og, _ = oracle_grads(ora, x, tgt, loss)
    check_fp32(g, None, og, None, T, "feature extractor only, loss on aggregated", float64_of(ora, x, tgt, loss))


def test_frozen_parameters_frames_grad_loss_on_aligned():
    B, T, Fc, s, H, W = 2, 3, 32, 2, 23, 31
    net, ora = sr_pair(Fc, 2, 1, s, True)
    for p in net.parameters():
        p.requires_grad_(False)
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W), use_out=False, which=set(range(T, 2 * T)))
    g, gx = hip_grads(net, x, tgt, loss)
    assert not g and all(p.grad is None for p in net.parameters())
    _, ogx = oracle_grads(ora, x, tgt, loss)
    check_fp32({}, gx, {}, ogx, T, "frozen parameters, loss on aligned", float64_of(ora, x, tgt, loss))


# ------------------------------------------------------------------ (7) modes
@pytest.mark.parametrize("bf16", [False, True])
def test_deterministic_steps_bit_identical(bf16):
    B, T, Fc, s, H, W = 2, 3, 64, 2, 48, 64
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W))
    runs = []
    for _ in range(2):
        net, _ = sr_pair(Fc, 2, 1, s, True, bf16=bf16)
        net.deterministic = True
        g, gx = hip_grads(net, x, tgt, loss)
        runs.append(({n: t.clone() for n, t in g.items()}, gx.clone()))
    for n in runs[0][0]:
        assert torch.equal(runs[0][0][n], runs[1][0][n]), n
    assert torch.equal(runs[0][1], runs[1][1])


def test_hip_graphs_with_intermediates_run_eagerly():
    """use_hip_graphs=True: a step that returns intermediates is never captured (frames without a gradient, so that only
    return_intermediate keeps it eager), and its gradients stay right"""
    B, T, Fc, s, H, W = 2, 3, 32, 2, 24, 32
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W))
    net, ora = sr_pair(Fc, 1, 1, s, True)
    net.deterministic = True
    ref, _ = hip_grads(net, x, tgt, loss, frames_grad=False)
    ref = {n: t.clone() for n, t in ref.items()}
    net.use_hip_graphs = True
    for _ in range(4):                                        # past the graph warm-up: still no graph for this step
        net.zero_grad(set_to_none=True)
        g, _ = hip_grads(net, x, tgt, loss, frames_grad=False)
        for n in ref:
            assert torch.equal(g[n], ref[n]), n
    assert len(net._step_graphs.entries) == 0
    og, _ = oracle_grads(ora, x, tgt, loss)
    check_fp32(g, None, og, None, T, "use_hip_graphs=True", float64_of(ora, x, tgt, loss))


def test_retain_backward_state_two_grads():
    B, T, Fc, s, H, W = 2, 3, 32, 2, 19, 26
    x = synth.formula_clip(B, T, H, W)
    tgt = synth.formula_target(B, H * s, W * s)
    loss = make_loss(weights(T, B, Fc, H, W))
    net, ora = sr_pair(Fc, 2, 1, s, True)
    net.deterministic = True
    net.retain_backward_state = True
    xg = x.cuda().requires_grad_()
    out, inter = net(xg, return_intermediate=True)
    total = loss(out, inter, tgt.cuda())
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    g1 = [t.clone() for t in torch.autograd.grad(total, [xg] + params, retain_graph=True)]
    g2 = [t.clone() for t in torch.autograd.grad(total, [xg] + params)]
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    og, ogx = oracle_grads(ora, x, tgt, loss)
    check_fp32(dict(zip(names, g2[1:])), g2[0], og, ogx, T, "retain_backward_state, second grad", float64_of(ora, x, tgt, loss))
