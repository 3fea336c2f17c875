"""GPU: the libnvq launch sequence of the five flat-bucket consumers (AGEM.project, ops.clip_grad_norm_, BucketAdamW with
max_grad_norm, SynapticIntelligence.update_importance) in the two gradient states the shared layer of nerve_cl/_bucket.py tells
apart, and the equivalence of the two routes.

Aliasing state (zero_grad -> ONE backward): every ``.grad`` of a bucketed network is the view of its last gradient bucket; a
consumer launches once over the whole bucket per network plus once per loose parameter that carries a gradient.
Accumulated state (two backwards): autograd replaced ``.grad`` by sums, nothing aliases; one launch per parameter with a gradient.
The expected sequences are computed here from ``_bucket_layout()`` and the parameter list.

Equivalence.  csrc/bucket_ops.hip: ``bucket_moments_kernel`` sums per block of ``flat_blocks(n)`` blocks and the final kernel
adds the block partials, so g.r / r.r / g.g over ONE bucket and over 47 tensors chained with ``accumulate`` are double sums of the
same exact products in a different order: they MAY differ in their last bits, for all three consumers that read them (project:
c = g.r / r.r; clip and nvq_adam_step: coef = max_norm / (sqrt(g.g) + 1e-6)).  ``bucket_project_kernel``, ``bucket_clip_kernel``
and ``adam_element`` (csrc/optim.hip) are per element and read the sums only: equal sums give equal bits.  So each comparison
asserts bit equality when the two routes' sums are bit-equal, and otherwise the bound of test_agem_gpu.py::_check_projection
(projection) resp. its clipping bound 4 * 2^-24 |g| (clip); the optimizer's bound is derived at ``_adam_bound``.
nvq_si_update reads no sums: it is per element, hence bit-equal always."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EPS24 = 2.0 ** -24
CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B, H, W = 2, 16, 24
RECORDED = ("bucket_moments", "bucket_project", "bucket_clip", "adam_step", "si_update", "fisher_accumulate", "ewc_penalty_grad")
LR = 1e-3


def _dev():
    return torch.device("cuda", 0)


def _engine():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    eng = eng.to(_dev()).train()
    eng.super_resolution.deterministic = True
    return eng


def _data():
    from oracle import synth
    x, y = synth.formula_clip(B, 3, H, W), synth.formula_target(B, 2 * H, 2 * W)
    return x.to(_dev()), y.to(_dev())


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _flat_grads(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])


def _aliased(net) -> bool:
    mask = net.grad_alias_mask()
    return mask is not None and all(mask)


def _by_segment(agem, grads: bool):
    """the gradients (or AGEM's reference slices) of the parameters that carry a gradient, in segment order"""
    out = []
    for sg, ref in zip(agem._segs, agem._ref):
        views = sg.views(ref)
        out += [(p.grad if grads else views[n]).reshape(-1) for n, p in sg.named if p.grad is not None]
    return torch.cat(out).clone()


def _backward(eng, x, y, sign=1.0, backwards=1, mix=0.5):
    """the loss of test_agem_gpu.py::_conflict_step; the forward reads enhancement_strength with .item(), so the last term is what
    gives this loose parameter a gradient"""
    eng.zero_grad()
    for _ in range(backwards):
        out = eng(x)["enhanced"]
        (sign * F.mse_loss(out, y) + mix * F.mse_loss(out, y.flip(0) * 0.5)
         + sign * 1e-3 * (eng.enhancement_strength ** 2).sum()).backward()


def _to_clones(eng):
    """the same gradient values outside the bucket: every consumer takes its per-tensor route"""
    for p in eng.parameters():
        if p.grad is not None:
            p.grad = p.grad.clone()


class _Recorder:
    """(name, numel of the first tensor argument) of every recorded _nvq call; ``clip_acc``: the acc argument of the last
    bucket_clip call (clip_grad_norm_ keeps its own to itself)"""

    def __init__(self, monkeypatch):
        from nerve_cl import _nvq
        self.calls, self.clip_acc = [], None
        for name in RECORDED:
            monkeypatch.setattr(_nvq, name, self._wrap(name, getattr(_nvq, name)))

    def _wrap(self, name, fn):
        def wrapped(first, *args, **kw):
            self.calls.append((name, first.numel()))
            if name == "bucket_clip":
                self.clip_acc = args[0]
            return fn(first, *args, **kw)
        return wrapped

    def take(self):
        out, self.calls = self.calls, []
        return out


def _expected_sizes(eng, aliasing: bool, whole_bucket: bool):
    """numel of the gradient each launch reads, in launch order: the bucketed networks in module order, then the loose parameters.
    ``whole_bucket``: the launch covers the bucket's padding behind the last slot too (the segment consumers); the optimizer's
    run ends with the last slot."""
    from nerve_cl._bucket import BucketedNet
    nets = [m for m in eng.modules() if isinstance(m, BucketedNet)]
    inside = {id(p) for net in nets for p in net.parameters()}
    sizes = []
    for net in nets:
        lay, total = net._bucket_layout()
        if aliasing:
            sizes.append(total if whole_bucket else max(o + k for o, k in lay.values()))
        else:
            sizes += [p.numel() for _, p in net.named_parameters() if p.grad is not None and p.numel()]
    sizes += [p.numel() for p in eng.parameters() if id(p) not in inside and p.grad is not None and p.numel()]
    return sizes


def _steps(rec, backwards: int, clones: bool = False):
    """One step of each consumer on a fresh engine each -> {consumer: (launches, results...)}"""
    from nerve_cl import ops
    from nerve_cl.continual import AGEM, SynapticIntelligence
    from nerve_cl.optim import BucketAdamW
    x, y = _data()
    aliasing = backwards == 1 and not clones
    out = {}

    def prepare(eng):
        _backward(eng, x, y, -1.0, backwards)
        assert _aliased(eng.super_resolution) == (backwards == 1)
        if clones:
            _to_clones(eng)
            assert not _aliased(eng.super_resolution)
        rec.take()

    eng = _engine()
    agem = AGEM(eng)
    _backward(eng, x, y, 1.0, mix=0.0)
    agem.capture_reference()
    prepare(eng)
    g0, r = _by_segment(agem, True), _by_segment(agem, False)
    agem.project()
    sizes = _expected_sizes(eng, aliasing, True)
    out["agem"] = dict(calls=rec.take(), want=[("bucket_moments", n) for n in sizes] + [("bucket_project", n) for n in sizes],
                       g0=g0, r=r, g1=_by_segment(agem, True), sums=agem.stats[:3].clone())
    assert agem.num_projections() == 1 and _aliased(eng.super_resolution) == aliasing

    eng = _engine()
    prepare(eng)
    g0 = _flat_grads(eng).clone()
    max_norm = 0.5 * g0.double().norm().item()
    norm = ops.clip_grad_norm_(eng, max_norm)
    sizes = _expected_sizes(eng, aliasing, True)
    out["clip"] = dict(calls=rec.take(), want=[("bucket_moments", n) for n in sizes] + [("bucket_clip", n) for n in sizes],
                       g0=g0, g1=_flat_grads(eng).clone(), norm=norm.clone(), max_norm=max_norm, sums=rec.clip_acc[:3].clone())
    assert _aliased(eng.super_resolution) == aliasing

    eng = _engine()
    opt = BucketAdamW(eng.parameters(), lr=LR, max_grad_norm=max_norm)
    prepare(eng)
    theta0 = torch.cat([p.detach().reshape(-1) for p in eng.parameters()]).clone()
    opt.step()
    sizes = _expected_sizes(eng, aliasing, False)
    out["adam"] = dict(calls=rec.take(), want=[("bucket_moments", n) for n in sizes] + [("adam_step", n) for n in sizes],
                       theta0=theta0, theta1=torch.cat([p.detach().reshape(-1) for p in eng.parameters()]).clone(),
                       sums=opt._acc[2:3].clone(), launches=opt.last_launches)

    eng = _engine()
    si = SynapticIntelligence(eng)
    prepare(eng)
    with torch.no_grad():
        for p in eng.parameters():
            p.mul_(1.0 + 2.0 ** -6)                       # theta - p_old != 0 without an optimizer: W moves
    si.update_importance()
    out["si"] = dict(calls=rec.take(), want=[("si_update", n) for n in _expected_sizes(eng, aliasing, True)],
                     W=torch.cat([si.W[n].reshape(-1) for n in sorted(si.W)]).clone())
    return out


@pytest.fixture(scope="module")
def runs():
    mp = pytest.MonkeyPatch()
    try:
        rec = _Recorder(mp)
        yield {"aliasing": _steps(rec, 1), "accumulated": _steps(rec, 2), "clones": _steps(rec, 1, clones=True), "eng": _engine()}
    finally:
        mp.undo()


@pytest.mark.parametrize("consumer", ["agem", "clip", "adam", "si"])
@pytest.mark.parametrize("state", ["aliasing", "accumulated"])
def test_launch_sequence(runs, state, consumer):
    got = runs[state][consumer]
    assert got["calls"] == got["want"]
    n = len(got["want"]) // (1 if consumer == "si" else 2)
    nparams = sum(1 for _ in runs["eng"].parameters())
    assert n == (2 if state == "aliasing" else nparams)     # the SR bucket and enhancement_strength / every parameter
    if consumer == "adam":
        assert got["launches"] == n


def _check_projection(g0, r, g1, c):
    """tests/test_agem_gpu.py::_check_projection"""
    gd, rd = g0.double(), r.double()
    err = (g1.double() - (gd - c * rd)).abs()
    assert bool((err <= 4 * EPS24 * (gd.abs() + (c * rd).abs())).all())
    assert abs((g1.double() * rd).sum().item()) <= 8 * EPS24 * (gd.norm() * rd.norm()).item()


def test_projection_is_the_same_on_both_routes(runs):
    a, b = runs["aliasing"]["agem"], runs["clones"]["agem"]
    assert torch.equal(_bits(a["g0"]), _bits(b["g0"])) and torch.equal(_bits(a["r"]), _bits(b["r"]))
    assert len(b["want"]) > len(a["want"])                  # the second engine went per tensor
    if torch.equal(a["sums"], b["sums"]):
        assert torch.equal(_bits(a["g1"]), _bits(b["g1"]))
    gr, rr = (a["g0"].double() * a["r"].double()).sum().item(), (a["r"].double() ** 2).sum().item()
    assert gr < 0
    for run in (a, b):
        _check_projection(run["g0"], run["r"], run["g1"], gr / rr)


def test_clipping_is_the_same_on_both_routes(runs):
    a, b = runs["aliasing"]["clip"], runs["clones"]["clip"]
    assert torch.equal(_bits(a["g0"]), _bits(b["g0"])) and a["max_norm"] == b["max_norm"]
    assert len(b["want"]) > len(a["want"])                  # the second engine went per tensor
    if torch.equal(a["sums"], b["sums"]):
        assert torch.equal(_bits(a["g1"]), _bits(b["g1"])) and torch.equal(_bits(a["norm"]), _bits(b["norm"]))
    norm64 = a["g0"].double().norm().item()
    want = a["g0"].double() * (a["max_norm"] / (norm64 + 1e-6))
    for run in (a, b):                                      # the clipping bound of test_agem_gpu.py
        assert bool(((run["g1"].double() - want).abs() <= 4 * EPS24 * a["g0"].double().abs()).all())
        assert abs(run["norm"].item() - norm64) <= 2.0 ** -23 * norm64


def _adam_bound(theta0):
    """|theta_a - theta_b| when the two routes' g.g differ in their last bits: coef differs by at most one fp32 rounding
    (2^-24 relative after the cast), so the clipped gradient differs by 2^-23 relative at most.  In the first step
    m / denom = g / (|g| + eps') up to the kernel's nine fp32 roundings, a function of slope <= 1 in relative terms and of
    magnitude <= 1, so the two updates differ by at most (2 + 2 * 9) * 2^-24 * lr, rounded up to 32; the final fma rounds
    theta once on each route, 2 * 2^-24 |theta|."""
    return 2 * EPS24 * theta0.double().abs() + 32 * EPS24 * LR


def test_adam_step_is_the_same_on_both_routes(runs):
    a, b = runs["aliasing"]["adam"], runs["clones"]["adam"]
    assert torch.equal(_bits(a["theta0"]), _bits(b["theta0"]))
    assert a["launches"] == 2 and b["launches"] == len(b["want"]) // 2 > 2
    assert not torch.equal(a["theta0"], a["theta1"])
    if torch.equal(a["sums"], b["sums"]):
        assert torch.equal(_bits(a["theta1"]), _bits(b["theta1"]))
    assert bool(((a["theta1"].double() - b["theta1"].double()).abs() <= _adam_bound(a["theta0"])).all())


def test_flat_grad_copies_what_the_fp32_kernels_cannot_take():
    """the GPU half of test_bucket_layer_cpu.py's flat_grad test: here a float64 gradient is NOT taken as it is"""
    from nerve_cl._bucket import flat_grad
    g = torch.randn(6, 4, device=_dev())
    flat, dst = flat_grad(g)
    assert dst is None and flat.data_ptr() == g.data_ptr() and flat.shape == (24,)
    for other in (g.double(), g.t()):
        flat, dst = flat_grad(other)
        assert dst.data_ptr() == other.data_ptr() and dst.dtype == other.dtype and dst.stride() == other.stride()
        assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.data_ptr() != other.data_ptr()
        assert torch.equal(flat, other.float().contiguous().view(-1))


def test_si_update_is_the_same_on_both_routes(runs):
    a, b = runs["aliasing"]["si"], runs["clones"]["si"]
    assert len(a["want"]) == 2 and len(b["want"]) > 2
    assert a["W"].abs().max() > 0
    assert torch.equal(_bits(a["W"]), _bits(b["W"]))
