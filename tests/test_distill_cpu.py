"""CPU: the argument surface of the distillation losses (nerve_cl.ops.distill_loss / cosine_feature_loss and their modules),
ContinualDistillation on plain CPU modules (its torch composition against the formula restated here in float64), and the
--strategy distill flags of experiments/train_continual.py.  No kernel runs here."""
import importlib.util
import os
import sys

import pytest
import torch
import torch.nn as nn

from nerve_cl import ops
from nerve_cl.continual import ContinualDistillation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    sys.path.insert(0, os.path.join(REPO, "experiments"))     # (the scripts import their sibling _common.py)
    spec = importlib.util.spec_from_file_location(f"{name}_script", os.path.join(REPO, "experiments", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_script_accepts_the_distill_strategy_and_its_flags():
    parser = _script("train_continual").build_parser()
    d = parser.parse_args([])
    assert d.strategy == "ewc" and d.distill_alpha == 0.5 and d.feature_distill == 0.0
    a = parser.parse_args(["--strategy", "distill", "--distill-alpha", "0.3", "--feature-distill", "0.1", "--loss", "l1"])
    assert a.strategy == "distill" and a.distill_alpha == 0.3 and a.feature_distill == 0.1 and a.loss == "l1"
    with pytest.raises(SystemExit):
        parser.parse_args(["--strategy", "lwf"])


# ------------------------------------------------------------------------------------------------- argument errors (section 2)

DISTILL = [ops.distill_loss, lambda s, t, y=None, **k: ops.DistillLoss(**k)(s, t, y)]
COSINE = [ops.cosine_feature_loss, lambda s, t, **k: ops.CosineFeatureLoss(**k)(s, t)]
IDS = ["function", "module"]


@pytest.mark.parametrize("fn", DISTILL, ids=IDS)
def test_distill_argument_errors_come_before_the_device(fn):
    s = torch.rand(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="shapes differ"):
        fn(s, torch.rand(2, 3, 8, 7))
    with pytest.raises(RuntimeError, match="shapes differ"):
        fn(s, s.clone(), torch.rand(2, 3, 9, 8))
    with pytest.raises(RuntimeError, match="empty"):
        fn(s[:0], s[:0])
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            fn(s, s.clone(), s.clone(), alpha=alpha)
    for bad in ("sum", None):
        with pytest.raises(ValueError, match="reduction"):
            fn(s, s.clone(), reduction=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # every argument is fine: only then the device is asked for
        fn(s, s.clone(), s.clone(), alpha=0.3, reduction="none")


@pytest.mark.parametrize("fn", COSINE, ids=IDS)
def test_cosine_argument_errors_come_before_the_device(fn):
    s = torch.rand(2, 4, 5, 6)
    with pytest.raises(RuntimeError, match=r"needs \(B, C, H, W\)"):
        fn(s[0], s[0])
    with pytest.raises(RuntimeError, match="shapes differ"):
        fn(s, torch.rand(2, 4, 6, 5))
    with pytest.raises(RuntimeError, match="empty"):
        fn(s[:, :0], s[:, :0])
    for eps in (0.0, -1e-8, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            fn(s, s.clone(), eps=eps)
    with pytest.raises(ValueError, match="reduction"):
        fn(s, s.clone(), reduction="sum")
    with pytest.raises(RuntimeError, match="equal length"):
        fn([s, s], [s])
    with pytest.raises(RuntimeError, match="shapes differ"):        # every entry of a list is checked
        fn([s, s], [s.clone(), torch.rand(2, 4, 5, 5)])
    with pytest.raises(TypeError, match="both"):
        fn([s], s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn([s, s], [s.clone(), s.clone()], reduction="none")


def test_return_terms_is_refused_on_cpu_like_the_rest():
    s = torch.rand(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distill_loss(s, s.clone(), return_terms=True)


# ------------------------------------------------------------------------------------------ ContinualDistillation on CPU modules

class TinyNet(nn.Module):
    """(B, 3, H, W) -> (B, 3, H, W) with SuperResolutionNet's return_intermediate signature"""

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 6, 3, padding=1)
        self.b = nn.Conv2d(6, 3, 3, padding=1)

    def forward(self, x, return_intermediate=False):
        f = torch.tanh(self.a(x))
        out = self.b(f)
        if return_intermediate:
            return out, {"aggregated": f, "features": [f[:, :3], 2.0 * f[:, 3:]]}
        return out


def cosine64(s, t, eps=1e-8):
    """the formula of the issue in float64: mean over positions of 1 - ab / (max(sqrt a, eps) max(sqrt b, eps))"""
    s, t = s.double(), t.double()
    a, b, ab = (s * s).sum(1), (t * t).sum(1), (s * t).sum(1)
    ns = torch.maximum(a.sqrt(), torch.tensor(eps, dtype=torch.float64))
    nt = torch.maximum(b.sqrt(), torch.tensor(eps, dtype=torch.float64))
    return (1 - ab / (ns * nt)).mean()


def test_defaults_on_a_plain_module_return_exactly_the_three_keys():
    torch.manual_seed(0)
    model = nn.Conv2d(3, 3, 3, padding=1)
    cd = ContinualDistillation(model)
    x, y = torch.randn(2, 3, 8, 8), torch.randn(2, 3, 8, 8)
    first = cd.compute_loss(x, y, nn.MSELoss())
    assert set(first) == {"task", "distill", "total"} and float(first["distill"]) == 0.0
    cd.register_task()
    with torch.no_grad():
        model.weight.add_(0.05)
    losses = cd.compute_loss(x, y, nn.MSELoss())
    assert set(losses) == {"task", "distill", "total"}
    assert all(v.requires_grad for v in losses.values())
    with torch.no_grad():
        s, t = model(x).double(), cd.teacher(x).double()
    d, m = ((s - t) ** 2).mean(), ((s - y.double()) ** 2).mean()
    assert losses["task"].item() == pytest.approx(float(m), rel=1e-5)
    assert losses["distill"].item() == pytest.approx(float(0.5 * d + 0.5 * m), rel=1e-5)
    assert losses["total"].item() == pytest.approx(float(m + 0.5 * d + 0.5 * m), rel=1e-5)


def test_feature_weight_on_a_cpu_module_matches_the_float64_formula():
    torch.manual_seed(1)
    model = TinyNet()
    cd = ContinualDistillation(model, alpha=0.3, feature_weight=0.5, feature_keys=("features", "aggregated"))
    x, y = torch.randn(2, 3, 6, 7), torch.randn(2, 3, 6, 7)
    before = cd.compute_loss(x, y, nn.MSELoss())
    assert set(before) == {"task", "distill", "total", "feature"} and float(before["feature"]) == 0.0
    cd.register_task()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn_like(p))
    losses = cd.compute_loss(x, y, nn.MSELoss())
    assert set(losses) == {"task", "distill", "total", "feature"}

    ref_model = TinyNet().double()
    ref_model.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    s, si = ref_model(x.double(), return_intermediate=True)
    with torch.no_grad():
        t, ti = cd.teacher.double()(x.double(), return_intermediate=True)
    d, m = ((s - t) ** 2).mean(), ((s - y.double()) ** 2).mean()
    feat = (cosine64(si["features"][0], ti["features"][0]) + cosine64(si["features"][1], ti["features"][1])) / 2 \
        + cosine64(si["aggregated"], ti["aggregated"])
    total = m + 0.3 * d + 0.7 * m + 0.5 * feat
    assert losses["feature"].item() == pytest.approx(feat.item(), rel=1e-5)
    assert losses["total"].item() == pytest.approx(total.item(), rel=1e-5)
    losses["total"].backward()
    total.backward()
    for (n, p), q in zip(model.named_parameters(), ref_model.parameters()):
        err = (p.grad.double() - q.grad).norm() / q.grad.norm()
        assert err < 1e-4, (n, float(err))


def test_fold_task_refuses_other_criteria():
    cd = ContinualDistillation(nn.Conv2d(3, 3, 1), fold_task=True)
    x = torch.randn(1, 3, 4, 4)
    for crit in (nn.L1Loss(), nn.MSELoss(reduction="sum"), ops.L1Loss(), ops.l1_loss):
        with pytest.raises(ValueError, match="fold_task"):
            cd.compute_loss(x, x, crit)
    cd.register_task()
    with pytest.raises(ValueError, match="fold_task"):
        cd.compute_loss(x, x, nn.L1Loss())
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the right criterion: the folded kernel has no CPU form
        cd.compute_loss(x, x, nn.MSELoss())
