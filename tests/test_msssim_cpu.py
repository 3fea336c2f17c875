"""CPU: the argument surface of the multi-scale SSIM (nerve_cl.ops.ms_ssim_loss / ms_ssim_l1_loss / MSSSIMLoss,
nerve_cl.metrics.ms_ssim): the weight and scale helpers, every argument error, the refusal of CPU tensors, and the two new
--loss names of the experiment scripts.  No kernel runs here."""
import importlib.util
import os
import sys

import pytest
import torch

from nerve_cl import metrics, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDARD = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
FNS = [ops.ms_ssim_loss, ops.ms_ssim_l1_loss, metrics.ms_ssim, lambda a, b, **k: ops.MSSSIMLoss(**k)(a, b)]
IDS = ["ms_ssim_loss", "ms_ssim_l1_loss", "metrics.ms_ssim", "MSSSIMLoss"]


@pytest.mark.parametrize("scales", [1, 2, 3, 4, 5])
def test_weights_are_the_standard_ones_renormalised(scales):
    w = ops.ms_ssim_weights(scales)
    assert len(w) == scales and all(v > 0 for v in w)
    assert sum(w) == pytest.approx(1.0, abs=1e-12)
    head = STANDARD[:scales]
    for got, std in zip(w, head):
        assert got == pytest.approx(std / sum(head), rel=1e-12)


def test_five_weights_are_the_standard_tuple():
    # the published five sum to 1.0001: dividing by that moves the fourth digit at most
    assert ops.ms_ssim_weights(5) == pytest.approx(STANDARD, rel=2e-4)
    assert ops.MS_SSIM_WEIGHTS == STANDARD
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="scales"):
            ops.ms_ssim_weights(bad)


@pytest.mark.parametrize("hw,want", [((22, 22), 2), ((128, 128), 4), ((175, 400), 4), ((176, 176), 5), ((4000, 4000), 5),
                                     ((400, 175), 4), ((11, 11), 1), ((10, 500), 0)])
def test_max_scales(hw, want):
    assert ops.ms_ssim_max_scales(*hw) == want


@pytest.mark.parametrize("fn", FNS, ids=IDS)
def test_shape_too_small_for_the_weights(fn):
    a = torch.rand(1, 3, 175, 400)
    with pytest.raises(RuntimeError, match="coarsest of 5 scales"):
        fn(a, a)                                            # default: five scales need 176
    b = torch.rand(1, 3, 21, 64)
    with pytest.raises(RuntimeError, match="coarsest of 2 scales"):
        fn(b, b, weights=[0.5, 0.5])
    with pytest.raises(RuntimeError, match="coarsest of 1 scales"):
        fn(b[..., :10, :], b[..., :10, :], weights=[1.0])


@pytest.mark.parametrize("fn", FNS, ids=IDS)
def test_non_4d_tensors(fn):
    a = torch.rand(3, 200, 200)
    with pytest.raises(RuntimeError, match=r"needs \(B, C, H, W\)"):
        fn(a, a)
    with pytest.raises(RuntimeError, match=r"needs \(B, C, H, W\)"):
        fn(a[None, None], a[None, None])


@pytest.mark.parametrize("fn", FNS, ids=IDS)
@pytest.mark.parametrize("weights", [[], [0.5, 0.0], [0.5, -0.5], [float("nan"), 1.0], [float("inf")], [0.1] * 9],
                         ids=["empty", "zero", "negative", "nan", "inf", "nine"])
def test_bad_weights(fn, weights):
    a = torch.rand(1, 1, 64, 64)
    with pytest.raises(ValueError, match="1 to 8 positive"):
        fn(a, a, weights=weights)


@pytest.mark.parametrize("fn", FNS, ids=IDS)
def test_reduction_names(fn):
    a = torch.rand(1, 1, 200, 200)
    for bad in ("sum", "batchmean", None):
        with pytest.raises(ValueError, match="reduction"):
            fn(a, a, reduction=bad)


@pytest.mark.parametrize("fn", FNS, ids=IDS)
def test_cpu_tensors_are_refused(fn):
    a, b = torch.rand(2, 3, 176, 180), torch.rand(2, 3, 176, 180)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(a[..., :40, :40], b[..., :40, :40], weights=[0.3, 0.7], reduction="none")


def test_the_loss_table_keeps_its_four_names():
    assert set(ops.LOSSES) == {"mse", "l1", "charbonnier", "ssim"}


def _script(name):
    sys.path.insert(0, os.path.join(REPO, "experiments"))     # (the scripts import their sibling _common.py)
    spec = importlib.util.spec_from_file_location(f"{name}_script", os.path.join(REPO, "experiments", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script", ["train_baseline", "train_continual"])
def test_the_scripts_accept_the_new_loss_names(script):
    parser = _script(script).build_parser()
    assert parser.parse_args([]).loss == "mse"
    for name in ("ms_ssim", "ms_ssim_l1", "ssim", "l1"):
        assert parser.parse_args(["--loss", name]).loss == name
    with pytest.raises(SystemExit):
        parser.parse_args(["--loss", "vmaf"])


def test_the_scripts_resolve_the_new_names_to_the_multi_scale_losses():
    common = _script("_common")
    assert common.resolve_loss("ssim") is ops.ssim_loss and common.resolve_loss("l1") is ops.l1_loss
    for name in ("ms_ssim", "ms_ssim_l1"):
        fn = common.resolve_loss(name)
        a = torch.rand(2, 3, 128, 128)
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # four scales fit 128 x 128: the shape check passes
            fn(a, a, reduction="none")
