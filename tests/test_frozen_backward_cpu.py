"""Frozen layers in SuperResolutionNet / LightweightSuperResolution: the backward plan (host only) and the new entry points'
declarations.  GPU behaviour: tests/test_frozen_backward_gpu.py."""
import os
import re

import pytest

from nerve_cl import _engine, _nvq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, T = 2, 3


def _names():
    return [n for _, names in _engine.sr_stages(NB, T) for n in names]


def _stage_names(prefixes):
    return [n for n in _names() if n.startswith(tuple(prefixes))]


ALL_STAGES = [st for st, _ in _engine.sr_stages(NB, T)]


def test_stage_list_covers_every_parameter():
    torch = pytest.importorskip("torch")
    from nerve_cl.models import SuperResolutionNet
    net = SuperResolutionNet(3, 2, 64, NB, 1)
    assert sorted(_names()) == sorted(n for n, _ in net.named_parameters())
    lnames = [n for _, names in _engine.light_stages() for n in names]
    from nerve_cl.models import LightweightSuperResolution
    assert sorted(lnames) == sorted(n for n, _ in LightweightSuperResolution(2).named_parameters())
    del torch


def test_p1_all_trainable():
    p = _engine.backward_plan(_names(), False, NB, T)
    assert p.wgrad == frozenset(_names())
    assert p.dx == frozenset(ALL_STAGES) - {"head"}          # the head's input gradient is the frames' gradient
    assert p.run == frozenset(ALL_STAGES)
    assert _engine.backward_plan(_names(), True, NB, T).dx == frozenset(ALL_STAGES)


def test_p2_alignment_front_end_frozen():
    need = [n for n in _names() if not n.startswith(("feature_extractor.", "motion_estimator."))]
    p = _engine.backward_plan(need, False, NB, T)
    assert p.wgrad == frozenset(need)
    front = {"head", "body.0", "body.1", "body.2", "flow.0", "flow.2", "flow.4", "flow.6"}
    assert not (p.run & front)                               # no extractor, correlation, flow-net or warp backward
    assert "att.0" not in p.dx and "att.2" in p.dx           # the first attention conv: weight gradient only
    assert "att.0" in p.run


def test_p3_head_only():
    need = _stage_names(["gff.", "upsampler."])
    p = _engine.backward_plan(need, False, NB, T)
    assert p.wgrad == frozenset(need)
    assert p.dx == {"up"} and p.run == {"gff", "up"}


def test_p4_all_frozen_frames_need_grad():
    p = _engine.backward_plan([], True, NB, T)
    assert not p.wgrad and p.frames and not p.empty
    assert p.dx == frozenset(ALL_STAGES)
    e = _engine.backward_plan([], False, NB, T)
    assert e.empty and not e.dx and not e.run


def test_p5_frozen_residual_blocks():
    need = [n for n in _names() if not n.startswith("residual_blocks.")]
    p = _engine.backward_plan(need, False, NB, T)
    assert p.wgrad == frozenset(need)
    assert {"rdb.0", "rdb.1"} <= p.dx                         # the input gradient runs through the frozen blocks


def test_p6_frozen_batchnorm_affine():
    need = [n for n in _names() if not re.match(r"feature_extractor\.body\.\d\.bn\.", n)]
    p = _engine.backward_plan(need, False, NB, T)
    assert p.wgrad == frozenset(need)
    assert not any(".bn." in n for n in p.wgrad)
    assert p.run == frozenset(ALL_STAGES)


def test_two_paths_motion_frozen_extractor_trainable():
    need = [n for n in _names() if not n.startswith("motion_estimator.")]
    p = _engine.backward_plan(need, False, NB, T)
    assert not any(n.startswith("motion_estimator.") for n in p.wgrad)
    # the flow net's, warp's and correlation's input gradients still run: the extractor gets gradient through them
    assert {"flow.0", "flow.2", "flow.4", "flow.6", "att.0"} <= p.dx
    assert {"body.0", "body.1", "body.2"} <= p.dx and "head" not in p.dx


def test_motion_trainable_extractor_frozen():
    need = _stage_names(["motion_estimator.flow_net.4", "motion_estimator.flow_net.6"])
    p = _engine.backward_plan(need, False, NB, T)
    assert "flow.4" not in p.dx and "flow.6" in p.dx and "att.0" in p.dx
    assert p.run & {"body.2", "flow.0", "flow.2"} == set()


def test_single_frame_has_no_motion_stage():
    names = [n for _, ns in _engine.sr_stages(NB, 1) for n in ns]
    assert not any(n.startswith("motion_estimator.") for n in names)


def test_light_plan():
    frozen_body = [n for _, ns in _engine.light_stages() for n in ns if n.startswith(("net.0.", "net.6."))]
    p = _engine.light_backward_plan(frozen_body, False)
    assert {"block.0", "block.3"} <= p.dx and "head" not in p.dx
    p = _engine.light_backward_plan(["net.6.weight"], False)
    assert p.run == {"up"} and not p.dx


def test_ex_entry_points_declared():
    with open(os.path.join(REPO, "include", "nvq.h")) as f:
        hdr = f.read()
    assert re.search(r"#define NVQ_NO_WGRAD 2\b", hdr)
    assert _nvq.NO_WGRAD == 2
    for name in ("nvq_pw_bn_backward_ex", "nvq_dwconv_backward_ex", "nvq_cbam_bwd_spatial_conv_ex", "nvq_cbam_bwd_channel_ex"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _nvq.SIGNATURES, name
        full = name[:-3]
        # one more argument than the full form: the flags word before the stream
        assert len(_nvq.SIGNATURES[name][1]) == len(_nvq.SIGNATURES[full][1]) + 1
