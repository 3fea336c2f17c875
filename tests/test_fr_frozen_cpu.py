"""Frozen layers in FrameRecoveryNet: the new BatchNorm backward entry point's declaration and binding.
GPU behaviour: tests/test_fr_frozen_gpu.py."""
import os
import re

from nerve_cl import _nvq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bn2_backward_ex_declared():
    with open(os.path.join(REPO, "include", "nvq.h")) as f:
        hdr = f.read()
    assert re.search(r"#define NVQ_NO_WGRAD 2\b", hdr)
    assert re.search(r"\bint nvq_bn2_backward_ex\(", hdr)
    assert "nvq_bn2_backward_ex" in _nvq.SIGNATURES
    res, args = _nvq.SIGNATURES["nvq_bn2_backward_ex"]
    fres, fargs = _nvq.SIGNATURES["nvq_bn2_backward"]
    # exactly one argument more than the full form: the flags word (an int) just before the stream
    assert res == fres and len(args) == len(fargs) + 1
    assert args[:-2] == fargs[:-1] and args[-1] == fargs[-1]
    assert args[-2] == _nvq.SIGNATURES["nvq_cbam_bwd_channel_ex"][1][-2]       # the int of the other _ex forms' flags


def test_bn2_backward_ex_header_argument_count():
    with open(os.path.join(REPO, "include", "nvq.h")) as f:
        hdr = f.read()

    def nargs(name):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        return len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs("nvq_bn2_backward_ex") == nargs("nvq_bn2_backward") + 1
    assert nargs("nvq_bn2_backward_ex") == len(_nvq.SIGNATURES["nvq_bn2_backward_ex"][1])
