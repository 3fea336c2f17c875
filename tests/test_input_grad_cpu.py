"""CPU: the argument checks of nvq_head_dgrad and nvq_bicubic_adjoint (refused before anything touches a device), and the
autograd surface of the SR modules' input gradient that needs no kernel."""
import ctypes as C

import pytest

from nerve_cl import _nvq

D = C.c_void_p(256)          # 16-B aligned dummy address: never dereferenced, every call below is refused on the host


def _dgrad(F=32, Cin=3, dout_ld=32, act=D, dout2=None, slots=(1, 0, 2), T=3):
    lib = _nvq.lib()
    return lib.nvq_head_dgrad(D, dout_ld, 0, dout2, 32, act, 32, 0, D, F, 2, T, Cin, 9, 33, _nvq.int_array(slots),
                              len(slots), D, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(Cin=2), b"in_channels"),
    (dict(F=8), b"F 8"),
    (dict(F=24), b"F 24"),
    (dict(dout_ld=36), b"dout ld"),
    (dict(act=None, dout2=D), b"dout2 needs act"),
    (dict(slots=(0, 1, 3)), b"maps to frame 3"),
])
def test_head_dgrad_refuses(kw, msg):
    assert _dgrad(**kw) == -1
    assert msg in _nvq.lib().nvq_last_error()


@pytest.mark.parametrize("s,tc,msg", [(5, 1, b"scale factor 5"), (0, 1, b"scale factor 0"), (2, 3, b"t_center 3")])
def test_bicubic_adjoint_refuses(s, tc, msg):
    lib = _nvq.lib()
    assert lib.nvq_bicubic_adjoint(D, None, 2, 3, 9, 33, s, 3, tc, 1.0, D, 0, None) == -1
    assert msg in lib.nvq_last_error()
