"""CPU: the argument checks of FrameRecoveryNet's input-gradient entry points (nvq_stem7_dgrad, nvq_mask_blend_backward_ex,
nvq_head_dgrad_tc), refused before anything touches a device."""
import ctypes as C

import pytest

from nerve_cl import _nvq

D = C.c_void_p(256)          # 16-B aligned dummy address: never dereferenced, every call below is refused on the host
D4 = C.c_void_p(260)         # 4-B aligned only


def _stem(Co=32, dy=D, dy_ld=32, dframe=D, dmask=D, N=2, H=37, W=53):
    return _nvq.lib().nvq_stem7_dgrad(dy, dy_ld, 0, D, N, H, W, Co, dframe, dmask, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(Co=8, dy_ld=8), b"Co 8"),
    (dict(Co=24), b"Co 24"),
    (dict(Co=80, dy_ld=80), b"Co 80"),
    (dict(dy_ld=36), b"dy ld 36"),
    (dict(Co=64, dy_ld=32), b"dy ld 32"),
    (dict(dy=D4), b"alignment"),
    (dict(dframe=None, dmask=None), b"NULL dframe and dmask"),
    (dict(dy=None), b"NULL dy"),
    (dict(N=0), b"N 0"),
    (dict(N=70000), b"N 70000"),
])
def test_stem7_dgrad_refuses(kw, msg):
    assert _stem(**kw) == -1
    assert msg in _nvq.lib().nvq_last_error()


def _blend(frame=D, rec=D, rec_ld=4, drec=D, dframe=D, dmask=D, C_=3):
    return _nvq.lib().nvq_mask_blend_backward_ex(D, frame, rec, rec_ld, D, 2, C_, 9, 33, drec, dframe, dmask, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(frame=None), b"dmask needs frame and rec"),
    (dict(rec=None), b"dmask needs frame and rec"),
    (dict(drec=None), b"NULL dout / mask / drec"),
    (dict(C_=5), b"C 5"),
])
def test_mask_blend_backward_ex_refuses(kw, msg):
    assert _blend(**kw) == -1
    assert msg in _nvq.lib().nvq_last_error()


def test_mask_blend_backward_ex_frame_and_rec_only_read_for_dmask():
    """(refused for another reason - N = 0 - only after the NULL checks: frame / rec may be NULL without dmask)"""
    lib = _nvq.lib()
    assert lib.nvq_mask_blend_backward_ex(D, None, None, 4, D, 0, 3, 9, 33, D, D, None, None) == -1
    assert b"N 0" in lib.nvq_last_error()


def _tc(F=32, dout_ld=128, slots=(0, 1, 2, 3), coffs=(0, 32, 64, 96), slot_images=0, T=4, Cin=3):
    return _nvq.lib().nvq_head_dgrad_tc(D, dout_ld, 0, D, F, 2, T, Cin, 9, 33, _nvq.int_array(slots), _nvq.int_array(coffs),
                                        len(slots), slot_images, D, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(Cin=4), b"in_channels 4"),
    (dict(F=24), b"F 24"),
    (dict(dout_ld=132), b"dout ld 132"),
    (dict(coffs=(0, 36, 64, 96)), b"channel offset 36"),
    (dict(coffs=(0, 32, 64, 104)), b"channel offset 104"),
    (dict(coffs=(0, 32, -8, 96)), b"channel offset -8"),
    (dict(slots=(0, 1, 2, 4)), b"maps to frame 4"),
    (dict(slot_images=1), b"slot_images 1"),
    (dict(slots=tuple(range(9)), coffs=(0,) * 9, T=8), b"slots 9"),
])
def test_head_dgrad_tc_refuses(kw, msg):
    assert _tc(**kw) == -1
    assert msg in _nvq.lib().nvq_last_error()
