"""CPU: the host side of the deterministic warp mode - the mode switch of SuperResolutionNet, the workspace size formula of
include/nvq.h and the argument checks of nvq_warp_backward_ex (refused before anything touches a device)."""
import ctypes as C

import pytest
import torch

from nerve_cl import _nvq


def test_workspace_formula():
    lib = _nvq.lib()
    for N, H, W in ((1, 9, 33), (8, 540, 960), (2, 21, 45)):
        tiles = N * ((H + 7) // 8) * ((W + 31) // 32)
        assert lib.nvq_warp_backward_workspace_bytes(N, H, W, 1) == 4 * (3 * tiles + 9 * N * H * W)
        assert lib.nvq_warp_backward_workspace_bytes(N, H, W, 0) == 0


def _call(flags, records, overwrite):
    lib = _nvq.lib()
    dummy = C.c_void_p(256)
    return lib.nvq_warp_backward_ex(dummy, 64, 0, dummy, 64, dummy, 4, 64, 1, 9, 33, dummy, 64, dummy, 4, records,
                                    1 << 20, 0, 0, overwrite, 0, flags, dummy, 1 << 20, None)


@pytest.mark.parametrize("records,overwrite", [(None, 1), (C.c_void_p(256), 0), (None, 0)])
def test_deterministic_mode_refuses_scatter_and_accumulate(records, overwrite):
    assert _call(_nvq.WARP_DETERMINISTIC, records, overwrite) != 0
    assert b"deterministic mode exists for the gather form" in _nvq.lib().nvq_last_error()


def test_unknown_flags_are_refused():
    assert _call(2, C.c_void_p(256), 1) != 0
    assert b"unknown flags" in _nvq.lib().nvq_last_error()


def test_mode_switch(monkeypatch):
    from nerve_cl.models import SuperResolutionNet
    from nerve_cl.models.super_resolution import resolve_deterministic
    monkeypatch.delenv("NVQ_DETERMINISTIC", raising=False)
    net = SuperResolutionNet(3, 2, 16, 1, 1)
    assert net.deterministic is None
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert resolve_deterministic(net.deterministic) is False
        torch.use_deterministic_algorithms(True)
        assert resolve_deterministic(net.deterministic) is True
        assert resolve_deterministic(False) is False
    finally:
        torch.use_deterministic_algorithms(prev)
    assert resolve_deterministic(True) is True
    monkeypatch.setenv("NVQ_DETERMINISTIC", "1")
    assert SuperResolutionNet(3, 2, 16, 1, 1).deterministic is True
