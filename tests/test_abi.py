"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/pfst_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os

import pytest

from pfst_amd import _lib


def test_header_parses_and_library_exports_every_symbol():
    decls = _lib.parse_header()
    assert len(decls) >= 40
    assert os.path.exists(_lib.LIB_PATH), 'run python -m pfst_amd.build'
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in decls if not hasattr(L, n)]
    assert not missing, missing
    assert _lib.lib().pfst_abi_version() == 1


def test_argument_validation_without_gpu():
    # bad arguments are rejected on the host before any launch
    L = _lib.lib()
    assert L.pfst_fill_f32(None, 10, 0.0, None) == -1
    assert b'spatial.hip' in L.pfst_last_error()
    assert L.pfst_conv_igemm(None, 0, None, None, None, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, None, None, None) == -1


def test_conv_geometry_refusals_name_the_condition():
    """one geometry rule (csrc/conv_launch.h) behind the five forward / data-gradient / weight-gradient entry points: a wrong output size or
    kernel size is PFST_ERR_ARG, and the message is the violated condition"""
    L = _lib.lib()
    p = 256          # any non-null address: refused before anything is launched
    # (Hi, Wi, Ho, Wo, ksize, stride, dil, pad, mode) -> what the message must contain
    cases = [((8, 8, 9, 8, 3, 1, 1, 1, 0), b'Ho == (Hi + 2 * pad - span - 1) / stride + 1'),
             ((8, 8, 4, 4, 3, 2, 1, 1, 1), b'Hi == (Ho + 2 * pad - span - 1) / stride + 1'),      # data gradient: 8 = out of a 15 / 16 input
             ((8, 8, 8, 8, 5, 1, 1, 2, 0), b'ksize == 1 || ksize == 3')]
    for (Hi, Wi, Ho, Wo, k, s, d, pad, mode), msg in cases:
        assert L.pfst_conv_igemm(p, 16 * Hi * Wi, p, None, p, 16 * Ho * Wo, 1, 16, Hi, Wi, 16, Ho, Wo, k, s, d, pad, mode, 0, None, None, None) == -1
        assert msg in L.pfst_last_error(), L.pfst_last_error()
        assert L.pfst_conv_igemm_split(p, 16 * Hi * Wi, p, None, p, 16 * Ho * Wo, 1, 16, Hi, Wi, 16, Ho, Wo, k, s, d, pad, mode, 0, None, None, None) == -1
        assert msg in L.pfst_last_error(), L.pfst_last_error()
        if mode == 0:
            for fn in (L.pfst_conv_wgrad, L.pfst_conv_wgrad_split):
                assert fn(p, 16 * Hi * Wi, p, 16 * Ho * Wo, p, 1, 16, Hi, Wi, 16, Ho, Wo, k, s, d, pad, None) == -1
                assert msg in L.pfst_last_error(), L.pfst_last_error()


def test_f16x3_chain_grid_policy():
    """pfst_f16x3_chain_grid (host logic, no GPU): every tile is covered by chains of at most 8, never fewer workgroups than resident slots
    when there are that many tiles, no chain for launches that cannot chain, and the last round of workgroups is never mostly empty when a
    better split exists (9216 tiles on 512 slots: 1536 workgroups x 6 = three full rounds, not 1152 x 8 = two and a quarter)."""
    from pfst_amd._lib import lib
    L = lib()
    assert L.pfst_f16x3_set_slots(512) == 0
    try:
        for total in (1, 100, 512, 513, 600, 2304, 4096, 9216, 16384, 100000):
            g = L.pfst_f16x3_chain_grid(total, 1)
            assert 0 < g <= total and -(-total // g) <= 8, (total, g)
            assert g == total if total <= 512 else g >= 512, (total, g)
            assert L.pfst_f16x3_chain_grid(total, 0) == total
        assert L.pfst_f16x3_chain_grid(9216, 1) == 1536 and L.pfst_f16x3_chain_grid(16384, 1) == 2048
        assert L.pfst_f16x3_chain_grid(0, 1) == 0
    finally:
        L.pfst_f16x3_set_slots(0)


def test_call_refuses_a_wrong_argument_count():
    """ctypes lets surplus arguments through on cdecl functions; _lib.call does not (an appended argument at the wrong call site would move
    the stream out of its slot and the launch onto the default stream)"""
    from pfst_amd import _lib
    _lib.lib()
    n = len(_lib._decls['pfst_fill_f32'][1])
    with pytest.raises(TypeError, match='takes'):
        _lib.call('pfst_fill_f32', *([0] * (n + 1)))
    with pytest.raises(TypeError, match='takes'):
        _lib.call('pfst_fill_f32', *([0] * (n - 1)))
