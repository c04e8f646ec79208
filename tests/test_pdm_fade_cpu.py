"""dspi_pdm_fade / dspi_pdm_fade_state without a GPU: the symbols, the header's words, the refusals of both calls, and the mode on host-only
contexts (include/dspi.h)."""
import os

import numpy as np
import pytest

from dspi_amd import host
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_NODEVICE = -10, -11      # include/dspi.h


def test_symbols_and_header():
    L = host.lib()
    for name in ("dspi_pdm_fade", "dspi_pdm_fade_state", "dspi_process_pdm", "dspi_pdm_running"): assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "int dspi_pdm_fade(dspi_ctx *ctx, int enable);",
                 "int dspi_pdm_fade_state(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get);",
                 "THE RUNNING BYTE STAYS 1 WHILE THE STREAM FADES", "the firmware would need that request",
                 "fade_out_pos | (uint32_t)(uint16_t)fade_base_pcm << 16"):
        assert word in text, word
    # the paragraph about the default stands, and the new section comes after it
    for word in ("NOT MODELLED: the fade-out on disable", "IMMEDIATE STOP", "1,023 samples"):
        assert word in text and text.index(word) < text.index("THE FADE-OUT, OPT-IN"), word


@pytest.mark.parametrize("flavor", [0, 1])
def test_the_mode_on_a_host_only_context(flavor):
    d = Dspi(flavor, 10, device=None)
    assert d.pdm_fade() is False                      # off after dspi_create
    assert d.pdm_fade(1) is True and d.pdm_fade() is True and d.pdm_fade(-1) is True
    assert d.pdm_fade(1) is True                      # (again: nothing)
    assert d.pdm_fade(0) is False and d.pdm_fade() is False
    assert d.L.dspi_pdm_fade(None, 1) == E_INVAL
    # the bytes' own calls go on working beside the mode
    d.pdm_fade(1)
    assert d.pdm_running(2, 2, set=[1, 1]).tolist() == [1, 1]
    d.boot_streams([2]); d.resize_streams(13); d.pause_streams(11, 2); d.resize_streams(11)
    assert d.pdm_running().tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert d.pdm_fade(0) is False
    assert d.pdm_running().tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]      # nobody was fading: disabling the mode stops nobody
    d.close()


def test_fade_state_refusals():
    d = Dspi(1, 12, device=None)
    get = np.full(16, 0xEEEEEEEE, dtype=np.uint32)
    one = np.zeros(4, dtype=np.uint32)
    call = lambda first, count, s, g=get: d.L.dspi_pdm_fade_state(d.h, first, count, s.ctypes.data if s is not None else None, g.ctypes.data if g is not None else None)
    assert call(0, 1, None) == E_INVAL and b"mode is off" in d.L.dspi_last_error(d.h)      # the mode is off
    d.pdm_fade(1)
    for first, count, vals in ((0, 0, None), (12, 1, None), (11, 2, None), (0, 13, None), (0xFFFFFFFF, 2, None), (2, 3, [0, 1024, 0]), (0, 1, [0xFFFF]),
                               (0, 1, [29501 << 16]), (0, 2, [5, ((-29501) & 0xFFFF) << 16]), (0, 1, [0x8000 << 16])):
        s = None if vals is None else np.array(vals, dtype=np.uint32)
        assert call(first, count, s) == E_INVAL, (first, count, vals)
        assert (get == 0xEEEEEEEE).all()                                                      # checked before anything is written
    assert call(0, 4, one) == E_NODEVICE and call(0, 4, None) == E_NODEVICE                   # valid, but a host-only context has no bases
    assert (get == 0xEEEEEEEE).all()
    assert d.L.dspi_pdm_fade_state(None, 0, 1, None, None) == E_INVAL
    d.close()
