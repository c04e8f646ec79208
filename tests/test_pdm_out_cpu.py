"""dspi_process_pdm / dspi_pdm_running without a GPU: the symbols, the header's words, the refusals, and the running bytes through every
stream maintenance call on host-only contexts, where they are bookkeeping (include/dspi.h)."""
import ctypes as C
import os

import numpy as np
import pytest

from dspi_amd import host
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_NODEVICE = -10, -11      # include/dspi.h


def test_symbols_and_header():
    L = host.lib()
    for name in ("dspi_process_pdm", "dspi_pdm_running", "dspi_process", "dspi_pdm_modulate", "dspi_pdm_restart"): assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "8 + PDM words from the call: detect by symbol (dspi_process_pdm; with it dspi_pdm_running; additions only)",
                 "const dspi_out *out, uint32_t *pdm_words, uint32_t flags);",
                 "int dspi_pdm_running(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint8_t *set, uint8_t *get);",
                 "NOT MODELLED: the fade-out on disable", "IMMEDIATE STOP", "1,023 samples"):
        assert word in text, word


def test_error_codes():
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    assert f"#define DSPI_E_INVAL ({E_INVAL})" in text and f"#define DSPI_E_NODEVICE ({E_NODEVICE})" in text


@pytest.mark.parametrize("flavor", [0, 1])
def test_refusals(flavor):
    d = Dspi(flavor, 10, device=None)
    pcm = np.zeros((10, 48, 2), dtype=np.int16)
    words = np.zeros((10, 48, 8), dtype=np.uint32)
    out = host._Out(None, None, None, None)
    call = lambda pcm_p, out_p, words_p, flags=0: d.L.dspi_process_pdm(d.h, pcm_p, 16, 1, 48, out_p, words_p, flags)
    assert call(pcm.ctypes.data, C.byref(out), None) == E_INVAL                    # NULL pdm_words
    assert call(None, C.byref(out), words.ctypes.data) == E_INVAL
    assert call(pcm.ctypes.data, None, words.ctypes.data) == E_INVAL
    assert d.L.dspi_process_pdm(None, pcm.ctypes.data, 16, 1, 48, C.byref(out), words.ctypes.data, 0) == E_INVAL
    assert call(pcm.ctypes.data, C.byref(out), words.ctypes.data) == E_NODEVICE      # a host-only context
    for bit in (0x40, 0x80, 0x100, 0x80000000):                                      # the flags of dspi_process, and its refusals: no new bit
        assert call(pcm.ctypes.data, C.byref(out), words.ctypes.data, bit) == E_INVAL
        assert d.L.dspi_process(d.h, pcm.ctypes.data, 16, 1, 48, C.byref(out), bit) == E_INVAL
    assert not words.any()
    assert not d.pdm_running().any()      # refused calls change nothing
    d.close()


def test_running_bytes_on_a_host_only_context():
    d = Dspi(1, 12, device=None)
    assert d.pdm_running().tolist() == [0] * 12                      # 0 after dspi_create
    assert d.pdm_running(3, 4, set=[1, 0, 1, 1]).tolist() == [1, 0, 1, 1]
    assert d.pdm_running().tolist() == [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0]
    before = d.pdm_running().tolist()
    get = np.full(16, 0xEE, dtype=np.uint8)
    for first, count, vals in ((0, 0, None), (12, 1, None), (11, 2, None), (0, 13, None), (0xFFFFFFFF, 2, None), (2, 3, [1, 2, 0]), (0, 1, [255])):
        s = None if vals is None else np.array(vals, dtype=np.uint8)
        assert d.L.dspi_pdm_running(d.h, first, count, s.ctypes.data if s is not None else None, get.ctypes.data) == E_INVAL, (first, count, vals)
        assert d.pdm_running().tolist() == before and (get == 0xEE).all()      # checked before anything is written
    assert d.L.dspi_pdm_running(d.h, 0, 12, None, None) == 12                 # both may be NULL
    assert d.L.dspi_pdm_running(None, 0, 1, None, None) == E_INVAL
    d.close()


def test_running_bytes_travel():
    """what the maintenance calls that work on host-only contexts do to the byte — pause / resume: nothing; boot: to 0; resize: the new slots
    are 0 and a cut slot's byte is gone.  (Moves and migrations need run-time state: tests/test_gpu_pdm_out.py, and the module's own rules in
    tests/test_pdmlife_cpu.py.)"""
    d = Dspi(1, 10, device=None)
    d.pdm_running(0, 10, set=[1, 0, 1, 0, 1, 0, 1, 0, 1, 0])
    d.pause_streams(2, 4); assert d.pdm_running().tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    d.resume_streams(2, 2, as_is=True); assert d.pdm_running().tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]      # (4, 5 stay paused)
    d.boot_streams([0, 4])
    assert d.pdm_running().tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 1, 0]
    assert d.streams_paused().tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    d.resize_streams(13)
    assert d.pdm_running().tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0]
    d.pdm_running(12, 1, set=[1]); d.pause_streams(11, 2); d.resize_streams(11); d.resize_streams(13)
    assert d.pdm_running().tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0]
    d.close()
