"""The fade model (tests/pdmfade_model.py) against the reference's own object code: a signal, then the model's 1 023 synthetic fade samples,
go through pdm_processing_loop as the firmware build of the oracle runs it (orc_pdm_ref_run), then the re-enable (orc_pdm_ref_restart_keep_rng)
and a second signal; the model's words are equal throughout.  That holds the fade's modulator arithmetic and the RNG's 8 184 draws to the
reference loop.  The target formula stays our reading of pdm_generator.c:327; the cancel, and a disable before the fade-in has completed,
need a loop local poked and are held to the restatement only."""
import ctypes as C

import numpy as np
import pytest

import orclib
from pdmfade_model import FadeStream, fade_samples, pcm_of

pytestmark = pytest.mark.skipif(not orclib.ref_available(1, "fw"), reason="the firmware build of the oracle is not here")


def signals():
    rng = np.random.default_rng(23)
    a = np.concatenate([(rng.uniform(-0.9, 0.9, 1200) * (1 << 28)).astype(np.int32),
                        (np.sin(np.arange(800) * 2 * np.pi * 60 / 48000) * 0.7 * (1 << 28) - 0.2 * (1 << 28)).astype(np.int32)])
    b = (rng.uniform(-0.5, 0.5, 1500) * (1 << 28)).astype(np.int32)
    return a, b


@pytest.mark.parametrize("calls", [(1023,), (480, 480, 63), (1000, 48)], ids=["one-call", "three-calls", "ends-inside"])
def test_a_whole_fade_and_its_re_enable_are_the_reference_loops(calls):
    a, b = signals()
    assert a.size >= 1024
    fw = orclib.load(1, "fw")
    fw.orc_pdm_ref_restart()
    ref = lambda x: (lambda out: (fw.orc_pdm_ref_run(np.ascontiguousarray(x).ctypes.data_as(C.c_void_p), C.c_uint32(x.size), out.ctypes.data_as(C.c_void_p)), out)[1])(np.zeros((x.size, 8), dtype=np.uint32))
    m = FadeStream()
    assert np.array_equal(m.call(True, a, a.size), ref(a)), "the first signal"
    base = pcm_of(a[-1], 1024)
    assert m.base == base and base != 0
    synth = fade_samples(base, 1024, 1023)
    assert synth.size == 1023 and (np.abs(synth >> 14) <= 29500).all() and (synth >> 14)[-1] == (base >> 10)
    want = ref(synth)                                               # the fade, as normal samples through the reference loop
    at = 0
    for k, frames in enumerate(calls):                              # ... and as the model's calls: sub off, whatever `sub` holds
        words = m.call(False, np.full(frames, 0x7FFFFFFF, dtype=np.int32), frames)
        n = min(frames, 1023 - at)
        assert np.array_equal(words[:n], want[at:at + n]), f"fade call {k}"
        assert not words[n:].any(), "the rest of the call after the fade's end is zero words"
        at += n
        assert m.running == (0 if at == 1023 else 1) and m.pos == (0 if at == 1023 else 1024 - at)
    assert at == 1023
    assert m.call(False, b[:10], 10) is None                        # a stopped stream
    fw.orc_pdm_ref_restart_keep_rng()
    assert np.array_equal(m.call(True, b, b.size), ref(b)), "after the re-enable: the RNG stands where the fade left it"
