"""dspi_pdm_fade on the GPU (include/dspi.h): the PDM fade-out on disable, per stream, opt-in.  A stream whose sub goes off ramps its last
level to silence over 1 023 more samples, the modulator running on; a re-enable during the ramp cancels it into a partial fade-in; after the
ramp the stream is stopped and its next enable goes through the re-enable reset with the RNG where the fade left it.

The model is tests/pdmfade_model.py: one PdmOracle per stream plus the rule, the base computed from the `sub` words the call itself returned
(or, where the caller passes no out->sub, those of a twin context's dspi_process).  Every comparison is for equality.  A stream that is not
modulated leaves its words unwritten (a sentinel survives in device buffers, host buffers read zeros); the frames after a fade's end inside
a call are ZERO words on every path.  Streams that are never disabled are also held to a plain PdmOracle throughout.

Shapes: 130 float streams and 70 Q28 streams (one full row and a ragged one), 48-frame packets.  Disabled: a full row's first stream, one
inside it, and the last of the ragged row."""
import numpy as np
import pytest

from conftest import has_gpu
from orclib import PdmOracle
from pdmfade_model import FadeStream
from dspi_amd import wire as W, workloads as WL
from test_gpu_pdm_out import FS, Rig, make, sub_setup
from test_gpu_snapshot import fid, hand_over, packets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS = (W.F32_FMA, 0)
R = W.REQ


def streams_of(flavor): return 130 if int(flavor) else 70


def faders(S): return (0, 37, S - 1)


class FadeRig(Rig):
    """Rig's context, input and raw call, with the fade model beside every slot"""

    def __init__(self, flavor, S=None, n=10, B=48, mode=True, packets_total=100, twin=False):
        S = S or streams_of(flavor)
        super().__init__(flavor, S, n=n, B=B, packets_total=packets_total)
        self.mode = mode
        if mode: assert self.d.pdm_fade(1) is True
        else: assert self.d.pdm_fade() is False
        self.m = [FadeStream() for _ in range(S)]
        self.plain = {s: PdmOracle() for s in range(S)}      # the neighbours: dropped the moment anything but plain modulation happens to a slot
        self.plain_started = set()
        self.twin = make(flavor, S) if twin else None         # its dspi_process gives the sub words of calls made without out->sub

    def close(self):
        self.d.close()
        if self.twin: self.twin.close()

    def touch(self, *slots):
        for s in slots: self.plain.pop(s, None)

    def set_sub(self, s, on):
        self.touch(s)
        super().set_sub(s, on)
        if self.twin: self.twin.vendor_set(R["SET_OUTPUT_ENABLE"], self.d.N - 1, b"\x01" if on else b"\x00", stream=s)

    def set_mode(self, on):
        assert self.d.pdm_fade(1 if on else 0) is bool(on)
        if self.mode and not on:
            for x in self.m: x.stop_now()
        if on and not self.mode:
            for x in self.m: x.pos, x.base = 0, 0
        self.mode = bool(on)

    def call(self, mem="device", tiled=False, with_sub=True, n=None, what=""):
        d, S, B = self.d, self.S, self.B
        n = n or self.n
        F = n * B
        pcm = packets(self.data, 16, B, self.pos, self.pos + n)
        sub, words, unwritten = self.raw_call(pcm, n, mem, tiled, with_sub)
        if self.twin:
            tsub = self.twin.process_host(pcm, n, B, want_pairs=False, want_peaks=False)[1]
            if sub is None: sub = tsub
        assert sub is not None, "a call without out->sub needs the twin"
        for s in range(S):
            if self.paused[s]:
                assert (words[s] == unwritten).all(), f"{what}: stream {s} is paused, its words were written"
                continue
            x = self.m[s]
            was = x.pos
            want = x.call(self.sub_on[s], sub[s], F, self.mode)
            if want is None:
                assert (words[s] == unwritten).all(), f"{what}: stream {s} is not modulated, its words were written"
                continue
            if not np.array_equal(want, words[s]):
                f = int(np.argwhere((want != words[s]).any(axis=1))[0][0])
                raise AssertionError(f"{what}: stream {s} (sub {'on' if self.sub_on[s] else 'off'}, fade position {was} before the call): PDM words differ from the model's from frame {f}")
            if s in self.plain:
                if s not in self.plain_started: self.plain[s].restart(); self.plain_started.add(s)
                assert np.array_equal(self.plain[s].run(sub[s]), words[s]), f"{what}: neighbour {s}: words differ from a plain PdmOracle's"
        assert d.pdm_running().tolist() == [x.running for x in self.m], f"{what}: the running bytes"
        if self.mode: assert d.pdm_fade_state().tolist() == [x.word() for x in self.m], f"{what}: the fade words"
        self.pos += n
        return sub, words

    def fade_out(self, mem="device", what="", **kw):
        """calls until nobody fades any more; how many"""
        k = 0
        while any(x.pos for x in self.m) or k == 0:
            self.call(mem, what=f"{what}, fade call {k}", **kw); k += 1
            assert k < 20
        return k


# ---- 1. call lengths; a fade and its re-enable -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B_,fade_calls", [(10, 48, 3), (24, 48, 1), (31, 33, 1)], ids=["spans-three-calls", "ends-inside-a-call", "ends-with-the-call"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_a_fade_and_its_re_enable(flavor, n, B_, fade_calls):
    """disable after the fade-in is complete, follow the fade to its end (byte 0, then unwritten), re-enable: the words are the model's — the RNG
    has advanced through the fade's 8 184 draws.  Without the feature this fails at the first line (no such symbol), and with an immediate stop
    at the re-enable."""
    x = FadeRig(flavor, n=n, B=B_, packets_total=8 * n + 30)
    S = x.S
    while x.pos * B_ < 1024: x.call(n=min(n, 24), what="fade-in")
    assert all(int(m.o.st[8]) == 1024 for m in x.m)
    for s in faders(S): x.set_sub(s, False)
    assert x.fade_out(what="fading") == fade_calls
    assert [x.m[s].running for s in faders(S)] == [0, 0, 0] and x.d.pdm_running(37, 1).tolist() == [0]
    x.call(what="stopped")                                       # unwritten: the sentinel survives
    x.call("host", what="stopped, host")                         # zeros
    for s in faders(S): x.set_sub(s, True)
    x.call(what="re-enabled")
    x.call("host", tiled=True, what="and on")
    assert len(x.plain) == S - 3
    x.close()


# ---- 2. fade-in and cancel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_disable_during_the_fade_in_and_cancel_mid_fade(flavor):
    x = FadeRig(flavor)
    S = x.S
    x.call(what="480 frames of fade-in")
    for s in faders(S): x.set_sub(s, False)                      # the base is a scaled sample, the fade-in position stays 480
    x.call(what="fading from inside the fade-in")
    assert [x.m[s].pos for s in faders(S)] == [544] * 3 and all(int(x.m[s].o.st[8]) == 480 for s in faders(S))
    x.set_sub(0, True); x.set_sub(S - 1, True)                   # cancel: fade-in position 480 again (1024 - 544), no reset
    x.call(what="cancelled at 544")
    assert int(x.m[0].o.st[8]) == 960 and x.m[37].pos == 64
    x.set_sub(37, True)                                          # cancel 63 samples before the end
    x.call("host", what="cancelled at 64")
    for s in faders(S): x.set_sub(s, False)
    x.call(n=21, what="fading again")                            # 1008 frames: position 16
    x.set_sub(37, True)
    x.call(what="cancelled at 16")
    x.fade_out(what="the others to their end")
    x.close()


# ---- 3. memory paths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "direct", "staged"])
@pytest.mark.parametrize("tiled", [False, True], ids=["major", "tiled"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_memory_paths(flavor, tiled, mem, monkeypatch):
    """a whole fade, the stopped stream and the re-enable on each memory path and in both layouts, the calls alternately with and without out->sub"""
    if mem == "staged": monkeypatch.setenv("DSPI_NO_DIRECT", "1")
    n = 2 if mem == "direct" else 10
    x = FadeRig(flavor, n=n, packets_total=120, twin=True)
    monkeypatch.delenv("DSPI_NO_DIRECT", raising=False)
    S, path = x.S, "device" if mem == "device" else "host"
    k = 0

    def call(what):
        nonlocal k
        before = x.d.direct_stats()["calls"]
        x.call(path, tiled=tiled, with_sub=k % 2 == 0, what=what); k += 1
        if mem != "device": assert (x.d.direct_stats()["calls"] > before) == (mem == "direct"), "the call did not take the memory path this case is about"

    call("on"); call("on")
    for s in faders(S): x.set_sub(s, False)
    while x.m[0].running: call("fading")                       # (11 direct calls, 3 otherwise: the last one ends the fade inside it)
    call("stopped"); call("stopped")
    for s in faders(S): x.set_sub(s, True)
    call("re-enabled"); call("and on")
    x.close()


# ---- 4. lifecycle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_pause_swap_boot(flavor):
    x = FadeRig(flavor, n=5)
    S = x.S
    x.call(what="on")
    for s in faders(S): x.set_sub(s, False)
    x.call(what="fading")
    x.touch(36, 37, 38); x.pause(36, 3)                                    # a fading stream and its neighbours sit two calls out
    x.call(what="37 paused"); x.call("host", what="37 paused, host")
    assert x.m[37].pos == 784 and x.m[0].pos == 304
    x.resume(36, 3)
    x.call(what="resumed")
    assert x.m[37].pos == 544
    # a fading stream (37, the full row) swaps with a running one (S - 2, the ragged row): position, base, byte and parameters travel
    x.touch(S - 2)
    assert x.d.move_streams([(37, S - 2), (S - 2, 37)], as_is=True) == 2
    for book in (x.m, x.sub_on): book[37], book[S - 2] = book[S - 2], book[37]
    assert x.d.pdm_fade_state(S - 2, 1).tolist() == [x.m[S - 2].word()] and x.m[S - 2].pos == 544
    x.call(what="swapped")
    # the fading slot is power-cycled: nothing fades there any more, base 0
    x.d.boot_streams([S - 2], as_is=True)
    x.m[S - 2] = FadeStream()
    x.sub_on[S - 2] = x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=S - 2) == b"\x01"
    assert x.d.pdm_fade_state(S - 2, 1).tolist() == [0] and x.d.pdm_running(S - 2, 1).tolist() == [0]
    x.call(what="booted")
    if not x.sub_on[S - 2]:
        sub_setup(x.d, flavor, stream=S - 2); x.set_sub(S - 2, True)
    x.call(what="the booted slot's sub on")
    x.fade_out(what="the rest")
    x.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_grow_and_shrink(flavor):
    x = FadeRig(flavor, n=5)
    S = x.S
    x.call(what="on")
    x.set_sub(S - 1, False); x.set_sub(0, False)
    x.call(what="fading")
    G = 130 if int(flavor) else 70
    grown = S + G                                                           # a third row, past the capacity: the arrays are reallocated, the bases come over
    assert x.d.resize_streams(grown) == grown
    x.S = grown
    x.data = WL.synth_pcm16(grown, x.B * 100, FS)
    x.m += [FadeStream() for _ in range(G)]; x.running += [0] * G; x.paused += [False] * G
    x.sub_on += [x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01" for s in range(S, grown)]
    x.plain = {}
    assert x.d.pdm_fade_state(S - 1, 3).tolist() == [x.m[S - 1].word(), 0, 0]
    for s in (S, grown - 1):
        if not x.sub_on[s]: sub_setup(x.d, flavor, stream=s); x.set_sub(s, True)
    x.call(what="grown")
    x.set_sub(grown - 1, False)
    x.call(what="a new slot fades")
    assert x.m[grown - 1].pos == 784
    # the fading new slot is cut and comes back: power-on, nothing fades, base 0 — shown by a fade from base 0 (byte set by hand, sub off)
    x.pause(S + 10, G - 10)
    assert x.d.resize_streams(S + 10) == S + 10 and x.d.resize_streams(grown) == grown
    for s in range(S + 10, grown): x.m[s] = FadeStream(); x.paused[s] = False
    x.sub_on[S + 10:] = [x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01" for s in range(S + 10, grown)]
    assert x.d.pdm_fade_state(grown - 1, 1).tolist() == [0]
    assert not x.sub_on[grown - 1]
    x.d.pdm_running(grown - 1, 1, set=[1]); x.m[grown - 1].running = 1
    x.call(what="regrown")
    assert x.m[grown - 1].pos == 784 and x.m[grown - 1].base == 0
    x.call("host", tiled=True, what="regrown, tiled")
    x.close()


@pytest.mark.parametrize("dst_mode", [True, False], ids=["both-fade", "destination-off"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_migrate_a_fading_stream(flavor, dst_mode):
    S = 70 if int(flavor) else 40
    a, b = FadeRig(flavor, S, n=4), FadeRig(flavor, S, n=4, mode=dst_mode)
    a.call(what="source"); b.call(what="destination")
    a.set_sub(3, False)
    a.call(what="source, 3 fading")
    b.touch(5, 6); b.pause(5, 2)
    assert a.d.migrate_streams(b.d, [(2, 5), (3, 6)], as_is=True, paused=False) == 2      # a running and a fading stream
    for src, dst in ((2, 5), (3, 6)):
        b.m[dst], b.sub_on[dst], b.paused[dst] = a.m[src], a.sub_on[src], False
        a.paused[src] = True; a.touch(src)                                                  # (the source slot stays behind as a paused, frozen copy)
    if not dst_mode: b.m[6].stop_now()                                                      # the fade ends as an immediate stop, byte 0
    assert b.d.pdm_running(5, 2).tolist() == [1, 1 if dst_mode else 0]
    if dst_mode: assert b.d.pdm_fade_state(5, 2).tolist() == [b.m[5].word(), b.m[6].word()] and b.m[6].pos == 832
    b.call(what="arrived")
    b.call("host", what="arrived, host")
    b.set_sub(6, True)                                                                      # both-fade: a cancel; destination-off: through the reset
    b.call(what="the arrival's sub on again")
    a.close(); b.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_a_fading_stream_through_a_snapshot(flavor):
    """snapshots carry neither the byte nor the fade word: dspi_pdm_running and dspi_pdm_fade_state do"""
    S = 70 if int(flavor) else 40
    a, b = FadeRig(flavor, S, n=4), FadeRig(flavor, S, n=4)
    a.call(what="source"); b.call(what="destination")
    a.set_sub(4, False)
    a.call(what="source, 4 fading")
    hand_over(a.d, b.d, 4, 1, 9)
    assert b.d.pdm_fade_state(9, 1).tolist() == [b.m[9].word()], "an import leaves the slot's fade word alone"
    b.d.pdm_running(9, 1, set=a.d.pdm_running(4, 1)); b.d.pdm_fade_state(9, 1, set=a.d.pdm_fade_state(4, 1))
    b.touch(9)
    b.m[9], b.sub_on[9] = a.m[4], b.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=9) == b"\x01"
    assert not b.sub_on[9] and b.m[9].pos == 832
    b.call(what="imported, carried")
    b.fade_out(what="to its end")
    a.close(); b.close()


# ---- 5. the mode --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_mode_off_ends_the_fades_and_mode_off_is_the_default(flavor):
    x = FadeRig(flavor, mode=False, n=5)
    S = x.S
    x.call(what="mode off"); x.set_sub(0, False); x.call(what="mode off: an immediate stop")
    assert x.m[0].running == 0
    x.set_sub(0, True); x.call("host", what="mode off: the re-enable")
    x.set_mode(True)
    for s in faders(S): x.set_sub(s, False)
    x.call(what="fading")
    assert x.m[0].pos == 784
    x.set_mode(False)                                            # every fade in flight ends at once: byte 0, no more words
    assert x.d.pdm_running(0, 1).tolist() == [0]
    x.call(what="mode off again")
    x.set_mode(True)
    for s in faders(S): x.set_sub(s, True)
    x.call(what="mode on, re-enabled: through the reset")
    x.close()
