"""dspi_process_pdm on the GPU (include/dspi.h): the PDM words straight out of the call, each stream's modulator run only while the device's
sub output is on (GET_CORE1_MODE == 1), brought up through the re-enable reset when it comes on, and carried through pauses, moves, boots,
migrations, resizes and snapshots by the context's running bytes.

The oracle is one PdmOracle (tests/orclib.py) per stream, fed the Q28 sub words of the call itself — which the chain's own oracle holds for
sampled streams here and for every stream elsewhere — with .restart() exactly where the rule says reset.  A stream that is not modulated
must leave its words unwritten: a sentinel survives in device buffers, host buffers read zeros.

Shapes: 300 float streams (three rows, the last ragged) and 150 Q28 streams (three rows, the last ragged), 48-frame packets, 10 packets per
call (2 on the direct path: its area holds 2 MiB).  No figures: every comparison is for equality."""
import numpy as np
import pytest

from conftest import has_gpu
from orclib import PdmOracle
from dspi_amd import wire as W, workloads as WL
from test_gpu_snapshot import context, fid, hand_over, oracle, packets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS = (W.F32_FMA, 0)
FS, B = 48000, 48
SENT = 0x5A5A5A5A
R = W.REQ


def streams_of(flavor): return 300 if int(flavor) else 150


def sub_setup(x, flavor, **kw):
    """the sub output on, on a context (kw: stream=) or an oracle: the interlock (usb_audio.c:1891-1904) refuses it while outputs 2..N-2 are enabled"""
    N = W.dims(int(flavor))[1]
    for o in range(2, N - 1): x.vendor_set(R["SET_OUTPUT_ENABLE"], o, b"\x00", **kw)
    x.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01", **kw)


def make(flavor, S):
    d = context(flavor, S, FS, WL.full_chain_blob(int(flavor)))
    sub_setup(d, flavor)
    for s in (0, S // 2, S - 1): assert d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01", "the sub is not on"
    return d


def untile_words(words, S):
    nt, F, _, Rw = words.shape
    return words.transpose(0, 3, 1, 2).reshape(nt * Rw, F, 8)[:S]


class Rig:
    """A context and the model of include/dspi.h's rule beside it: per slot the stream's PdmOracle, its running byte, whether its sub is on and
    whether it is paused.  call() makes one dspi_process_pdm call and holds every stream's words to the model."""

    def __init__(self, flavor, S, n=10, B=B, packets_total=64, chain=()):
        self.flavor, self.S, self.n, self.B = flavor, S, n, B
        self.d = make(flavor, S)
        self.data = WL.synth_pcm16(S, B * packets_total, FS)
        self.pos = 0
        self.pdm = [PdmOracle() for _ in range(S)]
        self.running, self.sub_on, self.paused = [0] * S, [True] * S, [False] * S
        # the chain's own oracle for a few slots: the sub words the modulators are fed are the device's
        self.chain = {s: oracle(flavor, FS, WL.full_chain_blob(int(flavor)), setup=lambda o: sub_setup(o, flavor)) for s in chain}

    def close(self): self.d.close()

    def set_sub(self, s, on):
        d, N = self.d, self.d.N
        d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01" if on else b"\x00", stream=s)
        self.sub_on[s] = d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01"
        assert self.sub_on[s] == on, f"stream {s}: GET_CORE1_MODE after the request"
        if s in self.chain: self.chain[s].vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01" if on else b"\x00")

    def pause(self, first, count):
        assert self.d.pause_streams(first, count) == count
        for s in range(first, first + count): self.paused[s] = True

    def resume(self, first, count):
        assert self.d.resume_streams(first, count, as_is=True) == count
        for s in range(first, first + count): self.paused[s] = False

    def raw_call(self, pcm, n, mem, tiled, with_sub):
        """one call; (sub or None, words, the value of an unwritten word), both stream-major"""
        d, S, B = self.d, self.S, self.B
        F = n * B
        Rw = d.tile_streams(); nt = (S + Rw - 1) // Rw
        if mem == "device":
            import torch
            dev = torch.device("cuda", 0)
            t_pcm = torch.from_numpy(pcm).to(dev)
            t_words = torch.full((nt, F, 8, Rw) if tiled else (S, F, 8), SENT, dtype=torch.int32, device=dev)
            t_sub = torch.full((nt, F, Rw) if tiled else (S, F), SENT, dtype=torch.int32, device=dev) if with_sub else None
            torch.cuda.synchronize()
            d.process_pdm_device(t_pcm.data_ptr(), n, B, t_words.data_ptr(), sub_ptr=t_sub.data_ptr() if with_sub else 0, tiled=tiled)
            d.sync()
            words = t_words.cpu().numpy().view(np.uint32)
            sub = t_sub.cpu().numpy() if with_sub else None
            unwritten = SENT
        else:
            words = np.full((nt, F, 8, Rw) if tiled else (S, F, 8), SENT, dtype=np.uint32)
            _, sub, _, words = d.process_pdm_host(pcm, n, B, want_pairs=False, want_sub=with_sub, want_peaks=False, tiled=tiled, words=words)
            unwritten = 0
        if tiled:
            words = untile_words(words, S)
            if with_sub: sub = d.untile(None, sub)[1]
        return sub, words, unwritten

    def call(self, mem="host", tiled=False, with_sub=True, n=None, sub_from=None, what=""):
        d, S, B = self.d, self.S, self.B
        n = n or self.n
        pcm = packets(self.data, 16, B, self.pos, self.pos + n)
        sub, words, unwritten = self.raw_call(pcm, n, mem, tiled, with_sub)
        if sub is None: sub = sub_from
        for s in range(S):
            if self.paused[s] or not self.sub_on[s]:
                assert (words[s] == unwritten).all(), f"{what}: stream {s} is not modulated, its words were written"
                if not self.paused[s]: self.running[s] = 0
                continue
            if not self.running[s]: self.pdm[s].restart(); self.running[s] = 1
            want = self.pdm[s].run(sub[s])
            assert np.array_equal(want, words[s]), f"{what}: stream {s}: PDM words differ from the oracle's from frame {int(np.argwhere(want != words[s])[0][0])}"
        assert d.pdm_running().tolist() == self.running, f"{what}: the running bytes"
        for s, o in self.chain.items():
            if self.paused[s]: continue
            rs = o.process(pcm[s], n, B, 16)[1]
            if with_sub and self.sub_on[s]: assert np.array_equal(rs, sub[s]), f"{what}: stream {s}: the sub words differ from the chain's oracle"
        self.pos += n
        return sub, words

    def modulate_and_process(self, what):
        """dspi_process and dspi_pdm_modulate on the same context still give their oracles' words: dspi_pdm_modulate runs EVERY active stream's
        modulator from the stored words (so this also reads every frozen state), and knows nothing of the running bytes"""
        d, S, B, n = self.d, self.S, self.B, 2
        pcm = packets(self.data, 16, B, self.pos, self.pos + n)
        before = d.pdm_running().tolist()
        _, sub, _ = d.process_host(pcm, n, B, want_pairs=False, want_peaks=False)
        for s, o in self.chain.items():
            if not self.paused[s]: assert np.array_equal(o.process(pcm[s], n, B, 16)[1], sub[s]), f"{what}: dspi_process, stream {s}: sub words differ from the chain's oracle"
        self.pos += n
        fed = np.ascontiguousarray(sub + (np.arange(S, dtype=np.int32) * 7919)[:, None])      # (stopped subs are zeros: every stream gets words of its own)
        words = d.pdm_host(fed)
        for s in range(S):
            if self.paused[s]: assert not words[s].any(), f"{what}: dspi_pdm_modulate wrote a paused stream's words"
            else: assert np.array_equal(self.pdm[s].run(fed[s]), words[s]), f"{what}: dspi_pdm_modulate, stream {s}: words differ from the oracle's (its state was not what the rule leaves)"
        assert d.pdm_running().tolist() == before, f"{what}: dspi_process / dspi_pdm_modulate touched the running bytes"


# ---- 1. equals the two-call route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sub", [True, False], ids=["sub", "nosub"])
@pytest.mark.parametrize("mem", ["device", "direct", "staged"])
@pytest.mark.parametrize("tiled", [False, True], ids=["major", "tiled"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_equals_the_two_calls(flavor, tiled, mem, with_sub, monkeypatch):
    """everyone on, nobody paused, three calls: the words of dspi_process + dspi_pdm_modulate on a twin context, and every stream's oracle's"""
    if mem == "staged": monkeypatch.setenv("DSPI_NO_DIRECT", "1")
    S = streams_of(flavor)
    n = 2 if mem == "direct" else 10
    x = Rig(flavor, S, n=n, chain=(0, S - 1))
    monkeypatch.delenv("DSPI_NO_DIRECT", raising=False)
    twin = make(flavor, S)
    for k in range(3):
        pcm = packets(x.data, 16, B, x.pos, x.pos + n)
        _, tsub, _ = twin.process_host(pcm, n, B, want_pairs=False, want_peaks=False)
        if tiled:
            Rw = twin.tile_streams(); nt = (S + Rw - 1) // Rw
            pad = np.zeros((nt * Rw, n * B), dtype=np.int32); pad[:S] = tsub
            twords = untile_words(twin.pdm_host(np.ascontiguousarray(pad.reshape(nt, Rw, -1).transpose(0, 2, 1)), tiled=True), S)
        else: twords = twin.pdm_host(tsub)
        before = x.d.direct_stats()["calls"]
        sub, words = x.call(mem, tiled, with_sub, sub_from=tsub, what=f"call {k}")
        if mem != "device": assert (x.d.direct_stats()["calls"] > before) == (mem == "direct"), "the call did not take the memory path this case is about"
        assert np.array_equal(words, twords), f"call {k}: the words differ from dspi_process + dspi_pdm_modulate"
        if with_sub: assert np.array_equal(sub, tsub), f"call {k}: the sub words differ from dspi_process's"
    x.modulate_and_process("after the three calls")
    x.close(); twin.close()


# ---- 2. the device's own on/off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B_", [(10, 48), (1, 1), (3, 45)], ids=["10x48", "F1", "F135"])
@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_per_stream_on_off(flavor, mem, n, B_):
    """the sub off on s % 8 != 3: the listed lanes straddle every row in one wave and the list length (38 / 19) is no multiple of 64; then some
    come on again, through the reset, beside neighbours that run on (reset and carried lanes share a wave); also with F = 1 and an odd F"""
    S = streams_of(flavor)
    x = Rig(flavor, S, n=n, B=B_, chain=(3, 4, S - 1))
    x.call(mem, what="everyone on")
    for s in range(S):
        if s % 8 != 3: x.set_sub(s, False)
    x.call(mem, what="s % 8 == 3 only")                       # the others: stops; their words unwritten, their state frozen
    x.call(mem, tiled=True, what="s % 8 == 3 only, tiled")
    for s in range(S):
        if s % 8 in (4, 5) or s >= S - 3: x.set_sub(s, True)
    x.call(mem, what="some on again")                         # r-lanes beside carried lanes
    x.call(mem, with_sub=True, tiled=True, what="and on")
    x.modulate_and_process("after the on/off calls")
    x.close()


# ---- 3. lifecycle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_pause_move_boot(flavor, mem):
    S = streams_of(flavor)
    x = Rig(flavor, S, n=8, chain=(0, 7))
    for s in range(S):
        if s % 3 == 1: x.set_sub(s, False)
    x.call(mem, what="before")
    x.pause(5, 6)                                             # listed and unlisted streams sit a call out: frozen, bytes left alone
    x.call(mem, what="5..10 paused")
    assert x.running[6] == 1 and x.running[7] == 0
    x.resume(5, 6)
    x.call(mem, what="resumed")
    # a running stream (0) and a stopped one (1) swap slots; the bytes, the oracles and the parameters travel
    assert x.running[0] == 1 and x.running[1] == 0
    assert x.d.move_streams([(0, 1), (1, 0)], as_is=True) == 2
    for book in (x.pdm, x.running, x.sub_on): book[0], book[1] = book[1], book[0]
    x.chain.pop(0)      # (the chain's oracle follows a stream's row of the input: slot 0's stream has moved)
    x.call(mem, what="swapped")
    assert x.running[0] == 0 and x.running[1] == 1
    # one running slot is power-cycled: factory parameters (sub off), a modulator that never ran
    assert x.running[2] == 1
    x.d.boot_streams([2], as_is=True)
    x.pdm[2], x.running[2] = PdmOracle(), 0
    x.sub_on[2] = x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=2) == b"\x01"
    assert x.d.pdm_running(2, 1).tolist() == [0]
    x.call(mem, what="booted")
    if not x.sub_on[2]:
        sub_setup(x.d, flavor, stream=2); x.set_sub(2, True)
    x.call(mem, what="the booted slot's sub on")              # from power-on: the oracle is a fresh one
    x.modulate_and_process("after the lifecycle calls")
    x.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_migrate_and_grow(flavor):
    S = 70 if int(flavor) else 40
    a, b = Rig(flavor, S, n=4), Rig(flavor, S, n=4)
    a.set_sub(3, False)
    a.call("device", what="source"); b.call("device", what="destination")
    b.pause(5, 2)
    assert a.d.migrate_streams(b.d, [(2, 5), (3, 6)], as_is=True, paused=False) == 2      # a running and a stopped stream into paused slots
    for src, dst in ((2, 5), (3, 6)):
        b.pdm[dst], b.running[dst], b.sub_on[dst], b.paused[dst] = a.pdm[src], a.running[src], a.sub_on[src], False
        a.paused[src] = True
    assert b.d.pdm_running(5, 2).tolist() == [1, 0] and a.d.pdm_running(2, 2).tolist() == [1, 0]
    b.set_sub(6, True)
    b.call("device", what="arrived")                          # 5 runs on (no reset), 6 comes up through the reset
    a.call("device", what="the source after the migration")
    # growing by a partial row: the new slots never ran
    grown = S + 9
    assert b.d.resize_streams(grown) == grown
    b.S = grown
    b.data = WL.synth_pcm16(grown, b.B * 64, FS)
    b.pdm += [PdmOracle() for _ in range(9)]; b.running += [0] * 9; b.paused += [False] * 9
    b.sub_on += [b.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01" for s in range(S, grown)]
    assert b.d.pdm_running(S, 9).tolist() == [0] * 9
    for s in range(S, grown, 2):
        if not b.sub_on[s]:
            sub_setup(b.d, flavor, stream=s); b.set_sub(s, True)
    b.call("device", what="grown")
    b.call("host", tiled=True, what="grown, tiled")
    b.modulate_and_process("after the resize")
    a.close(); b.close()


@pytest.mark.parametrize("carry", [True, False], ids=["carried", "not-carried"])
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_snapshot_import(flavor, carry):
    """the byte does not travel with a snapshot: carried by dspi_pdm_running the imported stream runs on, else it comes up through the reset"""
    S = 70 if int(flavor) else 40
    a, b = Rig(flavor, S, n=4), Rig(flavor, S, n=4)
    a.call("host", what="source"); b.set_sub(9, False); b.call("host", what="destination")
    assert a.d.pdm_running(4, 1).tolist() == [1] and b.d.pdm_running(9, 1).tolist() == [0]
    hand_over(a.d, b.d, 4, 1, 9)
    assert b.d.pdm_running(9, 1).tolist() == [0], "an import leaves the slot's byte alone"
    b.pdm[9], b.sub_on[9] = a.pdm[4], b.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=9) == b"\x01"
    assert b.sub_on[9], "the parameters travel with the snapshot: the sub is on"
    if carry:
        b.d.pdm_running(9, 1, set=a.d.pdm_running(4, 1)); b.running[9] = 1
    b.call("host", what="imported, carried" if carry else "imported, not carried")      # (not carried: the model restarts the oracle, as the rule says)
    a.close(); b.close()


# ---- 4. nobody listed / one stream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_nobody_listed_and_one_stream(flavor):
    x = Rig(flavor, 70 if int(flavor) else 40, n=4)
    x.call("device", what="on")
    N = x.d.N
    x.d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x00")      # everyone's sub off, one broadcast request
    x.sub_on = [x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01" for s in range(x.S)]
    assert not any(x.sub_on)
    x.call("device", what="all off, device")                    # the sentinel is intact: no word written, no modulator launched
    x.call("host", what="all off, host")
    x.call("device", tiled=True, with_sub=False, sub_from=None, what="all off, tiled, no sub")
    x.modulate_and_process("all off")
    x.close()
    one = Rig(flavor, 1, n=3)
    one.call("device", what="one stream")
    one.call("host", tiled=True, what="one stream, tiled")
    one.set_sub(0, False); one.call("host", what="one stream, off")
    one.set_sub(0, True); one.call("device", what="one stream, on again")
    one.modulate_and_process("one stream")
    one.close()
