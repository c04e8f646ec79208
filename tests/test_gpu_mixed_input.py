"""dspi_process_mixed on the GPU (include/dspi.h): 16- and 24-bit devices side by side in one call.

Every case is held to two things, for every stream:
  the oracle    each stream's own Oracle(detmath=True), fed the same packets AT ITS NATIVE DEPTH — pair words, sub words, per-packet peaks,
                clip flags, status bytes are equal.  This holds the widening identity to the reference's arithmetic, not only to the library's
                own 24-bit path.
  a twin        a second context with the same preset that gets CPU-widened input through dspi_process at 24 bit: every output word is equal.
                This isolates the intake (dspi_intake.hip on device buffers and on staged host buffers, intake_widen_cpu on the direct path).
The 16-bit streams take WL.synth_pcm16, the 24-bit streams WL.pcm16_to_pcm24_bytes of theirs, whose low bytes are not zero.

Shapes: 130 float streams (a whole row of 128 and a partial one), 70 Q28 streams (row 64); 96 kHz, 96-frame packets, 10 per call where nothing
else is said.  No figures: every comparison is for equality."""
import struct

import numpy as np
import pytest

from conftest import has_gpu
from orclib import Oracle, spdif_encode
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, context, fid, oracle, packets
from test_gpu_pdm_out import sub_setup

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B, N = 96000, 96, 10
FILL = 0xA5      # what a paused stream's input bytes hold: never read
R = W.REQ


def streams_of(flavor): return 130 if int(flavor) else 70


def widen(row16):
    """int16 [frames][2] -> the packed 24-bit bytes of s << 8, uint8 [frames * 6]"""
    s = np.ascontiguousarray(row16).reshape(-1).view(np.uint8).reshape(-1, 2)
    w = np.zeros((s.shape[0], 3), dtype=np.uint8)
    w[:, 1:] = s
    return w.reshape(-1)


class Rig:
    """A context, its twin and one oracle per slot.  `src[slot]` is the row of the input data the slot's stream is fed from (it follows the
    stream through a move); call() makes one dspi_process_mixed call and holds every stream to its oracle and to the twin."""

    def __init__(self, flavor, S, fs=FS, B=B, total=2 * N, rows=None, monkeypatch=None, staged=False):
        self.flavor, self.S, self.fs, self.B = flavor, S, fs, B
        self.blob = WL.full_chain_blob(int(flavor))
        if staged: monkeypatch.setenv("DSPI_NO_DIRECT", "1")      # (read once at dspi_create)
        self.d = context(flavor, S, fs, self.blob)
        if staged: monkeypatch.delenv("DSPI_NO_DIRECT", raising=False)
        self.t = context(flavor, S, fs, self.blob)
        self.o = [oracle(flavor, fs, self.blob) for _ in range(S)]
        self.p16 = WL.synth_pcm16(rows or S, B * total, fs)
        self.p24 = WL.pcm16_to_pcm24_bytes(self.p16)
        assert (self.p24.reshape(self.p24.shape[0], -1, 3)[:, :, 0] != 0).any(), "the 24-bit input's low bytes are not zero"
        self.src = list(range(S))
        self.paused = set()
        self.spdif_pos = 0

    def close(self):
        self.d.close(); self.t.close()

    def request(self, s, req, wvalue, payload):
        for x in (self.d, self.t): x.vendor_set(req, wvalue, payload, stream=s)
        self.o[s].vendor_set(req, wvalue, payload)

    def row(self, s, depth, p0, p1):
        """slot s's packets [p0, p1) at its native depth"""
        return packets(self.p16[self.src[s]], 16, self.B, p0, p1) if depth == 16 else packets(self.p24[self.src[s]], 24, self.B, p0, p1)

    def inputs(self, depths, p0, p1):
        """(the call's flat mixed buffer, the twin's packed 24-bit input [S][F * 6])"""
        F = (p1 - p0) * self.B
        parts, twin = [], np.full((self.S, F * 6), FILL, dtype=np.uint8)
        for s in range(self.S):
            if s in self.paused:
                parts.append(np.full(F * (6 if depths[s] == 24 else 4), FILL, dtype=np.uint8))
                continue
            r = self.row(s, depths[s], p0, p1)
            parts.append(np.ascontiguousarray(r).reshape(-1).view(np.uint8))
            twin[s] = widen(r) if depths[s] == 16 else r
        buf = np.concatenate(parts)
        total, off = self.d.mixed_pcm_bytes(depths, p1 - p0, self.B)
        assert total == buf.nbytes and off[-1] == total
        return buf, twin

    def call(self, depths, p0, p1, mem="host", tiled=False, spdif=False, pdm=False, what="", behind=None):
        """behind (device buffers): called right behind the asynchronous call, before anything waits for it; what it returns is returned too.
        The status bytes are then those after whatever it did and are not compared here."""
        d, S, Bk, n = self.d, self.S, self.B, p1 - p0
        F = n * Bk
        depths = np.asarray(depths, dtype=np.uint8)
        buf, twin_in = self.inputs(depths, p0, p1)
        before = d.direct_stats()["calls"]
        words = twords = None
        if mem == "device":
            import torch
            dev = torch.device("cuda", 0)
            t_pcm = torch.from_numpy(buf).to(dev)
            Rw = d.tile_streams(); nt = (S + Rw - 1) // Rw
            t_pairs = torch.zeros((nt, d.P * 2, F, Rw) if tiled else (S, d.P, F, 4 if spdif else 2), dtype=torch.int32, device=dev)
            t_sub = torch.zeros((nt, F, Rw) if tiled else (S, F), dtype=torch.int32, device=dev)
            t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
            t_clip = torch.zeros(S, dtype=torch.int16, device=dev)
            t_words = torch.zeros((nt, F, 8, Rw) if tiled else (S, F, 8), dtype=torch.int32, device=dev) if pdm else None
            torch.cuda.synchronize()
            d.process_mixed_device(t_pcm.data_ptr(), depths, n, Bk, t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), words_ptr=t_words.data_ptr() if pdm else 0,
                                   tiled=tiled, spdif=spdif, clip_ptr=t_clip.data_ptr())
            late = behind() if behind else None
            d.sync()
            pairs, sub = t_pairs.cpu().numpy(), t_sub.cpu().numpy()
            if spdif: pairs = pairs.view(np.uint32)
            peaks, clip = t_peaks.cpu().numpy().view(np.uint16), t_clip.cpu().numpy().view(np.uint16)
            if pdm: words = t_words.cpu().numpy().view(np.uint32)
        else:
            got = d.process_mixed_host(buf, depths, n, Bk, tiled=tiled, spdif=spdif, clip=True, pdm=pdm)
            pairs, sub, peaks = got[:3]
            clip = d.last_clip.copy()
            if pdm: words = got[3]
            if mem != "host": assert (d.direct_stats()["calls"] > before) == (mem == "direct"), f"{what}: the call did not take the memory path this case is about"
        self.verify((pairs, sub, peaks, clip, words), depths, p0, p1, twin_in, tiled, spdif, pdm, what, status=behind is None)
        if tiled: pairs, sub = d.untile(pairs, sub)
        return (pairs, sub, peaks, late) if behind else (pairs, sub, peaks)

    def verify(self, got, depths, p0, p1, twin_in, tiled=False, spdif=False, pdm=False, what="", status=True):
        """one call's outputs against the twin (which makes its call here) and against every stream's oracle (which is fed here)"""
        d, t, S, Bk, n = self.d, self.t, self.S, self.B, p1 - p0
        F = n * Bk
        pairs, sub, peaks, clip, words = got
        # the twin: dspi_process / dspi_process_pdm at 24 bit on CPU-widened input — every output word
        if pdm: tp, ts, tk, twords = t.process_pdm_host(twin_in, n, Bk, 24, tiled=tiled)
        else: tp, ts, tk = t.process_host(twin_in, n, Bk, 24, tiled=tiled, spdif=spdif, clip=True)
        assert np.array_equal(pairs, tp), f"{what}: pair words differ from the twin's: streams {sorted(set(np.argwhere(pairs != tp)[:, 0].tolist()))[:8]}"
        assert np.array_equal(sub, ts), f"{what}: sub words differ from the twin's"
        assert np.array_equal(peaks, tk), f"{what}: peaks differ from the twin's"
        if pdm: assert np.array_equal(words, twords), f"{what}: PDM words differ from dspi_process_pdm's on the twin"
        else: assert np.array_equal(clip, t.last_clip), f"{what}: clip flags differ from the twin's"
        # the oracles, at the native depths
        if tiled: pairs, sub = d.untile(pairs, sub)
        for s in range(S):
            o = self.o[s]
            if s in self.paused:
                assert not pairs[s].any() and not sub[s].any() and not peaks[s].any(), f"{what}: paused stream {s} has output"
                if status: assert d.status(s) == o.status(), f"{what}: paused stream {s}: status"
                continue
            rp, rs, rk, rclip = o.process(self.row(s, depths[s], p0, p1), n, Bk, int(depths[s]))
            if spdif: rp = np.stack([spdif_encode(rp[p], self.spdif_pos, self.fs)[0] for p in range(d.P)])
            assert np.array_equal(rp, pairs[s]), f"{what}: stream {s} ({depths[s]} bit): pair words differ from the oracle's"
            assert np.array_equal(rs, sub[s]), f"{what}: stream {s} ({depths[s]} bit): sub words differ from the oracle's"
            assert np.array_equal(rk, peaks[s]), f"{what}: stream {s} ({depths[s]} bit): peaks differ from the oracle's"
            assert int(clip[s]) == rclip, f"{what}: stream {s}: clip flags"
            if status: assert d.status(s) == o.status(), f"{what}: stream {s}: status bytes"
        if spdif: self.spdif_pos = (self.spdif_pos + F) % 192


def pattern(name, S):
    s = np.arange(S)
    if name == "alternating": return np.where(s % 2 == 1, 24, 16)
    if name == "thirds": return np.where(s % 3 == 0, 24, 16)
    if name == "one16": return np.where(s == 5, 16, 24)
    if name == "row16": return np.where(s < (128 if S > 128 else 64), 16, 24)      # a whole 16-bit row beside a 24-bit row
    if name == "random": return np.random.default_rng(11).choice(np.array([16, 24]), S)
    if name == "all16": return np.full(S, 16)
    if name == "all24": return np.full(S, 24)
    raise KeyError(name)


# ---- 1. depth patterns ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["alternating", "one16", "row16", "random", "all16", "all24"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_depth_patterns(flavor, name):
    S = streams_of(flavor)
    x = Rig(flavor, S, total=N)
    depths = pattern(name, S).astype(np.uint8)
    got = x.call(depths, 0, N, what=name)
    if name.startswith("all"):      # uniform depths: the call IS dspi_process at that depth
        depth = int(depths[0])
        u = context(flavor, S, FS, x.blob)
        data = x.p16 if depth == 16 else x.p24
        want = u.process_host(packets(data, depth, B, 0, N), N, B, depth)
        for a, b in zip(got, want): assert np.array_equal(a, b), "uniform depths differ from dspi_process"
        u.close()
    x.close()


# ---- 2. short runs, runs that are only 2-byte aligned -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("name", ["alternating", "thirds"])
@pytest.mark.parametrize("n,Bk", [(1, 1), (3, 45), (9, 44), (1, 192)], ids=["1x1", "3x45", "9x44", "1x192"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_short_and_unaligned_runs(flavor, n, Bk, name, mem, monkeypatch):
    """two consecutive calls (state carries): runs of 4 / 6 bytes, of 540 / 810, of 1584 / 2376 and of 768 / 1152; with F odd a 24-bit run
    is 6 mod 12 bytes long, so most runs start 2, 6 or 10 bytes off a 16-byte boundary on one side or both.  Host buffers: the staged path
    (the intake kernel again, fed by the chunk upload)."""
    S = streams_of(flavor)
    x = Rig(flavor, S, B=Bk, total=2 * n, monkeypatch=monkeypatch, staged=mem == "host")
    depths = pattern(name, S)
    x.call(depths, 0, n, mem=mem if mem == "device" else "staged", what="first call")
    x.call(depths, n, 2 * n, mem=mem if mem == "device" else "staged", what="second call")
    x.close()


# ---- 3. the three memory paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "direct", "staged"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_memory_paths(flavor, mem, monkeypatch):
    """device: a torch tensor's data_ptr(); direct: host arrays at 1 x 48 frames (the CPU copy widens); staged: DSPI_NO_DIRECT=1"""
    S = streams_of(flavor)
    n, Bk = (1, 48) if mem == "direct" else (N, B)
    x = Rig(flavor, S, B=Bk, total=3 * n, monkeypatch=monkeypatch, staged=mem == "staged")
    depths = pattern("random", S)
    for k in range(3): x.call(depths, k * n, (k + 1) * n, mem=mem, what=f"{mem}, call {k}")
    x.close()


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_staged_in_chunks(flavor):
    """a host call that moves 32 MiB or more takes the staged path's pipeline (dspi_plan.cpp plan_call: here two chunks of one row each, the
    caller's buffers pinned): each chunk's byte range of the mixed buffer goes up by itself, behind it the intake of that chunk's streams"""
    S = streams_of(flavor)
    n = 65 if int(flavor) else 193
    x = Rig(flavor, S, total=n)
    assert S * n * B * (6 + 8 * x.d.P + 4) >= 32 << 20 and S > x.d.tile_streams()
    x.call(pattern("random", S), 0, n, mem="staged", what="two chunks")
    x.close()


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_staged_call_behind_an_unsynchronised_device_call(flavor):
    """A device-buffer call is asynchronous; the header lets a host call follow it without dspi_sync.  Here the host call is one that takes the
    staged pipeline with two chunks, whose uploads run on a stream of their own: they must not touch what the device call still reads (the two
    paths keep separate scratches).  The widening pass alone (dspi_debug_intake) is queued in between too: it writes the device path's scratch
    behind the chain that reads it, on the same stream.  Both calls equal their oracles and the twin."""
    S = streams_of(flavor)
    n1, n2 = 10, 65 if int(flavor) else 193
    x = Rig(flavor, S, total=n1 + n2)
    assert S * n2 * B * (6 + 8 * x.d.P + 4) >= 32 << 20
    depths = pattern("random", S).astype(np.uint8)
    buf2, twin2 = x.inputs(depths, n1, n1 + n2)

    import torch
    t_buf2 = torch.from_numpy(buf2).to("cuda:0")      # (there before the device call: nothing below waits for the GPU until that call is queued)
    torch.cuda.synchronize()

    def behind():
        x.d.debug_intake(t_buf2.data_ptr(), depths, n2, B)
        got = x.d.process_mixed_host(buf2, depths, n2, B, clip=True)
        return got + (x.d.last_clip.copy(), None)
    late = x.call(depths, 0, n1, mem="device", what="the device call", behind=behind)[3]
    x.verify(late, depths, n1, n1 + n2, twin2, what="the staged call behind it")
    x.close()


# ---- 4. output flags ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("flag", ["tiled", "spdif"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_output_flags(flavor, flag, mem):
    """DSPI_OUT_TILED, and DSPI_OUT_SPDIF (off the latency layout a two-pass route: the chain's words, then the encoder), two calls each"""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=4)
    depths = pattern("alternating", S)
    for k in range(2): x.call(depths, 2 * k, 2 * k + 2, mem=mem, tiled=flag == "tiled", spdif=flag == "spdif", what=f"{flag}, call {k}")
    x.close()


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_pdm_words(flavor, mem):
    """pdm_words, the sub on on every third stream: the words of dspi_process_pdm on the twin"""
    S = streams_of(flavor)
    x = Rig(flavor, S, B=48, total=4)
    for s in range(S):
        if s % 3 == 0:
            for y in (x.d, x.t): sub_setup(y, flavor, stream=s)
            sub_setup(x.o[s], flavor)
        else: x.request(s, R["SET_OUTPUT_ENABLE"], x.d.N - 1, b"\x00")
    for s in range(S): assert (x.d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=s) == b"\x01") == (s % 3 == 0), f"stream {s}: GET_CORE1_MODE"
    depths = pattern("alternating", S)
    for k in range(2): x.call(depths, 2 * k, 2 * k + 2, mem=mem, pdm=True, what=f"pdm, call {k}")
    assert x.d.pdm_running().tolist() == [1 if s % 3 == 0 else 0 for s in range(S)] == x.t.pdm_running().tolist()
    x.close()


# ---- 5. paused streams --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "direct", "staged"])
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_paused_streams(flavor, mem, monkeypatch):
    """paused slots: their input bytes hold 0xA5 and are never read, their state and status are the oracle's that was not fed, and after the
    resume they continue exactly.  A paused slot's depth differs from its neighbours': its entry still sizes its run."""
    S = streams_of(flavor)
    n, Bk = (1, 48) if mem == "direct" else (3, B)
    x = Rig(flavor, S, B=Bk, total=3 * n, monkeypatch=monkeypatch, staged=mem == "staged")
    who = (3, 64, 129) if int(flavor) else (3, 64)
    depths = np.full(S, 16, dtype=np.uint8)
    depths[1::4] = 24
    for s in who: depths[s] = 24; depths[s - 1] = 16; depths[s + 1 if s + 1 < S else s - 1] = 16
    x.call(depths, 0, n, mem=mem, what="before the pause")
    for s in who:
        for y in (x.d, x.t): assert y.pause_streams(s, 1) == 1
        x.paused.add(s)
    x.call(depths, n, 2 * n, mem=mem, what="paused")
    for s in who:
        for y in (x.d, x.t): assert y.resume_streams(s, 1, as_is=True) == 1
    x.paused.clear()
    # (the paused streams missed packets [n, 2n): they go on with [2n, 3n) like everyone else, their oracles were not fed in between)
    x.call(depths, 2 * n, 3 * n, mem=mem, what="after the resume")
    x.close()


# ---- 6. a format change -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_format_change(flavor):
    """the host re-opens stream 5 at the other depth between two calls: its oracle is fed accordingly, its neighbours are untouched"""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=6)
    depths = pattern("thirds", S).astype(np.uint8)
    assert depths[5] == 16
    x.call(depths, 0, 2, mem="device", what="16 bit")
    depths[5] = 24
    x.call(depths, 2, 4, mem="device", what="24 bit")
    depths[5] = 16
    x.call(depths, 4, 6, mem="device", what="16 bit again")
    x.close()


# ---- 7. after a lifecycle call --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_after_a_move(flavor):
    """a dspi_move_streams swap of a 16-bit and a 24-bit stream: the caller swaps the depth entries and the buffer slots, both continue exactly"""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=4)
    depths = pattern("alternating", S).astype(np.uint8)
    a, b = 6, S - 3
    assert depths[a] != depths[b]
    x.call(depths, 0, 2, what="before the move")
    for y in (x.d, x.t): assert y.move_streams([(a, b), (b, a)]) == 2
    depths[a], depths[b] = depths[b], depths[a]
    x.src[a], x.src[b] = x.src[b], x.src[a]
    x.o[a], x.o[b] = x.o[b], x.o[a]
    x.call(depths, 2, 4, what="after the move")
    x.close()


@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_after_a_grow(flavor):
    """dspi_resize_streams grows the context by 30 streams, the depth vector grows with it: the old streams continue exactly, the new ones are
    devices that have just been powered on"""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=4, rows=S + 30)
    x.call(pattern("alternating", S), 0, 2, mem="device", what="before the grow")
    n = S + 30
    for y in (x.d, x.t): assert y.resize_streams(n) == n
    x.S = n
    x.src += list(range(S, n))
    x.o += [Oracle(flavor, detmath=True) for _ in range(S, n)]
    x.call(pattern("thirds", n), 2, 4, mem="device", what="after the grow")
    x.call(pattern("thirds", n), 2, 4, what="after the grow, host buffers")      # (the same packets again: every oracle is fed them again too)
    x.close()


# ---- 7b. other front ends in between ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_table_survives_other_front_ends(flavor):
    """The device's table of a call's front end is one buffer for every kind of call, and a mixed call keeps its own there while the depths
    and the frame count repeat.  mixed, packets, mixed, patched, mixed on one context, device buffers, the same depths and 2 x 48 frames every
    time: each mixed call would find its table cached unless the call in between had said that the table is no longer a mixed call's.  The
    packet table describes the mixed layout itself, the patched call takes the depths as its sources (no LINK stream, no view).  A twin makes
    five plain mixed calls on the same bytes: pairs, sub, peaks and clip flags are equal after every call.  One full row and 3 streams."""
    from test_gpu_packets import Outs, Source, contiguous, run_mixed, run_packets, same, to_dev
    n, Bk = 2, 48
    blob = WL.full_chain_blob(int(flavor))
    probe = context(flavor, 1, FS, blob)
    S = probe.tile_streams() + 3
    probe.close()
    d, t = context(flavor, S, FS, blob), context(flavor, S, FS, blob)
    depths = pattern("alternating", S).astype(np.uint8)
    src = Source(S, Bk, 5 * n)
    _, at = d.mixed_pcm_bytes(depths, n, Bk)

    def run_patched(buf):
        total, off = d.patched_bytes(depths, n, Bk)
        pin = np.full(max(total, 16), FILL, dtype=np.uint8)
        for s in range(S): pin[int(off[s]):int(off[s]) + int(at[s + 1] - at[s])] = buf[int(at[s]):int(at[s + 1])]
        a, o = to_dev(pin), Outs(d, n, Bk)
        d.process_patched_device(a.data_ptr(), depths, None, None, n, Bk, pairs_ptr=o.pairs.data_ptr(), **o.ptrs())
        d.sync()
        return o.fetch()

    for k, kind in enumerate(("mixed", "packets", "mixed", "patched", "mixed")):
        buf, table = contiguous(lambda s, p: src.packet(s, depths[s], k * n + p), depths, n)
        assert buf.size == at[-1]
        want = run_mixed(t, buf, depths, n, Bk)
        got = run_packets(d, buf, depths, table, n, Bk) if kind == "packets" else run_patched(buf) if kind == "patched" else run_mixed(d, buf, depths, n, Bk)
        same(got, want, f"call {k} ({kind})")
    d.close(); t.close()


# ---- 8. the refusal -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_preamp_refusal(flavor):
    """REQ_SET_PREAMP_CH channel 0 at -640 dB on stream 7 (10^-32 < 2^-103).  Float: with stream 7 at 16 bit the call is refused and nothing was
    advanced — the following legal call, stream 7 at 24 bit, equals every oracle from the first packet.  Q28: both succeed."""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=4)
    x.request(7, R["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0))
    depths = pattern("thirds", S).astype(np.uint8)
    assert depths[7] == 16
    if int(flavor):
        buf, _ = x.inputs(depths, 0, 2)
        with pytest.raises(DspiError) as e: x.d.process_mixed_host(buf, depths, 2, B)
        assert e.value.code == host.E_UNSUPPORTED and "stream 7" in str(e.value)
        import torch
        t_pcm = torch.from_numpy(buf).to("cuda:0"); t_sub = torch.zeros((S, 2 * B), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(DspiError) as e: x.d.process_mixed_device(t_pcm.data_ptr(), depths, 2, B, sub_ptr=t_sub.data_ptr())
        assert e.value.code == host.E_UNSUPPORTED
        x.d.sync()
        assert not t_sub.cpu().numpy().any(), "a refused call wrote"
        depths[7] = 24
    x.call(depths, 0, 2, what="the legal call")
    x.call(depths, 2, 4, what="the call after")
    x.close()


@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_small_preamp_that_is_not_refused(flavor):
    """-600 dB (10^-30 >= 2^-103) on a 16-bit stream: the call succeeds and equals the oracle"""
    S = streams_of(flavor)
    x = Rig(flavor, S, total=4)
    x.request(7, R["SET_PREAMP_CH"], 0, struct.pack("<f", -600.0))
    depths = pattern("thirds", S)
    assert depths[7] == 16
    x.call(depths, 0, 2, what="-600 dB")
    x.call(depths, 2, 4, mem="device", what="-600 dB, device buffers")
    x.close()
