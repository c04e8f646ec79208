"""Per-stream S/PDIF block positions on the GPU (dspi_spdif_per_stream / dspi_spdif_stream_pos / dspi_spdif_encode_v, include/dspi.h).
The expectation is always the oracle's encoder, per stream and pair: orclib.spdif_encode(words[s, p], pos_s, fs_s), where `words` are the
pair words of a TWIN context that goes through the same calls without DSPI_OUT_SPDIF (other tests pin those words to the oracle) and pos_s
is the test's own arithmetic (Book below: one position per stream, a flagged call adds its frames to every active one).

Shapes: float S = 150 (R = 128: one full row and a ragged one with an odd last stream), Q28 S = 100 (R = 64), 48 kHz, 48-frame packets;
the staged-chunk test alone needs 256 streams x 1 920 frames, the smallest call that the host-buffer path cuts in two."""
import numpy as np
import pytest

import orclib
from conftest import has_gpu
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_gpu_snapshot import context

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48
FILL = 0x5A5A5A5A
WARM = 12      # packets before anything is compared: a context's first 512 samples are the power-on mute, whose words are all zero


def warm(d, seed=900):
    """the power-on mute played out, without DSPI_OUT_SPDIF (no position moves)"""
    d.process_host(WL.synth_pcm16(d.n_streams, WARM * B, FS, first_stream=seed), WARM, B, 16)
    return d


def size(flavor):
    return 150 if int(flavor) else 100


def expect(words, pos, fs, streams=None):
    """{stream: uint32 [P][F][4]} from the oracle's encoder; fs: one rate or one per stream"""
    out = {}
    for s in (range(words.shape[0]) if streams is None else streams):
        rate = int(fs[s]) if np.ndim(fs) else int(fs)
        out[int(s)] = np.stack([orclib.spdif_encode(words[s, p], int(pos[s]), rate)[0] for p in range(words.shape[1])])
    return out


def assert_streams(got, want, what):
    for s, w in want.items():
        assert np.array_equal(got[s], w), f"{what}: subframes of stream {s} differ at {np.argwhere(got[s] != w)[:3].tolist()}"


def tile_words(pairs, R):
    """stream-major pair words [S][P][F][2] -> DSPI_OUT_TILED [tile][2P][F][R]"""
    S, P, F, _ = pairs.shape
    nt = -(-S // R)
    t = np.zeros((nt * R, 2 * P, F), dtype=np.int32)
    t[:S] = pairs.transpose(0, 1, 3, 2).reshape(S, 2 * P, F)
    return np.ascontiguousarray(t.reshape(nt, R, 2 * P, F).transpose(0, 2, 3, 1))


def untile_subframes(sf, S):
    """[tile][P][F][4][R] -> [S][P][F][4]"""
    nt, P, F, _, R = sf.shape
    return sf.transpose(0, 4, 1, 2, 3).reshape(nt * R, P, F, 4)[:S]


def process_spdif(d, pcm, n, mem):
    """one DSPI_OUT_SPDIF call: the subframes, uint32 [S][P][F][4]; device buffers are pre-filled with FILL"""
    if mem == "host": return d.process_host(pcm, n, B, 16, spdif=True)[0]
    import torch
    dev = torch.device("cuda", 0)
    S, F = d.n_streams, n * B
    t_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    t_pairs = torch.full((S, d.P, F, 4), FILL, dtype=torch.int32, device=dev)
    t_sub = torch.zeros((S, F), dtype=torch.int32, device=dev); t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    d.process_device(t_pcm.data_ptr(), n, B, 16, t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), spdif=True)
    d.sync()
    return t_pairs.cpu().numpy().view(np.uint32)


class Book:
    """the test's own arithmetic: one position per stream, who is paused, and the two contexts that go through the same calls — x with
    DSPI_OUT_SPDIF and per-stream positions, the twin t without the flag"""

    def __init__(self, flavor, mem, packets):
        self.S, self.mem = size(flavor), mem
        blob = WL.full_chain_blob(flavor)
        self.x, self.t = warm(context(flavor, self.S, FS, blob)), warm(context(flavor, self.S, FS, blob))
        self.pcm = WL.synth_pcm16(self.S, packets * B, FS)
        self.at = 0
        self.pos = np.zeros(self.S, dtype=np.int64)
        self.active = np.ones(self.S, dtype=bool)
        self.ctx_pos = 0
        self.fs = np.full(self.S, FS)      # each stream's rate: the sample-rate byte of its channel status

    def both(self, name, *args, **kw):
        return [getattr(d, name)(*args, **kw) for d in (self.x, self.t)]

    def check_get(self, what):
        if self.x.spdif_per_stream(): assert np.array_equal(self.x.spdif_stream_pos(), self.pos), f"{what}: dspi_spdif_stream_pos is not the test's arithmetic"
        assert self.x.spdif_block_pos() == self.ctx_pos, f"{what}: the context's own value"

    def call(self, n, what):
        """one call on both contexts; every active stream against the oracle's encoder at its own position, paused regions untouched"""
        pcm = np.ascontiguousarray(self.pcm[:, self.at * B:(self.at + n) * B]); self.at += n
        words = self.t.process_host(pcm, n, B, 16)[0]
        assert int(np.abs(words[self.active]).max()) > 0 or not self.active.any()
        got = process_spdif(self.x, pcm, n, self.mem)
        assert_streams(got, expect(words, self.pos, self.fs, np.flatnonzero(self.active)), what)
        p = ~self.active
        if p.any(): assert (got[p] == (0 if self.mem == "host" else FILL)).all(), f"{what}: a paused stream's region was written"
        self.pos[self.active] = (self.pos[self.active] + n * B) % 192
        self.ctx_pos = (self.ctx_pos + n * B) % 192
        self.check_get(what)
        return got

    def close(self):
        self.x.close(); self.t.close()


# ---- 1. dspi_spdif_encode_v -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
def test_encode_v(flavor):
    """random positions (0, 191 and values that wrap inside the call among them), streams at three rates: stream-major with an even frame
    count (the frame-pair kernel) and an odd one, tiled, host and device buffers; equal positions give dspi_spdif_encode's words"""
    import torch
    S, F = size(flavor), 144
    d = context(flavor, S, FS, WL.full_chain_blob(flavor))
    rates = np.full(S, FS)
    for s, r in ((1, 44100), (2, 96000), (S - 1, 44100), (S - 2, 96000)):
        assert d.set_rate(r, stream=s) == 0; rates[s] = r
    R, P = d.tile_streams(), d.P
    words = warm(d).process_host(WL.synth_pcm16(S, F, FS), 3, B, 16)[0]
    assert int(np.abs(words[:, :, :B]).max()) > 0
    pos = np.random.default_rng(7).integers(0, 192, S).astype(np.uint32)
    pos[[0, 1, 2, 3, S - 1]] = (0, 191, 100, 148, 191)      # 100 + 144 and 148 + 45 wrap inside the call, 191 at its second frame
    want = expect(words, pos, rates)
    odd = np.ascontiguousarray(words[:, :, :45])
    want_odd = {s: w[:, :45] for s, w in want.items()}
    # host buffers
    assert_streams(d.spdif_encode_v_host(words, pos), want, "host, stream-major, 144 frames")
    assert_streams(d.spdif_encode_v_host(odd, pos), want_odd, "host, stream-major, 45 frames")
    assert_streams(untile_subframes(d.spdif_encode_v_host(tile_words(words, R), pos, tiled=True), S), want, "host, tiled, 144 frames")
    # device buffers; positions there are taken modulo 192
    dev = torch.device("cuda", 0)
    big = (pos + 192 * np.linspace(0, 22369619, S).astype(np.uint64)).astype(np.uint32)      # (the largest multiples of 192 that fit)
    assert big.max() > 2 ** 31 and np.array_equal(big % 192, pos)
    t_pos = torch.from_numpy(big.view(np.int32)).to(dev)
    for tiled, w, wanted, what in ((False, words, want, "device, stream-major, 144 frames"), (False, odd, want_odd, "device, stream-major, 45 frames"),
                                   (True, tile_words(odd, R), want_odd, "device, tiled, 45 frames")):
        t_in = torch.from_numpy(w).to(dev)
        n_frames = w.shape[2]
        t_out = torch.full((-(-S // R), P, n_frames, 4, R) if tiled else (S, P, n_frames, 4), FILL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.spdif_encode_v_device(t_in.data_ptr(), n_frames, t_pos.data_ptr(), t_out.data_ptr(), tiled=tiled)
        d.sync()
        got = t_out.cpu().numpy().view(np.uint32)
        if tiled:
            nt = -(-S // R)
            if nt * R > S: assert (got.transpose(0, 4, 1, 2, 3).reshape(nt * R, -1)[S:] == FILL).all(), "columns past the last stream were written"
            got = untile_subframes(got, S)
        assert_streams(got, wanted, what)
    # all positions equal: dspi_spdif_encode, word for word (both stream-major kernels and the tiled one)
    same = np.full(S, 77, dtype=np.uint32)
    for w, tiled in ((words, False), (odd, False), (tile_words(words, R), True)):
        assert np.array_equal(d.spdif_encode_v_host(w, same, tiled=tiled), d.spdif_host(w, 77, tiled=tiled)[0]), (w.shape, tiled)
    # refusals: a host position of 192, an undefined flag bit, a null list
    bad = pos.copy(); bad[S // 2] = 192
    with pytest.raises(DspiError) as e: d.spdif_encode_v_host(words, bad)
    assert e.value.code == host.E_INVAL
    out = np.zeros((S, P, F, 4), dtype=np.uint32)
    for flags in (0x4, 0x10, 0x100, 0x80000000):
        assert d.L.dspi_spdif_encode_v(d.h, words.ctypes.data, F, pos.ctypes.data, out.ctypes.data, flags) == host.E_INVAL, hex(flags)
    assert d.L.dspi_spdif_encode_v(d.h, words.ctypes.data, F, None, out.ctypes.data, 0) == host.E_INVAL
    assert not out.any()
    d.close()


# ---- 2. dspi_process in the mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,layout", [(W.F32_FMA, "packed"), (W.F32_FMA, "skew"), (0, "packed")], ids=("fma-two-pass", "fma-latency-layout", "q28"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_process(flavor, layout, mem, monkeypatch):
    """two calls of 3 x 48 frames from distinct positions, so that every stream wraps; on the latency layout the two-pass route runs over the
    latency kernels.  Beside it: with the mode on and no position set, the words are a mode-off context's."""
    monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    n = 3
    k = Book(flavor, mem, 2 * n)
    S = k.S
    assert k.x.spdif_block_pos(50) == 50; k.ctx_pos = 50
    assert k.x.spdif_per_stream(1) is True
    k.pos[:] = 50
    k.check_get("after the enable")
    k.pos[:] = (np.arange(S) * 7 + 191) % 192      # distinct, with 191 (stream 0) and 0 (stream 55) among them; 288 frames: everybody wraps
    assert len(set(k.pos.tolist())) == S and {0, 191} <= set(k.pos.tolist())
    assert np.array_equal(k.x.spdif_stream_pos(set=k.pos), k.pos)
    blob = WL.full_chain_blob(flavor)
    on, off = warm(context(flavor, S, FS, blob)), warm(context(flavor, S, FS, blob))
    for d in (on, off): assert d.spdif_block_pos(50) == 50
    assert on.spdif_per_stream(1) is True
    for c in range(2):
        got = k.call(n, f"call {c}")
        plan = k.x.launch_plan()
        assert (plan["latency_layout"] > 0 and plan["packed_shared"] == 0) if layout == "skew" else plan["latency_layout"] == 0, plan
        pcm = np.ascontiguousarray(k.pcm[:, c * n * B:(c + 1) * n * B])
        a, b = process_spdif(on, pcm, n, mem), process_spdif(off, pcm, n, mem)
        assert np.array_equal(a, b), f"call {c}: mode on without a set differs from mode off"
        assert on.spdif_block_pos() == off.spdif_block_pos() == k.ctx_pos and set(on.spdif_stream_pos().tolist()) == {k.ctx_pos}
        assert not np.array_equal(a, got)
    # calls without the flag move nobody
    k.t.process_host(np.ascontiguousarray(k.pcm[:, :B]), 1, B, 16); k.x.process_host(np.ascontiguousarray(k.pcm[:, :B]), 1, B, 16)
    k.check_get("after a call without the flag")
    on.close(); off.close(); k.close()


# ---- 3. lifecycle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_lifecycle(flavor, mem):
    """pauses (one group across a row edge, one the last stream), moves (a swap and a one-way move into a paused slot), boots (an active and a
    paused slot) and an import, each followed by a call: positions freeze, travel, restart at 0 and stay as the header says"""
    k = Book(flavor, mem, 16)
    S, x = k.S, k.x
    R = x.tile_streams()
    k.call(1, "before the mode")      # (mode off: every stream at the context's position, which the Book's zeros are)
    assert x.spdif_per_stream(1) is True
    k.pos[:] = k.ctx_pos
    k.check_get("after the enable")
    k.pos[:] = (np.arange(S) * 11 + 5) % 192
    x.spdif_stream_pos(set=k.pos)
    k.call(2, "distinct positions")
    # pauses
    for first, count in ((4, 3), (R - 2, 6), (S - 1, 1)):
        k.both("pause_streams", first, count); k.active[first:first + count] = False
    k.check_get("after the pauses")
    frozen = k.pos[~k.active].copy()
    k.call(1, "paused, first call"); k.call(2, "paused, second call")
    assert np.array_equal(k.pos[~k.active], frozen)
    k.both("resume_streams", 0, S); k.active[:] = True
    k.check_get("after the resume")
    k.call(1, "resumed")
    # moves: a swap, and a one-way move into a paused slot (its source stays behind as a frozen copy)
    k.both("pause_streams", 40, 1); k.active[40] = False
    k.call(1, "slot 40 paused")
    assert k.pos[10] != k.pos[20] and k.pos[30] != k.pos[40]
    k.both("move_streams", [(10, 20), (20, 10), (30, 40)])
    k.pos[[10, 20]] = k.pos[[20, 10]]; k.pos[40] = k.pos[30]
    k.active[40], k.active[30] = True, False
    assert np.array_equal(x.streams_paused().astype(bool), ~k.active)
    k.check_get("after the moves")
    k.call(1, "moved")
    # boots: an active slot and a paused one
    k.both("boot_streams", [50, 30])
    k.pos[[50, 30]] = 0
    k.fs[[50, 30]] = 44100      # (the sample rate is a power-on value too: the channel status says 44.1 kHz until the host sets another)
    k.check_get("after the boots")
    got = k.call(1, "booted")
    z = orclib.spdif_encode(np.zeros((2, 2), dtype=np.int32), 0, FS)[0]      # (frame 0 with preamble Z, frame 1 with X)
    assert z[0, 0] & 0xFF != z[1, 0] & 0xFF
    assert ((got[50, :, 0, 0] & 0xFF) == (z[0, 0] & 0xFF)).all() and ((got[50, :, 1, 0] & 0xFF) == (z[1, 0] & 0xFF)).all(), "the first frame after a boot carries preamble Z"
    k.both("resume_streams", 30, 1); k.active[30] = True
    assert k.pos[30] == 0
    got = k.call(1, "the booted paused slot, resumed")
    assert ((got[30, :, 0, 0] & 0xFF) == (z[0, 0] & 0xFF)).all()
    # an import leaves the slot's position alone (the streams of a snapshot bring none)
    assert k.pos[60] != k.pos[70]
    for d in (k.x, k.t): assert d.import_streams(70, *d.export_streams(60, 1)) == 1
    k.check_get("after the import")
    k.call(2, "imported")
    k.close()


# ---- 4. staged chunks -----------------------------------------------------------------------------------------------------------------------
def test_staged_chunks():
    """host buffers of 20 x 96 frames on 256 float streams: 35 MB through the link, so the call is cut into two chunks of one row and the
    encoder runs once with a first stream above 0 — the position array is indexed by ABSOLUTE stream"""
    flavor, S, fs, Bk, n = W.F32_FMA, 256, 96000, 96, 20
    blob = WL.full_chain_blob(flavor)
    x, t = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    pcm = WL.synth_pcm16(S, n * Bk, fs)
    assert S * (n * Bk) * (4 * 16 + 4 + 4) >= 32 << 20 and x.tile_streams() == 128
    x.spdif_per_stream(1)
    pos = (np.arange(S) * 5 + 1) % 192
    assert len(set(pos[[0, 127, 128, 255]].tolist())) == 4
    x.spdif_stream_pos(set=pos)
    words = t.process_host(pcm, n, Bk, 16)[0]
    got = x.process_host(pcm, n, Bk, 16, spdif=True)[0]
    assert x.direct_stats()["calls"] == 0
    assert_streams(got, expect(words, pos, fs, (0, 127, 128, 255)), "two chunks")
    assert np.array_equal(x.spdif_stream_pos(), (pos + n * Bk) % 192)
    x.close(); t.close()


# ---- 5. failed calls, all-paused calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
def test_failed_call_moves_nobody(flavor):
    S = size(flavor)
    d = context(flavor, S, FS, WL.full_chain_blob(flavor))
    pcm = WL.synth_pcm16(S, 2 * B, FS)
    d.spdif_block_pos(33)
    d.spdif_per_stream(1)
    pos = (np.arange(S) * 13 + 2) % 192
    d.spdif_stream_pos(set=pos)
    with pytest.raises(DspiError) as e: d.process_host(pcm, 2, B, 16, spdif=True, tiled=True)
    assert e.value.code == host.E_INVAL
    with pytest.raises(DspiError): d.process_host(pcm, 2, B, 16, spdif=True, i2s_slots=True)
    assert np.array_equal(d.spdif_stream_pos(), pos) and d.spdif_block_pos() == 33
    # every stream paused: the context's value advances as it always did, no stream's does
    d.pause_streams(0, S)
    pairs = d.process_host(pcm, 2, B, 16, spdif=True)[0]
    assert not pairs.any()
    assert np.array_equal(d.spdif_stream_pos(), pos) and d.spdif_block_pos() == (33 + 2 * B) % 192
    d.close()
