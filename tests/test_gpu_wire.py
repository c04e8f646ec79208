"""S/PDIF and I2S slots in one call, per device, on the GPU (dspi_process_wire / dspi_wire_encode, include/dspi.h).  The expectation is always
the oracle's, per stream and pair by the stream's OWN output types: orclib.spdif_encode(words[s, p], pos_s, fs_s) for an S/PDIF slot,
orclib.i2s_frames(words[s, p]) in the first half of the region for an I2S slot — `words` being the pair words of a TWIN context that goes
through the same calls without the wire layout (other tests pin those words to the oracle), pos_s the test's own arithmetic.  Where the
reference's own encoders are built (oracle/_ref) a few streams are held to them as well.

Shapes: float S = 150 (R = 128: one full row and a partial one), Q28 S = 100 (R = 64), 48-frame packets; the staged-chunk test alone needs
256 streams x 1 920 frames, the smallest call that the host-buffer path cuts in two.  Types: five layouts (all S/PDIF, all I2S, slot 0 only,
the last slot only, alternating slots) by stream % 5, so neighbouring streams differ, and pairs inside a stream do."""
import math

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
WARM = 12      # packets before anything is compared: the power-on mute is 512 samples and a type switch arms one of 256, whose words are all zero
R = W.REQ


def size(flavor):
    return 150 if int(flavor) else 100


def type_table(S, P, only=None):
    """bool [S][P]: slot p of stream s is an I2S slot.  only: {stream: layout index}, every other stream all S/PDIF"""
    layouts = [(), tuple(range(P)), (0,), (P - 1,), tuple(range(0, P, 2))]
    t = np.zeros((S, P), dtype=bool)
    for s in range(S):
        k = s % 5 if only is None else only.get(s, 0)
        t[s, list(layouts[k])] = True
    return t


def set_types(d, types):
    for s, p in np.argwhere(types): assert d.vendor_get(R["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1, int(s)) == b"\x00"


def set_rates(d, rates):
    for s in np.flatnonzero(rates != FS): assert d.set_rate(int(rates[s]), stream=int(s)) == 0


def three_rates(S):
    rates = np.full(S, FS)
    for s, r in ((1, 44100), (2, 96000), (3, 44100), (4, 96000), (S - 1, 44100), (S - 2, 96000)): rates[s] = r
    return rates


def warm(d, seed=900):
    d.process_host(WL.synth_pcm16(d.n_streams, WARM * B, FS, first_stream=seed), WARM, B, 16)
    return d


def check(got, words, pos, fs, types, tail, what, streams=None, skip=()):
    """every region of `streams` against the oracle; tail: what the second half of an I2S region holds (0: host buffers, FILL: device)"""
    S, P, F, _ = words.shape
    ref_streams = set(list(range(min(S, 6))) + [S - 1]) if orclib.spdif_ref_available() and orclib.i2s_ref_available() else set()
    for s in (range(S) if streams is None else streams):
        if s in skip: continue
        rate = int(fs[s]) if np.ndim(fs) else int(fs)
        for p in range(P):
            region = got[s, p].reshape(-1)
            if types[s, p]:
                want = orclib.i2s_frames(words[s, p]).reshape(-1)
                assert np.array_equal(region[:2 * F], want), f"{what}: I2S words of stream {s} pair {p} differ at {np.flatnonzero(region[:2 * F] != want)[:3].tolist()}"
                assert (region[2 * F:] == tail).all(), f"{what}: the tail of stream {s} pair {p} is not {tail:#x}"
                if s in ref_streams:
                    ref = orclib.i2s_ref_give(words[s, p], B, math.gcd(F, 48))
                    assert len(ref) == F and np.array_equal(region[:2 * F], ref.reshape(-1)), f"{what}: stream {s} pair {p} against the reference's I2S producer"
            else:
                want = orclib.spdif_encode(words[s, p], int(pos[s]), rate)[0]
                assert np.array_equal(got[s, p], want), f"{what}: subframes of stream {s} pair {p} differ at {np.argwhere(got[s, p] != want)[:3].tolist()}"
                if s in ref_streams:
                    assert np.array_equal(got[s, p], orclib.spdif_encode(words[s, p], int(pos[s]), rate, ref=True)[0]), f"{what}: stream {s} pair {p} against the reference's encoder"


def process_wire(d, pcm, n, mem, enabled_only=False, pdm=False, clip=False):
    """one dspi_process_wire call: the wire words uint32 [S][P][F][4] (with pdm: and the PDM words); device buffers are pre-filled with FILL"""
    if mem == "host":
        r = d.process_wire_host(pcm, n, B, 16, enabled_only=enabled_only, pdm=pdm, clip=clip)
        return (r[0], r[3]) if pdm else r[0]
    import torch
    dev = torch.device("cuda", 0)
    S, F = d.n_streams, n * B
    t_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    t_wire = torch.full((S, d.P, F, 4), FILL, dtype=torch.int32, device=dev)
    t_sub = torch.zeros((S, F), dtype=torch.int32, device=dev); t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
    t_words = torch.zeros((S, F, 8), dtype=torch.int32, device=dev) if pdm else None
    t_clip = torch.zeros((S,), dtype=torch.int16, device=dev) if clip else None
    torch.cuda.synchronize()
    d.process_wire_device(t_pcm.data_ptr(), n, B, t_wire.data_ptr(), 16, t_sub.data_ptr(), t_peaks.data_ptr(), t_words.data_ptr() if pdm else 0, enabled_only=enabled_only,
                          clip_ptr=t_clip.data_ptr() if clip else 0)
    d.sync()
    if clip: d.last_clip = t_clip.cpu().numpy().view(np.uint16)
    wire = t_wire.cpu().numpy().view(np.uint32)
    return (wire, t_words.cpu().numpy().view(np.uint32)) if pdm else wire


def process_spdif(d, pcm, n, mem, enabled_only=False):
    """the twin's DSPI_OUT_SPDIF call on the same kind of buffers"""
    if mem == "host": return d.process_host(pcm, n, B, 16, spdif=True, enabled_only=enabled_only)[0]
    import torch
    dev = torch.device("cuda", 0)
    S, F = d.n_streams, n * B
    t_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    t_pairs = torch.full((S, d.P, F, 4), FILL, dtype=torch.int32, device=dev)
    t_sub = torch.zeros((S, F), dtype=torch.int32, device=dev); t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    d.process_device(t_pcm.data_ptr(), n, B, 16, t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), spdif=True, enabled_only=enabled_only)
    d.sync()
    return t_pairs.cpu().numpy().view(np.uint32)


def silent_pairs(x, flavor, **kw):
    """outputs 2..N-2 off and the sub on (the interlock of usb_audio.c:1891-1904 wants that order): every pair but pair 0 is silent"""
    N = W.dims(int(flavor))[1]
    for o in range(2, N - 1): x.vendor_set(R["SET_OUTPUT_ENABLE"], o, b"\x00", **kw)
    x.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01", **kw)


class Pair:
    """x takes the wire calls, the twin t the same packets without a flag; the test's own arithmetic of the positions beside them"""

    def __init__(self, flavor, packets, types=None, rates=None, setup=None, S=None):
        self.S = S or size(flavor)
        blob = WL.full_chain_blob(int(flavor))
        self.x, self.t = context(flavor, self.S, FS, blob), context(flavor, self.S, FS, blob)
        self.types = type_table(self.S, self.x.P) if types is None else types
        self.fs = np.full(self.S, FS) if rates is None else rates
        for d in (self.x, self.t):
            if setup: setup(d)
            set_rates(d, self.fs); set_types(d, self.types); warm(d)
        self.pcm = WL.synth_pcm16(self.S, packets * B, FS)
        self.at = 0
        self.pos = np.zeros(self.S, dtype=np.int64)
        self.active = np.ones(self.S, dtype=bool)
        self.ctx_pos = 0

    def packets(self, n):
        pcm = np.ascontiguousarray(self.pcm[:, self.at * B:(self.at + n) * B]); self.at += n
        return pcm

    def check_positions(self, what):
        if self.x.spdif_per_stream(): assert np.array_equal(self.x.spdif_stream_pos(), self.pos), f"{what}: dspi_spdif_stream_pos is not the test's arithmetic"
        assert self.x.spdif_block_pos() == self.ctx_pos, f"{what}: the context's own value"

    def call(self, n, mem, what, **kw):
        pcm = self.packets(n)
        r = self.t.process_pdm_host(pcm, n, B) if kw.get("pdm") else self.t.process_host(pcm, n, B, 16)
        words = r[0]
        assert int(np.abs(words[self.active]).max()) > 0
        got = process_wire(self.x, pcm, n, mem, **kw)
        wire = got[0] if kw.get("pdm") else got
        paused = np.flatnonzero(~self.active)
        check(wire, words, self.pos, self.fs, self.types, 0 if mem == "host" else FILL, what, skip=set(paused.tolist()))
        if len(paused): assert (wire[paused] == (0 if mem == "host" else FILL)).all(), f"{what}: a paused stream's region was written"
        self.pos[self.active] = (self.pos[self.active] + n * B) % 192
        self.ctx_pos = (self.ctx_pos + n * B) % 192
        self.check_positions(what)
        return (wire, got[1], r[3]) if kw.get("pdm") else wire

    def close(self):
        self.x.close(); self.t.close()


# ---- 1. dspi_wire_encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
def test_wire_encode(flavor):
    """144 frames (the frame-pair kernel) and 45 (the single-frame kernel: a wave spans regions of different type), positions 0, 191, 100 and
    148 among random ones (blocks wrap inside the call), streams at three rates; host buffers: I2S tails zero; device buffers pre-filled:
    the tails keep the fill, positions are taken modulo 192; no I2S slot anywhere: dspi_spdif_encode_v's words; the refusals"""
    import torch
    S, F = size(flavor), 144
    blob = WL.full_chain_blob(int(flavor))
    d, plain = context(flavor, S, FS, blob), context(flavor, S, FS, blob)
    rates, types = three_rates(S), type_table(S, d.P)
    assert all(types[s].tolist() != types[s + 1].tolist() for s in range(S - 1)) and {tuple(r) for r in types.tolist()} >= {(False,) * d.P, (True,) * d.P}
    for c in (d, plain): set_rates(c, rates)
    set_types(d, types)
    words = warm(d).process_host(WL.synth_pcm16(S, F, FS), 3, B, 16)[0]
    assert int(np.abs(words[:, :, :45]).max()) > 0
    pos = np.random.default_rng(7).integers(0, 192, S).astype(np.uint32)
    pos[[0, 1, 2, 3, S - 1]] = (0, 191, 100, 148, 191)      # 100 + 144 and 148 + 45 wrap inside the call, 191 at its second frame
    odd = np.ascontiguousarray(words[:, :, :45])
    # host buffers
    check(d.wire_encode_host(words, pos), words, pos, rates, types, 0, "host, 144 frames")
    check(d.wire_encode_host(odd, pos), odd, pos, rates, types, 0, "host, 45 frames")
    # device buffers; positions there are taken modulo 192
    dev = torch.device("cuda", 0)
    big = (pos + 192 * np.linspace(0, 22369619, S).astype(np.uint64)).astype(np.uint32)      # (the largest multiples of 192 that fit)
    assert big.max() > 2 ** 31 and np.array_equal(big % 192, pos)
    t_pos = torch.from_numpy(big.view(np.int32)).to(dev)
    for w, what in ((words, "device, 144 frames"), (odd, "device, 45 frames")):
        t_in = torch.from_numpy(w).to(dev)
        t_out = torch.full((S, d.P, w.shape[2], 4), FILL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.wire_encode_device(t_in.data_ptr(), w.shape[2], t_pos.data_ptr(), t_out.data_ptr())
        d.sync()
        check(t_out.cpu().numpy().view(np.uint32), w, pos, rates, types, FILL, what)
    # no I2S slot anywhere: dspi_spdif_encode_v, word for word (both kernels)
    for w in (words, odd): assert np.array_equal(plain.wire_encode_host(w, pos), plain.spdif_encode_v_host(w, pos)), w.shape
    # refusals: a host position of 192, every flag but DSPI_MEM_DEVICE, a null list
    bad = pos.copy(); bad[S // 2] = 192
    with pytest.raises(DspiError) as e: d.wire_encode_host(words, bad)
    assert e.value.code == host.E_INVAL
    out = np.zeros((S, d.P, F, 4), dtype=np.uint32)
    for flags in (0x2, 0x4, 0x8, 0x10, 0x20, 0x100, 0x80000000):
        assert d.L.dspi_wire_encode(d.h, words.ctypes.data, F, pos.ctypes.data, out.ctypes.data, flags) == host.E_INVAL, hex(flags)
    assert d.L.dspi_wire_encode(d.h, words.ctypes.data, F, None, out.ctypes.data, 0) == host.E_INVAL
    assert not out.any()
    d.close(); plain.close()


# ---- 2. dspi_process_wire -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,layout", [(W.F32_FMA, "packed"), (W.F32_FMA, "skew"), (0, "packed")], ids=("fma-packed", "fma-latency-layout", "q28"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_process_wire(flavor, layout, mem, monkeypatch):
    """two calls of 3 x 48 frames with the context's one position, then two with per-stream positions on and distinct (every stream wraps), a
    paused stream in the middle of a row throughout; on the latency layout the two-pass route runs over the latency kernels"""
    monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    n = 3
    k = Pair(flavor, 4 * n, rates=three_rates(size(flavor)))
    S, x = k.S, k.x
    for d in (k.x, k.t): d.pause_streams(71, 1)
    k.active[71] = False
    assert k.types[71].all() and not k.types[70].any() and k.types[72].any()
    assert x.spdif_block_pos(50) == 50
    k.ctx_pos = 50; k.pos[:] = 50
    for c in range(2): k.call(n, mem, f"one position, call {c}")
    plan = x.launch_plan()
    assert (plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0) if layout == "skew" else plan["latency_layout"] == 0, plan
    assert x.spdif_per_stream(1) is True
    k.pos[:] = k.ctx_pos
    k.check_positions("after the enable")
    k.pos[:] = (np.arange(S) * 7 + 191) % 192      # distinct, with 191 (stream 0) and 0 (stream 55) among them; 288 frames: everybody wraps
    assert len(set(k.pos.tolist())) == S and {0, 191} <= set(k.pos.tolist())
    assert np.array_equal(x.spdif_stream_pos(set=k.pos), k.pos)
    frozen = k.pos[71]
    for c in range(2): k.call(n, mem, f"per-stream positions, call {c}")
    assert k.pos[71] == frozen and x.spdif_stream_pos(71, 1)[0] == frozen
    plan = x.launch_plan()
    assert (plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0) if layout == "skew" else plan["latency_layout"] == 0, plan
    k.close()


# ---- 3. the shortcut ----------------------------------------------------------------------------------------------------------------------
def test_shortcut(monkeypatch):
    """no I2S slot: the bytes of dspi_process(DSPI_OUT_SPDIF) on a twin, host and device.  Which route served a call shows with
    DSPI_OUT_ENABLED_ONLY on device buffers: the latency layout's fused encoder leaves silent pairs unwritten, the two-pass route writes the
    subframes of silence (include/dspi.h).  One stream with an I2S slot takes the call to the two-pass route; pausing that stream returns it"""
    monkeypatch.setenv("DSPI_F32_LAYOUT", "skew")
    flavor, n = W.F32_FMA, 2
    S = size(flavor)
    none = np.zeros((S, 4), dtype=bool)
    k = Pair(flavor, 12 * n, types=none, setup=lambda d: silent_pairs(d, flavor))
    x, t = k.x, k.t

    def same_as_spdif(what, mem, enabled_only):
        pcm = k.packets(n)
        assert t.spdif_block_pos(x.spdif_block_pos()) == x.spdif_block_pos()
        a, b = process_wire(x, pcm, n, mem, enabled_only=enabled_only), process_spdif(t, pcm, n, mem, enabled_only=enabled_only)
        assert np.array_equal(a, b), f"{what}: not the bytes of dspi_process(DSPI_OUT_SPDIF)"
        assert x.spdif_block_pos() == t.spdif_block_pos()
        assert (a[:, 0] != (FILL if mem == "device" else 0)).any()
        return a
    for mem in ("host", "device"): same_as_spdif(f"no I2S slot, {mem}", mem, False)
    a = same_as_spdif("no I2S slot, enabled only", "device", True)
    assert (a[k.active][:, 1:] == FILL).all(), "the fused encoder leaves silent pairs unwritten: the call did not run on the latency layout's own encoder"
    plan = x.launch_plan()
    assert plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0, plan
    # stream 9, slot 0 becomes I2S (both contexts: the switch mutes the pipeline): two passes, silent pairs carry silence in their own format
    for d in (x, t): set_types(d, type_table(S, 4, only={9: 2})); warm(d, seed=901)
    k.types = type_table(S, 4, only={9: 2})
    k.ctx_pos = x.spdif_block_pos(); k.pos[:] = k.ctx_pos
    wire = k.call(n, "device", "one I2S slot, enabled only", enabled_only=True)
    silence = orclib.spdif_encode(np.zeros((n * B, 2), dtype=np.int32), int(k.pos[3] - n * B) % 192, FS)[0]
    assert np.array_equal(wire[3, 1], silence) and np.array_equal(wire[9, 3], silence), "a silent S/PDIF pair carries the subframes of silence"
    plan = x.launch_plan()
    assert plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0, plan
    # ... and pausing that stream returns the call to the shortcut
    for d in (x, t): d.pause_streams(9, 1)
    k.active[9] = False
    a = same_as_spdif("the I2S stream paused, enabled only", "device", True)
    assert (a[k.active][:, 1:] == FILL).all() and (a[9] == FILL).all()
    same_as_spdif("the I2S stream paused, host", "host", False)
    k.close()


# ---- 4. staged chunks ---------------------------------------------------------------------------------------------------------------------
def test_staged_chunks():
    """host buffers of 20 x 96 frames on 256 float streams: the call is cut into two chunks of one row, so the wire encoder runs once with a
    first stream above 0 — types, rates, positions and the activity record are indexed by ABSOLUTE stream"""
    flavor, S, fs, Bk, n = W.F32_FMA, 256, 96000, 96, 20
    blob = WL.full_chain_blob(flavor)
    x, t = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    types = type_table(S, 4, only={0: 2, 127: 1, 128: 4, 255: 3})
    for d in (x, t): set_types(d, types)
    pcm = WL.synth_pcm16(S, n * Bk, fs)
    assert S * (n * Bk) * (4 * 16 + 4 + 4) >= 32 << 20 and x.tile_streams() == 128
    x.spdif_per_stream(1)
    pos = (np.arange(S) * 5 + 1) % 192
    x.spdif_stream_pos(set=pos)
    words = t.process_host(pcm, n, Bk, 16)[0]
    assert int(np.abs(words[[0, 127, 128, 255]]).max()) > 0
    got = x.process_wire_host(pcm, n, Bk, 16)[0]
    assert x.direct_stats()["calls"] == 0
    check(got, words, pos, fs, types, 0, "two chunks", streams=(0, 1, 126, 127, 128, 129, 254, 255))
    assert np.array_equal(x.spdif_stream_pos(), (pos + n * Bk) % 192)
    x.close(); t.close()


def test_staged_small(monkeypatch):
    """DSPI_NO_DIRECT=1: the small shape through the staged path, whose device buffer comes back whole (the encoder zeroes the I2S tails)"""
    monkeypatch.setenv("DSPI_NO_DIRECT", "1")
    k = Pair(W.F32_FMA, 6)
    k.call(3, "host", "staged, first call")
    for d in (k.x, k.t): d.pause_streams(129, 2)
    k.active[129:131] = False
    k.call(3, "host", "staged, second call, two streams paused")
    assert k.x.direct_stats()["calls"] == 0
    k.close()


# ---- 5. pdm_words, DSPI_OUT_ENABLED_ONLY, DSPI_OUT_CLIP_FLAGS -----------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_pdm_words_enabled_only_clip(flavor, mem):
    """the sub on and every pair but pair 0 silent: the PDM words are dspi_process_pdm's on the twin; with DSPI_OUT_ENABLED_ONLY a silent
    S/PDIF pair carries the subframes of silence at the stream's position and a silent I2S pair zero words; the clip flags are the twin's"""
    k = Pair(flavor, 6, setup=lambda d: silent_pairs(d, flavor))
    S, P = k.S, k.x.P
    k.x.spdif_per_stream(1)
    k.pos[:] = (np.arange(S) * 11 + 5) % 192
    k.x.spdif_stream_pos(set=k.pos)
    pos0 = k.pos.copy()
    wire, words_x, words_t = k.call(3, mem, "pdm words, enabled only", pdm=True, enabled_only=True)
    assert words_t.any() and np.array_equal(words_x, words_t), "the PDM words differ from dspi_process_pdm's"
    s_spdif, s_i2s = 5, 6      # layouts 0 (all S/PDIF) and 1 (all I2S)
    assert not k.types[s_spdif].any() and k.types[s_i2s].all()
    silence = orclib.spdif_encode(np.zeros((3 * B, 2), dtype=np.int32), int(pos0[s_spdif]), FS)[0]
    assert np.array_equal(wire[s_spdif, P - 1], silence), "a silent S/PDIF pair: the subframes of silence at the stream's position"
    assert not wire[s_i2s, P - 1].reshape(-1)[:2 * 3 * B].any(), "a silent I2S pair: zero words"
    # the clip flags
    pcm = k.packets(3)
    k.t.process_host(pcm, 3, B, 16, clip=True)
    process_wire(k.x, pcm, 3, mem, clip=True)
    assert np.array_equal(k.x.last_clip, k.t.last_clip), "DSPI_OUT_CLIP_FLAGS differs from the twin's"
    k.close()


# ---- 6. a failed call moves nobody --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))
def test_failed_call_moves_nobody(flavor):
    k = Pair(flavor, 4)
    S, x = k.S, k.x
    x.spdif_block_pos(33); k.ctx_pos = 33
    x.spdif_per_stream(1)
    k.pos[:] = (np.arange(S) * 13 + 2) % 192
    x.spdif_stream_pos(set=k.pos)
    k.call(2, "host", "before the failed calls")
    pcm = np.ascontiguousarray(k.pcm[:, :2 * B])
    with pytest.raises(DspiError) as e: x.process_wire_host(pcm, 2, B, 20)
    assert e.value.code == host.E_INVAL
    wire = np.full((S, x.P, 2 * B, 4), FILL, dtype=np.uint32)
    out = host._Out(wire.ctypes.data, None, None, None)
    import ctypes as C
    for flags in (0x40, 0x10, 0x8, 0x2, 0x80000000):
        assert x.L.dspi_process_wire(x.h, pcm.ctypes.data, 16, 2, B, C.byref(out), None, flags) == host.E_INVAL, hex(flags)
    assert (wire == FILL).all(), "a refused call wrote something"
    k.check_positions("after the failed calls")
    k.call(2, "host", "the next call")
    k.close()
