"""Wire words on tiled and mixed-depth contexts, on the GPU (dspi_process_devices / dspi_wire_encode_tiled, include/dspi.h).  As in
tests/test_gpu_wire.py the expectation is always the oracle's, per stream and pair by the stream's OWN output types — check() there:
orclib.spdif_encode(words[s, p], pos_s, fs_s) for an S/PDIF slot, orclib.i2s_frames(words[s, p]) for an I2S slot, the reference's own
encoders for a few streams where oracle/_ref is built —, placed by host.py untile_wire; `words` are the pair words of a TWIN context that
goes through the same packets without the wire layout.  A third twin makes the stream-major dspi_process_wire call, whose bytes every tiled
call equals after untile_wire.

Shapes: float S = 150 (R = 128: one full tile and 22 columns of a second), Q28 S = 100 (R = 64), 48-frame packets, the five type layouts by
stream % 5 (neighbouring LANES differ), three rates, device buffers pre-filled.  The chunked test alone needs 256 streams x 19 x 96 frames,
the smallest call plan_call cuts in two."""
import ctypes as C
import struct

import numpy as np
import pytest

import orclib
from conftest import has_gpu
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import DspiError
from test_gpu_snapshot import context
from test_gpu_mixed_input import pattern, widen
from test_gpu_wire import B, FILL, FS, check, set_rates, set_types, silent_pairs, size, three_rates, type_table, warm

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

R = W.REQ
FLAVORS = pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=("fma", "q28"))


def mixed_inputs(p16, p24, depths, f0, f1):
    """frames [f0, f1) of every stream at its own depth, back to back (the call's buffer), and the same as packed 24-bit rows [S][F * 6] (the
    twins' input: a 16-bit stream's samples widened on the CPU)"""
    parts, twin = [], np.zeros((len(depths), (f1 - f0) * 6), dtype=np.uint8)
    for s, depth in enumerate(depths):
        if depth == 16:
            r = np.ascontiguousarray(p16[s, f0:f1])
            parts.append(r.reshape(-1).view(np.uint8)); twin[s] = widen(r)
        else:
            r = np.ascontiguousarray(p24[s, f0 * 6:f1 * 6])
            parts.append(r); twin[s] = r
    return np.concatenate(parts), twin


def devices_call(d, buf, depths, n, mem, tiled, Bk=B, enabled_only=False, pdm=False, clip=False):
    """one dspi_process_devices call -> dict(wire, sub, peaks, words); device buffers are pre-filled with FILL.  clip: d.last_clip"""
    if mem == "host":
        r = d.process_devices_host(buf, depths, n, Bk, tiled=tiled, enabled_only=enabled_only, clip=clip, pdm=pdm)
        return dict(wire=r[0], sub=r[1], peaks=r[2], words=r[3] if pdm else None)
    import torch
    dev = torch.device("cuda", 0)
    S, F, Rw = d.n_streams, n * Bk, d.tile_streams()
    nt = (S + Rw - 1) // Rw
    t_pcm = torch.from_numpy(np.ascontiguousarray(buf).view(np.uint8).reshape(-1)).to(dev)
    t_wire = torch.full((nt, d.P, F, 4, Rw) if tiled else (S, d.P, F, 4), FILL, dtype=torch.int32, device=dev)
    t_sub = torch.zeros((nt, F, Rw) if tiled else (S, F), dtype=torch.int32, device=dev)
    t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
    t_words = torch.zeros((nt, F, 8, Rw) if tiled else (S, F, 8), dtype=torch.int32, device=dev) if pdm else None
    t_clip = torch.zeros((S,), dtype=torch.int16, device=dev) if clip else None
    torch.cuda.synchronize()
    d.process_devices_device(t_pcm.data_ptr(), depths, n, Bk, t_wire.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), t_words.data_ptr() if pdm else 0,
                             tiled=tiled, enabled_only=enabled_only, clip_ptr=t_clip.data_ptr() if clip else 0)
    d.sync()
    if clip: d.last_clip = t_clip.cpu().numpy().view(np.uint16)
    return dict(wire=t_wire.cpu().numpy().view(np.uint32), sub=t_sub.cpu().numpy(), peaks=t_peaks.cpu().numpy().view(np.uint16),
                words=t_words.cpu().numpy().view(np.uint32) if pdm else None)


def wire_call(d, pcm, depth, n, mem, Bk=B, enabled_only=False):
    """the third twin's stream-major dspi_process_wire call on the same kind of buffers"""
    if mem == "host": return d.process_wire_host(pcm, n, Bk, depth, enabled_only=enabled_only)[0]
    import torch
    dev = torch.device("cuda", 0)
    S, F = d.n_streams, n * Bk
    t_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    t_wire = torch.full((S, d.P, F, 4), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d.process_wire_device(t_pcm.data_ptr(), n, Bk, t_wire.data_ptr(), depth, enabled_only=enabled_only)
    d.sync()
    return t_wire.cpu().numpy().view(np.uint32)


def absent_columns(wire_t, S):
    """the columns past the last stream, of every region of the last tile"""
    nt, P, F, _, Rw = wire_t.shape
    return wire_t.reshape(nt, P, 4 * F, Rw)[-1, :, :, S % Rw:] if S % Rw else wire_t[:0]


def by_stream(a, S, tiled):
    """a tiled array [tiles][...][R] as [S][...]: the columns of the streams there are"""
    return np.moveaxis(a, -1, 1).reshape((a.shape[0] * a.shape[-1],) + a.shape[1:-1])[:S] if tiled else a


class Trio:
    """x takes dspi_process_devices, t the same packets without a flag (the words the oracle encodes), w dspi_process_wire stream-major; the
    test's own arithmetic of the positions beside them"""

    def __init__(self, flavor, frames, types=None, rates=None, setup=None, S=None, fs=FS, Bk=B):
        self.S, self.B, self.rate = S or size(flavor), Bk, fs
        blob = WL.full_chain_blob(int(flavor))
        self.x, self.t, self.w = (context(flavor, self.S, fs, blob) for _ in range(3))
        self.all = (self.x, self.t, self.w)
        self.types = type_table(self.S, self.x.P) if types is None else types
        self.fs = np.full(self.S, fs) if rates is None else rates
        for d in self.all:
            if setup: setup(d)
            if rates is not None: set_rates(d, self.fs)
            set_types(d, self.types)
            d.process_host(WL.synth_pcm16(self.S, 12 * Bk, fs, first_stream=900), 12, Bk, 16)      # past the power-on and type-switch mutes
        self.p16 = WL.synth_pcm16(self.S, frames, fs)
        self.p24 = WL.pcm16_to_pcm24_bytes(self.p16)
        self.at = 0
        self.pos = np.zeros(self.S, dtype=np.int64)
        self.active = np.ones(self.S, dtype=bool)
        self.ctx_pos = 0

    def pause(self, streams):
        for s in streams:
            for d in self.all: d.pause_streams(int(s), 1)
            self.active[s] = False

    def check_positions(self, what):
        for d in (self.x, self.w):
            if d.spdif_per_stream(): assert np.array_equal(d.spdif_stream_pos(), self.pos), f"{what}: dspi_spdif_stream_pos is not the test's arithmetic"
            assert d.spdif_block_pos() == self.ctx_pos, f"{what}: the context's own value"

    def call(self, n, depths, mem, tiled, what, against_wire=True, **kw):
        """one call of n packets on all three; returns x's outputs (the wire words stream-major, also as they came: `raw`)"""
        F = n * self.B
        depths = np.asarray(depths, dtype=np.uint8)
        uniform = int(depths[0]) if (depths == depths[0]).all() else 0
        buf, twin24 = mixed_inputs(self.p16, self.p24, depths, self.at, self.at + F)
        twin_in, twin_depth = (np.ascontiguousarray(self.p16[:, self.at:self.at + F]), 16) if uniform == 16 else (twin24, 24)
        self.at += F
        pdm, eo = kw.get("pdm", False), kw.get("enabled_only", False)
        ref = self.t.process_pdm_host(twin_in, n, self.B, twin_depth, tiled=tiled, enabled_only=eo) if pdm else self.t.process_host(twin_in, n, self.B, twin_depth, tiled=tiled, enabled_only=eo)
        words = self.t.untile(ref[0], None)[0] if tiled else ref[0]
        assert int(np.abs(words[self.active]).max()) > 0
        got = devices_call(self.x, buf, depths, n, mem, tiled, Bk=self.B, **kw)
        fill = 0 if mem == "host" else FILL
        got["raw"] = got["wire"]
        if tiled:
            assert (absent_columns(got["raw"], self.S) == fill).all(), f"{what}: a column past the last stream was written"
            got["wire"] = self.x.untile_wire(got["raw"], self.types)
        paused = np.flatnonzero(~self.active)
        check(got["wire"], words, self.pos, self.fs, self.types, fill, what, skip=set(paused.tolist()))
        if len(paused): assert (got["wire"][paused] == fill).all(), f"{what}: a paused stream's column was written"
        if against_wire:
            sm = wire_call(self.w, twin_in, twin_depth, n, mem, Bk=self.B, enabled_only=eo)
            assert np.array_equal(got["wire"], sm), f"{what}: not the words of the stream-major dspi_process_wire: streams {sorted(set(np.argwhere(got['wire'] != sm)[:, 0].tolist()))[:8]}"
        # (tiled sub and PDM words: the columns past the last stream are nobody's, in this call as in dspi_process_pdm)
        assert np.array_equal(by_stream(got["sub"], self.S, tiled), by_stream(ref[1], self.S, tiled)), f"{what}: sub words differ from the twin's"
        assert np.array_equal(got["peaks"], ref[2]), f"{what}: peaks differ from the twin's"
        if pdm: assert ref[3].any() and np.array_equal(by_stream(got["words"], self.S, tiled), by_stream(ref[3], self.S, tiled)), f"{what}: the PDM words differ from dspi_process_pdm's"
        self.pos[self.active] = (self.pos[self.active] + F) % 192
        self.ctx_pos = (self.ctx_pos + F) % 192
        if against_wire: self.check_positions(what)
        return got

    def close(self):
        for d in self.all: d.close()


# ---- 1. dspi_wire_encode_tiled ------------------------------------------------------------------------------------------------------------
@FLAVORS
def test_wire_encode_tiled(flavor):
    """144 frames and 45 (both cross a 32-frame slice, even and odd), positions 0, 191, 100 and 148 among random ones, three rates, neighbouring
    lanes of different type, two streams paused (the call does not know); host buffers: tails and the columns past S zero; device buffers pre-filled: the fill survives there, positions
    are taken modulo 192; no I2S slot anywhere: every column below S is dspi_spdif_encode_v(TILED) word for word; the refusals"""
    import torch
    S, F = size(flavor), 144
    blob = WL.full_chain_blob(int(flavor))
    d, plain = context(flavor, S, FS, blob), context(flavor, S, FS, blob)
    Rw = d.tile_streams(); nt = -(-S // Rw)
    rates, types = three_rates(S), type_table(S, d.P)
    assert S % Rw and all(types[s].tolist() != types[s + 1].tolist() for s in range(S - 1))
    for c in (d, plain): set_rates(c, rates)
    set_types(d, types)
    tiled = warm(d).process_host(WL.synth_pcm16(S, F, FS), 3, B, 16, tiled=True)[0]
    odd_t = np.ascontiguousarray(tiled[:, :, :45])
    words, odd = d.untile(tiled, None)[0], d.untile(odd_t, None)[0]
    assert int(np.abs(odd).max()) > 0
    pos = np.random.default_rng(7).integers(0, 192, S).astype(np.uint32)
    pos[[0, 1, 2, 3, S - 1]] = (0, 191, 100, 148, 191)
    d.pause_streams(7, 2)      # the stateless call is unaware of pauses: columns 7 and 8 are encoded like the rest
    for wt, w, what in ((tiled, words, "host, 144 frames"), (odd_t, odd, "host, 45 frames")):
        got = d.wire_encode_tiled_host(wt, pos)
        assert not absent_columns(got, S).any(), f"{what}: columns past S"
        check(d.untile_wire(got, types), w, pos, rates, types, 0, what)
    dev = torch.device("cuda", 0)
    big = (pos + 192 * np.linspace(0, 22369619, S).astype(np.uint64)).astype(np.uint32)
    assert big.max() > 2 ** 31 and np.array_equal(big % 192, pos)
    t_pos = torch.from_numpy(big.view(np.int32)).to(dev)
    for wt, w, what in ((tiled, words, "device, 144 frames"), (odd_t, odd, "device, 45 frames")):
        t_in = torch.from_numpy(wt).to(dev)
        t_out = torch.full((nt, d.P, wt.shape[2], 4, Rw), FILL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.wire_encode_tiled_device(t_in.data_ptr(), wt.shape[2], t_pos.data_ptr(), t_out.data_ptr())
        d.sync()
        got = t_out.cpu().numpy().view(np.uint32)
        assert (absent_columns(got, S) == FILL).all(), f"{what}: the fill past S"
        check(d.untile_wire(got, types), w, pos, rates, types, FILL, what)
    # no I2S slot anywhere: dspi_spdif_encode_v(TILED), word for word, in every column below S
    for wt in (tiled, odd_t):
        a, b = plain.wire_encode_tiled_host(wt, pos), plain.spdif_encode_v_host(wt, pos, tiled=True)
        assert a.shape == b.shape and np.array_equal(a[:-1], b[:-1]) and np.array_equal(a[-1][..., :S % Rw], b[-1][..., :S % Rw]), wt.shape
    # refusals: a host position of 192, every flag but DSPI_MEM_DEVICE, a null list
    bad = pos.copy(); bad[S // 2] = 192
    with pytest.raises(DspiError) as e: d.wire_encode_tiled_host(tiled, bad)
    assert e.value.code == host.E_INVAL
    out = np.zeros((nt, d.P, F, 4, Rw), dtype=np.uint32)
    for flags in (0x2, 0x4, 0x8, 0x10, 0x20, 0x100, 0x80000000):
        assert d.L.dspi_wire_encode_tiled(d.h, tiled.ctypes.data, F, pos.ctypes.data, out.ctypes.data, flags) == host.E_INVAL, hex(flags)
    assert d.L.dspi_wire_encode_tiled(d.h, tiled.ctypes.data, F, None, out.ctypes.data, 0) == host.E_INVAL
    assert not out.any()
    d.close(); plain.close()


# ---- 2. dspi_process_devices, tiled -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,layout", [(W.F32_FMA, "packed"), (W.F32_FMA, "skew"), (0, "packed")], ids=("fma-packed", "fma-latency-layout", "q28"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_process_devices_tiled(flavor, layout, mem, monkeypatch):
    """uniform 16-bit depths: two calls with the context's one position, then per-stream positions on and distinct, two calls with streams
    paused in between: their columns hold fill or zero, their positions freeze; every call is the third twin's dspi_process_wire re-laid"""
    monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    n = 2
    k = Trio(flavor, 5 * n * B, rates=three_rates(size(flavor)))
    S, x = k.S, k.x
    u16 = np.full(S, 16, dtype=np.uint8)
    for d in (k.x, k.w): assert d.spdif_block_pos(50) == 50
    k.ctx_pos = 50; k.pos[:] = 50
    for c in range(2): k.call(n, u16, mem, True, f"one position, call {c}")
    plan = x.launch_plan()
    assert (plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0) if layout == "skew" else plan["latency_layout"] == 0, plan
    for d in (k.x, k.w): assert d.spdif_per_stream(1) is True
    k.pos[:] = (np.arange(S) * 7 + 191) % 192      # distinct, with 191 (stream 0) and 0 (stream 55) among them
    assert len(set(k.pos.tolist())) == S and {0, 191} <= set(k.pos.tolist())
    for d in (k.x, k.w): assert np.array_equal(d.spdif_stream_pos(set=k.pos), k.pos)
    k.call(n, u16, mem, True, "per-stream positions")
    paused = [6, 71, S - 2]      # an all-I2S column, one between lanes of other types, one in the last, partial tile
    assert k.types[71].all() and not k.types[70].any()
    k.pause(paused)
    frozen = k.pos[paused].copy()
    for c in range(2): k.call(n, u16, mem, True, f"per-stream positions, three streams paused, call {c}")
    assert np.array_equal(k.pos[paused], frozen) and np.array_equal(x.spdif_stream_pos()[paused], frozen)
    k.close()


# ---- 3. mixed depths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("alternating", "random"))
@FLAVORS
def test_mixed_depths(flavor, name):
    """16- and 24-bit streams in one call, stream-major and tiled, host and device buffers, against the oracle and against dspi_process_wire
    on input widened beforehand; then all depths equal: the call IS dspi_process_wire at that depth, byte for byte"""
    n = 2
    k = Trio(flavor, 6 * n * B, rates=three_rates(size(flavor)))
    depths = pattern(name, k.S).astype(np.uint8)
    assert {16, 24} == set(depths.tolist())
    k.call(n, depths, "host", False, f"{name}, stream-major, host")
    k.call(n, depths, "device", True, f"{name}, tiled, device")
    k.call(n, depths, "host", True, f"{name}, tiled, host")
    k.call(n, depths, "device", False, f"{name}, stream-major, device")
    k.call(n, np.full(k.S, 24, dtype=np.uint8), "device", False, "every depth 24, stream-major: dspi_process_wire at 24 bit")
    k.call(n, np.full(k.S, 16, dtype=np.uint8), "host", False, "every depth 16, stream-major: dspi_process_wire at 16 bit")
    k.close()


def test_no_i2s_slot_is_process_mixed_spdif(monkeypatch):
    """stream-major and no active stream with an I2S slot: the bytes AND the route of dspi_process_mixed with DSPI_OUT_SPDIF — on the latency
    layout with DSPI_OUT_ENABLED_ONLY on device buffers the fused encoder leaves the silent pairs unwritten (tests/test_gpu_wire.py
    test_shortcut); the same call tiled takes two passes and writes them: silence in its own format"""
    import torch
    monkeypatch.setenv("DSPI_F32_LAYOUT", "skew")
    flavor, n = W.F32_FMA, 2
    S, F = size(flavor), n * B
    k = Trio(flavor, 3 * F, types=np.zeros((S, 4), dtype=bool), setup=lambda d: silent_pairs(d, flavor))
    x, m = k.x, k.w      # (the third context makes the dspi_process_mixed calls here)
    depths = pattern("alternating", S).astype(np.uint8)
    dev = torch.device("cuda", 0)
    for c, (mem, eo) in enumerate((("host", False), ("device", True))):
        buf, twin = mixed_inputs(k.p16, k.p24, depths, c * F, (c + 1) * F)
        a = devices_call(x, buf, depths, n, mem, False, enabled_only=eo)["wire"]
        if mem == "host": b = m.process_mixed_host(buf, depths, n, B, spdif=True, enabled_only=eo)[0]
        else:
            t_pcm = torch.from_numpy(buf).to(dev); t_pairs = torch.full((S, 4, F, 4), FILL, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            m.process_mixed_device(t_pcm.data_ptr(), depths, n, B, pairs_ptr=t_pairs.data_ptr(), spdif=True, enabled_only=eo)
            m.sync()
            b = t_pairs.cpu().numpy().view(np.uint32)
        assert np.array_equal(a, b), f"{mem}: not the bytes of dspi_process_mixed(DSPI_OUT_SPDIF)"
        assert x.spdif_block_pos() == m.spdif_block_pos() == ((c + 1) * F) % 192
        if eo: assert (a[:, 1:] == FILL).all() and (a[:, 0] != FILL).any(), "the fused encoder leaves silent pairs unwritten: the call did not take dspi_process_mixed's route"
    plan = x.launch_plan()
    assert plan["latency_layout"] + plan["latency_layout_paired"] > 0 and plan["packed_shared"] == 0, plan
    # tiled: two passes whatever the types — the silent pairs carry the subframes of silence at the context's position
    pos = x.spdif_block_pos()
    buf, _ = mixed_inputs(k.p16, k.p24, depths, 2 * F, 3 * F)
    wire = x.untile_wire(devices_call(x, buf, depths, n, "device", True, enabled_only=True)["wire"], k.types)
    silence = orclib.spdif_encode(np.zeros((F, 2), dtype=np.int32), pos, FS)[0]
    assert np.array_equal(wire[3, 1], silence) and np.array_equal(wire[S - 1, 3], silence) and (wire[:, 0] != FILL).all()
    k.close()


# ---- 4. tiled + mixed + pdm_words + DSPI_OUT_ENABLED_ONLY + DSPI_OUT_CLIP_FLAGS -----------------------------------------------------------
@FLAVORS
@pytest.mark.parametrize("mem", ("host", "device"))
def test_everything_at_once(flavor, mem):
    """the sub on and every pair but pair 0 silent: PDM words, sub and peaks are dspi_process_pdm's on the twin (Trio.call), a silent S/PDIF
    pair carries the subframes of silence at the stream's position and a silent I2S pair zero words, the clip flags are the twin's"""
    n = 3
    k = Trio(flavor, 2 * n * B, setup=lambda d: silent_pairs(d, flavor))
    S, P = k.S, k.x.P
    depths = pattern("alternating", S).astype(np.uint8)
    k.x.spdif_per_stream(1)
    k.pos[:] = (np.arange(S) * 11 + 5) % 192
    k.x.spdif_stream_pos(set=k.pos)
    pos0 = k.pos.copy()
    got = k.call(n, depths, mem, True, "everything at once", against_wire=False, pdm=True, enabled_only=True, clip=True)
    clip_x = k.x.last_clip.copy()
    s_spdif, s_i2s = 5, 6      # layouts 0 (all S/PDIF) and 1 (all I2S)
    assert not k.types[s_spdif].any() and k.types[s_i2s].all()
    silence = orclib.spdif_encode(np.zeros((n * B, 2), dtype=np.int32), int(pos0[s_spdif]), FS)[0]
    assert np.array_equal(got["wire"][s_spdif, P - 1], silence), "a silent S/PDIF pair: the subframes of silence at the stream's position"
    assert not got["wire"][s_i2s, P - 1].reshape(-1)[:2 * n * B].any(), "a silent I2S pair: zero words"
    # the clip flags are sticky: the twin reports, with its next call, those of both calls; so does x
    buf, twin = mixed_inputs(k.p16, k.p24, depths, k.at, k.at + n * B)
    k.t.process_host(twin, n, B, 24, tiled=True, clip=True)
    devices_call(k.x, buf, depths, n, mem, True, clip=True)
    assert np.array_equal(k.x.last_clip, k.t.last_clip), "DSPI_OUT_CLIP_FLAGS differs from the twin's"
    assert not (clip_x & ~k.x.last_clip).any(), "a sticky clip flag of the first call is gone"
    k.close()


# ---- 5. the host-buffer paths -------------------------------------------------------------------------------------------------------------
def test_staged_chunks():
    """the smallest tiled call plan_call cuts in chunks (moved >= 32 MiB: input, regions, sub words and peaks; 256 float streams, 96-frame
    packets): the tiled encoder runs per chunk with a first tile above 0 — types, rates, positions are indexed by ABSOLUTE stream"""
    flavor, S, fs, Bk = W.F32_FMA, 256, 96000, 96
    depths = pattern("alternating", S).astype(np.uint8)
    moved = lambda n: S * n * Bk * (6 + 4 * 16 + 4) + S * n * 11 * 2      # (a mixed call is planned as the 24-bit call it becomes: 6 bytes per input frame)
    n = next(n for n in range(1, 100) if moved(n) >= 32 << 20)
    assert moved(n - 1) < 32 << 20 and n == 19
    types = type_table(S, 4, only={0: 2, 127: 1, 128: 4, 255: 3})
    k = Trio(flavor, n * Bk, types=types, S=S, fs=fs, Bk=Bk)
    assert k.x.tile_streams() == 128
    k.x.spdif_per_stream(1)
    pos = (np.arange(S) * 5 + 1) % 192
    k.x.spdif_stream_pos(set=pos)
    buf, twin = mixed_inputs(k.p16, k.p24, depths, 0, n * Bk)
    words = k.t.process_host(twin, n, Bk, 24)[0]
    assert int(np.abs(words[[0, 127, 128, 255]]).max()) > 0
    got = k.x.process_devices_host(buf, depths, n, Bk, tiled=True)[0]
    assert k.x.direct_stats()["calls"] == 0
    check(k.x.untile_wire(got, types), words, pos, fs, types, 0, "two chunks", streams=(0, 1, 126, 127, 128, 129, 254, 255))
    assert np.array_equal(k.x.spdif_stream_pos(), (pos + n * Bk) % 192)
    k.close()


@pytest.mark.parametrize("path", ("direct", "staged"))
@FLAVORS
def test_direct_and_staged_small(flavor, path, monkeypatch):
    """host buffers small enough for the direct area, and the same through the staged path (DSPI_NO_DIRECT=1), whose staging buffer comes
    back whole: tails, paused columns and the columns past S are zeros on both"""
    if path == "staged": monkeypatch.setenv("DSPI_NO_DIRECT", "1")
    k = Trio(flavor, 4 * B)
    depths = pattern("alternating", k.S).astype(np.uint8)
    k.call(2, depths, "host", True, f"{path}, first call")
    k.pause([70, k.S - 1])
    k.call(2, depths, "host", True, f"{path}, second call, two streams paused")
    assert (k.x.direct_stats()["calls"] > 0) == (path == "direct"), "the call did not take the path this case is about"
    k.close()


# ---- 6. a failed call moves nobody --------------------------------------------------------------------------------------------------------
@FLAVORS
def test_failed_call_moves_nobody(flavor):
    """a bad depth in the middle of the vector, a refused flag, (float) the preamp refusal of a 16-bit stream: nothing is written, no position
    moves, and the next call continues where the last good one ended"""
    k = Trio(flavor, 4 * B)
    S, x = k.S, k.x
    depths = pattern("alternating", S).astype(np.uint8)
    for d in (k.x, k.w): d.spdif_block_pos(33); d.spdif_per_stream(1)
    k.ctx_pos = 33
    k.pos[:] = (np.arange(S) * 13 + 2) % 192
    for d in (k.x, k.w): d.spdif_stream_pos(set=k.pos)
    k.call(2, depths, "host", True, "before the failed calls")
    buf, _ = mixed_inputs(k.p16, k.p24, depths, k.at, k.at + 2 * B)
    Rw = x.tile_streams(); nt = -(-S // Rw)
    wire = np.full((nt, x.P, 2 * B, 4, Rw), FILL, dtype=np.uint32)
    out = host._Out(wire.ctypes.data, None, None, None)
    raw = lambda dp, flags: x.L.dspi_process_devices(x.h, buf.ctypes.data, dp.ctypes.data, 2, B, C.byref(out), None, flags)
    bad = depths.copy(); bad[S // 2] = 20
    for flags in (0x2, 0x0): assert raw(bad, flags) == host.E_INVAL and f"stream {S // 2}" in x.L.dspi_last_error(x.h).decode()
    for flags in (0x40, 0x10, 0x12, 0x8, 0x80000000): assert raw(depths, flags) == host.E_INVAL, hex(flags)
    if int(flavor):
        assert depths[8] == 16
        x.vendor_set(R["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=8)
        for flags in (0x2, 0x0): assert raw(depths, flags) == host.E_UNSUPPORTED and "stream 8" in x.L.dspi_last_error(x.h).decode()
        for d in k.all: d.vendor_set(R["SET_PREAMP_CH"], 0, struct.pack("<f", -3.0), stream=8)      # (all three: the next call compares them)
    assert (wire == FILL).all(), "a refused call wrote something"
    k.check_positions("after the failed calls")
    k.call(2, depths, "host", True, "the next call")
    k.close()
