"""Input from a packet table on the GPU (include/dspi.h: dspi_process_packets).

The call IS dspi_process_mixed on the input that its table describes, so nearly every case is held to a TWIN: a second context with the same
presets that gets the same packets, gathered on the CPU into dspi_process_mixed's contiguous layout, through dspi_process_mixed (with wire
words: dspi_process_devices) on device buffers — every output word, the clip flags and the status bytes are equal.  The programme bus is held
to the chain oracle as well.  The arena is poisoned between and around the packets.

Shapes: 130 float streams (a whole row of 128 and a ragged one), 70 Q28 streams (row 64); 96 kHz, 3 packets per call, mixed 16 / 24 bit depths
where nothing else is said.  No figures: every comparison is for equality."""
import ctypes as C
import struct

import numpy as np
import pytest

import packets_model as M
from conftest import has_gpu
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import DspiError
from test_gpu_snapshot import context, fid, oracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, NB = 96000, 3
FLAVORS = (1, 0)
POISON = 0xA5      # the arena between and around the packets: never read
PREFILL = 0x5A     # device outputs before a call that must not write them


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the call"""
    assert hasattr(host.lib(), "dspi_process_packets"), "libdspi_mi355x has no dspi_process_packets"


def streams_of(flavor): return 130 if int(flavor) else 70


def depths_of(S): return np.random.default_rng(11).choice(np.array([16, 24], dtype=np.uint8), S)


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Source:
    """every stream's packets at its native depth: packet(s, depth, k) = the bytes of packet k of input row s"""

    def __init__(self, rows, Bk, total):
        self.Bk = Bk
        self.p16 = WL.synth_pcm16(rows, Bk * total, FS)
        self.p24 = WL.pcm16_to_pcm24_bytes(self.p16)

    def packet(self, row, depth, k):
        Bk = self.Bk
        if depth == 16: return np.ascontiguousarray(self.p16[row, k * Bk:(k + 1) * Bk]).reshape(-1).view(np.uint8)
        return self.p24[row, k * Bk * 6:(k + 1) * Bk * 6]

    def native(self, row, depth, k0, k1):
        """what the oracle eats: packets [k0, k1) of a row, int16 [frames][2] or packed 24-bit bytes"""
        Bk = self.Bk
        return np.ascontiguousarray(self.p16[row, k0 * Bk:k1 * Bk] if depth == 16 else self.p24[row, k0 * Bk * 6:k1 * Bk * 6])


def contiguous(packets_of, depths, n):
    """dspi_process_mixed's own layout of packets_of(s, k), and the table that describes it"""
    parts, table, at = [], np.zeros((len(depths), n), dtype=np.uint64), 0
    for s in range(len(depths)):
        for k in range(n):
            p = packets_of(s, k)
            table[s, k] = at; at += p.size; parts.append(p)
    return np.concatenate(parts), table


def scattered(packets_of, depths, n, rng, share=False):
    """the same packets at random even offsets, in random order, poison in between, in front and behind.  share: equal packets (one
    programme for many streams) are stored once."""
    S = len(depths)
    order = [(s, k) for s in range(S) for k in range(n)]
    rng.shuffle(order)
    table, chunks, at, seen = np.zeros((S, n), dtype=np.uint64), [], 0, {}
    for s, k in order:
        p = packets_of(s, k)
        key = p.tobytes() if share else None
        if share and key in seen: table[s, k] = seen[key]; continue
        gap = 2 * int(rng.integers(1, 20))
        chunks.append(np.full(gap, POISON, dtype=np.uint8)); at += gap
        table[s, k] = at
        if share: seen[key] = at
        chunks.append(p); at += p.size
    chunks.append(np.full(2 * int(rng.integers(0, 9)), POISON, dtype=np.uint8))
    return np.concatenate(chunks), table


class Outs:
    """device outputs of one call"""

    def __init__(self, d, n, Bk, tiled=False, wire=False, pdm=False, fill=0):
        import torch
        S, F, P, Cn, R = d.n_streams, n * Bk, d.P, d.C, d.tile_streams()
        nt = (S + R - 1) // R
        shape = ((nt, P, F, 4, R) if tiled else (S, P, F, 4)) if wire else ((nt, P * 2, F, R) if tiled else (S, P, F, 2))
        assert fill < 0x80
        mk = lambda shape, dt: torch.full(shape, fill * (0x01010101 if dt == torch.int32 else 0x0101), dtype=dt, device=dev())
        self.pairs, self.sub = mk(shape, torch.int32), mk((nt, F, R) if tiled else (S, F), torch.int32)
        self.peaks, self.clip = mk((S, n, Cn), torch.int16), mk((S,), torch.int16)
        self.words = mk((nt, F, 8, R) if tiled else (S, F, 8), torch.int32) if pdm else None
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(sub_ptr=self.sub.data_ptr(), peaks_ptr=self.peaks.data_ptr(), clip_ptr=self.clip.data_ptr(), words_ptr=self.words.data_ptr() if self.words is not None else 0)

    def fetch(self):
        return [t.cpu().numpy() for t in (self.pairs, self.sub, self.peaks, self.clip)] + ([self.words.cpu().numpy()] if self.words is not None else [])


NAMES = ("pairs", "sub", "peaks", "clip flags", "PDM words")


def run_packets(d, arena, depths, table, n, Bk, tiled=False, wire=False, pdm=False, fill=0):
    a = to_dev(arena)
    o = Outs(d, n, Bk, tiled, wire, pdm, fill)
    d.process_packets_device(a.data_ptr(), arena.size, depths, table, n, Bk, pairs_ptr=o.pairs.data_ptr(), tiled=tiled, wire=wire, **o.ptrs())
    table[:] = 0xDEADBEEF      # the caller may reuse its table when the call returns
    d.sync()
    return o.fetch()


def run_mixed(d, buf, depths, n, Bk, tiled=False, wire=False, pdm=False, fill=0):
    a = to_dev(buf)
    o = Outs(d, n, Bk, tiled, wire, pdm, fill)
    if wire: d.process_devices_device(a.data_ptr(), depths, n, Bk, o.pairs.data_ptr(), tiled=tiled, **o.ptrs())
    else: d.process_mixed_device(a.data_ptr(), depths, n, Bk, pairs_ptr=o.pairs.data_ptr(), tiled=tiled, **o.ptrs())
    d.sync()
    return o.fetch()


def same(got, want, what, d=None, t=None):
    for g, w, name in zip(got, want, NAMES): assert np.array_equal(g, w), f"{what}: {name} differ from the twin's"
    if d is not None:
        for s in range(d.n_streams): assert d.status(s) == t.status(s), f"{what}: stream {s}: status bytes"


def pair(flavor, S=None):
    S = S or streams_of(flavor)
    blob = WL.full_chain_blob(int(flavor))
    return context(flavor, S, FS, blob), context(flavor, S, FS, blob), blob


# ---- 1. the mixed call, by table; 2. arrival order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("contiguous", "arrival"))
@pytest.mark.parametrize("Bk", (45, 96, 192))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_the_mixed_call_by_table(flavor, Bk, order):
    """contiguous: a table that describes dspi_process_mixed's own layout.  arrival: the same packets at random even offsets in random order
    in a poisoned arena, another arena and another table in the second call.  Two calls in a row: state carries.  192 frames: the longest
    packet the call takes, two of the kernel's tiles."""
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src, rng = depths_of(S), Source(S, Bk, 2 * NB), np.random.default_rng(Bk)
    for c in range(2):
        of = lambda s, k: src.packet(s, depths[s], c * NB + k)
        buf, table = contiguous(of, depths, NB)
        want = run_mixed(t, buf, depths, NB, Bk)
        arena = buf
        if order == "arrival": arena, table = scattered(of, depths, NB, rng)
        assert d.packets_check(depths, table, NB, Bk, arena.size) is None
        same(run_packets(d, arena, depths, table, NB, Bk), want, f"{order}, call {c}", d, t)
    d.close(); t.close()


# ---- 3. the programme bus, held to the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_programme_bus(flavor):
    """two programmes in the arena, one 16 bit and one 24 bit, each stored ONCE; streams alternate between them, every third stream on a preset
    of another structure.  The first eight streams are held to their oracles, fed their programme at its native depth; every stream to
    dspi_process_mixed on a twin whose input holds the programmes replicated."""
    Bk = 96
    d, t, blob = pair(flavor)
    S = d.n_streams
    blob_b = WL.full_chain_blob(int(flavor), max_delay_ms=7.0)
    for s in range(0, S, 3):
        for x in (d, t): assert x.load_bulk(blob_b, stream=s) == 0
    depths = np.where(np.arange(S) % 2 == 0, 16, 24).astype(np.uint8)
    src = Source(2, Bk, NB)
    of = lambda s, k: src.packet(s % 2, depths[s], k)
    arena, table = scattered(of, depths, NB, np.random.default_rng(3), share=True)
    assert len(np.unique(table)) == 2 * NB and arena.size < 2 * NB * (Bk * 6 + 40), "the programmes are stored once"
    buf, _ = contiguous(of, depths, NB)
    got = run_packets(d, arena, depths, table, NB, Bk)
    same(got, run_mixed(t, buf, depths, NB, Bk), "programme bus", d, t)
    pairs, sub, peaks, clip = got
    for s in range(8):
        o = oracle(flavor, FS, blob_b if s % 3 == 0 else blob)
        rp, rs, rk, rclip = o.process(src.native(s % 2, int(depths[s]), 0, NB), NB, Bk, int(depths[s]))
        assert np.array_equal(rp, pairs[s]) and np.array_equal(rs, sub[s]), f"stream {s} ({depths[s]} bit): words differ from the oracle's"
        assert np.array_equal(rk, peaks[s].view(np.uint16)) and int(clip[s].view(np.uint16)) == rclip, f"stream {s}: peaks or clip flags differ from the oracle's"
        assert d.status(s) == o.status(), f"stream {s}: status bytes"
    d.close(); t.close()


# ---- 4. concealment by reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_concealment_by_reference(flavor):
    """stream 9's packet 1 did not arrive: its entry names its packet 0 again.  The twin is fed that packet twice."""
    Bk = 45
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src = depths_of(S), Source(S, Bk, NB)
    lost = lambda s, k: src.packet(s, depths[s], 0 if (s, k) == (9, 1) else k)
    arena, table = scattered(lambda s, k: src.packet(s, depths[s], k), depths, NB, np.random.default_rng(4))
    table[9, 1] = table[9, 0]
    buf, _ = contiguous(lost, depths, NB)
    same(run_packets(d, arena, depths, table, NB, Bk), run_mixed(t, buf, depths, NB, Bk), "concealment", d, t)
    d.close(); t.close()


# ---- 5. paused streams -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_paused_streams(flavor, tiled):
    """every third stream is paused and its entries point far beyond the arena: the call succeeds, the paused regions of the device outputs
    stay as they were pre-filled (the twin's too: both are compared whole), the active streams are the twin's"""
    Bk = 45
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src = depths_of(S), Source(S, Bk, NB)
    for s in range(0, S, 3):
        for x in (d, t): x.pause_streams(s, 1)
    of = lambda s, k: src.packet(s, depths[s], k)
    arena, table = scattered(of, depths, NB, np.random.default_rng(5))
    table[0::3] = np.uint64(2 ** 63 + 1)
    buf, _ = contiguous(lambda s, k: np.full(Bk * (6 if depths[s] == 24 else 4), POISON, dtype=np.uint8) if s % 3 == 0 else of(s, k), depths, NB)
    assert d.packets_check(depths, table, NB, Bk, arena.size) is None
    got = run_packets(d, arena, depths, table, NB, Bk, tiled=tiled, fill=PREFILL)
    same(got, run_mixed(t, buf, depths, NB, Bk, tiled=tiled, fill=PREFILL), "paused", d, t)
    pairs, sub, peaks, clip = got
    if not tiled:
        for g in (pairs, sub, peaks): assert (g[0::3].view(np.uint8) == PREFILL).all(), "a paused stream's region was written"
        assert not (pairs[1::3].view(np.uint8) == PREFILL).all()
    d.close(); t.close()


# ---- 6. wire words ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled,pdm", ((False, False), (True, False), (True, True)), ids=("wire", "wire-tiled", "wire-tiled-pdm"))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_wire_words(flavor, tiled, pdm):
    """DSPI_OUT_WIRE, and DSPI_OUT_WIRE | DSPI_OUT_TILED: dspi_process_devices on the contiguous input; on one case with pdm_words"""
    Bk = 96
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src = depths_of(S), Source(S, Bk, 2 * NB)
    rng = np.random.default_rng(6)
    for c in range(2):
        of = lambda s, k: src.packet(s, depths[s], c * NB + k)
        arena, table = scattered(of, depths, NB, rng)
        buf, _ = contiguous(of, depths, NB)
        same(run_packets(d, arena, depths, table, NB, Bk, tiled=tiled, wire=True, pdm=pdm), run_mixed(t, buf, depths, NB, Bk, tiled=tiled, wire=True, pdm=pdm), f"wire, call {c}", d, t)
    d.close(); t.close()


# ---- 7. a long packet --------------------------------------------------------------------------------------------------------------------------------
def test_a_long_packet():
    """block_len 700, n_blocks 1, 3 streams, source residues 2 and 14: a packet of five tiles.  The calls refuse a block_len above 192 as
    dspi_process_mixed does (asserted here), so the kernel is launched by itself (dspi_packetrx_launch_raw, no interface) and its output,
    the packed 24-bit array the chain would read, is held to the model's gather; the bytes behind the array stay as they were."""
    import torch
    Bk, n, S = 700, 1, 3
    assert M.check([24, 16, 24], [[0]] * 3, n, Bk, 1 << 20) == ("lengths",)
    d = context(0, S, FS, WL.full_chain_blob(0))
    with pytest.raises(DspiError) as e: d.packets_check([24, 16, 24], np.zeros((S, n), dtype=np.uint64), n, Bk, 1 << 20)
    assert e.value.code == host.E_INVAL
    d.close()
    L = host.lib()
    L.dspi_packetrx_launch_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    rng = np.random.default_rng(7)
    for depths, entries in (([24, 16, 24], [2, 4366, 7198]), ([16, 24, 16], [14, 2818, 7026])):
        assert [x % 16 for x in entries[:2]] in ([2, 14], [14, 2])
        arena = np.full(7198 + 6 * Bk + 10, POISON, dtype=np.uint8)
        for x, dp in zip(entries, depths): arena[x:x + Bk * M.frame_bytes(dp)] = rng.integers(0, 256, Bk * M.frame_bytes(dp), dtype=np.uint8)
        table = np.array(entries, dtype=np.uint64).reshape(S, n)
        assert M.check(depths, table.tolist(), n, Bk, arena.size, max_block_len=Bk) is None
        t_arena, t_table, t_depths = to_dev(arena), to_dev(table.view(np.int64)), to_dev(np.array(depths, dtype=np.uint8))
        t_dst = torch.full((S * 6 * Bk * n + 64,), PREFILL, dtype=torch.uint8, device=dev())
        torch.cuda.synchronize()
        assert L.dspi_packetrx_launch_raw(t_arena.data_ptr(), t_table.data_ptr(), t_depths.data_ptr(), t_dst.data_ptr(), S, n, Bk) == 0
        got = t_dst.cpu().numpy()
        want = np.concatenate([M.gather(arena, table[s], depths[s], Bk) for s in range(S)])
        assert np.array_equal(got[:-64], want), "the long packets differ from the model's gather"
        assert (got[-64:] == PREFILL).all(), "bytes behind the array were written"


# ---- 8. refusals write nothing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_refusals_write_nothing(flavor):
    """an odd entry, an entry whose packet ends one byte past the arena, a missing DSPI_MEM_DEVICE and (float) the preamp's refusal, between two
    good calls: the pre-filled outputs are untouched, no status byte changes, and the next good call equals the twin that never saw them"""
    Bk = 45
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src = depths_of(S), Source(S, Bk, 2 * NB)
    s16 = int(np.argmax(depths == 16))
    for x in (d, t): assert x.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", 0.0), stream=s16) >= 0
    rng = np.random.default_rng(8)
    for c in range(2):
        of = lambda s, k: src.packet(s, depths[s], c * NB + k)
        arena, table = scattered(of, depths, NB, rng)
        buf, _ = contiguous(of, depths, NB)
        if c == 1:
            a, o = to_dev(arena), Outs(d, NB, Bk, fill=PREFILL)
            before = [d.status(s) for s in range(S)]
            out = host._Out(o.pairs.data_ptr(), o.sub.data_ptr(), o.peaks.data_ptr(), o.clip.data_ptr())
            dp = np.ascontiguousarray(depths)
            call = lambda tab, ab, flags: d.L.dspi_process_packets(d.h, a.data_ptr(), ab, dp.ctypes.data, tab.ctypes.data, NB, Bk, C.byref(out), None, flags)
            err = lambda: d.L.dspi_last_error(d.h).decode()
            flags = host.MEM_DEVICE | host.OUT_CLIP_FLAGS
            odd = table.copy(); odd[S - 1, 2] += 1
            assert call(odd, arena.size, flags) == host.E_INVAL and f"entry {(S - 1) * NB + 2} " in err()
            last = int(np.argmax(table))
            ends = int(table.reshape(-1)[last]) + Bk * M.frame_bytes(int(depths[last // NB]))
            assert d.packets_check(depths, table, NB, Bk, ends) is None
            assert call(table, ends - 1, flags) == host.E_INVAL and f"entry {last} " in err()
            assert call(table, arena.size, host.OUT_CLIP_FLAGS) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
            if int(flavor):
                assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=s16) >= 0
                assert call(table, arena.size, flags) == host.E_UNSUPPORTED and f"stream {s16} " in err()
                assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", 0.0), stream=s16) >= 0
            d.sync()
            for g, name in zip(o.fetch(), NAMES): assert (g.view(np.uint8) == PREFILL).all(), f"a refused call wrote {name}"
            assert [d.status(s) for s in range(S)] == before, "a refused call changed a status byte"
        same(run_packets(d, arena, depths, table, NB, Bk), run_mixed(t, buf, depths, NB, Bk), f"call {c}", d, t)
    d.close(); t.close()
