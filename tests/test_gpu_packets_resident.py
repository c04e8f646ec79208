"""Resident packet tables on the GPU (include/dspi.h: dspi_process_packets_resident, dspi_packets_emit_resident and the two check calls): the
table lies in device memory and its entries are checked there.

The checker's answer is held to the host-table checks (dspi_packets_check, dspi_packets_emit_check) on the same arrays — by itself through the
raw launcher, where a workgroup cap of 1 or 2 makes the grid-stride loop go round at small sizes and an odd count has a tail, and through the
two check calls, code, message and *bad_entry.  The two audio calls are held to the host-table calls on a TWIN context that gets the same
arrays from host memory: every output byte is equal.

NO TEST HERE HANDS AN ILLEGAL TABLE TO DSPI_TABLE_CHECKED: illegal tables go to the default route, the check calls and the raw checker only
(the raw checker reads nothing but the table).

Shapes: 130 float streams, 70 Q28 streams; 96 kHz, 3 packets of 45 or 96 frames.  No figures: every comparison is for equality."""
import ctypes as C
import random

import numpy as np
import pytest

import packets_model as MI
import packets_out_model as MO
from conftest import has_gpu
from dspi_amd import host, workloads as WL
from dspi_amd.host import Dspi
from test_gpu_packets import NAMES, PREFILL, Outs, Source, contiguous, depths_of, pair, run_mixed, run_packets, same, scattered
from test_gpu_packets_out import buffers, fleet, warm
from test_gpu_snapshot import context, fid, oracle
from test_packets_out_cpu import ILLEGAL, arena_bytes, make_table

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, NB = 96000, 3
FLAVORS = (1, 0)
CAPS = (1, 2, 3, 0)
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the calls"""
    assert hasattr(host.lib(), "dspi_process_packets_resident"), "libdspi_mi355x has no dspi_process_packets_resident"


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    """a device copy that has landed; a uint64 table travels as int64"""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev())
    torch.cuda.synchronize()
    return t


def err(d): return d.L.dspi_last_error(d.h).decode()


# ---- 1. the raw checker --------------------------------------------------------------------------------------------------------------------------
def raw_check(kind, t_table, t_kinds, t_active, entries, per, bl, ab, cap, t_word):
    ans = C.c_uint64(12345)
    rc = host.lib().dspi_tablecheck_launch_raw(kind, t_table.data_ptr(), t_kinds.data_ptr(), t_active.data_ptr() if t_active is not None else None, entries, per, bl, ab, cap,
                                               t_word.data_ptr(), C.byref(ans))
    assert rc == 0, rc
    return ans.value


# (kind, flavor, streams, packets per row of the HOST check): entries = streams * pairs * packets.  1, 2, 3, 511, 512, 513, 1025 entries, 1560
# (several rounds of the loop at caps 1 and 2), an odd count of 599 979 (two rounds at the default cap, and a tail); emit tables of 1560 and 420
RAW = ((0, 0, 1, 1), (0, 0, 1, 2), (0, 0, 3, 1), (0, 0, 7, 73), (0, 0, 8, 64), (0, 0, 27, 19), (0, 0, 25, 41), (0, 1, 130, 12), (0, 0, 129, 4651), (1, 1, 130, 3), (1, 0, 70, 3))


@pytest.mark.parametrize("kind,flavor,n,nb", RAW, ids=lambda v: str(v))
def test_raw_checker(kind, flavor, n, nb):
    """device tables with no, one (first, last, around 512) and several illegal entries, SKIP words, and a paused first stream whose row is
    illegal: at every cap the word equals *bad_entry of the host check on a host-only context with the same pauses, or is all ones"""
    h = Dspi(flavor, n, device=None)
    per = (h.P if kind else 1) * nb
    E, bl = n * per, 45
    assert E in (1, 2, 3, 511, 512, 513, 1025, 1560, 599979, 420)
    rng = np.random.default_rng(E + kind)
    kinds = rng.choice(np.array([24, 32] if kind else [16, 24], dtype=np.uint8), n)
    size = np.repeat(np.where(kinds == 24, 6, 8 if kind else 4) * bl, per)
    legal = (np.arange(E, dtype=np.uint64) * 1600)
    ab = 1600 * E
    if kind: legal[rng.random(E) < 0.1] = MO.SKIP

    def host_answer(tab):
        bad = C.c_uint64(NONE)
        if kind: rc = h.L.dspi_packets_emit_check(h.h, kinds.ctypes.data, tab.ctypes.data, nb, bl, ab, 0, C.byref(bad))
        else: rc = h.L.dspi_packets_check(h.h, kinds.ctypes.data, tab.ctypes.data, nb, bl, ab, C.byref(bad))
        assert (rc == 0) == (bad.value == NONE) and rc in (0, host.E_INVAL)
        return bad.value
    spots = sorted({0, E - 1, E // 2} | {i for i in (511, 512, 513) if i < E})
    variants = [("legal", [], [])] + [(f"one at {i}", [i], []) for i in spots]
    variants.append(("several", [int(x) for x in rng.integers(0, E, 5)], []))
    variants.append(("ends two bytes past the arena", [E - 1], []))
    if not kind: variants.append(("a SKIP word in an input table", [E // 3], []))
    if n > 1: variants += [("a paused row", list(range(per)), [0]), ("a paused row and one more", list(range(per)) + [E - 2], [0])]
    t_kinds, t_word = to_dev(kinds), to_dev(np.zeros(1, dtype=np.uint64))
    refused = 0
    for name, where, paused in variants:
        tab = legal.copy()
        for i in where:
            if name.startswith("ends"): tab[i] = ab - int(size[i]) + 2
            elif name.startswith("a SKIP"): tab[i] = MO.SKIP
            elif paused and i < per: tab[i] = 2 ** 63 + 1                                      # the paused row: anything
            else: tab[i] = (0 if legal[i] == MO.SKIP else int(legal[i])) + 1                    # odd
        for s in paused: h.pause_streams(s, 1)
        want = host_answer(tab)
        if name == "legal" or name == "a paused row": assert want == NONE, name
        else: assert want == min(i for i in where if not (paused and i < per)), (name, want)
        bits = None
        if paused:
            bits = np.full((n + 31) // 32, 0xffffffff, dtype=np.uint32)
            for s in paused: bits[s >> 5] &= ~np.uint32(1 << (s & 31))
        t_tab, t_bits = to_dev(tab), to_dev(bits.view(np.int32)) if bits is not None else None
        for cap in CAPS:
            assert raw_check(kind, t_tab, t_kinds, t_bits, E, per, bl, ab, cap, t_word) == want, (name, cap)
        for s in paused: h.resume_streams(s, 1)
        refused += want != NONE
    assert refused >= 4
    h.close()


# ---- 2. the check calls --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_check_calls(flavor):
    """random fleets with 0, 1 and several illegal entries and paused streams whose rows hold ILLEGAL: the return code, the message (the call's
    name apart), *bad_entry, and '*bad_entry is not written on success' equal the host-table check's on the same arrays"""
    Bk = 45
    d = context(flavor, 130 if int(flavor) else 70, FS, WL.full_chain_blob(int(flavor)))
    S, P = d.n_streams, d.P
    r = random.Random(7 + int(flavor))
    paused = sorted(r.sample(range(S), 5)) + [S - 1]
    for s in paused: d.pause_streams(s, 1)
    # the emit kind
    formats = [r.choice((24, 32)) for _ in range(S)]
    etab, eab = make_table(r, formats, P, NB, Bk, set(paused))
    formats = np.array(formats, dtype=np.uint8)
    etab = np.array(etab, dtype=np.uint64)
    assert (etab[paused[0]] == ILLEGAL).all()
    # the input kind
    depths, src = depths_of(S), Source(S, Bk, NB)
    arena, itab = scattered(lambda s, k: src.packet(s, depths[s], k), depths, NB, np.random.default_rng(3))
    itab[paused] = np.uint64(ILLEGAL)
    live = [s for s in range(S) if s not in paused]
    seen = set()
    for kind, kinds, tab, ab, per in ((0, depths, itab, arena.size, NB), (1, formats, etab, eab, P * NB)):
        for n_bad in (0, 1, 1, 4, 9):
            t = tab.copy()
            for _ in range(n_bad):
                s, i = r.choice(live), r.randrange(per)
                t[s, i] = r.choice((int(t[s, i]) + 1 if t[s, i] != MO.SKIP else 1, 2 ** 63, ab - 2, 2 ** 64 - 2))
            dt = to_dev(t)
            hb, rb = C.c_uint64(12345), C.c_uint64(12345)
            if kind:
                hrc = d.L.dspi_packets_emit_check(d.h, kinds.ctypes.data, t.ctypes.data, NB, Bk, ab, 0, C.byref(hb)); htext = err(d)
                rrc = d.L.dspi_packets_emit_check_resident(d.h, kinds.ctypes.data, dt.data_ptr(), NB, Bk, ab, 0, C.byref(rb)); rtext = err(d)
            else:
                hrc = d.L.dspi_packets_check(d.h, kinds.ctypes.data, t.ctypes.data, NB, Bk, ab, C.byref(hb)); htext = err(d)
                rrc = d.L.dspi_packets_check_resident(d.h, kinds.ctypes.data, dt.data_ptr(), NB, Bk, ab, C.byref(rb)); rtext = err(d)
            assert (hrc == 0) == (n_bad == 0) and hrc in (0, host.E_INVAL)
            assert rrc == hrc and rb.value == hb.value, (kind, n_bad, rrc, hrc, rb.value, hb.value)
            if hrc: assert rtext.replace("_check_resident", "_check") == htext and f"entry {hb.value} " in rtext, (rtext, htext)
            else: assert rb.value == 12345
            seen.add((kind, hrc != 0))
            # the wrapper
            if kind == 0 and n_bad == 4:
                with pytest.raises(host.DspiError) as e: d.packets_check_resident(depths, dt.data_ptr(), NB, Bk, ab)
                assert e.value.code == host.E_INVAL and d.bad_entry == hb.value
    assert len(seen) == 4
    assert d.packets_check_resident(depths, to_dev(itab).data_ptr(), NB, Bk, arena.size) is None and d.bad_entry is None
    assert d.packets_emit_check_resident(formats, to_dev(etab).data_ptr(), NB, Bk, eab) is None and d.bad_entry is None
    d.close()


# ---- 3. dspi_process_packets_resident against dspi_process_packets on a twin ---------------------------------------------------------------
def run_resident(d, arena, depths, table, n, Bk, tiled=False, wire=False, pdm=False, fill=0, checked=False):
    a, tab = to_dev(arena), to_dev(table)
    o = Outs(d, n, Bk, tiled, wire, pdm, fill)
    d.process_packets_resident_device(a.data_ptr(), arena.size, depths, tab.data_ptr(), n, Bk, pairs_ptr=o.pairs.data_ptr(), tiled=tiled, wire=wire, checked=checked, **o.ptrs())
    d.sync()
    return o.fetch()


@pytest.mark.parametrize("Bk", (45, 96))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_process_equals_the_host_table_call(flavor, Bk):
    """mixed 16 / 24 bit depths, packets at random even offsets in random order in a poisoned arena; two calls in a row, the second with the
    caller's warrant after dspi_packets_check_resident accepted its table: pairs, sub, peaks, clip flags, PDM words and the status bytes
    equal the twin's, which took the same table from host memory"""
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src, rng = depths_of(S), Source(S, Bk, 2 * NB), np.random.default_rng(Bk)
    for c in range(2):
        arena, table = scattered(lambda s, k: src.packet(s, depths[s], c * NB + k), depths, NB, rng)
        want = run_packets(t, arena, depths, table.copy(), NB, Bk, pdm=True)
        if c: assert d.packets_check_resident(depths, to_dev(table).data_ptr(), NB, Bk, arena.size) is None
        same(run_resident(d, arena, depths, table, NB, Bk, pdm=True, checked=bool(c)), want, f"call {c}", d, t)
    d.close(); t.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_equal_and_overlapping_entries_and_the_oracle(flavor):
    """two programmes stored once (every stream's entries name the same packets) and, for stream 9, a sliding window (its packets overlap
    each other by half): the twin's bytes, and for the first six streams the chain oracle's, fed the programme at its native depth"""
    Bk = 96
    d, t, blob = pair(flavor)
    S = d.n_streams
    depths = np.where(np.arange(S) % 2 == 0, 16, 24).astype(np.uint8)
    src = Source(2, Bk, NB)
    arena, table = scattered(lambda s, k: src.packet(s % 2, depths[s], k), depths, NB, np.random.default_rng(3), share=True)
    assert len(np.unique(table)) == 2 * NB
    first = int(table[9].min())
    table[9] = [first, first + 3 * Bk, first + 6 * Bk]      # (24 bit: half a packet each, inside the programme's bytes or the poison behind them)
    assert depths[9] == 24 and int(table[9, 2]) + 6 * Bk <= arena.size
    got = run_resident(d, arena, depths, table, NB, Bk)
    same(got, run_packets(t, arena, depths, table.copy(), NB, Bk), "programme bus", d, t)
    pairs, sub, peaks, clip = got
    for s in range(6):
        rp, rs, rk, rclip = oracle(flavor, FS, blob).process(src.native(s % 2, int(depths[s]), 0, NB), NB, Bk, int(depths[s]))
        assert np.array_equal(rp, pairs[s]) and np.array_equal(rs, sub[s]), f"stream {s} ({depths[s]} bit): words differ from the oracle's"
        assert np.array_equal(rk, peaks[s].view(np.uint16)) and int(clip[s].view(np.uint16)) == rclip, f"stream {s}: peaks or clip flags differ from the oracle's"
    d.close(); t.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_wire_tiled(flavor):
    """DSPI_OUT_WIRE | DSPI_OUT_TILED with pdm_words, as the host-table call"""
    Bk = 96
    d, t, _ = pair(flavor)
    depths, src = depths_of(d.n_streams), Source(d.n_streams, Bk, NB)
    arena, table = scattered(lambda s, k: src.packet(s, depths[s], k), depths, NB, np.random.default_rng(6))
    want = run_packets(t, arena, depths, table.copy(), NB, Bk, tiled=True, wire=True, pdm=True)
    same(run_resident(d, arena, depths, table, NB, Bk, tiled=True, wire=True, pdm=True), want, "wire tiled", d, t)
    d.close(); t.close()


# ---- 4. dspi_packets_emit_resident against dspi_packets_emit -------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_emit_equals_the_host_table_call(flavor, tiled):
    """mixed formats, a shuffled table with SKIP entries, paused streams whose rows hold ILLEGAL: behind dspi_process with nothing waiting in
    between, the whole pattern-filled arena equals the one dspi_packets_emit leaves on a twin, and the model's"""
    Bk = 45
    S = 130 if int(flavor) else 70
    paused = sorted(set(range(0, S, 7)) | {S - 1})
    d, formats, table, ab, pcm = fleet(flavor, Bk, 61, paused)
    t = warm(context(flavor, S, FS, WL.full_chain_blob(int(flavor))))
    for s in paused:
        for x in (d, t): x.pause_streams(s, 1)
    pattern, tab = arena_bytes(61, ab), np.array(table, dtype=np.uint64)
    assert (tab[0] == ILLEGAL).all() and (tab == MO.SKIP).any()
    arenas = []
    for x, resident in ((d, True), (t, False)):
        p, pairs, arena = buffers(x, pcm, Bk, tiled, pattern)
        dt = to_dev(tab)
        x.process_device(p.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr(), tiled=tiled)
        if resident: x.packets_emit_resident_device(pairs.data_ptr(), NB, Bk, formats, dt.data_ptr(), arena.data_ptr(), ab, tiled=tiled)
        else: x.packets_emit_device(pairs.data_ptr(), NB, Bk, formats, tab.copy(), arena.data_ptr(), ab, tiled=tiled)
        x.sync()
        arenas.append(arena.cpu().numpy())
        words = pairs.cpu().numpy()
    active = [0 if s in paused else 1 for s in range(S)]
    assert np.array_equal(arenas[0], arenas[1]) and not np.array_equal(arenas[0], pattern)
    assert np.array_equal(arenas[0], MO.emit(pattern, words, formats, table, d.P, NB, Bk, d.tile_streams() if tiled else 0, active))
    d.close(); t.close()


# ---- 5. reuse ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_reuse_process(flavor):
    """one device table, one arena, three calls: the first by the default route, the second and third with DSPI_TABLE_CHECKED and no dspi_sync
    between them; the outputs equal three host-table calls on the twin"""
    Bk = 96
    d, t, _ = pair(flavor)
    depths, src = depths_of(d.n_streams), Source(d.n_streams, Bk, NB)
    arena, table = scattered(lambda s, k: src.packet(s, depths[s], k), depths, NB, np.random.default_rng(9))
    a, tab = to_dev(arena), to_dev(table)
    outs = [Outs(d, NB, Bk) for _ in range(3)]
    for c, o in enumerate(outs):
        d.process_packets_resident_device(a.data_ptr(), arena.size, depths, tab.data_ptr(), NB, Bk, pairs_ptr=o.pairs.data_ptr(), checked=c > 0, **o.ptrs())
    d.sync()
    for c, o in enumerate(outs): same(o.fetch(), run_packets(t, arena, depths, table.copy(), NB, Bk), f"call {c}")
    same([], [], "status", d, t)
    d.close(); t.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_reuse_emit(flavor):
    """the emit side: three rounds of dspi_process and dspi_packets_emit_resident on one device table, into an arena each; the first emit by the
    default route, the others with the warrant, nothing waiting anywhere after the first; the arenas equal the twin's three host-table rounds"""
    Bk = 45
    d, formats, table, ab, pcm = fleet(flavor, Bk, 71)
    t = warm(context(flavor, d.n_streams, FS, WL.full_chain_blob(int(flavor))))
    pattern, tab = arena_bytes(71, ab), np.array(table, dtype=np.uint64)
    dt = to_dev(tab)
    got, want = [], []
    for x, resident, keep in ((d, True, got), (t, False, want)):
        rounds = [buffers(x, pcm, Bk, False, pattern) for _ in range(3)]
        for c, (p, pairs, arena) in enumerate(rounds):
            x.process_device(p.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr())
            if resident: x.packets_emit_resident_device(pairs.data_ptr(), NB, Bk, formats, dt.data_ptr(), arena.data_ptr(), ab, checked=c > 0)
            else: x.packets_emit_device(pairs.data_ptr(), NB, Bk, formats, tab.copy(), arena.data_ptr(), ab)
        x.sync()
        keep += [arena.cpu().numpy() for _, _, arena in rounds]
    for c in range(3): assert np.array_equal(got[c], want[c]) and not np.array_equal(got[c], pattern), f"round {c}"
    d.close(); t.close()


# ---- 6. refusals write nothing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_process_refusals_write_nothing(flavor):
    """between two good calls: an illegal entry on the default route (the host-table call's code and text) and a table pointer offset by 8
    bytes, with either route; the pre-filled outputs are untouched, no status byte changes, and the next call equals the twin, which never
    saw them"""
    Bk = 45
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths, src, rng = depths_of(S), Source(S, Bk, 2 * NB), np.random.default_rng(8)
    for c in range(2):
        arena, table = scattered(lambda s, k: src.packet(s, depths[s], c * NB + k), depths, NB, rng)
        if c == 1:
            a, o = to_dev(arena), Outs(d, NB, Bk, fill=PREFILL)
            before = [d.status(s) for s in range(S)]
            out = host._Out(o.pairs.data_ptr(), o.sub.data_ptr(), o.peaks.data_ptr(), o.clip.data_ptr())
            dp = np.ascontiguousarray(depths)
            flags = host.MEM_DEVICE | host.OUT_CLIP_FLAGS
            call = lambda ptr, ab, tf=0: d.L.dspi_process_packets_resident(d.h, a.data_ptr(), ab, dp.ctypes.data, ptr, NB, Bk, C.byref(out), None, flags, tf)
            odd = table.copy(); odd[S - 1, 2] += 1; odd[S - 1, 0] = 2 ** 63
            assert call(to_dev(odd).data_ptr(), arena.size) == host.E_INVAL and f"entry {(S - 1) * NB} (stream {S - 1}, packet 0)" in err(d)
            text = err(d)
            assert d.L.dspi_process_packets(d.h, a.data_ptr(), arena.size, dp.ctypes.data, odd.ctypes.data, NB, Bk, C.byref(out), None, flags) == host.E_INVAL
            assert err(d) == text.replace("dspi_process_packets_resident", "dspi_process_packets")
            last = int(np.argmax(table))
            ends = int(table.reshape(-1)[last]) + Bk * MI.frame_bytes(int(depths[last // NB]))
            good = to_dev(table)
            assert d.packets_check_resident(depths, good.data_ptr(), NB, Bk, ends) is None
            assert call(good.data_ptr(), ends - 1) == host.E_INVAL and f"entry {last} " in err(d)
            padded = to_dev(np.concatenate([np.zeros(1, dtype=np.uint64), table.reshape(-1)]))      # the table at an address that is 8 mod 16
            for tf in (0, host.TABLE_CHECKED):
                assert call(padded.data_ptr() + 8, arena.size, tf) == host.E_INVAL and "16-byte aligned" in err(d)
            d.sync()
            for g, name in zip(o.fetch(), NAMES): assert (g.view(np.uint8) == PREFILL).all(), f"a refused call wrote {name}"
            assert [d.status(s) for s in range(S)] == before, "a refused call changed a status byte"
        same(run_resident(d, arena, depths, table, NB, Bk), run_packets(t, arena, depths, table.copy(), NB, Bk), f"call {c}", d, t)
    d.close(); t.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_emit_refusals_write_nothing(flavor):
    """an odd entry and an arena two bytes short on the default route, a table pointer offset by 8 bytes: the arena keeps its pattern, and the
    good call behind them equals the model"""
    Bk = 45
    d, formats, table, ab, pcm = fleet(flavor, Bk, 51)
    per = d.P * NB
    pattern = arena_bytes(51, ab)
    src, pairs, arena = buffers(d, pcm, Bk, False, pattern)
    d.process_device(src.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr())
    fm, tab = np.array(formats, dtype=np.uint8), np.array(table, dtype=np.uint64)
    call = lambda ptr, nbytes, tf=0: d.L.dspi_packets_emit_resident(d.h, pairs.data_ptr(), NB, Bk, fm.ctypes.data, ptr, arena.data_ptr(), nbytes, host.MEM_DEVICE, tf)
    live = np.argwhere(tab != MO.SKIP)
    s, i = (int(x) for x in live[len(live) // 2])
    odd = tab.copy(); odd[s, i] += 1
    assert call(to_dev(odd).data_ptr(), ab) == host.E_INVAL and f"entry {s * per + i} (stream {s}, pair {i // NB}, packet {i % NB})" in err(d)
    text = err(d)
    assert d.L.dspi_packets_emit(d.h, pairs.data_ptr(), NB, Bk, fm.ctypes.data, odd.ctypes.data, arena.data_ptr(), ab, host.MEM_DEVICE) == host.E_INVAL
    assert err(d) == text.replace("dspi_packets_emit_resident", "dspi_packets_emit")
    good = to_dev(tab)
    ends = tab.copy().reshape(-1); ends[ends == MO.SKIP] = 0
    last = int(np.argmax(ends + np.repeat(np.where(fm == 24, 6, 8).astype(np.uint64) * Bk, per)))      # (the entry that ends with the arena)
    assert call(good.data_ptr(), ab - 2) == host.E_INVAL and f"entry {last} " in err(d)
    padded = to_dev(np.concatenate([np.zeros(1, dtype=np.uint64), tab.reshape(-1)]))
    for tf in (0, host.TABLE_CHECKED):
        assert call(padded.data_ptr() + 8, ab, tf) == host.E_INVAL and "16-byte aligned" in err(d)
    d.sync()
    assert np.array_equal(arena.cpu().numpy(), pattern), "a refused call wrote the arena"
    assert call(good.data_ptr(), ab) == 0
    d.sync()
    assert np.array_equal(arena.cpu().numpy(), MO.emit(pattern, pairs.cpu().numpy(), formats, table, d.P, NB, Bk))
    d.close()


@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_a_paused_row_is_not_looked_at_until_it_is_resumed(flavor):
    """stream 4 is paused and its row holds ILLEGAL: the default route accepts the table and the call equals the twin's; after
    dspi_resume_streams the default route refuses the same table and names that row's first entry, as the host-table call does"""
    Bk = 45
    d, t, _ = pair(flavor)
    depths, src = depths_of(d.n_streams), Source(d.n_streams, Bk, NB)
    for x in (d, t): x.pause_streams(4, 1)
    arena, table = scattered(lambda s, k: src.packet(s, depths[s], k), depths, NB, np.random.default_rng(5))
    table[4] = np.uint64(ILLEGAL)
    same(run_resident(d, arena, depths, table, NB, Bk, fill=PREFILL), run_packets(t, arena, depths, table.copy(), NB, Bk, fill=PREFILL), "paused", d, t)
    for x in (d, t): x.resume_streams(4, 1)
    a, tab, o = to_dev(arena), to_dev(table), Outs(d, NB, Bk, fill=PREFILL)
    with pytest.raises(host.DspiError) as e:
        d.process_packets_resident_device(a.data_ptr(), arena.size, depths, tab.data_ptr(), NB, Bk, pairs_ptr=o.pairs.data_ptr(), **o.ptrs())
    assert e.value.code == host.E_INVAL and f"entry {4 * NB} (stream 4, packet 0)" in err(d)
    with pytest.raises(host.DspiError): d.packets_check_resident(depths, tab.data_ptr(), NB, Bk, arena.size)
    assert d.bad_entry == 4 * NB
    with pytest.raises(host.DspiError): t.packets_check(depths, table, NB, Bk, arena.size)
    assert t.bad_entry == 4 * NB
    d.sync()
    for g, name in zip(o.fetch(), NAMES): assert (g.view(np.uint8) == PREFILL).all(), f"the refused call wrote {name}"
    d.close(); t.close()


# ---- 7. the front end's cache ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_the_mixed_table_survives_a_resident_call(flavor):
    """mixed, resident packets (default route), mixed, resident packets (warranted), mixed on one context with the same depths and lengths
    every time: each mixed call would find its table cached unless the resident call, which uploads the depths alone into the same
    buffer, had said that the table is no longer a mixed call's.  A twin makes five plain mixed calls on the same bytes."""
    n, Bk = 2, 48
    d, t, _ = pair(flavor)
    S = d.n_streams
    depths = np.where(np.arange(S) % 2 == 0, 16, 24).astype(np.uint8)
    src = Source(S, Bk, 5 * n)
    for k, kind in enumerate(("mixed", "default", "mixed", "checked", "mixed")):
        buf, table = contiguous(lambda s, p: src.packet(s, depths[s], k * n + p), depths, n)
        want = run_mixed(t, buf, depths, n, Bk)
        got = run_mixed(d, buf, depths, n, Bk) if kind == "mixed" else run_resident(d, buf, depths, table, n, Bk, checked=kind == "checked")
        same(got, want, f"call {k} ({kind})")
    d.close(); t.close()
