"""Outputs to a packet table on the GPU (include/dspi.h: dspi_packets_emit).

dspi_process writes a context's pair words into a device buffer, stream-major or tiled, and dspi_packets_emit, behind it on the context's
stream with no synchronisation in between, turns them into packets in a device arena that was pre-filled with a pattern.  The WHOLE arena is
compared — with the model (tests/packets_out_model.py) applied to the same pair words, pattern bytes included; between a stream-major twin and
a tiled twin; with the chain oracle's pair words; and, the closed loop, through dspi_process_packets on a second context with the emit table
as its input table.

Shapes: 130 float streams (a whole tile of 128 and two columns), 70 Q28 streams (64 + 6); 96 kHz, 3 packets per call.  No figures: every
comparison is for equality."""
import functools
import random

import numpy as np
import pytest

import packets_out_model as M
from conftest import has_gpu
from dspi_amd import host, workloads as WL
from test_gpu_snapshot import context, fid, oracle
from test_packets_out_cpu import ILLEGAL, arena_bytes, make_table

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, NB = 96000, 3
FLAVORS = (1, 0)
LAYOUTS = (False, True)
lid = lambda tiled: "tiled" if tiled else "stream-major"


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the call"""
    assert hasattr(host.lib(), "dspi_packets_emit"), "libdspi_mi355x has no dspi_packets_emit"


def streams_of(flavor): return 130 if int(flavor) else 70


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


WARM_NB, WARM_BK = 16, 128      # 21 ms at 96 kHz: past the chain's silence and fade-in at power-on, so that the words under test are not zeros


@functools.lru_cache(maxsize=None)
def warm_pcm(S): return WL.synth_pcm16(S, WARM_NB * WARM_BK, FS)


def warm(d):
    """one process call that nobody looks at; warm_oracle does the same to a stream's oracle"""
    import torch
    p = to_dev(warm_pcm(d.n_streams))
    pairs = torch.zeros((d.n_streams, d.P, WARM_NB * WARM_BK, 2), dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    d.process_device(p.data_ptr(), WARM_NB, WARM_BK, 16, pairs_ptr=pairs.data_ptr())
    d.sync()
    assert pairs.any().item(), "the chain is still silent after the warm-up"
    return d


def warm_oracle(flavor, blob, S, s):
    o = oracle(flavor, FS, blob)
    o.process(warm_pcm(S)[s], WARM_NB, WARM_BK)
    return o


def buffers(d, pcm, Bk, tiled, pattern):
    """the device buffers of a process call and the emit behind it: pcm, pair words (zero), the arena holding `pattern`; everything has landed"""
    import torch
    S, F, P, R = d.n_streams, NB * Bk, d.P, d.tile_streams()
    pairs = torch.zeros(((S + R - 1) // R, 2 * P, F, R) if tiled else (S, P, F, 2), dtype=torch.int32, device=dev())
    p, arena = to_dev(pcm), to_dev(pattern)
    torch.cuda.synchronize()
    return p, pairs, arena


def process_and_emit(d, pcm, Bk, formats, table, pattern, tiled):
    """dspi_process into device pair words, then dspi_packets_emit behind it — nothing waits in between — into a pattern-filled device arena:
    (the arena, the pair words) as the two calls left them"""
    p, pairs, arena = buffers(d, pcm, Bk, tiled, pattern)
    d.process_device(p.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr(), tiled=tiled)
    tab = np.array(table, dtype=np.uint64)
    d.packets_emit_device(pairs.data_ptr(), NB, Bk, formats, tab, arena.data_ptr(), pattern.size, tiled=tiled)
    tab[:] = 0xDEADBEEF      # the caller may reuse its table when the call returns
    d.sync()
    return arena.cpu().numpy(), pairs.cpu().numpy()


def fleet(flavor, Bk, seed, paused=()):
    S = streams_of(flavor)
    d = warm(context(flavor, S, FS, WL.full_chain_blob(int(flavor))))
    r = random.Random(seed)
    formats = [r.choice((24, 32)) for _ in range(S)]
    table, ab = make_table(r, formats, d.P, NB, Bk, set(paused))
    return d, formats, table, ab, WL.synth_pcm16(S, NB * Bk, FS)


# ---- 1. against the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", LAYOUTS, ids=lid)
@pytest.mark.parametrize("Bk", (45, 96, 192))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_against_the_model(flavor, Bk, tiled):
    """a shuffled table, mixed formats, every even residue mod 16, touching entries and SKIPs: the whole arena equals the model applied to the
    pair words the process call wrote (fetched afterwards), pattern bytes included"""
    d, formats, table, ab, pcm = fleet(flavor, Bk, 10 * Bk + int(flavor))
    assert d.packets_emit_check(formats, table, NB, Bk, ab, overlap=True) is None
    pattern = arena_bytes(Bk, ab)
    got, words = process_and_emit(d, pcm, Bk, formats, table, pattern, tiled)
    assert words.any(), "the chain wrote nothing"
    assert np.array_equal(got, M.emit(pattern, words, formats, table, d.P, NB, Bk, d.tile_streams() if tiled else 0))
    d.close()


# ---- 2. layout independence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_layout_independence(flavor):
    """the same input through a stream-major twin and a tiled twin, one table: identical arenas"""
    Bk = 45
    d, formats, table, ab, pcm = fleet(flavor, Bk, 21)
    t = warm(context(flavor, d.n_streams, FS, WL.full_chain_blob(int(flavor))))
    pattern = arena_bytes(21, ab)
    a = process_and_emit(d, pcm, Bk, formats, table, pattern, False)[0]
    b = process_and_emit(t, pcm, Bk, formats, table, pattern, True)[0]
    assert not np.array_equal(a, pattern) and np.array_equal(a, b)
    d.close(); t.close()


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", LAYOUTS, ids=lid)
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_against_the_oracle(flavor, tiled):
    """format 32 and the identity table — entry (s, p, k) at 8 Bk ((s P + p) NB + k) —: the arena IS int32 [stream][pair][F][2], and equals the
    oracle's pair words stream by stream"""
    Bk = 96
    S = streams_of(flavor)
    blob = WL.full_chain_blob(int(flavor))
    d = warm(context(flavor, S, FS, blob))
    P, F = d.P, NB * Bk
    pcm = WL.synth_pcm16(S, F, FS)
    table = (np.arange(S * P * NB, dtype=np.uint64) * (8 * Bk)).reshape(S, P * NB)
    pattern = arena_bytes(3, S * P * F * 8)
    got = process_and_emit(d, pcm, Bk, [32] * S, table, pattern, tiled)[0].view("<i4").reshape(S, P, F, 2)
    assert got.any()
    for s in range(S):
        rp = warm_oracle(flavor, blob, S, s).process(pcm[s], NB, Bk)[0]
        assert np.array_equal(rp, got[s]), f"stream {s}: the arena differs from the oracle's pair words"
    d.close()


# ---- 4. the closed loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,tiled,fb", ((1, True, 0), (0, False, 1)), ids=("f32-tiled-into-q28", "q28-stream-major-into-f32"))
def test_closed_loop(fa, tiled, fb):
    """A emits every pair at format 24 into a shuffled arena; B runs dspi_process_packets on the SAME arena with A's table rows for pair p as its
    table and every depth 24.  WHICH CASE: A and B are two contexts, each with a HIP stream of its own, so A is waited for (dspi_sync) between
    the two calls; the arena never leaves the device.  B's pairs, sub, peaks and clip flags equal the chain oracle of B's flavour fed, at 24
    bit, the oracle's own pair-p output of A."""
    import torch
    Bk, p = 96, 1
    S = streams_of(fa)
    blob_a, blob_b = WL.full_chain_blob(fa), WL.full_chain_blob(fb)
    A, B = warm(context(fa, S, FS, blob_a)), warm(context(fb, S, FS, blob_b))
    P, F = A.P, NB * Bk
    pcm = WL.synth_pcm16(S, F, FS)
    table, ab = make_table(random.Random(31), [24] * S, P, NB, Bk, skip=0.0)
    table = np.array(table, dtype=np.uint64)
    out = [torch.zeros(shape, dtype=dt, device=dev()) for shape, dt in (((S, B.P, F, 2), torch.int32), ((S, F), torch.int32), ((S, NB, B.C), torch.int16), ((S,), torch.int16))]
    src, pairs, arena = buffers(A, pcm, Bk, tiled, arena_bytes(31, ab))
    A.process_device(src.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr(), tiled=tiled)
    A.packets_emit_device(pairs.data_ptr(), NB, Bk, [24] * S, table, arena.data_ptr(), ab, tiled=tiled)
    A.sync()
    rows = np.ascontiguousarray(table.reshape(S, P, NB)[:, p, :])
    assert B.packets_check([24] * S, rows, NB, Bk, ab) is None
    B.process_packets_device(arena.data_ptr(), ab, [24] * S, rows, NB, Bk, pairs_ptr=out[0].data_ptr(), sub_ptr=out[1].data_ptr(), peaks_ptr=out[2].data_ptr(), clip_ptr=out[3].data_ptr())
    B.sync()
    bp, bs, bk, bc = (x.cpu().numpy() for x in out)
    for s in list(range(0, S, 9)) + [S - 2, S - 1]:
        ap = warm_oracle(fa, blob_a, S, s).process(pcm[s], NB, Bk)[0][p]
        fed = np.ascontiguousarray(ap.astype("<i4")).view(np.uint8).reshape(F, 2, 4)[:, :, :3].reshape(-1)      # the 24-bit USB packets of pair p
        rp, rs, rk, rclip = warm_oracle(fb, blob_b, S, s).process(fed, NB, Bk, 24)
        assert ap.any() and rp.any()
        assert np.array_equal(rp, bp[s]) and np.array_equal(rs, bs[s]), f"stream {s}: B's words differ from the oracle's"
        assert np.array_equal(rk, bk[s].view(np.uint16)) and int(bc[s].view(np.uint16)) == rclip, f"stream {s}: B's peaks or clip flags differ from the oracle's"
    A.close(); B.close()


# ---- 5. paused streams -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", LAYOUTS, ids=lid)
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_paused_streams(flavor, tiled):
    """every third stream and the last one are paused and their rows hold illegal offsets: the call succeeds, nothing is written for them (the
    whole arena equals the model's, which leaves the pattern wherever no active stream's entry points), their neighbours are exact"""
    Bk = 45
    S = streams_of(flavor)
    paused = sorted(set(range(0, S, 3)) | {S - 1})
    d, formats, table, ab, pcm = fleet(flavor, Bk, 41, paused)
    assert all(x == ILLEGAL for x in table[0]) and table[1] != table[0]
    for s in paused: d.pause_streams(s, 1)
    active = [0 if s in paused else 1 for s in range(S)]
    assert d.packets_emit_check(formats, table, NB, Bk, ab, overlap=True) is None
    pattern = arena_bytes(41, ab)
    got, words = process_and_emit(d, pcm, Bk, formats, table, pattern, tiled)
    want = M.emit(pattern, words, formats, table, d.P, NB, Bk, d.tile_streams() if tiled else 0, active)
    assert np.array_equal(got, want) and not np.array_equal(got, pattern)
    d.close()


# ---- 6. refusals write nothing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_refusals_write_nothing(flavor):
    """an undefined flag, a format of 16, an odd entry and an entry whose packet ends two bytes past the arena, on a device arena: it keeps its
    pattern, and the good call behind them equals the model"""
    Bk = 45
    d, formats, table, ab, pcm = fleet(flavor, Bk, 51)
    S, per = d.n_streams, d.P * NB
    pattern = arena_bytes(51, ab)
    src, pairs, arena = buffers(d, pcm, Bk, False, pattern)
    d.process_device(src.data_ptr(), NB, Bk, 16, pairs_ptr=pairs.data_ptr())
    fm, tab = np.array(formats, dtype=np.uint8), np.array(table, dtype=np.uint64)
    call = lambda f, t, nbytes, flags: d.L.dspi_packets_emit(d.h, pairs.data_ptr(), NB, Bk, f.ctypes.data, t.ctypes.data, arena.data_ptr(), nbytes, flags)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    assert call(fm, tab, ab, host.MEM_DEVICE | host.OUT_SPDIF) == host.E_INVAL and "flags" in err()
    low = fm.copy(); low[S - 1] = 16
    assert call(low, tab, ab, host.MEM_DEVICE) == host.E_INVAL and f"stream {S - 1} " in err()
    live = np.argwhere(tab != M.SKIP)
    s, i = (int(x) for x in live[len(live) // 2])
    odd = tab.copy(); odd[s, i] += 1
    assert call(fm, odd, ab, host.MEM_DEVICE) == host.E_INVAL and f"entry {s * per + i} " in err()
    ends = tab.copy().reshape(-1); ends[ends == M.SKIP] = 0
    last = int(np.argmax(ends + np.repeat(np.where(fm == 24, 6, 8).astype(np.uint64) * Bk, per)))      # (the entry that ends with the arena)
    assert call(fm, tab, ab - 2, host.MEM_DEVICE) == host.E_INVAL and f"entry {last} " in err()
    d.sync()
    assert np.array_equal(arena.cpu().numpy(), pattern), "a refused call wrote the arena"
    assert call(fm, tab, ab, host.MEM_DEVICE) == 0
    d.sync()
    assert np.array_equal(arena.cpu().numpy(), M.emit(pattern, pairs.cpu().numpy(), formats, table, d.P, NB, Bk))
    d.close()
