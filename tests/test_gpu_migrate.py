"""Migration between two contexts on the GPU (dspi_migrate_streams / dspi_plan_migration, include/dspi.h): a stream that changes its context
goes on exactly as if it had stayed.  Every audio comparison is with the oracle, one oracle per STREAM fed that stream's own packets,
whichever slot of whichever context the stream sits in — never with another run of the library.  One schedule record (test_gpu_pause.py's
Sched) per context; relocate_across() below makes the records follow the streams from one schedule to the other.

    figures: none.  Source: 300 float streams (both contracts) / 200 Q28 streams — three rows, the last partial.  Destination: 2R + 5 streams,
    R = dspi_tile_streams: row 0 has residents and a handful of paused slots, row 1 is paused whole, the 5-stream last row partly.  48-frame
    packets at 48 kHz, the full chain (delays and leveller on).  The source has played out its power-on mute (12 packets, its row 1 one
    fewer), the destination has run 5 packets: the two contexts' write positions differ.
    The two-device path runs only where hipGetDeviceCount >= 2; on a one-GPU box its code is covered through DSPI_MIGRATE_VIA=copy."""
import struct

import numpy as np
import pytest

import orclib
from conftest import has_gpu
from orclib import PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, VOL, check, fid, oracle, packets
from test_gpu_realign import assert_rows_uniform
from test_gpu_pause import Sched
from test_gpu_move import move, streams_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48
TOTAL = 24          # packets of input per stream
SRC_RUN, DST_RUN = 12, 5


def sched_on(device, flavor, S, first_stream, statuses=False, total=TOTAL):
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, total * B, FS, first_stream=first_stream).copy()
    d = Dspi(flavor, S, device=device)
    assert d.set_rate(FS) == 0
    d.set_volume(VOL)
    assert d.load_bulk(blob) == 0
    return Sched(d, flavor, FS, blob, data, 16, B, VOL, statuses)


def dst_paused(R):
    """the destination's paused slots: a handful in row 0 (two lane mates among them), row 1 whole, two of the last row's five"""
    return [10, 11, 40, 41, 50] + list(range(R, 2 * R)) + [2 * R + 1, 2 * R + 3]


def two_contexts(flavor, statuses=False, dst_device=0, before_runs=None):
    """(source schedule, destination schedule, R) as the module's docstring describes them"""
    xs = sched_on(0, flavor, streams_of(flavor), 0, statuses)
    R = xs.d.tile_streams()
    xd = sched_on(dst_device, flavor, 2 * R + 5, 1000, statuses)
    if before_runs: before_runs(xs, xd)
    xs.run(SRC_RUN - 1)
    xs.pause(R, R); xs.run(1); xs.resume(R, R, as_is=True)      # the source's row 1 is one packet younger than its rows 0 and 2
    xd.run(DST_RUN)
    for s in dst_paused(R): xd.pause(s, 1)
    return xs, xd, R


def scattered_list(flavor, R):
    """nine entries: two lane mates (20, 21) into two lane mates; two streams of source row 0 (20, 30) into destination rows 0 and 1; source
    rows 0, 1 and 2 into destination row 1, whose lowest destination (R + 2) is not the list's first entry; both paused slots of the last row"""
    S = streams_of(flavor)
    return [(20, 10), (21, 11), (30, R + 7), (R + 5, R + 2), (2 * R + 10, 2 * R + 1), (R + 9, 2 * R + 3), (50, 40), (2 * R + 11, R + 60), (S - 1, 41)]


def relocate_across(xs, xd, moves, paused=False):
    """xs.d.migrate_streams(xd.d, moves) has been applied: input, position, history, hooks, frozen status and clip flags of every listed stream
    go from the source's schedule to the destination's.  The source slot keeps its record as a frozen copy (paused); the destination slot
    loses its own.  paused: DSPI_MIGRATE_PAUSED, every arrival is paused."""
    if not xd.data.flags.writeable: xd.data = xd.data.copy()
    for s, d in [(int(s), int(d)) for s, d in moves]:
        xd.data[d] = xs.data[s]; xd.pos[d] = xs.pos[s]; xd.last_clip[d] = xs.last_clip[s]
        xd.parts[d] = list(xs.parts[s]); xd.hooks[d] = {k: list(v) for k, v in xs.hooks[s].items()}
        xd.frozen.pop(d, None)
        here = (xs.d.status(s), int(xs.last_clip[s]))
        if s in xs.frozen: xd.frozen[d] = xs.frozen[s]
        elif paused: xd.frozen[d] = here
        if s not in xs.frozen: xs.frozen[s] = here


def migrate(xs, xd, moves, as_is=False, paused=False):
    assert xs.d.migrate_streams(xd.d, moves, as_is=as_is, paused=paused) == len(moves)
    relocate_across(xs, xd, moves, paused)


def assert_active_uniform(d, what):
    """every row's ACTIVE streams share one delay write index and one ring position"""
    R, S = d.tile_streams(), d.n_streams
    w, r = d.stream_positions(0, S)
    a = ~d.streams_paused().astype(bool)
    for row in range(-(-S // R)):
        sl = slice(row * R, min(S, (row + 1) * R))
        assert len(set(w[sl][a[sl]].tolist())) <= 1 and len(set(r[sl][a[sl]].tolist())) <= 1, f"{what}: the active streams of row {row} stand at different positions"


def close(*xs):
    for x in xs: x.d.close()


# ---- 1. a scattered list (also: 7. batches, 8. transports, 12. two devices) ----------------------------------------------------------------------
def scattered(flavor, as_is, statuses=False, dst_device=0):
    xs, xd, R = two_contexts(flavor, statuses, dst_device)
    s_d, d_d = xs.d, xd.d
    moves = scattered_list(flavor, R)
    ws, rs = s_d.stream_positions(0, s_d.n_streams)
    wd, rd = d_d.stream_positions(0, d_d.n_streams)
    assert ws[0] == SRC_RUN * B and ws[R] == (SRC_RUN - 1) * B and wd[0] == DST_RUN * B
    status = {s: s_d.status(s) for s, _ in moves}
    bulk = {s: s_d.collect_bulk(s) for s, _ in moves}
    src_paused, dst_paused_before = s_d.streams_paused().copy(), d_d.streams_paused().copy()
    migrate(xs, xd, moves, as_is=as_is)
    for s, t in moves:
        assert d_d.status(t) == status[s] and d_d.collect_bulk(t) == bulk[s], f"stream {s} -> {t}: status / parameters differ"
        assert s_d.status(s) == status[s] and s_d.collect_bulk(s) == bulk[s], f"the frozen copy in slot {s}"
    want = src_paused.copy(); want[[s for s, _ in moves]] = 1
    assert np.array_equal(s_d.streams_paused(), want), "every source slot is paused, nothing else in the source changes"
    want = dst_paused_before.copy(); want[[t for _, t in moves]] = 0
    assert np.array_equal(d_d.streams_paused(), want), "the activity travels with the stream"
    w1, r1 = d_d.stream_positions(0, d_d.n_streams)
    w2, r2 = s_d.stream_positions(0, s_d.n_streams)
    assert np.array_equal(w2, ws) and np.array_equal(r2, rs), "the source's positions are untouched"
    if as_is:
        for s, t in moves: assert w1[t] == ws[s] and r1[t] == rs[s], "DSPI_MIGRATE_AS_IS keeps every stream's own positions"
    else:
        assert_rows_uniform(d_d, "after the default migration", rows=(0, 2))      # (their paused slots were paused at the rows' own positions)
        assert w1[0] == wd[0] and r1[0] == rd[0] and w1[2 * R] == wd[2 * R], "the rows' residents did not move"
        for t in (R + 2, R + 7, R + 60):
            assert w1[t] == ws[R + 5] and r1[t] == rs[R + 5], "a row without a resident takes the pair of the stream at its lowest destination"
        assert w1[R + 2] != w1[0]
    others = np.ones(d_d.n_streams, dtype=bool); others[[t for _, t in moves]] = False
    assert np.array_equal(w1[others], wd[others]) and np.array_equal(r1[others], rd[others]), "a slot the list does not name was moved"
    for n in (2, 3):
        xs.run(n); xd.run(n)
    if not as_is: assert_active_uniform(d_d, "after the continuation")
    # the frozen copies are the streams as they stood at the call: resumed, and fed the same input, they go the same way
    xs.resume(0, s_d.n_streams)
    xs.run(1)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("as_is", (False, True), ids=("realigned", "as-is"))
def test_scattered_list(flavor, as_is):
    scattered(flavor, as_is, statuses=True)


@pytest.mark.parametrize("flavor,batch", ((W.F32_FMA, 2), (0, 3), (W.F32_FMA, 3), (0, 2)), ids=("fma-2", "q28-3", "fma-3", "q28-2"))
def test_batches(flavor, batch, monkeypatch):
    """the nine entries through a scratch of two / three records: five / three batches, the source's stream waiting for the destination's
    scatter before every gather but the first"""
    monkeypatch.setenv("DSPI_MOVE_BATCH", str(batch))
    scattered(flavor, False)


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("via", ("copy", "host"))
def test_transports(flavor, via, monkeypatch):
    """DSPI_MIGRATE_VIA=copy (the two-device code with equal device numbers) and =host give the oracle's words, as the default transport does
    in test_scattered_list; host also in batches"""
    monkeypatch.setenv("DSPI_MIGRATE_VIA", via)
    if via == "host": monkeypatch.setenv("DSPI_MOVE_BATCH", "4")
    scattered(flavor, False)


def test_two_devices():
    import torch
    if torch.cuda.device_count() < 2: pytest.skip("hipGetDeviceCount < 2: the two-device path is covered through DSPI_MIGRATE_VIA=copy only")
    scattered(W.F32_FMA, False, dst_device=1)


# ---- 2. parameters travel by value ----------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_parameters_travel_by_value(flavor):
    """Sources with presets of their own, one of which the destination already holds; one source with a preset-slot load (mute, zeroed lines)
    issued right before the call with no dspi_process in between; a band change on an arrival at its new slot."""
    gain_a, gain_b = (W.REQ["SET_PREAMP"], 0, struct.pack("<f", -1.25)), (W.REQ["SET_PREAMP"], 0, struct.pack("<f", -7.5))
    band = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, FS, other); image = ref.save_slot(0); ref.close()

    def presets(xs, xd):
        xs.request("vendor_set", *gain_a, stream=20); xs.request("vendor_set", *gain_a, stream=21); xs.request("vendor_set", *gain_b, stream=50)
        xd.request("vendor_set", *gain_a, stream=0)
    xs, xd, R = two_contexts(flavor, before_runs=presets)
    moves = scattered_list(flavor, R)
    assert xs.d.image_count() == 4 and xd.d.image_count() == 2
    xs.request("load_slot", image, -1, stream=30)
    assert xs.d.image_count() == 5
    bulk = {s: xs.d.collect_bulk(s) for s, _ in moves}
    migrate(xs, xd, moves)
    assert xs.d.image_count() == 5, "the source keeps its objects"
    # (five objects arrived — the shared one, A twice, B, the slot load —; dspi_debug_image_count folds what is equal, as the next commit does)
    assert xd.d.image_count() == 4, "the shared preset and both A fold into the destination's own"
    for s, t in moves: assert xd.d.collect_bulk(t) == bulk[s]
    assert xd.d.collect_bulk(R + 7) != xd.d.collect_bulk(R + 2)
    xs.run(1); xd.run(1)
    assert xd.d.image_count() == 4, "the shared preset and A fold into the destination's own at its next commit"
    xd.request("vendor_set", *band, stream=R + 2); xd.request("set_volume", -7 * 256, stream=11)
    xs.run(2); xd.run(2); xd.run(3)
    assert xd.d.image_count() == 6
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


# ---- 3. activity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("paused", (False, True), ids=("as-it-was", "DSPI_MIGRATE_PAUSED"))
def test_activity(flavor, paused):
    xs, xd, R = two_contexts(flavor)
    moves = scattered_list(flavor, R)
    xs.pause(30, 1); xs.pause(R + 9, 1)
    xs.run(1); xd.run(1)
    frozen = {s: xs.frozen[s] for s in (30, R + 9)}
    migrate(xs, xd, moves, paused=paused)
    p = xd.d.streams_paused().astype(bool)
    for s, t in moves: assert p[t] == (paused or s in frozen), (s, t)
    for s, t in moves:
        if s in frozen: assert xd.d.status(t) == frozen[s][0], "a paused source arrives paused and frozen"
    assert xs.d.streams_paused()[[s for s, _ in moves]].all(), "every source slot is paused afterwards"
    xs.run(2); xd.run(2)
    for _, t in moves: xd.resume(t, 1)
    assert_active_uniform(xd.d, "after the resumes")
    xs.run(1); xd.run(2); xd.run(1)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


# ---- 4. S/PDIF positions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("modes", ((True, True), (False, True), (True, False)), ids=("both-per-stream", "destination-only", "source-only"))
def test_spdif_positions(flavor, modes):
    """DSPI_OUT_SPDIF subframes of the arrivals (and of some residents) against the oracle's encoder on the oracle's pair words, at the position
    the contract names: the stream's own / the source context's / none (the destination's context position)."""
    src_on, dst_on = modes
    xs, xd, R = two_contexts(flavor)
    s_d, d_d = xs.d, xd.d
    moves = scattered_list(flavor, R)
    s_d.spdif_block_pos(48); d_d.spdif_block_pos(96)
    assert s_d.spdif_per_stream(int(src_on)) == src_on and d_d.spdif_per_stream(int(dst_on)) == dst_on      # (every stream takes its context's position)
    if src_on:
        s_d.spdif_stream_pos(20, 2, set=[100, 191])
        s_d.pause_streams(50, 1)                                                         # a paused source: its frozen position travels
        s_d.spdif_stream_pos(50, 1, set=[7])
        s_d.resume_streams(50, 1)
    own = {s: 48 for s, _ in moves}
    if src_on: own.update({20: 100, 21: 191, 50: 7})
    migrate(xs, xd, moves)
    assert s_d.spdif_block_pos() == 48 and d_d.spdif_block_pos() == 96, "the contexts' own positions are not touched"
    if src_on: assert all(int(s_d.spdif_stream_pos(s, 1)[0]) == own[s] for s, _ in moves), "the frozen copies keep their positions"
    expect = {t: (own[s] if src_on else 48) if dst_on else 96 for s, t in moves}
    expect.update({r: 96 for r in (0, 12, 2 * R, 2 * R + 4)})
    if dst_on: assert all(int(d_d.spdif_stream_pos(t, 1)[0]) == p for t, p in expect.items())
    n = 5      # 240 frames: every position wraps inside the call
    pcm, paused = xd.input(n)
    got = d_d.process_host(pcm, n, B, 16, spdif=True)[0]
    for t, pos in expect.items():
        o = oracle(flavor, FS, xd.blob)
        for p0, p1, _, _ in xd.parts[t]: o.process(packets(xd.data[t], 16, B, p0, p1), p1 - p0, B, 16)
        at = int(xd.pos[t])
        words = o.process(packets(xd.data[t], 16, B, at, at + n), n, B, 16)[0]
        o.close()
        if t in dict((d, s) for s, d in moves): assert int(np.abs(words).max()) > 0      # (the arrivals have played out their power-on mute)
        for p in range(d_d.P):
            assert np.array_equal(got[t][p], orclib.spdif_encode(words[p], pos, FS)[0]), f"subframes of the stream in slot {t}, pair {p}, expected at block position {pos}"
    assert not got[paused].any()
    assert d_d.spdif_block_pos() == (96 + n * B) % 192
    if dst_on: assert all(int(d_d.spdif_stream_pos(t, 1)[0]) == (p + n * B) % 192 for t, p in expect.items())
    close(xs, xd)


# ---- 5. PDM ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("used", (True, False), ids=("modulator-used", "modulator-never-used"))
def test_pdm_continues(flavor, used):
    """dspi_pdm_modulate before the call on the source and after it on the destination against ONE PdmOracle per stream; a source that never
    ran the modulator hands over power-on words, also into a context whose own modulators have a history"""
    xs, xd, R = two_contexts(flavor)
    moves = scattered_list(flavor, R)
    sub = xs.run(2)[1]
    pdm = {s: PdmOracle() for s, _ in moves}
    if used:
        words = xs.d.pdm_host(sub)
        for s, _ in moves: assert np.array_equal(pdm[s].run(sub[s]), words[s]), f"PDM words of source stream {s} before the call"
    else:
        xd.d.pdm_host(np.full((xd.d.n_streams, 64), 12345678, dtype=np.int32))
    migrate(xs, xd, moves)
    for n in (1, 2):
        sub = xd.run(n)[1]
        words = xd.d.pdm_host(sub)
        for s, t in moves: assert np.array_equal(pdm[s].run(sub[t]), words[t]), f"PDM words of the stream {s} -> {t} after the call"
    xd.verify([t for _, t in moves] + [0, 2 * R], what="destination ")
    close(xs, xd)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_refusals(flavor):
    xs, xd, R = two_contexts(flavor)
    s_d, d_d = xs.d, xd.d
    Ss, Sd = s_d.n_streams, d_d.n_streams
    L = s_d.L
    before = (s_d.streams_paused().copy(), d_d.streams_paused().copy(), s_d.image_count(), d_d.image_count())

    def mg(moves, flags=0, a=s_d, b=d_d):
        m = np.asarray(moves, dtype=np.uint32).reshape(-1, 2)
        return L.dspi_migrate_streams(a.h if a else None, b.h if b else None, m.ctypes.data if len(m) else None, len(m), flags)
    for bad in ([], [(Ss, 10)], [(0, Sd)], [(0, Ss - 1)], [(1, 10), (1, 11)], [(1, 10), (2, 10)], [(1, 0)], [(1, 10), (2, 12)]):
        assert mg(bad) == host.E_INVAL, bad
        with pytest.raises(DspiError) as e: s_d.migrate_streams(d_d, bad)
        assert e.value.code == host.E_INVAL
    assert L.dspi_migrate_streams(s_d.h, d_d.h, None, 2, 0) == host.E_INVAL
    for flags in (0x4, 0x100, 0x80000001): assert mg([(1, 10)], flags) == host.E_INVAL
    assert mg([(1, 10)], a=None) == host.E_INVAL and mg([(1, 10)], b=None) == host.E_INVAL
    assert mg([(1, 10)], a=d_d) == host.E_INVAL and mg([(1, 10)], b=s_d) == host.E_INVAL      # src == dst
    for fl in ((0, 1) if int(flavor) else (1, W.F32_FMA)):      # another flavour; the float flavour's other contract
        q = Dspi(fl, 16, device=0); q.pause_streams(0, 16)
        assert mg([(1, 10)], b=q) == host.E_INVAL, fl
        q.close()
    h = Dspi(flavor, 16, device=None); h.pause_streams(0, 16)
    assert mg([(1, 10)], b=h) == host.E_NODEVICE and mg([(1, 20)], b=h) == host.E_INVAL
    h.close()
    after = (s_d.streams_paused(), d_d.streams_paused(), s_d.image_count(), d_d.image_count())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # no byte of either context has changed: both continue exactly, every stream of both
    xs.run(2); xd.run(2)
    xd.resume(0, Sd)
    xs.run(1); xd.run(1)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


# ---- 9. there and back ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_there_and_back(flavor):
    xs, xd, R = two_contexts(flavor)
    moves = scattered_list(flavor, R)
    migrate(xs, xd, moves)
    xs.run(2); xd.run(2)
    # some come back, into other slots of the source (vacated by others: paused, frozen copies that are now overwritten)
    back = [(10, 21), (R + 2, 30), (2 * R + 3, 2 * R + 11), (41, 20)]
    migrate(xd, xs, back)
    assert not xs.d.streams_paused()[[t for _, t in back]].any() and xd.d.streams_paused()[[s for s, _ in back]].all()
    assert_active_uniform(xs.d, "the source after the return")
    xs.run(1); xd.run(1); xs.run(2); xd.run(2)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


# ---- 10. the plan, a grow, the migration, a shrink ------------------------------------------------------------------------------------------------
def grow(x, n):
    """x.d.resize_streams(n, paused=True): the schedule's per-slot records follow; the new slots are paused power-on devices"""
    old = x.d.n_streams
    x.d.resize_streams(n, paused=True)
    x.data = np.concatenate([x.data, np.zeros((n - old,) + x.data.shape[1:], dtype=x.data.dtype)])
    x.pos = np.concatenate([x.pos, np.zeros(n - old, dtype=np.int64)])
    x.last_clip = np.concatenate([x.last_clip, np.zeros(n - old, dtype=np.uint16)])
    for s in range(old, n):
        x.parts.append([]); x.hooks.append(dict())
        x.frozen[s] = (x.d.status(s), 0)


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_plan_round_trip(flavor):
    xs, xd, R = two_contexts(flavor)
    s_d, d_d = xs.d, xd.d
    Ss, Sd = s_d.n_streams, d_d.n_streams
    free = len(dst_paused(R))
    want = free + 9                                    # more than the destination has room for
    assert len(s_d.plan_migration(d_d, want)) == free
    grow(xd, Sd + want - free)
    plan = s_d.plan_migration(d_d, want)
    assert len(plan) == want and plan[:, 0].tolist() == list(range(Ss - want, Ss))
    assert plan[:, 1].tolist() == sorted(dst_paused(R)) + list(range(Sd, Sd + 9))
    migrate(xs, xd, plan)
    assert not d_d.streams_paused().any(), "every paused slot of the destination was filled"
    # the source's top is paused, which is what a cut range must be
    assert s_d.resize_streams(Ss - want) == Ss - want
    assert len(s_d.plan_migration(d_d, want)) == 0
    assert_active_uniform(d_d, "after the planned migration")
    xs.run(2); xd.run(2); xs.run(1); xd.run(1)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)


# ---- 11. a small random crossing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_random_crossing(seed):
    """random legal sequences of run / pause / resume / migrate (both directions) / move over the two contexts, verified at the end"""
    rng = np.random.default_rng(seed)
    flavor = (W.F32_FMA, 0, 1)[seed % 3]
    xs, xd, R = two_contexts(flavor)
    xx = (xs, xd)
    left = TOTAL - SRC_RUN - 1
    for step in range(14):
        op = rng.choice(["run", "run", "pause", "resume", "migrate", "migrate", "move"])
        if op == "run" and left >= 2:
            n = int(rng.integers(1, 3)); left -= n
            xs.run(n); xd.run(n)
        elif op in ("pause", "resume"):
            x = xx[int(rng.integers(0, 2))]
            first = int(rng.integers(0, x.d.n_streams - 1)); count = int(rng.integers(1, min(40, x.d.n_streams - first) + 1))
            if op == "pause": x.pause(first, count)
            else: x.resume(first, count, as_is=bool(rng.integers(0, 2)))
        elif op == "migrate":
            a, b = (xs, xd) if rng.integers(0, 2) else (xd, xs)
            free = np.flatnonzero(b.d.streams_paused())
            k = int(min(len(free), rng.integers(1, 12)))
            if not k: continue
            moves = list(zip(rng.choice(a.d.n_streams, k, replace=False).tolist(), rng.choice(free, k, replace=False).tolist()))
            migrate(a, b, moves, as_is=bool(rng.integers(0, 4) == 0), paused=bool(rng.integers(0, 4) == 0))
        elif op == "move":
            x = xx[int(rng.integers(0, 2))]
            p = x.d.streams_paused().astype(bool)
            if not p.any() or p.all(): continue
            k = int(min(p.sum(), (~p).sum(), rng.integers(1, 8)))
            moves = list(zip(rng.choice(np.flatnonzero(~p), k, replace=False).tolist(), rng.choice(np.flatnonzero(p), k, replace=False).tolist()))
            move(x, moves, as_is=bool(rng.integers(0, 2)))
    xs.run(1); xd.run(1)
    xs.verify(what="source "); xd.verify(what="destination ")
    close(xs, xd)
