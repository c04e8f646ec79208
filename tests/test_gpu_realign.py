"""Realignment on the GPU (DSPI_SNAP_REALIGN on dspi_import_streams, dspi_realign_streams, include/dspi.h): imported streams take the delay
write index and the leveller ring position of their destination row, their lines and rings rotated to match, and go on exactly as the
oracle does.  Every audio comparison is with the oracle fed the whole input — pair words, sub words, per-packet peaks, status bytes, clip
flags (check() of test_gpu_snapshot.py) — never with another run of the library; dspi_debug_stream_positions proves that a scenario
really was misaligned before and is uniform per row after."""
import struct

import numpy as np
import pytest

from conftest import has_gpu
from orclib import PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, as_input, check, context, fid, oracle, packets, part, run, _fuzz_seeds, _tile_input

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

RING = 1024


def line_len(flavor):
    return 4096 if int(flavor) else 2048


def assert_rows_uniform(d, what, rows=None):
    """every row's streams (those below n_streams) share one delay write index and one ring position"""
    R, S = d.tile_streams(), d.n_streams
    w, r = d.stream_positions(0, S)
    for row in (range((S + R - 1) // R) if rows is None else rows):
        ws, rs = w[row * R:(row + 1) * R], r[row * R:(row + 1) * R]
        assert len(set(ws.tolist())) == 1 and len(set(rs.tolist())) == 1, f"{what}: row {row} holds write indices {sorted(set(ws.tolist()))}, ring positions {sorted(set(rs.tolist()))}"


def rows_mixed(d, rows):
    R = d.tile_streams()
    w, r = d.stream_positions(0, d.n_streams)
    return all(len(set(w[row * R:(row + 1) * R].tolist())) > 1 and len(set(r[row * R:(row + 1) * R].tolist())) > 1 for row in rows)


def touched_rows(d, first, count):
    R = d.tile_streams()
    return range(first // R, (first + count - 1) // R + 1)


def relocation(flavor, fs, B, depth=16, n=12, nb=7, SA=300, SB=200, f0=100, t0=91, cnt=70):
    """The set-up of test_gpu_snapshot.py::test_relocation_beside_foreign_streams up to the hand-over: A (SA streams) has run n packets, B (SB
    streams, another preset) nb packets."""
    blob_a = WL.full_chain_blob(flavor)
    blob_b = WL.full_chain_blob(flavor, max_delay_ms=7.0)
    blob_b["preamp"]["preamp_db"][:] = (-1.0, -5.0)
    blob_b["leveller"]["speed"] = 2
    da = as_input(WL.synth_pcm16(SA, 2 * n * B, fs), depth)
    db = as_input(WL.synth_pcm16(SB, (nb + n) * B, fs, first_stream=1000), depth)
    a = context(flavor, SA, fs, blob_a)
    b = context(flavor, SB, fs, blob_b, vol=-11 * 256)
    a1 = run(a, da, depth, B, 0, n)
    b1 = run(b, db, depth, B, 0, nb)
    return dict(flavor=flavor, fs=fs, B=B, depth=depth, n=n, nb=nb, SA=SA, SB=SB, f0=f0, t0=t0, cnt=cnt, blob_a=blob_a, blob_b=blob_b, da=da, db=db, a=a, b=b, a1=a1, b1=b1)


def assert_ages_differ(x):
    """the precondition: A's and B's positions are what their frame counts say, and differ"""
    L = line_len(x["flavor"])
    wa, ra = x["a"].stream_positions(0, x["SA"])
    wb, rb = x["b"].stream_positions(0, x["SB"])
    fa, fb = x["n"] * x["B"], x["nb"] * x["B"]
    assert set(wa.tolist()) == {fa % L} and set(ra.tolist()) == {fa % RING}, (sorted(set(wa.tolist())), sorted(set(ra.tolist())))
    assert set(wb.tolist()) == {fb % L} and set(rb.tolist()) == {fb % RING}, (sorted(set(wb.tolist())), sorted(set(rb.tolist())))
    assert fa % L != fb % L and fa % RING != fb % RING
    return (fa % L, fa % RING), (fb % L, fb % RING)


def continue_and_check(x, n2=None):
    """B's next packets: streams [t0, t0 + cnt) carry A's input from packet n on, the others B's own from packet nb on; all SB streams
    against their oracles"""
    flavor, fs, B, depth, n, nb, f0, t0, cnt, a, b = (x[k] for k in ("flavor", "fs", "B", "depth", "n", "nb", "f0", "t0", "cnt", "a", "b"))
    n2 = n if n2 is None else n2
    mixed = packets(x["db"], depth, B, nb, nb + n2)
    mixed[t0:t0 + cnt] = packets(x["da"], depth, B, n, n + n2)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n2)
    for s in range(x["SB"]):
        tail = (b2[0][s], b2[1][s], b2[2][s], b2[3][s])
        if t0 <= s < t0 + cnt:
            k = s - t0 + f0
            check(oracle(flavor, fs, x["blob_a"]), x["da"][k], depth, B, [part(x["a1"], k, 0, n), (n, n + n2, tail, b.status(s))], f"imported stream {k} -> {s}")
        else:
            check(oracle(flavor, fs, x["blob_b"], vol=-11 * 256), x["db"][s], depth, B, [part(x["b1"], s, 0, nb), (nb, nb + n2, tail, b.status(s))], f"resident stream {s}")
    return b2


# ---- 1. relocation, realigned; 2. unaligned shifts -----------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("fs,B", [(48000, 48), (44100, 45)], ids=("48k-576-vs-336", "44k1-540-vs-315"))
def test_relocation_realigned(flavor, fs, B):
    """Streams [100, 170) of A (300 streams, 12 packets) go to [91, 161) of B (200 streams, another preset, 7 packets) with the flag: an odd
    shift across a row boundary.  With 48-frame packets the positions are 576 against 336, with 45-frame packets 540 against 315 — a
    rotation by 225 words, odd and not a multiple of four (record-side runs that start on no 16-byte boundary), on 4096-word float lines and
    2048-word Q28 lines.  Afterwards every stream of B in a touched row reports the residents' positions, and B's next 12 packets are the
    oracles' for all 200 streams."""
    x = relocation(flavor, fs, B)
    pa, pb = assert_ages_differ(x)
    assert (pa[0], pb[0]) == ((576, 336) if B == 48 else (540, 315))
    a, b = x["a"], x["b"]
    head, state = a.export_streams(x["f0"], x["cnt"])
    assert b.import_streams(x["t0"], head, state, realign=True) == x["cnt"]
    assert b.image_count() == 2
    w, r = b.stream_positions(0, x["SB"])
    assert set(w.tolist()) == {pb[0]} and set(r.tolist()) == {pb[1]}, (sorted(set(w.tolist())), sorted(set(r.tolist())))
    wa, ra = a.stream_positions(0, x["SA"])      # (the source is not touched)
    assert set(wa.tolist()) == {pa[0]} and set(ra.tolist()) == {pa[1]}
    continue_and_check(x)
    assert_rows_uniform(b, "after 12 more packets")
    a.close(); b.close()


# ---- 3. whole rows into a fresh context are the plain import --------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_whole_rows_into_a_fresh_context_are_the_plain_import(flavor):
    """300 streams into a fresh 300-stream context, once plain and once with the flag: no row has a resident (the last one is partly
    filled), every row's first stream moves by 0 and its row mates already agree with it: the two destinations export the same bytes."""
    fs, B, n, S = 48000, 48, 9, 300
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, n * B, fs)
    a = context(flavor, S, fs, blob)
    run(a, data, 16, B, 0, n)
    head, state = a.export_streams(0, S)
    p, q = Dspi(flavor, S, device=0), Dspi(flavor, S, device=0)
    assert p.import_streams(0, head, state) == S and q.import_streams(0, head, state, realign=True) == S
    hp, sp = p.export_streams(0, S)
    hq, sq = q.export_streams(0, S)
    assert hp == hq and np.array_equal(sp, sq)
    assert np.array_equal(sp, state)      # (and both are what A gave)
    w, _ = q.stream_positions(0, S)
    assert set(w.tolist()) == {(n * B) % line_len(flavor)}
    for d in (a, p, q): d.close()


# ---- 4. many ages in one row ----------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_many_ages_in_one_row(flavor):
    """Five donors that ran 3, 5, 8, 13 and 21 packets give one stream each, one import at a time with the flag, into scattered slots of row 1
    of a destination that ran 10 (the row's first slot among them: its neighbour is then the second).  The row's positions stay uniform
    after every import, and all of the destination's streams go on like their oracles."""
    fs, B, depth, nb, n2 = 48000, 48, 16, 10, 8
    ages = (3, 5, 8, 13, 21)
    blob = WL.full_chain_blob(flavor)
    R = 128 if int(flavor) else 64
    SB = 2 * R + 40
    b = context(flavor, SB, fs, blob)
    assert b.tile_streams() == R
    slots = [R + 17, R, R + 2, R + R // 2 + 1, 2 * R - 1]      # scattered over row 1: odd and even, the first and the last
    db = WL.synth_pcm16(SB, (nb + n2) * B, fs, first_stream=3000)
    b1 = run(b, db, depth, B, 0, nb)
    want = (nb * B % line_len(flavor), nb * B % RING)
    donors = []
    for i, (age, slot) in enumerate(zip(ages, slots)):
        dd = WL.synth_pcm16(3, (age + n2) * B, fs, first_stream=100 * (i + 1))
        d = context(flavor, 3, fs, blob)
        d1 = run(d, dd, depth, B, 0, age)
        wd, rd = d.stream_positions(1, 1)
        assert (int(wd[0]), int(rd[0])) == (age * B % line_len(flavor), age * B % RING) != want
        head, state = d.export_streams(1, 1)
        assert b.import_streams(slot, head, state, realign=True) == 1
        w, r = b.stream_positions(0, SB)
        assert set(w.tolist()) == {want[0]} and set(r.tolist()) == {want[1]}, f"after the donor of age {age}: {sorted(set(w.tolist()))} {sorted(set(r.tolist()))}"
        donors.append((age, slot, dd, d1))
        d.close()
    mixed = packets(db, depth, B, nb, nb + n2)
    for age, slot, dd, _ in donors: mixed[slot] = packets(dd, depth, B, age, age + n2)[1]
    b2 = run(b, mixed, depth, B, 0, n2)
    assert b.image_count() == 1
    taken = {slot: (age, dd, d1) for age, slot, dd, d1 in donors}
    for s in range(SB):
        tail = tuple(x[s] for x in b2)
        if s in taken:
            age, dd, d1 = taken[s]
            check(oracle(flavor, fs, blob), dd[1], depth, B, [part(d1, 1, 0, age), (age, age + n2, tail, b.status(s))], f"donor of age {age} -> {s}")
        else:
            check(oracle(flavor, fs, blob), db[s], depth, B, [part(b1, s, 0, nb), (nb, nb + n2, tail, b.status(s))], f"resident stream {s}")
    assert_rows_uniform(b, "after the continuation")
    b.close()


# ---- 5. in place ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_realign_in_place(flavor):
    """The plain import of test 1 leaves B's touched rows mixed (asserted); dspi_realign_streams over B's whole range makes every row
    uniform — the rows align to their first streams — without touching an image, the next packets are the oracles', and a second call
    changes nothing."""
    x = relocation(flavor, 48000, 48)
    pa, pb = assert_ages_differ(x)
    a, b = x["a"], x["b"]
    head, state = a.export_streams(x["f0"], x["cnt"])
    assert b.import_streams(x["t0"], head, state) == x["cnt"]
    rows = touched_rows(b, x["t0"], x["cnt"])
    assert rows_mixed(b, rows)
    images = b.image_count()
    w0, r0 = b.stream_positions(0, x["SB"])
    assert b.realign_streams(0, x["SB"]) == x["SB"]
    assert_rows_uniform(b, "after dspi_realign_streams")
    w, r = b.stream_positions(0, x["SB"])
    R = b.tile_streams()
    first_of_row = np.arange(x["SB"]) // R * R      # the range holds every row whole: each aligns to the positions its first stream had
    assert np.array_equal(w, w0[first_of_row]) and np.array_equal(r, r0[first_of_row])
    assert {int(v) for v in w} <= {pa[0], pb[0]} and int(w[0]) == pb[0]
    assert b.image_count() == images
    h1, s1 = b.export_streams(0, x["SB"])
    assert b.realign_streams(0, x["SB"]) == x["SB"]
    h2, s2 = b.export_streams(0, x["SB"])
    assert h1 == h2 and np.array_equal(s1, s2)
    continue_and_check(x)
    a.close(); b.close()


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_realign_in_place_part_of_a_context(flavor):
    """... over a range that starts and ends inside rows, in a context long enough for several chunks of the device scratch (2 float rows / 8
    Q28 rows each): the range's first row aligns to its resident below, the last to the resident behind the range, the rows between to
    their own first streams — in two of them these came from A — and streams outside the range are not written."""
    S = 700
    x = relocation(flavor, 48000, 48, n=6, nb=4, SA=S, SB=S, f0=0, t0=30, cnt=S - 60)
    pa, pb = assert_ages_differ(x)
    a, b = x["a"], x["b"]
    R = b.tile_streams()
    f1, c1 = 2 * R + 5, 3 * R - 9      # the streams of A that go over: [f1, f1 + c1) -> the same slots of B; rows 2 .. 4
    head, state = a.export_streams(f1, c1)
    assert b.import_streams(f1, head, state) == c1
    x.update(f0=f1, t0=f1, cnt=c1)
    assert rows_mixed(b, (2, 4))
    before_h, before_s = b.export_streams(0, S)
    lo, cnt = R + 11, S - R - 11 - 40      # realign [lo, lo + cnt): from inside row 1 to inside the last row
    assert b.realign_streams(lo, cnt) == cnt
    w, r = b.stream_positions(0, S)
    want_w = np.full(S, pb[0]); want_r = np.full(S, pb[1])
    want_w[3 * R:5 * R] = pa[0]; want_r[3 * R:5 * R] = pa[1]      # rows 3 and 4 lie inside the range whole and begin with streams that came from A
    assert np.array_equal(w, want_w) and np.array_equal(r, want_r), (np.flatnonzero(w != want_w)[:8].tolist(), np.flatnonzero(r != want_r)[:8].tolist())
    after_h, after_s = b.export_streams(0, S)
    outside = np.r_[0:lo, lo + cnt:S]
    assert after_h == before_h and np.array_equal(after_s[outside], before_s[outside])
    continue_and_check(x, n2=6)
    a.close(); b.close()


# ---- 6. other kernel families ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (1, W.F32_FMA), ids=fid)
@pytest.mark.parametrize("blob_kind", ("latency-preset", "full-chain"))
def test_latency_layout(flavor, blob_kind, monkeypatch):
    """DSPI_F32_LAYOUT=skew: the latency layout's own preset class (master PEQ, delays at the edge values, leveller off: only the delay
    lines rotate) and the full chain (its leveller shape: the rings rotate too).  37 streams of A go to [3, 40) of a 64-stream B of
    another age, realigned."""
    from test_gpu_parity import _latency_blob
    monkeypatch.setenv("DSPI_F32_LAYOUT", "skew")
    fs, B, depth, n, nb, S, SB, t0 = 48000, 48, 16, 12, 5, 37, 64, 3
    blob = _latency_blob() if blob_kind == "latency-preset" else WL.full_chain_blob(flavor)
    da = WL.synth_pcm16(S, 2 * n * B, fs)
    db = WL.synth_pcm16(SB, (nb + n) * B, fs, first_stream=700)
    a = context(flavor, S, fs, blob, vol=-7 * 256)
    b = context(flavor, SB, fs, blob, vol=-7 * 256)
    a1 = run(a, da, depth, B, 0, n)
    b1 = run(b, db, depth, B, 0, nb)
    wa, _ = a.stream_positions(0, S)
    wb, rb = b.stream_positions(0, SB)
    assert set(wa.tolist()) == {n * B} and set(wb.tolist()) == {nb * B}
    head, state = a.export_streams(0, S)
    assert b.import_streams(t0, head, state, realign=True) == S
    w, r = b.stream_positions(0, SB)
    assert set(w.tolist()) == {nb * B} and np.array_equal(r, np.full(SB, rb[0]))
    mixed = packets(db, depth, B, nb, nb + n)
    mixed[t0:t0 + S] = packets(da, depth, B, n, 2 * n)
    b2 = run(b, mixed, depth, B, 0, n)
    assert b.launch_plan()["latency_layout"] > 0 and b.launch_plan()["packed_shared"] == 0, b.launch_plan()
    for s in range(SB):
        tail = tuple(x[s] for x in b2)
        if t0 <= s < t0 + S: check(oracle(flavor, fs, blob, vol=-7 * 256), da[s - t0], depth, B, [part(a1, s - t0, 0, n), (n, 2 * n, tail, b.status(s))], f"imported stream {s - t0} -> {s}")
        else: check(oracle(flavor, fs, blob, vol=-7 * 256), db[s], depth, B, [part(b1, s, 0, nb), (nb, nb + n, tail, b.status(s))], f"resident stream {s}")
    a.close(); b.close()


@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("kind", ("per-lane-values", "one-stream"))
def test_per_stream_presets(flavor, kind):
    """The imported streams carry presets of their own.  per-lane-values: every stream of A and of B has its own preamp on one shared
    structure — the packed float kernel with per-lane values (Q28: the per-lane-image kernel).  one-stream: A's preset differs from B's in
    structure (other delays in samples), so the rows that hold both run the one-stream kernel.  The path is read from launch_plan()."""
    fs, B, depth, n, nb = 48000, 48, 16, 9, 4
    SA, SB, f0, t0, cnt = 150, 200, 20, 91, 70
    blob_a = WL.full_chain_blob(flavor)
    blob_b = blob_a if kind == "per-lane-values" else WL.full_chain_blob(flavor, max_delay_ms=7.0)
    preamp = lambda db: (W.REQ["SET_PREAMP"], 0, struct.pack("<f", db))
    own_a = {s: preamp(-9.0 + 0.05 * s) for s in range(SA)} if kind == "per-lane-values" else {}
    own_b = {s: preamp(-2.0 - 0.03 * s) for s in range(SB)} if kind == "per-lane-values" else {}
    da = WL.synth_pcm16(SA, (n + n) * B, fs)
    db = WL.synth_pcm16(SB, (nb + n) * B, fs, first_stream=1000)
    a, b = context(flavor, SA, fs, blob_a), context(flavor, SB, fs, blob_b)
    for d, own in ((a, own_a), (b, own_b)):
        for s, rq in own.items(): assert d.vendor_set(*rq, stream=s) == 0
    a1 = run(a, da, depth, B, 0, n)
    b1 = run(b, db, depth, B, 0, nb)
    head, state = a.export_streams(f0, cnt)
    assert b.import_streams(t0, head, state, realign=True) == cnt
    w, r = b.stream_positions(0, SB)
    assert set(w.tolist()) == {nb * B} and set(r.tolist()) == {nb * B}
    mixed = packets(db, depth, B, nb, nb + n)
    mixed[t0:t0 + cnt] = packets(da, depth, B, n, 2 * n)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n)
    plan = b.launch_plan()
    if kind == "one-stream" or not int(flavor): assert plan["one_stream_per_lane_images"] > 0, plan
    else: assert plan["packed_per_lane_values"] > 0, plan
    for s in range(SB):
        tail = tuple(x[s] for x in b2)
        if t0 <= s < t0 + cnt:
            k = s - t0 + f0
            setup = (lambda o, rq=own_a[k]: o.vendor_set(*rq)) if k in own_a else None
            check(oracle(flavor, fs, blob_a, setup=setup), da[k], depth, B, [part(a1, k, 0, n), (n, 2 * n, tail, b.status(s))], f"imported stream {k} -> {s}")
        else:
            setup = (lambda o, rq=own_b[s]: o.vendor_set(*rq)) if s in own_b else None
            check(oracle(flavor, fs, blob_b, setup=setup), db[s], depth, B, [part(b1, s, 0, nb), (nb, nb + n, tail, b.status(s))], f"resident stream {s}")
    a.close(); b.close()


# ---- 7. device buffers, asynchronous --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_device_buffers_asynchronous(flavor):
    """4096 streams, DSPI_MEM_DEVICE | DSPI_SNAP_REALIGN, the records in a torch tensor.  The import lands in the upper part of a destination
    of another age — from inside one row to the context's end, so the first touched row has residents and the others none — and
    dspi_process is enqueued behind it with no synchronisation in between: the targets are computed on the device, in stream order."""
    import torch
    fs, B, n, nb, S = 96000, 96, 3, 2, 4096
    blob = WL.full_chain_blob(flavor)
    base_a = WL.synth_pcm16(256, 2 * n * B, fs)
    base_b = WL.synth_pcm16(256, (nb + n) * B, fs, first_stream=5000)
    da, db = _tile_input(base_a, S), _tile_input(base_b, S)
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    R = b.tile_streams()
    t0 = 5 * R + 7
    cnt = S - t0
    a1 = run(a, da, 16, B, 0, n)
    b1 = run(b, db, 16, B, 0, nb)
    rec = a.snapshot_sizes(0, 1)[1]
    buf = torch.empty(cnt * rec // 4, dtype=torch.int32, device="cuda")
    head = a.export_streams_device(0, cnt, buf.data_ptr(), buf.numel() * 4)
    a.sync()                                  # the source is synced before the import reads the records (include/dspi.h)
    dev = torch.device("cuda", 0)
    n_out, n_ch, n_pairs = (9, 11, 4) if int(flavor) else (5, 7, 2)
    mixed = packets(db, 16, B, nb, nb + n)
    mixed[t0:] = packets(da, 16, B, n, 2 * n)[:cnt]
    pcm = torch.from_numpy(mixed).to(dev)
    pairs = torch.empty((S, n_pairs, n * B, 2), dtype=torch.int32, device=dev); sub = torch.empty((S, n * B), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, n_ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    assert b.import_streams_device(t0, head, buf.data_ptr(), buf.numel() * 4, realign=True) == cnt
    b.process_device(pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())      # no sync after the import
    b.sync()
    del buf
    a.close()
    w, r = b.stream_positions(0, S)
    L = line_len(flavor)
    want_w = np.full(S, (nb + n) * B % L); want_w[6 * R:] = 2 * n * B % L      # row 5 took its residents' age, the rows behind it have none: A's
    assert np.array_equal(w, want_w), np.flatnonzero(w != want_w)[:8].tolist()
    assert_rows_uniform(b, "after the import and the launch behind it")
    pairs, sub, peaks = pairs.cpu().numpy(), sub.cpu().numpy(), peaks.cpu().numpy().view(np.uint16)
    rng = np.random.default_rng(9)
    for s in sorted(set(int(v) for v in rng.integers(0, S, 32)) | {0, t0 - 1, t0, t0 + 1, 6 * R - 1, 6 * R, S - 1}):
        out = (pairs[s], sub[s], peaks[s])
        o = oracle(flavor, fs, blob)
        if s >= t0: hist = (da[s - t0], [(0, n), (n, 2 * n)], a1, s - t0)
        else: hist = (db[s], [(0, nb), (nb, nb + n)], b1, s)
        row, (first, second), o1, k = hist
        rp, rs, rk, _ = o.process(packets(row, 16, B, *first), first[1] - first[0], B, 16)
        assert np.array_equal(rp, o1[0][k]) and np.array_equal(rs, o1[1][k]) and np.array_equal(rk, o1[2][k]), f"stream {s} before the hand-over"
        rp, rs, rk, _ = o.process(packets(row, 16, B, *second), second[1] - second[0], B, 16)
        assert np.array_equal(rp, out[0]), f"stream {s}: pairs differ: {np.argwhere(rp != out[0])[:3].tolist()}"
        assert np.array_equal(rs, out[1]) and np.array_equal(rk, out[2]), f"stream {s}: sub or peaks differ"
        assert o.status() == b.status(s), f"stream {s}: status differs"
    b.close()


# ---- 8. pending operations and PDM ----------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_pending_preset_load_and_pdm(flavor):
    """A preset load made after A's last packet and before the export (it arms the mute and zeroes the delay lines: state operations pending
    on the image) takes effect at B's next packet under realign exactly as the oracle says — zeroed lines are zero however they are
    rotated, and the lines' new contents are written from the new position on —, and the PDM words of both halves are one PdmOracle's."""
    fs, B, depth, n, nb, S, SB, t0 = 48000, 48, 16, 12, 5, 85, 150, 31
    blob = WL.full_chain_blob(flavor)
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, fs, other); image = ref.save_slot(0); ref.close()
    request = lambda x: x.load_slot(image)
    da = WL.synth_pcm16(S, 2 * n * B, fs)
    db = WL.synth_pcm16(SB, (nb + n) * B, fs, first_stream=2000)
    a, b = context(flavor, S, fs, blob), context(flavor, SB, fs, blob)
    a1 = run(a, da, depth, B, 0, n)
    wa = a.pdm_host(a1[1])
    b1 = run(b, db, depth, B, 0, nb)
    wb1 = b.pdm_host(b1[1])
    assert request(a) == 0
    head, state = a.export_streams(0, S)
    assert b.import_streams(t0, head, state, realign=True) == S
    w, r = b.stream_positions(0, SB)
    assert set(w.tolist()) == {nb * B} and set(r.tolist()) == {nb * B}
    mixed = packets(db, depth, B, nb, nb + n)
    mixed[t0:t0 + S] = packets(da, depth, B, n, 2 * n)
    b2 = run(b, mixed, depth, B, 0, n)
    wb2 = b.pdm_host(b2[1])
    for s in range(SB):
        tail = tuple(x[s] for x in b2)
        po = PdmOracle()
        if t0 <= s < t0 + S:
            k = s - t0
            check(oracle(flavor, fs, blob), da[k], depth, B, [part(a1, k, 0, n), (n, 2 * n, tail, b.status(s))], f"imported stream {k} -> {s}", at={n: lambda o: request(o)})
            assert np.array_equal(po.run(a1[1][k]), wa[k]), f"PDM words before the hand-over, stream {k}"
        else:
            check(oracle(flavor, fs, blob), db[s], depth, B, [part(b1, s, 0, nb), (nb, nb + n, tail, b.status(s))], f"resident stream {s}")
            assert np.array_equal(po.run(b1[1][s]), wb1[s]), f"PDM words of resident stream {s}, first part"
        assert np.array_equal(po.run(b2[1][s]), wb2[s]), f"PDM words after the hand-over, stream {s}"
    a.close(); b.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_refusals(flavor):
    """dspi_export_streams refuses the flag; a bad range to dspi_realign_streams and a corrupt head under the flag return errors; the
    destination exports the same bytes before and after."""
    import ctypes as C
    fs, B, n, S = 48000, 48, 5, 150
    blob = WL.full_chain_blob(flavor)
    b = context(flavor, S, fs, blob)
    run(b, WL.synth_pcm16(S, n * B, fs), 16, B, 0, n)
    a = context(flavor, 40, fs, blob); run(a, WL.synth_pcm16(40, 3 * B, fs), 16, B, 0, 3)
    head, state = a.export_streams(0, 40)
    h0, s0 = b.export_streams(0, S)
    hb, sb = a.snapshot_sizes(0, 40)
    hbuf, sbuf = C.create_string_buffer(hb), C.create_string_buffer(sb)
    for flags in (host.SNAP_REALIGN, host.SNAP_REALIGN | host.MEM_DEVICE):
        assert a.L.dspi_export_streams(a.h, 0, 40, C.byref(host._Snapshot(C.addressof(hbuf), hb, C.addressof(sbuf), sb)), flags) == host.E_INVAL
    for first, count in ((0, 0), (S, 1), (S - 1, 2), (0, S + 1), (0xFFFFFFFF, 2)):
        with pytest.raises(DspiError) as e: b.realign_streams(first, count)
        assert e.value.code == host.E_INVAL, (first, count)
    flipped = bytearray(head); flipped[len(head) // 2] ^= 0x10
    for what, hd, st, first, code in (("flipped byte", bytes(flipped), state, 0, host.E_INVAL), ("head one byte short", head[:-1], state, 0, host.E_INVAL),
                                      ("state one record short", head, state[:-1], 0, host.E_SHORT), ("past n_streams", head, state, S - 39, host.E_INVAL),
                                      ("flipped header byte", bytes([head[0] ^ 1]) + head[1:], state, 0, host.E_INVAL)):
        with pytest.raises(DspiError) as e: b.import_streams(first, hd, st, realign=True)
        assert e.value.code == code, (what, str(e.value))
    assert b.image_count() == 1
    h1, s1 = b.export_streams(0, S)
    assert h1 == h0 and np.array_equal(s1, s0)
    # ... and the snapshot it refused in pieces is taken whole
    assert b.import_streams(S - 40, head, state, realign=True) == 40
    assert_rows_uniform(b, "after the import")
    a.close(); b.close()


# ---- 10. a short fuzz -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_fuzz(seed):
    """test_gpu_snapshot.py::test_fuzz with the flag, or with a plain import followed by dspi_realign_streams over a random range that holds
    the imported one: random flavour, presets, ranges, shifts, ages and packet lengths.  Replay one seed alone:
    DSPI_FUZZ_SEED0=<seed> DSPI_SNAPSHOT_FUZZ_SEEDS=1 pytest tests/test_gpu_realign.py -m gpu -k test_fuzz"""
    from test_gpu_fuzz import random_blob, RATES
    rng = np.random.default_rng(47000 + seed)
    flavor = (1, W.F32_FMA, 0)[int(rng.integers(0, 3))]
    fs, Bs = RATES[seed % 3]
    B = int(rng.choice(Bs)); depth = 16 if rng.random() < 0.5 else 24
    SA, SB = int(rng.choice([3, 70, 131, 300])), int(rng.choice([2, 64, 129, 260]))
    cnt = int(rng.integers(1, min(SA, SB) + 1))
    f0, t0 = int(rng.integers(0, SA - cnt + 1)), int(rng.integers(0, SB - cnt + 1))
    na, nb, n2 = int(rng.integers(1, 14)), int(rng.integers(0, 9)), int(rng.integers(2, 12))
    in_place = bool(rng.integers(0, 2))
    r_lo = int(rng.integers(0, t0 + 1)); r_hi = int(rng.integers(t0 + cnt, SB + 1))
    blob_a, blob_b = random_blob(rng, flavor, fs), random_blob(rng, flavor, fs)
    vol_a, vol_b = int(rng.choice([0, -5 * 256, -20 * 256])), int(rng.choice([0, -9 * 256]))
    print(f"realign fuzz seed {seed}: flavor {fid(flavor)} fs {fs} B {B} depth {depth} A {SA} streams x {na} packets, B {SB} x {nb}, [{f0}, {f0 + cnt}) -> {t0}, "
          f"{'plain, then realign [%d, %d)' % (r_lo, r_hi) if in_place else 'realigning import'}, then {n2} packets", flush=True)
    da = as_input(WL.synth_pcm16(SA, (na + n2) * B, fs, first_stream=int(rng.integers(0, 20))), depth)
    db = as_input(WL.synth_pcm16(SB, (nb + n2) * B, fs, first_stream=500 + int(rng.integers(0, 20))), depth)
    a, b = context(flavor, SA, fs, blob_a, vol_a), context(flavor, SB, fs, blob_b, vol_b)
    a1 = run(a, da, depth, B, 0, na)
    b1 = run(b, db, depth, B, 0, nb) if nb else None
    assert_rows_uniform(b, f"seed {seed}: before the import")      # (per row: a float context's odd last stream runs on the one-stream kernel and may stand elsewhere)
    wb0, rb0 = b.stream_positions(0, SB)
    head, state = a.export_streams(f0, cnt)
    assert b.import_streams(t0, head, state, realign=not in_place) == cnt
    if in_place: assert b.realign_streams(r_lo, r_hi - r_lo) == r_hi - r_lo
    # a row with a resident keeps B's positions; a row the written range covers whole (as far as B has it) takes A's: uniform either way
    assert_rows_uniform(b, f"seed {seed}")
    R = b.tile_streams()
    w, r = b.stream_positions(0, SB)
    lo, hi = (r_lo, r_hi) if in_place else (t0, t0 + cnt)
    for row in range((SB + R - 1) // R):
        if not (lo // R <= row <= (hi - 1) // R):      # a row the call does not touch keeps what it had
            assert np.array_equal(w[row * R:(row + 1) * R], wb0[row * R:(row + 1) * R]) and np.array_equal(r[row * R:(row + 1) * R], rb0[row * R:(row + 1) * R]), f"seed {seed}: untouched row {row}"
        elif row * R < lo or hi < min((row + 1) * R, SB):
            res = row * R if row * R < lo else hi      # the row's resident neighbour (dspi_snapshot.h snap_row_target)
            assert (w[row * R], r[row * R]) == (wb0[res], rb0[res]), f"seed {seed}: row {row} has a resident and left its positions"
    mixed = packets(db, depth, B, nb, nb + n2)
    mixed[t0:t0 + cnt] = packets(da, depth, B, na, na + n2)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n2)
    a2 = run(a, da, depth, B, na, na + n2)
    tail = lambda out, s, p0, p1, st: (p0, p1, tuple(v[s] for v in out), st)
    for k in sorted(set(int(v) for v in rng.integers(0, cnt, 6)) | {0, cnt - 1}):      # imported, and the same streams going on at the source
        for who, out, s, d in (("imported", b2, t0 + k, b), ("source", a2, f0 + k, a)):
            check(oracle(flavor, fs, blob_a, vol_a), da[f0 + k], depth, B, [part(a1, f0 + k, 0, na), tail(out, s, na, na + n2, d.status(s))], f"seed {seed}: {who} stream {f0 + k} -> {s}")
    for s in sorted(set(int(v) for v in rng.integers(0, SB, 6)) | {max(t0 - 1, 0), min(t0 + cnt, SB - 1)}):      # B's own, the range's neighbours among them
        if t0 <= s < t0 + cnt: continue
        check(oracle(flavor, fs, blob_b, vol_b), db[s], depth, B, ([part(b1, s, 0, nb)] if nb else []) + [tail(b2, s, nb, nb + n2, b.status(s))], f"seed {seed}: resident stream {s}")
    a.close(); b.close()
