"""Stream snapshots on the GPU (dspi_export_streams / dspi_import_streams, include/dspi.h): a stream exported after packet k and
imported anywhere else continues from packet k + 1 with exactly the words of an uninterrupted run.  Every comparison is with the
oracle fed the whole input — pair words, sub words, per-packet peaks, status bytes, clip flags — never with another run of the library."""
import os
import struct

import numpy as np
import pytest

from conftest import has_gpu
from orclib import Oracle, PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS_WITH_KERNEL = (1, W.F32_FMA, 0)
VOL = -20 * 256


def fid(flavor):
    return "q28" if not int(flavor) else "fma" if getattr(flavor, "fma", False) else "f32"


def as_input(pcm, depth):
    return pcm if depth == 16 else WL.pcm16_to_pcm24_bytes(pcm)


def packets(data, depth, B, p0, p1):
    """packets [p0, p1) of int16 [S][frames][2] or of packed 24-bit bytes [S][frames * 6] (also of one stream's row)"""
    unit = B if depth == 16 else B * 6
    return np.ascontiguousarray(data[..., p0 * unit:p1 * unit, :] if depth == 16 else data[..., p0 * unit:p1 * unit])


def context(flavor, S, fs, blob, vol=VOL):
    d = Dspi(flavor, S, device=0)
    assert d.set_rate(fs) == 0
    d.set_volume(vol)
    assert d.load_bulk(blob) == 0
    return d


def oracle(flavor, fs, blob, vol=VOL, setup=None):
    o = Oracle(flavor, detmath=True)
    assert o.set_rate(fs) == 0
    o.set_volume(vol)
    assert o.load_bulk(blob) == 0
    if setup: setup(o)
    return o


def run(d, data, depth, B, p0, p1):
    """(pairs, sub, peaks, clip flags) of packets [p0, p1)"""
    pairs, sub, peaks = d.process_host(packets(data, depth, B, p0, p1), p1 - p0, B, depth, clip=True)
    return pairs, sub, peaks, d.last_clip.copy()


def check(o, row, depth, B, parts, what, at=None):
    """One stream against its oracle.  row: the stream's whole input; parts: [(p0, p1, (pairs, sub, peaks, clip) of the stream's row in that call,
    status bytes after it or None)] in time order; at: {packet: hook(oracle)} requests made at a packet boundary."""
    for p0, p1, (pairs, sub, peaks, clip), status in parts:
        if at and p0 in at: at[p0](o)
        rp, rs, rk, rclip = o.process(packets(row, depth, B, p0, p1), p1 - p0, B, depth)
        assert np.array_equal(rp, pairs), f"{what}: pairs differ in packets [{p0}, {p1}): {np.argwhere(rp != pairs)[:3].tolist()}"
        assert np.array_equal(rs, sub), f"{what}: sub differs in packets [{p0}, {p1})"
        assert np.array_equal(rk, peaks), f"{what}: peaks differ in packets [{p0}, {p1})"
        assert int(clip) == rclip == int.from_bytes(o.status()[-2:], "little"), f"{what}: clip flags differ after packet {p1}"
        if status is not None: assert o.status() == status, f"{what}: status differs after packet {p1}"


def part(out, s, p0, p1, status=None):
    return (p0, p1, (out[0][s], out[1][s], out[2][s], out[3][s]), status)


def hand_over(a, b, first, count, to):
    head, state = a.export_streams(first, count)
    assert state.shape[0] == count and state.nbytes == a.snapshot_sizes(first, count)[1] and len(head) == a.snapshot_sizes(first, count)[0]
    assert b.import_streams(to, head, state) == count
    return head, state


# ---- 1. continuation, 2. the source is unchanged --------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("fs,B,depth", [(96000, 96, 16), (48000, 48, 24), (44100, 45, 16)])
def test_continuation(flavor, fs, B, depth):
    """A runs 12 packets, every stream goes to a FRESH context (factory defaults, another rate, no volume: the parameters travel) that
    runs 12 more: the 24 packets are the oracle's."""
    S, n = 85, 12
    blob = WL.full_chain_blob(flavor)
    data = as_input(WL.synth_pcm16(S, 2 * n * B, fs), depth)
    a = context(flavor, S, fs, blob)
    o1 = run(a, data, depth, B, 0, n)
    b = Dspi(flavor, S, device=0)
    assert b.set_rate(44100 if fs != 44100 else 48000) == 0
    hand_over(a, b, 0, S, 0)
    o2 = run(b, data, depth, B, n, 2 * n)
    assert b.image_count() == 1
    for s in range(S):
        check(oracle(flavor, fs, blob), data[s], depth, B, [part(o1, s, 0, n, a.status(s)), part(o2, s, n, 2 * n, b.status(s))], f"stream {s}")
    a.close(); b.close()


@pytest.mark.parametrize("flavor", (1, W.F32_FMA), ids=fid)
@pytest.mark.parametrize("fs,B,depth", [(96000, 96, 16), (48000, 48, 24), (44100, 45, 16)])
def test_continuation_latency_layout_preset(flavor, fs, B, depth, monkeypatch):
    """... on the latency layout's own preset class (master PEQ, delays at the edge values): there the EQ state lives in registers during
    a launch and must have gone back to the state array before the export reads it."""
    from test_gpu_parity import _latency_blob
    monkeypatch.setenv("DSPI_F32_LAYOUT", "skew")
    S, n = 37, 12
    blob = _latency_blob()
    data = as_input(WL.synth_pcm16(S, 2 * n * B, fs), depth)
    a = context(flavor, S, fs, blob, vol=-7 * 256)
    o1 = run(a, data, depth, B, 0, n)
    b = Dspi(flavor, S + 6, device=0)
    hand_over(a, b, 0, S, 3)      # (an odd shift: every stream changes its side of a stream pair)
    pad = np.zeros((3,) + data.shape[1:], dtype=data.dtype)
    o2 = run(b, np.concatenate([pad, data, pad]), depth, B, n, 2 * n)
    for d in (a, b): assert d.launch_plan()["latency_layout"] > 0 and d.launch_plan()["packed_shared"] == 0, d.launch_plan()
    for s in range(S):
        check(oracle(flavor, fs, blob, vol=-7 * 256), data[s], depth, B, [part(o1, s, 0, n), part(o2, s + 3, n, 2 * n, b.status(s + 3))], f"stream {s}")
    a.close(); b.close()


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_the_source_is_unchanged(flavor):
    """A goes on for the same 12 packets after the export and equals the oracle too (and so does the importer)."""
    fs, B, depth, S, n = 96000, 96, 16, 85, 12
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, 2 * n * B, fs)
    a = context(flavor, S, fs, blob)
    o1 = run(a, data, depth, B, 0, n)
    b = Dspi(flavor, S, device=0)
    hand_over(a, b, 0, S, 0)
    o2a = run(a, data, depth, B, n, 2 * n)
    o2b = run(b, data, depth, B, n, 2 * n)
    assert a.image_count() == 1
    for s in range(S):
        check(oracle(flavor, fs, blob), data[s], depth, B, [part(o1, s, 0, n), part(o2a, s, n, 2 * n, a.status(s))], f"source stream {s}")
        check(oracle(flavor, fs, blob), data[s], depth, B, [part(o1, s, 0, n), part(o2b, s, n, 2 * n, b.status(s))], f"importer stream {s}")
    a.close(); b.close()


# ---- 3. relocation beside foreign streams ---------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_relocation_beside_foreign_streams(flavor):
    """Streams [100, 170) of A (300 streams) go to [91, 161) of B (200 streams on another preset, after another number of frames with
    delays and the leveller active: other delay write indices, other ring positions).  An odd shift — every float stream changes its side
    of a packed lane — across the row boundary at stream 128 in both contexts and flavours.  Afterwards every one of B's 200 streams is
    its own oracle's: the 70 imported ones A's continued, the other 130 their own history."""
    fs, B, depth, n, nb = 48000, 48, 16, 12, 7
    blob_a = WL.full_chain_blob(flavor)
    blob_b = WL.full_chain_blob(flavor, max_delay_ms=7.0)
    blob_b["preamp"]["preamp_db"][:] = (-1.0, -5.0)
    blob_b["leveller"]["speed"] = 2
    SA, SB, f0, t0, cnt = 300, 200, 100, 91, 70
    da = WL.synth_pcm16(SA, 2 * n * B, fs)
    db = WL.synth_pcm16(SB, (nb + n) * B, fs, first_stream=1000)
    a = context(flavor, SA, fs, blob_a)
    b = context(flavor, SB, fs, blob_b, vol=-11 * 256)
    a1 = run(a, da, depth, B, 0, n)
    b1 = run(b, db, depth, B, 0, nb)
    hand_over(a, b, f0, cnt, t0)
    assert b.image_count() == 2
    # B's next 12 packets: rows [91, 161) carry A's input from packet 12 on, the others B's own from packet 7 on
    mixed = packets(db, depth, B, nb, nb + n)
    mixed[t0:t0 + cnt] = packets(da, depth, B, n, 2 * n)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n)
    for s in range(SB):
        if t0 <= s < t0 + cnt:
            k = s - t0 + f0
            row = da[k]
            check(oracle(flavor, fs, blob_a), row, depth, B, [part(a1, k, 0, n), (n, 2 * n, (b2[0][s], b2[1][s], b2[2][s], b2[3][s]), b.status(s))], f"imported stream {k} -> {s}")
        else:
            check(oracle(flavor, fs, blob_b, vol=-11 * 256), db[s], depth, B, [part(b1, s, 0, nb), (nb, nb + n, (b2[0][s], b2[1][s], b2[2][s], b2[3][s]), b.status(s))], f"resident stream {s}")
    a.close(); b.close()


# ---- 4. images ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_images_travel_and_fold_back(flavor):
    """The exported range mixes streams on the shared preset with streams that were given a band or a gain of their own; the destination
    already holds the shared preset: it ends with one image per distinct parameter set (the shared one folded back), and every imported
    stream reads back the source's parameters and goes on like its oracle."""
    fs, B, depth, n, S = 48000, 48, 16, 6, 150
    blob = WL.full_chain_blob(flavor)
    R = W.REQ
    own = {10: (R["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_PEAKING, 0, 900.0, 2.0, -5.0)),
           20: (R["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 3, 1, W.FILTER_LOWSHELF, 0, 200.0, 0.8, 4.0)),
           30: (R["SET_PREAMP"], 0, struct.pack("<f", -7.5)),
           40: (R["SET_PREAMP"], 0, struct.pack("<f", -1.25)), 41: (R["SET_PREAMP"], 0, struct.pack("<f", -1.25)),      # two streams, one parameter set
           120: (R["SET_PREAMP"], 0, struct.pack("<f", 2.0))}                                                        # outside the exported range
    data = WL.synth_pcm16(S, 2 * n * B, fs)
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    for s, (req, wv, pl) in own.items(): assert a.vendor_set(req, wv, pl, stream=s) == 0
    a1 = run(a, data, depth, B, 0, n)
    b1 = run(b, data, depth, B, 0, n)
    f0, cnt, t0 = 0, 100, 20
    head, _ = hand_over(a, b, f0, cnt, t0)
    assert b.image_count() == 5      # shared + streams 10, 20, 30 + the set of 40 and 41
    assert len(head) == a.snapshot_sizes(f0, cnt)[0] and a.snapshot_sizes(f0, cnt)[0] > a.snapshot_sizes(50, cnt)[0]
    for k in range(cnt):
        assert b.collect_bulk(t0 + k) == a.collect_bulk(f0 + k), k
    mixed = packets(data, depth, B, n, 2 * n)
    mixed[t0:t0 + cnt] = packets(data, depth, B, n, 2 * n)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n)
    assert b.image_count() == 5
    for k in (0, 9, 10, 11, 20, 30, 40, 41, 42, 99):
        s = t0 + k
        setup = (lambda o, rq=own[k]: o.vendor_set(*rq)) if k in own else None
        check(oracle(flavor, fs, blob, setup=setup), data[k], depth, B, [part(a1, k, 0, n), (n, 2 * n, tuple(x[s] for x in b2), b.status(s))], f"imported stream {k} -> {s}")
    for s in (0, 19, 120, 149):      # residents (120: B's stream 120 never left the shared preset)
        check(oracle(flavor, fs, blob), data[s], depth, B, [part(b1, s, 0, n), (n, 2 * n, tuple(x[s] for x in b2), b.status(s))], f"resident stream {s}")
    a.close(); b.close()


# ---- 5. pending operations travel ------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("kind", ("band", "preset"))
def test_pending_operations_travel(flavor, kind):
    """A request with a side effect on run-time state — a band redesign that resets the band's state; a preset load that arms the mute and
    zeroes the delay lines — made after A's last packet and before the export takes effect at B's next packet, exactly as it would have
    at A's: the oracle gets the same request at the same packet boundary."""
    fs, B, depth, n, S = 48000, 48, 16, 12, 85
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, 2 * n * B, fs)
    if kind == "band":
        rq = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 1, 4, W.FILTER_HIGHSHELF, 0, 3000.0, 0.9, -6.0))
        request = lambda x: x.vendor_set(*rq)
    else:
        other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
        other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
        ref = oracle(flavor, fs, other); image = ref.save_slot(0); ref.close()
        request = lambda x: x.load_slot(image)
    a = context(flavor, S, fs, blob)
    a1 = run(a, data, depth, B, 0, n)
    assert request(a) == 0
    b = Dspi(flavor, S + 1, device=0)
    hand_over(a, b, 0, S, 1)
    pad = np.zeros((1,) + data.shape[1:], dtype=data.dtype)
    b2 = run(b, np.concatenate([pad, data]), depth, B, n, 2 * n)
    for s in range(S):
        check(oracle(flavor, fs, blob), data[s], depth, B, [part(a1, s, 0, n), part(b2, s + 1, n, 2 * n, b.status(s + 1))], f"stream {s}",
              at={n: lambda o: request(o)})
    a.close(); b.close()


# ---- 6. PDM ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("used", (True, False), ids=("modulator-used", "modulator-never-used"))
def test_pdm_state_travels(flavor, used):
    """The PDM modulator's words go along: the PDM words of both halves equal one PdmOracle per stream run over the whole sub signal.  A
    source that never ran the modulator hands over power-on modulators, also into a context whose own had been running."""
    fs, B, n = 48000, 48, 10
    S = 150 if int(flavor) else 90
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, 2 * n * B, fs)
    a = context(flavor, S, fs, blob)
    a1 = run(a, data, 16, B, 0, n)
    w1 = a.pdm_host(a1[1]) if used else None
    b = Dspi(flavor, S + 5, device=0)
    if not used: b.pdm_host(np.full((S + 5, 64), 12345678, dtype=np.int32))      # B's modulators have a history of their own
    hand_over(a, b, 0, S, 5)
    pad = np.zeros((5,) + data.shape[1:], dtype=data.dtype)
    b2 = run(b, np.concatenate([pad, data]), 16, B, n, 2 * n)
    w2 = b.pdm_host(b2[1])
    for s in range(S):
        check(oracle(flavor, fs, blob), data[s], 16, B, [part(a1, s, 0, n), part(b2, s + 5, n, 2 * n)], f"stream {s}")
        o = PdmOracle()
        if used: assert np.array_equal(o.run(a1[1][s]), w1[s]), f"PDM words before the hand-over, stream {s}"
        assert np.array_equal(o.run(b2[1][s + 5]), w2[s + 5]), f"PDM words after the hand-over, stream {s}"
    a.close(); b.close()


# ---- 7. refusals leave the destination alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_refusals_leave_the_destination_alone(flavor):
    fs, B, n, S = 48000, 48, 8, 70
    blob = WL.full_chain_blob(flavor)
    data = WL.synth_pcm16(S, 2 * n * B, fs)
    b = context(flavor, S, fs, blob)
    b1 = run(b, data, 16, B, 0, n)
    a = context(flavor, 40, fs, blob); run(a, data[:40], 16, B, 0, 3)
    head, state = a.export_streams(0, 40)
    # float into Q28 / Q28 into float; canonical into FMA
    others = [0 if int(flavor) else 1] + ([1] if int(flavor) else [])
    for of in others:
        x = context(of, 40, fs, WL.full_chain_blob(of)); run(x, data[:40], 16, B, 0, 2)
        oh, os_ = x.export_streams(0, 40)
        with pytest.raises(DspiError) as e: b.import_streams(0, oh, os_)
        assert e.value.code == host.E_INVAL and ("flavour" in str(e.value) or "contract" in str(e.value)), str(e.value)
        x.close()
    flipped = bytearray(head); flipped[len(head) // 2] ^= 0x10
    for what, hd, st, first, code in (("flipped byte", bytes(flipped), state, 0, host.E_INVAL), ("head one byte short", head[:-1], state, 0, host.E_INVAL),
                                      ("state one record short", head, state[:-1], 0, host.E_SHORT), ("past n_streams", head, state, S - 39, host.E_INVAL),
                                      ("flipped header byte", bytes([head[0] ^ 1]) + head[1:], state, 0, host.E_INVAL)):
        with pytest.raises(DspiError) as e: b.import_streams(first, hd, st)
        assert e.value.code == code, (what, str(e.value))
    assert b.image_count() == 1
    b2 = run(b, data, 16, B, n, 2 * n)
    for s in range(S):
        check(oracle(flavor, fs, blob), data[s], 16, B, [part(b1, s, 0, n), part(b2, s, n, 2 * n, b.status(s))], f"stream {s}")
    # ... and the snapshot it refused in pieces is taken whole
    assert b.import_streams(S - 40, head, state) == 40
    a.close(); b.close()


# ---- 8. device buffers at size ------------------------------------------------------------------------------------------------------------
def _tile_input(base, S):
    return np.ascontiguousarray(np.broadcast_to(base[None], (S // base.shape[0],) + base.shape).reshape((S,) + base.shape[1:]))


def _device_hand_over(a, b, S, chunk, buf):
    for first in range(0, S, chunk):
        cnt = min(chunk, S - first)
        head = a.export_streams_device(first, cnt, buf.data_ptr(), buf.numel() * 4)
        a.sync()                                  # B's stream does not wait for A's
        assert b.import_streams_device(first, head, buf.data_ptr(), buf.numel() * 4) == cnt
        b.sync()                                  # ... and the buffer is reused


@pytest.mark.parametrize("flavor,S,chunk_bytes", [(W.F32_FMA, 4096, None), (0, 4096, None), (W.F32_FMA, 65536, 1 << 30)], ids=("f32-4096", "q28-4096", "f32-65536-chunked"))
def test_device_buffers_at_size(flavor, S, chunk_bytes):
    """DSPI_MEM_DEVICE: the records in a torch tensor, A to B device to device with the dspi_sync in between; 32 seeded streams against the
    oracle over the continuation.  The full float context (10.3 GB of state) goes through one 1 GB buffer in chunks of whole rows."""
    import torch
    fs, B, n = 96000, 96, 3
    blob = WL.full_chain_blob(flavor)
    base = WL.synth_pcm16(256, 2 * n * B, fs)
    data = _tile_input(base, S)
    a = context(flavor, S, fs, blob)
    a1 = run(a, data, 16, B, 0, n)
    rec = a.snapshot_sizes(0, 1)[1]
    assert a.snapshot_sizes(0, S)[1] == S * rec
    chunk = S if chunk_bytes is None else (chunk_bytes // rec) // a.tile_streams() * a.tile_streams()
    assert 0 < chunk <= S
    buf = torch.empty(chunk * rec // 4, dtype=torch.int32, device="cuda")
    b = Dspi(flavor, S, device=0)
    _device_hand_over(a, b, S, chunk, buf)
    del buf
    a.close()
    b2 = run(b, data, 16, B, n, 2 * n)
    assert b.image_count() == 1
    rng = np.random.default_rng(8)
    for s in sorted(set(int(x) for x in rng.integers(0, S, 32)) | {0, S - 1, chunk - 1, chunk % S}):
        check(oracle(flavor, fs, blob), data[s], 16, B, [part(a1, s, 0, n), part(b2, s, n, 2 * n, b.status(s))], f"stream {s}")
    b.close()


# ---- 9. seeded fuzz --------------------------------------------------------------------------------------------------------------------
def _fuzz_seeds():
    s0 = int(os.environ.get("DSPI_FUZZ_SEED0", 0))
    return range(s0, s0 + int(os.environ.get("DSPI_SNAPSHOT_FUZZ_SEEDS", 40)))


@pytest.mark.both_layouts
@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_fuzz(seed):
    """Random flavour, presets from the parity fuzzer's generator, split point, range, shift and destination size.  Replay one seed alone:
    DSPI_FUZZ_SEED0=<seed> DSPI_SNAPSHOT_FUZZ_SEEDS=1 pytest tests/test_gpu_snapshot.py -m gpu -k test_fuzz"""
    from test_gpu_fuzz import random_blob, RATES
    rng = np.random.default_rng(31000 + seed)
    flavor = (1, W.F32_FMA, 0)[int(rng.integers(0, 3))]
    fs, Bs = RATES[seed % 3]
    B = int(rng.choice(Bs)); depth = 16 if rng.random() < 0.5 else 24
    SA, SB = int(rng.choice([3, 70, 131, 300])), int(rng.choice([2, 64, 129, 260]))
    cnt = int(rng.integers(1, min(SA, SB) + 1))
    f0, t0 = int(rng.integers(0, SA - cnt + 1)), int(rng.integers(0, SB - cnt + 1))
    na, nb, n2 = int(rng.integers(1, 14)), int(rng.integers(0, 9)), int(rng.integers(2, 12))
    blob_a, blob_b = random_blob(rng, flavor, fs), random_blob(rng, flavor, fs)
    vol_a, vol_b = int(rng.choice([0, -5 * 256, -20 * 256])), int(rng.choice([0, -9 * 256]))
    print(f"snapshot fuzz seed {seed}: flavor {fid(flavor)} fs {fs} B {B} depth {depth} A {SA} streams x {na} packets, B {SB} x {nb}, [{f0}, {f0 + cnt}) -> {t0}, then {n2} packets", flush=True)
    da = as_input(WL.synth_pcm16(SA, (na + n2) * B, fs, first_stream=int(rng.integers(0, 20))), depth)
    db = as_input(WL.synth_pcm16(SB, (nb + n2) * B, fs, first_stream=500 + int(rng.integers(0, 20))), depth)
    a, b = context(flavor, SA, fs, blob_a, vol_a), context(flavor, SB, fs, blob_b, vol_b)
    a1 = run(a, da, depth, B, 0, na)
    b1 = run(b, db, depth, B, 0, nb) if nb else None
    hand_over(a, b, f0, cnt, t0)
    mixed = packets(db, depth, B, nb, nb + n2)
    mixed[t0:t0 + cnt] = packets(da, depth, B, na, na + n2)[f0:f0 + cnt]
    b2 = run(b, mixed, depth, B, 0, n2)
    a2 = run(a, da, depth, B, na, na + n2)
    tail = lambda out, s, p0, p1, st: (p0, p1, tuple(x[s] for x in out), st)
    for k in sorted(set(int(x) for x in rng.integers(0, cnt, 6)) | {0, cnt - 1}):      # imported, and the same streams going on at the source
        for who, out, s, d in (("imported", b2, t0 + k, b), ("source", a2, f0 + k, a)):
            check(oracle(flavor, fs, blob_a, vol_a), da[f0 + k], depth, B, [part(a1, f0 + k, 0, na), tail(out, s, na, na + n2, d.status(s))], f"seed {seed}: {who} stream {f0 + k} -> {s}")
    for s in sorted(set(int(x) for x in rng.integers(0, SB, 6)) | {max(t0 - 1, 0), min(t0 + cnt, SB - 1)}):      # B's own, the range's neighbours among them
        if t0 <= s < t0 + cnt: continue
        check(oracle(flavor, fs, blob_b, vol_b), db[s], depth, B, ([part(b1, s, 0, nb)] if nb else []) + [tail(b2, s, nb, nb + n2, b.status(s))], f"seed {seed}: resident stream {s}")
    a.close(); b.close()
