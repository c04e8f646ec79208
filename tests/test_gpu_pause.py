"""Paused streams on the GPU (dspi_pause_streams / dspi_resume_streams / dspi_streams_paused, include/dspi.h): a stream that sits calls out
stands exactly still, and goes on afterwards exactly as a device that received no packet in between.  Every audio comparison is with the
oracle, never with another run of the library: an active stream's oracle gets all packets, a paused stream's oracle only the packets the
stream took part in, with the parameter requests issued at the same points between packets (Sched below keeps that record per stream).

    test_pause_run_resume_run    figures: none; 300 float / 200 Q28 streams (48-frame, 16-bit) and 299 / 199 (45-frame, 24-bit: the odd count's
                                 last stream is in the paused set)
    test_few_active_streams      the issue's 2 048-stream context is ALREADY on the latency layout on a 256-CU device (1 024 stream pairs = the
                                 size rule's limit of 4 pairs per CU), so "moves to the latency layout and back" cannot be seen there; the test
                                 runs that size as stated (latency layout before, during, after) and a 4 096-stream context beside it, where
                                 the move is real"""
import struct

import numpy as np
import pytest

from conftest import has_gpu
from orclib import Oracle, PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, VOL, as_input, check, context, fid, oracle, packets, _fuzz_seeds, _tile_input
from test_gpu_realign import RING, assert_rows_uniform, line_len

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]


class Sched:
    """A context and, per stream, the record of the calls it took part in.  run() makes one dspi_process call on host buffers: active streams
    get the next packets of their OWN input, paused slots random bytes; request() makes a parameter call and notes it, for every stream it
    addresses, at the stream's own position between packets; verify() replays each stream's record on a fresh oracle."""

    def __init__(self, d, flavor, fs, blob, data, depth, B, vol=VOL, statuses=True):
        self.d, self.flavor, self.fs, self.blob, self.data, self.depth, self.B, self.vol, self.statuses = d, flavor, fs, blob, data, depth, B, vol, statuses
        S = d.n_streams
        self.pos = np.zeros(S, dtype=np.int64)
        self.parts = [[] for _ in range(S)]
        self.hooks = [dict() for _ in range(S)]
        self.frozen = {}                    # paused stream -> (status bytes, clip flags) when it was paused
        self.rng = np.random.default_rng(1234)
        self.last_clip = np.zeros(S, dtype=np.uint16)

    def request(self, name, *args, stream=None, want=0):
        d, S = self.d, self.d.n_streams
        rc = getattr(d, name)(*args, stream=host.ALL if stream is None else stream)
        assert rc == want or rc is None or name == "set_volume", (name, rc)
        for s in (range(S) if stream is None else (stream,)):
            self.hooks[s].setdefault(int(self.pos[s]), []).append((name, args))

    def pause(self, first, count):
        was = self.d.streams_paused().astype(bool)
        assert self.d.pause_streams(first, count) == count
        for s in range(first, first + count):
            if not was[s]: self.frozen[s] = (self.d.status(s), int(self.last_clip[s]))

    def resume(self, first, count, as_is=False):
        assert self.d.resume_streams(first, count, as_is=as_is) == count
        for s in range(first, first + count): self.frozen.pop(s, None)

    def input(self, n):
        d, B, depth = self.d, self.B, self.depth
        S = d.n_streams
        paused = d.streams_paused().astype(bool)
        if depth == 16: pcm = self.rng.integers(-32768, 32768, (S, n * B, 2), dtype=np.int16)
        else: pcm = self.rng.integers(0, 256, (S, n * B * 6), dtype=np.uint8)
        for s in np.flatnonzero(~paused):
            pcm[s] = packets(self.data[s], depth, B, int(self.pos[s]), int(self.pos[s]) + n)
        return pcm, paused

    def record(self, n, paused, pairs, sub, peaks, clip, frozen_outputs=True):
        d = self.d
        for s in range(d.n_streams):
            if paused[s]:
                if frozen_outputs:
                    assert not pairs[s].any() and not sub[s].any() and not peaks[s].any(), f"paused stream {s}: its regions of the host buffers are not zero"
                status, was_clip = self.frozen[s]
                assert int(clip[s]) == was_clip, f"paused stream {s}: clip flags {int(clip[s]):#x}, {was_clip:#x} before the pause"
                if self.statuses: assert d.status(s) == status, f"paused stream {s}: status changed during the pause"
            else:
                p0 = int(self.pos[s])
                self.parts[s].append((p0, p0 + n, (pairs[s], sub[s], peaks[s], clip[s]), d.status(s) if self.statuses else None))
                self.pos[s] += n
        self.last_clip = clip

    def run(self, n, **kw):
        pcm, paused = self.input(n)
        pairs, sub, peaks = self.d.process_host(pcm, n, self.B, self.depth, clip=True, **kw)
        clip = self.d.last_clip.copy()
        self.record(n, paused, pairs, sub, peaks, clip)
        return pairs, sub, peaks, clip

    def verify(self, streams=None, what=""):
        for s in (range(self.d.n_streams) if streams is None else streams):
            o = oracle(self.flavor, self.fs, self.blob, self.vol)
            at = {p: (lambda o, rq=rq: [getattr(o, nm)(*a) for nm, a in rq]) for p, rq in self.hooks[s].items()}
            check(o, self.data[s], self.depth, self.B, self.parts[s], f"{what}stream {s}", at=at)
            o.close()


def mixed_set(S, R):
    """a whole row, even streams only, odd streams only, both streams of some lanes, a range across a row boundary — and the last stream of an odd count"""
    p = np.zeros(S, dtype=bool)
    p[R:2 * R] = True
    p[10:30:2] = True
    p[41:61:2] = True
    p[2 * R + 6:2 * R + 10] = True
    p[2 * R - 6:2 * R + 2] = True
    if S & 1: p[S - 1] = True
    return p


def runs_of(mask):
    """[(first, count)] of the True runs"""
    out, s, n = [], 0, len(mask)
    while s < n:
        if not mask[s]: s += 1; continue
        e = s
        while e < n and mask[e]: e += 1
        out.append((s, e - s)); s = e
    return out


def new_sched(flavor, S, fs, B, depth, packets_total, blob=None, vol=VOL, first_stream=0, statuses=True):
    blob = WL.full_chain_blob(flavor) if blob is None else blob
    data = as_input(WL.synth_pcm16(S, packets_total * B, fs, first_stream=first_stream), depth)
    return Sched(context(flavor, S, fs, blob, vol), flavor, fs, blob, data, depth, B, vol, statuses)


# ---- 1. pause, run, resume, run ------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("fs,B,depth,odd", [(48000, 48, 16, False), (44100, 45, 24, True)], ids=("48f-16bit", "45f-24bit-odd-count"))
def test_pause_run_resume_run(flavor, fs, B, depth, odd):
    S = (300 if int(flavor) else 200) - (1 if odd else 0)
    x = new_sched(flavor, S, fs, B, depth, 16)
    R = x.d.tile_streams()
    x.run(5)
    p = mixed_set(S, R)
    for first, count in runs_of(p): x.pause(first, count)
    assert np.array_equal(x.d.streams_paused().astype(bool), p)
    x.run(2); x.run(3)
    w, r = x.d.stream_positions(0, S)
    L = line_len(flavor)
    assert set(w[p].tolist()) == {5 * B % L} and set(w[~p].tolist()) == {10 * B % L}, "paused streams stand still while their rows advance"
    for first, count in runs_of(p): x.resume(first, count)
    assert not x.d.streams_paused().any()
    assert_rows_uniform(x.d, "after the default resume")
    x.run(5)
    x.verify()
    x.d.close()


# ---- 2. the plan follows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_the_plan_follows(flavor):
    R = 128 if int(flavor) else 64
    S = 4 * R
    x = new_sched(flavor, S, 48000, 48, 16, 8, statuses=False)
    key = "packed_shared" if int(flavor) else "q28_shared"
    x.run(1)
    assert x.d.launch_plan()[key] == 4 and sum(x.d.launch_plan().values()) == 4
    x.pause(R, 2 * R)                      # rows 1 and 2, whole
    x.run(1)
    assert x.d.launch_plan()[key] == 2 and sum(x.d.launch_plan().values()) == 2, x.d.launch_plan()
    x.pause(5, 1)                          # one stream of a lane: float -> a per-lane-image item beside the row's packed item
    x.run(1)
    plan = x.d.launch_plan()
    assert plan[key] == 2 and plan["one_stream_per_lane_images"] == (1 if int(flavor) else 0), plan
    x.pause(0, S)
    x.run(1)
    assert sum(x.d.launch_plan().values()) == 0, x.d.launch_plan()
    x.resume(0, S)
    x.run(2)
    assert x.d.launch_plan()[key] == 4 and sum(x.d.launch_plan().values()) == 4
    x.verify(sorted({0, 4, 5, R - 1, R, R + 1, 3 * R - 1, 3 * R, S - 1}))
    x.d.close()


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_everything_paused_is_no_audio(flavor):
    """A DSPI_BOOT_POPULATED_FLASH context whose every stream is paused: dspi_process returns OK, launches nothing, advances the S/PDIF block
    position, and does not make the devices "running": dspi_load_flash_dump afterwards is still the boot — every word from frame 0 is the
    oracle's booted from the dump (no preset-load mute, no zeroed lines)."""
    from test_flash_dump import make_slots
    fl = int(flavor)
    slots = make_slots(fl); occ = sum(1 << n for n in slots)
    dump = W.flash_dump(W.flash_directory(default_slot=4, last_active_slot=9, slot_occupied=occ, master_volume_db=-17.0), slots)
    fs, B, S, n = 48000, 48, 70, 10
    pcm = WL.synth_pcm16(S, n * B, fs)
    d = Dspi(flavor, S, device=0, populated_flash=True)
    assert d.pause_streams(0, S) == S
    junk = np.random.default_rng(3).integers(-32768, 32768, (S, 3 * B, 2), dtype=np.int16)
    pairs, sub, peaks = d.process_host(junk, 3, B, spdif=True)
    assert not pairs.any() and not sub.any() and not peaks.any()
    assert sum(d.launch_plan().values()) == 0 and d.spdif_block_pos() == 3 * B % 192
    assert d.resume_streams(0, S) == S
    assert d.load_flash_dump(dump) == 4
    assert d.set_rate(fs) == 0
    d.set_volume(-12 * 256)
    bp, bs, bk = d.process_host(pcm, n, B)
    for s in (0, 5, 64, S - 1):
        ob = Oracle(flavor, detmath=True, flash=dump)
        assert ob.boot_selection == 4 and ob.set_rate(fs) == 0
        ob.set_volume(-12 * 256)
        rp, rs, rk, _ = ob.process(pcm[s], n, B)
        assert np.array_equal(rp, bp[s]) and np.array_equal(rs, bs[s]) and np.array_equal(rk, bk[s]), f"boot path after an all-paused call, stream {s}"
        assert ob.status() == d.status(s)
        ob.close()
    d.close()


# ---- 3. what the caller finds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
def test_device_buffers_keep_their_bytes(flavor, tiled):
    """DSPI_MEM_DEVICE: buffers pre-filled with a sentinel keep it in every paused region of pairs, sub and peaks (tiled: the paused
    columns), and the active streams' words are the oracle's."""
    import torch
    fs, B, n = 48000, 48, 4
    S = 300 if int(flavor) else 200
    x = new_sched(flavor, S, fs, B, 16, 2 * n, statuses=False)
    d, R = x.d, x.d.tile_streams()
    x.run(n)
    p = mixed_set(S, R)
    for first, count in runs_of(p): x.pause(first, count)
    dev = torch.device("cuda", 0)
    nt, P, C_ = -(-S // R), d.P, d.C
    SENT = 0x5A5A5A5A
    pcm, paused = x.input(n)
    assert np.array_equal(paused, p)
    t_pcm = torch.from_numpy(pcm).to(dev)
    pairs = torch.full((nt, 2 * P, n * B, R) if tiled else (S, P, n * B, 2), SENT, dtype=torch.int32, device=dev)
    sub = torch.full((nt, n * B, R) if tiled else (S, n * B), SENT, dtype=torch.int32, device=dev)
    peaks = torch.full((S, n, C_), 0x5A5A, dtype=torch.int16, device=dev)
    clip = torch.full((S,), 0x5A5A, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    d.process_device(t_pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr(), tiled=tiled, clip_ptr=clip.data_ptr())
    d.sync()
    pairs, sub, peaks, clip = pairs.cpu().numpy(), sub.cpu().numpy(), peaks.cpu().numpy().view(np.uint16), clip.cpu().numpy().view(np.uint16)
    if tiled:
        full = np.zeros(nt * R, dtype=bool); full[:S] = p
        cols = full.reshape(nt, R)
        assert (pairs.transpose(0, 3, 1, 2)[cols] == SENT).all() and (sub.transpose(0, 2, 1)[cols] == SENT).all(), "a paused column was written"
        pairs, sub = d.untile(pairs, sub)
    assert (pairs[p] == SENT).all() and (sub[p] == SENT).all() and (peaks[p] == 0x5A5A).all(), "a paused stream's region was written"
    for s in np.flatnonzero(p): assert int(clip[s]) == x.frozen[int(s)][1] and d.status(int(s)) == x.frozen[int(s)][0]
    frozen = dict(x.frozen)
    x.record(n, paused, np.where(p[:, None, None, None], 0, pairs), np.where(p[:, None], 0, sub), np.where(p[:, None, None], 0, peaks), clip)
    assert frozen == x.frozen
    x.verify()
    d.close()


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("path", ("staged", "direct"))
def test_host_buffers_hold_zeros(flavor, path, monkeypatch):
    """host buffers pre-filled with a sentinel (process_host's `out`): paused regions come back as zeros on the staged path (DSPI_NO_DIRECT
    set) and on the direct path (unset, one packet per call); clip flags and status are the values before the pause"""
    if path == "staged": monkeypatch.setenv("DSPI_NO_DIRECT", "1")
    else: monkeypatch.delenv("DSPI_NO_DIRECT", raising=False)
    fs, B = 48000, 48
    S = 300 if int(flavor) else 200
    x = new_sched(flavor, S, fs, B, 16, 8)
    d, R = x.d, x.d.tile_streams()
    x.run(1); x.run(1)
    if path == "direct": assert d.direct_stats()["calls"] == 2
    else: assert d.direct_stats()["calls"] == 0
    p = mixed_set(S, R)
    for first, count in runs_of(p): x.pause(first, count)
    for _ in range(2):
        pcm, paused = x.input(1)
        pairs = np.full((S, d.P, B, 2), 0x5A5A5A5A, dtype=np.int32); sub = np.full((S, B), 0x5A5A5A5A, dtype=np.int32); peaks = np.full((S, 1, d.C), 0x5A5A, dtype=np.uint16)
        pairs, sub, peaks = d.process_host(pcm, 1, B, 16, out=(pairs, sub, peaks), clip=True)      # (pairs and sub in place; the peaks array is the call's own)
        x.record(1, paused, pairs, sub, peaks, d.last_clip.copy())
    if path == "direct": assert d.direct_stats()["calls"] == 4
    for first, count in runs_of(p): x.resume(first, count)
    x.run(1); x.run(1)
    x.verify()
    d.close()


# ---- 4. requests while paused ---------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("how", ("single", "broadcast"))
def test_requests_while_paused(flavor, how):
    """A band type change that resets a filter path, a preset-slot load (mute plus zeroed lines) and a volume change land on paused streams —
    one at a time, or as broadcasts that reach active and paused streams alike — between calls the paused streams sit out; their state
    operations are applied at the next commit, paused or not; after the resume every stream matches an oracle that received the requests
    between the same packets of ITS OWN input.  Broadcasts fold the images back (merge_images)."""
    fs, B = 48000, 48
    S = 150 if int(flavor) else 100
    x = new_sched(flavor, S, fs, B, 16, 24)
    d, R = x.d, x.d.tile_streams()
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, fs, other); image = ref.save_slot(0); ref.close()
    band = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    x.run(4)
    x.pause(20, 30); x.pause(R - 3, 10)
    x.run(2)
    targets = (None,) if how == "broadcast" else (21, 22, 47, R + 2)
    for t in targets: x.request("vendor_set", *band, stream=t)
    x.run(2)
    for t in targets: x.request("load_slot", image, -1, stream=t)
    x.run(1)
    for t in targets: x.request("set_volume", -7 * 256, stream=t)
    x.run(3)
    x.resume(0, S)
    assert_rows_uniform(d, "after the resume")
    x.run(6)
    if how == "broadcast": assert d.image_count() == 1
    else: assert d.image_count() == 5      # one image per addressed stream beside the shared one (single-stream calls ask for no fold-back pass)
    x.verify()
    d.close()


# ---- 5. positions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("as_is", (False, True), ids=("realigned", "as-is"))
def test_positions(flavor, as_is):
    """45-frame packets, five of them missed: the paused streams stand 225 words behind their rows (odd, not a multiple of four).  Row 0 has its
    lowest-numbered streams [0, 4) paused, and the first resume leaves 0 and 1 paused: the target is stream 4's positions, the next active
    one.  Row 1 is paused whole and resumed in two calls: the first takes the positions of its own first stream (nobody in the row is
    active), the second aligns to what the first made active."""
    fs, B, depth = 44100, 45, 16
    S = 300 if int(flavor) else 200
    x = new_sched(flavor, S, fs, B, depth, 20)
    d, R = x.d, x.d.tile_streams()
    L = line_len(flavor)
    x.run(3)
    x.pause(0, 4); x.pause(R, R); x.pause(2 * R + 9, 7)
    x.run(2); x.run(3)
    w, r = d.stream_positions(0, S)
    p = d.streams_paused().astype(bool)
    assert set(w[p].tolist()) == {3 * B} and set(r[p].tolist()) == {3 * B} and set(w[~p].tolist()) == {8 * B} and set(r[~p].tolist()) == {8 * B}
    assert (8 * B - 3 * B) % 4 == 1
    x.resume(2, 2, as_is); x.resume(R + 5, 20, as_is); x.resume(2 * R, min(R, S - 2 * R), as_is)      # (the last range holds residents)
    w, r = d.stream_positions(0, S)
    if as_is:
        assert set(w[p].tolist()) == {3 * B} and set(r[p].tolist()) == {3 * B}, "DSPI_RESUME_AS_IS keeps the stale positions"
    else:
        assert w[2] == w[3] == 8 * B and r[2] == r[3] == 8 * B and w[0] == w[1] == 3 * B, "row 0: the target is the next ACTIVE stream's"
        assert set(w[R:2 * R].tolist()) == {3 * B}, "row 1: nobody active, the first resumed stream's positions"
        assert set(w[2 * R:min(3 * R, S)].tolist()) == {8 * B}
    x.run(2)
    x.resume(0, S, as_is)
    w, r = d.stream_positions(0, S)
    if as_is: assert set(w[:R].tolist()) == {3 * B, 5 * B, 10 * B} and set(w[R:2 * R].tolist()) == {3 * B, 5 * B}, "as-is: every stream keeps the positions its own packets gave it"
    else:
        assert_rows_uniform(d, "after the second resume")
        assert w[0] == 10 * B % L and w[R] == 5 * B % L
    x.run(6)
    if not as_is: assert_rows_uniform(d, "after the continuation")
    x.verify()
    d.close()


# ---- 6. every kernel family -----------------------------------------------------------------------------------------------------------------
def _shape_blob(flavor, shape):
    from test_gpu_parity import _latency_blob
    if shape == 1: return _latency_blob()
    b = WL.full_chain_blob(flavor)
    if shape == 2: b["leveller"]["enabled"] = 0
    return b


@pytest.mark.parametrize("flavor", (1, W.F32_FMA), ids=fid)
@pytest.mark.parametrize("shape", (1, 2, 3))
def test_latency_layout_shapes(flavor, shape, monkeypatch):
    """small contexts on the float latency layout, all three shapes: one of a lane's two streams paused (first and second), and one whole
    workgroup part paused (8 stream pairs in shape 1, 2 in shapes 2 and 3)"""
    monkeypatch.delenv("DSPI_F32_LAYOUT", raising=False)
    fs, B, S = 48000, 48, 40
    x = new_sched(flavor, S, fs, B, 16, 14, blob=_shape_blob(flavor, shape), vol=-7 * 256)
    d = x.d
    ppw = 8 if shape == 1 else 2
    x.run(3)
    before = d.launch_plan()
    assert before["latency_layout"] == -(-S // (2 * ppw)) and before["latency_layout_paired"] == 0 and sum(before.values()) == before["latency_layout"], before
    x.pause(2, 1); x.pause(7, 1); x.pause(2 * ppw, 2 * ppw)      # a first stream, a second stream, part 1 whole
    x.run(2); x.run(2)
    plan = d.launch_plan()
    assert plan["latency_layout"] == before["latency_layout"] - 1 and sum(plan.values()) == plan["latency_layout"], plan
    x.resume(0, S)
    x.run(4)
    assert d.launch_plan() == before
    x.verify()
    d.close()


@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("kind", ("per-lane-values", "several-structures"))
def test_per_stream_presets(flavor, kind):
    """per-lane-values: every stream its own preamp on one structure — float: the packed kernel with per-lane values, with holes (single
    streams of lanes, whole lanes, the row's first stream); Q28: per-lane rows.  several-structures: every third stream on a preset of
    another structure, so rows run the one-stream kernel beside the packed one; pausing all streams of the second structure in row 0 leaves
    that row with one structure."""
    fs, B = 48000, 48
    S = 200 if int(flavor) else 100
    x = new_sched(flavor, S, fs, B, 16, 14)
    d, R = x.d, x.d.tile_streams()
    if kind == "per-lane-values":
        for s in range(S): x.request("vendor_set", W.REQ["SET_PREAMP"], 0, struct.pack("<f", -9.0 + 0.05 * s), stream=s)
    else:
        blob_b = WL.full_chain_blob(flavor, max_delay_ms=7.0)
        for s in range(0, S, 3): x.request("load_bulk", blob_b, stream=s)
    x.run(3)
    plan0 = d.launch_plan()
    if not int(flavor): assert plan0["one_stream_per_lane_images"] > 0, plan0
    elif kind == "per-lane-values": assert plan0["packed_per_lane_values"] == 2 and plan0["one_stream_per_lane_images"] == 0, plan0
    else: assert plan0["one_stream_per_lane_images"] > 0 and plan0["packed_shared"] > 0, plan0
    if kind == "per-lane-values": x.pause(0, 1); x.pause(9, 1); x.pause(20, 4); x.pause(R - 1, 3)
    else:
        for s in range(0, R, 3): x.pause(s, 1)
        x.pause(R + 1, 1)
    x.run(2); x.run(2)
    plan = d.launch_plan()
    if int(flavor) and kind == "per-lane-values": assert plan["packed_per_lane_values"] == 2 and plan["one_stream_per_lane_images"] > 0, plan
    if not int(flavor) and kind == "several-structures": assert plan["q28_shared"] == 1 and plan["one_stream_per_lane_images"] == plan0["one_stream_per_lane_images"] - 1, plan
    x.resume(0, S)
    x.run(4)
    assert d.launch_plan() == plan0
    x.verify()
    d.close()


@pytest.mark.parametrize("flavor", (1, W.F32_FMA), ids=fid)
def test_value_tile_mask_comes_from_the_active_streams(flavor):
    """pv_build_kernel with the activity bitmap: row 0 is a per-lane-value row whose ACTIVE streams differ in band 3 of the left master channel
    (every third stream has its own), while its first stream — paused, so the mask's reference is the next active one — differs from all of
    them in band 5, as does paused stream 7.  During the pause the row stays on the packed kernel with per-lane band coefficients, and every
    stream is its oracle's before, during and after."""
    fs, B, S = 48000, 48, 200
    x = new_sched(flavor, S, fs, B, 16, 12)
    d = x.d
    eq = lambda band, f, g: (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, band, W.FILTER_PEAKING, 0, f, 1.1, g))
    x.request("vendor_set", *eq(3, 700.0, 2.0)); x.request("vendor_set", *eq(5, 2500.0, -2.0))      # one structure for everybody
    for s in range(1, 128, 3): x.request("vendor_set", *eq(3, 700.0 + 5.0 * s, 2.5), stream=s)
    for s in (0, 7): x.request("vendor_set", *eq(5, 3100.0 + s, -4.0), stream=s)
    x.run(3)
    assert d.launch_plan()["packed_per_lane_values_and_bands"] == 1, d.launch_plan()
    x.pause(0, 1); x.pause(7, 1)
    x.run(2); x.run(2)
    plan = d.launch_plan()
    assert plan["packed_per_lane_values_and_bands"] == 1 and plan["one_stream_per_lane_images"] > 0, plan      # (the paused streams' lane mates)
    x.resume(0, S)
    x.run(3)
    x.verify()
    d.close()


@pytest.mark.parametrize("layout", ("lat", "chain"))
def test_q28_wave_layouts(layout, monkeypatch):
    monkeypatch.setenv("DSPI_Q28_LAYOUT", layout)
    x = new_sched(0, 100, 44100, 45, 16, 12)
    x.run(3)
    x.pause(3, 5); x.pause(60, 10); x.pause(99, 1)
    x.run(2); x.run(1)
    x.resume(0, 100)
    x.run(4)
    x.verify()
    x.d.close()


@pytest.mark.auto_layout
@pytest.mark.parametrize("S", (2048, 4096))
def test_few_active_streams(S):
    """paused down to 16 active streams (one per row of the first sixteen rows) the context runs on the latency layout; resumed it is back where
    it was: the packed kernel at 4 096 streams; at 2 048 the size rule has the whole context on the latency layout to begin with (see the
    module's docstring)"""
    flavor, fs, B = W.F32_FMA, 48000, 48
    base = WL.synth_pcm16(64, 9 * B, fs)
    x = Sched(context(flavor, S, fs, WL.full_chain_blob(flavor)), flavor, fs, WL.full_chain_blob(flavor), _tile_input(base, S), 16, B, statuses=False)
    d, R = x.d, x.d.tile_streams()
    x.run(2)
    plan0 = d.launch_plan()
    if S == 4096: assert plan0["packed_shared"] == S // R and plan0["latency_layout"] == 0, plan0
    else: assert plan0["latency_layout"] == S // 4 and plan0["packed_shared"] == 0, plan0
    x.pause(0, S)
    keep = [row * R + 2 * row + (row & 1) for row in range(16)]
    for s in keep: x.resume(s, 1)
    x.run(2); x.run(1)
    plan = d.launch_plan()
    assert plan["latency_layout"] == 16 and sum(v for k, v in plan.items() if k != "latency_layout_paired") == 16, plan
    x.resume(0, S)
    assert_rows_uniform(d, "after the resume")
    x.run(3)
    assert d.launch_plan() == plan0
    x.verify(sorted(set(keep) | {0, 1, R, S - 3 * R + 5, S - 1}))
    d.close()


# ---- 7. PDM ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
def test_pdm(flavor, tiled):
    """dspi_pdm_modulate before, during and after a pause against one PdmOracle per stream fed the frames of the calls the stream took part
    in; a paused stream's words are zero in host buffers"""
    fs, B, n = 48000, 48, 2
    S = 150 if int(flavor) else 100
    x = new_sched(flavor, S, fs, B, 16, 8, statuses=False)
    d, R = x.d, x.d.tile_streams()
    nt = -(-S // R)
    pdm = [PdmOracle() for _ in range(S)]

    def modulate(sub, paused):
        if tiled:
            t = np.zeros((nt * R, sub.shape[1]), dtype=np.int32); t[:S] = sub
            words = d.pdm_host(np.ascontiguousarray(t.reshape(nt, R, -1).transpose(0, 2, 1)), tiled=True)      # [tile][frame][8][R]
            words = words.transpose(0, 3, 1, 2).reshape(nt * R, sub.shape[1], 8)[:S]
        else: words = d.pdm_host(sub)
        for s in range(S):
            if paused[s]: assert not words[s].any(), f"paused stream {s}: PDM words written"
            else: assert np.array_equal(pdm[s].run(sub[s]), words[s]), f"PDM words of stream {s}"

    nobody = np.zeros(S, dtype=bool)
    modulate(x.run(n)[1], nobody)
    x.pause(5, 3); x.pause(R - 2, 6); x.pause(S - 1, 1)
    p = d.streams_paused().astype(bool)
    junk = np.random.default_rng(5).integers(-2**28, 2**28, (S, n * B), dtype=np.int32)
    for _ in range(2):
        sub = x.run(n)[1]
        modulate(np.where(p[:, None], junk, sub), p)      # (a paused stream's slot of `sub` is not read either)
    x.resume(0, S)
    modulate(x.run(n)[1], nobody)
    x.verify(sorted({0, 5, 6, R - 2, R, R + 3, S - 1}))
    d.close()


# ---- 8. DSPI_OUT_SPDIF ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,layout", [(W.F32_FMA, "packed"), (W.F32_FMA, "skew"), (0, "packed")], ids=("fma-two-pass", "fma-fused", "q28-two-pass"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_spdif(flavor, layout, mem, monkeypatch):
    """DSPI_OUT_SPDIF with paused streams on the two-pass path (packed kernel, Q28) and on the latency layout's fused encoder: the active
    streams' subframes are the oracle's pair words through the S/PDIF restatement (orclib.spdif_encode) at the context's running block
    position; paused regions are zeros (host) / untouched (device)."""
    import orclib
    monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    fs, B, n = 48000, 48, 3
    S = 150 if int(flavor) else 100
    x = new_sched(flavor, S, fs, B, 16, 4 * n, statuses=False)
    d, R = x.d, x.d.tile_streams()
    x.run(n)
    x.pause(4, 3); x.pause(R - 2, 6); x.pause(S - 1, 1)
    p = d.streams_paused().astype(bool)
    frames = n * B
    got = []
    for call in range(2):
        pos = d.spdif_block_pos()
        pcm, paused = x.input(n)
        if mem == "host":
            pairs, sub, peaks = d.process_host(pcm, n, B, 16, spdif=True, clip=True)
            clip = d.last_clip.copy()
            assert not pairs[p].any()
        else:
            import torch
            dev = torch.device("cuda", 0)
            t_pcm = torch.from_numpy(pcm).to(dev)
            t_pairs = torch.full((S, d.P, frames, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            t_sub = torch.zeros((S, frames), dtype=torch.int32, device=dev); t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
            t_clip = torch.zeros((S,), dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            d.process_device(t_pcm.data_ptr(), n, B, 16, t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), spdif=True, clip_ptr=t_clip.data_ptr())
            d.sync()
            pairs, sub = t_pairs.cpu().numpy().view(np.uint32), t_sub.cpu().numpy()
            peaks, clip = t_peaks.cpu().numpy().view(np.uint16), t_clip.cpu().numpy().view(np.uint16)
            assert (pairs[p] == 0x5A5A5A5A).all(), "a paused stream's subframes were written"
        plan = d.launch_plan()
        assert (plan["latency_layout"] > 0 and plan["packed_shared"] == 0) if layout == "skew" else plan["latency_layout"] == 0, plan
        assert d.spdif_block_pos() == (pos + frames) % 192
        got.append((pos, pairs))
        # the oracle produces pair WORDS: the record keeps none for this call (checked through the subframes below), sub / peaks / clip as usual
        for s in np.flatnonzero(~p):
            if s % 7 and s not in (3, 7, R - 3, R + 4): continue      # (every seventh active stream and the pauses' neighbours: the oracle's whole history each)
            o = oracle(flavor, fs, x.blob)
            at = int(x.pos[s])
            rp, rs, rk, _ = o.process(packets(x.data[s], 16, B, 0, at + n), at + n, B, 16)
            o.close()
            for pr in range(d.P):
                want, nxt = orclib.spdif_encode(np.ascontiguousarray(rp[pr, at * B:]), pos, fs)
                assert nxt == (pos + frames) % 192 and np.array_equal(want, pairs[s][pr]), f"call {call}: subframes of stream {s}, pair {pr} differ"
            assert np.array_equal(rs[at * B:], sub[s]) and np.array_equal(rk[at:], peaks[s])
        x.pos[~p] += n
    d.close()


# ---- 9. snapshots ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_snapshots(flavor):
    """A stream's record exported while paused equals, byte for byte, its record exported just before the pause.  Activity does not travel: the
    record goes into a PAUSED slot of another context, which stays paused through two calls, and into an active one; after the resume both
    continue exactly."""
    fs, B, n = 48000, 48, 4
    S = 150 if int(flavor) else 100
    x = new_sched(flavor, S, fs, B, 16, 16)
    d = x.d
    x.run(n)
    src = (11, 12, 40)
    before = {s: d.export_streams(s, 1) for s in src}
    for s in src: x.pause(s, 1)
    x.run(2); x.run(1)
    for s in src:
        head, state = d.export_streams(s, 1)
        assert head == before[s][0] and np.array_equal(state, before[s][1]), f"the record of paused stream {s} changed"
    y = new_sched(flavor, S, fs, B, 16, 16, first_stream=500)
    y.run(2)
    y.pause(70, 2)
    y.run(1)
    # 11 -> y's paused slot 70, 12 -> y's active slot 3: their inputs and histories move with them
    for s, t in ((11, 70), (12, 3)):
        assert y.d.import_streams(t, *before[s]) == 1
        y.data[t] = x.data[s]; y.parts[t] = list(x.parts[s]); y.hooks[t] = dict(x.hooks[s]); y.pos[t] = x.pos[s]
    y.frozen[70] = x.frozen[11]
    assert y.d.streams_paused().tolist() == [1 if s in (70, 71) else 0 for s in range(S)]
    y.run(2); y.run(1)
    y.resume(0, S)
    y.run(3)
    y.verify(sorted({0, 2, 3, 4, 69, 70, 71, 72, S - 1}), what="importer ")
    x.resume(0, S)
    x.run(3)
    x.verify(sorted({10, 11, 12, 13, 40, 41}), what="source ")
    d.close(); y.d.close()


# ---- 10. fuzz -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.auto_layout
@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_fuzz(seed, monkeypatch):
    """A random schedule of pauses, resumes (default / as-is), requests and calls on a random preset, flavour, layout, packet length and bit
    depth, all streams against their oracles.  Replay one seed alone:
    DSPI_FUZZ_SEED0=<seed> DSPI_SNAPSHOT_FUZZ_SEEDS=1 pytest tests/test_gpu_pause.py -m gpu -k test_fuzz"""
    from test_gpu_fuzz import random_blob, RATES
    rng = np.random.default_rng(83000 + seed)
    flavor = (1, W.F32_FMA, 0)[int(rng.integers(0, 3))]
    layout = ("packed", "skew", None)[int(rng.integers(0, 3))]
    if layout: monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    fs, Bs = RATES[seed % 3]
    B = int(rng.choice(Bs)); depth = 16 if rng.random() < 0.5 else 24
    S = int(rng.choice([1, 2, 3, 37, 70, 131, 200]))
    blob = random_blob(rng, flavor, fs)
    vol = int(rng.choice([0, -5 * 256, -20 * 256]))
    steps = int(rng.integers(4, 9))
    print(f"pause fuzz seed {seed}: flavor {fid(flavor)} layout {layout} fs {fs} B {B} depth {depth} S {S}, {steps} steps", flush=True)
    data = as_input(WL.synth_pcm16(S, 40 * B, fs, first_stream=int(rng.integers(0, 20))), depth)
    x = Sched(context(flavor, S, fs, blob, vol), flavor, fs, blob, data, depth, B, vol, statuses=S <= 70)
    x.run(int(rng.integers(1, 4)))
    for _ in range(steps):
        what = rng.choice(["pause", "pause", "resume", "resume-as-is", "request", "request-all", "run"])
        first = int(rng.integers(0, S)); count = int(rng.integers(1, S - first + 1))
        if rng.random() < 0.5: count = min(count, int(rng.integers(1, 6)))
        if what == "pause": x.pause(first, count)
        elif what == "resume": x.resume(first, count)
        elif what == "resume-as-is": x.resume(first, count, as_is=True)
        elif what in ("request", "request-all"):
            t = None if what == "request-all" else first
            k = int(rng.integers(0, 3))
            if k == 0: x.request("set_volume", int(rng.choice([0, -3 * 256, -12 * 256])), stream=t)
            elif k == 1: x.request("vendor_set", W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, int(rng.integers(0, 10)), W.FILTER_PEAKING, 0, float(rng.uniform(100, 8000)), 1.0, float(rng.uniform(-6, 6))), stream=t)
            else: x.request("vendor_set", W.REQ["SET_PREAMP"], 0, struct.pack("<f", float(rng.uniform(-12, 0))), stream=t)
        x.run(int(rng.integers(1, 4)))
    x.resume(0, S)
    x.run(int(rng.integers(1, 4)))
    streams = range(S) if S <= 70 else sorted(set(int(v) for v in rng.integers(0, S, 24)) | {0, S - 1})
    x.verify(streams, what=f"seed {seed}: ")
    x.d.close()


# ---- 11. full size --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,S", [(W.F32_FMA, 65536), (0, 16384)], ids=("fma-65536", "q28-16384"))
def test_full_size(flavor, S):
    """Device buffers at the benchmark's sizes: the upper half of the rows paused for three launches, then resumed; 32 sampled streams across
    both halves against the oracle, and the paused half's tiled columns untouched."""
    import torch
    fs, B, n = 96000 if int(flavor) else 48000, 96 if int(flavor) else 48, 2
    blob = WL.full_chain_blob(flavor)
    base = WL.synth_pcm16(256, 6 * n * B, fs)
    d = context(flavor, S, fs, blob)
    R, P, C_ = d.tile_streams(), d.P, d.C
    nt = S // R
    dev = torch.device("cuda", 0)
    pcm = [torch.from_numpy(_tile_input(np.ascontiguousarray(base[:, k * n * B:(k + 1) * n * B]), S)).to(dev) for k in range(6)]
    junk = torch.from_numpy(np.random.default_rng(2).integers(-32768, 32768, (S // 2, n * B, 2), dtype=np.int16)).to(dev)
    SENT = 0x5A5A5A5A
    pairs = torch.full((nt, 2 * P, n * B, R), SENT, dtype=torch.int32, device=dev); sub = torch.full((nt, n * B, R), SENT, dtype=torch.int32, device=dev)
    peaks = torch.full((S, n, C_), 0x5A5A, dtype=torch.int16, device=dev)
    rng = np.random.default_rng(11)
    sample = sorted(set(int(v) for v in rng.integers(0, S // 2, 16)) | set(int(v) for v in rng.integers(S // 2, S, 16)) | {0, S // 2 - 1, S // 2, S - 1})
    lane, tile = [s % R for s in sample], [s // R for s in sample]
    got = {s: [] for s in sample}

    def call(k_low, k_high, paused_high):
        x = pcm[k_low].clone()
        x[S // 2:] = junk if paused_high else pcm[k_high][S // 2:]
        pairs.fill_(SENT); sub.fill_(SENT); peaks.fill_(0x5A5A)
        torch.cuda.synchronize()
        d.process_device(x.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr(), tiled=True)
        d.sync()
        pw = pairs[tile, :, :, lane].cpu().numpy(); sw = sub[tile, :, lane].cpu().numpy(); kw = peaks[sample].cpu().numpy().view(np.uint16)
        if paused_high:
            assert bool((pairs[nt // 2:] == SENT).all()) and bool((sub[nt // 2:] == SENT).all()) and bool((peaks[S // 2:] == 0x5A5A).all()), "the paused half was written"
        for i, s in enumerate(sample):
            if paused_high and s >= S // 2: continue
            got[s].append((pw[i].reshape(P, 2, n * B).transpose(0, 2, 1), sw[i], kw[i]))

    call(0, 0, False)
    assert d.pause_streams(S // 2, S // 2) == S // 2
    for k in (1, 2, 3): call(k, 0, True)
    plan = d.launch_plan()
    assert sum(plan.values()) == nt // 2, plan
    assert d.resume_streams(S // 2, S // 2) == S // 2
    call(4, 1, False); call(5, 2, False)
    assert sum(d.launch_plan().values()) == nt
    assert_rows_uniform(d, "after the resume")
    for s in sample:
        o = oracle(flavor, fs, blob)
        ks = (0, 1, 2, 3, 4, 5) if s < S // 2 else (0, 1, 2)
        assert len(got[s]) == len(ks)
        for k, (gp, gs, gk) in zip(ks, got[s]):
            rp, rs, rk, _ = o.process(np.ascontiguousarray(base[s % 256, k * n * B:(k + 1) * n * B]), n, B, 16)
            assert np.array_equal(rp, gp) and np.array_equal(rs, gs) and np.array_equal(rk, gk), f"stream {s}, its call {k}"
        assert o.status() == d.status(s)
        o.close()
    d.close()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_refusals(flavor):
    S = 150
    x = new_sched(flavor, S, 48000, 48, 16, 6, statuses=False)
    d = x.d
    x.run(1)
    x.pause(10, 20)
    want = d.streams_paused().copy()
    for first, count in ((0, 0), (S, 1), (S - 1, 2), (0, S + 1), (0xFFFFFFFF, 2)):
        with pytest.raises(DspiError) as e: d.pause_streams(first, count)
        assert e.value.code == host.E_INVAL, (first, count)
        with pytest.raises(DspiError) as e: d.resume_streams(first, count)
        assert e.value.code == host.E_INVAL, (first, count)
        assert d.L.dspi_streams_paused(d.h, first, count, None) == host.E_INVAL
    for bad in (0x2, 0x3, 0x100, 0x80000000):
        assert d.L.dspi_resume_streams(d.h, 0, S, bad) == host.E_INVAL, hex(bad)
    assert np.array_equal(d.streams_paused(), want)
    x.run(2)
    x.resume(0, S)
    x.run(2)
    x.verify(sorted({0, 9, 10, 29, 30, S - 1}))
    d.close()
