"""Resizing on the GPU (dspi_resize_streams / dspi_reserve_streams / dspi_stream_capacity, include/dspi.h): a context gains slots that are
devices that have just been powered on, gives paused slots back, and its other streams do not notice — whether the arrays were
reallocated under them or not.  Every audio comparison is with the oracle, one oracle per stream, never with another run of the library.
ResizeSched below is test_gpu_boot.py's schedule record (BootSched) for a context whose size changes: a grown slot is a "booted" slot with
a fresh oracle from ITS packet 0, on input of its own; a cut slot's record is dropped.

    figures: none.  48 kHz, 48-frame packets, the full chain (delays and leveller on), at most 12 packets per stream.  Sizes are the
    smallest at which rows, lanes and padding columns can go wrong: 70 -> 100 stays in its row for both row widths (R = 128 float, 64 Q28),
    the next sizes are the first to open a new row and the first to leave a row holding one stream (130 and 257 float, 130 and 193 Q28);
    the layout test alone needs 4 352 streams, a size that the latency layout's size rule (1 024 stream pairs on a 256-CU device) does not take."""
import numpy as np
import pytest

from conftest import has_gpu
from orclib import PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, VOL, as_input, context, fid
from test_gpu_realign import assert_rows_uniform
from test_gpu_pause import mixed_set, runs_of, _shape_blob
from test_gpu_move import relocate, streams_of
from test_gpu_boot import BootSched, v2_dump
from test_gpu_spdif_pos import assert_streams, expect, warm

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48


def row_of(flavor):
    return 128 if int(flavor) else 64


def rows_of(n, R):
    return -(-n // R)


class ResizeSched(BootSched):
    """BootSched whose context changes its size.  The per-slot records are kept for `room` slots from the start (every slot has input of
    its own); grow() makes the new slots booted slots at their packet 0, shrink() drops the cut slots' records."""

    def __init__(self, *a, room, **kw):
        super().__init__(*a, **kw)
        S = self.d.n_streams
        self.pos = np.zeros(room, dtype=np.int64)
        self.parts += [[] for _ in range(room - S)]
        self.hooks += [dict() for _ in range(room - S)]
        o = self.fresh(None); self.power_on = o.status(); o.close()

    def grow(self, n, paused=False, check_status=8):
        d, old = self.d, self.d.n_streams
        was = d.streams_paused().astype(bool)
        assert d.resize_streams(n, paused=paused) == n == d.n_streams == int(d.L.dspi_num_streams(d.h))
        now = d.streams_paused().astype(bool)
        assert np.array_equal(now[:old], was) and (now[old:] == paused).all(), "old slots keep their activity, new slots are active / arrive paused"
        self.last_clip = np.concatenate([self.last_clip, np.zeros(n - old, dtype=np.uint16)])
        for s in range(old, n):
            self.booted[s] = None
            self.parts[s] = []; self.hooks[s] = {}; self.pos[s] = 0
            if paused: self.frozen[s] = (self.power_on, 0)
        for s in sorted({old, n - 1} | set(np.linspace(old, n - 1, check_status).astype(int).tolist())):
            assert d.status(s) == self.power_on, f"new slot {s}: status bytes are not the power-on ones"

    def shrink(self, n):
        d, old = self.d, self.d.n_streams
        was = d.streams_paused().astype(bool)
        assert d.resize_streams(n) == n == d.n_streams
        assert np.array_equal(d.streams_paused().astype(bool), was[:n])
        self.last_clip = self.last_clip[:n].copy()
        for s in range(n, old):
            self.parts[s] = []; self.hooks[s] = {}; self.pos[s] = 0
            self.frozen.pop(s, None); self.booted.pop(s, None)

    def move(self, moves, as_is=False):
        moves = [(int(s), int(t)) for s, t in moves]
        applied = [(s, t) for s, t in moves if s != t]
        assert self.d.move_streams(moves, as_is=as_is) == len(applied)
        relocate(self, moves)
        was = dict(self.booted)      # how a slot was booted travels with the stream
        for s, t in applied:
            if s in was: self.booted[t] = was[s]
            else: self.booted.pop(t, None)


def new_resize_sched(flavor, S, room, packets_total, blob=None, vol=VOL, statuses=True):
    blob = WL.full_chain_blob(flavor) if blob is None else blob
    data = as_input(WL.synth_pcm16(room, packets_total * B, FS), 16)
    return ResizeSched(context(flavor, S, FS, blob, vol), flavor, FS, blob, data, 16, B, vol, statuses, room=room)


def fresh_record(flavor):
    f = Dspi(flavor, 1, device=0)
    try: return f.export_streams(0, 1)[1][0]
    finally: f.close()


def assert_new_records(d, old, before, fresh, position, what):
    """after a grow from `old`: every old slot's record is its record before the call, every new slot's the fresh one-stream context's,
    byte for byte — but for the two write-position words of the new slots in the row that was grown where that row has an active
    resident: they are the row's (`position`; None: the row has no resident, the slots keep the power-on positions)"""
    n, R = d.n_streams, d.tile_streams()
    after = d.export_streams(0, n)[1]
    assert np.array_equal(after[:old], before), f"{what}: an old slot's record changed"
    w, r = d.stream_positions(0, n)
    for s in range(old, n):
        diff = np.flatnonzero(after[s] != fresh)
        if position and old % R and s // R == (old - 1) // R:
            assert len(diff) == 2 and set(after[s][diff].tolist()) == {position} and (w[s], r[s]) == (position, position), f"{what}: new slot {s}: words {diff.tolist()[:8]} are not power-on words"
        else:
            assert len(diff) == 0 and (w[s], r[s]) == (0, 0), f"{what}: new slot {s}: {len(diff)} words are not power-on words"
    return after


def grow_sizes(R):
    """from 70: the same row; the first size with a new row (and two streams in it); the first after that with a row holding one stream"""
    n2 = rows_of(100, R) * R + 2
    return 100, n2, rows_of(n2, R) * R + 1


# ---- 1. bytes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("reserved", (False, True), ids=("capacity-is-use", "reserved"))
def test_bytes(flavor, reserved):
    R = row_of(flavor)
    sizes = grow_sizes(R)
    assert sizes == ((100, 130, 257) if R == 128 else (100, 130, 193))
    room = max(3 * R, rows_of(sizes[-1], R) * R)
    x = new_resize_sched(flavor, 70, sizes[-1], 6, statuses=False)
    d = x.d
    assert d.stream_capacity() == rows_of(70, R) * R
    if reserved: assert d.reserve_streams(room) == room
    d.pdm_host(x.run(6)[1])                               # the modulator words are not power-on words any more
    fresh = fresh_record(flavor)
    before = d.export_streams(0, 70)[1]
    assert not np.array_equal(before[0], fresh)
    for n, position in zip(sizes, (6 * B, 6 * B, 0)):      # (the third grows a row whose residents arrived with the second: they stand at 0)
        old = d.n_streams
        x.grow(n)
        assert d.stream_capacity() == (room if reserved else rows_of(n, R) * R), "reserved: the grows change no allocation; else every row crossing reallocates to exactly the rows needed"
        before = assert_new_records(d, old, before, fresh, position, f"{old} -> {n}")
    d.close()


# ---- 2. running on --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_running_on(flavor):
    S, R = streams_of(flavor), row_of(flavor)
    n = S + R + 30
    x = new_resize_sched(flavor, S, n, 12)
    d = x.d
    x.run(5)
    x.grow(n)
    new_row = rows_of(S, R) * R
    w, r = d.stream_positions(0, n)
    assert (w[S], r[S]) == (5 * B, 5 * B) and (w[new_row - 1], r[new_row - 1]) == (5 * B, 5 * B), "a new slot in the old partial row takes the row's positions"
    assert (w[new_row], r[new_row]) == (0, 0) and (w[n - 1], r[n - 1]) == (0, 0), "a slot in a whole new row has the power-on positions"
    assert_rows_uniform(d, "after the grow")
    x.enumerate(range(S, n), blob_on=(S, S + 1, new_row - 1, new_row, new_row + 5, n - 1))
    x.run(3); x.run(2)
    # every row still on one delay write index; the leveller ring only turns in lanes whose leveller runs (the arrivals with the blob), so
    # its position is compared there: an arrival with the blob stands where its row's old residents stand
    w, r = d.stream_positions(0, n)
    for row in range(rows_of(n, R)): assert len(set(w[row * R:(row + 1) * R].tolist())) == 1, f"after the continuation: row {row} holds write indices {sorted(set(w[row * R:(row + 1) * R].tolist()))}"
    assert w[S] == w[0] == 10 * B and w[new_row] == 5 * B
    assert r[S] == r[S + 1] == r[new_row - 1] == r[S - 1] == 10 * B and r[new_row] == r[new_row + 5] == r[n - 1] == 5 * B
    for s in range(S, n): assert x.pos[s] == 5
    x.verify()
    d.close()


# ---- 3. arriving paused ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_arriving_paused(flavor):
    R = row_of(flavor)
    n = rows_of(70, R) * R + 10                          # into the grown row and a new one
    x = new_resize_sched(flavor, 70, n, 12)
    d = x.d
    dump, code = v2_dump(flavor)
    x.run(3)
    x.grow(n, paused=True)
    x.run(1)                                             # they sit this one out (run() checks: zero outputs, power-on status)
    some = [70, 71, n - 3, n - 1]
    x.boot(some, dump, want=code)
    x.enumerate(some, blob_on=some[:2])
    for s in some: x.resume(s, 1)
    x.run(2); x.run(2)
    paused = d.streams_paused().astype(bool)
    for s in range(70, n):
        assert paused[s] == (s not in some)
        assert x.pos[s] == (4 if s in some else 0)
        if s not in some: assert d.status(s) == x.power_on, f"paused arrival {s} does not report power-on status"
    x.verify()
    d.close()


# ---- 4. shrinking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_shrinking(flavor):
    S = streams_of(flavor)
    x = new_resize_sched(flavor, S, S, 12)
    d, R = x.d, x.d.tile_streams()
    x.run(3)
    x.pause(70, S - 71)                                  # the top but for its last slot
    before, cap = d.export_streams(0, S)[1], d.stream_capacity()
    with pytest.raises(DspiError) as e: d.resize_streams(70)
    assert e.value.code == host.E_INVAL and d.n_streams == S == int(d.L.dspi_num_streams(d.h)) and d.stream_capacity() == cap
    assert np.array_equal(d.export_streams(0, S)[1], before), "a refused shrink changed a record"
    x.pause(S - 1, 1)
    old_size = x.input(1)[0]
    x.shrink(70)
    assert d.stream_capacity() == cap, "shrinking keeps the capacity"
    with pytest.raises(AssertionError): d.process_host(old_size, 1, B)      # (buffers are sized by dspi_num_streams: the old size is the wrong size now)
    x.run(2)                                             # host buffers of the new size; the cut columns are padding of row 0 / 1 now
    x.pause(1, 69)
    x.shrink(1)
    x.run(2)
    assert d.stream_capacity() == cap
    # the cut columns ran audio for five packets: a grow writes power-on state into them whatever they hold
    fresh = fresh_record(flavor)
    one = d.export_streams(0, 1)[1]
    x.grow(70)
    assert_new_records(d, 1, one, fresh, 7 * B, "1 -> 70 over dirty columns")
    x.enumerate(range(1, 70), blob_on=(1, 2, 69))
    x.run(2)
    x.verify()
    d.close()


# ---- 5. the compaction recipe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_compaction_recipe(flavor):
    S = streams_of(flavor)
    x = new_resize_sched(flavor, S, S, 12)
    d, R = x.d, x.d.tile_streams()
    key = "packed_shared" if int(flavor) else "q28_shared"
    x.run(3)
    for first, count in runs_of(mixed_set(S, R)): x.pause(first, count)
    x.run(1)
    scattered = d.launch_plan()
    if int(flavor): assert scattered["one_stream_per_lane_images"] > 0, scattered
    x.move(d.plan_compaction(one_way=True))
    A = int((~d.streams_paused().astype(bool)).sum())
    assert A < S - R and not d.streams_paused()[:A].any() and d.streams_paused()[A:].all()
    x.shrink(A)
    assert d.stream_capacity() == rows_of(S, R) * R
    assert d.reserve_streams(A) == rows_of(A, R) * R == d.stream_capacity(), "the capacity has fallen to rows(A) x R"
    x.run(2); x.run(1)
    plan = d.launch_plan()
    assert plan[key] == rows_of(A, R) and plan["one_stream_per_lane_images"] <= (A % 2 if int(flavor) else 0), plan
    assert plan["packed_per_lane_values"] == plan["packed_per_lane_values_and_bands"] == plan["latency_layout"] == 0, plan
    x.verify()
    d.close()


# ---- 6. parameters across a reallocation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_parameters_across_a_reallocation(flavor):
    import struct
    from test_gpu_snapshot import oracle
    R = row_of(flavor)
    n = rows_of(70, R) * R + 10                          # a new row: capacity is use, so the arrays are reallocated
    x = new_resize_sched(flavor, 70, n, 12)
    d = x.d
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, FS, other); image = ref.save_slot(0); ref.close()
    band = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    band2 = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 1, 2, W.FILTER_LOWSHELF, 0, 450.0, 0.7, -2.0))
    x.run(2)
    x.request("load_bulk", other, stream=9)               # a preset of its own ...
    x.run(1)
    images = d.image_count()
    assert images == 2
    x.request("load_slot", image, -1, stream=9)           # ... with requests pending on it: a preset-slot load (mute, zeroed lines) and
    x.request("vendor_set", *band, stream=9)              # a band change that resets a filter path
    x.request("vendor_set", *band2)                       # and a broadcast one on every object (it leaves the two presets different)
    cap = d.stream_capacity()
    x.grow(n)
    assert d.stream_capacity() == rows_of(n, R) * R > cap
    x.enumerate(range(70, n))
    x.run(2); x.run(2)
    assert d.image_count() == images + 1, "the old objects and ONE for the arrivals"
    x.verify()
    d.close()


# ---- 7. layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("skew", "packed"))
def test_forced_layouts(layout, monkeypatch):
    monkeypatch.setenv("DSPI_F32_LAYOUT", layout)
    flavor = W.F32_FMA
    x = new_resize_sched(flavor, 40, 200, 8)
    d = x.d
    x.run(3)
    x.grow(200)
    x.enumerate(range(40, 200), blob_on=range(40, 200))
    x.run(2); x.run(1)
    plan = d.launch_plan()
    if layout == "skew": assert plan["latency_layout"] > 0 and plan["packed_shared"] == 0, plan
    else: assert plan["latency_layout"] == 0, plan
    x.verify()
    d.close()


def test_across_the_size_rule(monkeypatch):
    """40 -> 4 352 -> 40 under the library's own size rule, one preset: the latency layout only at 40, none of it at 4 352"""
    monkeypatch.delenv("DSPI_F32_LAYOUT", raising=False)
    flavor, N, vol = W.F32_FMA, 4352, -7 * 256
    blob = _shape_blob(flavor, 3)
    x = new_resize_sched(flavor, 40, N, 8, blob=blob, vol=vol, statuses=False)
    d = x.d

    def on_latency_layout(plan):
        return plan["latency_layout"] > 0 and plan["packed_shared"] == plan["packed_per_lane_values"] == plan["packed_per_lane_values_and_bands"] == plan["one_stream_per_lane_images"] == 0
    x.run(2)
    assert on_latency_layout(d.launch_plan()), d.launch_plan()
    x.grow(N)
    x.request("set_rate", FS); x.request("set_volume", vol); x.request("load_bulk", blob)      # every device the context's preset: one object again
    x.run(2)
    plan = d.launch_plan()
    assert plan["latency_layout"] == 0 and plan["latency_layout_paired"] == 0 and sum(plan.values()) > 0, plan
    x.verify([40, 41, 127, 128, 1000, 2175, N - 2, N - 1], what="at 4 352: ")      # (8 new ones spread over the rows, before their records go with the shrink)
    x.pause(40, N - 40)
    x.shrink(40)
    x.run(2)
    assert on_latency_layout(d.launch_plan()), d.launch_plan()
    x.verify(list(range(8)))
    d.close()


# ---- 8. per-stream S/PDIF -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_spdif_per_stream(flavor):
    """x with DSPI_OUT_SPDIF and per-stream positions, the twin t without the flag (its pair words are what the oracle's encoder gets), both
    through the same resize: old streams continue their blocks, new ones start at frame 0 (preamble Z) with the power-on rate's status"""
    R = row_of(flavor)
    S, n = 70, rows_of(70, R) * R + 20
    blob = WL.full_chain_blob(flavor)
    x, t = warm(context(flavor, S, FS, blob)), warm(context(flavor, S, FS, blob))
    pcm = WL.synth_pcm16(n, 5 * B, FS)
    assert x.spdif_per_stream(1)
    pos = (np.arange(S, dtype=np.int64) * 5 + 1) % 192
    x.spdif_stream_pos(0, S, set=pos)
    fs = np.full(S, FS)
    at = 0

    def call(k, what):
        nonlocal at, pos
        part = np.ascontiguousarray(pcm[:x.n_streams, at * B:(at + k) * B]); at += k
        words = t.process_host(part, k, B, 16)[0]
        got = x.process_host(part, k, B, 16, spdif=True)[0]
        assert_streams(got, expect(words, pos, fs), what)
        pos = (pos + k * B) % 192
        assert np.array_equal(x.spdif_stream_pos(), pos), f"{what}: positions read back"
        return got
    call(1, "before the grow")
    assert x.resize_streams(n) == n and t.resize_streams(n) == n
    pos = np.concatenate([pos, np.zeros(n - S, dtype=np.int64)]); fs = np.concatenate([fs, np.full(n - S, 44100)])
    assert np.array_equal(x.spdif_stream_pos(), pos), "old slots keep their positions, new slots stand at 0"
    call(2, "after the grow")      # (new streams: the oracle's encoder from position 0, frame 0 of a block with preamble Z)
    call(2, "the call after")
    x.close(); t.close()


# ---- 9. PDM ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
def test_pdm(flavor, tiled):
    R = row_of(flavor)
    n = rows_of(70, R) * R + 22
    x = new_resize_sched(flavor, 70, n, 8, statuses=False)
    d = x.d
    pdm = [PdmOracle() for _ in range(70)]

    def modulate(sub):
        S = d.n_streams; nt = rows_of(S, R)
        if tiled:
            tl = np.zeros((nt * R, sub.shape[1]), dtype=np.int32); tl[:S] = sub
            words = d.pdm_host(np.ascontiguousarray(tl.reshape(nt, R, -1).transpose(0, 2, 1)), tiled=True)      # [tile][frame][8][R]
            words = words.transpose(0, 3, 1, 2).reshape(nt * R, sub.shape[1], 8)[:S]
        else: words = d.pdm_host(sub)
        for s in range(S): assert np.array_equal(pdm[s].run(sub[s]), words[s]), f"PDM words of stream {s}"

    modulate(x.run(2)[1])
    x.grow(n)
    pdm += [PdmOracle() for _ in range(n - 70)]
    x.enumerate(range(70, n), blob_on=range(70, n))
    modulate(x.run(2)[1]); modulate(x.run(2)[1])
    x.verify(sorted({0, 1, 68, 69, 70, 71, rows_of(70, R) * R - 1, rows_of(70, R) * R, n - 2, n - 1}))
    d.close()


# ---- 10. device buffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_device_buffers(flavor):
    """process_device, a reallocating resize, process_device on buffers of the new size, with no sync of the caller's in between: the
    resize orders itself behind the first call, and the outputs are those of the host-buffer run"""
    import torch
    dev = torch.device("cuda", 0)
    R = row_of(flavor)
    S, n = 70, rows_of(70, R) * R + 30
    blob = WL.full_chain_blob(flavor)
    d, h = warm(context(flavor, S, FS, blob)), warm(context(flavor, S, FS, blob))      # (the power-on mute played out: the words compared below are not all zero)
    pcm = WL.synth_pcm16(n, 4 * B, FS)
    first, second = np.ascontiguousarray(pcm[:S, :2 * B]), np.ascontiguousarray(pcm[:, 2 * B:])

    def buffers(part):
        k, F = part.shape[0], part.shape[1]
        return (torch.from_numpy(part).to(dev), torch.zeros((k, d.P, F, 2), dtype=torch.int32, device=dev), torch.zeros((k, F), dtype=torch.int32, device=dev),
                torch.zeros((k, 2, d.C), dtype=torch.int16, device=dev))
    b1, b2 = buffers(first), buffers(second)
    torch.cuda.synchronize()
    d.process_device(b1[0].data_ptr(), 2, B, 16, b1[1].data_ptr(), b1[2].data_ptr(), b1[3].data_ptr())
    assert d.resize_streams(n) == n and d.stream_capacity() == rows_of(n, R) * R
    d.process_device(b2[0].data_ptr(), 2, B, 16, b2[1].data_ptr(), b2[2].data_ptr(), b2[3].data_ptr())
    d.sync()
    want1 = h.process_host(first, 2, B, 16)
    assert h.resize_streams(n) == n
    want2 = h.process_host(second, 2, B, 16)
    for b, want, what in ((b1, want1, "before the resize"), (b2, want2, "after the resize")):
        assert np.array_equal(b[1].cpu().numpy(), want[0]) and np.array_equal(b[2].cpu().numpy(), want[1]), what
        assert np.array_equal(b[3].cpu().numpy().view(np.uint16), want[2]), what
    assert int(np.abs(want2[0][:S]).max()) > 0
    d.close(); h.close()


# ---- 11. sequences --------------------------------------------------------------------------------------------------------------------------
STEPS = ("run", "pause", "resume", "move", "boot", "grow", "grow_paused", "shrink", "reserve")


@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("seed", range(6))
def test_sequences(flavor, seed):
    """30 random legal steps against a model of three facts (who is paused, the stream count, the capacity), every slot verified at the end.
    The generator draws only from the steps that are legal in the state at hand, so no step is left out."""
    R = row_of(flavor)
    top, packets = 3 * R + 5, 12
    rng = np.random.default_rng(77000 + 10 * seed + (2 if not int(flavor) else 1 if getattr(flavor, "fma", False) else 0))
    n = int(rng.integers(1, top + 1))
    x = new_resize_sched(flavor, n, top, packets, statuses=False)
    d = x.d
    dump, code = v2_dump(flavor)
    active, cap = np.ones(n, dtype=bool), rows_of(n, R)
    done = []
    for step in range(30):
        tail = n                                         # [tail, n) is the paused tail
        while tail > 1 and not active[tail - 1]: tail -= 1
        legal = ["pause", "resume", "move", "boot", "reserve"]
        if active.any() and int(x.pos[:n][active].max()) < packets: legal.append("run")
        if n < top: legal += ["grow", "grow_paused"]
        if tail < n: legal += ["shrink", "shrink"]
        what = legal[int(rng.integers(0, len(legal)))]
        if what == "run": x.run(1)
        elif what in ("pause", "resume"):
            first = int(rng.integers(0, n))
            count = n - first if rng.random() < 0.5 else int(rng.integers(1, n - first + 1))
            if what == "pause": x.pause(first, count); active[first:first + count] = False
            else: x.resume(first, count); active[first:first + count] = True
        elif what == "move":
            k = int(rng.integers(1, min(n, 6) + 1))
            ring = rng.choice(n, k, replace=False).tolist()      # a cycle: every destination is a source
            moves = [(ring[i], ring[(i + 1) % k]) for i in range(k)]
            free = [s for s in np.flatnonzero(~active).tolist() if s not in ring]
            src = [s for s in range(n) if s not in ring and s not in free[:1]]
            if free and src: moves.append((int(src[int(rng.integers(0, len(src)))]), free[0]))      # ... and one stream into a paused slot, its own left behind
            x.move(moves)
            was = active.copy()
            dsts = {t for _, t in moves}
            for s, t in moves: active[t] = was[s]
            for s, t in moves:
                if s != t and s not in dsts: active[s] = False
        elif what == "boot":
            l = rng.choice(n, int(rng.integers(1, min(n, 5) + 1)), replace=False).tolist()
            if rng.random() < 0.5: x.boot(l)
            else: x.boot(l, dump, want=code)
            x.enumerate(l, blob_on=l[:1])
        elif what in ("grow", "grow_paused"):
            old, n = n, int(rng.integers(n + 1, top + 1))
            x.grow(n, paused=what == "grow_paused", check_status=3)
            active = np.concatenate([active, np.full(n - old, what == "grow")])
            cap = max(cap, rows_of(n, R))
            x.enumerate(range(old, n), blob_on=(old,))
        elif what == "shrink":
            n = int(rng.integers(tail, n))
            x.shrink(n); active = active[:n].copy()
        elif what == "reserve":
            want = int(rng.integers(n, top + 1))
            cap = rows_of(want, R)
            assert d.reserve_streams(want) == cap * R
        done.append(what)
        assert int(d.L.dspi_num_streams(d.h)) == n == d.n_streams and d.stream_capacity() == cap * R, (step, done)
        assert np.array_equal(d.streams_paused().astype(bool), ~active), (step, done)
    x.verify()
    d.close()
