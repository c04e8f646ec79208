"""Stream moves on the GPU (dspi_move_streams / dspi_plan_compaction, include/dspi.h): a stream that changes its slot goes on exactly as if it
had stayed.  Every audio comparison is with the oracle, one oracle per STREAM fed that stream's own packets, whichever slot the stream sits
in — never with another run of the library.  The schedule record of test_gpu_pause.py (Sched) is kept per slot; relocate() below makes it
follow the streams: input, position, history, requests, frozen status and clip flags move from src to dst with every entry.

    figures: none.  300 float streams (both contracts) / 200 Q28 streams: three rows, the last partial; 48-frame packets, the full chain
    (delays and leveller on), both float layouts."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu
from orclib import PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import DspiError
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, fid, oracle
from test_gpu_realign import assert_rows_uniform
from test_gpu_pause import Sched, new_sched

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48


def streams_of(flavor):
    return 300 if int(flavor) else 200


def relocate(x, moves):
    """x.d.move_streams has applied `moves`: the per-slot records follow.  A source that is no destination keeps its record (a frozen copy,
    paused); a destination that is no source loses its own."""
    moves = [(int(s), int(d)) for s, d in moves if int(s) != int(d)]
    data, pos, clip = x.data.copy(), x.pos.copy(), x.last_clip.copy()
    parts, hooks, frozen = [list(p) for p in x.parts], [{k: list(v) for k, v in h.items()} for h in x.hooks], dict(x.frozen)
    if not x.data.flags.writeable: x.data = x.data.copy()
    for s, d in moves:
        x.data[d] = data[s]; x.pos[d] = pos[s]; x.last_clip[d] = clip[s]
        x.parts[d] = list(parts[s]); x.hooks[d] = {k: list(v) for k, v in hooks[s].items()}
        x.frozen.pop(d, None)
        if s in frozen: x.frozen[d] = frozen[s]
    dsts = {d for _, d in moves}
    for s, _ in moves:
        if s not in dsts: x.frozen[s] = (x.d.status(s), int(clip[s]))


def move(x, moves, as_is=False):
    applied = sum(1 for s, d in moves if int(s) != int(d))
    assert x.d.move_streams(moves, as_is=as_is) == applied
    relocate(x, moves)


def permutation_list(R):
    """a swap across rows, a swap inside a row, a swap of two lane mates, a 3-cycle over three rows, an identity"""
    return [(3, R + 7), (R + 7, 3), (20, 50), (50, 20), (10, 11), (11, 10), (30, R + 30), (R + 30, 2 * R + 30), (2 * R + 30, 30), (60, 60)]


# ---- 1. permutation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
@pytest.mark.parametrize("as_is", (False, True), ids=("realigned", "as-is"))
def test_permutation(flavor, as_is):
    S = streams_of(flavor)
    x = new_sched(flavor, S, FS, B, 16, 12)
    d, R = x.d, x.d.tile_streams()
    x.run(5)
    x.pause(R, R); x.run(1); x.resume(R, R, as_is=True)      # row 1 is one packet younger than rows 0 and 2
    w0, r0 = d.stream_positions(0, S)
    assert set(w0[R:2 * R].tolist()) == {5 * B} and set(w0[:R].tolist()) == {6 * B}
    moves = permutation_list(R)
    status = {s: d.status(s) for s, _ in moves}
    bulk = {s: d.collect_bulk(s) for s, _ in moves}
    move(x, moves, as_is=as_is)
    for s, t in moves: assert d.status(t) == status[s] and d.collect_bulk(t) == bulk[s], f"stream {s} -> {t}: status / parameters differ"
    assert not d.streams_paused().any()
    w1, r1 = d.stream_positions(0, S)
    if as_is:
        for s, t in moves: assert w1[t] == w0[s] and r1[t] == r0[s], "DSPI_MOVE_AS_IS keeps every stream's own positions"
        assert w1[3] == 5 * B and w1[R + 7] == 6 * B
    else:
        assert_rows_uniform(d, "after the default move")
        assert w1[0] == 6 * B and w1[R] == 5 * B and w1[2 * R] == 6 * B, "the rows' residents did not move"
    x.run(2); x.run(3)
    if not as_is: assert_rows_uniform(d, "after the continuation")
    x.verify()
    d.close()


# ---- 1b. a row without a resident -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_row_without_resident(flavor):
    """Three active streams, from rows 0, 1 and 0, into the partial last row while all of it is paused: the row has no resident, so every
    arrival takes the positions of the arrival at the row's lowest destination (dspi_move.h, the row-target rule) — the SECOND entry of the
    list, whose source stands in row 1, one packet younger than row 0."""
    S = streams_of(flavor)
    x = new_sched(flavor, S, FS, B, 16, 12)
    d, R = x.d, x.d.tile_streams()
    L = (S - 1) // R * R                                     # the last row's first slot
    x.run(4)
    x.pause(L, S - L); x.run(1)                              # nobody in the last row is a resident, and it stands a packet behind the others
    x.pause(R, R); x.run(1); x.resume(R, R, as_is=True)      # row 1 is one packet younger than row 0, one older than the last
    w0, r0 = d.stream_positions(0, S)
    moves = [(3, L + 5), (R + 7, L + 1), (20, L + 3)]
    dsts = [t for _, t in moves]
    assert w0[3] != w0[R + 7] and w0[L + 1] not in (w0[3], w0[R + 7]), "the three rows stand at three positions"
    move(x, moves)
    w1, r1 = d.stream_positions(0, S)
    for t in dsts: assert w1[t] == w0[R + 7] and r1[t] == r0[R + 7], f"slot {t}: ({w1[t]}, {r1[t]}), the lowest destination's arrival stood at ({w0[R + 7]}, {r0[R + 7]})"
    others = np.setdiff1d(np.arange(S), dsts + [s for s, _ in moves])
    assert np.array_equal(w1[others], w0[others]) and np.array_equal(r1[others], r0[others]), "a slot the list does not name was written"
    want = np.zeros(S, dtype=np.uint8); want[L:] = 1; want[dsts] = 0; want[[3, R + 7, 20]] = 1
    assert np.array_equal(d.streams_paused(), want)
    x.run(1); x.run(1)
    w2, r2 = d.stream_positions(0, S)
    assert len(set(w2[dsts].tolist())) == 1 and len(set(r2[dsts].tolist())) == 1, "the row's active streams share one position"
    x.verify()
    d.close()


# ---- 2. one-way -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_one_way(flavor):
    S = streams_of(flavor)
    x = new_sched(flavor, S, FS, B, 16, 12)
    d, R = x.d, x.d.tile_streams()
    x.run(4)
    x.pause(40, 3); x.pause(R + 5, 1)
    x.run(1)
    # refusals change nothing: the context continues exactly (the verification at the end covers every stream)
    paused = d.streams_paused().copy()
    for bad in ([(1, 2)], [(1, 41), (3, 41)], [(1, 41), (1, 42)], [(1, S)], [(S, 41)], [(7, 41), (41, 8)], []):
        with pytest.raises(DspiError) as e: d.move_streams(bad)
        assert e.value.code == host.E_INVAL, bad
    assert d.L.dspi_move_streams(d.h, None, 1, 0) == host.E_INVAL
    m = np.array([[7, 41]], dtype=np.uint32)
    for flags in (0x2, 0x100, 0x80000000): assert d.L.dspi_move_streams(d.h, m.ctypes.data, 1, flags) == host.E_INVAL
    assert np.array_equal(d.streams_paused(), paused)
    x.run(1)
    # active streams into paused slots: within a row, across rows, and a chain whose head stays behind
    moves = [(7, 41), (R + 9, 40), (2 * R + 1, R + 5), (8, 2 * R + 1)]
    status = {s: d.status(s) for s, _ in moves}
    move(x, moves)
    want = paused.copy(); want[[41, 40, R + 5, 2 * R + 1]] = 0; want[[7, R + 9, 8]] = 1
    assert np.array_equal(d.streams_paused(), want), "a source that is no destination becomes paused, activity travels with the stream"
    for s, t in moves: assert d.status(t) == status[s]
    for s in (7, R + 9, 8): assert d.status(s) == status[s], "the frozen copy keeps its status bytes"
    x.run(2); x.run(1)
    # the frozen copies are the streams as they stood at the move: resumed, and fed the same input, they go the same way
    x.resume(0, S)
    x.run(2)
    x.verify()
    d.close()


# ---- 3. parameters travel by reference ------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_parameters_travel_by_reference(flavor):
    """A band change that resets a filter path on one stream and a preset-slot load (mute, zeroed lines) on another, immediately before the
    move with no dspi_process in between: the pending state operations reach the streams at their new slots.  No image is added.  The PDM
    modulator words travel too: dspi_pdm_modulate before and after the move against one PdmOracle per stream."""
    S = streams_of(flavor)
    x = new_sched(flavor, S, FS, B, 16, 12, statuses=False)
    d, R = x.d, x.d.tile_streams()
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, FS, other); image = ref.save_slot(0); ref.close()
    band = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    pdm = [PdmOracle() for _ in range(S)]

    def modulate(sub):
        words = d.pdm_host(sub)
        for s in range(S): assert np.array_equal(pdm[s].run(sub[s]), words[s]), f"PDM words of the stream in slot {s}"

    modulate(x.run(3)[1])
    x.request("vendor_set", *band, stream=5)
    x.request("load_slot", image, -1, stream=R + 3)
    images = d.image_count()
    assert images == 3
    bulk = d.collect_bulk(R + 3)
    moves = [(5, 2 * R + 8), (2 * R + 8, 5), (R + 3, 9), (9, R + 3), (70, R + 70), (R + 70, 70)]
    old_pdm = list(pdm)
    move(x, moves)
    for s, t in moves: pdm[t] = old_pdm[s]
    assert d.image_count() == images, "a move adds no parameter object"
    assert d.collect_bulk(9) == bulk and d.collect_bulk(R + 3) != bulk
    modulate(x.run(2)[1]); modulate(x.run(3)[1])
    assert d.image_count() == images
    x.verify()
    d.close()


# ---- 4. small batches -----------------------------------------------------------------------------------------------------------------------
def small_batches(flavor_id):
    """(runs in a child process, DSPI_MOVE_BATCH=3) a 7-cycle and a 9-chain across rows through a scratch of three records"""
    flavor = {"f32": 1, "fma": W.F32_FMA, "q28": 0}[flavor_id]
    assert os.environ.get("DSPI_MOVE_BATCH") == "3"
    S = streams_of(flavor)
    x = new_sched(flavor, S, FS, B, 16, 10, statuses=False)
    R = x.d.tile_streams()
    x.run(3)
    x.pause(R, R); x.run(1); x.resume(R, R, as_is=True)
    x.pause(2 * R + 40, 1)
    x.run(1)
    cyc = [4, R + 4, 2 * R + 4, 17, R + 17, 2 * R + 17, 90]
    chain = [6, R + 6, 2 * R + 6, 33, R + 33, 2 * R + 33, 50, R + 50, 2 * R + 20, 2 * R + 40]
    assert len(set(cyc + chain)) == 17      # (with 64- and with 128-stream rows)
    moves = [(cyc[i], cyc[(i + 1) % 7]) for i in range(7)] + [(chain[i], chain[i + 1]) for i in range(9)]
    move(x, moves)
    want = np.zeros(S, dtype=np.uint8); want[6] = 1
    assert np.array_equal(x.d.streams_paused(), want)
    x.run(2); x.run(2)
    x.verify()
    x.d.close()
    print("small batches ok")


@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_small_batches(flavor):
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, DSPI_MOVE_BATCH="3")
    code = f"import sys; sys.path[:0] = [{tests!r}, {os.path.dirname(tests)!r}]; import test_gpu_move as t; t.small_batches({fid(flavor)!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "small batches ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 5. compaction --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("one_way", (False, True), ids=("swap", "one-way"))
def test_compaction(flavor, one_way):
    S = 384 if int(flavor) else 192
    x = new_sched(flavor, S, FS, B, 16, 10, statuses=False)
    d, R = x.d, x.d.tile_streams()
    key = "packed_shared" if int(flavor) else "q28_shared"
    x.run(2)
    for s in range(1, S, 2): x.pause(s, 1)
    x.run(2)
    plan = d.launch_plan()
    if int(flavor): assert plan["one_stream_per_lane_images"] > 0 and plan[key] == 0, plan      # every lane has lost its mate
    moves = d.plan_compaction(one_way)
    assert len(moves) == (S // 4 if one_way else S // 2)
    move(x, moves)
    p = d.streams_paused().astype(bool)
    assert not p[:S // 2].any() and p[S // 2:].all()
    x.run(1); x.run(2)
    plan = d.launch_plan()
    assert plan[key] == -(-(S // 2) // R) and sum(v for k, v in plan.items() if k != "latency_layout_paired") == plan[key], plan
    assert_rows_uniform(d, "the compacted rows", rows=range(S // 2 // R))
    if one_way:
        assert d.plan_compaction().shape == (0, 2)
        x.verify(range(S // 2))
    else:
        x.resume(0, S)      # the paused devices are all still there, at their new slots
        x.run(2)
        assert d.launch_plan()[key] == S // R
        x.verify()
    d.close()
