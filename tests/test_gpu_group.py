"""Grouping on the GPU (dspi_plan_grouping + dspi_move_streams, include/dspi.h): a context whose presets lie scattered over its slots is put
in order by one list, its streams go on exactly as if they had stayed, and the launch plan returns to the shared-preset and per-lane-value
kernels.  Every audio comparison is with the oracle, one oracle per STREAM fed that stream's own packets and given that stream's own preset,
whichever slot the stream sits in (test_gpu_pause.py's Sched, made to follow the streams by test_gpu_move.py's relocate) — never with
another run of the library.  The caller's side of the contract is exercised too: the PCM columns are permuted by the returned list.

    figures: none.  Float: 321 streams (two rows and a half, an odd last stream), Q28: 133; 48-frame packets, the full chain."""
import struct

import numpy as np
import pytest

import orclib
from conftest import has_gpu
from dspi_amd import wire as W, workloads as WL
from test_gpu_snapshot import check, fid, oracle, packets
from test_gpu_pause import new_sched
from test_gpu_move import move

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48
ONE, PACKED, PV_BANDS, PV = "one_stream_per_lane_images", "packed_shared", "packed_per_lane_values_and_bands", "packed_per_lane_values"


def presets(flavor):
    """x and x_gain differ in one band gain; y has another structure: shorter delays and a bypassed band"""
    x = WL.full_chain_blob(flavor)
    x_gain = WL.full_chain_blob(flavor)
    W.set_band(x_gain, 0, 3, W.FILTER_PEAKING, WL.PEQ_FREQS[3], 1.41, 1.5)
    y = WL.full_chain_blob(flavor, max_delay_ms=1.0)
    W.set_band(y, 1, 4, W.FILTER_FLAT, WL.PEQ_FREQS[4], 1.41, 0.0)
    return x, x_gain, y


def scattered(flavor, S, blobs, packets_total, statuses=True):
    """a context whose stream s was given blobs[s % len(blobs)] by a call of its own (blobs[0]: the context's, broadcast)"""
    x = new_sched(flavor, S, FS, B, 16, packets_total, blob=blobs[0], statuses=statuses)
    for s in range(S):
        if s % len(blobs): x.request("load_bulk", blobs[s % len(blobs)], stream=s)
    return x


def layout(d, which):
    """(A, [(preset, first slot, size)] of the runs of equal `which` among the active slots) — `which` follows the streams like every record"""
    active = ~d.streams_paused().astype(bool)
    A = int(active.sum())
    assert active[:A].all() and not active[A:].any(), "after the list slots [0, A) are active and [A, n) paused"
    runs = []
    for s in range(A):
        if runs and runs[-1][0] == which[s]: runs[-1][2] += 1
        else: runs.append([which[s], s, 1])
    return A, runs


def group(x, which, one_way):
    """plans, checks the list against the activity, applies it; `which` (the preset of the stream in every slot) follows"""
    d = x.d
    active = ~d.streams_paused().astype(bool)
    moves = d.plan_grouping(one_way)
    srcs, dsts = set(moves[:, 0].tolist()), set(moves[:, 1].tolist())
    assert len(srcs) == len(moves) == len(dsts) and all(active[t] == 0 or t in srcs for t in dsts)
    assert moves[:, 1].tolist() == sorted(moves[:, 1].tolist()) and (moves[:, 0] != moves[:, 1]).all()
    move(x, moves)      # (Sched's input, positions, history, requests and frozen status go from src to dst: the caller's per-stream buffers)
    old = which.copy()
    for s, t in moves.tolist(): which[t] = old[s]
    return moves


def one_stream_items_before(plan, rows):
    assert plan[ONE] >= rows, f"scattered presets: at least one one-stream item per row, {plan}"


# ---- 1. float, both contracts, both modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (1, W.F32_FMA), ids=fid)
@pytest.mark.parametrize("one_way", (False, True), ids=("swap", "one-way"))
def test_three_presets_of_two_structures(flavor, one_way):
    R = 128
    S = 2 * R + R // 2 + 1
    x = scattered(flavor, S, presets(flavor), 6)      # s % 3: x, x_gain, y
    d = x.d
    assert d.tile_streams() == R
    which = np.arange(S) % 3
    x.run(1)
    for s in range(3, S, 7): x.pause(s, 1)
    x.run(1)
    n_paused = len(range(3, S, 7))
    A = S - n_paused
    rows = -(-A // R)
    one_stream_items_before(d.launch_plan(), -(-S // R))
    moves = group(x, which, one_way)
    assert len(moves) > A // 2
    # the layout: x, then x_gain beside it (the same structure), then y; every preset in one run
    A2, runs = layout(d, which)
    assert A2 == A and [r[0] for r in runs] == [0, 1, 2] and sum(r[2] for r in runs) == A
    if one_way: assert d.streams_paused()[A:].all() and int(d.streams_paused().sum()) == S - A
    assert d.image_count() == 3, "the separate calls' equal objects were folded, and a move adds none"
    x.run(2)
    plan = d.launch_plan()
    groups = 3
    assert plan[ONE] <= groups, plan
    assert plan[PACKED] + plan[PV_BANDS] + plan[PV] <= rows + groups - 1 and plan[PACKED] > 0, plan
    assert plan["latency_layout"] == 0, plan
    w, r = d.stream_positions(0, S)
    for row in range(rows):
        lo, hi = row * R, min((row + 1) * R, A)
        assert len(set(w[lo:hi].tolist())) == 1 and len(set(r[lo:hi].tolist())) == 1, f"row {row}: the write positions of its active streams differ"
    assert d.plan_grouping(one_way).shape == (0, 2) and d.plan_grouping(not one_way).shape == (0, 2), "a grouped context is not disturbed"
    # the paused devices — moved up, or (one-way) the copies the movers left behind — stand where they stood: resumed, they go on
    x.resume(0, S)
    x.run(1)
    x.verify()
    d.close()


# ---- 2. Q28 ---------------------------------------------------------------------------------------------------------------------------------
def test_q28_two_presets():
    R = 64
    S = 2 * R + 5
    x0, _, y0 = presets(0)
    x = scattered(0, S, (x0, y0), 5)
    d = x.d
    assert d.tile_streams() == R
    which = np.arange(S) % 2
    rows = -(-S // R)
    x.run(2)
    plan = d.launch_plan()
    assert plan[ONE] == rows and plan["q28_shared"] == 0, f"every row on the per-lane path, {plan}"
    moves = group(x, which, False)
    assert sorted(moves[:, 0].tolist()) == sorted(moves[:, 1].tolist()), "nothing paused: a pure permutation"
    A, runs = layout(d, which)
    assert A == S and [r[0] for r in runs] == [0, 1]
    x.run(2)
    plan = d.launch_plan()
    assert plan[ONE] <= 1 and plan["q28_shared"] >= rows - 1, plan
    assert d.plan_grouping().shape == (0, 2)
    x.run(1)
    x.verify()
    d.close()


# ---- 3. one structure with every stream its own values, between streams of a second structure -----------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA,), ids=fid)
def test_own_values_interleaved_with_a_second_structure(flavor):
    R = 128
    S = 2 * R + 2
    x0, _, y0 = presets(flavor)
    x = scattered(flavor, S, (x0, y0), 5, statuses=False)
    d = x.d
    for s in range(0, S, 2): x.request("vendor_set", W.REQ["SET_PREAMP"], 0, struct.pack("<f", -9.0 + 0.05 * s), stream=s)
    which = np.where(np.arange(S) % 2 == 0, np.arange(S) + 100, 1)      # an own value each, or y
    x.run(2)
    one_stream_items_before(d.launch_plan(), -(-S // R))
    group(x, which, False)
    A, runs = layout(d, which)
    assert A == S and len(runs) == S // 2 + 1 and runs[-1][0] == 1 and runs[-1][2] == S // 2, "the own-value streams first (one class), then y in one run"
    assert d.image_count() == S // 2 + 1
    x.run(2)
    plan = d.launch_plan()
    assert plan[PV_BANDS] + plan[PV] > 0 and plan[ONE] <= 2, plan
    assert d.plan_grouping().shape == (0, 2)
    x.run(1)
    x.verify()
    d.close()


# ---- 4. per-stream S/PDIF positions travel with the streams -------------------------------------------------------------------------------
def test_spdif_positions_travel():
    flavor, R = W.F32_FMA, 128
    S = R + 12
    x0, _, y0 = presets(flavor)
    x = scattered(flavor, S, (x0, y0), 14, statuses=False)
    d = x.d
    which = np.arange(S) % 2
    x.run(6); x.run(6)      # (the power-on mute played out: the words below are not all zero)
    x.pause(7, 2)
    assert d.spdif_per_stream(1) is True
    pos = (np.arange(S) * 11 + 5) % 192
    d.spdif_stream_pos(set=pos)
    moves = group(x, which, False)
    want = pos.copy()
    for s, t in moves.tolist(): want[t] = pos[s]
    assert len(moves) > S // 2 and np.array_equal(d.spdif_stream_pos(), want), "pos[dst] := old pos[src], for all entries at once"
    # one DSPI_OUT_SPDIF call: every active stream's subframes are its oracle's words, encoded at the position that came with it
    n = 1
    pcm, paused = x.input(n)
    got = d.process_host(pcm, n, B, 16, spdif=True)[0]
    assert paused.sum() == 2 and paused[S - 2:].all() and not got[paused].any()
    loud = 0
    for s in np.flatnonzero(~paused):
        o = oracle(flavor, FS, x.blob, x.vol)
        at = {p: (lambda o, rq=rq: [getattr(o, nm)(*a) for nm, a in rq]) for p, rq in x.hooks[s].items()}
        check(o, x.data[s], 16, B, x.parts[s], f"stream in slot {s}", at=at)
        p0 = int(x.pos[s])
        words = o.process(packets(x.data[s], 16, B, p0, p0 + n), n, B, 16)[0]
        o.close()
        loud += int(np.abs(words).max() > 0)
        sub = np.stack([orclib.spdif_encode(words[p], int(want[s]), FS)[0] for p in range(words.shape[0])])
        assert np.array_equal(got[s], sub), f"slot {s}: subframes differ from the oracle's words encoded at position {int(want[s])}"
    assert loud > S // 2
    after = want.copy(); after[~paused] = (after[~paused] + n * B) % 192
    assert np.array_equal(d.spdif_stream_pos(), after)
    d.close()
