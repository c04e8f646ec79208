"""Lifecycle fuzz on the GPU: random legal sequences of every stream-maintenance call (tests/lifecycle_model.py draws them and follows them)
on a main context and a side context of 70 streams, every verified slot replayed on a fresh oracle — pair words in every output form,
S/PDIF subframes at the slot's own block position, I2S slot words, sub, peaks, clip flags, status bytes, PDM words and, at the end, the
parameters.  Nothing is compared with another run of the library, and nothing has a tolerance.

    test_fuzz        the default seeds; tests/test_lifecycle_cpu.py::test_default_seeds_contain_the_crossings says what they contain
    test_scenario_*  four fixed sequences at 299 float / 199 Q28 streams (three rows, a ragged odd last stream), where a failure reads plainly"""
import os
import struct

import numpy as np
import pytest

from conftest import has_gpu
from dspi_amd import wire as W, workloads as WL
from test_boot_cpu import flash_cases
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, fid
import lifecycle_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]


def _fuzz_seeds():
    s0 = int(os.environ.get("DSPI_FUZZ_SEED0", 0))
    return range(s0, s0 + int(os.environ.get("DSPI_LIFECYCLE_FUZZ_SEEDS", 32)))


def close(lives):
    for x in lives: x.d.close()


@pytest.mark.auto_layout
@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_fuzz(seed, monkeypatch):
    """One random sequence on a random flavour, float layout, rate, packet length, bit depth, preset and size.  Every stream is verified up
    to 131 streams; beyond, every slot an op named, each one's lane mate, slots 0 and S - 1 and 16 random others.  Replay one seed alone:
    DSPI_FUZZ_SEED0=<seed> DSPI_LIFECYCLE_FUZZ_SEEDS=1 pytest tests/test_gpu_lifecycle_fuzz.py -m gpu -k test_fuzz -s"""
    cfg, ops = M.schedule(seed)
    if cfg["layout"]: monkeypatch.setenv("DSPI_F32_LAYOUT", cfg["layout"])
    print(M.describe(cfg, ops), flush=True)
    lives = M.new_lives(cfg)
    M.execute(cfg, ops, lives)
    named = M.named(ops)
    rng = np.random.default_rng(seed)
    for c, x in enumerate(lives):
        S = x.d.n_streams
        if S <= 131: streams = range(S)
        else:
            hit = {s for s in named.get(c, ()) if s < S}
            streams = sorted(hit | {s ^ 1 for s in hit if (s ^ 1) < S} | {0, S - 1} | {int(v) for v in rng.integers(0, S, 16)})
        x.verify(streams, what=f"seed {seed}, {'side' if c else 'main'} context: ")
    close(lives)


# ---- the fixed scenarios ----------------------------------------------------------------------------------------------------------------------
FS, B = 48000, 48


def scenario(flavor, mode=False):
    """the main context (299 float / 199 Q28 streams) and the side context on the full chain, warmed up past the power-on mute"""
    fl = fid(flavor)
    blob, blob2 = WL.full_chain_blob(flavor), WL.full_chain_blob(flavor, max_delay_ms=7.0)
    blob2["preamp"]["preamp_db"][:] = (-1.0, -5.0)
    cfg = dict(seed=-1, flavor=fl, layout=None, fs=FS, B=B, depth=16, S=M.sizes(fl)[-1], side=M.SIDE, R=M.row(fl), blob=blob, blob2=blob2,
               vol=-20 * 256, vol_side=-9 * 256, first_stream=0)
    lives = M.new_lives(cfg)
    for x in lives: x.run(M.WARM)
    if mode:
        for x in lives: x.spdif_mode(7, 191)
    return cfg, lives


def checked(lives, what):
    for x in lives: x.check_books(what)


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_booted_stream_travels(flavor):
    """(a) a slot boots from a dump, its host sets it up, it plays, it moves across a row edge, it is exported into the side context and
    comes back at another index of the main one: wherever it sits it is the oracle booted from that dump"""
    cfg, (x, y) = scenario(flavor)
    R, S = cfg["R"], cfg["S"]
    dump, code = flash_cases(flavor)[0]
    x.boot([R - 2, 5], dump, want=code)
    x.enumerate([R - 2, 5], blob_on=[5])
    x.run(2)
    x.move([(R - 2, R + 1), (R + 1, R - 2), (5, 2 * R + 9), (2 * R + 9, 5)])      # (an odd shift across the row edge: the stream changes its side of a lane)
    checked((x, y), "after the move")
    x.run(1, mem="device", tiled=True)
    y.import_(33, x.export(R + 1, 1)); y.import_(8, x.export(2 * R + 9, 1), realign=True)
    y.run(2); x.run(2)
    x.import_(S - 1, y.export(33, 1), realign=True); x.import_(R, y.export(8, 1))
    checked((x, y), "after the imports")
    x.run(3); y.run(1)
    for s in (R + 1, 2 * R + 9, S - 1, R): assert s in x.booted
    x.verify(sorted({0, 4, 5, 6, R - 2, R - 1, R, R + 1, R + 2, 2 * R + 8, 2 * R + 9, S - 2, S - 1}), what="main: ")
    y.verify((7, 8, 9, 32, 33, 34, M.SIDE - 1), what="side: ")
    close((x, y))


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_stale_stash(flavor):
    """(b) an export; then a broadcast band change that resets a filter path and a per-stream preset load on the source, with no run in
    between; then the now stale stash is imported beside the source with DSPI_SNAP_REALIGN.  The copy knows nothing of the two requests,
    the source has them: both go their own way."""
    cfg, (x, y) = scenario(flavor)
    R = cfg["R"]
    stash = x.export(R - 3, 6)
    x.request("vendor_set", W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    x.request("load_slot", "image", -1, stream=R - 1)
    x.import_(R + 3, stash, realign=True)
    checked((x, y), "after the import")
    x.run(2); x.run(1, enabled_only=True)
    # (the copy plays the source's input from the export on: the two differ by the requests alone)
    assert x.d.collect_bulk(R - 1) != x.d.collect_bulk(R + 5) and x.d.collect_bulk(R - 3) != x.d.collect_bulk(R + 3)
    x.run(2)
    x.verify(sorted({0, R - 4} | set(range(R - 3, R + 10))), what="main: ")
    close((x, y))


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_frozen_copy_keeps_the_old_preset(flavor):
    """(c) pauses, a one-way compaction, then a per-stream dspi_load_bulk to a moved stream, whose parameter object the frozen copy it left
    behind still references: the moved stream plays the new preset; the copy, resumed, still plays the old one"""
    cfg, (x, y) = scenario(flavor)
    R, S = cfg["R"], cfg["S"]
    x.pause(3, 4); x.pause(R - 1, 2)
    x.run(1)
    moves = M.compaction(x.paused, True)
    assert [tuple(m) for m in x.d.plan_compaction(one_way=True).tolist()] == moves and len(moves) == 6
    x.move(moves)
    checked((x, y), "after the compaction")
    (src, dst), (src2, dst2) = moves[0], moves[-1]
    x.request("load_bulk", "blob2", stream=dst)
    x.request("vendor_set", W.REQ["SET_PREAMP"], 0, struct.pack("<f", -7.5), stream=dst2)
    x.run(2)
    x.resume(src, 1); x.resume(src2, 1, as_is=True)
    assert x.d.collect_bulk(src) == x.d.collect_bulk(0) != x.d.collect_bulk(dst)
    x.run(2)
    x.check_image_count("at the end")
    x.verify(sorted({0, 2, 3, 4, 6, 7, R - 2, R - 1, R, R + 1, src, src2, dst, dst2, S - 7, S - 1}), what="main: ")
    close((x, y))


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_spdif_positions_and_pdm_on_device_buffers(flavor):
    """(d) per-stream S/PDIF positions and the PDM modulators through a pause, a move, a boot and an import whose position is carried over,
    on device buffers: every subframe at the slot's own position and the stream's own rate, every PDM word its modulator's"""
    cfg, (x, y) = scenario(flavor, mode=True)
    R, S = cfg["R"], cfg["S"]
    dev = dict(mem="device", spdif=True)
    x.run(1, **dev); x.modulate()
    x.pause(R - 2, 4); x.pause(S - 1, 1)
    x.run(2, **dev); x.modulate(tiled=True)
    x.move([(7, R - 1), (R + 5, 7), (20, 21), (21, 20)])      # (a chain into a paused slot: slot R + 5 keeps a frozen copy)
    checked((x, y), "after the move")
    x.run(1, **dev); x.modulate()
    x.boot([21, R], None); x.boot([S - 1], flash_cases(flavor)[0][0], want=flash_cases(flavor)[0][1])
    x.run(1, **dev)                                           # (before their hosts set them up: 44.1 kHz in the channel status)
    x.enumerate([21, R, S - 1])
    x.run(1, **dev); x.modulate()
    stash = x.export(6, 3)
    y.import_(40, stash); y.spdif_carry(40, stash)
    y.pause(50, 1); y.import_(50, x.export(R - 1, 1))           # (into a paused slot, no carry: the slot's position stays)
    checked((x, y), "after the imports")
    y.run(2, **dev); y.modulate(); x.run(1, **dev)
    x.resume(0, S); y.resume(0, M.SIDE)
    x.run(1, **dev); y.run(1, **dev); x.modulate(); y.modulate(tiled=True)
    x.verify(sorted({0, 6, 7, 8, 20, 21, R - 3, R - 2, R - 1, R, R + 1, R + 2, R + 5, S - 2, S - 1}), what="main: ")
    y.verify((0, 39, 40, 41, 42, 43, 50, 51, M.SIDE - 1), what="side: ")
    close((x, y))
