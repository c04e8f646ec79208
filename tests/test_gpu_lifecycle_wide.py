"""The wide lifecycle fuzz on the GPU: random legal sequences of every stream-maintenance call, now with resizes and reserves, migrations and the
rebalance, grouping, dspi_process_pdm with the running byte, dspi_pdm_fade and dspi_process_mixed (tests/lifecycle_wide.py draws them and follows
them), on a main context and a side context whose sizes change.  Every verified slot is replayed on a fresh oracle fed the bytes the call fed it,
at the depth the call gave its slot; every PDM word is held, at the call, to the slot's live modulator model, whose sub words the replay holds to
the chain's oracle.  Nothing is compared with another run of the library, and nothing has a tolerance.

    test_fuzz_wide     the default seeds; tests/test_lifecycle_wide_cpu.py::test_default_wide_seeds_contain_the_crossings says what they contain
    test_scenario_*    four fixed sequences at 299 float / 199 Q28 streams (three rows, a ragged odd last stream), where a failure reads plainly"""
import os

import numpy as np
import pytest

from conftest import has_gpu
from dspi_amd import workloads as WL
from test_boot_cpu import flash_cases
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, fid
import lifecycle_model as M
import lifecycle_wide as X

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]


def _fuzz_seeds():
    s0 = int(os.environ.get("DSPI_FUZZ_SEED0", 0))
    return range(s0, s0 + int(os.environ.get("DSPI_LIFECYCLE_FUZZ_SEEDS", 32)))


@pytest.fixture
def new_lives():
    """X.new_lives_wide whose contexts are closed when the test ends, however it ends"""
    made = []

    def make(cfg):
        made.append(X.new_lives_wide(cfg))
        return made[-1]
    yield make
    for lives in made:
        for x in lives: x.d.close()


@pytest.mark.auto_layout
@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_fuzz_wide(seed, monkeypatch, new_lives):
    """One random sequence on a flavour, float layout, rate, packet length, bit depth and starting size that go round with the seed.  Every
    stream is verified up to 131 streams; beyond, every slot an op named, each one's lane mate, slots 0 and S - 1 and 16 random others.
    Replay one seed alone:
    DSPI_FUZZ_SEED0=<seed> DSPI_LIFECYCLE_FUZZ_SEEDS=1 pytest tests/test_gpu_lifecycle_wide.py -m gpu -k test_fuzz_wide -s"""
    cfg, ops = X.schedule_wide(seed)
    if cfg["layout"]: monkeypatch.setenv("DSPI_F32_LAYOUT", cfg["layout"])
    print(X.describe(cfg, ops), flush=True)
    lives = new_lives(cfg)
    X.execute_wide(cfg, ops, lives)
    named = X.named(ops, [x.d.n_streams for x in lives])
    rng = np.random.default_rng(seed)
    for c, x in enumerate(lives):
        S = x.d.n_streams
        if S <= 131: streams = range(S)
        else:
            hit = named.get(c, set())
            streams = sorted(hit | {s ^ 1 for s in hit if (s ^ 1) < S} | {0, S - 1} | {int(v) for v in rng.integers(0, S, 16)})
        x.verify(streams, what=f"seed {seed}, {'side' if c else 'main'} context: ")


# ---- the fixed scenarios ----------------------------------------------------------------------------------------------------------------------
FS, B = 48000, 48


def scenario(new_lives, flavor, mode=False, depth=16):
    """the main context (299 float / 199 Q28 streams) and the side context on the full chain, warmed up past the power-on mute; room for a row more"""
    fl = fid(flavor)
    blob, blob2 = WL.full_chain_blob(flavor), WL.full_chain_blob(flavor, max_delay_ms=7.0)
    blob2["preamp"]["preamp_db"][:] = (-1.0, -5.0)
    S, R = M.sizes(fl)[-1], M.row(fl)
    cfg = dict(seed=-1, flavor=fl, layout=None, fs=FS, B=B, depth=depth, S=S, side=M.SIDE, R=R, top=S + R, blob=blob, blob2=blob2,
               vol=-20 * 256, vol_side=-9 * 256, first_stream=0)
    lives = new_lives(cfg)
    for x in lives: x.run(M.WARM)
    if mode:
        for x in lives: x.spdif_mode(7, 191)
    return cfg, lives, np.random.default_rng(5)


def checked(lives, what):
    for x in lives: x.check_books(what)


def depths(rng, x, pattern):
    return X.depth_vector(rng, pattern, x.d.n_streams)


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_rebalance(flavor, new_lives):
    """(a) streams that run PDM, two of them fading, are rebalanced from the main context into a side context grown paused for them, and the
    main context is shrunk; calls in mixed depths on both sides before and after.  The arrivals go on exactly: chain, modulator, byte, fade"""
    cfg, (x, y), rng = scenario(new_lives, flavor)
    R, S = cfg["R"], cfg["S"]
    for z in (x, y): z.pdm_fade(True)
    x.request("sub_on"); y.request("sub_on", stream=3)
    x.run(2, form="pdm"); y.run(1, form="mixed_pdm", depths=depths(rng, y, "alternating"))
    x.request("sub_off", stream=S - 2); x.request("sub_off", stream=S - 7)
    x.run(2, form="mixed_pdm", depths=depths(rng, x, "lane_mates"), mem="device")
    assert x.m[S - 2].pos == 1024 - 2 * B == x.m[S - 7].pos and x.m[S - 1].running == 1
    checked((x, y), "before the rebalance")
    want = 9
    y.pause(10, 2)                                       # two paused slots it has; for the other seven it is grown
    y.grow(M.SIDE + want - 2, paused=True)
    plan = [tuple(m) for m in x.d.plan_migration(y.d, want).tolist()]
    assert plan == X.migration_pairing(x.paused, y.paused, want) == list(zip(range(S - want, S), [10, 11] + list(range(M.SIDE, M.SIDE + 7))))
    x.migrate_to(y, plan)
    x.shrink(S - want)
    checked((x, y), "after the rebalance")
    assert y.m[M.SIDE + 5].pos == 1024 - 2 * B and not y.paused.any()
    y.run(2, form="mixed_pdm", depths=depths(rng, y, "random"), mem="device", tiled=True, i2s=True)
    x.run(1, form="mixed", depths=depths(rng, x, "all_but_one"))
    y.request("sub_on", stream=M.SIDE + 5)               # a cancel at its new home
    y.run(2, form="pdm", i2s=True, enabled_only=True); x.run(1, form="pdm", mem="device", enabled_only=True)
    checked((x, y), "at the end")
    x.verify(sorted({0, 1, R - 1, R, 2 * R, S - want - 2, S - want - 1}), what="main: ")
    y.verify(sorted({0, 3, 9, 10, 11, 12, M.SIDE - 1} | set(range(M.SIDE, M.SIDE + 7))), what="side: ")


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_stale_stash_across_resizes(flavor, new_lives):
    """(b) two stashes of the top; the context is shrunk below them, regrown (new devices there) and its capacity reserved up and back (two
    reallocations); then the stashes come back into the regrown slots, one with its running bytes and fade words carried, one without: the
    streams are rewound to the export, the second under the slots' own bytes"""
    cfg, (x, y), rng = scenario(new_lives, flavor, depth=24)
    R, S = cfg["R"], cfg["S"]
    x.pdm_fade(True)
    x.request("sub_on")
    x.run(2, form="pdm")
    x.request("sub_off", stream=S - 5)
    x.run(1, form="pdm", mem="device")
    carried, plain = x.export(S - 6, 2), x.export(S - 3, 2)
    assert carried["running"].tolist() == [1, 1] and int(carried["fade"][1]) & 0xFFFF == 1024 - B
    x.pause(S - 8, 8)
    x.shrink(S - 8)
    x.run(1, form="mixed", depths=depths(rng, x, "alternating"))
    x.grow(S)
    x.enumerate(range(S - 8, S), blob_on=(S - 6, S - 3))
    x.reserve(S + R); x.reserve(S)
    checked((x, y), "after the resizes")
    assert x.d.pdm_running(S - 8, 8).tolist() == [0] * 8 and not x.d.pdm_fade_state(S - 8, 8).any()
    x.import_(S - 6, carried); x.pdm_carry(S - 6, carried)
    x.import_(S - 3, plain, realign=True)
    checked((x, y), "after the imports")
    assert x.d.pdm_running(S - 6, 5).tolist() == [1, 1, 0, 0, 0]
    x.run(2, form="pdm"); x.run(1, form="mixed_pdm", depths=depths(rng, x, "random"), mem="device")
    x.verify(sorted({0, R, S - 9} | set(range(S - 8, S))), what="main: ")


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_grouping(flavor, new_lives):
    """(c) two structurally different presets assigned alternately, boots and a per-stream dspi_load_bulk in between, some streams paused; the
    context is grouped; calls in mixed depths before and after the grouping move, per-stream S/PDIF positions on: every moved stream is still
    its oracle's, at its own block position, at the depth its new slot is given"""
    cfg, (x, y), rng = scenario(new_lives, flavor, mode=True)
    R, S = cfg["R"], cfg["S"]
    dump, code = flash_cases(flavor)[0]
    for s in range(1, S, 2): x.request("load_bulk", "blob2", stream=s)
    x.boot([4, R + 1], dump, want=code); x.boot([R - 1], None)
    x.enumerate([4, R + 1, R - 1], blob_on=[4])
    x.request("load_bulk", "blob2", stream=2 * R)
    x.pause(20, 3); x.pause(2 * R + 2, 1)
    x.run(2, form="mixed", depths=depths(rng, x, "lane_mates"), spdif=True)
    assert x.d.image_count() >= 4
    moves = X.group(x, one_way=False, what="the grouping")
    assert len(moves) > S // 4, "alternating presets: most streams move"
    checked((x, y), "after the grouping move")
    x.run(2, form="mixed", depths=depths(rng, x, "random"), spdif=True, mem="device")
    x.run(1, form="mixed", depths=depths(rng, x, "alternating"))
    assert X.group(x, one_way=True, what="the second grouping") == []
    named = {v for m in moves[:6] + moves[-6:] for v in m}
    x.verify(sorted({0, 1, 4, 19, 20, R - 1, R, R + 1, 2 * R, S - 5, S - 4, S - 1} | named), what="main: ")


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_scenario_mode_off_migration_and_mode_toggle(flavor, new_lives):
    """(d) a fading stream migrates into a context whose fade mode is off (the fade has ended: byte 0, position 0) and back into one whose
    mode is on; then the mode is switched off and on under fades in flight"""
    cfg, (x, y), rng = scenario(new_lives, flavor)
    R, S = cfg["R"], cfg["S"]
    x.pdm_fade(True)
    x.request("sub_on"); y.request("sub_on")
    x.run(2, form="pdm"); y.run(2, form="pdm")
    for s in (7, R + 1, S - 1): x.request("sub_off", stream=s)
    x.run(2, form="pdm", mem="device")
    assert [x.m[s].pos for s in (7, R + 1, S - 1)] == [1024 - 2 * B] * 3
    y.pause(30, 2)
    x.migrate_to(y, [(7, 30), (8, 31)])                    # a fading and a running stream into the mode-off context
    checked((x, y), "after the migration into the mode-off context")
    assert y.d.pdm_running(30, 2).tolist() == [0, 1] and x.d.pdm_running(7, 2).tolist() == [1, 1], "the fade has ended at the destination; the frozen copy keeps its byte"
    y.run(1, form="pdm"); x.run(1, form="mixed_pdm", depths=depths(rng, x, "alternating"))
    y.pdm_fade(True)
    y.request("sub_off", stream=31)
    y.run(1, form="pdm", mem="device")
    assert y.m[31].pos == 1024 - B
    y.migrate_to(x, [(31, 8), (30, 7)], as_is=True)        # back over the frozen copies, both modes on: the fade travels
    checked((x, y), "after the migration back")
    assert x.m[8].pos == 1024 - B and x.m[7].pos == 0
    x.run(1, form="pdm")
    x.pdm_fade(False)                                       # three fades in flight end at once
    checked((x, y), "after the mode went off")
    assert x.d.pdm_running(8, 1).tolist() == [0] and x.d.pdm_running(S - 1, 1).tolist() == [0]
    x.run(1, form="pdm", mem="device")
    x.pdm_fade(True)
    x.request("sub_on", stream=8); x.request("sub_on", stream=S - 1)
    x.run(2, form="pdm"); y.run(1, form="pdm")
    checked((x, y), "at the end")
    x.verify(sorted({0, 6, 7, 8, 9, R, R + 1, S - 2, S - 1}), what="main: ")
    y.verify((0, 29, 30, 31, 32, M.SIDE - 1), what="side: ")
