"""Grouping without a GPU: the rule of dspi_plan_grouping (include/dspi.h; dspi_amd/csrc/dspi_group.{h,cpp}) through a g++ driver
(tests/group_driver.cpp) — on hand-made populations whose lists are written out here, and on random ones held to the rule restated in
Python and to what follows from it (legality, minimality, idempotence, coverage) —, and the call itself on host-only contexts."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("group") / "group_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "group_driver.cpp"),
                    os.path.join(CSRC, "dspi_group.cpp"), os.path.join(CSRC, "dspi_move.cpp")], check=True)
    return str(exe)


def run(driver, mode, arg, cases):
    """one line of input per case, one line of output per case"""
    text = "".join(c + "\n" for c in cases)
    out = subprocess.run([driver, mode] + ([str(arg)] if arg is not None else []), input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return out


def case(active, obj, cls):
    """a population as the driver reads it; cls None: no class table (one class)"""
    act = "-" if all(active) else "".join("1" if a else "0" for a in active)
    cls = [] if cls is None else list(cls)
    return " ".join([act, str(len(cls))] + [str(int(c)) for c in cls] + [str(int(o)) for o in obj])


def parse(line):
    """(list of (src, dst), move_validate's verdict)"""
    nums, verdict = line.split("|")
    v = list(map(int, nums.split()))
    return list(zip(v[0::2], v[1::2])), verdict.strip()


# ---- the rule, restated -------------------------------------------------------------------------------------------------------------------
def runs_by_rule(active, obj, cls):
    """[(object, first slot of its run, size)] in run order, and A"""
    n = len(active)
    members = {}
    for s in range(n):
        if active[s]: members.setdefault(obj[s], []).append(s)
    klass = (lambda g: 0) if cls is None else (lambda g: cls[g])
    first_c = {}
    for g, m in members.items(): first_c[klass(g)] = min(first_c.get(klass(g), n), m[0])
    order = sorted(members, key=lambda g: (first_c[klass(g)], members[g][0]))
    runs, at = [], 0
    for g in order:
        runs.append((g, at, len(members[g]))); at += len(members[g])
    return runs, members, at


def expected_plan(active, obj, cls, one_way):
    n = len(active)
    runs, members, A = runs_by_rule(active, obj, cls)
    moves = []
    for g, at, size in runs:
        residents = {s for s in members[g] if at <= s < at + size}
        free = [d for d in range(at, at + size) if d not in residents]
        movers = [s for s in members[g] if s not in residents]
        assert len(free) == len(movers)
        moves += list(zip(movers, free))
    if not one_way:
        H = [s for s in range(A) if not active[s]]
        T = [s for s in range(A, n) if active[s]]
        assert len(H) == len(T)
        moves += list(zip(H, T))
    return sorted(moves, key=lambda m: m[1])


def apply(moves, ident, active, obj):
    """what dspi_move_streams does to the books: dst takes what src held, all at once; a source that is no destination stays behind paused"""
    ident2, active2, obj2 = list(ident), list(active), list(obj)
    for s, d in moves: ident2[d], active2[d], obj2[d] = ident[s], active[s], obj[s]
    dsts = {d for _, d in moves}
    for s, _ in moves:
        if s not in dsts: active2[s] = False
    return ident2, active2, obj2


# ---- the rule on hand-made cases ----------------------------------------------------------------------------------------------------------
HAND = {
    # name: (active, object per slot, class per object or None, the list, the one-way list)
    "alternating objects": ([1] * 6, [0, 1, 0, 1, 0, 1], [0, 1], [(4, 1), (1, 4)], None),
    "an odd group size": ([1] * 7, [0, 1, 0, 1, 0, 1, 0], [0, 1], [(4, 1), (6, 3), (1, 4), (3, 6)], None),
    "a paused hole below A": ([1, 0, 1, 1, 1, 1], [0, 0, 1, 0, 1, 1], None, [(3, 1), (5, 3), (1, 5)], [(3, 1), (5, 3)]),
    "actives above A": ([0, 0, 1, 1], [0, 0, 0, 1], [0, 1], [(2, 0), (3, 1), (0, 2), (1, 3)], [(2, 0), (3, 1)]),
    # object 2 is held by the paused slot 0 alone: it is no group, and its class (object 1's) does not begin at slot 0 because of it
    "an object held only by paused streams": ([0, 1, 1, 1, 1], [2, 0, 1, 0, 1], [0, 1, 1], [(3, 0), (4, 3), (0, 4)], [(3, 0), (4, 3)]),
    "two classes interleaved": ([1] * 8, [0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 0, 1], [(4, 1), (6, 3), (1, 4), (3, 6)], None),
    "one object": ([1, 1, 0, 1, 1], [0] * 5, [0], [(4, 2), (2, 4)], [(4, 2)]),
    "one object, nothing paused": ([1] * 5, [0] * 5, None, [], None),
    "nothing active": ([0] * 5, [0, 1, 0, 1, 2], [0, 1, 0], [], None),
    "already grouped": ([1, 1, 1, 1, 1, 0, 0], [3, 3, 1, 0, 0, 1, 3], [0, 1, 0, 2], [], None),
}


@pytest.mark.parametrize("one_way", (False, True), ids=("swap", "one-way"))
def test_hand_made_cases(driver, one_way):
    got = run(driver, "plan", int(one_way), [case(a, o, c) for a, o, c, _, _ in HAND.values()])
    for (name, (active, obj, cls, two, one)), line in zip(HAND.items(), got):
        want = one if (one_way and one is not None) else two
        moves, verdict = parse(line)
        assert moves == want, (name, moves)
        assert verdict == "ok", (name, verdict)
        assert moves == expected_plan(active, obj, cls, one_way), name      # (the restatement below agrees with the lists written out above)


def test_a_context_with_one_object_is_compacted_only(driver):
    """coverage: with one object the movers are compaction's — the active streams above A come down into the holes, ascending"""
    active = [1, 0, 1, 0, 0, 1, 1]
    moves, _ = parse(run(driver, "plan", 1, [case(active, [0] * 7, None)])[0])
    assert moves == [(5, 1), (6, 3)]


def test_classes(driver):
    # (flags, delay[0], kinds[0]) per image: a class is the first image with the same bytes
    sigs = [(1, 5, 2), (1, 5, 2), (1, 6, 2), (3, 5, 2), (1, 5, 3), (1, 6, 2), (1, 5, 2)]
    got = run(driver, "classes", None, [" ".join(f"{a} {b} {c}" for a, b, c in sigs), ""])
    assert list(map(int, got[0].split())) == [0, 0, 2, 3, 4, 2, 0] and got[1] == ""


# ---- the property test --------------------------------------------------------------------------------------------------------------------
def random_population(rng):
    n = int(rng.integers(1, 701))
    kind = rng.integers(0, 4)
    n_obj = int(rng.integers(1, 3 if kind == 0 else 12 if kind < 3 else max(2, n // 2)))
    obj = rng.integers(0, n_obj, n)
    if rng.random() < 0.3:      # long stretches of one object, as arrivals in batches leave them
        obj = np.repeat(rng.integers(0, n_obj, -(-n // 9)), 9)[:n]
    cls = None if rng.random() < 0.25 else rng.integers(0, int(rng.integers(1, 5)), n_obj)
    p = (0.0, 0.1, 0.5, 0.97)[int(rng.integers(0, 4))]
    active = rng.random(n) >= p
    return active.tolist(), obj.tolist(), None if cls is None else cls.tolist()


def check_layout(name, ident, active, obj, cls, runs, A):
    """slots [0, A) active, [A, n) paused, every object's active streams in the run the rule gave it, the runs in the rule's order"""
    assert all(active[:A]) and not any(active[A:]), name
    at = 0
    for g, first, size in runs:
        assert first == at and all(o == g for o in obj[at:at + size]), (name, g)
        at += size
    assert at == A, name
    if cls is not None:      # runs of one structure lie next to each other: a class, once left, does not return
        seen, last = set(), None
        for g, _, _ in runs:
            if cls[g] != last:
                assert cls[g] not in seen, (name, "a class in two places")
                seen.add(cls[g]); last = cls[g]


@pytest.mark.parametrize("one_way", (False, True), ids=("swap", "one-way"))
def test_random_populations(driver, one_way):
    rng = np.random.default_rng(20261019)
    pops = [random_population(rng) for _ in range(2500)]
    first = run(driver, "plan", int(one_way), [case(*p) for p in pops])
    after = []
    for k, ((active, obj, cls), line) in enumerate(zip(pops, first)):
        n = len(active)
        moves, verdict = parse(line)
        assert verdict == "ok", (k, verdict)                                            # legality: move_validate accepts the list
        assert all(s != d for s, d in moves) and [d for _, d in moves] == sorted(d for _, d in moves), k
        srcs, dsts = {s for s, _ in moves}, {d for _, d in moves}
        assert len(srcs) == len(moves) and len(dsts) == len(moves), k                   # no slot is named twice on either side
        assert all(d in srcs for d in dsts if active[d]), k                             # every active destination is itself a source
        assert moves == expected_plan(active, obj, cls, one_way), k                     # the rule, entry for entry
        runs, members, A = runs_by_rule(active, obj, cls)
        outside = sum(1 for g, at, size in runs for s in members[g] if not at <= s < at + size)
        holes = sum(1 for s in range(A) if not active[s])
        assert len(moves) == outside + (0 if one_way else holes), k                     # minimality: every entry is a stream that has to move
        ident2, active2, obj2 = apply(moves, list(range(n)), active, obj)
        check_layout(k, ident2, active2, obj2, cls, runs, A)
        if not one_way:      # nobody is lost, nobody changes between active and paused
            assert sorted(zip(ident2, active2)) == sorted(zip(range(n), active)), k
            assert all(obj2[s] == obj[ident2[s]] for s in range(n)), k
        else:                # the active streams are all there, once each
            assert sorted(ident2[:A]) == [s for s in range(n) if active[s]], k
        after.append((active2, obj2, cls))
    second = run(driver, "plan", int(one_way), [case(*p) for p in after])
    for k, line in enumerate(second):
        assert parse(line) == ([], "ok"), (k, "planning again on the result is not empty")   # idempotence


# ---- host-only contexts -------------------------------------------------------------------------------------------------------------------
def presets(flavor):
    """x and x_gain differ in one band gain, y has another structure (a shorter delay, a bypassed band)"""
    x = WL.full_chain_blob(flavor)
    x_gain = WL.full_chain_blob(flavor)
    W.set_band(x_gain, 0, 3, W.FILTER_PEAKING, WL.PEQ_FREQS[3], 1.41, 1.5)
    y = WL.full_chain_blob(flavor, max_delay_ms=1.0)
    W.set_band(y, 1, 4, W.FILTER_FLAT, WL.PEQ_FREQS[4], 1.41, 0.0)
    return x, x_gain, y


def plan_raw(d, cap, flags=0, fill=0xA5A5A5A5):
    buf = (C.c_uint32 * (2 * max(cap, 1)))(*([fill] * (2 * max(cap, 1))))
    rc = d.L.dspi_plan_grouping(d.h, buf, cap, flags)
    return rc, list(buf)


def test_symbol():
    L = host.lib()
    assert hasattr(L, "dspi_plan_grouping") and host.GROUP_ONE_WAY == 1
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + grouping: detect by symbol", "#define DSPI_GROUP_ONE_WAY 0x1u",
                 "int dspi_plan_grouping(dspi_ctx *ctx, dspi_stream_move *moves, uint32_t cap, uint32_t flags);"):
        assert word in text, word


@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_context(flavor):
    S = 301
    d = Dspi(flavor, S, device=None)
    L = d.L
    assert L.dspi_plan_grouping(None, None, 0, 0) == host.E_INVAL
    assert d.plan_grouping().shape == (0, 2) and d.plan_grouping(True).shape == (0, 2)      # one object, nothing paused
    x, x_gain, y = presets(flavor)
    which = [s % 3 for s in range(S)]      # 0: x, 1: y, 2: x with another gain
    for s in range(S): assert d.load_bulk((x, y, x_gain)[which[s]], stream=s) == 0      # every stream by a call of its own
    for s in range(5, S, 7): d.pause_streams(s, 1)
    active = [not p for p in d.streams_paused()]
    bulk = {s: d.collect_bulk(s) for s in (0, 1, 2, 5, S - 1)}
    # the structures as the library sees them: float x and x_gain are one class, on Q28 everything is
    cls = [0, 1, 0] if flavor else None
    for one_way in (False, True):
        flags = host.GROUP_ONE_WAY if one_way else 0
        want = expected_plan(active, which, cls, one_way)
        got = [tuple(m) for m in d.plan_grouping(one_way).tolist()]
        assert got == want, "streams given the same blob by separate calls are one group"
        n = len(want)
        assert n > S // 2
        assert L.dspi_plan_grouping(d.h, None, 0, flags) == n                          # count only
        assert L.dspi_plan_grouping(d.h, None, n, flags) == n
        rc, buf = plan_raw(d, n - 1, flags)
        assert rc == host.E_SHORT and all(w == 0xA5A5A5A5 for w in buf), "a short cap writes nothing"
        rc, buf = plan_raw(d, 0, flags)
        assert rc == host.E_SHORT and all(w == 0xA5A5A5A5 for w in buf)
        rc, buf = plan_raw(d, n, flags)
        assert rc == n and list(zip(buf[0::2], buf[1::2])) == want
    for flags in (0x2, 0x100, 0x80000001): assert L.dspi_plan_grouping(d.h, None, 0, flags) == host.E_INVAL
    # the layout this list gives: x, x_gain, y on float (x_gain's run beside x's, whose structure it has); x, y, x_gain on Q28
    runs, _, A = runs_by_rule(active, which, cls)
    assert [g for g, _, _ in runs] == ([0, 2, 1] if flavor else [0, 1, 2]) and A == sum(active)
    # the fold happened, and nothing else: three objects for 301 streams, the activity as it was, every stream on its own blob
    assert d.image_count() == 3
    assert [not p for p in d.streams_paused()] == active
    for s, b in bulk.items(): assert d.collect_bulk(s) == b
    before = d.image_count()
    d.plan_grouping(); d.plan_grouping(True)
    assert d.image_count() == before == 3, "planning adds no parameter object"
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_image_count_is_unchanged_where_nothing_folds(flavor):
    """every stream its own preamp: as many objects as streams before the call and after it"""
    S = 40
    d = Dspi(flavor, S, device=None)
    for s in range(S): d.vendor_set(W.REQ["SET_PREAMP"], 0, struct.pack("<f", -9.0 + 0.05 * s), stream=s)
    before = d.image_count()
    assert before == S
    assert d.plan_grouping().shape == (0, 2), "one structure, one stream per object, nothing paused: every run is where it is"
    assert d.image_count() == before
    d.pause_streams(3, 2)
    active = [s not in (3, 4) for s in range(S)]
    for one_way in (False, True):      # (every run behind the hole shifts down: the rule gives runs in order, it does not look for the fewest moves)
        assert [tuple(m) for m in d.plan_grouping(one_way).tolist()] == expected_plan(active, list(range(S)), [0] * S if flavor else None, one_way)
    assert d.image_count() == before
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_equal_objects_fold_into_one_group(flavor):
    """two streams loaded with the same blob through separate calls, between streams on another preset: the call folds the two objects
    (dspi_debug_image_count alone would not: no broadcast call has asked for the pass) and the two end in one run"""
    S = 6
    d = Dspi(flavor, S, device=None)
    x, _, y = presets(flavor)
    assert d.load_bulk(y) == 0
    assert d.load_bulk(x, stream=1) == 0 and d.load_bulk(x, stream=4) == 0
    assert d.image_count() == 3      # y, and x twice
    got = [tuple(m) for m in d.plan_grouping().tolist()]
    assert got == expected_plan([1] * S, [0, 1, 0, 0, 1, 0], [0, 1] if flavor else None, False) == [(5, 1), (1, 5)]
    assert got != expected_plan([1] * S, [0, 1, 0, 0, 2, 0], [0, 1, 1] if flavor else None, False), "(unfolded, the two would be two runs)"
    assert d.image_count() == 2, "the fold happened"
    assert d.plan_grouping().tolist() == [list(m) for m in got] and d.image_count() == 2
    d.close()
