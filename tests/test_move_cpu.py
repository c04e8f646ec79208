"""Stream moves without a GPU: the list rules, the compaction rule, the realignment targets and the batch schedule
(dspi_amd/csrc/dspi_move.{h,cpp}) through a g++ driver (tests/move_driver.cpp), and the two calls of include/dspi.h on host-only contexts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("move") / "move_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "move_driver.cpp"),
                    os.path.join(CSRC, "dspi_move.cpp")], check=True)
    return str(exe)


def run(driver, mode, arg, cases):
    """one line of input per case, one line of output per case"""
    text = "".join(c + "\n" for c in cases)
    out = subprocess.run([driver, mode] + ([str(arg)] if arg is not None else []), input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return out


def flat(moves):
    return " ".join(f"{s} {d}" for s, d in moves)


def bits(active):
    return "".join("1" if a else "0" for a in active)


def mixed_set(S, R):
    """tests/test_gpu_pause.py's pattern of paused streams, written out again (that module needs a GPU to import)"""
    p = np.zeros(S, dtype=bool)
    p[R:2 * R] = True
    p[10:30:2] = True
    p[41:61:2] = True
    p[2 * R + 6:2 * R + 10] = True
    p[2 * R - 6:2 * R + 2] = True
    if S & 1: p[S - 1] = True
    return p


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_move_streams") and hasattr(L, "dspi_plan_compaction")
    assert host.MOVE_AS_IS == 1 and host.COMPACT_ONE_WAY == 1
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("typedef struct dspi_stream_move { uint32_t src, dst; } dspi_stream_move;", "#define DSPI_MOVE_AS_IS      0x1u", "#define DSPI_COMPACT_ONE_WAY 0x1u",
                 "int dspi_move_streams(dspi_ctx *ctx, const dspi_stream_move *moves, uint32_t n, uint32_t flags);",
                 "int dspi_plan_compaction(const dspi_ctx *ctx, dspi_stream_move *moves, uint32_t cap, uint32_t flags);"):
        assert word in text, word


# ---- the batch schedule -------------------------------------------------------------------------------------------------------------------
def execute(line, moves, cap, n_slots):
    """runs the batches on an integer array; returns the array and the number of batches"""
    arr = np.arange(n_slots, dtype=np.int64) + 1000
    rec = np.full(cap, -1, dtype=np.int64)
    tok = line.split()
    batches = 0
    i = 0
    gathering = True
    seen = set()
    while i < len(tok):
        if tok[i] == "B":
            batches += 1; gathering = True; seen = set(); i += 1
            continue
        kind, slot, r = tok[i], int(tok[i + 1]), int(tok[i + 2]); i += 3
        assert 0 <= r < cap, f"record {r} with a scratch of {cap}"
        if kind == "g":
            assert gathering, "a gather after a scatter inside one batch"
            assert r not in seen, "a record gathered twice in one batch"
            seen.add(r); rec[r] = arr[slot]
        else:
            gathering = False
            assert rec[r] >= 0, "a record scattered before it was gathered"
            arr[slot] = rec[r]; rec[r] = -1      # (every record is scattered once)
    want = np.arange(n_slots, dtype=np.int64) + 1000
    for s, d in moves:
        want[d] = 1000 + s
    return arr, want, batches


def named_lists():
    swaps = [(0, 9), (9, 0), (3, 4), (4, 3), (20, 150), (150, 20)]
    cycle7 = [(k, (k + 1) % 7 + 0) for k in range(7)]
    cycle7 = [(10 * s + 1, 10 * d + 1) for s, d in cycle7]
    chain9 = [(5 + 7 * k, 5 + 7 * (k + 1)) for k in range(9)]            # 5 -> 12 -> ... -> 68, which is free
    mixed = swaps[:2] + [(100 + s, 100 + d) for s, d in cycle7] + [(300 + s, 300 + d) for s, d in chain9] + [(250, 250), (260, 261), (262, 260)]
    return dict(swaps=swaps, cycle7=cycle7, chain9=chain9, mixed=mixed)


def random_list(rng, n_slots=64):
    """a random partial injection: random disjoint cycles and chains, shuffled, with some identities"""
    slots = rng.permutation(n_slots).tolist()
    moves = []
    while len(slots) > 1 and rng.random() < 0.9:
        k = int(min(len(slots), rng.integers(1, 14)))
        grp, slots = slots[:k], slots[k:]
        if k == 1:
            moves.append((grp[0], grp[0]))
        elif rng.random() < 0.5:
            moves += [(grp[i], grp[(i + 1) % k]) for i in range(k)]
        else:
            moves += [(grp[i], grp[i + 1]) for i in range(k - 1)]
    if not moves: moves = [(slots[0], slots[1])]
    order = rng.permutation(len(moves))
    return [moves[i] for i in order]


@pytest.mark.parametrize("cap", (2, 3, 8))
def test_batch_schedule(driver, cap):
    rng = np.random.default_rng(77)
    lists = list(named_lists().items()) + [(f"random {i}", random_list(rng)) for i in range(200)]
    lines = run(driver, "schedule", cap, [flat(m) for _, m in lists])
    for (name, moves), line in zip(lists, lines):
        n_slots = max(max(s, d) for s, d in moves) + 1
        got, want, batches = execute(line, moves, cap, n_slots)
        assert np.array_equal(got, want), (name, cap)
        applied = sum(1 for s, d in moves if s != d)
        assert batches >= -(-applied // cap) and batches <= applied + 1, (name, cap, batches)
    # whole cycles share a batch where they fit: three swaps in a scratch of 8 are one batch, a 7-cycle too
    by = dict(zip((n for n, _ in lists), lines))
    if cap == 8: assert by["swaps"].count("B") == 1 and by["cycle7"].count("B") == 1
    # a cycle longer than the scratch holds one record (record 0) from its first batch to its last
    if cap == 3:
        tok = by["cycle7"].split("B")[1:]
        assert len(tok) == 3 and " g 61 0 " in " " + tok[0] and " s 1 0 " in " " + tok[-1], by["cycle7"]
        assert all("0" not in t.split()[2::3] for t in tok[1:-1])


# ---- validation ---------------------------------------------------------------------------------------------------------------------------
def test_validation(driver):
    n = 10
    act = bits([1, 1, 1, 1, 0, 0, 1, 1, 1, 1])
    cases = {
        "empty": (f"{n} {act}", "empty"),
        "src out of range": (f"{n} {act} 10 4", "out of range"),
        "dst out of range": (f"{n} {act} 0 10", "out of range"),
        "far out of range": (f"{n} {act} 4294967295 4", "out of range"),
        "source twice": (f"{n} {act} 0 4 0 5", "source of two"),
        "destination twice": (f"{n} {act} 0 4 1 4", "destination of two"),
        "identity and source": (f"{n} {act} 0 0 0 4", "source of two"),
        "identity and destination": (f"{n} {act} 4 4 0 4", "destination of two"),
        "active destination": (f"{n} {act} 0 1", "active"),
        "active destination, nothing paused": (f"{n} - 4 5", "active"),
        "active destination at a chain's end": (f"{n} {act} 4 0 0 1", "active"),
    }
    ok = {
        "swap": f"{n} {act} 0 1 1 0",
        "swap, nothing paused": f"{n} - 0 1 1 0",
        "active into paused": f"{n} {act} 0 4",
        "paused into paused": f"{n} {act} 4 5",
        "chain into paused": f"{n} {act} 0 1 1 4",
        "cycle": f"{n} {act} 0 1 1 2 2 0",
        "identity": f"{n} {act} 3 3",
        "identity beside a swap": f"{n} {act} 3 3 0 4 4 0",
    }
    got = run(driver, "validate", None, [c for c, _ in cases.values()] + list(ok.values()))
    for (name, (_, msg)), g in zip(cases.items(), got):
        assert msg in g, (name, g)
    for name, g in zip(ok, got[len(cases):]):
        assert g == "ok", (name, g)


# ---- the compaction rule ------------------------------------------------------------------------------------------------------------------
def expected_compaction(active, one_way):
    active = np.asarray(active, dtype=bool)
    A = int(active.sum())
    H = [s for s in range(A) if not active[s]]
    T = [s for s in range(A, len(active)) if active[s]]
    assert len(H) == len(T)
    out = []
    for h, t in zip(H, T):
        out.append((t, h))
        if not one_way: out.append((h, t))
    return out


def activity_patterns():
    S = 300
    one_hole = np.ones(S, dtype=bool); one_hole[17] = False
    return {"nothing paused": np.ones(S, dtype=bool), "everything paused": np.zeros(S, dtype=bool), "every second": np.arange(S) % 2 == 0,
            "every second, odd": np.arange(S) % 2 == 1, "one hole": one_hole, "mixed_set": ~mixed_set(S, 128), "mixed_set odd": ~mixed_set(199, 64)}


@pytest.mark.parametrize("one_way", (False, True), ids=("swap", "one-way"))
def test_compaction_rule(driver, one_way):
    pats = activity_patterns()
    got = run(driver, "compact", int(one_way), [bits(a) for a in pats.values()])
    for (name, active), g in zip(pats.items(), got):
        v = list(map(int, g.split()))
        moves = list(zip(v[0::2], v[1::2]))
        assert moves == expected_compaction(active, one_way), name
        # ... and it does what it is for
        after = active.copy()
        for s, d in moves: after[d] = active[s]
        if one_way:
            for s, d in moves: after[s] = False
        A = int(active.sum())
        assert after[:A].all() and not after[A:].any(), name
    assert got[0] == "" and got[1] == ""
    assert len(got[4].split()) == (2 if one_way else 4)


# ---- the realignment targets --------------------------------------------------------------------------------------------------------------
def test_targets(driver):
    row, n = 8, 21      # three rows, the last partial
    act = [1] * n
    for s in (2, 8, 9, 20): act[s] = 0
    cases = [
        (f"{n} {bits(act)} 0 17 17 0", {(0, 17): 16, (17, 0): 1}),                         # residents: 1 in row 0, 16 in row 2
        (f"{n} {bits(act)} 0 1 1 0 3 2", {(0, 1): 4, (1, 0): 4, (3, 2): 4}),               # 2 is paused, 3 leaves: 4 is the lowest resident
        (f"{n} - 8 0 9 1 10 2 11 3 12 4 13 5 14 6 15 7 0 8 1 9 2 10 3 11 4 12 5 13 6 14 7 15",
         {**{(8 + k, k): 8 for k in range(8)}, **{(k, 8 + k): 0 for k in range(8)}}),      # whole rows: the stream arriving at the row's lowest slot
        (f"{n} {bits(act)} 16 20 5 5 17 9", {(16, 20): 18, (17, 9): 10}),                  # an identity is a resident; paused slots never are
        (f"{n} {bits([0] * 8 + [1] * 13)} 8 3 9 1", {(8, 3): 9, (9, 1): 9}),                # a row of paused slots: the lowest DESTINATION's arrival
    ]
    got = run(driver, "targets", row, [c for c, _ in cases])
    for (case, want), g in zip(cases, got):
        v = list(map(int, g.split()))
        assert {(v[i], v[i + 1]): v[i + 2] for i in range(0, len(v), 3)} == want, case


def expected_list_targets(moves, n, row, active, listed):
    """the row-target rule (dspi_move.h) restated: per entry (src, dst, target, from_entry)"""
    out = []
    for s, d in moves:
        r = d // row
        residents = [x for x in range(r * row, min((r + 1) * row, n)) if (active is None or active[x]) and not (listed is not None and listed[x])]
        if residents:
            out.append((s, d, residents[0], 0))
        else:
            out.append((s, d, min((i for i, m in enumerate(moves) if m[1] // row == r), key=lambda i: moves[i][1]), 1))
    return out


def test_list_targets_random(driver):
    """list_targets in both call shapes — a move (no identities; its sources and destinations marked in `listed`) and a migration (listed
    null, sources in another context, every destination paused) — over 2 000 seeded lists, row width 8, up to 40 slots, mostly paused
    contexts: those are the ones that have rows without a resident.  The share of lists that reach the from_entry branch is asserted."""
    rng = np.random.default_rng(2024)
    row, cases, want = 8, [], []
    for k in range(2000):
        n = int(rng.integers(2, 41))
        active = rng.random(n) < (0.15 if k % 4 else 0.6)
        paused = np.flatnonzero(~active)
        if k % 2 == 0:      # a move: some sources; destinations among the paused slots and the sources themselves
            src = rng.permutation(n)[:int(rng.integers(1, n + 1))]
            pool = rng.permutation(np.union1d(src, paused))
            moves = [(int(s), int(d)) for s, d in zip(src, pool) if s != d] or [(0, n - 1)]
            listed = np.zeros(n, dtype=bool)
            for s, d in moves: listed[s] = listed[d] = True
        else:               # a migration: distinct paused destinations, sources from a context of its own
            if len(paused) == 0: paused = np.array([int(rng.integers(0, n))]); active[paused] = False
            dst = rng.permutation(paused)[:int(rng.integers(1, len(paused) + 1))]
            src = rng.permutation(40)[:len(dst)]
            moves, listed = [(int(s), int(d)) for s, d in zip(src, dst)], None
        cases.append(f"{n} {bits(active)} {'-' if listed is None else bits(listed)} {flat(moves)}")
        want.append(expected_list_targets(moves, n, row, active, listed))
    got = run(driver, "list_targets", row, cases)
    reached = [0, 0]
    for k, (case, w, g) in enumerate(zip(cases, want, got)):
        v = list(map(int, g.split()))
        assert [tuple(v[i:i + 4]) for i in range(0, len(v), 4)] == w, case
        reached[k % 2] += any(t[3] for t in w)
    print("lists that reach from_entry, of 1 000 each: moves", reached[0], "migrations", reached[1])
    assert reached[0] >= 250 and reached[1] >= 250, reached      # a quarter of either shape's 1 000 lists


def test_row_items(driver):
    got = run(driver, "items", 8, ["9 0 3 1 12 2 13 3 14 4 15 5 2 6"])[0].split("I")[1:]
    rows = [list(map(int, g.split())) for g in got]
    assert rows[0] == [0, 0b01, 0, -1, -1, 6, 1, -1, -1, -1, -1]
    assert rows[1] == [1, 0b11, 0b10, -1, 0, -1, -1, 2, 3, 4, 5]


# ---- host-only contexts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_context(flavor):
    S = 300
    d = Dspi(flavor, S, device=None)
    assert d.plan_compaction().shape == (0, 2)
    p = mixed_set(S, d.tile_streams())
    s = 0
    while s < S:
        if not p[s]: s += 1; continue
        e = s
        while e < S and p[e]: e += 1
        d.pause_streams(s, e - s); s = e
    for one_way in (False, True):
        want = expected_compaction(~p, one_way)
        assert [tuple(m) for m in d.plan_compaction(one_way).tolist()] == want
        n = len(want)
        buf = (C.c_uint32 * (2 * n))()
        flags = host.COMPACT_ONE_WAY if one_way else 0
        assert d.L.dspi_plan_compaction(d.h, None, 0, flags) == n                       # count only
        assert d.L.dspi_plan_compaction(d.h, buf, n - 1, flags) == host.E_SHORT and not any(buf)
        assert d.L.dspi_plan_compaction(d.h, buf, n, flags) == n and any(buf)
    assert d.L.dspi_plan_compaction(d.h, None, 0, 0x2) == host.E_INVAL
    # dspi_move_streams: a bad list is refused, a good one meets the missing device; nothing changes either way
    paused = d.streams_paused().copy()
    a0 = int(np.flatnonzero(~p)[0]); a1 = int(np.flatnonzero(~p)[1]); h0 = int(np.flatnonzero(p)[0])

    def mv(moves, flags=0):
        m = np.asarray(moves, dtype=np.uint32).reshape(-1, 2)
        return d.L.dspi_move_streams(d.h, m.ctypes.data if len(m) else None, len(m), flags)
    for bad in ([], [(a0, S)], [(S, h0)], [(a0, h0), (a0, a1)], [(a0, h0), (a1, h0)], [(a0, a1)]):
        assert mv(bad) == host.E_INVAL, bad
    assert d.L.dspi_move_streams(d.h, None, 3, 0) == host.E_INVAL
    for flags in (0x2, 0x100, 0x80000001): assert mv([(a0, h0)], flags) == host.E_INVAL
    for good in ([(a0, h0)], [(a0, a1), (a1, a0)], d.plan_compaction().tolist()):
        assert mv(good) == host.E_NODEVICE
        assert mv(good, host.MOVE_AS_IS) == host.E_NODEVICE
    with pytest.raises(DspiError) as e: d.move_streams([(a0, h0)])
    assert e.value.code == host.E_NODEVICE
    assert np.array_equal(d.streams_paused(), paused) and d.image_count() == 1
    d.close()
