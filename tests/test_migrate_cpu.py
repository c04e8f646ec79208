"""Migration between two contexts without a GPU: the list rules, the rebalancing plan, the realignment targets and the batches
(dspi_amd/csrc/dspi_migrate.{h,cpp}) through a g++ driver (tests/migrate_driver.cpp), and the two calls of include/dspi.h on host-only
contexts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dspi_amd import host, workloads as WL
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("migrate") / "migrate_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "migrate_driver.cpp"),
                    os.path.join(CSRC, "dspi_migrate.cpp"), os.path.join(CSRC, "dspi_move.cpp")], check=True)
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


def pairs_of(line):
    v = list(map(int, line.split()))
    return list(zip(v[0::2], v[1::2]))


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_migrate_streams") and hasattr(L, "dspi_plan_migration")
    assert host.MIGRATE_AS_IS == 1 and host.MIGRATE_PAUSED == 2
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_MIGRATE_AS_IS  0x1u", "#define DSPI_MIGRATE_PAUSED 0x2u",
                 "int dspi_migrate_streams(dspi_ctx *src, dspi_ctx *dst, const dspi_stream_move *moves, uint32_t n, uint32_t flags);",
                 "int dspi_plan_migration(const dspi_ctx *src, const dspi_ctx *dst, uint32_t want, dspi_stream_move *moves, uint32_t cap, uint32_t flags);"):
        assert word in text, word
    assert text.index("stream moves: a stream changes its slot") < text.index("dspi_migrate_streams") < text.index("grouping: streams of one preset")


# ---- validation ---------------------------------------------------------------------------------------------------------------------------
def test_validation(driver):
    ns, nd = 12, 10
    act = bits([1, 1, 1, 1, 0, 0, 1, 1, 0, 0])      # the destination context: 4, 5, 8, 9 are paused
    cases = {
        "empty": (f"{ns} {nd} {act}", "empty"),
        "source out of range": (f"{ns} {nd} {act} 12 4", "source index out of range"),
        "destination out of range": (f"{ns} {nd} {act} 0 10", "destination index out of range"),
        "a source the destination context would have": (f"{nd} {ns} {act}11 11 4", "source index out of range"),
        "far out of range": (f"{ns} {nd} {act} 4294967295 4", "source index out of range"),
        "source twice": (f"{ns} {nd} {act} 0 4 0 5", "source of two"),
        "destination twice": (f"{ns} {nd} {act} 0 4 1 4", "destination of two"),
        "active destination": (f"{ns} {nd} {act} 0 4 1 6", "active"),
        "active destination, nothing paused": (f"{ns} {nd} - 4 5", "active"),
    }
    ok = {
        "one": f"{ns} {nd} {act} 0 4",
        "the same number on both sides": f"{ns} {nd} {act} 4 4 5 5",
        "crossing": f"{ns} {nd} {act} 9 4 4 9 11 8",
        "all paused slots": f"{ns} {nd} {act} 0 9 1 8 2 5 3 4",
    }
    got = run(driver, "validate", None, [c for c, _ in cases.values()] + list(ok.values()))
    for (name, (_, msg)), g in zip(cases.items(), got):
        assert msg in g, (name, g)
    for name, g in zip(ok, got[len(cases):]):
        assert g == "ok", (name, g)


# ---- the realignment targets --------------------------------------------------------------------------------------------------------------
def test_targets(driver):
    row, n = 8, 21      # the destination context: three rows, the last partial
    act = [1] * n
    for s in (2, 5, 17, 19, 20): act[s] = 0       # row 0: residents 0, 1, ...; row 2: residents 16, 18
    for s in range(8, 16): act[s] = 0             # row 1: nobody
    cases = [
        # a row with a resident: the lowest one, whatever the arrivals
        (f"{n} {bits(act)} 40 5 41 2", [(5, 0, 0), (2, 0, 0)]),
        # a row with none, whose lowest destination is not the list's first entry: entry 2 (source 9 -> 9) supplies the pair
        (f"{n} {bits(act)} 7 12 3 15 9 9 30 2", [(12, 2, 1), (15, 2, 1), (9, 2, 1), (2, 0, 0)]),
        # a partial last row: its residents are below n only; all of it paused: the arrival at its lowest destination
        (f"{n} {bits(act)} 1 20 2 17", [(20, 16, 0), (17, 16, 0)]),
        (f"{n} {bits(act[:16] + [0] * 5)} 1 20 2 19 5 2", [(20, 1, 1), (19, 1, 1), (2, 0, 0)]),
        # resident 0 is paused: the next active slot of the row
        (f"{n} {bits([0, 0, 0, 1] + act[4:])} 6 1 8 0", [(1, 3, 0), (0, 3, 0)]),
    ]
    got = run(driver, "targets", row, [c for c, _ in cases])
    for (case, want), g in zip(cases, got):
        v = list(map(int, g.split()))
        assert [tuple(v[i:i + 3]) for i in range(0, len(v), 3)] == want, case


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def expected_plan(src_active, dst_active, want):
    """the rule of include/dspi.h, restated"""
    a = [s for s in range(len(src_active)) if src_active[s]]
    p = [s for s in range(len(dst_active)) if not dst_active[s]]
    k = min(want, len(a), len(p))
    return list(zip(sorted(a[len(a) - k:]) if k else [], p[:k]))


def test_plan_by_hand(driver):
    src = [1, 1, 0, 1, 1, 0, 1, 0]      # active: 0 1 3 4 6
    dst = [1, 0, 0, 1, 0, 1, 0, 0, 0]   # paused: 1 2 4 6 7 8
    cases = [
        (3, bits(src), bits(dst), [(3, 1), (4, 2), (6, 4)]),            # limited by `want`
        (9, bits(src), bits(dst), [(0, 1), (1, 2), (3, 4), (4, 6), (6, 7)]),      # limited by the source's active streams
        (9, bits(src), bits([1, 0, 1, 1, 0, 1]), [(4, 1), (6, 4)]),     # limited by the destination's paused slots
        (0, bits(src), bits(dst), []),
        (4, bits(src), "-6", []),                                        # nothing paused at the destination
        (2, "-5", bits(dst), [(3, 1), (4, 2)]),                          # nothing paused at the source
        (5, bits([0] * 4), bits(dst), []),
    ]
    for want, s, d, exp in cases:
        got = pairs_of(run(driver, "plan", want, [f"{s} {d}"])[0])
        assert got == exp, (want, s, d, got)


def test_plan_random(driver):
    rng = np.random.default_rng(2025)
    by_want = {}
    for i in range(300):
        ns, nd = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sa = rng.random(ns) < rng.random(); da = rng.random(nd) < rng.random()
        if not da.all() and i % 3 == 0: da[np.flatnonzero(~da)[0]:] = False      # (a context with a paused tail, as after a grow)
        n_act, n_free = int(sa.sum()), int((~da).sum())
        want = [int(rng.integers(0, 80)), n_act, n_free, max(0, min(n_act, n_free) - 1)][i % 4]
        by_want.setdefault(want, []).append((sa, da))
    limited = {"want": 0, "active": 0, "paused": 0}
    for want, pops in by_want.items():
        got = run(driver, "plan", want, [f"{bits(sa) if not sa.all() else '-%d' % len(sa)} {bits(da) if not da.all() else '-%d' % len(da)}" for sa, da in pops])
        checks = []
        for (sa, da), g in zip(pops, got):
            moves = pairs_of(g)
            assert moves == expected_plan(sa, da, want), (want, bits(sa), bits(da), moves)
            k, n_act, n_free = len(moves), int(sa.sum()), int((~da).sum())
            assert k == min(want, n_act, n_free)
            if k and k == want and k < n_act and k < n_free: limited["want"] += 1
            if k and k == n_act and k < want and k < n_free: limited["active"] += 1
            if k and k == n_free and k < want and k < n_act: limited["paused"] += 1
            # order is kept on both sides, and the source's remaining active streams all lie below the chosen ones
            assert moves == sorted(moves) and [d for _, d in moves] == sorted(d for _, d in moves)
            chosen = {s for s, _ in moves}
            if k: assert all(s < moves[0][0] for s in range(len(sa)) if sa[s] and s not in chosen)
            if k: checks.append(f"{len(sa)} {len(da)} {bits(da)} {flat(moves)}")
        # ... and the validation accepts every list the plan writes
        for c, g in zip(checks, run(driver, "validate", None, checks) if checks else []): assert g == "ok", (c, g)
    assert all(v > 5 for v in limited.values()), limited      # k met each of its three bounds alone


# ---- the batches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (2, 3, 9))
def test_batches(driver, cap):
    moves = [(40 - 3 * i, 5 + 7 * i) for i in range(9)]
    tok = run(driver, "batches", cap, [flat(moves)])[0].split("B")[1:]
    assert len(tok) == -(-9 // cap)
    at = 0
    for t in tok:
        v = t.split()
        ent = [(v[i], int(v[i + 1]), int(v[i + 2])) for i in range(0, len(v), 3)]
        k = len(ent) // 2
        assert k == min(cap, 9 - at)      # consecutive pieces of the list, full but for the last
        assert ent[:k] == [("g", moves[at + j][0], j) for j in range(k)] and ent[k:] == [("s", moves[at + j][1], j) for j in range(k)]
        at += k
    assert at == 9


# ---- host-only contexts -------------------------------------------------------------------------------------------------------------------
def _books(d):
    return (d.streams_paused().tobytes(), d.image_count(), tuple(d.collect_bulk(s) for s in range(d.n_streams)))


@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_contexts(flavor):
    Ss, Sd = 40, 30
    src, dst = Dspi(flavor, Ss, device=None), Dspi(flavor, Sd, device=None)
    other = WL.full_chain_blob(flavor)
    assert src.load_bulk(other, stream=37) == 0 and dst.load_bulk(other, stream=3) == 0
    # nothing paused at the destination: nothing to plan
    assert src.plan_migration(dst, 5).shape == (0, 2)
    src.pause_streams(10, 5); src.pause_streams(38, 2)
    dst.pause_streams(2, 3); dst.pause_streams(20, 10)
    sa = ~src.streams_paused().astype(bool); da = ~dst.streams_paused().astype(bool)
    for want in (0, 4, 13, 33, 100):
        exp = expected_plan(sa, da, want)
        assert [tuple(m) for m in src.plan_migration(dst, want).tolist()] == exp, want
    n = 4
    buf = (C.c_uint32 * (2 * n))()
    L = src.L
    assert L.dspi_plan_migration(src.h, dst.h, n, None, 0, 0) == n                      # count only
    assert L.dspi_plan_migration(src.h, dst.h, n, buf, n - 1, 0) == host.E_SHORT and not any(buf)
    assert L.dspi_plan_migration(src.h, dst.h, n, buf, n, 0) == n and list(buf) == [34, 2, 35, 3, 36, 4, 37, 20]
    assert L.dspi_plan_migration(src.h, dst.h, n, buf, n, 1) == host.E_INVAL
    assert L.dspi_plan_migration(None, dst.h, n, buf, n, 0) == host.E_INVAL and L.dspi_plan_migration(src.h, None, n, buf, n, 0) == host.E_INVAL
    q = Dspi(1 - flavor, 8, device=None); q.pause_streams(0, 8)
    assert L.dspi_plan_migration(src.h, q.h, n, buf, n, 0) == host.E_INVAL
    # dspi_migrate_streams: a bad list is refused, a good one meets the missing device; neither context changes either way
    before = (_books(src), _books(dst))

    def mg(moves, flags=0, a=src, b=dst):
        m = np.asarray(moves, dtype=np.uint32).reshape(-1, 2)
        return L.dspi_migrate_streams(a.h if a else None, b.h if b else None, m.ctypes.data if len(m) else None, len(m), flags)
    for bad in ([], [(Ss, 2)], [(0, Sd)], [(0, 35)], [(0, 2), (0, 3)], [(0, 2), (1, 2)], [(0, 5)], [(0, 2), (1, 0)]):
        assert mg(bad) == host.E_INVAL, bad
        assert "dspi_migrate_streams" in src.L.dspi_last_error(src.h).decode() and src.L.dspi_last_error(src.h) == dst.L.dspi_last_error(dst.h)
    assert L.dspi_migrate_streams(src.h, dst.h, None, 3, 0) == host.E_INVAL
    for flags in (0x4, 0x100, 0x80000001): assert mg([(0, 2)], flags) == host.E_INVAL
    assert mg([(0, 2)], a=None) == host.E_INVAL and mg([(0, 2)], b=None) == host.E_INVAL
    assert mg([(0, 2)], b=src) == host.E_INVAL and mg([(2, 0)], a=dst, b=dst) == host.E_INVAL      # one context on both sides
    assert mg([(0, 0)], b=q) == host.E_INVAL                                                       # flavours differ
    if flavor:
        f = Dspi(host_flavor_fma(), 8, device=None); f.pause_streams(0, 8)
        assert mg([(0, 0)], b=f) == host.E_INVAL                                                   # float contracts differ
        f.close()
    for good in ([(0, 2)], [(12, 3), (37, 29)], src.plan_migration(dst, 100).tolist()):
        for flags in (0, host.MIGRATE_AS_IS, host.MIGRATE_PAUSED, host.MIGRATE_AS_IS | host.MIGRATE_PAUSED):
            assert mg(good, flags) == host.E_NODEVICE
    with pytest.raises(DspiError) as e: src.migrate_streams(dst, [(0, 2)])
    assert e.value.code == host.E_NODEVICE
    assert (_books(src), _books(dst)) == before
    for d in (src, dst, q): d.close()


def host_flavor_fma():
    from dspi_amd import wire as W
    return W.F32_FMA
