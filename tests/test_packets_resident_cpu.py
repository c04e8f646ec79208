"""Resident packet tables, without a GPU: the checker's arithmetic (dspi_amd/csrc/dspi_tablecheck.h) through a g++ driver
(tests/tablecheck_driver.cpp) — the walker over every workgroup and thread, and the kernel's per-lane body with its reduction replayed lane by
lane against packets_check / packets_emit_check and against the two models written from the header's prose (tests/packets_model.py,
tests/packets_out_model.py) — and the four calls of include/dspi.h on host-only contexts: every refusal that comes before the device, in its
order, with the codes and texts of the host-table calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import packets_model as MI
import packets_out_model as MO
from dspi_amd import host
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
CALLS = ("dspi_packets_check_resident", "dspi_packets_emit_check_resident", "dspi_process_packets_resident", "dspi_packets_emit_resident", "dspi_debug_table_check_launch")
ENTRIES = (1, 2, 3, 511, 512, 513, 1025, 1200001)      # the last: three rounds of the grid-stride loop at the default cap, and a tail
CAPS = (1, 2, 3, 0)                                     # 0: the launch's default
DEFAULT_WGS, THREADS = 1024, 256
PITCH = 1600                                            # the legal tables' entries: i * PITCH, longer than any packet (192 * 8)
DUMMY = 0x1000                                          # a 16-byte aligned "device" table that nothing may dereference


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the calls"""
    assert hasattr(host.lib(), "dspi_process_packets_resident"), "libdspi_mi355x has no dspi_process_packets_resident"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes — asked of an empty program,
    so that a sanitized build of the driver that fails for any other reason fails here —, else plain; which build ran is printed (pytest -s, or
    with the failure's captured output)"""
    tmp = tmp_path_factory.mktemp("tablecheck")
    exe = tmp / "tablecheck_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "tablecheck_driver.cpp"),
           os.path.join(CSRC, "dspi_packets.cpp"), os.path.join(CSRC, "dspi_packets_out.cpp"), os.path.join(CSRC, "dspi_intake.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("tablecheck_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def nums(v): return " ".join(str(int(x)) for x in v)


# ---- the symbols and the header's words -------------------------------------------------------------------------------------------------------
def test_symbols():
    """four calls and the hook, or none; the header declares them and says what the warrant is"""
    L = host.lib()
    assert all(hasattr(L, name) for name in CALLS), [name for name in CALLS if not hasattr(L, name)]
    assert L.dspi_abi_version() == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ", "#define DSPI_TABLE_CHECKED 0x1u ",
                 "int dspi_packets_check_resident(dspi_ctx *ctx, const uint8_t *bit_depths, const uint64_t *table /* DEVICE */, uint32_t n_blocks,",
                 "int dspi_packets_emit_check_resident(dspi_ctx *ctx, const uint8_t *formats, const uint64_t *table /* DEVICE */, uint32_t n_blocks,",
                 "int dspi_process_packets_resident(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths,",
                 "int dspi_packets_emit_resident(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats,",
                 "int dspi_debug_table_check_launch(dspi_ctx *ctx,",
                 "WAITS for its 8-byte answer", "THE CALLER WARRANTS", "violated warrant is out-of-bounds access",
                 "LEFT OUT: overlap detection on device tables; depth and format vectors in device memory; a check fused into the packet kernels; arenas in\n"
                 " * host memory; an option of dspi_host.",
                 "detect by symbol (dspi_process_packets_resident;"):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()      # the kernel is the library's
    assert "dspi_tablecheck" in mk.split("KERNELS =")[1].split("\n")[0]
    assert host.TABLE_CHECKED == 1


# ---- the walker -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_stream", (1, 3))
def test_walker(driver, per_stream):
    """every entry count with every cap: the driver asserts that every index is loaded and judged exactly once with its own stream, every load
    inside the table, every pair load 16-byte aligned, the one single load the tail of an odd count, no index at or above `entries` judged;
    here the grid and the loop are held to what the counts say they must be"""
    cases = [(e, cap) for e in ENTRIES for cap in CAPS]
    got = run(driver, [f"walk {e} {per_stream} {cap}" for e, cap in cases])
    for (e, cap), line in zip(cases, got):
        assert line.startswith("ok "), (e, cap, line)
        wgs, pairs, tails, max_it = map(int, line.split()[1:])
        want_wgs = min(max(1, -(-(e // 2) // THREADS)), cap or DEFAULT_WGS)
        assert (wgs, pairs, tails) == (want_wgs, e // 2, e % 2), (e, cap, line)
        assert max_it == -(-(e // 2) // (want_wgs * THREADS)), (e, cap, line)      # the loop's rounds: the first thread's
    # several rounds at small sizes, which the GPU suite repeats on the device, and three at the default cap
    assert dict(zip(cases, got))[(1025, 1)].split()[4] == "2" and dict(zip(cases, got))[(1200001, 0)].split()[4] == "3"


# ---- the answer -------------------------------------------------------------------------------------------------------------------------------
def legal(n, per): return [[PITCH * (s * per + i) for i in range(per)] for s in range(n)]


def answer_cases():
    """(kind, n, P, nb, bl, arena_bytes, kinds, active, table) with the name of the case"""
    rng = np.random.default_rng(5)
    out = []
    for kind, n, P, nb, a, b in ((0, 130, 1, 4, 16, 24), (1, 70, 2, 4, 24, 32), (0, 43, 1, 3, 16, 24), (1, 43, 1, 3, 24, 32), (0, 130, 1, 12, 16, 24)):
        per, bl = P * nb, (45 if n != 70 else 96)
        kinds = [int(x) for x in rng.choice((a, b), n)]
        size = lambda s: bl * (MO.frame_bytes(kinds[s]) if kind else MI.frame_bytes(kinds[s]))
        E, ab = n * per, PITCH * n * per
        everyone = [1] * n

        def with_bad(where, value=lambda s: 301):
            t = legal(n, per)
            for i in where:
                if i < E: t[i // per][i % per] = value(i // per)      # (the small tables have fewer entries than some of the spots)
            return t
        out.append(("none", kind, n, P, nb, bl, ab, kinds, everyone, legal(n, per)))
        spots = [0, E - 1] + [i for i in (511, 512, 513) if i < E]
        for i in spots: out.append((f"one at {i}", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([i])))
        out.append(("several", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([E - 1, 77, 300, 78, E // 2])))
        out.append(("a neighbour pair", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([100, 101])))
        paused = [3, 17, n - 1]
        active = [0 if s in paused else 1 for s in range(n)]
        out.append(("paused rows only", kind, n, P, nb, bl, ab, kinds, active, with_bad([s * per + i for s in paused for i in range(per)], lambda s: 2 ** 63 + 1)))
        out.append(("paused rows and one more", kind, n, P, nb, bl, ab, kinds, active, with_bad([s * per + i for s in paused for i in range(per)] + [18 * per + 1], lambda s: 2 ** 63 + 1)))
        out.append(("SKIP entries", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([40, 9, E - 2], lambda s: MO.SKIP)))
        out.append(("2^63 and above", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([E - 3, 200], lambda s: 2 ** 63 + 2 * s)))
        out.append(("2^64 - 2", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([64], lambda s: 2 ** 64 - 2)))
        out.append(("two bytes past the arena", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([E - 1, 129], lambda s: ab - size(s) + 2)))
        out.append(("ending with the arena", kind, n, P, nb, bl, ab, kinds, everyone, with_bad([E - 1, 129], lambda s: ab - size(s))))
        out.append(("bytes > arena_bytes", kind, n, P, nb, bl, 100, kinds, active, legal(n, per)))
        out.append(("an empty arena", kind, n, P, nb, bl, 0, kinds, everyone, [[0] * per for _ in range(n)]))
    return out


def test_answer_equals_the_host_check_and_the_models(driver):
    """the kernel's per-lane arithmetic and its reduction, lane by lane on the CPU, at caps 1, 2 and the default: the word equals *at of
    packets_check / packets_emit_check wherever they say Entry and is all ones wherever they say Ok, and both equal the models"""
    cases = [c + (cap,) for c in answer_cases() for cap in (1, 2, 0)]
    got = run(driver, [f"answer {kind} {n} {P} {nb} {bl} {ab} {cap} {nums(kinds)} {nums(active)} {nums(x for r in tab for x in r)}" for _, kind, n, P, nb, bl, ab, kinds, active, tab, cap in cases])
    seen = set()
    for (name, kind, n, P, nb, bl, ab, kinds, active, tab, cap), line in zip(cases, got):
        act = None if all(active) else active
        want = MO.check(kinds, tab, P, nb, bl, ab, act) if kind else MI.check(kinds, tab, nb, bl, ab, act)
        assert want is None or want[0] == "entry", (name, want)
        word, verdict = line.split(" ", 1)
        assert verdict == ("ok" if want is None else f"entry {want[1]}"), (name, kind, n, cap, line)
        assert word == ("none" if want is None else str(want[1])), (name, kind, n, cap, line)
        seen.add((name, kind, want is None))
    # what the cases are there for
    for kind in (0, 1):
        assert ("paused rows only", kind, True) in seen and ("paused rows and one more", kind, False) in seen and ("ending with the arena", kind, True) in seen
        assert ("SKIP entries", kind, bool(kind)) in seen      # legal in an emit table, illegal in an input table
        for name in ("one at 0", "one at 511", "one at 512", "one at 513", "several", "2^63 and above", "2^64 - 2", "two bytes past the arena", "bytes > arena_bytes", "an empty arena"):
            assert (name, kind, False) in seen, (name, kind)
    by = {(c[0], c[1], c[2], c[4], c[-1]): l for c, l in zip(cases, got)}
    assert by[("several", 0, 130, 4, 0)].startswith("77 ") and by[("a neighbour pair", 1, 70, 4, 1)].startswith("100 ")
    assert by[("one at 128", 0, 43, 3, 2)].startswith("128 ")                      # the tail of an odd count
    assert by[("bytes > arena_bytes", 0, 130, 4, 0)].startswith("0 ") and by[("several", 0, 130, 12, 1)].startswith("77 ")


# ---- the calls on host-only contexts: every refusal that comes before the device, in its order ---------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_process_refusals_in_their_order(flavor):
    """dspi_process_packets_resident and dspi_packets_check_resident: 1 to 4 as dspi_process_packets / dspi_packets_check give them (code and
    text, the call's name apart), the table_flags rule with the flag rule, then DSPI_E_NODEVICE — the table pointer is never dereferenced"""
    S, F, NB, AB = 12, 48, 2, 100000
    d = Dspi(flavor, S, device=None)
    good = np.array([16, 24] * (S // 2), dtype=np.uint8)
    worse = good.copy(); worse[9] = 32; worse[11] = 8
    table = np.array(legal(S, NB), dtype=np.uint64)
    out = host._Out(DUMMY, None, None, None)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    res = lambda ar, dp, t, nb, bl, o, flags, tf=0: d.L.dspi_process_packets_resident(d.h, ar, AB, dp.ctypes.data if dp is not None else None, t, nb, bl, C.byref(o) if o else None, None, flags, tf)
    hst = lambda ar, dp, t, nb, bl, o, flags: d.L.dspi_process_packets(d.h, ar, AB, dp.ctypes.data if dp is not None else None, t, nb, bl, C.byref(o) if o else None, None, flags)

    def both(ar, dp, t_res, nb, bl, o, flags, code, word):
        """the resident call and the host-table call refuse alike"""
        rc = res(ar, dp, t_res, nb, bl, o, flags); text = err()
        assert rc == code and word in text, (rc, text)
        assert hst(ar, dp, table.ctypes.data if t_res else None, nb, bl, o, flags) == code and err() == text.replace("dspi_process_packets_resident", "dspi_process_packets")
    M = host.MEM_DEVICE
    # 1. a NULL ctx; DSPI_MEM_DEVICE missing; the flag rule; then table_flags — all before a pointer, a length or a depth is looked at
    assert d.L.dspi_process_packets_resident(None, DUMMY, AB, good.ctypes.data, DUMMY, NB, F, C.byref(out), None, M, 0) == host.E_INVAL
    both(None, worse, None, 0, 193, None, 0, host.E_INVAL, "DSPI_MEM_DEVICE is required")
    both(None, worse, None, 0, 193, None, M | 0x40000000, host.E_INVAL, "flag")
    both(None, worse, None, 0, 193, None, M | host.OUT_WIRE | host.OUT_I2S_SLOTS, host.E_INVAL, "DSPI_OUT_WIRE")
    for tf in (2, 0x80000000, 3):
        assert res(None, worse, None, 0, 193, None, M, tf) == host.E_INVAL and "table_flags" in err(), tf
        assert res(None, worse, None, 0, 193, None, 0, tf) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()      # (the flags first)
    # 2. the pointers and the lengths: before a depth
    for ar, dp, t, o in ((None, worse, DUMMY, out), (DUMMY, None, DUMMY, out), (DUMMY, worse, None, out), (DUMMY, worse, DUMMY, None)):
        both(ar, dp, t, NB, F, o, M, host.E_INVAL, "required")
    for nb, bl in ((0, F), (NB, 0), (NB, 193)):
        both(DUMMY, worse, DUMMY, nb, bl, out, M, host.E_INVAL, "block_len")
    # 3. a depth, the lowest stream first: before the entry count
    both(DUMMY, worse, DUMMY, NB, F, out, M, host.E_INVAL, "stream 9")
    both(DUMMY, worse, DUMMY, 2 ** 31 // S + 1, F, out, M, host.E_INVAL, "stream 9")
    # 4. the entry count: before the device (the host-table call does not read its table here either)
    both(DUMMY, good, DUMMY, 2 ** 31 // S + 1, F, out, M, host.E_INVAL, "2^31 - 1 entries")
    # then DSPI_E_NODEVICE, with either route and whatever the table's alignment: the text of every audio call
    for tf in (0, host.TABLE_CHECKED):
        for t in (DUMMY, DUMMY + 8):
            assert res(DUMMY, good, t, NB, F, out, M, tf) == host.E_NODEVICE
            text = err()
            assert hst(DUMMY, good, table.ctypes.data, NB, F, out, M) == host.E_NODEVICE and err() == text
    # the check call: 2 to 4 as dspi_packets_check, then DSPI_E_NODEVICE; *bad_entry is not written
    bad = C.c_uint64(12345)
    chk = lambda dp, t, nb, bl: d.L.dspi_packets_check_resident(d.h, dp.ctypes.data if dp is not None else None, t, nb, bl, AB, C.byref(bad))
    hck = lambda dp, nb, bl: d.L.dspi_packets_check(d.h, dp.ctypes.data, table.ctypes.data, nb, bl, AB, None)
    assert d.L.dspi_packets_check_resident(None, good.ctypes.data, DUMMY, NB, F, AB, None) == host.E_INVAL
    assert chk(None, DUMMY, NB, F) == host.E_INVAL and chk(good, None, NB, F) == host.E_INVAL
    for dp, nb, bl, word in ((worse, 0, F, "block_len"), (worse, NB, 193, "block_len"), (worse, NB, F, "stream 9"), (good, 2 ** 31 // S + 1, F, "2^31 - 1 entries")):
        assert chk(dp, DUMMY, nb, bl) == host.E_INVAL and word in err()
        text = err()
        assert hck(dp, nb, bl) == host.E_INVAL and err() == text.replace("dspi_packets_check_resident", "dspi_packets_check")
    assert chk(good, DUMMY, NB, F) == host.E_NODEVICE and chk(good, DUMMY + 8, NB, F) == host.E_NODEVICE and "host-only" in err()
    assert bad.value == 12345
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_emit_refusals_in_their_order(flavor):
    """dspi_packets_emit_resident and dspi_packets_emit_check_resident: 1 to 4 as dspi_packets_emit / dspi_packets_emit_check give them, with
    DSPI_MEM_DEVICE required and the table_flags rule in 1, check_flags != 0 refused, then DSPI_E_NODEVICE"""
    S, F, NB, AB = 12, 48, 2, 200000
    d = Dspi(flavor, S, device=None)
    P = d.P
    good = np.array([24, 32] * (S // 2), dtype=np.uint8)
    worse = good.copy(); worse[9] = 16; worse[11] = 8
    table = np.array(legal(S, P * NB), dtype=np.uint64)
    pairs = np.zeros(S * P * NB * F * 2, dtype=np.int32)
    pattern = (np.arange(AB) * 7 + 3).astype(np.uint8)
    arena = pattern.copy()
    err = lambda: d.L.dspi_last_error(d.h).decode()
    ptr = lambda a: a.ctypes.data if a is not None else None
    res = lambda pr, fm, t, ar, nb, bl, flags, tf=0: d.L.dspi_packets_emit_resident(d.h, ptr(pr), nb, bl, ptr(fm), t, ptr(ar), AB, flags, tf)
    hst = lambda pr, fm, t, ar, nb, bl, flags: d.L.dspi_packets_emit(d.h, ptr(pr), nb, bl, ptr(fm), t, ptr(ar), AB, flags)

    def both(pr, fm, t_res, ar, nb, bl, flags, word):
        rc = res(pr, fm, t_res, ar, nb, bl, flags); text = err()
        assert rc == host.E_INVAL and word in text, (rc, text)
        assert hst(pr, fm, table.ctypes.data if t_res else None, ar, nb, bl, flags) == host.E_INVAL and err() == text.replace("dspi_packets_emit_resident", "dspi_packets_emit")
    M = host.MEM_DEVICE
    # 1. a NULL ctx; an undefined flag bit; DSPI_MEM_DEVICE missing (the CPU path stays with host tables); table_flags
    assert d.L.dspi_packets_emit_resident(None, ptr(pairs), NB, F, ptr(good), DUMMY, ptr(arena), AB, M, 0) == host.E_INVAL
    for flags in (0x4, 0x80000000, M | host.OUT_SPDIF, host.OUT_TILED | host.OUT_WIRE, host.OUT_I2S_SLOTS):
        both(None, worse, None, None, 0, 193, flags, "flags")
    for flags in (0, host.OUT_TILED):
        assert res(None, worse, None, None, 0, 193, flags) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    for tf in (2, 0x80000000, 3):
        assert res(None, worse, None, None, 0, 193, M, tf) == host.E_INVAL and "table_flags" in err(), tf
    # 2. the pointers and the lengths: before a format
    for pr, fm, t, ar in ((None, worse, DUMMY, arena), (pairs, None, DUMMY, arena), (pairs, worse, None, arena), (pairs, worse, DUMMY, None)):
        both(pr, fm, t, ar, NB, F, M, "required")
    for nb, bl in ((0, F), (NB, 0), (NB, 193)):
        both(pairs, worse, DUMMY, arena, nb, bl, M | host.OUT_TILED, "block_len")
    # 3. a format, the lowest stream first; 4. the entry count
    both(pairs, worse, DUMMY, arena, NB, F, M, "stream 9")
    both(pairs, worse, DUMMY, arena, 2 ** 31 // (S * P) + 1, F, M, "stream 9")
    both(pairs, good, DUMMY, arena, 2 ** 31 // (S * P) + 1, F, M, "2^31 - 1 entries")
    # then DSPI_E_NODEVICE: before any alignment is looked at, with either route; the text is dspi_packets_emit's
    for tf in (0, host.TABLE_CHECKED):
        for t in (DUMMY, DUMMY + 8):
            assert res(pairs, good, t, arena, NB, F, M, tf) == host.E_NODEVICE
            text = err()
            assert hst(pairs, good, table.ctypes.data, arena, NB, F, M) == host.E_NODEVICE and err() == text.replace("dspi_packets_emit_resident", "dspi_packets_emit")
    assert np.array_equal(arena, pattern)
    # the check call: check_flags first (the overlap rule stays with host tables), then 2 to 4, then DSPI_E_NODEVICE
    bad = C.c_uint64(12345)
    chk = lambda fm, t, nb, bl, cf=0: d.L.dspi_packets_emit_check_resident(d.h, ptr(fm), t, nb, bl, AB, cf, C.byref(bad))
    assert d.L.dspi_packets_emit_check_resident(None, ptr(good), DUMMY, NB, F, AB, 0, None) == host.E_INVAL
    for cf in (host.EMIT_CHECK_OVERLAP, 2, 0x80000000):
        assert chk(None, None, 0, 193, cf) == host.E_INVAL and "check_flags" in err(), cf
    assert chk(None, DUMMY, NB, F) == host.E_INVAL and "required" in err() and chk(good, None, NB, F) == host.E_INVAL and "required" in err()
    for fm, nb, bl, word in ((worse, 0, F, "block_len"), (worse, NB, 193, "block_len"), (worse, NB, F, "stream 9"), (good, 2 ** 31 // (S * P) + 1, F, "2^31 - 1 entries")):
        assert chk(fm, DUMMY, nb, bl) == host.E_INVAL and word in err()
        text = err()
        assert d.L.dspi_packets_emit_check(d.h, ptr(fm), table.ctypes.data, nb, bl, AB, 0, None) == host.E_INVAL and err() == text.replace("dspi_packets_emit_check_resident", "dspi_packets_emit_check")
    assert chk(good, DUMMY, NB, F) == host.E_NODEVICE and chk(good, DUMMY + 8, NB, F) == host.E_NODEVICE and "host-only" in err()
    assert bad.value == 12345
    # the timing hook on a host-only context: its arguments, then DSPI_E_NODEVICE
    assert d.L.dspi_debug_table_check_launch(d.h, 2, DUMMY, DUMMY, NB, F, AB) == host.E_INVAL and d.L.dspi_debug_table_check_launch(d.h, 1, DUMMY, DUMMY + 8, NB, F, AB) == host.E_INVAL
    assert d.L.dspi_debug_table_check_launch(d.h, 1, DUMMY, DUMMY, NB, F, AB) == host.E_NODEVICE
    d.close()
