"""Outputs to a packet table, without a GPU: dspi_amd/csrc/dspi_packets_out.{h,cpp} through a g++ driver (tests/packets_out_driver.cpp) against the
model written from the header's prose (tests/packets_out_model.py) — the check in its order with the overlap rule, the arena that
packets_emit_cpu leaves from either source layout, and both kernels' address arithmetic walked for every workgroup, lane group, lane and
iteration — and the two calls of include/dspi.h on host-only contexts: every refusal in its order, and the host path against the model."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import packets_out_model as M
from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
BLOCK_LENS = (1, 2, 7, 44, 45, 96, 168, 169, 192)
N_BLOCKS = 3
FLEETS = ((130, 4, 128), (70, 2, 64))      # (streams, pairs, R): the float flavour (a tile of 128 plus two columns), the Q28 one (64 + 6)
ILLEGAL = 2 ** 63 + 1                      # what a paused stream's row holds


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the call"""
    assert hasattr(host.lib(), "dspi_packets_emit"), "libdspi_mi355x has no dspi_packets_emit"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes — asked of an empty program,
    so that a sanitized build of the driver that fails for any other reason fails here —, else plain; which build ran is printed (pytest -s, or
    with the failure's captured output)"""
    tmp = tmp_path_factory.mktemp("packets_out")
    exe = tmp / "packets_out_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "packets_out_driver.cpp"),
           os.path.join(CSRC, "dspi_packets_out.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("packets_out_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def arena_bytes(seed, n):
    """the driver's arena: byte i of an arena made with `seed`"""
    i = np.arange(n, dtype=np.uint64)
    return ((i * 131 + seed * 17 + (i >> 8) * 7 + 1) & 0xff).astype(np.uint8)


def source(seed, n, P, F, R):
    """the driver's source: word i of the buffer made with `seed`, in the layout's shape"""
    shape = ((n + R - 1) // R, 2 * P, F, R) if R else (n, P, F, 2)
    i = np.arange(int(np.prod(shape)), dtype=np.uint64)
    w = (i * 2654435761 + seed * 40503 + (i >> 7) * 97 + 12345) & 0xffffffff
    return w.astype(np.uint32).view(np.int32).reshape(shape)


def flat(rows): return " ".join(str(int(x)) for r in rows for x in r)
def nums(v): return " ".join(str(int(x)) for x in v)


def make_table(r, formats, P, n_blocks, block_len, paused=(), skip=0.1):
    """(table rows, arena_bytes): the live entries in shuffled order, one behind the other — a third of them touching their predecessor, the
    others at the next address of a residue that walks through every even residue mod 16 —, a tenth of the entries SKIP, a paused stream's row
    full of illegal offsets; the arena ends exactly with the last entry"""
    n = len(formats)
    tab = [[M.SKIP] * (P * n_blocks) for _ in range(n)]
    live = [(s, i) for s in range(n) if s not in paused for i in range(P * n_blocks) if r.random() >= skip]
    r.shuffle(live)
    at, res = 2 * r.randrange(0, 8), 0
    for s, i in live:
        if r.random() >= 1 / 3:
            res = (res + 2) % 16
            at += (res - at) % 16
        tab[s][i] = at
        at += block_len * M.frame_bytes(formats[s])
    for s in paused: tab[s] = [ILLEGAL] * (P * n_blocks)
    return tab, at


def fleet_case(r, n, P, R, block_len, with_paused):
    formats = [r.choice((24, 32)) for _ in range(n)]
    paused = sorted(r.sample(range(n), 5)) + [n - 1] if with_paused else []
    tab, ab = make_table(r, formats, P, N_BLOCKS, block_len, set(paused))
    active = [0 if s in paused else 1 for s in range(n)]
    return formats, active, tab, ab


# ---- the symbols and the header's words -------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_packets_emit", "dspi_packets_emit_check"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "#define DSPI_PACKET_SKIP UINT64_MAX ", "#define DSPI_EMIT_CHECK_OVERLAP 0x1u ",
                 "int dspi_packets_emit_check(const dspi_ctx *ctx, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len,\n"
                 "                            uint64_t arena_bytes, uint32_t check_flags, uint64_t *bad_entry /* may be NULL */);",
                 "int dspi_packets_emit(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats,\n"
                 "                      const uint64_t *table, void *arena, uint64_t arena_bytes, uint32_t flags);",
                 "dspi_packets_emit is the packetiser that the packet-table section above leaves out",
                 "table[(s * n_pairs + p) * n_blocks + k] is the byte",
                 "the caller may reuse its emit table when the call returns",
                 "AN EMIT ENTRY IS LEGAL when it is DSPI_PACKET_SKIP, or when it is even and offset + block_len * frame bytes <= arena_bytes",
                 "Entries of one call must not overlap each other or the source; the call does not check this",
                 "nothing outside the union of the entries is written",
                 "Rows of PAUSED streams are neither read nor checked, their source columns are not read, and nothing is written for them",
                 "AN EMIT TABLE CAN BE THE NEXT CONTEXT'S INPUT TABLE",
                 "the first illegal emit entry of an active stream, in table order",
                 "dspi_packets_emit_check applies refusals 2 to 5",
                 "LEFT OUT of the packetiser: the sub channel; wire-layout and S/PDIF sources; 16-bit packets; per-packet lengths; tables in device memory; a\n"
                 " * fused process-and-emit call; an option of dspi_host.",
                 "detect by symbol (dspi_packets_emit; with it dspi_packets_emit_check; additions only)",
                 # the packet-table section's own sentence stands as it stood
                 "packet-table OUTPUT (a packetiser); per-packet lengths (block_len is one number per call); an option of dspi_host."):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()      # the module and the kernel are the library's
    assert "dspi_packets_out" in mk.split("HOST =")[1].split("\n")[0] and "dspi_packettx" in mk.split("KERNELS =")[1].split("\n")[0]
    assert host.PACKET_SKIP == M.SKIP and host.EMIT_CHECK_OVERLAP == 1


# ---- packets_emit_cpu and the walker against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_len", BLOCK_LENS)
def test_emit_cpu_equals_the_model(driver, block_len):
    """both fleets, both source layouts, mixed formats, a shuffled table with every even residue mod 16, SKIP entries and paused streams whose
    rows hold illegal offsets: the whole arena, the pattern between and around the entries included"""
    r = random.Random(block_len)
    cases = []
    for n, P, R in FLEETS:
        for layout in (0, R):
            formats, active, tab, ab = fleet_case(r, n, P, R, block_len, True)
            cases.append((n, P, layout, formats, active, tab, ab, r.randrange(1, 1000)))
    got = run(driver, [f"emit {n} {P} {N_BLOCKS} {block_len} {R} {ab} {seed} {nums(f)} {nums(a)} {flat(tab)}" for n, P, R, f, a, tab, ab, seed in cases])
    for (n, P, R, f, a, tab, ab, seed), line in zip(cases, got):
        want = M.emit(arena_bytes(seed, ab), source(seed, n, P, N_BLOCKS * block_len, R), f, tab, P, N_BLOCKS, block_len, R, a)
        assert bytes.fromhex(line) == want.tobytes(), (n, R)


@pytest.mark.parametrize("block_len", BLOCK_LENS)
def test_walker(driver, block_len):
    """both kernels' address functions for every workgroup, lane group, lane and iteration (the driver asserts: every source access aligned,
    inside the buffer and inside the frames of a packet that an active stream emits; every destination byte inside an entry written exactly
    once, no byte outside one written, no 16-byte store misaligned; the bytes packets_emit_cpu's); here the whole arena is held to the model
    as well.  With and without paused streams, the arena at every kind of address."""
    r = random.Random(100 + block_len)
    cases = []
    for n, P, R in FLEETS:
        for layout in (0, R):
            for with_paused in (False, True):
                formats, active, tab, ab = fleet_case(r, n, P, R, block_len, with_paused)
                cases.append((n, P, layout, formats, active, tab, ab, r.randrange(1, 1000), r.randrange(0, 16, 2)))
    got = run(driver, [f"walk {n} {P} {N_BLOCKS} {block_len} {R} {ab} {seed} {res} {nums(f)} {nums(a)} {flat(tab)}" for n, P, R, f, a, tab, ab, seed, res in cases])
    for (n, P, R, f, a, tab, ab, seed, res), line in zip(cases, got):
        assert line.startswith("ok "), (n, R, res, line[:200])
        want = M.emit(arena_bytes(seed, ab), source(seed, n, P, N_BLOCKS * block_len, R), f, tab, P, N_BLOCKS, block_len, R, a)
        assert bytes.fromhex(line[3:]) == want.tobytes(), (n, R, res)


def test_walker_small_and_uniform(driver):
    """fewer entries than one workgroup carries, one packet per stream, a last tile of one column, all-24 and all-32 fleets on 16-byte
    aligned entries (every piece but a packet's last whole), and a table of SKIP entries only"""
    r = random.Random(3)
    cases = []
    for n, P, R, nb, bl in ((1, 2, 64, 1, 45), (3, 4, 128, 1, 96), (65, 2, 64, 2, 44), (129, 4, 128, 1, 32)):
        for layout in (0, R):
            for fmt in (24, 32):
                tab = [[16 * 100 * (s * P * nb + i) for i in range(P * nb)] for s in range(n)]
                cases.append((n, P, layout, nb, bl, [fmt] * n, tab, 16 * 100 * n * P * nb, 0))
            cases.append((n, P, layout, nb, bl, [r.choice((24, 32)) for _ in range(n)], [[M.SKIP] * (P * nb) for _ in range(n)], 64, 6))
    got = run(driver, [f"walk {n} {P} {nb} {bl} {R} {ab} 5 {res} {nums(f)} {nums([1] * n)} {flat(tab)}" for n, P, R, nb, bl, f, tab, ab, res in cases])
    for (n, P, R, nb, bl, f, tab, ab, res), line in zip(cases, got):
        assert line.startswith("ok "), (n, R, line[:200])
        want = M.emit(arena_bytes(5, ab), source(5, n, P, nb * bl, R), f, tab, P, nb, bl, R)
        assert bytes.fromhex(line[3:]) == want.tobytes(), (n, R)


# ---- the check --------------------------------------------------------------------------------------------------------------------------------
def test_check_equals_the_model(driver):
    r = random.Random(11)
    cases = []
    for _ in range(400):
        n, P, nb, bl = r.randrange(1, 6), r.choice((2, 4)), r.randrange(0, 4), r.choice((0, 1, 45, 96, 192, 193))
        formats = [r.choice((16, 8, 0, 33)) if r.random() < 0.1 else r.choice((24, 32)) for _ in range(n)]
        active = [int(r.random() < 0.8) for _ in range(n)]
        ab = r.choice((0, 100, 3000, 20000))
        overlap = int(r.random() < 0.5)
        def entry(s):
            size = bl * {24: 6, 32: 8}.get(formats[s], 8)
            x = r.random()
            if x < 0.03: return 2 * r.randrange(0, 3000) + 1                      # odd
            if x < 0.06: return max(0, ab - size) + 2                              # one sample past
            if x < 0.07: return 2 ** 64 - 2                                        # offset + length wraps
            if x < 0.20: return M.SKIP
            return 2 * r.randrange(0, max(0, ab - size) // 2 + 1) if ab >= size else 0
        tab = [[entry(s) for _ in range(P * nb)] for s in range(n)]
        cases.append((n, P, nb, bl, ab, overlap, formats, active, tab))
    # the overlap rule: identical entries, the smallest overlap two legal entries can have (two bytes: offsets and lengths are even, so no two
    # legal entries share ONE byte), entries that touch, an entry inside another, an overlap with a paused stream's row and with a SKIP
    bl, size = 45, 45 * 6
    for tab, active in (([[0, 1000], [1000, 2000]], [1, 1]), ([[0, size - 2], [1000, 2000]], [1, 1]), ([[0, size], [2 * size, 3 * size]], [1, 1]),
                        ([[3000, 0], [4000, 2]], [1, 1]), ([[0, 1000], [0, 1000]], [1, 0]), ([[0, M.SKIP], [M.SKIP, 1000]], [1, 1]),
                        ([[2000, 1000], [1000 + size - 2, 0]], [1, 1])):
        cases.append((2, 2, 1, bl, 20000, 1, [24, 24], active, tab))
    cases.append((2, 2, 1, bl, 20000, 1, [32, 24], [1, 1], [[0, 1000], [45 * 8 - 2, 2000]]))
    script = []
    for n, P, nb, bl, ab, overlap, formats, active, tab in cases:
        early = nb == 0 or bl == 0 or bl > 192 or any(f not in (24, 32) for f in formats)
        script.append(f"check {n} {P} {nb} {bl} 192 {ab} {overlap} {nums(formats)} {nums(active)}" + ("" if early else " " + flat(tab)))
    got = run(driver, script)
    seen = set()
    for (n, P, nb, bl, ab, overlap, formats, active, tab), line in zip(cases, got):
        want = M.check(formats, tab, P, nb, bl, ab, active, bool(overlap))
        assert line == ("ok" if want is None else " ".join(map(str, want))), (n, P, nb, bl, ab, overlap, formats, active, tab)
        seen.add("ok" if want is None else want[0])
    assert seen == {"ok", "lengths", "format", "entry", "overlap"}
    # the named cases, spelt out: identical -> the first of the two; two bytes -> the first; touching -> none
    assert got[400] == "overlap 1" and got[401] == "overlap 0" and got[402] == "ok" and got[403] == "overlap 1" and got[404] == "ok" and got[405] == "ok" and got[406] == "overlap 1"
    assert got[407] == "overlap 0"


def test_entry_count_overflow(driver):
    """65 536 streams of 4 pairs and 8 192 packets are one entry too many; one packet fewer is looked at (and its first entry refused: an empty arena)"""
    assert M.check([24] * 4, None, 4, 2 ** 27, 45, 100) == ("overflow",)
    n = 65536
    ones = " ".join(["24"] * n) + " " + " ".join(["1"] * n)
    assert run(driver, [f"check {n} 4 8192 45 192 0 0 {ones}"]) == ["overflow"]


# ---- the calls on host-only contexts: every refusal in its order -----------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_refusals_in_their_order(flavor):
    S, F, NB = 12, 48, 2
    d = Dspi(flavor, S, device=None)
    P = d.P
    per = P * NB
    AB = 100000
    mixed = np.array([24, 32] * (S // 2), dtype=np.uint8)
    worse = mixed.copy(); worse[9] = 16; worse[11] = 8
    good = np.zeros((S, per), dtype=np.uint64)
    for s in range(S): good[s] = [800 * (s * per + i) for i in range(per)]
    good[3, 1] = M.SKIP
    odd = good.copy(); odd[5, 1] = 301; odd[9, 0] = 2 ** 63
    past = good.copy(); past[4, 0] = AB - 6 * F + 2             # (stream 4 is 24 bit: one sample past the end)
    edge = good.copy(); edge[4, 0] = AB - 6 * F; edge[5, 0] = AB - 8 * F - 6 * F      # entries that end with the arena, or with a neighbour, are legal
    pairs = np.arange(S * P * NB * F * 2, dtype=np.int32)
    pattern = (np.arange(AB) * 7 + 3).astype(np.uint8)
    arena = pattern.copy()
    err = lambda: d.L.dspi_last_error(d.h).decode()
    untouched = lambda: np.array_equal(arena, pattern)
    call = lambda pr, fm, t, ar, nb, bl, flags, ab=AB: d.L.dspi_packets_emit(d.h, pr.ctypes.data if pr is not None else None, nb, bl, fm.ctypes.data if fm is not None else None,
                                                                             t.ctypes.data if t is not None else None, ar.ctypes.data if ar is not None else None, ab, flags)
    # 1. a NULL ctx; an undefined flag bit: before the pointers, the lengths, a format or an entry are looked at
    assert d.L.dspi_packets_emit(None, pairs.ctypes.data, NB, F, mixed.ctypes.data, good.ctypes.data, arena.ctypes.data, AB, 0) == host.E_INVAL
    for flags in (0x4, 0x80000000, host.MEM_DEVICE | host.OUT_SPDIF, host.OUT_TILED | host.OUT_WIRE, host.OUT_I2S_SLOTS, host.OUT_CLIP_FLAGS):
        assert call(None, worse, odd, None, 0, 193, flags) == host.E_INVAL and "flags" in err(), flags
    # 2. the pointers and the lengths: before a format
    for pr, fm, t, ar in ((None, worse, odd, arena), (pairs, None, odd, arena), (pairs, worse, None, arena), (pairs, worse, odd, None)):
        for flags in (0, host.MEM_DEVICE, host.OUT_TILED):
            assert call(pr, fm, t, ar, NB, F, flags) == host.E_INVAL and "required" in err()
    for nb, bl in ((0, F), (NB, 0), (NB, 193)):
        assert call(pairs, worse, odd, arena, nb, bl, 0) == host.E_INVAL and "block_len" in err(), (nb, bl)
    # 3. a format, the lowest stream first: before the entry count and an entry
    assert call(pairs, worse, odd, arena, NB, F, 0) == host.E_INVAL and "stream 9" in err()
    assert call(pairs, worse, odd, arena, 2 ** 31 // (S * P) + 1, F, 0) == host.E_INVAL and "stream 9" in err()
    # 4. the entry count: before an entry (the table is not read)
    assert call(pairs, mixed, odd, arena, 2 ** 31 // (S * P) + 1, F, 0) == host.E_INVAL and "2^31 - 1 entries" in err()
    # 5. the first illegal entry of an active stream, in table order, with its index: before the host-only context's refusal
    for flags in (0, host.OUT_TILED, host.MEM_DEVICE):
        assert call(pairs, mixed, odd, arena, NB, F, flags) == host.E_INVAL and f"entry {5 * per + 1} " in err()
        assert call(pairs, mixed, past, arena, NB, F, flags) == host.E_INVAL and f"entry {4 * per} " in err()
        assert call(pairs, mixed, good, arena, NB, F, flags, ab=800 * (S * per - 1) + 8 * F - 1) == host.E_INVAL and f"entry {S * per - 1} " in err()
    assert untouched()      # a refused call writes nothing (without DSPI_MEM_DEVICE a call that got as far as writing would have written here)
    # 6. DSPI_MEM_DEVICE on a host-only context
    for t in (good, edge):
        assert call(pairs, mixed, t, arena, NB, F, host.MEM_DEVICE) == host.E_NODEVICE and call(pairs, mixed, t, arena, NB, F, host.MEM_DEVICE | host.OUT_TILED) == host.E_NODEVICE
    assert untouched()
    # a paused stream's rows are neither read nor checked (its format is)
    d.pause_streams(5, 1); d.pause_streams(9, 1)
    assert call(pairs, mixed, odd, arena, NB, F, host.MEM_DEVICE) == host.E_NODEVICE
    assert call(pairs, worse, odd, arena, NB, F, host.MEM_DEVICE) == host.E_INVAL and "stream 9" in err()
    d.resume_streams(5, 1)
    assert call(pairs, mixed, odd, arena, NB, F, 0) == host.E_INVAL and f"entry {5 * per + 1} " in err()
    assert untouched()
    # ... and the accepted call writes: stream 9 is paused, its row illegal
    fixed = odd.copy(); fixed[5, 1] = 300
    assert call(pairs, mixed, fixed, arena, NB, F, 0) == 0
    assert not untouched()
    d.close()


def test_emit_check_on_a_host_only_context():
    """dspi_packets_emit_check: refusals 2 to 5 and the overlap rule with the index of the entry, equal to the model's, on a context without a device"""
    S, NB = 7, 2
    d = Dspi(0, S, device=None)
    P, r = d.P, random.Random(5)
    per = P * NB
    d.pause_streams(2, 2)
    active = [0 if s in (2, 3) else 1 for s in range(S)]
    seen = set()
    for _ in range(300):
        bl, nb = r.choice((45, 96, 192, 193, 0)), r.choice((NB, NB, NB, 0))
        formats = [r.choice((24, 32)) for _ in range(S)]
        if r.random() < 0.1: formats[r.randrange(S)] = 16
        ab, overlap = 40000, r.random() < 0.6
        tab = np.array([[M.SKIP if r.random() < 0.1 else 2 * r.randrange(0, 19000) + (r.random() < 0.01) for _ in range(P * max(nb, 1))] for _ in range(S)], dtype=np.uint64)
        if r.random() < 0.5: tab[2:4] = ILLEGAL      # (paused: anything)
        want = M.check(formats, tab.tolist(), P, nb, bl, ab, active, overlap)
        bad = C.c_uint64(12345)
        rc = d.L.dspi_packets_emit_check(d.h, np.array(formats, dtype=np.uint8).ctypes.data, tab.ctypes.data, nb, bl, ab, host.EMIT_CHECK_OVERLAP if overlap else 0, C.byref(bad))
        assert (rc == 0) == (want is None), (want, rc)
        if want is not None: assert rc == host.E_INVAL
        assert bad.value == (want[1] if want is not None and want[0] in ("entry", "overlap") else 12345)
        if want is not None and want[0] in ("entry", "overlap"): assert f"entry {want[1]} " in d.L.dspi_last_error(d.h).decode()
        seen.add("ok" if want is None else want[0])
    assert seen == {"ok", "lengths", "format", "entry", "overlap"}
    # the wrapper: bad_entry; identical entries, the smallest overlap, touching entries; NULL pointers; an undefined check flag
    size = 45 * 6
    tab = np.array([[2000 * (s * per + i) for i in range(per)] for s in range(S)], dtype=np.uint64)
    assert d.packets_emit_check([24] * S, tab, NB, 45, 60000, overlap=True) is None and d.bad_entry is None
    tab[6, 2] = 7
    with pytest.raises(DspiError) as e: d.packets_emit_check([24] * S, tab, NB, 45, 60000)
    assert e.value.code == host.E_INVAL and d.bad_entry == 6 * per + 2
    tab[6, 2] = tab[1, 1]                         # identical entries
    assert d.packets_emit_check([24] * S, tab, NB, 45, 60000) is None      # (not asked)
    with pytest.raises(DspiError): d.packets_emit_check([24] * S, tab, NB, 45, 60000, overlap=True)
    assert d.bad_entry == 1 * per + 1
    tab[6, 2] = tab[1, 1] + size - 2              # the smallest overlap of two legal entries: two bytes
    with pytest.raises(DspiError): d.packets_emit_check([24] * S, tab, NB, 45, 60000, overlap=True)
    assert d.bad_entry == 1 * per + 1
    tab[6, 2] = tab[1, 1] + size                  # touching
    assert d.packets_emit_check([24] * S, tab, NB, 45, 60000, overlap=True) is None
    fm = np.full(S, 24, dtype=np.uint8)
    assert d.L.dspi_packets_emit_check(None, fm.ctypes.data, tab.ctypes.data, NB, 45, 60000, 0, None) == host.E_INVAL
    assert d.L.dspi_packets_emit_check(d.h, None, tab.ctypes.data, NB, 45, 60000, 0, None) == host.E_INVAL
    assert d.L.dspi_packets_emit_check(d.h, fm.ctypes.data, None, NB, 45, 60000, 0, None) == host.E_INVAL
    assert d.L.dspi_packets_emit_check(d.h, fm.ctypes.data, tab.ctypes.data, NB, 45, 60000, 2, None) == host.E_INVAL
    tab[6, 2] = 7
    assert d.L.dspi_packets_emit_check(d.h, fm.ctypes.data, tab.ctypes.data, NB, 45, 60000, 0, None) == host.E_INVAL      # (bad_entry may be NULL)
    d.close()


# ---- the host path ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,n", ((1, 130), (0, 70)), ids=("f32", "q28"))
@pytest.mark.parametrize("block_len", (45, 96, 192))
def test_host_path_equals_the_model(flavor, n, block_len):
    """dspi_packets_emit without DSPI_MEM_DEVICE, through the C-ABI on a host-only context, from both layouts, with paused streams"""
    d = Dspi(flavor, n, device=None)
    P, R = d.P, d.tile_streams()
    assert (n, P, R) in FLEETS
    r = random.Random(7 * block_len + n)
    formats, active, tab, ab = fleet_case(r, n, P, R, block_len, True)
    for s in range(n):
        if not active[s]: d.pause_streams(s, 1)
    for layout in (0, R):
        pairs = source(block_len, n, P, N_BLOCKS * block_len, layout)
        pattern = arena_bytes(9, ab)
        got = d.packets_emit_host(pairs, N_BLOCKS, block_len, formats, tab, pattern.copy(), tiled=bool(layout))
        assert np.array_equal(got, M.emit(pattern, pairs, formats, tab, P, N_BLOCKS, block_len, layout, active)), layout
    d.close()
