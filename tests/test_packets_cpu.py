"""Input from a packet table, without a GPU: dspi_amd/csrc/dspi_packets.{h,cpp} through a g++ driver (tests/packets_driver.cpp) against the model
written from the header's prose (tests/packets_model.py) — the check in its order, the gathered and widened run, and the kernel's address
arithmetic walked for every workgroup and lane — and the three calls of include/dspi.h on host-only contexts: every refusal in its order."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import packets_model as M
from dspi_amd import host, wire as W
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
BLOCK_LENS = (1, 2, 7, 44, 45, 96, 168, 169, 192, 683, 700)
N_BLOCKS = 3


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here is about a library that has the call"""
    assert hasattr(host.lib(), "dspi_process_packets"), "libdspi_mi355x has no dspi_process_packets"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes — asked of an empty program,
    so that a sanitized build of the driver that fails for any other reason fails here —, else plain; which build ran is printed (pytest -s, or
    with the failure's captured output)"""
    tmp = tmp_path_factory.mktemp("packets")
    exe = tmp / "packets_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "packets_driver.cpp"),
           os.path.join(CSRC, "dspi_packets.cpp"), os.path.join(CSRC, "dspi_intake.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("packets_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def arena_bytes(seed, n):
    """the driver's arena: byte i of an arena made with `seed`"""
    i = np.arange(n, dtype=np.uint64)
    return ((i * 131 + seed * 17 + (i >> 8) * 7 + 1) & 0xff).astype(np.uint8)


def flat(rows): return " ".join(str(int(x)) for r in rows for x in r)


# ---- the symbols and the header's words -------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_process_packets", "dspi_packets_check", "dspi_debug_packets_intake"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "8 + input from a packet table: detect by symbol (dspi_process_packets; with it dspi_packets_check; additions only)",
                 "int dspi_packets_check(const dspi_ctx *ctx, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len,\n"
                 "                       uint64_t arena_bytes, uint64_t *bad_entry /* may be NULL: s * n_blocks + k of the first entry refused */);",
                 "int dspi_process_packets(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table,\n"
                 "                         uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words /* may be NULL */, uint32_t flags);",
                 "int dspi_debug_packets_intake(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table,\n"
                 "                              uint32_t n_blocks, uint32_t block_len);",
                 "table[s * n_blocks + k] is the byte offset in",
                 "AN ENTRY IS LEGAL when it is even and offset + block_len * frame bytes <= arena_bytes",
                 "Entries may be equal and may overlap in any way",
                 "Entries of PAUSED streams are neither read nor checked",
                 "Nothing outside [offset, offset + length) of an active",
                 "DSPI_MEM_DEVICE is REQUIRED: arena and everything in *out are device memory; table and bit_depths are host memory",
                 "the caller may reuse its table when the call returns",
                 "No state is added to the context",
                 "the first illegal entry of an active stream, in table order",
                 "dspi_packets_check applies refusals 2 to 5",
                 "LEFT OUT: arenas in host memory; tables in device memory; S/PDIF and linked sources in the same call"):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()      # the module and the kernel are the library's
    assert "dspi_packets" in mk.split("HOST =")[1].split("\n")[0] and "dspi_packetrx" in mk.split("KERNELS =")[1].split("\n")[0]


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------
def make_tables(r, depths, n_blocks, block_len):
    """[(name, table rows, arena_bytes)]: identity (the mixed call's own layout), reversed, all-equal (fan-out), overlapping (a sliding window
    of 2 bytes), random, and every even source residue mod 16; each arena ends exactly at the last byte of the entry that reaches furthest"""
    n = len(depths)
    size = [block_len * M.frame_bytes(d) for d in depths]
    ident, at = [], 0
    for s in range(n):
        ident.append([at + k * size[s] for k in range(n_blocks)]); at += n_blocks * size[s]
    total = at
    rev = [[total - o - size[s] for o in row] for s, row in enumerate(ident)]      # (the layout mirrored: even, since every size is)
    tabs = [("identity", ident, total), ("reversed", rev, total),
            ("fan-out", [[0] * n_blocks for _ in range(n)], max(size)),
            ("overlapping", [[2 * (s + k) for k in range(n_blocks)] for s in range(n)], max(2 * (s + n_blocks - 1) + size[s] for s in range(n)))]
    big = max(size) + 4096
    rnd = [[2 * r.randrange(0, (big - size[s]) // 2 + 1) for _ in range(n_blocks)] for s in range(n)]
    rnd[n - 1][n_blocks - 1] = big - size[n - 1]      # (one entry ends with the arena)
    tabs.append(("random", rnd, big))
    for res in range(0, 16, 2):
        tabs.append((f"residue {res}", [[res + 16 * (3 * s + k) for k in range(n_blocks)] for s in range(n)],
                     max(res + 16 * (3 * s + n_blocks - 1) + size[s] for s in range(n))))
    return tabs


@pytest.mark.parametrize("block_len", BLOCK_LENS)
def test_gather_equals_the_model(driver, block_len):
    r = random.Random(block_len)
    cases = []
    for depth in (16, 24):
        for name, tab, ab in make_tables(r, [depth, depth], N_BLOCKS, block_len):
            for row in tab: cases.append((depth, row, ab, r.randrange(1, 1000), name))
    got = run(driver, [f"gather {d} {N_BLOCKS} {block_len} {ab} {seed} " + " ".join(map(str, row)) for d, row, ab, seed, _ in cases])
    for (d, row, ab, seed, name), line in zip(cases, got):
        assert bytes.fromhex(line) == M.gather(arena_bytes(seed, ab), row, d, block_len).tobytes(), (name, d, row)


@pytest.mark.parametrize("block_len", BLOCK_LENS)
def test_walker(driver, block_len):
    """the kernel's address functions for every workgroup, lane group and lane (the driver asserts: sources inside their entries, every
    destination byte of an active stream written exactly once, the bytes packets_gather_cpu's); here the bytes are held to the model as well,
    and a paused stream with entries far outside the arena is neither read nor written"""
    r = random.Random(100 + block_len)
    cases = []
    for depths in ([16, 24, 16], [24, 24, 16], [16, 16, 24]):
        for name, tab, ab in make_tables(r, depths, N_BLOCKS, block_len):
            for src_res, dst_res in ((0, 0), (r.randrange(0, 16, 2), r.randrange(0, 16, 2))):
                cases.append((depths, [1, 1, 1], tab, ab, r.randrange(1, 1000), src_res, dst_res, name))
        name, tab, ab = make_tables(r, depths, N_BLOCKS, block_len)[4]
        tab = [list(row) for row in tab]; tab[1] = [2 ** 63 + 1] * N_BLOCKS
        cases.append((depths, [1, 0, 1], tab, ab, 77, 6, 10, "paused"))
    got = run(driver, [f"walk 3 {N_BLOCKS} {block_len} {ab} {seed} {sr} {dr} " + " ".join(map(str, d)) + " " + " ".join(map(str, a)) + " " + flat(tab)
                       for d, a, tab, ab, seed, sr, dr, _ in cases])
    for (d, a, tab, ab, seed, sr, dr, name), line in zip(cases, got):
        assert line.startswith("ok "), (name, d, sr, dr, line[:200])
        arena = arena_bytes(seed, ab)
        want = b"".join(M.gather(arena, tab[s], d[s], block_len).tobytes() if a[s] else b"\xcc" * (6 * block_len * N_BLOCKS) for s in range(3))
        assert bytes.fromhex(line[3:]) == want, (name, d, sr, dr)


def test_walker_many_workgroups(driver):
    """more jobs than one workgroup carries, a last workgroup that is not full, and one packet per stream"""
    r = random.Random(3)
    for n, nb, bl in ((37, 1, 45), (5, 11, 44), (2, 40, 7)):
        depths = [r.choice((16, 24)) for _ in range(n)]
        ab = 6 * bl + 3000
        tab = [[2 * r.randrange(0, (ab - bl * M.frame_bytes(depths[s])) // 2 + 1) for _ in range(nb)] for s in range(n)]
        line = run(driver, [f"walk {n} {nb} {bl} {ab} 9 4 2 " + " ".join(map(str, depths)) + " " + " ".join(["1"] * n) + " " + flat(tab)])[0]
        assert line.startswith("ok "), line[:200]
        arena = arena_bytes(9, ab)
        assert bytes.fromhex(line[3:]) == b"".join(M.gather(arena, tab[s], depths[s], bl).tobytes() for s in range(n))


def test_check_equals_the_model(driver):
    r = random.Random(11)
    cases = []
    for _ in range(300):
        n, nb, bl = r.randrange(1, 7), r.randrange(0, 5), r.choice((0, 1, 45, 96, 192, 193))
        depths = [r.choice((16, 24, 24, 16, 16, 24, 8, 32)) if r.random() < 0.15 else r.choice((16, 24)) for _ in range(n)]
        active = [int(r.random() < 0.8) for _ in range(n)]
        ab = r.choice((0, 100, 1200, 5000))
        def entry(s):
            size = bl * {16: 4, 24: 6}.get(depths[s], 6)
            x = r.random()
            if x < 0.05: return 2 * r.randrange(0, 3000) + 1                      # odd
            if x < 0.10: return max(0, ab - size) + 2                              # one sample past
            if x < 0.12: return 2 ** 64 - 2                                        # offset + length wraps
            return 2 * r.randrange(0, max(0, ab - size) // 2 + 1) if ab >= size else 0
        tab = [[entry(s) for _ in range(nb)] for s in range(n)]
        cases.append((n, nb, bl, ab, depths, active, tab))
    cases.append((2 ** 31, 1, 45, 100, None, None, None))      # (the overflow: the driver is given no table for it)
    script = []
    for n, nb, bl, ab, depths, active, tab in cases:
        if depths is None: continue
        early = nb == 0 or bl == 0 or bl > 192
        script.append(f"check {n} {nb} {bl} 192 {ab} " + " ".join(map(str, depths)) + " " + " ".join(map(str, active)) + ("" if early else " " + flat(tab)))
    got = run(driver, script)
    seen = set()
    for (n, nb, bl, ab, depths, active, tab), line in zip(cases, got):
        want = M.check(depths, tab, nb, bl, ab, active)
        assert line == ("ok" if want is None else " ".join(map(str, want))), (n, nb, bl, ab, depths, active, tab)
        seen.add("ok" if want is None else want[0])
    assert seen == {"ok", "lengths", "depth", "entry"}


def test_entry_count_overflow(driver):
    """65 536 streams of 32 768 packets are one entry too many; one packet fewer is looked at (and its first entry refused: an empty arena)"""
    assert M.check([24] * 4, None, 2 ** 29, 45, 100) == ("overflow",)
    n = 65536
    ones = " ".join(["24"] * n) + " " + " ".join(["1"] * n)
    got = run(driver, [f"check {n} 32768 45 192 0 {ones}"])
    assert got == ["overflow"]


# ---- the calls on host-only contexts: every refusal in its order -----------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_refusals_in_their_order(flavor):
    S, F, NB = 12, 48, 2
    d = Dspi(flavor, S, device=None)
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=7) >= 0
    mixed = np.array([16, 24] * (S // 2), dtype=np.uint8)      # stream 7: 24 bit
    low = mixed.copy(); low[7] = 16                             # stream 7: 16 bit, under the preamp's refusal on float contexts
    AB = 10000
    good = np.zeros((S, NB), dtype=np.uint64)
    for s in range(S): good[s] = [100 * s, 100 * s + 2000]
    odd = good.copy(); odd[5, 1] = 301; odd[9, 0] = 20001       # the first illegal entry in table order is 5 * NB + 1
    past = good.copy(); past[4, 0] = AB - 4 * F + 2             # (stream 4 is 16 bit: one sample past the end)
    edge = good.copy(); edge[4, 0] = AB - 4 * F; edge[5, 0] = AB - 6 * F      # entries that end with the arena are legal
    arena = np.zeros(16, dtype=np.uint8)      # (a pointer: nothing reads it on a host-only context)
    out = host._Out(None, None, None, None)
    po, pa = C.byref(out), arena.ctypes.data
    dev = host.MEM_DEVICE
    refused = host.E_UNSUPPORTED if flavor else host.E_NODEVICE
    err = lambda: d.L.dspi_last_error(d.h).decode()
    call = lambda a, dp, t, nb, bl, o, flags, ab=AB: d.L.dspi_process_packets(d.h, a, ab, dp.ctypes.data if dp is not None else None, t.ctypes.data if t is not None else None, nb, bl, o, None, flags)
    worse = low.copy(); worse[9] = 8
    # 1. the flag rule, DSPI_MEM_DEVICE first of all: before the pointers, the lengths, a depth or an entry are looked at
    assert d.L.dspi_process_packets(None, pa, AB, low.ctypes.data, good.ctypes.data, NB, F, po, None, dev) == host.E_INVAL
    assert call(None, worse, odd, 0, 193, None, 0) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    for flags in (dev | 0x80000000, dev | host.OUT_SPDIF | host.OUT_TILED, dev | host.OUT_WIRE | host.OUT_SPDIF, dev | host.OUT_WIRE | host.OUT_I2S_SLOTS):
        assert call(None, worse, odd, 0, 193, None, flags) == host.E_INVAL, flags
    assert call(None, worse, odd, 0, 193, None, dev | host.OUT_WIRE | host.OUT_SPDIF) == host.E_INVAL and "DSPI_OUT_WIRE" in err()
    # 2. the pointers and the lengths: before a depth
    for a, dp, t, o in ((None, worse, odd, po), (pa, None, odd, po), (pa, worse, None, po), (pa, worse, odd, None)):
        assert call(a, dp, t, NB, F, o, dev) == host.E_INVAL
    for nb, bl in ((0, F), (NB, 0), (NB, 193)):
        assert call(pa, worse, odd, nb, bl, po, dev) == host.E_INVAL and "block_len" in err(), (nb, bl)
    # 3. a depth: before an entry
    assert call(pa, worse, odd, NB, F, po, dev) == host.E_INVAL and "stream 9" in err()
    # 5. the first illegal entry of an active stream, in table order, with its index: before the preamp's refusal
    assert call(pa, low, odd, NB, F, po, dev) == host.E_INVAL and f"entry {5 * NB + 1} " in err()
    assert call(pa, low, past, NB, F, po, dev) == host.E_INVAL and f"entry {4 * NB} " in err()
    assert call(pa, low, good, NB, F, po, dev, ab=100 * 11 + 2000 + 6 * F - 1) == host.E_INVAL and f"entry {11 * NB + 1} " in err()
    # 6. the preamp: float contexts, active 16-bit streams only; 7. the host-only context
    assert call(pa, low, good, NB, F, po, dev) == refused
    if flavor: assert "stream 7" in err()
    assert call(pa, low, edge, NB, F, po, dev) == refused
    assert call(pa, mixed, good, NB, F, po, dev) == host.E_NODEVICE
    assert call(pa, mixed, edge, NB, F, po, dev | host.OUT_WIRE | host.OUT_TILED) == host.E_NODEVICE
    # a paused stream's entries are neither read nor checked, and its preamp does not count
    d.pause_streams(5, 1); d.pause_streams(9, 1)
    assert call(pa, mixed, odd, NB, F, po, dev) == host.E_NODEVICE
    d.pause_streams(7, 1)
    assert call(pa, low, odd, NB, F, po, dev) == host.E_NODEVICE
    d.resume_streams(5, 1)
    assert call(pa, low, odd, NB, F, po, dev) == host.E_INVAL and f"entry {5 * NB + 1} " in err()
    d.resume_streams(7, 1); d.resume_streams(9, 1)
    # the front end alone: refusals 2 to 5, no preamp rule, then the host-only context
    dbg = lambda a, dp, t, nb, bl: d.L.dspi_debug_packets_intake(d.h, a, AB, dp.ctypes.data if dp is not None else None, t.ctypes.data if t is not None else None, nb, bl)
    assert dbg(None, low, good, NB, F) == host.E_INVAL and dbg(pa, None, good, NB, F) == host.E_INVAL and dbg(pa, low, None, NB, F) == host.E_INVAL
    assert dbg(pa, worse, odd, NB, 193) == host.E_INVAL and "block_len" in err()
    assert dbg(pa, worse, odd, NB, F) == host.E_INVAL and "stream 9" in err()
    assert dbg(pa, low, odd, NB, F) == host.E_INVAL and f"entry {5 * NB + 1} " in err()
    assert dbg(pa, low, good, NB, F) == host.E_NODEVICE
    d.close()


def test_packets_check_on_a_host_only_context():
    """dspi_packets_check: refusals 2 to 5 with the index of the entry, equal to the model's, on a context without a device"""
    S, NB = 9, 3
    d = Dspi(0, S, device=None)
    r = random.Random(5)
    d.pause_streams(2, 2)
    active = [0 if s in (2, 3) else 1 for s in range(S)]
    seen = set()
    for _ in range(200):
        bl, nb = r.choice((45, 96, 192, 193, 0)), r.choice((NB, NB, NB, 0))
        depths = [r.choice((16, 24)) for _ in range(S)]
        if r.random() < 0.1: depths[r.randrange(S)] = 20
        ab = 4000
        tab = np.array([[2 * r.randrange(0, 1500) + (r.random() < 0.02) for _ in range(max(nb, 1))] for _ in range(S)], dtype=np.uint64)
        if r.random() < 0.5: tab[2:4] = 2 ** 64 - 1      # (paused: anything)
        want = M.check(depths, tab.tolist(), nb, bl, ab, active)
        bad = C.c_uint64(12345)
        rc = d.L.dspi_packets_check(d.h, np.array(depths, dtype=np.uint8).ctypes.data, tab.ctypes.data, nb, bl, ab, C.byref(bad))
        assert (rc == 0) == (want is None), (want, rc)
        if want is not None: assert rc == host.E_INVAL
        assert bad.value == (want[1] if want is not None and want[0] == "entry" else 12345)
        if want is not None and want[0] == "entry": assert f"entry {want[1]} " in d.L.dspi_last_error(d.h).decode()
        seen.add("ok" if want is None else want[0])
    assert seen == {"ok", "lengths", "depth", "entry"}
    # the wrapper: bad_entry, and NULL pointers
    tab = np.zeros((S, NB), dtype=np.uint64); tab[6, 2] = 7
    with pytest.raises(DspiError) as e: d.packets_check([24] * S, tab, NB, 45, 4000)
    assert e.value.code == host.E_INVAL and d.bad_entry == 6 * NB + 2
    tab[6, 2] = 8
    assert d.packets_check([24] * S, tab, NB, 45, 4000) is None and d.bad_entry is None
    dp = np.full(S, 24, dtype=np.uint8)
    assert d.L.dspi_packets_check(None, dp.ctypes.data, tab.ctypes.data, NB, 45, 4000, None) == host.E_INVAL
    assert d.L.dspi_packets_check(d.h, None, tab.ctypes.data, NB, 45, 4000, None) == host.E_INVAL
    assert d.L.dspi_packets_check(d.h, dp.ctypes.data, None, NB, 45, 4000, None) == host.E_INVAL
    tab[6, 2] = 7
    assert d.L.dspi_packets_check(d.h, dp.ctypes.data, tab.ctypes.data, NB, 45, 4000, None) == host.E_INVAL      # (bad_entry may be NULL)
    d.close()
