"""Stream boots without a GPU: the list rule, the kernel's work items and the rows' targets (dspi_amd/csrc/dspi_boot.{h,cpp}) through a g++
driver (tests/boot_driver.cpp), and dspi_boot_streams (include/dspi.h) on host-only contexts, where the call does its whole parameter half:
a booted stream's parameters are those of an oracle that has just been powered on, the same way."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from orclib import Oracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_flash_dump import make_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("boot") / "boot_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "boot_driver.cpp"),
                    os.path.join(CSRC, "dspi_boot.cpp")], check=True)
    return str(exe)


def run(driver, mode, arg, cases):
    """one line of input per case, one line of output per case"""
    text = "".join(c + "\n" for c in cases)
    out = subprocess.run([driver, mode] + ([str(arg)] if arg is not None else []), input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return out


def bits(active):
    return "".join("1" if a else "0" for a in active)


def flash_cases(flavor):
    """the four dumps of test_gpu_parity.py::test_flash_dump_boots_device_context and preset_boot_load's code for each: a v2 directory, a v1
    directory, a corrupt selected slot (factory defaults), a legacy sector (migrated to slot 0)"""
    fl = int(flavor)
    slots = make_slots(fl); occ = sum(1 << n for n in slots)
    D, F = W.flash_dump, W.flash_directory
    bad = dict(slots); b = bytearray(bad[4]); b[100] ^= 0x40; bad[4] = bytes(b)
    return [(D(F(default_slot=4, last_active_slot=9, slot_occupied=occ, master_volume_db=-17.0), slots), 4),
            (D(F(version=1, default_slot=9, slot_occupied=occ, master_volume_mode=1, names={9: "Night"}), slots), 9),
            (D(F(default_slot=4, slot_occupied=occ), bad), 16 + 4),
            (D(None, {}, W.legacy_sector_from_slot(slots[4], fl, version=7)), 32)]


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_boot_streams")
    assert host.BOOT_STREAMS_AS_IS == 1
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + stream boots: detect by symbol (dspi_boot_streams; with it DSPI_BOOT_STREAMS_AS_IS; additions only)",
                 "#define DSPI_BOOT_STREAMS_AS_IS 0x1u   /* keep the power-on write positions (delay write index 0, ring position 0) */",
                 "int dspi_boot_streams(dspi_ctx *ctx, const uint32_t *streams, uint32_t n,\n"
                 "                      const void *dump, size_t len, uint32_t flags, int *selection);"):
        assert word in text, word


# ---- validation ---------------------------------------------------------------------------------------------------------------------------
def test_validation(driver):
    cases = {
        "empty": ("10", "empty"),
        "null": ("10 null", "empty"),
        "at the count": ("10 3 10", "out of range"),
        "far out of range": ("10 4294967295", "out of range"),
        "listed twice": ("10 3 7 3", "listed twice"),
    }
    ok = {"one": "10 9", "unsorted": "10 7 0 3", "everybody": "4 3 2 1 0"}
    got = run(driver, "validate", None, [c for c, _ in cases.values()] + list(ok.values()))
    for (name, (_, msg)), g in zip(cases.items(), got):
        assert msg in g, (name, g)
    for name, g in zip(ok, got[len(cases):]):
        assert g == "ok", (name, g)


# ---- the work items -----------------------------------------------------------------------------------------------------------------------
def parse_items(line):
    out = []
    for g in line.split("I")[1:]:
        v = list(map(int, g.split()))
        out.append(dict(row=v[0], q_any=v[1], q_all=v[2], target=v[3], cols=v[4:]))
    return out


def expected_masks(cols, R):
    """q_any / q_all from the definition: bit q = columns 4q .. 4q + 3"""
    any_, all_ = 0, 0
    for q in range(R // 4):
        k = sum(1 for c in range(4 * q, 4 * q + 4) if c in cols)
        if k: any_ |= 1 << q
        if k == 4: all_ |= 1 << q
    return any_, all_


@pytest.mark.parametrize("R", (128, 64))
def test_row_items(driver, R):
    S = 2 * R + 45                           # three rows, the last partial, an odd count
    full = (1 << (R // 4)) - 1
    lists = {
        "one column": [40],
        "two lane mates": [10, 11],
        "a whole row": list(range(R, 2 * R)),
        "a whole row and the partial last one": list(range(R, 2 * R)) + list(range(2 * R, S)),
        "unsorted, three rows": [2 * R + 5, 7, R + 3, 4, 6, 2 * R + 4, 5],
    }
    got = run(driver, "items", R, [f"{S} - 0 " + " ".join(map(str, l)) for l in lists.values()])
    items = {name: parse_items(g) for name, g in zip(lists, got)}
    for name, l in lists.items():      # every list: the rows ascending, their columns, and both masks bit by bit
        rows = sorted({s // R for s in l})
        assert [it["row"] for it in items[name]] == rows, name
        for it in items[name]:
            cols = sorted(s % R for s in l if s // R == it["row"])
            assert it["cols"] == cols, name
            want_any, want_all = expected_masks(set(cols), R)
            for q in range(R // 4):
                assert (it["q_any"] >> q) & 1 == (want_any >> q) & 1 and (it["q_all"] >> q) & 1 == (want_all >> q) & 1, (name, it["row"], q)
            assert it["q_any"] >> (R // 4) == 0 and it["q_all"] >> (R // 4) == 0
    assert [(it["q_any"], it["q_all"]) for it in items["one column"]] == [(1 << 10, 0)]
    assert [(it["q_any"], it["q_all"]) for it in items["two lane mates"]] == [(1 << 2, 0)]
    assert [(it["q_any"], it["q_all"]) for it in items["a whole row"]] == [(full, full)]
    last = items["a whole row and the partial last one"][1]      # 45 columns: eleven whole groups and one column of the twelfth
    assert (last["q_any"], last["q_all"]) == ((1 << 12) - 1, (1 << 11) - 1)
    three = items["unsorted, three rows"]
    assert [(it["q_any"], it["q_all"]) for it in three] == [(0b10, 0b10), (0b1, 0), (0b10, 0)]


def test_targets(driver):
    R, S = 8, 21      # three rows, the last partial
    act = [1] * S
    for s in (0, 2, 12, 13, 14, 15, 20): act[s] = 0
    cases = [
        (f"{S} {bits(act)} 0 1 3", [(0, 4)]),                                       # 0 and 2 are paused, 1 and 3 listed: 4 is the lowest resident
        (f"{S} - 0 1 3", [(0, 0)]),                                                 # nothing paused: stream 0 itself
        (f"{S} - 0 0 9", [(0, 1), (1, 8)]),
        (f"{S} {bits(act)} 0 8 9 10 11", [(1, -1)]),                                # the unlisted columns are all paused
        (f"{S} - 0 8 9 10 11 12 13 14 15 16", [(1, -1), (2, 17)]),                  # a fully listed row
        (f"{S} {bits(act)} 0 16 17 18 19", [(2, -1)]),                              # the partial row: 20 is paused, nobody past it counts
        (f"{S} - 0 16 17 18 19 20", [(2, -1)]),                                     # the partial row listed whole
        (f"{S} {bits(act)} 0 20 12", [(1, 8), (2, 16)]),                            # a paused slot may be booted; its row's residents decide
        (f"{S} - 1 0 9", [(0, -1), (1, -1)]),                                       # power-on positions: nobody's
    ]
    got = run(driver, "items", R, [c for c, _ in cases])
    for (case, want), g in zip(cases, got):
        assert [(it["row"], it["target"]) for it in parse_items(g)] == want, case


# ---- host-only contexts -------------------------------------------------------------------------------------------------------------------
S = 301


def loaded(flavor):
    d = Dspi(flavor, S, device=None)
    assert d.load_bulk(WL.full_chain_blob(flavor)) == 0
    return d


def fresh_bulk(flavor, dump=None):
    o = Oracle(flavor, detmath=True, flash=dump)
    try: return o.collect_bulk(), o.boot_selection
    finally: o.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_null_dump(flavor):
    d = loaded(flavor)
    d.pause_streams(60, 10)
    paused = d.streams_paused().copy()
    before = [d.collect_bulk(s) for s in range(S)]
    booted = [3, 64, S - 1]
    assert d.boot_streams(booted) == 48
    want, _ = fresh_bulk(flavor)
    assert want != before[0]
    for s in range(S):
        assert d.collect_bulk(s) == (want if s in booted else before[s]), s
    assert d.image_count() == 2
    assert np.array_equal(d.streams_paused(), paused)
    # the selection pointer may be null, and the flag changes nothing about the parameters
    l = np.array([5], dtype=np.uint32)
    assert d.L.dspi_boot_streams(d.h, l.ctypes.data, 1, None, 0, host.BOOT_STREAMS_AS_IS, None) == 1
    assert d.collect_bulk(5) == want and d.image_count() == 2      # (equal objects fold)
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_dumps(flavor):
    d = loaded(flavor)
    before = d.collect_bulk(0)
    for k, (dump, code) in enumerate(flash_cases(flavor)):
        booted = [10 + k, 200 - k]
        assert d.boot_streams(booted, dump + b"tail") == code      # (a longer buffer is fine)
        want, sel = fresh_bulk(flavor, dump)
        assert sel == code
        for s in booted: assert d.collect_bulk(s) == want, (code, s)
        assert d.collect_bulk(0) == before
    # every stream from one dump: one object
    dump, code = flash_cases(flavor)[0]
    assert d.boot_streams(np.arange(S)[::-1], dump) == code
    assert d.image_count() == 1
    want, _ = fresh_bulk(flavor, dump)
    for s in (0, 128, S - 1): assert d.collect_bulk(s) == want
    d.close()


def test_populated_flash_context():
    """dump == NULL on a DSPI_BOOT_POPULATED_FLASH context: dspi_create's own device there, which a fresh context of that kind shows"""
    d = Dspi(1, S, device=None, populated_flash=True)
    ref = d.collect_bulk(0)
    assert d.load_bulk(WL.full_chain_blob(1)) == 0
    assert d.boot_streams([7]) == 48
    assert d.collect_bulk(7) == ref and d.collect_bulk(8) != ref and d.image_count() == 2
    assert d.boot_streams(range(S)) == 48
    assert d.image_count() == 1
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_refusals(flavor):
    d = loaded(flavor)
    assert d.load_bulk(WL.full_chain_blob(flavor, max_delay_ms=3.0), stream=9) == 0
    d.pause_streams(20, 5)
    images, paused = d.image_count(), d.streams_paused().copy()
    before = [d.collect_bulk(s) for s in range(S)]
    dump = flash_cases(flavor)[0][0]
    sel = C.c_int(-7)

    def boot(l, n=None, dump=None, length=None, flags=0):
        a = np.asarray([] if l is None else l, dtype=np.uint32)
        return d.L.dspi_boot_streams(d.h, a.ctypes.data if l is not None else None, len(a) if n is None else n, dump,
                                     (len(dump) if dump else 0) if length is None else length, flags, C.byref(sel))
    assert boot([1, 2], n=0) == host.E_INVAL
    assert boot(None, n=2) == host.E_INVAL
    assert boot([1, S]) == host.E_INVAL and boot([0xFFFFFFFF]) == host.E_INVAL
    assert boot([1, 9, 1]) == host.E_INVAL
    for flags in (0x2, 0x3, 0x100, 0x80000000): assert boot([1, 9], flags=flags) == host.E_INVAL, hex(flags)
    assert boot([1, 9], dump=dump, length=host_dump_bytes() - 1) == host.E_SHORT
    assert boot([1, 9], dump=dump, length=0) == host.E_SHORT
    with pytest.raises(DspiError) as e: d.boot_streams([4, 4])
    assert e.value.code == host.E_INVAL
    assert sel.value == -7, "a refused call writes no selection"
    assert d.image_count() == images and np.array_equal(d.streams_paused(), paused)
    for s in range(S): assert d.collect_bulk(s) == before[s], s
    d.close()


def host_dump_bytes():
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    assert "#define DSPI_FLASH_DUMP_BYTES (12 * 4096)" in text
    return 12 * 4096
