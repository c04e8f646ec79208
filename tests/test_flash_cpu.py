"""A stream's own flash without a GPU, the book and the sector rules (dspi_amd/csrc/dspi_flash.{h,cpp}) through a g++ driver
(tests/flash_driver.cpp) — built twice, plainly and as a stand-alone program under AddressSanitizer + UBSan, and every driver case runs on
both: clone on write and reference counts, a broadcast's (parameter object, flash object) pairs, moves with swaps, cycles and open ends,
arrivals by value, boots, grows and shrinks; a sector write's padding, the directory's CRC, the version 1 conversion, the fresh directory,
the legacy migration.  The requests themselves are tests/test_device_flash_cpu.py's, against the firmware build."""
import os
import struct
import subprocess
import zlib

import pytest

from dspi_amd import wire as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("flash_" + request.param) / "flash_driver"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (SAN if request.param == "sanitized" else ["-O2"]) +
                   ["-o", str(exe), os.path.join(ROOT, "tests", "flash_driver.cpp"), os.path.join(CSRC, "dspi_flash.cpp"), os.path.join(CSRC, "dspi_params.cpp")], check=True)
    return str(exe)


def run(driver, mode, cases):
    """one line of input per case, one line of output per case; a sanitizer report ends the program with a failure"""
    p = subprocess.run([driver, mode], input="".join(c + "\n" for c in cases), capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return out


def book(driver, script):
    f = [x.strip() for x in run(driver, "book", [script])[0].split("|")]
    num = lambda s: [int(v) for v in s.split()[1:]]
    return dict(tags=num(f[0]), objs=num(f[1]), refs=num(f[2]), distinct=num(f[3])[0], src_tags=num("x " + f[4][len("src tags"):]), src_distinct=int(f[5].split()[-1]))


# ---- the book ---------------------------------------------------------------------------------------------------------------------------
def test_clone_on_write_and_reference_counts(driver):
    b = book(driver, "n 6")
    assert b["tags"] == [0] * 6 and b["refs"] == [6] and b["distinct"] == 1, "streams share one object until one writes"
    b = book(driver, "n 6 w 2 7")
    assert b["tags"] == [0, 0, 7, 0, 0, 0] and sorted(b["refs"]) == [1, 5] and b["distinct"] == 2, "a write clones first"
    b = book(driver, "n 6 w 2 7 w 2 8 w 2 9")
    assert b["tags"] == [0, 0, 9, 0, 0, 0] and b["distinct"] == 2, "the only holder writes in place"
    b = book(driver, "n 2 w 0 1 w 1 2")
    assert b["tags"] == [1, 2] and b["refs"] == [1, 1] and b["distinct"] == 2, "the last holder of the original keeps it: no third object"
    b = book(driver, "n 3 w 0 1 w 1 2 w 2 3 drop")
    assert b["tags"] == [] and b["distinct"] == 0


def test_broadcast_pairs(driver):
    got = run(driver, "pairs", ["0,0,0,0 0,0,0,0", "0,0,1,1,0 0,1,1,1,0", "3,2,3,2 5,5,4,5", "1 9"])
    assert got[0] == "0:0@0 | 0 0 0 0", "streams that share both are ONE pair: the request is applied once"
    assert got[1] == "0:0@0 0:1@1 1:1@2 | 0 1 2 2 0"
    assert got[2] == "3:5@0 2:5@1 3:4@2 | 0 1 2 1"
    assert got[3] == "1:9@0 | 0"


def test_moves(driver):
    base = "n 6 w 1 1 w 2 2 w 3 3 "                      # tags 0 1 2 3 0 0, streams 0, 4 and 5 share the original
    assert book(driver, base)["tags"] == [0, 1, 2, 3, 0, 0]
    b = book(driver, base + "mv 1>2,2>1")
    assert b["tags"] == [0, 2, 1, 3, 0, 0] and sorted(b["refs"]) == [1, 1, 1, 3], "a swap"
    b = book(driver, base + "mv 1>2,2>3,3>1")
    assert b["tags"] == [0, 3, 1, 2, 0, 0] and b["distinct"] == 4, "a cycle: all sources are read before any destination is written"
    b = book(driver, base + "mv 1>4")
    assert b["tags"] == [0, 1, 2, 3, 1, 0] and sorted(b["refs"]) == [1, 1, 2, 2], "an open end: the source keeps its reference, by reference at the destination"
    b = book(driver, base + "mv 1>2")
    assert b["tags"] == [0, 1, 1, 3, 0, 0] and b["distinct"] == 3, "the destination's occupant lost its last holder: the object is freed"
    b = book(driver, base + "mv 1>2 w 2 9")
    assert b["tags"] == [0, 1, 9, 3, 0, 0], "after a move by reference a write still clones"
    b = book(driver, base + "mv 3>5,1>3,5>1")
    assert b["tags"] == [0, 0, 2, 1, 0, 3]


def test_arrive_and_leave(driver):
    b = book(driver, "n 4 w 3 5 sn 4 sw 1 9 sw 2 9 ar 1>0,0>2,3>1")
    assert b["tags"] == [9, 0, 0, 5] and b["src_tags"] == [0, 9, 9, 0], "by value; the source's slots keep theirs"
    assert b["src_distinct"] == 3 and b["distinct"] == 3, "src 0 and 3 share one object: it is copied once; main 3 keeps its own"
    assert b["objs"][1] == b["objs"][2] != b["objs"][0]
    b = book(driver, "n 2 sn 2 sw 0 4 ar 0>1 w 1 6")
    assert b["tags"] == [0, 6] and b["src_tags"] == [4, 0], "a write after the arrival does not reach the source"


def test_boot_grow_shrink(driver):
    b = book(driver, "n 5 w 1 1 bt 8 1,3")
    assert b["tags"] == [0, 8, 0, 8, 0] and sorted(b["refs"]) == [2, 3] and b["distinct"] == 2, "booted slots share the new object; slot 1's own is freed"
    b = book(driver, "n 3 w 2 2 rs 6 4")
    assert b["tags"] == [0, 0, 2, 4, 4, 4] and sorted(b["refs"]) == [1, 2, 3], "new slots share ONE flash"
    b = book(driver, "n 3 w 2 2 rs 6 4 w 4 5 rs 4 0")
    assert b["tags"] == [0, 0, 2, 4] and b["distinct"] == 3, "a shrink releases: the clone of slot 4 is gone"
    b = book(driver, "n 3 w 2 2 rs 2 0 rs 3 7")
    assert b["tags"] == [0, 0, 7] and b["distinct"] == 2 and sorted(b["refs"]) == [1, 2]


# ---- the sector rules -------------------------------------------------------------------------------------------------------------------
def sector(driver, script):
    f = [x.strip() for x in run(driver, "sector", [script])[0].split("|")]
    return dict(valid=int(f[0].split()[1]), wrote=int(f[1].split()[1]), dir=bytes.fromhex(f[2].split()[1]), cache=bytes.fromhex(f[3].split()[1]), used=[int(v) for v in f[4].split()[1:]])


def v2(startup=(0, 0, 0, 1), occupied=0, mode=0, db=-20.0, names=None):
    body = struct.pack("<BBBBHBBf", *startup, occupied, mode, 0, db) + b"".join((names or {}).get(n, b"").ljust(32, b"\0") for n in range(10))
    return struct.pack("<IHHI", 0x44535032, 2, 0, zlib.crc32(body) & 0xFFFFFFFF) + body


def test_sector_write_padding(driver):
    s = sector(driver, "write 3 300 170")
    assert s["used"] == [0, 0, 0, 300] + [0] * 8, "the payload, then 0xFF to the end of the sector"
    s = sector(driver, "write 3 4096 0 write 3 10 1")
    assert s["used"][3] == 10, "a write erases the sector first"
    s = sector(driver, "write 3 300 170 write 4 7 1 erase 3")
    assert s["used"][3] == 0 and s["used"][4] == 7 and s["valid"] == 0
    assert s["cache"] == v2()[12:24], "without a directory the requests see dir_ensure's fresh one"


@pytest.mark.parametrize("flavor", (1, 0))
def test_fresh_directory(driver, flavor):
    s = sector(driver, f"first {flavor} 0")
    fresh = v2(names={0: b"Default"})
    assert s["dir"] == fresh and s["valid"] == 1 and s["dir"][24:31] == b"Default"
    assert s["used"][1:] == [0] * 11 and s["used"][0] == sum(b != 0xFF for b in fresh), "bytes 0..343 are written, everything else is erased"
    assert struct.unpack_from("<I", s["dir"], 8)[0] == zlib.crc32(s["dir"][12:]) & 0xFFFFFFFF, "CRC-32 over everything after the 12-byte header"
    assert sector(driver, f"boot {flavor}") == dict(s, wrote=1), "a first boot writes exactly that"
    p = sector(driver, f"first {flavor} 1")
    assert p["used"] == [0] * 12 and p["valid"] == 1 and p["cache"] == fresh[12:24], "a populated context's flash: erased, the fresh directory in the cache only"
    assert sector(driver, f"first {flavor} 1 flush")["dir"] == fresh


def test_directory_validation_and_boot(driver):
    good = v2(startup=(1, 4, 9, 0), occupied=0x212, mode=1, db=-7.5, names={9: b"Night"})
    s = sector(driver, f"set {good.hex()} boot 1")
    assert s["valid"] == 1 and s["wrote"] == 0 and s["dir"] == good, "a valid directory: the boot writes nothing"
    assert s["cache"][:4] == bytes([1, 4, 9, 0])
    spec = v2(startup=(0, 4, 9, 1), occupied=0x212)
    s = sector(driver, f"set {spec.hex()} boot 1")
    assert s["dir"] == spec and s["cache"][:4] == bytes([0, 4, 4, 1]), "the boot sets last_active_slot in the cache only (flash_storage.c:1080)"
    s = sector(driver, f"set {spec.hex()} boot 1 flush")
    assert s["dir"] == v2(startup=(0, 4, 4, 1), occupied=0x212), "... and the next flush carries it to the flash"
    s = sector(driver, f"set {v2(startup=(1, 4, 77, 1)).hex()} boot 1")
    assert s["cache"][:4] == bytes([1, 4, 4, 1]), "a last active slot out of range falls back to the default slot"
    for name, broken in (("CRC", good[:30] + bytes([good[30] ^ 1]) + good[31:]), ("version 3", good[:4] + b"\x03" + good[5:]), ("magic", b"\x31" + good[1:])):
        s = sector(driver, f"set {broken.hex()}")
        assert s["valid"] == 0 and s["cache"] == v2()[12:24], name
        s = sector(driver, f"set {broken.hex()} boot 1")
        assert s["valid"] == 1 and s["wrote"] == 1 and s["dir"] == v2(names={0: b"Default"}), name + ": the boot creates a fresh directory"


def test_v1_conversion(driver):
    v1 = W.flash_directory(version=1, startup_mode=1, default_slot=9, last_active_slot=3, include_pins=0, slot_occupied=0x208, master_volume_mode=1, names={9: "Night", 3: "Day"})
    want = v2(startup=(1, 9, 3, 0), occupied=0x208, mode=1, db=-20.0, names={9: b"Night", 3: b"Day"})
    s = sector(driver, f"set {v1.hex()}")
    assert s["valid"] == 1 and s["dir"][:340] == v1[:340] and s["cache"] == want[12:24], "replacing the bytes converts in the cache and writes nothing"
    s = sector(driver, f"set {v1.hex()} boot 1")
    assert s["wrote"] == 1 and s["dir"] == want, "a boot persists the version 1 directory as version 2 (flash_storage.c:390-414)"
    assert s["used"][1:] == [0] * 11


@pytest.mark.parametrize("flavor", (1, 0))
def test_legacy_migration(driver, flavor):
    n_ch, n_out = (11, 9) if flavor else (7, 5)
    lb = 12 + n_ch * 12 * 16 + 4 + 4 + n_ch * 4 + 12 + 4 + 4 + 8 + 4 + 8 + 2 * n_out * 8 + n_out * 12 + 8
    s = sector(driver, f"legacy {flavor} 7 boot {flavor}")
    assert s["wrote"] == 1 and s["dir"] == v2(occupied=1, names={0: b"Migrated"})
    assert s["used"][1] > lb - 12 - 20 and s["used"][2:11] == [0] * 9 and s["used"][11] > 0, "the legacy data stands in slot 0's sector, the legacy sector stays"
    s = sector(driver, f"legacy {flavor} 7 write 11 4 1 boot {flavor}")
    assert s["dir"] == v2(names={0: b"Default"}) and s["used"][1] == 0, "a legacy sector that fails its test is not migrated"
