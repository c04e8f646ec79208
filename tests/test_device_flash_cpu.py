"""A stream's own flash on host-only contexts (dspi_device_flash, dspi_flash_read, dspi_flash_write, DSPI_BOOT_STREAMS_OWN_FLASH;
include/dspi.h) against the firmware build of the oracle (oracle/_ref/libref_fw_*: the reference's own request handlers, main loop and
flash_storage.c over a RAM flash), both flavours and the FMA contract: the power-on flash byte for byte, a scripted sequence over every
directory request, a seeded random fuzz, boots from flash dumps, reboots from the stream's own flash.  After EVERY step the answer of every
GET request the library serves, the parameter blob, a collected slot image and the full 48 KB are equal.  Without the firmware build those
legs skip and the recorded fixtures of tests/golden/ (tools/gen_flash_fixture.py) are replayed instead; the rest needs no oracle."""
import base64
import json
import os
import struct
import zlib

import numpy as np
import pytest

import flash_script as FS
import orclib
from orclib import Oracle
from dspi_amd import host, wire as W
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FL = [(1, False), (1, True), (0, False)]
R = W.REQ
E_INVAL, E_UNSUPPORTED, E_SHORT = -10, -14, -15
DIRECTORY_REQUESTS = [("get", 0x51), ("get", 0x52), ("get", 0x90), ("get", 0x91), ("get", 0x92), ("get", 0x93), ("set", 0x94), ("get", 0x95), ("set", 0x96), ("get", 0x97),
           ("set", 0x98), ("get", 0x99), ("get", 0x9A)]      # (thirteen; 0xD4 and 0xD6, the other two that write the directory, are served in both modes)


def need_fw(flavor, fma):
    if not orclib.ref_available(flavor, "fw", fma): pytest.skip("needs the firmware build under oracle/_ref")


def devices(flavor, fma, flash=None, stream=1):
    """a firmware build and stream `stream` of a three-stream host-only context whose streams own flashes"""
    fw = Oracle(flavor, ref="fw", fma=fma, flash=flash)
    d = Dspi(flavor, 3, device=None, fma=fma)
    assert d.device_flash(1) == 1
    return fw, d, FS.FwDev(fw), FS.LibDev(d, stream)


def same(a, b, what):
    x, y = FS.observe(a), FS.observe(b)
    for (req, wv), p, q in zip(FS.PROBES, x["gets"], y["gets"]): assert p == q, f"{what}: GET {req:#x} wValue {wv}: {p!r} / {q!r}"
    assert x["bulk"] == y["bulk"], f"{what}: parameter blob"
    assert x["slot"] == y["slot"], f"{what}: collected slot image"
    if x["flash"] != y["flash"]:
        at = next(i for i in range(len(x["flash"])) if x["flash"][i] != y["flash"][i])
        raise AssertionError(f"{what}: flash differs first at byte {at} (sector {at // 4096}, offset {at % 4096})")


def run_script(a, b, script, what):
    for i, step in enumerate(script):
        ra, rb = FS.apply(a, step), FS.apply(b, step)
        assert ra == rb, f"{what} step {i} {step[:3]}: the firmware answers {ra!r}, the library {rb!r}"
        same(a, b, f"{what} after step {i} {step[:3]}")


# ---- symbols, header words, the mode ------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_device_flash", "dspi_flash_read", "dspi_flash_write"): assert hasattr(L, name), name
    assert host.BOOT_STREAMS_OWN_FLASH == 2 and host.FLASH_DUMP_BYTES == 12 * 4096
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + a stream's own flash: detect by symbol (dspi_device_flash; with it dspi_flash_read, dspi_flash_write, DSPI_BOOT_STREAMS_OWN_FLASH; additions only)",
                 "#define DSPI_BOOT_STREAMS_OWN_FLASH 0x2u",
                 "int dspi_device_flash(dspi_ctx *ctx, int enable);\n"
                 "int dspi_flash_read(dspi_ctx *ctx, uint32_t stream, void *dump, size_t cap);\n"
                 "int dspi_flash_write(dspi_ctx *ctx, uint32_t first, uint32_t count, const void *dump, size_t len);\n",
                 "NO NEW KERNEL", "NO TIMING FIGURE", "65 536 distinct flashes are 3.2 GB"):
        assert word in text, word
    section = text.split("/* ---- a stream's own flash:")[1].split("int dspi_device_flash(")[0]
    for heading in ("the mode", "cost", "requests", "the mute", "the directory", "broadcast", "dspi_flash_read", "dspi_flash_write", "boots", "travel", "not touched", "host-only contexts"):
        assert f" *   {heading} " in section, heading


@pytest.mark.parametrize("flavor,fma", FL)
def test_mode_off_is_unchanged(flavor, fma):
    d = Dspi(flavor, 4, device=None, fma=fma)
    assert d.device_flash(-1) == 0, "off after dspi_create"
    before = d.collect_bulk(2)
    for kind, req in DIRECTORY_REQUESTS:
        for wv in (0, 3, 10):
            if kind == "get": assert d.L.dspi_vendor_get(d.h, 2, req, wv, bytes(64), 64) == E_UNSUPPORTED, hex(req)
            else: assert d.vendor_set(req, wv, b"\x01\x02", stream=2) == E_UNSUPPORTED, hex(req)
    assert d.L.dspi_flash_read(d.h, 0, bytes(host.FLASH_DUMP_BYTES), host.FLASH_DUMP_BYTES) == E_INVAL
    assert d.L.dspi_flash_write(d.h, 0, 1, bytes(host.FLASH_DUMP_BYTES), host.FLASH_DUMP_BYTES) == E_INVAL
    with pytest.raises(DspiError) as e: d.boot_streams([1], own_flash=True)
    assert e.value.code == E_INVAL and d.collect_bulk(2) == before
    assert d.device_flash(1) == 1 and d.device_flash(-1) == 1 and d.device_flash(1) == 1
    assert d.vendor_get(R["PRESET_GET_DIR"], 0, stream=2) == bytes([0, 0, 0, 0, 0, 1, 0])
    assert d.device_flash(0) == 0 and d.vendor_get(R["PRESET_GET_DIR"], 0, stream=2) is None, "turning it off drops the flashes"
    d.close()


@pytest.mark.parametrize("flavor,fma", FL)
def test_validation(flavor, fma):
    d = Dspi(flavor, 4, device=None, fma=fma)
    d.device_flash(1)
    n, dump = host.FLASH_DUMP_BYTES, bytes([7]) * host.FLASH_DUMP_BYTES
    keep = [d.flash_read(s) for s in range(4)]
    for first, count, length, want in ((0, 0, n, E_INVAL), (2, 3, n, E_INVAL), (4, 1, n, E_INVAL), (0xFFFFFFFF, 2, n, E_INVAL), (0, 4, n - 1, E_SHORT)):
        assert d.L.dspi_flash_write(d.h, first, count, dump, length) == want, (first, count, length)
    assert d.L.dspi_flash_read(d.h, 4, bytes(n), n) == E_INVAL and d.L.dspi_flash_read(d.h, 0, bytes(n), n - 1) == E_SHORT
    assert [d.flash_read(s) for s in range(4)] == keep, "ranges are validated before anything is written"
    with pytest.raises(DspiError) as e: d.boot_streams([1], dump=keep[0], own_flash=True)
    assert e.value.code == E_INVAL, "DSPI_BOOT_STREAMS_OWN_FLASH takes no dump"
    assert d.L.dspi_vendor_get(d.h, 1, R["PRESET_GET_NAME"], 10, bytes(64), 64) == E_UNSUPPORTED, "GET_NAME of a slot >= 10 stalls"
    assert d.L.dspi_vendor_get(d.h, 1, R["PRESET_GET_NAME"], 0, bytes(64), 31) == E_SHORT and d.L.dspi_vendor_get(d.h, 1, R["PRESET_SAVE"], 0, bytes(64), 0) == E_SHORT
    assert [d.flash_read(s) for s in range(4)] == keep, "a buffer that is too small is refused before anything is written"
    d.close()


# ---- against the firmware build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,fma", FL)
def test_power_on_flash(flavor, fma):
    need_fw(flavor, fma)
    fw, d, a, b = devices(flavor, fma)
    flash = fw.read_flash()
    assert all(d.flash_read(s) == flash for s in range(3)), "byte for byte the flash of a firmware that has just been powered on"
    assert flash[24:31] == b"Default" and set(flash[344:]) == {0xFF} and d.vendor_get(R["PRESET_GET_DIR"], 0, stream=2) == bytes([0, 0, 0, 0, 0, 1, 0])
    same(a, b, "power-on")
    fw.close(); d.close()


@pytest.mark.parametrize("flavor,fma", FL)
def test_scripted_sequence(flavor, fma):
    need_fw(flavor, fma)
    fw, d, a, b = devices(flavor, fma)
    untouched = FS.observe(FS.LibDev(d, 0))
    run_script(a, b, FS.scripted(flavor), "script")
    assert FS.observe(FS.LibDev(d, 0)) == untouched == FS.observe(FS.LibDev(d, 2)), "the neighbours' parameters and flashes are their own"
    # a second instance booted from that flash answers the same directory and writes nothing; so does the stream, rebooted from its own flash
    flash = fw.read_flash()
    fw2 = Oracle(flavor, ref="fw", fma=fma, flash=flash)
    assert fw2.read_flash() == flash
    d.boot_streams([1], own_flash=True)
    same(FS.FwDev(fw2), b, "rebooted from the own flash")
    fw.close(); fw2.close(); d.close()


@pytest.mark.parametrize("flavor,fma", FL)
def test_fuzz(flavor, fma):
    """24 seeded sequences of 30 requests; every eighth sequence ends with a reboot from the flash it left, and goes on"""
    need_fw(flavor, fma)
    for seq in range(24):
        rng = np.random.default_rng(1000 * (2 * flavor + fma) + seq)
        fw, d, a, b = devices(flavor, fma, stream=seq % 3)
        run_script(a, b, FS.random_script(rng, flavor, 30), f"sequence {seq}")
        if seq % 8 == 0:
            flash = fw.read_flash(); fw.close()
            fw = Oracle(flavor, ref="fw", fma=fma, flash=flash); a = FS.FwDev(fw)
            d.boot_streams([seq % 3], own_flash=True)
            same(a, b, f"sequence {seq} rebooted")
            run_script(a, b, FS.random_script(rng, flavor, 8), f"sequence {seq} after the reboot")
        fw.close(); d.close()


def boot_dumps(flavor):
    """the dumps of tests/test_oracle_vs_fw.py::test_boot_from_flash_dumps, and a legacy sector: (name, dump, selection)"""
    from test_oracle_vs_fw import _slots
    slots = _slots(flavor)
    occ = sum(1 << n for n in slots)
    D, F = W.flash_dump, W.flash_directory
    bad = dict(slots); x = bytearray(bad[4]); x[100] ^= 0x40; bad[4] = bytes(x)
    swapped = dict(slots); swapped[4] = slots[9]
    broken = bytearray(F(default_slot=4, slot_occupied=occ)); broken[30] ^= 1
    future = bytearray(F(default_slot=4, slot_occupied=occ)); future[4] = 3
    return [("default slot", D(F(default_slot=4, last_active_slot=9, slot_occupied=occ, master_volume_db=-17.0), slots), 4),
            ("last active", D(F(startup_mode=1, default_slot=4, last_active_slot=9, slot_occupied=occ, master_volume_mode=1), slots), 9),
            ("last active out of range", D(F(startup_mode=1, default_slot=4, last_active_slot=77, slot_occupied=occ), slots), 4),
            ("default out of range", D(F(startup_mode=0, default_slot=200, slot_occupied=occ), slots), 0),
            ("not occupied", D(F(default_slot=2, slot_occupied=occ), slots), 16 + 2),
            ("corrupt slot", D(F(default_slot=4, slot_occupied=occ), bad), 16 + 4),
            ("slot index mismatch", D(F(default_slot=4, slot_occupied=occ), swapped), 16 + 4),
            ("no directory", D(None, slots), 48),
            ("v1 directory", D(F(version=1, default_slot=9, slot_occupied=occ, master_volume_mode=1, names={9: "Night"}), slots), 9),
            ("directory CRC", D(bytes(broken), slots), 48),
            ("future version", D(bytes(future), slots), 48),
            ("legacy sector", W.flash_dump(None, {}, legacy=W.legacy_sector_from_slot(slots[4], flavor)), 32)]


@pytest.mark.parametrize("flavor,fma", FL)
def test_boots_from_flash_dumps(flavor, fma):
    """dspi_boot_streams(dump) and dspi_load_flash_dump leave the firmware build's flash (a created directory, a v1 directory persisted as v2, a
    legacy sector migrated into slot 0), and the requests go on from there as the firmware's do"""
    need_fw(flavor, fma)
    follow = [["get", R["PRESET_GET_DIR"], 0], ["set", R["PRESET_SET_NAME"], 2, b"after".hex()], ["get", R["PRESET_LOAD"], 4], ["get", 0x51, 0], ["get", R["PRESET_DELETE"], 9]]
    for name, dump, sel in boot_dumps(flavor):
        fw = Oracle(flavor, ref="fw", fma=fma, flash=dump)
        d = Dspi(flavor, 3, device=None, fma=fma); d.device_flash(1)
        assert d.boot_streams([2, 0], dump=dump) == sel, name
        a, b = FS.FwDev(fw), FS.LibDev(d, 2)
        same(a, b, f"booted from '{name}'")
        assert d.flash_read(0) == d.flash_read(2) and d.flash_read(1) != d.flash_read(2)
        run_script(a, b, follow, f"booted from '{name}'")
        # the running device that switches to the dump's preset (dspi_load_flash_dump) holds the same flash
        e = Dspi(flavor, 2, device=None, fma=fma); e.device_flash(1)
        assert e.load_flash_dump(dump, stream=1) == sel and e.flash_read(1) == Oracle(flavor, ref="fw", fma=fma, flash=dump).read_flash(), name
        # DSPI_BOOT_STREAMS_OWN_FLASH equals Oracle(ref="fw", flash=that_flash): carried by dspi_flash_write (boots nothing), then rebooted
        g = Dspi(flavor, 3, device=None, fma=fma); g.device_flash(1)
        live = g.save_slot(3, 1)
        assert g.flash_write(0, 2, dump) == 2 and g.flash_read(1) == dump and g.save_slot(3, 1) == live, "the bytes are replaced, nothing boots"
        assert g.boot_streams([1, 0], own_flash=True) == sel, name
        assert g.image_count() == 2, "the listed streams share one parameter object per distinct flash object"
        fw2 = Oracle(flavor, ref="fw", fma=fma, flash=dump)
        same(FS.FwDev(fw2), FS.LibDev(g, 1), f"own-flash reboot from '{name}'")
        same(FS.FwDev(fw2), FS.LibDev(g, 0), f"own-flash reboot from '{name}', the sharer")
        for x in (fw, fw2, d, e, g): x.close()


@pytest.mark.parametrize("flavor,fma", FL)
def test_null_boot_and_populated_contexts(flavor, fma):
    need_fw(flavor, fma)
    fw, d, a, b = devices(flavor, fma)
    run_script(a, b, [["get", R["PRESET_SAVE"], 3], ["set", R["SET_MASTER_VOLUME_MODE"], 0, "01"]], "before")
    d.boot_streams([1])                                            # dump NULL: the first-boot flash again
    fw.close(); fw = Oracle(flavor, ref="fw", fma=fma)
    same(FS.FwDev(fw), b, "dspi_boot_streams(NULL)")
    p = Dspi(flavor, 2, device=None, fma=fma, populated_flash=True)
    p.device_flash(1)
    assert set(p.flash_read(0)) == {0xFF}, "a DSPI_BOOT_POPULATED_FLASH context: an erased directory"
    assert p.vendor_get(R["PRESET_GET_DIR"], 0, stream=0) == bytes([0, 0, 0, 0, 0, 1, 0]) and p.vendor_get(R["PRESET_GET_NAME"], 0, stream=0)[:8] == b"Default\0"
    p.vendor_set(R["PRESET_SET_NAME"], 1, b"one", stream=0)
    assert p.flash_read(0)[:4] == b"2PSD" and set(p.flash_read(1)) == {0xFF}, "... which reaches the flash with the next flush"
    fw.close(); d.close(); p.close()


# ---- the book through the C ABI (no oracle needed) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,fma", FL)
def test_sharing_broadcast_and_resize(flavor, fma):
    S = 7
    d = Dspi(flavor, S, device=None, fma=fma)
    d.vendor_set(R["SET_PREAMP"], 0, struct.pack("<f", -5.0), stream=4)      # two parameter objects before the mode goes on
    d.device_flash(1)
    d.vendor_set(R["PRESET_SET_NAME"], 2, b"mine", stream=5)                 # ... and a flash of its own for stream 5
    name = lambda s, k: d.vendor_get(R["PRESET_GET_NAME"], k, stream=s).rstrip(b"\0")
    assert [name(s, 2) for s in range(S)] == [b""] * 5 + [b"mine", b""]
    # a broadcast: once per distinct (parameter object, flash object) pair; every stream saves ITS parameters into ITS flash
    assert d.vendor_get(R["PRESET_SAVE"], 6, stream=host.ALL) == b"\x00"
    flashes = [d.flash_read(s) for s in range(S)]
    assert len(set(flashes)) == 3 and flashes[0] == flashes[1] == flashes[2] == flashes[3] == flashes[6] and flashes[4] != flashes[0] != flashes[5]
    assert name(5, 2) == b"mine" and d.vendor_get(R["PRESET_GET_DIR"], 0, stream=5)[:2] == bytes([0x40, 0])
    slot6 = lambda f: f[7 * 4096:7 * 4096 + len(d.save_slot(0))]
    assert slot6(flashes[4]) == d.save_slot(6, 4) != slot6(flashes[0]) == d.save_slot(6, 0) == slot6(flashes[5])
    assert d.image_count() == 2, "stream 5's parameters equal the others' again (the same mute stands): the objects fold back whatever their flashes"
    d.vendor_set(R["PRESET_SET_NAME"], 1, b"all", stream=host.ALL)
    assert [name(s, 1) for s in range(S)] == [b"all"] * S and name(5, 2) == b"mine" and len({d.flash_read(s) for s in range(S)}) == 3
    # grow: the new slots share one first-boot flash; shrink: released
    first = Dspi(flavor, 1, device=None, fma=fma); first.device_flash(1)
    d.resize_streams(S + 3)
    assert [d.flash_read(s) for s in range(S, S + 3)] == [first.flash_read(0)] * 3
    d.vendor_set(R["PRESET_SET_NAME"], 0, b"grown", stream=S + 1)
    assert name(S + 1, 0) == b"grown" and name(S, 0) == name(S + 2, 0) == b"Default"
    d.pause_streams(S, 3); d.resize_streams(S)
    with pytest.raises(DspiError): d.flash_read(S)
    assert name(5, 2) == b"mine"
    d.close(); first.close()


def test_snapshots_do_not_carry_the_flash():
    """dspi_flash_read / dspi_flash_write carry it beside a snapshot; dspi_flash_write takes the three mirrors from the new directory"""
    a, b = Dspi(1, 2, device=None), Dspi(1, 3, device=None)
    a.device_flash(1); b.device_flash(1)
    a.vendor_set(R["SET_MASTER_VOLUME"], 0, struct.pack("<f", -33.0), stream=1)
    a.vendor_get(R["SAVE_MASTER_VOLUME"], 0, stream=1); a.vendor_set(R["SET_MASTER_VOLUME_MODE"], 0, b"\x01", stream=1); a.vendor_set(R["PRESET_SET_INCLUDE_PINS"], 0, b"\x00", stream=1)
    f = a.flash_read(1)
    assert b.flash_write(1, 2, f) == 2 and b.flash_read(1) == f == b.flash_read(2) and b.flash_read(0) != f
    for s in (1, 2):
        assert b.vendor_get(R["GET_SAVED_MASTER_VOLUME"], 0, stream=s) == struct.pack("<f", -33.0) and b.vendor_get(R["GET_MASTER_VOLUME_MODE"], 0, stream=s) == b"\x01"
        assert b.vendor_get(R["PRESET_GET_INCLUDE_PINS"], 0, stream=s) == b"\x00" and b.vendor_get(R["GET_MASTER_VOLUME"], 0, stream=s) == struct.pack("<f", -20.0), "the live parameters stay"
    assert b.vendor_get(R["GET_MASTER_VOLUME_MODE"], 0, stream=0) == b"\x00"
    b.vendor_set(R["PRESET_SET_NAME"], 0, b"two", stream=2)
    assert b.flash_read(1) == f != b.flash_read(2), "one shared object until one of them writes"
    a.close(); b.close()


# ---- the recorded fixtures (machines without the firmware build) ----------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (1, 0))
def test_replay_recorded_fixture(flavor):
    with open(os.path.join(ROOT, "tests", "golden", f"device_flash_{'f32' if flavor else 'q28'}.json")) as f: fx = json.load(f)
    assert fx["flavor"] == flavor and len(fx["steps"]) == len(fx["answers"]) >= 60
    d = Dspi(flavor, 2, device=None)
    d.device_flash(1)
    dev = FS.LibDev(d, 1)
    enc = lambda r: r.hex() if isinstance(r, bytes) else r
    for i, (step, want) in enumerate(zip(fx["steps"], fx["answers"])):
        assert enc(FS.apply(dev, step)) == want, f"step {i} {step[:3]}"
    got = FS.observe(dev)
    assert [enc(g) for g in got["gets"]] == fx["gets"] and fx["probes"] == [list(p) for p in FS.PROBES]
    assert got["bulk"].hex() == fx["bulk"] and got["slot"].hex() == fx["slot"]
    assert got["flash"] == zlib.decompress(base64.b64decode(fx["flash"])), "the final flash"
    d.close()
