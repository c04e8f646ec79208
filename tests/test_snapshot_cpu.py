"""Stream snapshots without a GPU: the record layout and the head (dspi_amd/csrc/dspi_snapshot.{h,cpp}) through a g++ driver
(tests/snapshot_driver.cpp), and the three calls of include/dspi.h on host-only contexts."""
import ctypes as C
import os
import subprocess

import pytest

from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")

# what dspi_image.h's make_state_map gives, written out independently: channels, outputs, line length, row width
FLAVORS = {0: dict(n_ch=7, n_out=5, max_delay=2048, row=64), 1: dict(n_ch=11, n_out=9, max_delay=4096, row=128)}
RING, PDM, BANDS = 1024, 9, 10


def n_slots(n_ch):
    # EQ pairs, loudness (2 channels x 2 stages x 2), crossfeed 4, leveller 5, ring position, write index, mute 3, peaks, 4 clip slots
    return n_ch * BANDS * 2 + 8 + 4 + 5 + 1 + 1 + 3 + n_ch + 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("snap") / "snapshot_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "snapshot_driver.cpp"),
                    os.path.join(CSRC, "dspi_snapshot.cpp")], check=True)
    return str(exe)


def run(driver, *args):
    return subprocess.run([driver, *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()


def parse_layout(lines):
    out, cur = {}, None
    for ln in lines:
        w = ln.split()
        if w[0] == "flavor":
            cur = dict(zip(w[2::2], map(int, w[3::2]))); cur["sections"] = []
            out[int(w[1])] = cur
        else:
            cur["sections"].append(tuple(map(int, w[2:])))
    return out


def test_record_layout(driver):
    lay = parse_layout(run(driver, "layout"))
    assert sorted(lay) == [0, 1]
    for flavor, f in FLAVORS.items():
        l = lay[flavor]
        assert (l["n_slots"], l["n_out"], l["max_delay"], l["ring"], l["pdm"], l["row"]) == (n_slots(f["n_ch"]), f["n_out"], f["max_delay"], RING, PDM, f["row"])
        want = [n_slots(f["n_ch"]), f["n_out"] * f["max_delay"], 2 * RING, PDM]
        assert [s[1] for s in l["sections"]] == want
        at = 0
        for off, ln, span in l["sections"]:      # ordered, disjoint, every section on a 16-byte boundary, no hole beyond the pad to four words
            assert off == at and off % 4 == 0 and span == (ln + 3) // 4 * 4
            at += span
        assert at == l["record_words"] and l["record_words"] % 4 == 0      # ... and they cover the record exactly
        assert l["stride"] == (l["params"] + 7) // 8 * 8 and l["header"] == 64


def test_head_sizes(driver):
    lay = parse_layout(run(driver, "layout"))
    stride = lay[1]["stride"]
    for count in (1, 2, 65536):
        for images in sorted({1, min(2, count), count}):
            hb, sb0, sb1 = map(int, run(driver, "head", count, images)[0].split())
            assert hb == 64 + images * stride + 4 * count
            assert sb0 == count * lay[0]["record_words"] * 4 and sb1 == count * lay[1]["record_words"] * 4
    # a whole float context: more than 2^32 bytes, so the sizes must not have been computed in 32 bits
    assert int(run(driver, "head", 65536, 1)[0].split()[2]) == 65536 * lay[1]["record_words"] * 4 > 1 << 33


def test_header_validation(driver):
    v = dict(ln.split(": ", 1) for ln in run(driver, "validate"))
    assert v["ok"] == "ok" and v["longer buffer"] == "ok"
    want = {"magic": "wrong magic", "version": "unknown format version", "flavor": "other flavour", "contract": "other float contract",
            "other flavour context": "other flavour", "other contract context": "other float contract",
            "fingerprint": "fingerprint differs", "params size": "fingerprint differs", "record size": "record size differs",
            "count": "sizes do not add up", "count zero": "no streams", "image count": "image count out of range", "image count zero": "image count out of range",
            "image count other": "sizes do not add up", "head size": "sizes do not add up", "crc": "CRC mismatch", "flags": "CRC mismatch",
            "body byte": "CRC mismatch", "index byte": "CRC mismatch", "truncated": "truncated", "shorter than header": "shorter than its header",
            "index out of range": "image index out of range", "foreign parameter object": "parameter object of another flavour"}
    assert set(want) | {"ok", "longer buffer"} == set(v)
    for case, msg in want.items():
        assert msg in v[case], (case, v[case])
    # each kind of damage is named by its own message
    by_field = [v[k] for k in ("magic", "version", "flavor", "contract", "fingerprint", "count", "record size", "image count", "crc", "truncated")]
    assert len(set(by_field)) == len(by_field)


@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_context(driver, flavor, tmp_path):
    lay = parse_layout(run(driver, "layout"))[flavor]
    d = Dspi(flavor, 300, device=None)
    for first, count in ((0, 300), (0, 1), (299, 1), (100, 70)):
        assert d.snapshot_sizes(first, count) == (64 + lay["stride"] + 4 * count, count * lay["record_words"] * 4)
    # streams with parameters of their own carry one object each
    d.set_volume(-3 * 256, stream=7); d.set_volume(-5 * 256, stream=9)
    assert d.snapshot_sizes(0, 300)[0] == 64 + 3 * lay["stride"] + 4 * 300
    assert d.snapshot_sizes(8, 2)[0] == 64 + 2 * lay["stride"] + 4 * 2
    assert d.snapshot_sizes(10, 20)[0] == 64 + lay["stride"] + 4 * 20
    L = d.L
    hb, sb = d.snapshot_sizes(0, 4)
    head, state = C.create_string_buffer(hb), C.create_string_buffer(sb)
    snap = host._Snapshot(C.addressof(head), hb, C.addressof(state), sb)
    # a range past n_streams, an empty range, undefined flag bits: DSPI_E_INVAL
    z = C.c_size_t(0)
    assert L.dspi_snapshot_sizes(d.h, 299, 2, C.byref(z), C.byref(z)) == host.E_INVAL
    assert L.dspi_snapshot_sizes(d.h, 0, 0, C.byref(z), C.byref(z)) == host.E_INVAL
    assert L.dspi_snapshot_sizes(d.h, 0xFFFFFFFF, 2, C.byref(z), C.byref(z)) == host.E_INVAL
    assert L.dspi_export_streams(d.h, 298, 4, C.byref(snap), 0) == host.E_INVAL
    for bad in (0x2, 0x20, 0x80000000, 0x1 | 0x40):
        assert L.dspi_export_streams(d.h, 0, 4, C.byref(snap), bad) == host.E_INVAL, hex(bad)
        assert L.dspi_import_streams(d.h, 0, C.byref(snap), bad) == host.E_INVAL, hex(bad)
    # too small a buffer: DSPI_E_SHORT, before the missing device is looked at
    assert L.dspi_export_streams(d.h, 0, 4, C.byref(host._Snapshot(C.addressof(head), hb - 1, C.addressof(state), sb)), 0) == host.E_SHORT
    assert L.dspi_export_streams(d.h, 0, 4, C.byref(host._Snapshot(C.addressof(head), hb, C.addressof(state), sb - 1)), 0) == host.E_SHORT
    # valid arguments: a host-only context has no run-time state
    for flags in (0, host.MEM_DEVICE):
        assert L.dspi_export_streams(d.h, 0, 4, C.byref(snap), flags) == host.E_NODEVICE
    with pytest.raises(DspiError) as e:
        d.export_streams(0, 4)
    assert e.value.code == host.E_NODEVICE
    # import: an empty head is refused as malformed
    assert L.dspi_import_streams(d.h, 0, C.byref(snap), 0) == host.E_INVAL
    assert b"magic" in L.dspi_last_error(d.h)
    # ... a well-formed one of this flavour passes validation and meets the missing device; out of range, short state and the other
    # flavour are refused before that
    path = tmp_path / "head.bin"
    run(driver, "write", flavor, 0, 4, 2, path)
    good = path.read_bytes()
    assert len(good) == 64 + 2 * lay["stride"] + 16

    def imp(first, hd, state_bytes=sb, flags=0):
        hbuf = C.create_string_buffer(hd, len(hd))
        return L.dspi_import_streams(d.h, first, C.byref(host._Snapshot(C.addressof(hbuf), len(hd), C.addressof(state), state_bytes)), flags)
    assert imp(0, good) == host.E_NODEVICE and imp(296, good, flags=host.MEM_DEVICE) == host.E_NODEVICE
    assert imp(297, good) == host.E_INVAL
    assert imp(0, good, state_bytes=sb - 1) == host.E_SHORT
    assert imp(0, good[:-1]) == host.E_INVAL and b"truncated" in L.dspi_last_error(d.h)
    run(driver, "write", 1 - flavor, 0, 4, 2, path)
    assert imp(0, path.read_bytes()) == host.E_INVAL and b"flavour" in L.dspi_last_error(d.h)
    if flavor:
        run(driver, "write", 1, 1, 4, 2, path)
        assert imp(0, path.read_bytes()) == host.E_INVAL and b"contract" in L.dspi_last_error(d.h)
    assert d.image_count() == 3      # nothing was taken in
    d.close()
