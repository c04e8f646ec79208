"""Realignment without a GPU (DSPI_SNAP_REALIGN, dspi_realign_streams, include/dspi.h): the target rule and the rotation's index arithmetic
(dspi_amd/csrc/dspi_snapshot.h) through a g++ driver (tests/realign_driver.cpp), and the calls' argument checks on host-only contexts."""
import ctypes as C
import os
import subprocess

import pytest

from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
LINE = {0: 2048, 1: 4096}
RING = 1024


def build(tmp, name, *sources):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), *sources], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("realign"), "realign_driver", os.path.join(ROOT, "tests", "realign_driver.cpp"))


@pytest.fixture(scope="module")
def snap_driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("realign_snap"), "snapshot_driver", os.path.join(ROOT, "tests", "snapshot_driver.cpp"), os.path.join(CSRC, "dspi_snapshot.cpp"))


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()


def targets(driver, R, n, first, count):
    out = {}
    for ln in run(driver, "target", R, n, first, count):
        w = ln.split()
        out[int(w[1])] = (int(w[3]), bool(int(w[5])))
    return out


def test_the_library_exports_the_new_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_realign_streams") and hasattr(L, "dspi_debug_stream_positions")
    assert host.SNAP_REALIGN == 0x100


@pytest.mark.parametrize("R", [64, 128])
def test_target_rule(driver, R):
    n = 5 * R
    # resident below the range: the row's first stream
    assert targets(driver, R, n, R + 7, 20) == {1: (R, True)}
    # resident above the range only: the stream behind the range's end
    assert targets(driver, R, n, R, 20) == {1: (R + 20, True)}
    assert targets(driver, R, n, R, R - 1) == {1: (2 * R - 1, True)}
    # ... a resident below wins over one above (the lowest-numbered one)
    assert targets(driver, R, n, R + 1, 5) == {1: (R, True)}
    # no resident: the first stream of the range that lands in the row, from its record
    assert targets(driver, R, n, R, R) == {1: (R, False)}
    assert targets(driver, R, n, 0, n) == {r: (r * R, False) for r in range(5)}
    # a range ending past the row: first row has a resident below, middle rows none, the last one above
    assert targets(driver, R, n, R - 9, 2 * R + 13) == {0: (0, True), 1: (R, False), 2: (2 * R, False), 3: (3 * R + 4, True)}
    # ... and ending exactly on a row boundary
    assert targets(driver, R, n, R - 9, R + 9) == {0: (0, True), 1: (R, False)}
    # the last row cut by n_streams: streams at and past n_streams are nobody's neighbours
    cut = 2 * R + 10
    assert targets(driver, R, cut, 2 * R, 10) == {2: (2 * R, False)}
    assert targets(driver, R, cut, 2 * R, 9) == {2: (2 * R + 9, True)}
    assert targets(driver, R, cut, 2 * R + 3, 7) == {2: (2 * R, True)}
    assert targets(driver, R, cut, R, R + 10) == {1: (R, False), 2: (2 * R, False)}
    # one stream: into the row's first slot (the neighbour is the second), anywhere else (the first)
    assert targets(driver, R, n, 3 * R, 1) == {3: (3 * R + 1, True)}
    assert targets(driver, R, n, 3 * R + 40, 1) == {3: (3 * R, True)}
    # a one-stream context has no neighbour at all
    assert targets(driver, R, 1, 0, 1) == {0: (0, False)}


def test_target_rule_does_not_depend_on_chunking(driver):
    """A host-buffer import and dspi_realign_streams go through scratch in chunks that end on row boundaries (2 float rows / 8 Q28 rows): every
    row's target is the same whether the rule sees the whole range or the row's chunk."""
    for R, rows in ((128, 2), (64, 8)):
        n = 21 * R + 17
        for first, count in ((0, n), (5, n - 5), (R + 3, 9 * R), (3 * R, 17 * R + 1), (2 * R - 1, 2)):
            whole = targets(driver, R, n, first, count)
            s, end, parts = first, first + count, {}
            while s < end:
                e = min(end, (s // R + rows) * R)
                parts.update(targets(driver, R, n, s, e - s))
                s = e
            assert parts == whole, (R, first, count)


@pytest.mark.parametrize("length", [2048, 4096, RING])
def test_rotation_index_arithmetic(driver, length):
    """Every d in [0, L) at p in {0, 1, L - 1}: a bijection that maps the record's write position onto the target."""
    assert run(driver, "sweep", length) == ["ok"]
    # the issue's two cases by hand: 576 -> 336 (a row that is 240 frames younger) and 540 -> 315 (shift odd and not a multiple of four)
    for w_s, w_t in ((576, 336), (540, 315), (0, length - 1), (length - 1, 0), (7, 7)):
        out = run(driver, "rotate", length, w_s, w_t, 0, 1, length - 1, w_t)
        d = (w_t - w_s) % length
        assert out[0] == f"shift {d}"
        assert out[1:5] == [f"src 0 {(0 - d) % length}", f"src 1 {(1 - d) % length}", f"src {length - 1} {(length - 1 - d) % length}", f"src {w_t} {w_s}"]
        assert out[5:] == [f"lands {w_t}", "bijection 1"]
    assert run(driver, "rotate", length, 540, 315)[0] == f"shift {length - 225}"


@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_context(snap_driver, flavor, tmp_path):
    d = Dspi(flavor, 300, device=None)
    L = d.L
    hb, sb = d.snapshot_sizes(0, 4)
    head, state = C.create_string_buffer(hb), C.create_string_buffer(sb)
    snap = host._Snapshot(C.addressof(head), hb, C.addressof(state), sb)
    # the export refuses the flag, alone or with DSPI_MEM_DEVICE
    for flags in (host.SNAP_REALIGN, host.SNAP_REALIGN | host.MEM_DEVICE):
        assert L.dspi_export_streams(d.h, 0, 4, C.byref(snap), flags) == host.E_INVAL
        assert b"flag bits" in L.dspi_last_error(d.h)
    # the import takes it: an empty head fails on its magic, not on the flag bits
    for flags in (0x100, 0x101):
        assert L.dspi_import_streams(d.h, 0, C.byref(snap), flags) == host.E_INVAL
        err = L.dspi_last_error(d.h)
        assert b"magic" in err and b"flag bits" not in err, err
    # ... other bits beside it are still refused
    for bad in (0x100 | 0x2, 0x100 | 0x200, 0x100 | 0x80000000):
        assert L.dspi_import_streams(d.h, 0, C.byref(snap), bad) == host.E_INVAL and b"flag bits" in L.dspi_last_error(d.h), hex(bad)
    # a well-formed head reaches the missing device; range and state size are checked before that
    path = tmp_path / "head.bin"
    run(snap_driver, "write", flavor, 0, 4, 2, path)
    good = path.read_bytes()

    def imp(first, flags, state_bytes=sb):
        hbuf = C.create_string_buffer(good, len(good))
        return L.dspi_import_streams(d.h, first, C.byref(host._Snapshot(C.addressof(hbuf), len(good), C.addressof(state), state_bytes)), flags)
    for flags in (0x100, 0x101):
        assert imp(0, flags) == host.E_NODEVICE and imp(296, flags) == host.E_NODEVICE
        assert imp(297, flags) == host.E_INVAL
        assert imp(0, flags, state_bytes=sb - 1) == host.E_SHORT
    assert d.image_count() == 1      # nothing was taken in
    # dspi_realign_streams: the range first, then the missing device
    for first, count in ((0, 0), (300, 1), (299, 2), (0, 301), (0xFFFFFFFF, 2)):
        assert L.dspi_realign_streams(d.h, first, count) == host.E_INVAL, (first, count)
        assert b"range" in L.dspi_last_error(d.h)
    for first, count in ((0, 300), (299, 1), (100, 70)):
        assert L.dspi_realign_streams(d.h, first, count) == host.E_NODEVICE
    with pytest.raises(DspiError) as e:
        d.realign_streams(0, 300)
    assert e.value.code == host.E_NODEVICE
    # dspi_debug_stream_positions likewise
    w, r = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    assert L.dspi_debug_stream_positions(d.h, 298, 4, w, r) == host.E_INVAL
    assert L.dspi_debug_stream_positions(d.h, 0, 4, None, r) == host.E_INVAL
    assert L.dspi_debug_stream_positions(d.h, 0, 4, w, r) == host.E_NODEVICE
    d.close()
