"""Resizing without a GPU: the validation rule, the row arithmetic and the new slots' work items (dspi_amd/csrc/dspi_resize.{h,cpp}) through a
g++ driver (tests/resize_driver.cpp) — built twice, plainly and as a stand-alone program under AddressSanitizer + UBSan, and every driver
case runs on both —, and dspi_resize_streams / dspi_reserve_streams / dspi_stream_capacity (include/dspi.h) on host-only contexts, where the
calls keep every book: parameter objects, references, activity, per-stream S/PDIF positions and the capacity number."""
import os
import subprocess

import numpy as np
import pytest

from dspi_amd import host, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_boot_cpu import bits, expected_masks, parse_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("resize_" + request.param) / "resize_driver"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (SAN if request.param == "sanitized" else ["-O2"]) +
                   ["-o", str(exe), os.path.join(ROOT, "tests", "resize_driver.cpp"), os.path.join(CSRC, "dspi_resize.cpp"), os.path.join(CSRC, "dspi_boot.cpp")], check=True)
    return str(exe)


def run(driver, mode, arg, cases):
    """one line of input per case, one line of output per case; a sanitizer report ends the program with a failure"""
    text = "".join(c + "\n" for c in cases)
    p = subprocess.run([driver, mode] + ([str(arg)] if arg is not None else []), input=text, capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return out


def rows_of(n, R):
    return -(-n // R)


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_resize_streams", "dspi_reserve_streams", "dspi_stream_capacity"): assert hasattr(L, name), name
    assert host.RESIZE_PAUSED == 1
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + resizing: detect by symbol (dspi_resize_streams; with it dspi_reserve_streams, dspi_stream_capacity, DSPI_RESIZE_PAUSED; additions only)",
                 "#define DSPI_RESIZE_PAUSED 0x1u   /* dspi_resize_streams, growing: the new slots arrive paused */\n"
                 "int dspi_resize_streams(dspi_ctx *ctx, uint32_t n_streams, uint32_t flags);   /* returns the new dspi_num_streams */\n"
                 "int dspi_reserve_streams(dspi_ctx *ctx, uint32_t n_streams);                  /* returns the new capacity */\n"
                 "uint32_t dspi_stream_capacity(const dspi_ctx *ctx);\n"):
        assert word in text, word
    for heading in ("what the call does", "new slots", "write positions", "activity", "open ends", "validation", "timing", "host-only contexts", "not touched"):
        assert f" *   {heading} " in text.split("/* ---- resizing:")[1].split("#define DSPI_RESIZE_PAUSED")[0], heading


# ---- the books, through the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (128, 64))
def test_validation(driver, R):
    S, N = 2 * R + 45, R + 10
    top = [1] * N + [0] * (S - N)                                  # [N, S) paused
    one = list(top); one[N + 7] = 1                                # ... but for one slot
    refused = {
        "a count of 0": (f"{S} 0 0 {bits([0] * S)}", "at least one stream"),
        "an active slot in the cut range": (f"{S} {N} 0 {bits(one)}", "is active"),
        "the last slot of the cut range is active": (f"{S} {S - 1} 0 {bits([0] * (S - 1) + [1])}", "is active"),
        "nothing is paused": (f"{S} {N} 0 -", "is active"),
        "flag bit 1": (f"{S} {S + 5} 0x2 -", "undefined flag"),
        "flag bit 31 beside the defined one": (f"{S} {S + 5} 0x80000001 -", "undefined flag"),
        "a flag bit on a shrink": (f"{S} {N} 0x4 {bits(top)}", "undefined flag"),
    }
    ok = {"shrink": f"{S} {N} 0 {bits(top)}", "shrink to one below a paused slot": f"{S} {S - 1} 0 {bits([1] * (S - 1) + [0])}",
          "DSPI_RESIZE_PAUSED on a shrink": f"{S} {N} 1 {bits(top)}", "shrink to 1": f"{S} 1 0 {bits([1] + [0] * (S - 1))}",
          "grow": f"{S} {S + 1} 0 -", "grow paused": f"{S} {3 * R} 1 {bits(one)}", "same size": f"{S} {S} 0 -"}
    got = run(driver, "validate", None, [c for c, _ in refused.values()] + list(ok.values()))
    for (name, (_, msg)), g in zip(refused.items(), got): assert msg in g, (name, g)
    for name, g in zip(ok, got[len(refused):]): assert g == "ok", (name, g)
    got = run(driver, "reserve", None, [f"{S} 0", f"{S} {S - 1}", f"{S} {S}", f"{S} {10 * S}", "1 1"])
    assert "at least one stream" in got[0] and "fewer streams" in got[1] and got[2:] == ["ok"] * 3
    got = run(driver, "bytes", None, ["3 100", "0 5", f"{1 << 26} {1 << 40}", f"{(1 << 32) - 1} {(1 << 32) + 2}", f"{(1 << 32) - 1} {(1 << 32) + 1}"])      # (the last: 2^64 - 1, the largest size_t)
    assert got == ["300", "0", "overflow", "overflow", str((1 << 64) - 1)]


@pytest.mark.parametrize("R", (128, 64))
def test_row_arithmetic(driver, R):
    changes = [(70, 100), (R - 1, R), (R, R + 1), (2 * R, 2 * R + 1), (300, 70), (300, R), (300, 1)]
    cases = []
    for a, b in changes:
        for cap in (rows_of(a, R), rows_of(max(a, b), R) + 2):      # capacity equal to use, and a larger one that holds both sizes
            cases.append((a, b, cap))
    got = [tuple(map(int, g.split())) for g in run(driver, "rows", R, [f"{a} {b} {cap}" for a, b, cap in cases])]
    for (a, b, cap), (before, after, capacity, copy, realloc) in zip(cases, got):
        assert (before, after) == (rows_of(a, R), rows_of(b, R)), (a, b)
        if rows_of(b, R) > cap: assert (capacity, copy, realloc) == (rows_of(b, R), rows_of(a, R), 1), (a, b, cap)      # exactly the rows needed, the rows in use come over
        else: assert (capacity, copy, realloc) == (cap, 0, 0), (a, b, cap)                                            # shrinks too: the capacity stays
    by = dict(zip(cases, got))
    assert by[(R - 1, R, 1)] == (1, 1, 1, 0, 0), "a row that fills up is no new row"
    assert by[(R, R + 1, 1)] == (1, 2, 2, 1, 1) and by[(R, R + 1, 4)] == (1, 2, 4, 0, 0)
    assert by[(2 * R, 2 * R + 1, 2)] == (2, 3, 3, 2, 1) and by[(2 * R, 2 * R + 1, 5)] == (2, 3, 5, 0, 0)
    assert by[(70, 100, rows_of(70, R))][2:] == (rows_of(70, R), 0, 0), "70 -> 100 stays in its row for both row widths"
    assert by[(300, 1, rows_of(300, R))] == (rows_of(300, R), 1, rows_of(300, R), 0, 0)
    # reserve: whichever way, and nothing where the capacity has the value already
    u = rows_of(70, R)
    res = [tuple(map(int, g.split())) for g in run(driver, "reserve_rows", R, [f"70 {3 * R} {u}", f"70 {3 * R} 3", f"70 {2 * R + 1} 3", f"70 70 3", f"70 70 {u}", f"70 {u * R} {u}", f"{R + 1} {R + 1} 9"])]
    assert res == [(u, u, 3, u, 1), (u, u, 3, 0, 0), (u, u, 3, 0, 0), (u, u, u, u, 1), (u, u, u, 0, 0), (u, u, u, 0, 0), (2, 2, 2, 2, 1)]


def new_slot_items(driver, R, cases):
    out = []
    for (a, b, _), g in zip(cases, run(driver, "items", R, [f"{a} {b} {act}" for a, b, act in cases])):
        head, rest = g.split("I", 1) if "I" in g else (g, "")
        assert head.split() == ["S", str(a), str(b - a)], g      # the new slots: [a, b), ascending
        items = parse_items("I" + rest) if rest else []
        # every item: the rows ascending, exactly the new slots' columns, both masks from their definition
        assert [it["row"] for it in items] == list(range(a // R, rows_of(b, R)))
        for it in items:
            cols = [s % R for s in range(a, b) if s // R == it["row"]]
            assert it["cols"] == cols
            assert (it["q_any"], it["q_all"]) == expected_masks(set(cols), R)
        out.append(items)
    return out


@pytest.mark.parametrize("R", (128, 64))
def test_new_slots(driver, R):
    r0 = 70 // R * R                                               # the first stream of the row that 70 -> 100 grows
    some = [1] * 70
    for s in (r0, r0 + 1, r0 + 2): some[s] = 0                     # its three lowest residents are paused
    none = [1] * 70
    for s in range(r0, 70): none[s] = 0                            # all of its residents are
    full = (1 << (R // 4)) - 1
    cases = [(70, 100, "-"), (70, 100, bits(some)), (70, 100, bits(none)),
             (R, 3 * R + 5, "-"),                                  # whole new rows, and a partial one
             (70, 2 * R + 1, bits(some)),                          # the grown row, a whole row, a row that holds one stream: no lane mate
             (R - 1, R, "-"), (R - 1, R, bits([0] * (R - 1))),     # one slot, the last of its row
             (1, 2, "-"), (2, 3, "-"),                             # a lane mate arrives; a stream without one
             (2 * R, 2 * R + 1, "-")]
    got = dict(zip([(a, b, act) for a, b, act in cases], new_slot_items(driver, R, cases)))
    tg = lambda key: [it["target"] for it in got[key]]
    assert tg(cases[0]) == [r0], "a partial row with active residents: the lowest of them"
    assert tg(cases[1]) == [r0 + 3], "... the lowest ACTIVE one"
    assert tg(cases[2]) == [-1], "a partial row whose residents are all paused has no target"
    assert tg(cases[3]) == [-1, -1, -1] and [(it["q_any"], it["q_all"]) for it in got[cases[3]]] == [(full, full), (full, full), (0b11, 0b1)], "whole new rows have no target"
    assert tg(cases[4]) == [r0 + 3] + [-1] * (rows_of(2 * R + 1, R) - 70 // R - 1)
    assert (got[cases[4]][-1]["cols"], got[cases[4]][-1]["q_any"], got[cases[4]][-1]["q_all"]) == ([0], 1, 0)
    assert tg(cases[5]) == [0] and tg(cases[6]) == [-1] and got[cases[5]][0]["q_any"] == 1 << (R // 4 - 1) and got[cases[5]][0]["q_all"] == 0
    assert tg(cases[7]) == [0] and got[cases[7]][0]["cols"] == [1] and tg(cases[8]) == [0] and got[cases[8]][0]["cols"] == [2]
    assert tg(cases[9]) == [-1], "the residents of other rows are nobody's target"


# ---- host-only contexts ---------------------------------------------------------------------------------------------------------------------
def loaded(flavor, S, **kw):
    d = Dspi(flavor, S, device=None, **kw)
    assert d.load_bulk(WL.full_chain_blob(flavor)) == 0
    return d


def power_on_bulk(flavor, **kw):
    f = Dspi(flavor, 1, device=None, **kw)
    try: return f.collect_bulk(0)
    finally: f.close()


def num_streams(d):
    return int(d.L.dspi_num_streams(d.h))


@pytest.mark.parametrize("flavor", [0, 1])
def test_grow(flavor):
    d = loaded(flavor, 70)
    R = d.tile_streams()
    assert d.stream_capacity() == rows_of(70, R) * R, "after dspi_create the capacity is the rows in use"
    assert d.load_bulk(WL.full_chain_blob(flavor, max_delay_ms=3.0), stream=9) == 0
    d.pause_streams(60, 5)
    images, paused = d.image_count(), d.streams_paused().copy()
    before = [d.collect_bulk(s) for s in range(70)]
    fresh = power_on_bulk(flavor)
    assert fresh != before[0] and before[9] != before[0] and images == 2
    assert d.resize_streams(70) == 70 and d.image_count() == images, "the same size does nothing"
    assert d.resize_streams(100) == 100 and num_streams(d) == 100 and d.n_streams == 100
    assert d.stream_capacity() == rows_of(100, R) * R
    assert np.array_equal(d.streams_paused(), np.concatenate([paused, np.zeros(30, dtype=np.uint8)])), "new slots are active"
    assert d.image_count() == images + 1, "all new slots share ONE new parameter object"
    for s in range(100): assert d.collect_bulk(s) == (before[s] if s < 70 else fresh), s
    # ... paused, into new rows; per-stream calls accept the new range and no further
    n = 2 * R + 1
    assert d.resize_streams(n, paused=True) == n and num_streams(d) == n and d.stream_capacity() == 3 * R
    assert np.array_equal(d.streams_paused(), np.concatenate([paused, np.zeros(30, dtype=np.uint8), np.ones(n - 100, dtype=np.uint8)]))
    for s in range(n): assert d.collect_bulk(s) == (before[s] if s < 70 else fresh), s
    assert d.image_count() == images + 1      # (equal objects fold)
    with pytest.raises(DspiError): d.collect_bulk(n)
    assert d.load_bulk(WL.full_chain_blob(flavor), stream=n - 1) == 0 and d.collect_bulk(n - 1) == before[0] and d.collect_bulk(n - 2) == fresh
    assert d.resume_streams(100, n - 100) == n - 100 and not d.streams_paused()[100:].any()
    d.close()


def test_grow_populated_flash_context():
    d = Dspi(1, 70, device=None, populated_flash=True)
    ref = d.collect_bulk(0)
    assert ref == power_on_bulk(1, populated_flash=True)
    assert d.load_bulk(WL.full_chain_blob(1)) == 0
    assert d.resize_streams(200) == 200
    assert d.collect_bulk(70) == ref and d.collect_bulk(199) == ref and d.collect_bulk(69) != ref and d.image_count() == 2
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_shrink(flavor):
    d = loaded(flavor, 300)
    R = d.tile_streams()
    assert d.load_bulk(WL.full_chain_blob(flavor, max_delay_ms=3.0), stream=250) == 0
    d.set_volume(-5 * 256, stream=10)
    assert d.image_count() == 3
    before = [d.collect_bulk(s) for s in range(300)]
    d.pause_streams(200, 100)
    assert d.L.dspi_resize_streams(d.h, 200, host.RESIZE_PAUSED) == 200, "DSPI_RESIZE_PAUSED on a shrink has no meaning and is accepted"
    d.n_streams = 200
    assert num_streams(d) == 200 and not d.streams_paused().any() and len(d.streams_paused()) == 200
    assert d.image_count() == 2, "an object held only by cut slots is gone"
    assert d.stream_capacity() == rows_of(300, R) * R, "shrinking keeps the capacity"
    with pytest.raises(DspiError): d.collect_bulk(200)
    assert d.reserve_streams(200) == rows_of(200, R) * R == d.stream_capacity(), "reserve returns the memory"
    assert d.reserve_streams(200) == rows_of(200, R) * R
    # a grow afterwards gives power-on parameters again, not the cut occupants'
    fresh = power_on_bulk(flavor)
    assert d.resize_streams(260) == 260 and d.stream_capacity() == rows_of(260, R) * R
    for s in range(260): assert d.collect_bulk(s) == (before[s] if s < 200 else fresh), s
    assert d.image_count() == 3
    # down to one stream, and up again
    d.pause_streams(1, 259)
    assert d.resize_streams(1) == 1 and d.image_count() == 1 and d.collect_bulk(0) == before[0]
    assert d.reserve_streams(1) == R
    assert d.resize_streams(70, paused=True) == 70 and d.streams_paused().tolist() == [0] + [1] * 69 and d.collect_bulk(69) == fresh
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_reserve(flavor):
    d = loaded(flavor, 70)
    R = d.tile_streams()
    u = rows_of(70, R) * R
    assert d.reserve_streams(3 * R) == 3 * R == d.stream_capacity() and num_streams(d) == 70
    assert d.reserve_streams(2 * R + 1) == 3 * R
    for n in sorted(n for n in {100, R + 2, 2 * R + 1, 3 * R} if n > 70):
        assert d.resize_streams(n) == n and d.stream_capacity() == 3 * R, "inside the capacity a grow changes no allocation"
    assert d.resize_streams(3 * R + 1) == 3 * R + 1 and d.stream_capacity() == 4 * R
    d.pause_streams(70, 3 * R + 1 - 70)
    assert d.resize_streams(70) == 70 and d.stream_capacity() == 4 * R
    assert d.reserve_streams(70) == u == d.stream_capacity()
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_spdif_positions(flavor):
    d = loaded(flavor, 70)
    assert d.spdif_block_pos(17) == 17
    # mode off: nothing per stream exists, the context's value is untouched
    assert d.resize_streams(75) == 75 and d.spdif_block_pos() == 17
    d.pause_streams(70, 5)
    assert d.resize_streams(70) == 70 and d.spdif_block_pos() == 17
    assert d.spdif_per_stream(1)
    pos = (np.arange(70, dtype=np.uint32) * 7 + 3) % 192
    d.spdif_stream_pos(0, 70, set=pos)
    d.pause_streams(10, 6)
    assert d.resize_streams(100) == 100
    assert np.array_equal(d.spdif_stream_pos(), np.concatenate([pos, np.zeros(30, dtype=np.uint32)])), "old slots keep theirs, new slots read 0"
    d.spdif_stream_pos(90, 10, set=np.full(10, 55, dtype=np.uint32))
    d.pause_streams(80, 20)
    assert d.resize_streams(80) == 80 and np.array_equal(d.spdif_stream_pos(), np.concatenate([pos, np.zeros(10, dtype=np.uint32)]))
    assert d.resize_streams(2 * 128 + 1, paused=True) == 257
    assert np.array_equal(d.spdif_stream_pos(), np.concatenate([pos, np.zeros(257 - 70, dtype=np.uint32)])), "... also after a shrink and a grow"
    assert d.spdif_block_pos() == 17
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_refusals(flavor):
    S = 300
    d = loaded(flavor, S)
    assert d.load_bulk(WL.full_chain_blob(flavor, max_delay_ms=3.0), stream=S - 1) == 0
    d.pause_streams(250, 50)
    d.reserve_streams(400)

    def facts():
        return (num_streams(d), d.streams_paused().tolist(), d.stream_capacity(), d.image_count(), d.collect_bulk(0), d.collect_bulk(S - 1))
    was = facts()
    L, h = d.L, d.h
    assert L.dspi_resize_streams(h, 0, 0) == host.E_INVAL
    assert L.dspi_resize_streams(h, 0, host.RESIZE_PAUSED) == host.E_INVAL
    assert L.dspi_resize_streams(h, 200, 0) == host.E_INVAL, "slots 200 .. 249 are active"
    assert L.dspi_resize_streams(h, 249, 0) == host.E_INVAL, "slot 249 is active"
    for flags in (0x2, 0x3, 0x100, 0x80000000):
        assert L.dspi_resize_streams(h, 350, flags) == host.E_INVAL and L.dspi_resize_streams(h, 260, flags) == host.E_INVAL and L.dspi_resize_streams(h, S, flags) == host.E_INVAL, hex(flags)
    assert L.dspi_resize_streams(h, 0xFFFFFFFF, 0) == host.E_INVAL, "no stream index could name the slots"
    assert L.dspi_reserve_streams(h, 0) == host.E_INVAL and L.dspi_reserve_streams(h, S - 1) == host.E_INVAL and L.dspi_reserve_streams(h, 0xFFFFFFFF) == host.E_INVAL
    with pytest.raises(DspiError) as e: d.resize_streams(10)
    assert e.value.code == host.E_INVAL and d.n_streams == S
    assert L.dspi_resize_streams(None, 10, 0) == host.E_INVAL and L.dspi_reserve_streams(None, 10) == host.E_INVAL and L.dspi_stream_capacity(None) == 0
    assert facts() == was, "a refused call leaves the context as it was"
    assert d.resize_streams(250) == 250      # (and the same books accept what is legal)
    d.close()
