"""dspi_process_devices / dspi_wire_encode_tiled without a GPU: the tiled wire layout of dspi_amd/csrc/dspi_wire.h through a g++ driver
(tests/wire_tiled_driver.cpp) — the region, column and tail arithmetic against a plain numpy re-lay of the stream-major wire layout, the flag
rules —; the calls' refusals, in their order, through the real library on host-only contexts; plan_call's new input (CallInput::wire_tiled)
through tests/wire_tiled_plan_driver.cpp, held to the checks of tests/test_launch_plan_cpu.py; the symbols and the header's new section."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from dspi_amd import host, wire as W
from dspi_amd.host import Dspi
import test_launch_plan_cpu as LP
from test_wire_cpu import build, ask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
MEM_DEVICE, OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20      # include/dspi.h
DEVICES_OK = [a | b | c | d for a in (0, MEM_DEVICE) for b in (0, OUT_TILED) for c in (0, OUT_ENABLED_ONLY) for d in (0, OUT_CLIP_FLAGS)]
DEVICES_REFUSED = [OUT_SPDIF, OUT_I2S_SLOTS, OUT_SPDIF | OUT_TILED, OUT_SPDIF | OUT_I2S_SLOTS, OUT_SPDIF | MEM_DEVICE, OUT_I2S_SLOTS | OUT_TILED, OUT_I2S_SLOTS | OUT_CLIP_FLAGS,
                   0x3F, 0x40, 0x42, 0x100, 0x80000000, 0x80000002]
ENCODE_REFUSED = [OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS, MEM_DEVICE | OUT_TILED, 0x40, 0x80000000]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wiretiled"), "wire_tiled_driver", [os.path.join(ROOT, "tests", "wire_tiled_driver.cpp")])


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wiretiledplan"), "wire_tiled_plan_driver", [os.path.join(ROOT, "tests", "wire_tiled_plan_driver.cpp"), os.path.join(CSRC, "dspi_plan.cpp")])


@pytest.fixture(scope="module")
def old_plan_driver(tmp_path_factory):
    """tests/launch_plan_driver.cpp, which knows nothing of the new member"""
    return build(tmp_path_factory.mktemp("oldplan"), "launch_plan_driver", [os.path.join(ROOT, "tests", "launch_plan_driver.cpp"), os.path.join(CSRC, "dspi_plan.cpp")])


# ---- 5. the symbols and the header ---------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_process_devices", "dspi_wire_encode_tiled", "dspi_process_wire", "dspi_wire_encode", "dspi_process_mixed"): assert hasattr(L, name), name
    for name in ("process_devices_host", "process_devices_device", "wire_encode_tiled_host", "wire_encode_tiled_device", "untile_wire"): assert hasattr(Dspi, name), name
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "8 + wire words on tiled and mixed-depth contexts: detect by symbol (dspi_process_devices; with it dspi_wire_encode_tiled; additions only)",
                 "int dspi_process_devices(dspi_ctx *ctx, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,",
                 "int dspi_wire_encode_tiled(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos,",
                 "THE TILED WIRE LAYOUT has the size and the regions of dspi_spdif_encode_v's tiled subframes",
                 "word offset ((t * P + p) * F) * 4 * R", "word (f * 4 + j) * R + c", "(side * F + f) * R + c",
                 "the call IS dspi_process_wire at that depth", "the call IS dspi_process_mixed with DSPI_OUT_SPDIF",
                 "A tiled call ALWAYS runs in two passes",
                 # what the earlier section says stays, and stays true of its two calls
                 "A tiled wire layout is left out: both calls refuse DSPI_OUT_TILED.", "Not combined with dspi_process_mixed.",
                 "8 + wire words per device: detect by symbol (dspi_process_wire; with it dspi_wire_encode; additions only)"):
        assert word in text, word


# ---- 2. the flag rules ---------------------------------------------------------------------------------------------------------------------
def test_flag_rules(driver):
    words = list(range(128)) + [0x100, 0x8000, 0x80000000, 0x80000001, 0x80000002, 0xFFFFFFFF] + [1 << b for b in range(7, 32)]
    got = ask(driver, [f"flags devices {w}" for w in words] + [f"flags encode {w}" for w in words])
    assert [int(g) for g in got[:len(words)]] == [int(w in DEVICES_OK) for w in words]
    assert [int(g) for g in got[len(words):]] == [int(w in (0, MEM_DEVICE)) for w in words]
    assert not set(DEVICES_REFUSED) & set(DEVICES_OK) and len(set(DEVICES_OK)) == 16


# ---- 1. the region arithmetic --------------------------------------------------------------------------------------------------------------
def relay(sm, types, R):
    """the stream-major wire layout [S][P][F][4] re-laid into the tiled one [tiles][P][4 F rows][R], plainly: per stream and pair, by type"""
    S, P, F, _ = sm.shape
    nt = -(-S // R)
    t = np.full((nt, P, 4 * F, R), -1, dtype=np.int64)
    for s in range(S):
        for p in range(P):
            flat = sm[s, p].reshape(-1)
            if types[s, p]:
                t[s // R, p, :F, s % R] = flat[0:2 * F:2]            # L words: the first plane
                t[s // R, p, F:2 * F, s % R] = flat[1:2 * F:2]       # R words: the second
            else:
                t[s // R, p, :, s % R] = flat
    return t


@pytest.mark.parametrize("P", (2, 4))
@pytest.mark.parametrize("R", (64, 128))
@pytest.mark.parametrize("F", (1, 45, 144))
def test_regions_against_a_relay(driver, F, R, P):
    """every word the driver's formulas name holds, in the re-laid array, the stream-major word it stands for; what they never name is the tail
    of an I2S column and the columns past the last stream"""
    S = R + 22
    rng = np.random.default_rng(F * 1000 + R + P)
    types = rng.random((S, P)) < 0.5
    sm = np.arange(S * P * F * 4, dtype=np.int64).reshape(S, P, F, 4)          # every word its own stream-major index
    tiled = relay(sm, types, R).reshape(-1)
    asks, want = [], []
    for s in sorted(set([0, 1, R - 1, R, S - 1] + rng.integers(0, S, 12).tolist())):
        for p in range(P):
            for f in sorted(set([0, F - 1, F // 2] + rng.integers(0, F, 3).tolist())):
                if types[s, p]:
                    for side in (0, 1):
                        asks.append(f"i2s {s // R} {p} {P} {F} {R} {s % R} {side} {f}"); want.append(int(sm[s, p].reshape(-1)[2 * f + side]))
                else:
                    for j in range(4):
                        asks.append(f"spdif {s // R} {p} {P} {F} {R} {s % R} {f} {j}"); want.append(int(sm[s, p, f, j]))
    got = [int(g) for g in ask(driver, asks)]
    assert [int(tiled[g]) for g in got] == want
    # the columns: first word, written rows, the tail's extent; every named word of a column lies in it, and the tail holds no word
    named = np.zeros(tiled.size, dtype=bool)
    cols = ask(driver, [f"column {s} {p} {P} {F} {R} {int(types[s, p])}" for s in range(S) for p in range(P)])
    k = 0
    for s in range(S):
        for p in range(P):
            first, written, tail_first, tail = map(int, cols[k].split()); k += 1
            i2s = bool(types[s, p])
            assert first == ((s // R * P + p) * F) * 4 * R + s % R and written == (2 * F if i2s else 4 * F)
            assert tail_first == first + written * R and tail == (2 * F if i2s else 0) and written + tail == 4 * F
            named[first + np.arange(written) * R] = True
            assert (tiled[tail_first + np.arange(tail) * R] == -1).all(), "a word in a tail"
    assert np.array_equal(named, tiled >= 0), "the columns' written words are exactly the words of the re-laid layout"
    shape = (-(-S // R), P, 4 * F, R)
    assert (tiled.reshape(shape)[-1, :, :, S % R:] == -1).all() and not named.reshape(shape)[-1, :, :, S % R:].any(), "columns past the last stream"
    # the regions tile the buffer in [tile][pair] order, 16 F R bytes each: the regions of dspi_spdif_encode_v's tiled subframes
    r = [list(map(int, g.split())) for g in ask(driver, [f"region {t} {p} {P} {F} {R}" for t in range(2) for p in range(P)])]
    assert r[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(r, r[1:])) and all(a[1] * 4 == 16 * F * R for a in r)


@pytest.mark.parametrize("P", (2, 4))
@pytest.mark.parametrize("R", (64, 128))
def test_regions_at_4_8_million_frames(driver, R, P):
    """the two formulas of the layout, in Python's integers: word offsets reach past 2^32 there"""
    F = 4800000
    cases = [(0, 0, 0), (0, P - 1, R - 1), (1, 0, 5), (3, P - 1, R - 1), (1000, 1, 63)]
    asks, want = [], []
    for t, p, c in cases:
        region = ((t * P + p) * F) * 4 * R
        for f in (0, 1, F // 2, F - 1):
            for j in range(4): asks.append(f"spdif {t} {p} {P} {F} {R} {c} {f} {j}"); want.append(region + (f * 4 + j) * R + c)
            for side in (0, 1): asks.append(f"i2s {t} {p} {P} {F} {R} {c} {side} {f}"); want.append(region + (side * F + f) * R + c)
        for i2s in (0, 1):
            asks.append(f"column {t * R + c} {p} {P} {F} {R} {i2s}")
            want.append((region + c, (2 if i2s else 4) * F, region + c + (2 if i2s else 4) * F * R, 2 * F if i2s else 0))
    got = ask(driver, asks)
    for a, g, w in zip(asks, got, want):
        assert (tuple(map(int, g.split())) if a.startswith("column") else int(g)) == w, a
    assert max(w if isinstance(w, int) else w[2] for w in want) > 2 ** 32
    # an I2S column's last slot word is the last row of the region's first half, its tail ends with the region
    t, p, c = 3, P - 1, R - 1
    first, written, tail_first, tail = map(int, ask(driver, [f"column {t * R + c} {p} {P} {F} {R} 1"])[0].split())
    last_word = int(ask(driver, [f"i2s {t} {p} {P} {F} {R} {c} 1 {F - 1}"])[0])
    assert last_word == first + (written - 1) * R == tail_first - R and tail_first + (tail - 1) * R == ((t * P + p + 1) * F) * 4 * R - 1


# ---- 3. the calls on host-only contexts ----------------------------------------------------------------------------------------------------
S, B = 70, 48


def _positions(d):
    return d.spdif_block_pos(), (d.spdif_stream_pos().tolist() if d.spdif_per_stream() else None)


@pytest.mark.parametrize("flavor", [0, 1], ids=("q28", "f32"))
@pytest.mark.parametrize("per_stream", [False, True])
def test_process_devices_refusals(flavor, per_stream):
    """a NULL ctx; then the flags, before anything else is looked at; then dspi_process_mixed's refusals in their order: pointers, a depth, the
    lengths, (float) the preamp of an active 16-bit stream, and last the host-only context's own"""
    d = Dspi(flavor, S, device=None)
    assert d.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 1 | (1 << 8), 1, 3) == b"\x00"      # stream 3, slot 1: I2S
    assert d.spdif_block_pos(77) == 77
    if per_stream:
        d.spdif_per_stream(1)
        d.spdif_stream_pos(set=(np.arange(S) * 5 + 1) % 192)
    before = _positions(d)
    R = d.tile_streams(); nt = -(-S // R)
    pcm = np.zeros(S * B * 6, dtype=np.uint8)
    pairs = np.full((nt, d.P, B, 4, R), 0x5A5A5A5A, dtype=np.uint32)
    words = np.full((nt, B, 8, R), 0x5A5A5A5A, dtype=np.uint32)
    out = host._Out(pairs.ctypes.data, None, None, None)
    u16, u24 = np.full(S, 16, dtype=np.uint8), np.full(S, 24, dtype=np.uint8)
    mixed = np.where(np.arange(S) % 2, 24, 16).astype(np.uint8)
    call = lambda flags, depths=mixed, pdm=None, nb=1, bl=B, pcm_p=pcm.ctypes.data, out_p=C.byref(out): \
        d.L.dspi_process_devices(d.h, pcm_p, depths.ctypes.data if depths is not None else None, nb, bl, out_p, pdm, flags)
    assert d.L.dspi_process_devices(None, pcm.ctypes.data, mixed.ctypes.data, 1, B, C.byref(out), None, 0) == host.E_INVAL
    bad = mixed.copy(); bad[S // 2] = 20
    for flags in DEVICES_REFUSED:
        for depths in (mixed, u16, bad, None):      # the flags come first: whatever else is wrong with the call
            assert call(flags, depths) == host.E_INVAL and "the flags are" in d.L.dspi_last_error(d.h).decode(), hex(flags)
        assert call(flags, pdm=words.ctypes.data) == host.E_INVAL and call(flags, nb=0) == host.E_INVAL and call(flags, pcm_p=None) == host.E_INVAL, hex(flags)
        assert _positions(d) == before, hex(flags)
    for flags in DEVICES_OK:
        # dspi_process_mixed's refusals, in its order
        assert call(flags, pcm_p=None) == host.E_INVAL and call(flags, None) == host.E_INVAL and call(flags, out_p=None) == host.E_INVAL
        assert call(flags, bad, nb=0) == host.E_INVAL and f"stream {S // 2}" in d.L.dspi_last_error(d.h).decode(), "a depth, before the lengths"
        for nb, bl in ((0, B), (1, 0), (1, 193)): assert call(flags, nb=nb, bl=bl) == host.E_INVAL
        # a legal call: the host-only context's refusal, whatever the depths
        for depths in (mixed, u16, u24):
            assert call(flags, depths) == host.E_NODEVICE, hex(flags)
            assert call(flags, depths, pdm=words.ctypes.data) == host.E_NODEVICE, hex(flags)
        assert _positions(d) == before, hex(flags)
    # the preamp refusal for an active 16-bit stream (float): behind the lengths, ahead of the host-only context's
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=8) >= 0 and mixed[8] == 16
    refused = host.E_UNSUPPORTED if flavor else host.E_NODEVICE
    for flags in (0, OUT_TILED, OUT_TILED | MEM_DEVICE):
        assert call(flags) == refused
        if flavor: assert "dspi_process_devices: stream 8" in d.L.dspi_last_error(d.h).decode()
        assert call(flags, nb=0) == host.E_INVAL and call(OUT_SPDIF | flags) == host.E_INVAL
        assert call(flags, u16) == host.E_NODEVICE, "uniform depths: the call is dspi_process_wire"
    d.pause_streams(8, 1)
    assert call(OUT_TILED) == host.E_NODEVICE
    assert _positions(d) == before
    assert (pairs == 0x5A5A5A5A).all() and (words == 0x5A5A5A5A).all(), "a refused call wrote something"
    d.close()


@pytest.mark.parametrize("flavor", [0, 1], ids=("q28", "f32"))
def test_wire_encode_tiled_refusals(flavor):
    d = Dspi(flavor, S, device=None)
    d.spdif_block_pos(33)
    d.spdif_per_stream(1)
    before = _positions(d)
    F = 45
    R = d.tile_streams(); nt = -(-S // R)
    pairs = np.zeros((nt, 2 * d.P, F, R), dtype=np.int32)
    pos = ((np.arange(S) * 7) % 192).astype(np.uint32)
    out = np.full((nt, d.P, F, 4, R), 0x5A5A5A5A, dtype=np.uint32)
    call = lambda flags, p=pos: d.L.dspi_wire_encode_tiled(d.h, pairs.ctypes.data, F, p.ctypes.data if p is not None else None, out.ctypes.data, flags)
    for flags in ENCODE_REFUSED: assert call(flags) == host.E_INVAL, hex(flags)
    assert call(0, None) == host.E_INVAL, "a NULL block_pos"
    assert call(MEM_DEVICE, None) == host.E_INVAL
    bad = pos.copy(); bad[S // 2] = 192
    assert call(0, bad) == host.E_INVAL, "a host position of 192"
    bad[S // 2] = 0xFFFFFFFF
    assert call(0, bad) == host.E_INVAL
    assert d.L.dspi_wire_encode_tiled(None, pairs.ctypes.data, F, pos.ctypes.data, out.ctypes.data, 0) == host.E_INVAL
    assert d.L.dspi_wire_encode_tiled(d.h, None, F, pos.ctypes.data, out.ctypes.data, 0) == host.E_INVAL
    assert d.L.dspi_wire_encode_tiled(d.h, pairs.ctypes.data, F, pos.ctypes.data, None, 0) == host.E_INVAL
    assert d.L.dspi_wire_encode_tiled(d.h, pairs.ctypes.data, 0, pos.ctypes.data, out.ctypes.data, 0) == host.E_INVAL
    assert call(0) == host.E_NODEVICE, "a legal call on a host-only context"
    pos[0] = 191
    assert call(0) == host.E_NODEVICE
    assert _positions(d) == before and (out == 0x5A5A5A5A).all()
    d.close()


def test_untile_wire():
    """the mapping of host.py untile_wire is the inverse of the re-lay above"""
    d = Dspi(0, 100, device=None)
    S, P, F, R = 100, d.P, 45, d.tile_streams()
    types = np.random.default_rng(3).random((S, P)) < 0.5
    sm = (np.arange(S * P * F * 4, dtype=np.int64) + 1).reshape(S, P, F, 4)
    t = relay(sm, types, R)
    t[t < 0] = 0
    back = d.untile_wire(t.astype(np.uint32).reshape(-(-S // R), P, F, 4, R), types)
    want = sm.copy()
    for s, p in np.argwhere(types): want[s, p].reshape(-1)[2 * F:] = 0
    assert np.array_equal(back, want)
    d.close()


# ---- 4. plan_call --------------------------------------------------------------------------------------------------------------------------
def _render(c, wire_slots=False, wire_tiled=False):
    return LP.render_call(c).rstrip("\n") + f" {int(wire_slots)} {int(wire_tiled)}\n"


def test_plan_call_member(plan_driver, old_plan_driver):
    """wire_tiled false: the layout is what tests/launch_plan_driver.cpp, which does not know the member, prints for every call of
    tests/test_launch_plan_cpu.py's generator, and passes its checks.  true: `pairs` is tile-column sized at n_pairs * F * 16 per column,
    spdif_two_pass, wire_encoder and wire_tiled are set whenever pairs are passed, whatever all_latency is, the scratch is the one the
    stream-major two-pass call gets, and nothing else moves: every other buffer is the tiled call's, the direct area, the memory path and
    the chunks follow their rules from the new size"""
    calls = [LP.call(seed) for seed in range(LP.N_CALLS)]
    run = lambda exe, text: subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    keep = MEM_DEVICE | OUT_ENABLED_ONLY | OUT_CLIP_FLAGS
    tiled_calls = [dict(c, flags=(c["flags"] & keep) | OUT_TILED) for c in calls]
    off = run(plan_driver, "".join(_render(c) for c in calls))
    old = run(old_plan_driver, "".join(LP.render_call(c) for c in calls))
    on = run(plan_driver, "".join(_render(dict(c, flags=c["flags"] | OUT_SPDIF), wire_tiled=True) for c in tiled_calls))
    plain = run(plan_driver, "".join(_render(c) for c in tiled_calls))
    stream_major = run(plan_driver, "".join(_render(dict(c, flags=(c["flags"] & keep) | OUT_SPDIF, all_latency=False)) for c in calls))
    assert len(off) == len(old) == len(on) == len(plain) == len(stream_major) == len(calls)
    seen = set()
    for c, ct, a, o, b, pl, sm in zip(calls, tiled_calls, off, old, on, plain, stream_major):
        assert a == o + " 0 0", "with the member off plan_call prints what it printed"
        LP.check_call(c, LP.parse_call(a.rsplit(" ", 2)[0]))
        lay, lay_t, lay_s = (LP.parse_call(x.rsplit(" ", 2)[0]) for x in (b, pl, sm))
        st = LP.STATE_MAP[c["flavor"]]
        R, P, F, n_wg = st["R"], st["P"], c["n_blocks"] * c["block_len"], -(-c["n"] // st["R"])
        passed = c["passed"]["pairs"]
        assert lay["pairs"]["bytes"] == (n_wg * R * P * F * 16 if passed else 0) and lay["pairs"]["per"] == P * F * 16 and lay["pairs"]["tile_cols"] == 1
        assert lay["pairs"]["per"] == 2 * lay_t["pairs"]["per"], "a column's regions are twice its tiled pair words"
        assert b.rsplit(" ", 2)[1:] == ([str(int(passed))] * 2) and bool(lay["two_pass"]) == passed, "two passes and the tiled wire encoder whenever pairs are passed"
        if passed and c["all_latency"]: seen.add("all_latency")
        if passed: seen.add(("flavour", c["flavor"]))
        for k in ("two_pass", "two_pass_rows", "two_pass_bytes"): assert lay[k] == lay_s[k], f"{k}: the scratch is sized as today"
        if passed: assert lay["two_pass_bytes"] == lay["two_pass_rows"] * R * P * F * 8 and 1 <= lay["two_pass_rows"] <= n_wg
        assert lay["frames"] == lay_t["frames"]
        for nm in ("pcm", "sub", "peaks", "clip"):
            for k in ("bytes", "per", "tile_cols"): assert lay[nm][k] == lay_t[nm][k], (nm, k)
        # the direct area, the memory path and the chunks: the rules of check_call, from the new size
        offs = [lay[nm]["off"] for nm in LP.BUFFERS]
        assert offs[0] == 0 and all(x % 256 == 0 for x in offs + [lay["direct_bytes"]])
        for k, nm in enumerate(LP.BUFFERS):
            end = offs[k + 1] if k + 1 < len(LP.BUFFERS) else lay["direct_bytes"]
            assert offs[k] + lay[nm]["bytes"] <= end < offs[k] + lay[nm]["bytes"] + 256, nm
        if ct["flags"] & MEM_DEVICE: assert lay["mem"] == LP.DEVICE
        else: assert lay["mem"] == (LP.DIRECT if not c["no_direct"] and lay["direct_bytes"] <= 2 * LP.MIB else LP.STAGED)
        moved = sum(lay[nm]["bytes"] for nm in ("pcm", "pairs", "sub", "peaks"))
        assert 1 <= lay["n_chunks"] <= 8 and (lay["n_chunks"] > 1) == (moved >= 32 * LP.MIB and n_wg >= 2)
        assert (lay["n_chunks"] - 1) * lay["rows_per_chunk"] < n_wg <= lay["n_chunks"] * lay["rows_per_chunk"]
        seen.add(("mem", lay["mem"])); seen.add(("chunks", min(lay["n_chunks"], 2)))
    assert seen >= {"all_latency", ("flavour", 0), ("flavour", 1), ("mem", LP.DEVICE), ("mem", LP.DIRECT), ("mem", LP.STAGED), ("chunks", 1), ("chunks", 2)}
