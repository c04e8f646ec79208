"""dspi_process_wire / dspi_wire_encode without a GPU: the layout module (dspi_amd/csrc/dspi_wire.{h,cpp}) through a g++ driver
(tests/wire_driver.cpp) — the flag rule, the region and tail arithmetic, the scan that decides between the two routes —; the calls' refusals
through the real library on host-only contexts; and plan_call's new input (CallInput::wire_slots) through tests/wire_plan_driver.cpp, held to
the checks of tests/test_launch_plan_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dspi_amd import host, wire as W
from dspi_amd.host import Dspi
import test_launch_plan_cpu as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
MEM_DEVICE, OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20      # include/dspi.h
PROCESS_OK = [a | b | c for a in (0, MEM_DEVICE) for b in (0, OUT_ENABLED_ONLY) for c in (0, OUT_CLIP_FLAGS)]
PROCESS_REFUSED = [OUT_SPDIF, OUT_I2S_SLOTS, OUT_TILED, OUT_SPDIF | OUT_I2S_SLOTS, OUT_SPDIF | MEM_DEVICE, OUT_TILED | OUT_ENABLED_ONLY, OUT_I2S_SLOTS | OUT_CLIP_FLAGS,
                   0x3F, 0x40, 0x100, 0x80000000, 0x80000001]
ENCODE_REFUSED = [OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS, MEM_DEVICE | OUT_TILED, 0x40, 0x80000000]


def build(tmp, name, sources):
    """a driver with its own main: under AddressSanitizer and UBSan where this g++ has their runtimes, else plain"""
    exe = tmp / name
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe)] + sources
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True).returncode != 0: subprocess.run(cmd, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wire"), "wire_driver", [os.path.join(ROOT, "tests", "wire_driver.cpp"), os.path.join(CSRC, "dspi_wire.cpp")])


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wireplan"), "wire_plan_driver", [os.path.join(ROOT, "tests", "wire_plan_driver.cpp"), os.path.join(CSRC, "dspi_plan.cpp")])


def ask(driver, lines):
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines), (lines, out)
    return out


# ---- the symbols and the header -----------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_process_wire", "dspi_wire_encode"): assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "8 + wire words per device: detect by symbol (dspi_process_wire; with it dspi_wire_encode; additions only)",
                 "int dspi_process_wire(dspi_ctx *ctx, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len,",
                 "int dspi_wire_encode(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos,",
                 "A tiled wire layout is left out"):
        assert word in text, word


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
def test_flag_rule(driver):
    words = list(range(128)) + [0x100, 0x8000, 0x80000000, 0x80000001, 0xFFFFFFFF]
    got = ask(driver, [f"flags process {w}" for w in words] + [f"flags encode {w}" for w in words])
    assert [int(g) for g in got[:len(words)]] == [int(w in PROCESS_OK) for w in words]
    assert [int(g) for g in got[len(words):]] == [int(w in (0, MEM_DEVICE)) for w in words]
    assert not set(PROCESS_REFUSED) & set(PROCESS_OK) and len(PROCESS_OK) == 8


@pytest.mark.parametrize("F", (1, 45, 144, 191, 1920, 4800000))
def test_regions(driver, F):
    """odd and even frame counts: the regions are DSPI_OUT_SPDIF's (16 F bytes each, back to back in [stream][pair] order); an I2S slot's words
    are the first 8 F bytes and its tail the rest, an S/PDIF slot's words the whole region; the last one at a 4.8M-frame call lies past 2^32"""
    P, cases = 4, [(0, 0), (0, 3), (1, 0), (149, 2), (70000, 3)]
    got = ask(driver, [f"region {s} {p} {P} {F} {i}" for s, p in cases for i in (0, 1)])
    k = 0
    for s, p in cases:
        for i2s in (0, 1):
            off, written, t0, t1 = map(int, got[k].split()); k += 1
            assert off == ((s * P + p) * F) * 4 * 4, "word offset ((s * P + p) * F) * 4"
            assert written == (8 * F if i2s else 16 * F) and t0 == off + written and t1 == off + 16 * F
            assert (t1 - t0) == (8 * F if i2s else 0)
            assert off % 16 == 0 and t0 % 8 == 0 and (F % 2 or t0 % 16 == 0), "the stores' alignment: 16 bytes per lane on even F, 8 on odd F"
    if F == 4800000: assert int(got[-1].split()[0]) > 2 ** 32
    # two pairs (NP = 2, the Q28 flavour): consecutive regions tile the buffer
    r = [list(map(int, g.split())) for g in ask(driver, [f"region {s} {p} 2 {F} 1" for s in range(3) for p in range(2)])]
    assert r[0][0] == 0 and all(a[3] == b[0] for a, b in zip(r, r[1:]))


def test_type_masks(driver):
    assert ask(driver, ["mask 0 0 0 0", "mask 1 1 1 1", "mask 1 0 0 0", "mask 0 0 0 1", "mask 1 0 1 0", "mask 0 1", "mask 2 0 1 0"]) == ["0", "15", "1", "8", "5", "2", "4"]


def test_route_decision(driver):
    S = 6
    none, img = "0 0 0", "0 1 2 0 1 2"
    got = ask(driver, [
        f"scan {S} - | {img} | {none}",                          # no I2S anywhere, nobody paused
        f"scan {S} 1 1 0 1 1 1 | {img} | {none}",                # ... with a paused stream
        f"scan {S} 1 1 0 1 1 0 | {img} | 0 0 5",                 # I2S only on paused streams (object 2: streams 2 and 5): the S/PDIF route
        f"scan {S} 1 1 0 1 1 1 | {img} | 0 0 5",                 # ... one of them active: the wire route
        f"scan {S} - | 0 0 0 1 0 0 | 0 1 0",                     # one active stream with one I2S slot
        f"scan {S} - | 0 0 0 0 0 0 | 0 15 15",                   # objects that no stream uses do not count
        f"scan {S} 0 0 0 0 0 0 | {img} | 15 15 15",              # every stream paused
        f"scan 1 - | 0 | 8", "scan 1 0 | 0 | 8"])
    assert got == ["0", "0", "0", "1", "1", "0", "0", "1", "0"]


# ---- the calls on host-only contexts ------------------------------------------------------------------------------------------------------
S, B = 70, 48


def _positions(d):
    return d.spdif_block_pos(), (d.spdif_stream_pos().tolist() if d.spdif_per_stream() else None)


@pytest.mark.parametrize("flavor", [0, 1])
@pytest.mark.parametrize("per_stream", [False, True])
def test_process_wire_refusals(flavor, per_stream):
    d = Dspi(flavor, S, device=None)
    assert d.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 1 | (1 << 8), 1, 3) == b"\x00"      # stream 3, slot 1: I2S
    assert d.spdif_block_pos(77) == 77
    if per_stream:
        d.spdif_per_stream(1)
        d.spdif_stream_pos(set=(np.arange(S) * 5 + 1) % 192)
    before = _positions(d)
    pcm = np.zeros((S, B, 2), dtype=np.int16)
    pairs = np.full((S, d.P, B, 4), 0x5A5A5A5A, dtype=np.uint32)
    words = np.full((S, B, 8), 0x5A5A5A5A, dtype=np.uint32)
    out = host._Out(pairs.ctypes.data, None, None, None)
    call = lambda flags, pdm=None, depth=16: d.L.dspi_process_wire(d.h, pcm.ctypes.data, depth, 1, B, C.byref(out), pdm, flags)
    for flags in PROCESS_REFUSED:
        assert call(flags) == host.E_INVAL, hex(flags)
        assert call(flags, words.ctypes.data) == host.E_INVAL, hex(flags)
        assert _positions(d) == before, hex(flags)
    # the flags come first: a refused flag with a bad depth or NULL pointers is still DSPI_E_INVAL, and a legal call is DSPI_E_NODEVICE here
    assert call(OUT_SPDIF, depth=20) == host.E_INVAL
    assert d.L.dspi_process_wire(d.h, None, 16, 1, B, C.byref(out), None, 0) == host.E_INVAL
    assert d.L.dspi_process_wire(d.h, pcm.ctypes.data, 16, 1, B, None, None, 0) == host.E_INVAL
    assert d.L.dspi_process_wire(None, pcm.ctypes.data, 16, 1, B, C.byref(out), None, 0) == host.E_INVAL
    for flags in PROCESS_OK:
        assert call(flags) == host.E_NODEVICE, hex(flags)
        assert call(flags, words.ctypes.data) == host.E_NODEVICE, hex(flags)
        assert _positions(d) == before, hex(flags)
    assert (pairs == 0x5A5A5A5A).all() and (words == 0x5A5A5A5A).all(), "a refused call wrote something"
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_wire_encode_refusals(flavor):
    d = Dspi(flavor, S, device=None)
    d.spdif_block_pos(33)
    d.spdif_per_stream(1)
    before = _positions(d)
    F = 45
    pairs = np.zeros((S, d.P, F, 2), dtype=np.int32)
    pos = ((np.arange(S) * 7) % 192).astype(np.uint32)
    out = np.full((S, d.P, F, 4), 0x5A5A5A5A, dtype=np.uint32)
    call = lambda flags, p=pos: d.L.dspi_wire_encode(d.h, pairs.ctypes.data, F, p.ctypes.data if p is not None else None, out.ctypes.data, flags)
    for flags in ENCODE_REFUSED: assert call(flags) == host.E_INVAL, hex(flags)
    assert call(0, None) == host.E_INVAL, "a NULL block_pos"
    assert call(MEM_DEVICE, None) == host.E_INVAL
    bad = pos.copy(); bad[S // 2] = 192
    assert call(0, bad) == host.E_INVAL, "a host position of 192"
    bad[S // 2] = 0xFFFFFFFF
    assert call(0, bad) == host.E_INVAL
    assert d.L.dspi_wire_encode(d.h, None, F, pos.ctypes.data, out.ctypes.data, 0) == host.E_INVAL
    assert d.L.dspi_wire_encode(d.h, pairs.ctypes.data, F, pos.ctypes.data, None, 0) == host.E_INVAL
    assert d.L.dspi_wire_encode(d.h, pairs.ctypes.data, 0, pos.ctypes.data, out.ctypes.data, 0) == host.E_INVAL
    assert call(0) == host.E_NODEVICE, "a legal call on a host-only context"
    pos[0] = 191
    assert call(0) == host.E_NODEVICE
    assert _positions(d) == before and (out == 0x5A5A5A5A).all()
    d.close()


# ---- plan_call ----------------------------------------------------------------------------------------------------------------------------
def _render(c, wire_slots):
    return LP.render_call(c).rstrip("\n") + f" {int(wire_slots)}\n"


def test_plan_call_member(plan_driver):
    """wire_slots false: the layout passes every check tests/test_launch_plan_cpu.py makes of today's, over its calls (every flag set
    dspi_process accepts); true: spdif_two_pass no longer depends on all_latency, its scratch is the one a launch off the latency layout gets,
    and nothing else of the layout moves"""
    calls = [LP.call(seed) for seed in range(LP.N_CALLS)]
    assert {c["flags"] for c in calls} == set(LP.ACCEPTED_FLAGS)
    run = lambda text: subprocess.run([plan_driver], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    off, on = run("".join(_render(c, False) for c in calls)), run("".join(_render(c, True) for c in calls))
    not_latency = run("".join(_render(dict(c, all_latency=False), False) for c in calls))
    assert len(off) == len(on) == len(not_latency) == len(calls)
    seen = set()
    for c, a, b, n in zip(calls, off, on, not_latency):
        assert a.endswith(" 0"), "wire_encoder without wire_slots"
        lay_off, lay_on = LP.parse_call(a.rsplit(" ", 1)[0]), LP.parse_call(b.rsplit(" ", 1)[0])
        LP.check_call(c, lay_off)
        spdif_pairs = bool(c["flags"] & OUT_SPDIF) and c["passed"]["pairs"]
        assert bool(lay_on["two_pass"]) == spdif_pairs and b.endswith(" 1" if spdif_pairs else " 0")
        if spdif_pairs and c["all_latency"]: assert lay_on["two_pass"] and not lay_off["two_pass"]; seen.add("forced")
        assert b.rsplit(" ", 1)[0] == n.rsplit(" ", 1)[0], "with wire_slots the layout is that of the same call off the latency layout"
        for k in lay_off:
            if not k.startswith("two_pass"): assert lay_off[k] == lay_on[k], k
    assert "forced" in seen
