"""Per-stream S/PDIF block positions without a GPU: the bookkeeping module (dspi_amd/csrc/dspi_spdifpos.{h,cpp}) through a g++ driver
(tests/spdifpos_driver.cpp) against a model that keeps one absolute position per stream and adds the frames to every active one — the naive
form of the contract in include/dspi.h —, and dspi_spdif_per_stream / dspi_spdif_stream_pos on host-only contexts, where they are
bookkeeping."""
import os
import subprocess

import numpy as np
import pytest

from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    for name in ("dspi_spdif_per_stream", "dspi_spdif_stream_pos", "dspi_spdif_encode_v"): assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("#define DSPI_ABI_VERSION 8 ",
                 "8 + per-stream S/PDIF positions: detect by symbol (dspi_spdif_per_stream; with it dspi_spdif_stream_pos, dspi_spdif_encode_v; additions only)",
                 "int dspi_spdif_per_stream(dspi_ctx *ctx, int enable);",
                 "int dspi_spdif_stream_pos(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get);",
                 "int dspi_spdif_encode_v(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos, uint32_t *subframes, uint32_t flags);",
                 "dspi_spdif_stream_pos, get on the source context, set on the destination"):
        assert word in text, word
    assert "and per-stream S/PDIF block positions" not in text      # (the boots' "not in scope" line is corrected)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes, else plain"""
    exe = tmp_path_factory.mktemp("spdifpos") / "spdifpos_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "spdifpos_driver.cpp"),
           os.path.join(CSRC, "dspi_spdifpos.cpp"), os.path.join(CSRC, "dspi_move.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0: subprocess.run(cmd, check=True)
    return str(exe)


class Model:
    """one absolute position per stream; a flagged call adds its frames to every active stream"""

    def __init__(self, n):
        self.n, self.on, self.pos, self.active = n, False, None, [True] * n

    def run(self, script):
        out = []
        for line in script:
            cmd, *a = line.split(); a = list(map(int, a))
            if cmd == "enable":
                if not self.on: self.on, self.pos = True, [a[0]] * self.n
            elif cmd == "disable": self.on, self.pos = False, None
            elif cmd == "advance":
                if self.on: self.pos = [(p + a[0]) % 192 if act else p for p, act in zip(self.pos, self.active)]
            elif cmd in ("pause", "resume"):
                for s in range(a[0], a[0] + a[1]): self.active[s] = cmd == "resume"
            elif cmd == "move":
                mv = list(zip(a[0::2], a[1::2]))
                old_p, old_a = list(self.pos), list(self.active)
                dsts = {d for _, d in mv}
                for s, d in mv: self.pos[d], self.active[d] = old_p[s], old_a[s]
                for s, _ in mv:
                    if s not in dsts: self.active[s] = False      # (the open end keeps its value, frozen)
            elif cmd == "boot":
                for s in a: self.pos[s] = 0
            elif cmd == "set": self.pos[a[0]] = a[1]
            elif cmd == "get": out.append("on " + " ".join(map(str, self.pos)) if self.on else "off")
        return out


def play(driver, n, script):
    """the driver's answers to the script's `get` lines, which must be the model's"""
    text = f"new {n}\n" + "".join(l + "\n" for l in script)
    got = subprocess.run([driver], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    want = Model(n).run(script)
    assert len(got) == len(want) == sum(1 for l in script if l == "get")
    for k, (g, w) in enumerate(zip(got, want)): assert g == w, (k, g, w)
    return [list(map(int, g.split()[1:])) for g in got]


def test_enable_copies_the_context_value(driver):
    got = play(driver, 5, ["get", "enable 77", "get", "advance 48", "enable 3", "get", "disable", "get", "enable 3", "get"])
    assert got == [[], [77] * 5, [125] * 5, [], [3] * 5]      # a second enable changes nothing; a disable drops the positions


def test_advance_with_a_paused_set(driver):
    got = play(driver, 8, ["enable 10", "pause 2 3", "pause 7 1", "advance 48", "get", "advance 45", "get"])
    assert got[0] == [58, 58, 10, 10, 10, 58, 58, 10] and got[1] == [103, 103, 10, 10, 10, 103, 103, 10]


def test_pause_calls_resume_gives_the_frozen_value(driver):
    script = ["enable 0", "advance 100", "pause 1 2", "get"] + ["advance 48"] * 7 + ["get", "resume 0 4", "get", "advance 48", "get",
              "pause 1 1", "pause 1 1", "resume 1 1", "resume 1 1", "get"]      # (pausing a paused stream and resuming an active one change nothing)
    got = play(driver, 4, script)
    assert got[0] == [100] * 4
    assert got[1] == got[2] == [(100 + 7 * 48) % 192, 100, 100, (100 + 7 * 48) % 192]
    assert got[3] == got[4] == [(100 + 8 * 48) % 192, 148, 148, (100 + 8 * 48) % 192]


def test_wrap_at_192(driver):
    got = play(driver, 3, ["enable 191", "get", "advance 1", "get", "set 1 191", "pause 2 1", "advance 191", "get", "advance 1", "get",
                           "advance 4294967295", "get"])
    assert got[:4] == [[191] * 3, [0] * 3, [191, 190, 0], [0, 191, 0]]
    assert got[4] == [4294967295 % 192, (191 + 4294967295) % 192, 0]


def test_moves_apply_at_once(driver):
    base = ["enable 0"] + [f"set {s} {10 * s + 1}" for s in range(8)]
    # a swap
    got = play(driver, 8, base + ["move 1 6 6 1", "get", "advance 48", "get"])
    assert got[0] == [1, 61, 21, 31, 41, 51, 11, 71] and got[1] == [p + 48 for p in got[0]]
    # a 3-cycle, one of its streams paused: the pause travels with the stream
    got = play(driver, 8, base + ["pause 2 1", "advance 5", "move 2 4 4 7 7 2", "get", "advance 48", "get"])
    assert got[0] == [6, 16, 76, 36, 21, 56, 66, 46]
    assert got[1] == [p + 48 if s != 4 else 21 for s, p in enumerate(got[0])]
    # a chain 0 -> 3 -> 5 with an open-end source (slot 0 keeps its value, frozen) into a paused slot (5, whose occupant is lost)
    got = play(driver, 8, base + ["pause 5 1", "advance 7", "move 3 5 0 3", "get", "advance 48", "get", "resume 0 1", "advance 1", "get"])
    assert got[0] == [8, 18, 28, 8, 48, 38, 68, 78]
    assert got[1] == [8] + [p + 48 for p in got[0][1:]]
    assert got[2] == [9] + [p + 49 for p in got[0][1:]]


def test_boot_to_zero(driver):
    got = play(driver, 6, ["enable 30", "pause 4 1", "advance 50", "boot 1 4", "get", "advance 48", "get", "resume 4 1", "advance 48", "get"])
    assert got == [[80, 0, 80, 80, 0, 80], [128, 48, 128, 128, 0, 128], [176, 96, 176, 176, 48, 176]]


def test_set_and_get(driver):
    got = play(driver, 4, ["enable 5", "advance 100", "pause 3 1", "advance 60", "set 0 0", "set 3 191", "get", "advance 1", "get", "resume 3 1", "advance 1", "get"])
    assert got == [[0, 165, 165, 191], [1, 166, 166, 191], [2, 167, 167, 0]]


def test_random_schedules(driver):
    """long random schedules of every command: the module against the model"""
    rng = np.random.default_rng(20)
    for n in (1, 2, 9, 70):
        script, active = ["enable %d" % rng.integers(0, 192)], np.ones(n, dtype=bool)
        for _ in range(300):
            k = int(rng.integers(0, 8))
            first = int(rng.integers(0, n)); count = int(rng.integers(1, n - first + 1))
            if k == 0: script.append(f"advance {int(rng.choice([1, 45, 48, 96, 144, 191, 192, 4800]))}")
            elif k == 1: script.append(f"pause {first} {count}"); active[first:first + count] = False
            elif k == 2: script.append(f"resume {first} {count}"); active[first:first + count] = True
            elif k == 3: script.append(f"set {first} {int(rng.integers(0, 192))}")
            elif k == 4: script.append("boot " + " ".join(map(str, rng.permutation(n)[:count])))
            elif k == 5 and n >= 2:      # a random permutation of some slots: cycles and swaps
                slots = rng.permutation(n)[:max(2, count)]
                script.append("move " + " ".join(f"{a} {b}" for a, b in zip(slots, np.roll(slots, -1))))
                active[np.roll(slots, -1)] = active[slots].copy()
            elif k == 6 and (~active).any() and active.any():      # a one-way move into a paused slot
                src, dst = int(rng.choice(np.flatnonzero(active))), int(rng.choice(np.flatnonzero(~active)))
                script.append(f"move {src} {dst}"); active[dst] = True; active[src] = False
            script.append("get")
        play(driver, n, script)


# ---- host-only contexts -------------------------------------------------------------------------------------------------------------------
S = 301


@pytest.mark.parametrize("flavor", [0, 1])
def test_mode_and_context_value(flavor):
    d = Dspi(flavor, S, device=None)
    assert d.spdif_per_stream() is False
    get = np.zeros(S, dtype=np.uint32)
    assert d.L.dspi_spdif_stream_pos(d.h, 0, S, None, get.ctypes.data) == host.E_INVAL, "mode off"
    assert d.spdif_block_pos(100) == 100
    assert d.spdif_per_stream(1) is True and d.spdif_per_stream() is True
    assert d.spdif_stream_pos().tolist() == [100] * S, "enable copies the context's value"
    assert d.spdif_block_pos() == 100
    # the context's own value keeps its meaning: set and read as before, and neither side sees the other
    assert d.spdif_block_pos(7) == 7 and d.spdif_stream_pos().tolist() == [100] * S
    assert d.spdif_stream_pos(3, 2, set=[191, 0]).tolist() == [191, 0] and d.spdif_block_pos() == 7
    assert d.spdif_per_stream(1) is True and d.spdif_stream_pos(2, 4).tolist() == [100, 191, 0, 100], "a second enable changes nothing"
    assert d.spdif_per_stream(0) is False and d.spdif_block_pos() == 7
    assert d.L.dspi_spdif_stream_pos(d.h, 0, S, None, get.ctypes.data) == host.E_INVAL
    assert d.spdif_per_stream(1) is True and d.spdif_stream_pos().tolist() == [7] * S, "the positions were dropped"
    assert d.L.dspi_spdif_per_stream(None, 1) == host.E_INVAL
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_validation(flavor):
    d = Dspi(flavor, S, device=None)
    d.spdif_per_stream(1)
    want = (np.arange(S) * 7 % 192).astype(np.uint32)
    assert np.array_equal(d.spdif_stream_pos(set=want), want)

    def call(first, values, count=None):
        v = np.asarray(values, dtype=np.uint32)
        return d.L.dspi_spdif_stream_pos(d.h, first, len(v) if count is None else count, v.ctypes.data, None)
    assert call(5, [1, 2, 192]) == host.E_INVAL, "a value of 192"
    assert call(5, [0xFFFFFFFF]) == host.E_INVAL
    assert call(S - 1, [1, 2]) == host.E_INVAL and call(S, [1]) == host.E_INVAL and call(0xFFFFFFFF, [1, 2]) == host.E_INVAL, "a range past the end"
    assert call(5, [1], count=0) == host.E_INVAL, "a count of 0"
    assert d.L.dspi_spdif_stream_pos(d.h, 0, 0, None, None) == host.E_INVAL
    with pytest.raises(DspiError) as e: d.spdif_stream_pos(0, 2, set=[5, 200])
    assert e.value.code == host.E_INVAL
    assert np.array_equal(d.spdif_stream_pos(), want), "a refused call changed a position"
    assert d.L.dspi_spdif_stream_pos(d.h, 0, S, None, None) == S      # (both pointers may be null)
    d.close()


@pytest.mark.parametrize("flavor", [0, 1])
def test_lifecycle_bookkeeping(flavor):
    """pauses, resumes and boots are bookkeeping on a host-only context; the positions follow them"""
    d = Dspi(flavor, S, device=None)
    d.spdif_block_pos(40)
    d.spdif_per_stream(1)
    d.pause_streams(60, 10)
    assert d.boot_streams([3, 64, S - 1]) == 48
    want = np.full(S, 40, dtype=np.uint32); want[[3, 64, S - 1]] = 0
    assert np.array_equal(d.spdif_stream_pos(), want), "dspi_boot_streams zeroes the listed positions, paused slots among them"
    assert d.boot_streams([5], as_is=True) == 48
    want[5] = 0
    d.resume_streams(0, S)
    assert np.array_equal(d.spdif_stream_pos(), want) and d.spdif_block_pos() == 40
    # a refused boot and a refused pause move nobody
    with pytest.raises(DspiError): d.boot_streams([7, 7])
    with pytest.raises(DspiError): d.pause_streams(S - 1, 2)
    assert np.array_equal(d.spdif_stream_pos(), want)
    # with the mode off the same calls work as before
    d.spdif_per_stream(0)
    assert d.boot_streams([9]) == 48 and d.spdif_block_pos() == 40
    d.close()
