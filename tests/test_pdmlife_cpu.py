"""Which streams' PDM modulators run in a dspi_process_pdm call, without a GPU: the bookkeeping module (dspi_amd/csrc/dspi_pdmlife.{h,cpp})
through a g++ driver (tests/pdmlife_driver.cpp) against a model that states the rule of include/dspi.h naively — one byte per stream, every
call walks every stream —, the rule that a list is rebuilt only after something that can change it, and the layout of the call's buffers
(dspi_plan.h plan_call): the words buffer and the sub scratch on the three memory paths, and every plan of a call without pdm_words held to
a restatement of the layout rule as it stood before the words existed."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes, else plain"""
    exe = tmp_path_factory.mktemp("pdmlife") / "pdmlife_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "pdmlife_driver.cpp"),
           os.path.join(CSRC, "dspi_pdmlife.cpp"), os.path.join(CSRC, "dspi_move.cpp"), os.path.join(CSRC, "dspi_plan.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0: subprocess.run(cmd, check=True)
    return str(exe)


def run(driver, script):
    return subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


class Model:
    """one byte per stream; a call walks every stream"""

    def __init__(self, n):
        self.n, self.running, self.active, self.sub = n, [0] * n, [True] * n, [False] * n

    def work(self):
        lst, unl, stops = [], [], []
        for s in range(self.n):
            if self.active[s] and self.sub[s]: lst.append((s, not self.running[s]))
            else:
                if self.active[s] and self.running[s]: stops.append(s)
                if unl and unl[-1][1] == s: unl[-1][1] = s + 1
                else: unl.append([s, s + 1])
        return lst, unl, stops

    def render(self):
        lst, unl, stops = self.work()
        return ("L" + "".join(f" r{s}" if r else f" {s}" for s, r in lst) + " U" + "".join(f" {a}-{b}" for a, b in unl) + " S" + "".join(f" {s}" for s in stops),
                int(any(r for _, r in lst)))

    def call(self):
        for s in range(self.n):
            if self.active[s]: self.running[s] = 1 if self.sub[s] else 0

    def step(self, line):
        """applies one script line; what the driver must print for it, or None"""
        cmd, *a = line.split(); a = list(map(int, a))
        if cmd == "sub": self.sub[a[0]] = bool(a[1])
        elif cmd in ("pause", "resume"):
            for s in range(a[0], a[0] + a[1]): self.active[s] = cmd == "resume"
        elif cmd == "move":
            mv = list(zip(a[0::2], a[1::2]))
            old = list(self.running), list(self.active), list(self.sub)
            dsts = {d for _, d in mv}
            for s, d in mv: self.running[d], self.active[d], self.sub[d] = old[0][s], old[1][s], old[2][s]
            for s, _ in mv:
                if s not in dsts: self.active[s] = False      # (the open end keeps its byte)
        elif cmd == "arrive": self.running[a[0]], self.active[a[0]], self.sub[a[0]] = a[1], bool(a[2]), bool(a[3])
        elif cmd == "boot":
            for s in a: self.running[s], self.sub[s] = 0, False
        elif cmd == "resize":
            n = a[0]
            self.running = (self.running + [0] * n)[:n]; self.active = (self.active + [True] * n)[:n]; self.sub = (self.sub + [False] * n)[:n]; self.n = n
        elif cmd == "set": self.running[a[0]:a[0] + len(a) - 1] = a[1:]
        elif cmd == "get": return "B " + " ".join(map(str, self.running))
        elif cmd in ("plan", "call"):
            text = self.render()
            if cmd == "call": self.call()
            return text
        return None


def play(driver, n, script):
    """the driver's answers to the script's `get`, `plan` and `call` lines are the model's; returns the driver's lines"""
    got = run(driver, [f"new {n}"] + script)
    m, k = Model(n), 0
    for line in script:
        want = m.step(line)
        cmd = line.split()[0]
        if cmd in ("set", "setnull"): assert got[k].startswith("ok"), (line, got[k]); k += 1; continue
        if want is None: continue
        if cmd == "get": assert got[k].rsplit(" ", 1)[0] == want, (line, got[k], want)
        else:
            text, resets = want
            f = got[k].split(" ", 3)
            assert f[0] == "W" and int(f[2]) == resets and f[3] == text, (line, got[k], want)
        k += 1
    assert k == len(got), got[k:]
    return got


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_every_combination(driver):
    """active / paused x sub on / off x running / not: eight streams, one of each, the running ones made so by a first call"""
    n = 8
    script = []
    for s in range(n):
        if s & 1: script.append(f"sub {s} 1")      # running after the first call: 1, 3, 5, 7
    script += ["call", "get"]
    for s in range(n):
        script.append(f"sub {s} {(s >> 1) & 1}")      # sub on: 2, 3, 6, 7
    script += ["pause 4 4", "plan", "get", "call", "get", "call", "get"]
    got = play(driver, n, script)
    # spelled out once: 0 off/not, 1 stops, 2 comes up through the reset, 3 runs on; 4..7 paused: unlisted, bytes left alone (5 and 7 stay 1)
    assert got[2].split(" ", 3)[3] == "L r2 3 U 0-2 4-8 S 1"
    assert got[3].startswith("B 0 1 0 1 0 1 0 1")      # (a plan alone changes no byte)
    assert got[5].startswith("B 0 0 1 1 0 1 0 1")
    assert got[6].split(" ", 3)[3] == "L 2 3 U 0-2 4-8 S"


@pytest.mark.parametrize("n", [1, 2, 64, 65, 300])
def test_shapes(driver, n):
    """one stream, a ragged last row, everyone listed, nobody listed, every second"""
    script = ["call", "get"]                                                  # nobody
    script += [f"sub {s} 1" for s in range(n)] + ["call", "get", "call"]      # everyone: through the reset, then carried
    script += [f"sub {s} 0" for s in range(0, n, 2)] + ["call", "get"]
    script += [f"sub {s} 0" for s in range(n)] + ["call", "get", "call"]
    got = play(driver, n, script)
    assert got[0].endswith(f"L U 0-{n} S") and got[2].endswith("L" + "".join(f" r{s}" for s in range(n)) + " U S")
    assert got[4].endswith("L" + "".join(f" {s}" for s in range(n)) + " U S")


def test_list_ranges(driver):
    """the words of a row chunk (the staged path's launches): reset bits do not disturb the order"""
    n = 20
    got = run(driver, [f"new {n}"] + [f"sub {s} 1" for s in (3, 4, 9, 15, 19)] + ["call", "sub 10 1", "plan", "range 0 20", "range 0 3", "range 4 10", "range 10 11", "range 16 19", "range 19 20"])
    assert got[1].endswith("L 3 4 9 r10 15 19 U 0-3 5-9 11-15 16-19 S")
    assert got[2:] == ["R 0 6", "R 0 0", "R 1 3", "R 3 4", "R 5 5", "R 5 6"]


def test_random_sequences(driver):
    for seed in range(30):
        r = random.Random(seed)
        n = r.choice((1, 5, 17, 70, 130))
        script, active = [], [True] * n
        for _ in range(60):
            op = r.choice(("sub", "sub", "sub", "call", "call", "plan", "pause", "resume", "boot", "set", "get"))
            s = r.randrange(n)
            if op == "sub": script.append(f"sub {s} {r.randrange(2)}")
            elif op in ("pause", "resume"):
                c = r.randrange(1, min(4, n - s) + 1)
                script.append(f"{op} {s} {c}")
                for k in range(s, s + c): active[k] = op == "resume"
            elif op == "boot": script.append(f"boot {s}")
            elif op == "set": script.append(f"set {s} {r.randrange(2)}")
            else: script.append(op)
        play(driver, n, script + ["call", "get"])


# ---- maintenance --------------------------------------------------------------------------------------------------------------------------
def test_moves(driver):
    n = 8
    on = [f"sub {s} 1" for s in (0, 2, 5)] + ["call", "get"]      # running: 0, 2, 5
    # a swap (running 0 <-> stopped 1), a cycle 2 -> 3 -> 4 -> 2, and an open-end move 5 -> 6 into a paused slot: 5 keeps its byte, frozen
    play(driver, n, on + ["move 0 1 1 0", "get", "call", "get", "move 2 3 3 4 4 2", "get", "call", "get", "pause 6 1", "move 5 6", "get", "call", "get", "resume 5 1", "call", "get"])


def test_boot_grow_shrink_arrive(driver):
    n = 5
    script = [f"sub {s} 1" for s in range(n)] + ["call", "get", "boot 1 3", "get", "call", "sub 1 1", "call", "get",
                                                 "resize 8", "get", "sub 7 1", "call", "get", "pause 6 2", "resize 6", "get", "resize 7", "get", "call",
                                                 "pause 2 1", "arrive 2 1 1 1", "call", "get", "pause 3 1", "arrive 3 0 0 1", "call", "get", "resume 3 1", "call", "get"]
    got = play(driver, n, script)
    assert got[2].startswith("B 1 0 1 0 1")          # boot: to 0
    assert got[6].startswith("B 1 1 1 0 1 0 0 0")    # grow: the new slots are 0
    assert got[10].startswith("B 1 1 1 0 1 0 0 ")    # shrunk and grown again: the cut slot's byte is gone
    assert got[12].split(" ", 3)[3].startswith("L 0 1 2 4 U")      # an arrival that was running runs on: no reset bit


def test_set_get_and_refusals(driver):
    n = 6
    got = run(driver, [f"new {n}", "sub 0 1", "sub 1 1", "call", "set 1 0 1 1", "get", "setnull 0 6", "set 4 1 2", "set 5 1 1", "set 6 1", "setnull 2 0", "setnull 0 7", "set 0 1 0 3", "get"])
    assert got[1] == "ok 0 1 1" and got[2].startswith("B 1 0 1 1 0 0") and got[3] == "ok 1 0 1 1 0 0"
    assert got[4:10] == ["refused: a value is 0 or 1", "refused: stream range out of bounds", "refused: stream range out of bounds", "refused: stream range out of bounds",
                         "refused: stream range out of bounds", "refused: a value is 0 or 1"]
    assert got[10] == got[2]      # every refused call left the book as it was (and wrote nothing to `get`: the driver says so otherwise)


# ---- the dirty rule -----------------------------------------------------------------------------------------------------------------------
def builds(line): return int(line.split()[1])


def test_dirty_rule(driver):
    n = 6
    setup = [f"new {n}", "sub 0 1", "sub 3 1", "call", "call"]      # the first call carries reset bits: the second builds again
    got = run(driver, setup + ["call", "call", "plan", "get"])
    assert [builds(l) for l in got[:5]] == [1, 2, 2, 2, 2] and got[5].endswith("clean")      # ... and after it nothing is built
    # a failed call (plan without the success) that carried reset bits leaves the list valid: nothing changed
    got = run(driver, [f"new {n}", "sub 0 1", "plan", "plan", "call", "call", "call"])
    assert [builds(l) for l in got] == [1, 1, 1, 2, 2] and got[2].split(" ", 3)[3] == "L r0 U 1-6 S" and got[3].split(" ", 3)[3] == "L 0 U 1-6 S"
    # every operation that can change the list makes the next call build; one that cannot, does not
    for op, dirty in (("sub 1 1", True), ("sub 0 0", True), ("sub 0 1", False), ("pause 0 1", True), ("resume 0 1", True), ("move 0 1", True), ("boot 3", True),
                      ("resize 7", True), ("resize 5", True), ("set 2 1", True), ("arrive 2 1 1 0", True), ("setnull 0 6", False), ("get", False), ("range 0 6", False)):
        pre = ["pause 1 1"] if op == "move 0 1" else []      # (a destination is a paused slot)
        got = run(driver, setup + pre + ["call", "call"] + [op, "call"])
        b = [builds(l) for l in got if l.startswith("W")]
        assert (b[-1] - b[-2] == 1) == dirty, (op, got)
    # a stop changes a byte and no list: the call after it builds nothing
    got = run(driver, setup + ["set 2 1", "call", "get", "call"])
    assert got[2] == "ok 1" and got[3].endswith("S 2") and got[4].startswith("B 1 0 0 1") and builds(got[5]) == builds(got[3])


# ---- the call's layout (plan_call) ----------------------------------------------------------------------------------------------------------
STATE_MAP = {0: dict(C=7, P=2, R=64, O=5), 1: dict(C=11, P=4, R=128, O=9)}
MEM_DEVICE, OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
ACCEPTED_FLAGS = [f for f in range(64) if not (f & OUT_SPDIF and f & (OUT_TILED | OUT_I2S_SLOTS))]
DEVICE, DIRECT, STAGED = 0, 1, 2
MIB, GIB = 1 << 20, 1 << 30
BUFFERS = ("pcm", "pairs", "sub", "peaks", "clip", "pdm_words", "sub_scratch")


def up(v): return (v + 255) & ~255


def layout_before(c):
    """plan_call as it stood before dspi_process_pdm, restated: every field of the layout of a dspi_process call"""
    sm = STATE_MAP[c["flavor"]]
    S, R, P, C, O = c["n"], sm["R"], sm["P"], sm["C"], sm["O"]
    F, flags, p = c["n_blocks"] * c["block_len"], c["flags"], c["passed"]
    n_wg = -(-S // R)
    tiled, spdif = bool(flags & OUT_TILED), bool(flags & OUT_SPDIF)
    def buf(passed, tile_cols, per): return dict(bytes=(n_wg * R if tile_cols else S) * per if passed else 0, per=per, tile_cols=int(tile_cols), off=0)
    L = dict(frames=F, pcm=buf(True, False, F * (6 if c["bit_depth"] == 24 else 4)),
             pairs=buf(p["pairs"], tiled, (O - 1) * F * 4 if tiled else P * F * (16 if spdif else 8)), sub=buf(p["sub"], tiled, F * 4),
             peaks=buf(p["peaks"], False, c["n_blocks"] * C * 2), clip=buf(p["clip"], False, 2))
    L["two_pass"] = int(spdif and p["pairs"] and not c["all_latency"]); L["two_pass_rows"] = L["two_pass_bytes"] = 0
    if L["two_pass"]:
        row_b = R * P * F * 8
        rows = max(1, GIB // row_b)
        if rows < 256 and 256 * row_b <= 2 * GIB: rows = 256
        L["two_pass_rows"] = min(n_wg, rows); L["two_pass_bytes"] = L["two_pass_rows"] * row_b
    at = 0
    for nm in ("pcm", "pairs", "sub", "peaks", "clip"): L[nm]["off"] = at; at += up(L[nm]["bytes"])
    L["direct_bytes"] = at
    L["mem"] = DEVICE if flags & MEM_DEVICE else DIRECT if not c["no_direct"] and at <= 2 * MIB else STAGED
    moved = sum(L[nm]["bytes"] for nm in ("pcm", "pairs", "sub", "peaks"))
    k = min(8, n_wg, moved // (16 * MIB)) if moved >= 32 * MIB and n_wg >= 2 else 1
    L["rows_per_chunk"] = -(-n_wg // k); L["n_chunks"] = -(-n_wg // L["rows_per_chunk"])
    return L


def call(seed):
    r = random.Random(seed)
    flavor = r.choice((0, 1))
    n = r.choice((1, 2, r.randrange(1, 300), r.randrange(300, 3000), r.randrange(3000, 70000), r.choice((65536, 65537, 65600))))
    n_blocks = r.choice((1, 1, 2, r.randrange(1, 20), r.randrange(1, 2001)))
    block_len = r.choice((1, 48, 96, 192, r.randrange(1, 193)))
    flags = ACCEPTED_FLAGS[seed % len(ACCEPTED_FLAGS)]
    passed = dict(pcm=True, pairs=r.random() < 0.6, sub=r.random() < 0.5, peaks=r.random() < 0.6, clip=bool(flags & OUT_CLIP_FLAGS) and r.random() < 0.8)
    return dict(flavor=flavor, n=n, n_blocks=n_blocks, block_len=block_len, bit_depth=r.choice((16, 24)), flags=flags, passed=passed,
                no_direct=r.random() < 0.3, all_latency=flavor == 1 and r.random() < 0.4)


def render_call(c, words):
    sm = STATE_MAP[c["flavor"]]
    p = c["passed"]
    f = (c["n"], -(-c["n"] // sm["R"]), sm["R"], sm["C"], sm["O"], sm["P"], c["n_blocks"], c["block_len"], c["bit_depth"], c["flags"],
         p["pairs"], p["sub"], p["peaks"], p["clip"], c["no_direct"], c["all_latency"], words)
    return "C " + " ".join(str(int(x)) for x in f)


def parse_call(line):
    f = line.split()
    assert f[0] == "L", line
    v = [int(x) for x in f[1:]]
    lay = dict(zip(("frames", "mem", "two_pass", "two_pass_rows", "two_pass_bytes", "direct_bytes", "n_chunks", "rows_per_chunk"), v[:8]))
    for k, name in enumerate(BUFFERS): lay[name] = dict(zip(("bytes", "per", "tile_cols", "off"), v[8 + 4 * k:12 + 4 * k]))
    return lay


N_CALLS = 600


def test_call_without_words_is_the_call_of_before(driver):
    calls = [call(seed) for seed in range(N_CALLS)]
    lays = [parse_call(l) for l in run(driver, [render_call(c, 0) for c in calls])]
    assert len(lays) == N_CALLS
    for c, lay in zip(calls, lays):
        want = layout_before(c)
        for key, v in want.items(): assert lay[key] == v, (c, key, lay[key], v)
        assert lay["pdm_words"]["bytes"] == 0 and lay["sub_scratch"]["bytes"] == 0, (c, lay)


def test_call_with_words(driver):
    calls = [call(seed) for seed in range(N_CALLS)]
    lays = [parse_call(l) for l in run(driver, [render_call(c, 1) for c in calls])]
    reached = set()
    for c, lay in zip(calls, lays):
        sm = STATE_MAP[c["flavor"]]
        S, R, F = c["n"], sm["R"], c["n_blocks"] * c["block_len"]
        n_wg, tiled = -(-S // R), bool(c["flags"] & OUT_TILED)
        before = layout_before(c)
        # the words: 32 bytes per frame and unit, the unit that of the sub words; behind the clip flags in the direct area
        w = lay["pdm_words"]
        assert w["per"] == 32 * F and bool(w["tile_cols"]) == tiled and w["bytes"] == (n_wg * R if tiled else S) * 32 * F, (c, w)
        assert w["off"] == before["direct_bytes"] and lay["direct_bytes"] == w["off"] + up(w["bytes"]), (c, lay)
        # every other buffer and the two-pass scratch: as without the words
        for key in ("frames", "pcm", "pairs", "sub", "peaks", "clip", "two_pass", "two_pass_rows", "two_pass_bytes"): assert lay[key] == before[key], (c, key)
        # the memory path and the chunks: the same rules with the words counted
        assert lay["mem"] == (DEVICE if c["flags"] & MEM_DEVICE else DIRECT if not c["no_direct"] and lay["direct_bytes"] <= 2 * MIB else STAGED), (c, lay)
        moved = sum(before[nm]["bytes"] for nm in ("pcm", "pairs", "sub", "peaks")) + w["bytes"]
        k = min(8, n_wg, moved // (16 * MIB)) if moved >= 32 * MIB and n_wg >= 2 else 1
        assert lay["rows_per_chunk"] == -(-n_wg // k) and lay["n_chunks"] == -(-n_wg // lay["rows_per_chunk"]), (c, lay)
        # the sub scratch: only without the caller's sub; the whole call's, on the staged path one chunk's
        sc = lay["sub_scratch"]
        if c["passed"]["sub"]: assert sc["bytes"] == 0, (c, sc)
        else:
            assert sc["per"] == 4 * F and bool(sc["tile_cols"]) == tiled, (c, sc)
            assert sc["bytes"] == (lay["rows_per_chunk"] * R * 4 * F if lay["mem"] == STAGED else w["bytes"] // 8), (c, sc)
        reached |= {("mem", lay["mem"], tiled, c["flavor"]), ("scratch", lay["mem"], bool(sc["bytes"])), ("chunks", min(lay["n_chunks"], 3))}
        if lay["mem"] != before["mem"]: reached.add("the words moved the call off the direct path")
        if lay["n_chunks"] != before["n_chunks"]: reached.add("the words changed the chunking")
    want = {("mem", m, t, f) for m in (DEVICE, DIRECT, STAGED) for t in (False, True) for f in (0, 1)} | {("scratch", m, b) for m in (DEVICE, DIRECT, STAGED) for b in (False, True)}
    assert reached >= want | {("chunks", 1), ("chunks", 2), ("chunks", 3), "the words moved the call off the direct path", "the words changed the chunking"}, want - reached


def test_direct_threshold_with_words(driver):
    """one packet of 48 frames, float, stream-major, pcm and the words alone: 192 + 1536 bytes per stream, each region rounded up to 256"""
    def lay(n): return parse_call(run(driver, [render_call(dict(flavor=1, n=n, n_blocks=1, block_len=48, bit_depth=16, flags=0, no_direct=False, all_latency=False,
                                                               passed=dict(pairs=False, sub=False, peaks=False, clip=False)), 1)])[0])
    n = max(k for k in range(1, 2000) if up(192 * k) + up(1536 * k) <= 2 * MIB)
    assert lay(n)["mem"] == DIRECT and lay(n + 1)["mem"] == STAGED and lay(n)["direct_bytes"] <= 2 * MIB < lay(n + 1)["direct_bytes"]
