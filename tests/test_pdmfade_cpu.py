"""The PDM fade-out's book without a GPU: dspi_amd/csrc/dspi_pdmfade.{h,cpp} beside an untouched PdmLife, through a g++ driver
(tests/pdmfade_driver.cpp) wired as the context wires them, against a model that states the rule of include/dspi.h naively: per stream a
running byte and a fade position, every call walks every stream."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes, else plain"""
    exe = tmp_path_factory.mktemp("pdmfade") / "pdmfade_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "pdmfade_driver.cpp"),
           os.path.join(CSRC, "dspi_pdmfade.cpp"), os.path.join(CSRC, "dspi_pdmlife.cpp"), os.path.join(CSRC, "dspi_move.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0: subprocess.run(cmd, check=True)
    return str(exe)


def run(driver, script):
    return subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


class Model:
    def __init__(self, n):
        self.n, self.mode = n, False
        self.running, self.pos, self.active, self.sub = [0] * n, [0] * n, [True] * n, [False] * n

    def entries(self):
        """(stream, reset, aux) of every listed stream, and the unlisted runs"""
        out, unl = [], []
        for s in range(self.n):
            if self.active[s] and (self.sub[s] or (self.mode and self.running[s])):
                reset = not self.running[s]
                aux = "0"
                if self.mode and not reset:
                    if self.sub[s]: aux = f"c{self.pos[s]}" if self.pos[s] else "0"
                    else: aux = f"f{self.pos[s] or 1024}"
                out.append((s, reset, aux))
            elif unl and unl[-1][1] == s: unl[-1][1] = s + 1
            else: unl.append([s, s + 1])
        return out, unl

    def render(self):
        e, unl = self.entries()
        return ("L" + "".join(f" r{s}" if r else f" {s}" for s, r, _ in e) + " A" + "".join(" " + a for _, _, a in e) + " U" + "".join(f" {a}-{b}" for a, b in unl)
                + f" any={int(any(a != '0' for _, _, a in e))}")

    def call(self, frames):
        e, _ = self.entries()
        listed = {s for s, _, _ in e}
        for s in range(self.n):
            if self.active[s] and s not in listed: self.running[s] = 0
        for s, reset, aux in e:
            self.running[s] = 1
            if not self.mode: continue
            if reset or aux[0] == "c": self.pos[s] = 0
            elif aux[0] == "f":
                p = int(aux[1:])
                if p - 1 <= frames: self.pos[s], self.running[s] = 0, 0
                else: self.pos[s] = p - frames

    def step(self, line):
        cmd, *a = line.split(); a = list(map(int, a))
        if cmd == "mode":
            if a[0] and not self.mode: self.pos = [0] * self.n
            if not a[0] and self.mode:
                for s in range(self.n):
                    if self.pos[s]: self.pos[s], self.running[s] = 0, 0
            self.mode = bool(a[0])
        elif cmd == "sub": self.sub[a[0]] = bool(a[1])
        elif cmd in ("pause", "resume"):
            for s in range(a[0], a[0] + a[1]): self.active[s] = cmd == "resume"
        elif cmd == "move":
            mv = list(zip(a[0::2], a[1::2]))
            old = list(self.running), list(self.active), list(self.sub), list(self.pos)
            dsts = {d for _, d in mv}
            for s, d in mv: self.running[d], self.active[d], self.sub[d], self.pos[d] = old[0][s], old[1][s], old[2][s], old[3][s]
            for s, _ in mv:
                if s not in dsts: self.active[s] = False
        elif cmd == "arrive":
            s, r, p, act, sub = a
            self.running[s], self.active[s], self.sub[s] = r, bool(act), bool(sub)
            if self.mode: self.pos[s] = p
            else:
                self.pos[s] = 0
                if p: self.running[s] = 0
        elif cmd == "boot":
            for s in a: self.running[s], self.pos[s], self.sub[s] = 0, 0, False
        elif cmd == "resize":
            n = a[0]
            for book, fill in ((self.running, 0), (self.pos, 0), (self.active, True), (self.sub, False)):
                del book[n:]; book.extend([fill] * (n - len(book)))
            self.n = n
        elif cmd == "run":
            for k, v in enumerate(a[1:]): self.running[a[0] + k] = v
        elif cmd == "pos": self.pos[a[0]] = a[1]
        elif cmd == "plan": return self.render()
        elif cmd == "call":
            r = self.render(); self.call(a[0]); return r
        elif cmd == "get": return "B" + "".join(f" {b}" for b in self.running) + " P" + "".join(f" {p}" for p in self.pos) + f" mode={int(self.mode)}"
        return None


def check(driver, n, script):
    """runs the script through the driver and the model; the printed lines agree (W <builds> and the dirty word aside).  Returns the driver's lines."""
    m = Model(n)
    want = [w for w in (m.step(l) for l in script) if w is not None]
    got = run(driver, [f"new {n}"] + script)
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        g2 = g.split(" ", 2)[2] if g.startswith("W ") else g.rsplit(" ", 1)[0]
        assert g2 == w, f"driver: {g}\nmodel:  {w}"
    return got


def builds(line): return int(line.split()[1])


@pytest.mark.parametrize("frames,left", [(48, 976), (1022, 2), (1023, 0), (1024, 0)])
def test_call_lengths_against_a_whole_fade(driver, frames, left):
    """a disable, then one call of `frames` frames: the position it leaves; 0 = the fade is over, the byte 0"""
    got = check(driver, 3, ["mode 1", "sub 0 1", "sub 1 1", "sub 2 1", "call 48", "sub 1 0", f"call {frames}", "get", "call 5", "get", "call 5", "get"])
    assert " A 0 f1024 0 " in got[1]
    assert got[2].startswith(f"B 1 {1 if left else 0} 1 P 0 {left} 0 ")
    if left == 2: assert " A 0 f2 0 " in got[3] and got[4].startswith("B 1 0 1 P 0 0 0 ")      # one more frame, then over
    if left == 0: assert " L 0 2 A 0 0 U 1-2 " in got[3]                                          # a stopped stream from the next call on


@pytest.mark.parametrize("frames", [48, 1022, 1023, 1024])
def test_call_lengths_against_a_remaining_fade(driver, frames):
    """a fade that stands at 600 (599 samples left) against each call length"""
    got = check(driver, 2, ["mode 1", "sub 0 1", "sub 1 1", "call 10", "sub 0 0", "call 424", "get", f"call {frames}", "get"])
    assert got[2].startswith("B 1 1 P 600 0 ")
    assert got[4].startswith("B 1 1 P 552 0 " if frames == 48 else "B 0 1 P 0 0 ")


@pytest.mark.parametrize("at", [1023, 512, 2])
def test_cancel(driver, at):
    """the sub comes on again while the fade stands at `at`: the aux word says so, no reset bit, the position is gone after the call"""
    got = check(driver, 2, ["mode 1", "sub 0 1", "sub 1 1", "call 10", "sub 1 0", f"call {1024 - at}", "get", "sub 1 1", "plan", "get", "call 7", "get", "call 7"])
    assert got[2].startswith(f"B 1 1 P 0 {at} ")
    assert f" L 0 1 A 0 c{at} " in got[3]
    assert got[4].startswith(f"B 1 1 P 0 {at} "), "a plan without a commit changes nothing"
    assert got[6].startswith("B 1 1 P 0 0 ") and " L 0 1 A 0 0 " in got[7]


def test_pause_freezes_the_fade(driver):
    got = check(driver, 3, ["mode 1", "sub 0 1", "sub 1 1", "sub 2 1", "call 4", "sub 1 0", "call 100", "pause 1 1", "call 100", "call 100", "get",
                            "resume 1 1", "call 100", "get"])
    assert got[4].startswith("B 1 1 1 P 0 924 0 ") and " A 0 f924 0 " in got[5] and got[6].startswith("B 1 1 1 P 0 824 0 ")


def test_move_arrive_boot_resize(driver):
    got = check(driver, 6, ["mode 1"] + [f"sub {s} 1" for s in range(6)] + ["call 8", "sub 1 0", "sub 4 0", "call 24", "get",
                            "move 1 2 2 1", "get", "call 24", "get",                 # a fading stream swaps with a running one
                            "pause 5 1", "move 2 5", "get", "call 24", "get",         # ... and moves one way into a paused slot
                            "arrive 0 1 300 1 0", "get", "call 24", "get",            # a fading arrival
                            "boot 4", "get", "call 24",
                            "pause 4 2", "resize 4", "resize 7", "get", "call 24", "get"])
    assert got[2].startswith("B 1 1 1 1 1 1 P 0 1000 0 0 1000 0 ")
    assert got[3].startswith("B 1 1 1 1 1 1 P 0 0 1000 0 1000 0 ")
    assert got[5].startswith("B 1 1 1 1 1 1 P 0 0 976 0 976 0 ")
    assert got[6].startswith("B 1 1 1 1 1 1 P 0 0 976 0 976 976 ")      # (the open-end source keeps its value, paused)
    assert got[9].startswith("B 1 1 1 1 1 1 P 300 0 976 0 952 952 ")
    assert got[12].startswith("B 1 1 1 1 0 1 P 276 0 976 0 0 928 ")
    assert got[14].startswith("B 1 1 1 1 0 0 0 P 252 0 976 0 0 0 0 ")      # (a cut position is gone, new slots have none)


def test_arrival_where_the_mode_is_off(driver):
    got = check(driver, 2, ["sub 0 1", "call 4", "arrive 1 1 500 1 0", "get", "arrive 1 1 0 1 1", "get"])
    assert got[1].startswith("B 1 0 P 0 0 mode=0") and got[2].startswith("B 1 1 P 0 0 mode=0")


def test_mode_off_is_pdmlife_word_for_word(driver, tmp_path):
    """the same script through this driver with the mode off and through tests/pdmlife_driver.cpp: the lists are PdmLife's own, every aux word is
    0, and the rule runs as seldom"""
    life = tmp_path / "pdmlife_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(life), os.path.join(ROOT, "tests", "pdmlife_driver.cpp"), os.path.join(CSRC, "dspi_pdmlife.cpp"),
                    os.path.join(CSRC, "dspi_move.cpp"), os.path.join(CSRC, "dspi_plan.cpp")], check=True)
    rnd = random.Random(5)
    script = []
    for _ in range(300):
        k = rnd.randrange(6)
        if k == 0: script.append(f"sub {rnd.randrange(12)} {rnd.randrange(2)}")
        elif k == 1: script.append(f"pause {rnd.randrange(10)} 2")
        elif k == 2: script.append(f"resume {rnd.randrange(10)} 2")
        elif k == 3: script.append(f"boot {rnd.randrange(12)}")
        else: script.append("call")
    ours = [l for l in run(driver, ["new 12"] + [l + " 48" if l == "call" else l for l in script]) if l.startswith("W ")]
    theirs = [l for l in subprocess.run([str(life)], input="new 12\n" + "".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n") if l.startswith("W ")]
    assert len(ours) == len(theirs) > 50
    for a, b in zip(ours, theirs):
        wa, wb = a.split(), b.split()                       # W builds L ... A ... U ... any=0   |   W builds resets L ... U ... S ...
        assert wa[1] == wb[1], "the rule ran more often"
        la, lb = wa[wa.index("L") + 1:wa.index("A")], wb[wb.index("L") + 1:wb.index("U")]
        assert la == lb and set(wa[wa.index("A") + 1:wa.index("U")]) <= {"0"} and wa[-1] == "any=0"
        assert wa[wa.index("U") + 1:-1] == wb[wb.index("U") + 1:wb.index("S")]


def test_a_steady_call_costs_nothing_and_a_fade_keeps_the_book_dirty(driver):
    got = run(driver, ["new 4", "mode 1", "sub 0 1", "sub 1 1", "call 48", "call 48", "call 48", "get", "sub 1 0", "call 48", "get", "call 48", "get"] + ["call 1000", "get", "call 48", "call 48", "get"])
    assert builds(got[0]) + 1 == builds(got[1]) == builds(got[2]), "reset bits make one rebuild, a steady call none"
    assert got[3].endswith("clean")
    assert got[5].endswith("dirty") and got[7].endswith("dirty"), "the book stays dirty while a stream fades"
    assert got[9].startswith("B 1 0 0 0 P 0 0 0 0") and builds(got[11]) == builds(got[10]) and got[12].endswith("clean")


def test_plan_without_commit_changes_nothing(driver):
    got = check(driver, 2, ["mode 1", "sub 0 1", "call 4", "sub 0 0", "get", "plan", "plan", "get", "call 10", "get"])
    assert got[2].split(" ", 2)[2] == got[3].split(" ", 2)[2] == got[5].split(" ", 2)[2] and " A f1024 " in got[2]
    assert builds(got[2]) == builds(got[3]) == builds(got[5]), "nothing changed between the plans: the rule ran once"
    assert got[1].rsplit(" ", 1)[0] == got[4].rsplit(" ", 1)[0] and got[6].startswith("B 1 0 P 1014 0")


def test_mode_off_ends_the_fades(driver):
    got = check(driver, 3, ["mode 1", "sub 0 1", "sub 1 1", "call 4", "sub 1 0", "call 10", "get", "mode 0", "get", "call 10", "mode 1", "get"])
    assert got[2].startswith("B 1 1 0 P 0 1014 0 mode=1") and got[3].startswith("B 1 0 0 P 0 0 0 mode=0") and " L 0 A 0 U 1-3 " in got[4]


def test_a_stream_set_running_by_hand_fades_and_a_reset_drops_a_stale_position(driver):
    got = check(driver, 2, ["mode 1", "run 0 1", "call 10", "get", "pos 1 77", "sub 1 1", "call 10", "get"])
    assert " L 0 A f1024 " in got[0] and got[1].startswith("B 1 0 P 1014 0") and " L 0 r1 A f1014 0 " in got[2] and got[3].startswith("B 1 1 P 1004 0")


def test_check_refusals(driver):
    got = run(driver, ["new 4", "mode 1", "check 0 0 0 0 0", "check 0", "check 4 0", "check 3 0 0", "check 0 1024", "check 0 1023", f"check 1 {29501 << 16}", f"check 1 {(29500 << 16) | 5}",
                       f"check 1 {((-29500) & 0xFFFF) << 16}", f"check 1 {((-29501) & 0xFFFF) << 16}"])
    assert got == ["ok", "stream range out of bounds", "stream range out of bounds", "stream range out of bounds", "a fade position is 0..1023", "ok",
                   "a base is within +-29500", "ok", "ok", "a base is within +-29500"]


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_against_the_model(driver, seed):
    rnd = random.Random(seed)
    n = 9
    script, paused = [], set()
    for _ in range(400):
        k = rnd.randrange(20)
        if k < 5: script.append(f"sub {rnd.randrange(n)} {rnd.randrange(2)}")
        elif k < 11: script.append(f"call {rnd.choice([1, 48, 48, 200, 511, 1022, 1023, 1024, 2000])}")
        elif k == 11: script.append("plan")
        elif k == 12:
            s = rnd.randrange(n); script.append(f"pause {s} 1"); paused.add(s)
        elif k == 13 and paused:
            s = rnd.choice(sorted(paused)); script.append(f"resume {s} 1"); paused.discard(s)
        elif k == 14: script.append(f"boot {rnd.randrange(n)}")
        elif k == 15: script.append(f"mode {rnd.randrange(2)}")
        elif k == 16:
            s = rnd.randrange(n); script.append(f"arrive {s} 1 {rnd.choice([0, 2, 500, 1023])} 1 {rnd.randrange(2)}"); paused.discard(s)      # (it arrives active)
        elif k == 17:
            a, b = rnd.sample([s for s in range(n) if s not in paused], 2); script.append(f"move {a} {b} {b} {a}")
        elif k == 18: script.append("get")
    script.append("get")
    check(driver, n, script)
