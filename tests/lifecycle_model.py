"""Lifecycle fuzz: one generator of legal stream-maintenance sequences and one model that follows them (no GPU needed to import this).

schedule(seed) draws a configuration and a list of ops — runs in every output form, PDM, pauses, resumes, requests, moves, compactions,
boots, enumerations, exports, imports (also of stashes that later ops have made stale), realignments, the per-stream S/PDIF mode, carried
S/PDIF positions and image counts — over two contexts: the main one (index 0) and a side context of 70 streams (index 1) that stands in
for another GPU.  The generator keeps its own record of which slots are paused, so that every op is legal by the rules of include/dspi.h,
and strings some ops into short motifs (a boot, then a move of the booted stream, then a run; an export, then a change at the source, then
the import of the now stale stash; ...) so that a few dozen seeds contain every crossing of two features (tests/test_lifecycle_cpu.py
counts them).

Life is the model: test_gpu_boot.BootSched (itself test_gpu_pause.Sched plus power cycles) per context, with test_gpu_move.relocate for
moves, and in addition per slot the PDM record, the S/PDIF record and position and the origin of the stream (which context's preset it
started on).  Its verify() replays each slot on a fresh oracle.  Everything is bit-exact; there is no tolerance anywhere in here.

host_schedule() is the same generator restricted to what a host-only context does (tests/test_lifecycle_cpu.py runs it)."""
import copy
import struct

import numpy as np

import orclib
from orclib import PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from test_boot_cpu import flash_cases
from test_gpu_boot import BootSched
from test_gpu_fuzz import RATES, random_blob
from test_gpu_move import relocate
from test_gpu_snapshot import as_input, context, oracle, packets

FLAVORS = {"f32": 1, "fma": W.F32_FMA, "q28": 0}
LAYOUTS = ("packed", "skew", None)
SIDE = 70                   # streams of the side context
WARM = 12                   # packets of the warm-up run: a context's first 512 samples are the power-on mute, whose words are all zero
TOTAL = WARM + 3 * 20       # packets of input per stream: the warm-up and at most 20 runs of at most 3 packets
FILL = 0x5A5A5A5A
KINDS = ("run", "pdm", "pause", "resume", "request", "move", "compact", "boot", "enumerate", "export", "import", "realign", "spdif_mode",
         "spdif_carry", "image_count")
REQUESTS = ("volume", "band", "preamp", "delay", "load_bulk", "load_slot", "clear_clips")


def row(fl):
    return 64 if fl == "q28" else 128


def sizes(fl):
    """the smallest shapes with lane mates, a row edge, a partial last row and cross-row traffic (three rows, a ragged odd last stream)"""
    R = row(fl)
    return (2, 3, 37, R - 1, R + 3, 199 if fl == "q28" else 299)


def compaction(paused, one_way):
    """dspi_plan_compaction's documented pairing: H = the paused slots below A, T = the active slots at or above A (A active streams)"""
    paused = np.asarray(paused, dtype=bool)
    A = int((~paused).sum())
    H, T = np.flatnonzero(paused[:A]), A + np.flatnonzero(~paused[A:])
    out = []
    for h, t in zip(H.tolist(), T.tolist()):
        out.append((t, h))
        if not one_way: out.append((h, t))
    return out


def moved_activity(paused, moves):
    """who is paused after dspi_move_streams: activity travels with the stream, an open-end source becomes paused"""
    new = paused.copy()
    dsts = {d for _, d in moves}
    for s, d in moves: new[d] = paused[s]
    for s, _ in moves:
        if s not in dsts: new[s] = True
    return new


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, rng, fl, sizes_):
        self.rng, self.fl, self.S = rng, fl, list(sizes_)
        self.paused = [np.zeros(S, dtype=bool) for S in self.S]
        self.unenum = [np.zeros(S, dtype=bool) for S in self.S]      # booted and not yet set up by its host
        self.due = [0] * len(self.S)                                 # runs left until the enumeration of a context's arrivals
        self.stashes = []                                            # (context, first, count, made with the S/PDIF mode on)
        self.mode = False
        self.ops = []

    def emit(self, **op):
        self.ops.append(op)
        return op

    def ctx(self):
        return 1 if len(self.S) > 1 and self.rng.random() < 0.25 else 0

    def range(self, c, cap=None):
        S = self.S[c]
        first = int(self.rng.integers(0, S)); count = int(self.rng.integers(1, S - first + 1))
        if self.rng.random() < 0.5: count = min(count, int(self.rng.integers(1, 6)))
        if cap: count = min(count, cap)
        return first, count

    # -- ops; each returns False where it has no legal instance
    def run(self, c, spdif=None):
        r = self.rng
        n = int(r.integers(1, 4))
        mem = "device" if r.random() < 0.4 else "host"
        tiled, enabled_only, clip, i2s = bool(r.random() < 0.4), bool(r.random() < 0.3), bool(r.random() < 0.7), bool(r.random() < 0.3)
        if spdif is None: spdif = self.mode and r.random() < 0.5
        if spdif: tiled = i2s = False
        self.emit(op="run", ctx=c, n=n, mem=mem, tiled=tiled, enabled_only=enabled_only, clip=clip, i2s=i2s, spdif=bool(spdif))
        if self.due[c] > 0:
            self.due[c] -= 1
            if self.due[c] == 0: self.enumerate(c)
        return True

    def pdm(self, c):
        self.emit(op="pdm", ctx=c, tiled=bool(self.rng.random() < 0.4)); return True

    def pause(self, c, first=None, count=None):
        if first is None: first, count = self.range(c)
        self.paused[c][first:first + count] = True
        self.emit(op="pause", ctx=c, first=first, count=count); return True

    def resume(self, c, first=None, count=None):
        if first is None: first, count = self.range(c)
        self.paused[c][first:first + count] = False
        self.emit(op="resume", ctx=c, first=first, count=count, as_is=bool(self.rng.random() < 0.3)); return True

    def request(self, c, stream="draw", kind=None):
        r = self.rng
        if stream == "draw": stream = None if r.random() < 0.4 else int(r.integers(0, self.S[c]))
        kinds = [k for k in REQUESTS if k != "load_bulk" or stream is not None]
        kind = kind or str(r.choice(kinds))
        N = 9 if FLAVORS[self.fl] else 5
        f = lambda v: struct.pack("<f", float(v))
        if kind == "volume": name, args = "set_volume", (int(r.choice([0, -3 * 256, -12 * 256])),)
        elif kind == "band":
            name, args = "vendor_set", (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", int(r.integers(0, 2)), int(r.integers(0, 10)),
                                        int(r.choice([W.FILTER_LOWSHELF, W.FILTER_HIGHSHELF, W.FILTER_PEAKING])), 0, float(r.uniform(100, 8000)), float(r.uniform(0.5, 2.0)), float(r.uniform(-6, 6))))
        elif kind == "preamp": name, args = "vendor_set", (W.REQ["SET_PREAMP"], 0, f(r.uniform(-12, 0)))
        elif kind == "delay": name, args = "vendor_set", (W.REQ["SET_OUTPUT_DELAY"], int(r.integers(0, N)), f(r.choice([0.0, r.uniform(0, 0.4), r.uniform(0, 9.0)])))
        elif kind == "load_bulk": name, args = "load_bulk", ("blob2",)      # (names are resolved by the executor: the second random preset, the preset image)
        elif kind == "load_slot": name, args = "load_slot", ("image", -1)
        else: name, args = "clear_clips", ()
        self.emit(op="request", ctx=c, stream=stream, kind=kind, name=name, args=args); return True

    def move_list(self, c, must_src=None, one_way=False):
        """a legal list mixing swaps, a 3-cycle, a chain and one-way entries: no slot is the source of two entries or the destination of two,
        and a destination that is no source is paused before the call.  must_src: the first entry's source; one_way: the first piece has an
        open end"""
        r, paused = self.rng, self.paused[c]
        pool = [int(v) for v in r.permutation(self.S[c])]      # the slots no entry names yet

        def take(s=None):
            s = pool[0] if s is None else s
            pool.remove(s)
            return s

        moves = []
        for i in range(int(r.integers(1, 5))):
            src = must_src if i == 0 else None
            hole = next((s for s in pool if paused[s] and s != src), None)
            kinds = [k for k, need, open_end in (("swap", 2, False), ("cycle", 3, False), ("one-way", 2, True), ("chain", 3, True))
                     if len(pool) >= need and (hole is not None or not open_end) and (open_end or not (one_way and i == 0))]
            if not kinds: break
            k = str(r.choice(kinds))
            if k in ("one-way", "chain"): take(hole)
            a = take(src)
            if k == "one-way": moves += [(a, hole)]; continue
            b = take()
            if k == "swap": moves += [(a, b), (b, a)]
            elif k == "chain": moves += [(a, b), (b, hole)]
            else:
                c3 = take()
                moves += [(a, b), (b, c3), (c3, a)]
        return moves

    def move(self, c, must_src=None, one_way=False):
        if self.S[c] < 2: return False
        moves = self.move_list(c, must_src, one_way)
        if not moves: return False
        self.apply_moves(c, moves)
        self.emit(op="move", ctx=c, moves=moves, as_is=bool(self.rng.random() < 0.3)); return True

    def apply_moves(self, c, moves):
        self.paused[c] = moved_activity(self.paused[c], moves)
        old = self.unenum[c].copy()
        for s, d in moves: self.unenum[c][d] = old[s]

    def compact(self, c):
        one_way = bool(self.rng.random() < 0.5)
        moves = compaction(self.paused[c], one_way)
        if not moves: return False
        self.apply_moves(c, moves)
        self.emit(op="compact", ctx=c, one_way=one_way, moves=moves, as_is=bool(self.rng.random() < 0.3)); return True

    def boot(self, c, must=None):
        r, S = self.rng, self.S[c]
        if r.random() < 0.3 and must is None:
            first, count = self.range(c, cap=8)
            streams = list(range(first, first + count))
        else:
            streams = [int(v) for v in r.permutation(S)[:int(r.integers(1, 6))]]
            if must is not None and must not in streams: streams[0] = must
        self.unenum[c][streams] = True
        self.emit(op="boot", ctx=c, streams=streams, dump=bool(r.random() < 0.6), as_is=bool(r.random() < 0.3))
        if len(self.S) > 1 and self.mode and r.random() < 0.4:      # (not on a host-only context) the first frame after the boot, at the power-on rate: preamble Z, 44.1 kHz in the channel status
            self.due[c] = 1; self.run(c, spdif=True)
        elif r.random() < 0.5: self.enumerate(c)
        else: self.due[c] = int(r.integers(1, 3))
        return True

    def enumerate(self, c):
        streams = np.flatnonzero(self.unenum[c]).tolist()
        if not streams: return False
        self.unenum[c][:] = False; self.due[c] = 0
        self.emit(op="enumerate", ctx=c, streams=streams, blob_on=[s for s in streams if self.rng.random() < 0.3]); return True

    def export(self, c, first=None, count=None):
        if first is None: first, count = self.range(c, cap=min(self.S))
        self.stashes.append((c, first, count, self.mode, self.unenum[c][first:first + count].copy()))
        self.emit(op="export", ctx=c, first=first, count=count, stash=len(self.stashes) - 1); return True

    def import_(self, c=None, stash=None, to=None):
        r = self.rng
        if not self.stashes: return False
        if stash is None: stash = int(r.integers(0, len(self.stashes)))
        count = self.stashes[stash][2]
        if c is None:
            c = self.ctx()
            if count > self.S[c]: c = 1 - c
        if count > self.S[c]: return False
        if to is None: to = int(r.integers(0, self.S[c] - count + 1))
        self.unenum[c][to:to + count] = self.stashes[stash][4]
        self.emit(op="import", ctx=c, stash=stash, to=to, count=count, realign=bool(r.random() < 0.5))
        if self.mode and self.stashes[stash][3] and r.random() < 0.9: self.emit(op="spdif_carry", ctx=c, stash=stash, to=to, count=count)
        return True

    def realign(self, c):
        first, count = self.range(c)
        self.emit(op="realign", ctx=c, first=first, count=count); return True

    def spdif_mode(self):
        if self.mode: return False
        self.mode = True
        self.emit(op="spdif_mode", ctx=0, mul=int(self.rng.choice([5, 7, 11, 13])), add=int(self.rng.integers(0, 192))); return True

    def image_count(self, c):
        self.emit(op="image_count", ctx=c); return True

    # -- motifs: the crossings of two features, each a few ops long
    def a_paused_slot(self, c):
        """a paused slot of the context, pausing one first where there is none"""
        p = np.flatnonzero(self.paused[c])
        if len(p) and self.rng.random() < 0.7: return int(self.rng.choice(p))
        first, count = self.range(c, cap=3)
        if count >= self.S[c]: first, count = 0, 1
        self.pause(c, first, count)
        return first

    def motif(self):
        r = self.rng
        c = self.ctx()
        S = self.S[c]
        k = int(r.choice(6, p=[0.1, 0.14, 0.16, 0.14, 0.31, 0.15]))
        if k == 0:      # a booted stream is moved, then plays
            s = int(r.integers(0, S))
            self.boot(c, must=s)
            self.move(c, must_src=s); self.run(c)
        elif k == 1:    # a stash goes stale: the source is changed after the export, then the stash comes back
            first, count = self.range(c, cap=min(self.S))
            self.export(c, first, count)
            stash = len(self.stashes) - 1
            s = first + int(r.integers(0, count))
            what = int(r.integers(0, 3))
            if what == 0: self.request(c, stream=s if r.random() < 0.6 else None)
            elif what == 1: self.boot(c, must=s)
            else: self.move(c, must_src=s)
            if r.random() < 0.5: self.run(c)
            self.import_(stash=stash, c=c if r.random() < 0.6 else None)
        elif k == 2:    # an import into a paused slot, which is resumed afterwards
            if not self.stashes: self.export(self.ctx())
            stash = int(r.integers(0, len(self.stashes)))
            count = self.stashes[stash][2]
            if count > S: c = 1 - c; S = self.S[c]
            if count > S: return
            to = int(r.integers(0, S - count + 1))
            self.pause(c, to, count)
            self.import_(c=c, stash=stash, to=to)
            if r.random() < 0.5: self.run(c)
            self.resume(c, to, count); self.run(c)
        elif k == 3:    # a one-way move, then a request to the moved stream alone: its parameter object is shared with the frozen copy
            if S < 2: return
            self.a_paused_slot(c)
            if self.paused[c].all(): self.resume(c, 0, 1)
            if not self.move(c, one_way=True): return
            src, dst = self.ops[-1]["moves"][0]      # (one-way: src -> hole; chain: src -> b -> hole; either way src stays behind as a frozen copy)
            self.request(c, stream=dst, kind=str(r.choice(["load_bulk", "band", "load_slot", "preamp", "delay"])))
            self.run(c)
            if r.random() < 0.5:
                self.resume(c, src, 1); self.run(c)      # the frozen copy goes its own way, without the request
        elif k == 4:    # PDM on both sides of a move, an import or a boot
            what = int(r.choice(3, p=[0.3, 0.37, 0.33]))
            if what == 1 and not self.stashes: self.export(self.ctx())
            self.pdm(c)
            if not ((what == 0 and self.move(c)) or (what == 1 and self.import_(c=c))): self.boot(c)
            self.run(c); self.pdm(c)
        else: self.compact_something(c)

    def compact_something(self, c):
        """a compaction, pausing a range first where there is nothing to compact, then a run"""
        S = self.S[c]
        if not compaction(self.paused[c], True):
            first, count = self.range(c, cap=max(1, S // 2))
            if first + count >= S: first = 0
            self.pause(c, first, count)
        if self.paused[c].all(): return False
        self.compact(c); self.run(c)
        return True

    def single(self):
        r = self.rng
        kind = str(r.choice(["run", "pdm", "pause", "resume", "resume", "request", "request", "move", "compact", "boot", "export", "import", "import", "import",
                             "import", "realign", "realign", "realign", "realign", "realign", "image_count", "image_count", "spdif_mode"]))
        c = self.ctx()
        return {"run": lambda: self.run(c), "pdm": lambda: self.pdm(c), "pause": lambda: self.pause(c), "resume": lambda: self.resume(c),
                "request": lambda: self.request(c), "move": lambda: self.move(c), "compact": lambda: self.compact_something(c), "boot": lambda: self.boot(c),
                "export": lambda: self.export(c), "import": lambda: self.import_(), "realign": lambda: self.realign(c),
                "image_count": lambda: self.image_count(c), "spdif_mode": self.spdif_mode}[kind]()


def schedule(seed):
    """(config, ops): a pure function of the seed"""
    rng = np.random.default_rng(52000 + seed)
    fl = ("f32", "fma", "q28")[int(rng.integers(0, 3))]
    layout = LAYOUTS[int(rng.integers(0, 3))]
    fs, Bs = RATES[seed % 3]
    B = int(rng.choice(Bs)); depth = 16 if rng.random() < 0.5 else 24
    S = int(rng.choice(sizes(fl)))
    flavor = FLAVORS[fl]
    P = 4 if int(flavor) else 2
    blob, blob2 = random_blob(rng, int(flavor), fs), random_blob(rng, int(flavor), fs)
    blob["i2s_config"]["output_types"][1] = 1               # slot 1 is an I2S slot on the main context's preset,
    blob2["i2s_config"]["output_types"][0] = 1              # slot 0 on the other one: DSPI_OUT_I2S_SLOTS has words to shift
    for b in (blob, blob2):                                 # (a preset whose every output is off says little: the first two play)
        b["outputs"]["enabled"][:P] = 1; b["outputs"]["mute"][:2] = 0; b["crosspoints"]["enabled"][:, :2] = 1
    cfg = dict(seed=seed, flavor=fl, layout=layout, fs=fs, B=B, depth=depth, S=S, side=SIDE, R=row(fl), blob=blob, blob2=blob2,
               vol=int(rng.choice([0, -5 * 256, -20 * 256])), vol_side=int(rng.choice([0, -9 * 256])), first_stream=int(rng.integers(0, 20)))
    g = _Gen(rng, fl, (S, SIDE))
    g.emit(op="run", ctx=0, n=WARM, mem="host", tiled=False, enabled_only=False, clip=True, i2s=False, spdif=False, warm=True)
    g.emit(op="run", ctx=1, n=WARM, mem="host", tiled=False, enabled_only=False, clip=True, i2s=False, spdif=False, warm=True)
    if rng.random() < 0.55: g.spdif_mode()
    target = len(g.ops) + int(rng.integers(8, 15))
    # (the mode's share, the motifs' weights and the chance of an S/PDIF run after a maintenance call are tuned against
    #  tests/test_lifecycle_cpu.py::test_default_seeds_contain_the_crossings: a change to the generator is meant to trip that test)
    while len(g.ops) < target - 2:
        last = g.ops[-1]
        if g.mode and last["op"] in ("pause", "resume", "move", "boot", "import", "spdif_carry") and rng.random() < (0.6 if last["op"] in ("move", "resume") else 0.9): g.run(last["ctx"], spdif=True)
        elif rng.random() < 0.45: g.motif()
        else: g.single()
    del g.ops[target - 2:]                                  # (a motif may run over; every prefix of a legal sequence is legal)
    g.due = [0, 0]
    g.run(1); g.run(0)                                      # a closing run on each context: whatever the last ops did is heard
    return cfg, g.ops


def host_schedule(seed, fl, S, n_ops=40):
    """the same generator on one host-only context: requests, pauses, resumes, boots, enumerations, the S/PDIF mode and positions,
    compaction plans, image counts — and the calls such a context must refuse after validating them (`refused`)"""
    rng = np.random.default_rng(61000 + seed)
    g = _Gen(rng, fl, (S,))
    while len(g.ops) < n_ops:
        kind = str(rng.choice(["request", "request", "request", "pause", "pause", "resume", "boot", "enumerate", "spdif_mode", "spdif_pos", "plan", "image_count", "refused"]))
        if kind == "request": g.request(0)
        elif kind == "pause": g.pause(0)
        elif kind == "resume": g.resume(0)
        elif kind == "boot": g.boot(0)
        elif kind == "enumerate": g.enumerate(0)
        elif kind == "spdif_mode": g.spdif_mode()
        elif kind == "spdif_pos":
            if g.mode:
                first, count = g.range(0)
                g.emit(op="spdif_pos", ctx=0, first=first, values=[int(v) for v in rng.integers(0, 192, count)])
        elif kind == "plan": g.emit(op="plan", ctx=0, one_way=bool(rng.random() < 0.5), moves=None)
        elif kind == "image_count": g.image_count(0)
        else:
            what = str(rng.choice(["move", "import", "export", "realign"]))
            first, count = g.range(0)
            moves = g.move_list(0) if S >= 2 else []
            if what == "move" and not moves: continue
            g.emit(op="refused", ctx=0, what=what, first=first, count=count, moves=moves)
    return g.ops[:n_ops]


def named(ops):
    """{context: every slot an op of the list names}"""
    out = {}
    for op in ops:
        s = out.setdefault(op["ctx"], set())
        k = op["op"]
        if k in ("pause", "resume", "export", "realign"): s.update(range(op["first"], op["first"] + op["count"]))
        elif k in ("import", "spdif_carry"): s.update(range(op["to"], op["to"] + op["count"]))
        elif k in ("move", "compact"): s.update(v for m in op["moves"] for v in m)
        elif k in ("boot", "enumerate"): s.update(op["streams"])
        elif k == "request" and op["stream"] is not None: s.add(op["stream"])
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
class Life(BootSched):
    """BootSched with everything else a slot carries through maintenance calls.  bases: [(preset, volume)] of the contexts a stream can have
    started in; home[s]: which of them slot s's stream started in (it travels with the stream, as `booted` does)."""

    def __init__(self, d, flavor, fs, bases, home, data, depth, B, blob2=None, image=None):
        blob, vol = bases[home]
        super().__init__(d, flavor, fs, blob, data.copy(), depth, B, vol, True)
        S = d.n_streams
        self.bases, self.home = bases, [home] * S
        self.names = {"blob2": blob2, "image": image}
        self.paused = np.zeros(S, dtype=bool)
        self.pdm = [[] for _ in range(S)]               # [(the sub words that were modulated, the words returned)], in order
        self.mode = False
        self.sp = np.zeros(S, dtype=np.int64)           # the slot's own S/PDIF block position (mode on)
        self.last_sub = None

    # -- requests, pauses
    def request(self, name, *args, stream=None, want=0):
        args = tuple(self.names.get(a, a) if isinstance(a, str) else a for a in args)
        if name != "clear_clips": return super().request(name, *args, stream=stream, want=want)
        S = self.d.n_streams
        self.d.clear_clips(stream=host.ALL if stream is None else stream)
        for s in (range(S) if stream is None else (stream,)):
            self.hooks[s].setdefault(int(self.pos[s]), []).append(("vendor_get", (W.REQ["CLEAR_CLIPS"], 0)))
            self.last_clip[s] = 0
            if s in self.frozen: self.frozen[s] = (self.frozen[s][0][:-2] + b"\0\0", 0)

    def pause(self, first, count):
        super().pause(first, count); self.paused[first:first + count] = True

    def resume(self, first, count, as_is=False):
        super().resume(first, count, as_is); self.paused[first:first + count] = False

    # -- moves: relocate, extended
    def relocate(self, moves):
        moves = [(int(s), int(d)) for s, d in moves if int(s) != int(d)]
        booted, home, pdm, sp = dict(self.booted), list(self.home), [list(p) for p in self.pdm], self.sp.copy()
        relocate(self, moves)
        for s, d in moves:
            self.home[d] = home[s]; self.pdm[d] = list(pdm[s]); self.sp[d] = sp[s]
            self.booted.pop(d, None)
            if s in booted: self.booted[d] = booted[s]
        self.paused = moved_activity(self.paused, moves)

    def move(self, moves, as_is=False):
        assert self.d.move_streams(moves, as_is=as_is) == sum(1 for s, d in moves if int(s) != int(d))
        self.relocate(moves)

    # -- boots
    def boot(self, streams, dump=None, as_is=False, want=48):
        super().boot(streams, dump, as_is, want)
        for s in streams: self.pdm[int(s)] = []; self.sp[int(s)] = 0

    # -- snapshots
    def export(self, first, count):
        """a stash: the snapshot and a deep copy of the records of the range as they stand now"""
        d = self.d
        head, state = d.export_streams(first, count)
        recs = [dict(data=self.data[s].copy(), pos=int(self.pos[s]), parts=list(self.parts[s]), hooks=copy.deepcopy(self.hooks[s]), booted=s in self.booted,
                     dump=self.booted.get(s), home=self.home[s], pdm=list(self.pdm[s]), status=d.status(s), clip=int.from_bytes(d.status(s)[-2:], "little"))
                for s in range(first, first + count)]
        return dict(head=head, state=state, recs=recs, sp=d.spdif_stream_pos(first, count).astype(np.int64) if self.mode else None)

    def import_(self, to, stash, realign=False):
        """the destination's records become the stash's: the slot is rewound to the stash's moment; its activity and S/PDIF position stay"""
        recs = stash["recs"]
        assert self.d.import_streams(to, stash["head"], stash["state"], realign=realign) == len(recs)
        for k, r in enumerate(recs):
            t = to + k
            self.data[t] = r["data"]; self.pos[t] = r["pos"]; self.parts[t] = list(r["parts"]); self.hooks[t] = copy.deepcopy(r["hooks"])
            self.home[t] = r["home"]; self.pdm[t] = list(r["pdm"]); self.last_clip[t] = r["clip"]
            self.booted.pop(t, None)
            if r["booted"]: self.booted[t] = r["dump"]
            self.frozen.pop(t, None)
            if self.paused[t]: self.frozen[t] = (r["status"], r["clip"])

    def spdif_mode(self, mul, add):
        assert self.d.spdif_per_stream(1) is True
        self.mode = True
        self.sp[:] = (np.arange(self.d.n_streams) * mul + add) % 192
        assert np.array_equal(self.d.spdif_stream_pos(set=self.sp), self.sp)

    def spdif_carry(self, to, stash):
        """what the header tells a migrating caller: the position at the origin when the stash was made, set at the destination"""
        self.d.spdif_stream_pos(to, len(stash["sp"]), set=stash["sp"])
        self.sp[to:to + len(stash["sp"])] = stash["sp"]

    # -- one dspi_process call in any form
    # (lib_host, lib_device, call and part_form are the seams a subclass with other calls overrides: tests/lifecycle_wide.py)
    def lib_host(self, pcm, n, **flags):
        return self.d.process_host(pcm, n, self.B, self.depth, **flags)

    def lib_device(self, pcm_ptr, n, pairs_ptr, sub_ptr, peaks_ptr, **flags):
        self.d.process_device(pcm_ptr, n, self.B, self.depth, pairs_ptr, sub_ptr, peaks_ptr, **flags)

    def part_form(self, s):
        return {}

    def call(self, pcm, n, mem, tiled, enabled_only, clip, i2s, spdif):
        """the library call on host or device buffers: (pairs, sub, peaks, clip flags or None, the value of an unwritten word, of an unwritten peak), stream-major"""
        d, B = self.d, self.B
        S, F, P, R = d.n_streams, n * B, d.P, d.tile_streams()
        nt = -(-S // R)
        if mem == "host":
            pairs, sub, peaks = self.lib_host(pcm, n, tiled=tiled, enabled_only=enabled_only, i2s_slots=i2s, spdif=spdif, clip=clip)
            flags = d.last_clip.copy() if clip else None
            fill, kfill = 0, 0
        else:
            import torch
            dev = torch.device("cuda", 0)
            t_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
            t_pairs = torch.full((nt, 2 * P, F, R) if tiled else (S, P, F, 4 if spdif else 2), FILL, dtype=torch.int32, device=dev)
            t_sub = torch.full((nt, F, R) if tiled else (S, F), FILL, dtype=torch.int32, device=dev)
            t_peaks = torch.full((S, n, d.C), 0x5A5A, dtype=torch.int16, device=dev)
            t_clip = torch.full((S,), 0x5A5A, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            self.lib_device(t_pcm.data_ptr(), n, t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), tiled=tiled, enabled_only=enabled_only,
                            i2s_slots=i2s, spdif=spdif, clip_ptr=t_clip.data_ptr() if clip else 0)
            d.sync()
            pairs, sub, peaks = t_pairs.cpu().numpy(), t_sub.cpu().numpy(), t_peaks.cpu().numpy().view(np.uint16)
            flags = t_clip.cpu().numpy().view(np.uint16) if clip else None
            fill, kfill = np.int32(FILL), 0x5A5A
        if tiled:
            if mem == "device" and nt * R > S:
                assert (pairs.transpose(0, 3, 1, 2).reshape(nt * R, -1)[S:] == fill).all() and (sub.transpose(0, 2, 1).reshape(nt * R, -1)[S:] == fill).all(), "columns past the last stream were written"
            pairs, sub = d.untile(pairs, sub)
        if spdif: pairs = pairs.view(np.uint32)
        return pairs, sub, peaks, flags, fill, kfill

    def run(self, n, mem="host", tiled=False, enabled_only=False, clip=True, i2s=False, spdif=False, **_):
        d, B = self.d, self.B
        F = n * B
        pcm, paused = self.input(n)
        assert np.array_equal(paused, self.paused)
        pairs, sub, peaks, flags, fill, kfill = self.call(pcm, n, mem, tiled, enabled_only, clip, i2s, spdif)
        # paused regions: zeros in host buffers, the untouched fill in device buffers (tiled: the column); frozen status bytes and clip flags
        for s in np.flatnonzero(paused):
            assert (pairs[s].view(np.int32) == fill).all() and (sub[s] == fill).all() and (peaks[s] == kfill).all(), f"paused stream {s}: its regions of the {mem} buffers were written"
            status, was_clip = self.frozen[s]
            if flags is not None: assert int(flags[s]) == was_clip, f"paused stream {s}: clip flags {int(flags[s]):#x}, {was_clip:#x} when it froze"
            assert d.status(int(s)) == status, f"paused stream {s}: status bytes changed while it was paused"
        form = dict(i2s=i2s, unwritten=np.int32(FILL) if enabled_only and mem == "device" else None)
        for s in np.flatnonzero(~paused):
            p0 = int(self.pos[s])
            status = d.status(int(s))
            self.last_clip[s] = int.from_bytes(status[-2:], "little")
            self.parts[s].append((p0, p0 + n, (pairs[s], sub[s], peaks[s], flags[s] if flags is not None else None), status, dict(form, spdif=int(self.sp[s]) if spdif else None, **self.part_form(int(s)))))
            self.pos[s] += n
            if spdif: self.sp[s] = (self.sp[s] + F) % 192
        self.last_sub = sub
        return pairs, sub, peaks, flags

    def modulated(self, sub, tiled=False):
        """dspi_pdm_modulate's words for sub [S][F] (host buffers), stream-major"""
        d = self.d
        S, R = d.n_streams, d.tile_streams()
        if not tiled: return d.pdm_host(sub)
        nt = -(-S // R)
        t = np.zeros((nt * R, sub.shape[1]), dtype=np.int32); t[:S] = sub
        words = d.pdm_host(np.ascontiguousarray(t.reshape(nt, R, -1).transpose(0, 2, 1)), tiled=True)      # [tile][frame][8][R]
        return words.transpose(0, 3, 1, 2).reshape(nt * R, sub.shape[1], 8)[:S]

    def modulate(self, tiled=False):
        """dspi_pdm_modulate on the sub words of the last run (host buffers)"""
        sub, S = self.last_sub, self.d.n_streams
        words = self.modulated(sub, tiled)
        for s in range(S):
            if self.paused[s]: assert not words[s].any(), f"paused stream {s}: PDM words written"
            else: self.pdm[s].append((sub[s].copy(), words[s].copy()))

    # -- the cheap checks after every op
    def check_books(self, what):
        d = self.d
        assert np.array_equal(d.streams_paused().astype(bool), self.paused), f"{what}: dspi_streams_paused is not the model's"
        assert set(self.frozen) == set(np.flatnonzero(self.paused).tolist()), what
        for s, (status, _) in self.frozen.items():      # (the clip flags come with the runs; the status bytes carry the same bits)
            assert d.status(s) == status, f"{what}: paused stream {s}: its status bytes are not the frozen ones"
        if self.mode: assert np.array_equal(d.spdif_stream_pos(), self.sp), f"{what}: dspi_spdif_stream_pos is not the model's: {np.flatnonzero(d.spdif_stream_pos() != self.sp)[:8].tolist()}"

    def check_image_count(self, what):
        d = self.d
        n, distinct = d.image_count(), len({d.collect_bulk(s) for s in range(d.n_streams)})
        assert distinct <= n <= d.n_streams, f"{what}: {n} parameter objects for {distinct} distinct parameter sets on {d.n_streams} streams"

    # -- the replay
    def fed(self, s, p0, p1, form):
        """(the bytes slot s's stream was fed in packets [p0, p1), their bit depth)"""
        return packets(self.data[s], self.depth, self.B, p0, p1), self.depth

    def at_part(self, o, s, form, at):
        """(a subclass's own look at the replayed oracle before a part is fed)"""

    def verify(self, streams=None, what=""):
        P, B = self.d.P, self.B
        for s in (range(self.d.n_streams) if streams is None else streams):
            s = int(s)
            tag = f"{what}{'booted ' if s in self.booted else ''}stream in slot {s}"
            o = self.fresh(self.booted[s]) if s in self.booted else oracle(self.flavor, self.fs, *self.bases[self.home[s]])
            rate = [44100 if s in self.booted else self.fs]      # (the power-on rate: the channel status says 44.1 kHz until the host sets another)

            def apply(p):
                for nm, a in self.hooks[s].get(p, ()):
                    getattr(o, nm)(*a)
                    if nm == "set_rate": rate[0] = a[0]

            for p0, p1, (pairs, sub, peaks, clip), status, form in self.parts[s]:
                apply(p0)
                at = f"{tag}, packets [{p0}, {p1})"
                self.at_part(o, s, form, at)
                pcm, depth = self.fed(s, p0, p1, form)
                rp, rs, rk, rclip = o.process(pcm, p1 - p0, B, depth)
                want = rp
                if form["spdif"] is not None:      # the subframes of the oracle's words at the slot's recorded position and the stream's rate
                    want = np.stack([orclib.spdif_encode(rp[p], form["spdif"], rate[0])[0] for p in range(P)])
                elif form["i2s"]:                  # the << 8 rule of test_i2s_slot_words_fused_into_the_chain, by the stream's own slot types
                    want = rp.copy()
                    for p in range(P):
                        if o.vendor_get(W.REQ["GET_OUTPUT_TYPE"], p, 1) == b"\x01": want[p] = (rp[p].astype(np.uint32) << np.uint32(8)).astype(np.int32)
                fill = form["unwritten"]
                silent = []
                if fill is not None:               # DSPI_OUT_ENABLED_ONLY on device buffers: a pair whose two outputs are off may be left as it was
                    outs = np.frombuffer(o.collect_bulk(), dtype=W.WIRE_BULK, count=1)[0]["outputs"]["enabled"]
                    silent = [p for p in range(P) if not outs[2 * p] and not outs[2 * p + 1]]
                for p in range(P):
                    ok = np.array_equal(want[p], pairs[p]) or (p in silent and (pairs[p].view(np.int32) == fill).all())
                    assert ok, f"{at}: pair {p} differs ({form}) at {np.argwhere(want[p] != pairs[p])[:3].tolist()}"
                assert np.array_equal(rs, sub) or (fill is not None and not rs.any() and (sub == fill).all()), f"{at}: sub differs ({form})"
                assert np.array_equal(rk, peaks), f"{at}: peaks differ"
                assert rclip == int.from_bytes(o.status()[-2:], "little") and (clip is None or int(clip) == rclip), f"{at}: clip flags differ"
                assert o.status() == status, f"{at}: status differs"
            apply(int(self.pos[s]))
            assert self.d.collect_bulk(s) == o.collect_bulk(), f"{tag}: dspi_collect_bulk is not the replayed oracle's"
            o.close()
            m = PdmOracle()
            for k, (sub, words) in enumerate(self.pdm[s]): assert np.array_equal(m.run(sub), words), f"{tag}: PDM words of its modulation {k} differ"


def preset_image(flavor, fs):
    """a preset-slot image of another structure than the random presets (dspi_load_preset_slot: zeroed lines and the preset mute)"""
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, fs, other); image = ref.save_slot(0); ref.close()
    return image


def new_lives(cfg, sizes_=None):
    """the two contexts of a configuration and their models: [main, side]"""
    flavor, fs, B, depth = FLAVORS[cfg["flavor"]], cfg["fs"], cfg["B"], cfg["depth"]
    bases = [(cfg["blob"], cfg["vol"]), (cfg["blob2"], cfg["vol_side"])]
    image = preset_image(flavor, fs)
    lives = []
    for home, S in enumerate(sizes_ or (cfg["S"], cfg["side"])):
        data = as_input(WL.synth_pcm16(S, TOTAL * B, fs, first_stream=cfg["first_stream"] + 500 * home), depth)
        lives.append(Life(context(flavor, S, fs, *bases[home]), flavor, fs, bases, home, data, depth, B, blob2=cfg["blob2"], image=image))
    return lives


def execute(cfg, ops, lives, stashes=None, step=None):
    """runs the ops on the contexts, the cheap checks after each; returns the stashes.  step(op, lives, stashes, what): a caller's own
    executor for the kinds it adds (True where it has done the op)"""
    stashes = {} if stashes is None else stashes
    dump, code = flash_cases(FLAVORS[cfg["flavor"]])[0]
    for i, op in enumerate(ops):
        x, k = lives[op["ctx"]], op["op"]
        what = f"seed {cfg['seed']}, op {i} ({k})"
        if step and step(op, lives, stashes, what): pass
        elif k == "run": x.run(**{a: v for a, v in op.items() if a not in ("op", "ctx", "warm")})
        elif k == "pdm": x.modulate(op["tiled"])
        elif k == "pause": x.pause(op["first"], op["count"])
        elif k == "resume": x.resume(op["first"], op["count"], op["as_is"])
        elif k == "request": x.request(op["name"], *op["args"], stream=op["stream"])
        elif k == "move": x.move(op["moves"], op["as_is"])
        elif k == "compact":
            assert [tuple(m) for m in x.d.plan_compaction(op["one_way"]).tolist()] == op["moves"], f"{what}: dspi_plan_compaction is not the documented pairing"
            x.move(op["moves"], op["as_is"])
        elif k == "boot": x.boot(op["streams"], dump if op["dump"] else None, op["as_is"], want=code if op["dump"] else 48)
        elif k == "enumerate": x.enumerate(op["streams"], blob_on=op["blob_on"])
        elif k == "export": stashes[op["stash"]] = x.export(op["first"], op["count"])
        elif k == "import": x.import_(op["to"], stashes[op["stash"]], op["realign"])
        elif k == "realign": assert x.d.realign_streams(op["first"], op["count"]) == op["count"]
        elif k == "spdif_mode":
            for y in lives: y.spdif_mode(op["mul"], op["add"])
        elif k == "spdif_carry": x.spdif_carry(op["to"], stashes[op["stash"]])
        elif k == "image_count": x.check_image_count(what)
        else: raise AssertionError(k)
        for y in lives: y.check_books(what)
    return stashes


def describe(cfg, ops):
    return (f"lifecycle fuzz seed {cfg['seed']}: flavor {cfg['flavor']} layout {cfg['layout']} fs {cfg['fs']} B {cfg['B']} depth {cfg['depth']} S {cfg['S']} + {cfg['side']}, "
            f"ops: {' '.join(op['op'] + ('*' if op['ctx'] else '') for op in ops)}")
