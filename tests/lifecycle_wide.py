"""The wide lifecycle fuzz: tests/lifecycle_model.py's generator and model, extended by everything merged since it was written (no GPU needed to
import this) — contexts that change their size (dspi_resize_streams / dspi_reserve_streams), streams that change their context
(dspi_migrate_streams / dspi_plan_migration), dspi_plan_grouping, the PDM words out of the call (dspi_process_pdm and its running byte), the
PDM fade-out (dspi_pdm_fade) and per-stream input depths (dspi_process_mixed).

schedule_wide(seed) draws a configuration and a list of ops over the same two contexts as schedule(seed); no context grows past 3R + 1
streams (R = 128 float, 64 Q28: the smallest shapes that have a new row, a row holding one stream, lane mates and a ragged end).  WideGen keeps
its own record of sizes, capacities, activity, the fade modes and the stashes, so that every op is legal by the validation paragraphs of
include/dspi.h, and strings the new ops into motifs so that a few dozen seeds hold every crossing that tests/test_lifecycle_wide_cpu.py counts.

WideLife is the model, written from the header per slot: Life plus, for every slot, the stream's input at both bit depths (the 24-bit version
has low bytes of its own, so the 24-bit route is fed bits the 16-bit route never sees), the depth of every recorded part (depth is an argument
of the call and does not travel), one live pdmfade_model.FadeStream (modulator, running byte, fade position and base), and the capacity.
Everything is bit-exact; there is no tolerance anywhere in here."""
import ctypes as C

import numpy as np

import lifecycle_model as M
from lifecycle_model import FLAVORS, LAYOUTS, SIDE, WARM, Life, compaction, row, sizes
from pdmfade_model import FadeStream
from dspi_amd import host as H, wire as W, workloads as WL
from test_gpu_fuzz import RATES, random_blob
from test_gpu_migrate import relocate_across
from test_gpu_pdm_out import sub_setup
from test_gpu_snapshot import context, packets

NEW_KINDS = ("grow", "shrink", "reserve", "migrate", "plan_migrate", "group", "pdm_fade", "pdm_carry")
KINDS = M.KINDS + NEW_KINDS
NEW_REQUESTS = ("sub_on", "sub_off")
REQUESTS = M.REQUESTS + NEW_REQUESTS
FORMS = ("process", "pdm", "mixed", "mixed_pdm")
PATTERNS = ("alternating", "random", "all_but_one", "lane_mates", "all16", "all24")
RUNS = 26                   # runs of at most 3 packets that a context makes after its warm-up
TOTAL = WARM + 2 * 3 * RUNS # packets of input per stream: one that migrates plays on in the other context, so it may meet both contexts' runs
SENT = 0x5A5A5A5A


def top(fl):
    """no context grows past this"""
    return 3 * row(fl) + 1


def rows_of(n, R):
    return -(-n // R)


def grow_targets(S, R):
    """from S, test_gpu_resize.grow_sizes's three classes: a size in the same row, the first sizes that open a row (with two streams, with one),
    the first size after that which leaves a row holding one stream"""
    edge = rows_of(S, R) * R
    return [n for n in (min(S + 1 + (edge - S) // 2, edge), edge + 2, edge + 1, edge + R + 1) if n > S]


def migration_pairing(src_paused, dst_paused, want):
    """dspi_plan_migration's documented pairing: the k highest active sources with the k lowest paused destinations, order kept"""
    src, dst = np.flatnonzero(~np.asarray(src_paused, dtype=bool)), np.flatnonzero(np.asarray(dst_paused, dtype=bool))
    k = min(int(want), len(src), len(dst))
    return list(zip(src[len(src) - k:].tolist(), dst[:k].tolist())) if k else []


def depth_vector(rng, pattern, S):
    s = np.arange(S)
    a, b = (16, 24) if rng.random() < 0.5 else (24, 16)
    if pattern == "alternating": v = np.where(s % 2 == 1, a, b)
    elif pattern == "random": v = rng.choice(np.array([16, 24]), S)
    elif pattern == "all_but_one": v = np.where(s == int(rng.integers(0, S)), a, b)
    elif pattern == "lane_mates":      # some lanes hold two depths, in either order; the others one
        v = np.repeat(rng.choice(np.array([16, 24]), (S + 1) // 2), 2)[:S]
        for lane in np.flatnonzero(rng.random(S // 2) < 0.6): v[2 * lane], v[2 * lane + 1] = (a, b) if rng.random() < 0.5 else (b, a)
    else: v = np.full(S, 16 if pattern == "all16" else 24)
    return [int(x) for x in v]


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
class WideGen(M._Gen):
    def __init__(self, rng, fl, sizes_):
        super().__init__(rng, fl, sizes_)
        self.R, self.top = row(fl), top(fl)
        self.cap = [rows_of(S, self.R) for S in self.S]       # rows
        self.fmode = [False] * len(self.S)
        self.left = [3 * RUNS] * len(self.S)                  # packets of input left
        self.host_only = len(self.S) == 1
        self.turn = 0

    # -- runs in four forms
    def run(self, c, spdif=None, form=None, pattern=None):
        r = self.rng
        if self.host_only: return False      # (no audio there)
        n = min(int(r.integers(1, 4)), self.left[c])
        if n == 0: return False
        self.left[c] -= n
        mem = "device" if r.random() < 0.4 else "host"
        tiled, enabled_only, clip, i2s = bool(r.random() < 0.4), bool(r.random() < 0.3), bool(r.random() < 0.7), bool(r.random() < 0.3)
        if spdif is None: spdif = self.mode and r.random() < 0.4
        if form is None: form = str(r.choice(FORMS, p=[0.3, 0.25, 0.25, 0.2]))
        if spdif: tiled = i2s = False      # (the one exclusion the flags have: "Not with DSPI_OUT_TILED or DSPI_OUT_I2S_SLOTS"; it holds for all four calls alike)
        depths = None
        if form in ("mixed", "mixed_pdm"):
            pattern = pattern or str(r.choice(PATTERNS, p=[0.2, 0.25, 0.15, 0.2, 0.1, 0.1]))
            depths = depth_vector(r, pattern, self.S[c])
        self.emit(op="run", ctx=c, n=n, mem=mem, tiled=tiled, enabled_only=enabled_only, clip=clip, i2s=i2s, spdif=bool(spdif), form=form, pattern=pattern if depths else None, depths=depths)
        if self.due[c] > 0:
            self.due[c] -= 1
            if self.due[c] == 0: self.enumerate(c)
        return True

    # -- requests: the sub output on and off
    def request(self, c, stream="draw", kind=None):
        r = self.rng
        if kind in NEW_REQUESTS or (kind is None and r.random() < 0.2):
            if stream == "draw": stream = None if r.random() < 0.4 else int(r.integers(0, self.S[c]))
            kind = kind or str(r.choice(NEW_REQUESTS))
            self.emit(op="request", ctx=c, stream=stream, kind=kind, name=kind, args=()); return True
        return super().request(c, stream, kind)

    # -- snapshots: an import with or without the PDM carry
    def import_(self, c=None, stash=None, to=None, carry=None):
        if not super().import_(c, stash, to): return False
        op = next(o for o in reversed(self.ops) if o["op"] == "import")
        if not self.host_only and (self.rng.random() < 0.5 if carry is None else carry):
            self.emit(op="pdm_carry", ctx=op["ctx"], stash=op["stash"], to=op["to"], count=op["count"])
        return True

    # -- sizes
    def resized(self, c, n, paused=False):
        old = self.S[c]
        self.S[c] = n
        if n > old:
            self.paused[c] = np.concatenate([self.paused[c], np.full(n - old, paused)])
            self.unenum[c] = np.concatenate([self.unenum[c], np.ones(n - old, dtype=bool)])
        else:
            self.paused[c], self.unenum[c] = self.paused[c][:n].copy(), self.unenum[c][:n].copy()

    def grow(self, c, n=None, paused=None, how=None, settle=True):
        """how: "inside" (a reserve first where the capacity is short), "realloc" (the capacity is brought down to the rows in use first where
        it is larger) or None (as it comes)"""
        r, S, R = self.rng, self.S[c], self.R
        cands = [t for t in grow_targets(S, R) if t <= self.top]
        if n is None:
            if not cands: return False
            n = int(r.choice(cands))
        if not S < n <= self.top: return False
        if how == "realloc" and rows_of(n, R) == rows_of(S, R):
            more = [t for t in cands if rows_of(t, R) > rows_of(S, R)]
            if not more: return False
            n = int(r.choice(more))
        if how == "inside" and rows_of(n, R) > self.cap[c]: self.reserve(c, int(r.integers(n, self.top + 1)))
        if how == "realloc" and self.cap[c] > rows_of(S, R): self.reserve(c, S)
        if paused is None: paused = bool(r.random() < 0.35)
        self.resized(c, n, paused)
        self.emit(op="grow", ctx=c, n=n, paused=paused, old=S, realloc=rows_of(n, R) > self.cap[c])
        self.cap[c] = max(self.cap[c], rows_of(n, R))
        if settle:
            if r.random() < 0.5: self.enumerate(c)
            else: self.due[c] = int(r.integers(1, 3))
        return True

    def cuttable(self, c):
        """the lowest n >= 1 with [n, S) paused"""
        n = self.S[c]
        while n > 1 and self.paused[c][n - 1]: n -= 1
        return n

    def shrink(self, c, n=None, by_compaction=None):
        r, S = self.rng, self.S[c]
        if S < 2: return False
        if by_compaction is None: by_compaction = n is None and not self.host_only and r.random() < 0.3
        if by_compaction:      # the header's recipe: a one-way compaction, then the cut to A
            moves = compaction(self.paused[c], True)
            A = int((~self.paused[c]).sum())
            if not 1 <= A < S: return False
            if moves:
                self.apply_moves(c, moves)
                self.emit(op="compact", ctx=c, one_way=True, moves=moves, as_is=bool(r.random() < 0.3))
            n = A
        else:
            if n is None:
                n = int(r.choice([S - 1, max(1, S - int(r.integers(1, 9))), max(1, (S - 1) // self.R * self.R + int(r.integers(0, 3)) - 1), int(r.integers(max(1, S // 2), S))]))
            n = max(1, min(n, S - 1))
            if not self.paused[c][n:].all(): self.pause(c, n, S - n)
        self.resized(c, n)
        self.emit(op="shrink", ctx=c, n=n, old=S); return True

    def reserve(self, c, n=None):
        r, S = self.rng, self.S[c]
        if n is None: n = S if self.cap[c] > rows_of(S, self.R) and r.random() < 0.5 else int(r.integers(S, max(S, self.top) + 1))
        self.cap[c] = rows_of(n, self.R)
        self.emit(op="reserve", ctx=c, n=n, rows=self.cap[c]); return True

    # -- migration
    def free_slots(self, c, k, fresh=None):
        """k distinct paused slots of context c, pausing a range first where it has too few (fresh: do so anyway)"""
        r, S = self.rng, self.S[c]
        k = min(k, S)
        have = np.flatnonzero(self.paused[c])
        if fresh is None: fresh = r.random() < 0.4
        if len(have) < k or fresh:
            first = int(r.integers(0, S - k + 1))
            self.pause(c, first, k)
            have = np.flatnonzero(self.paused[c])
        return [int(v) for v in r.choice(have, k, replace=False)]

    def migrate(self, c, srcs=None, as_is=None, paused=None, fresh=None):
        if self.host_only: return False
        r, t = self.rng, 1 - c
        if srcs is None: srcs = [int(v) for v in r.permutation(self.S[c])[:int(r.integers(1, 7))]]
        dsts = self.free_slots(t, len(srcs), fresh)
        moves = list(zip(srcs, dsts))
        if not moves: return False
        as_is = bool(r.random() < 0.3) if as_is is None else as_is
        paused = bool(r.random() < 0.25) if paused is None else paused
        self.apply_migration(c, moves, paused)
        self.emit(op="migrate", ctx=c, dst=t, moves=moves, as_is=as_is, paused=paused)
        if self.unenum[t].any() and self.due[t] == 0:
            if r.random() < 0.5: self.due[t] = int(r.integers(1, 3))
        return True

    def apply_migration(self, c, moves, paused):
        t = 1 - c
        for s, d in moves:
            self.paused[t][d] = paused or self.paused[c][s]
            self.unenum[t][d] = self.unenum[c][s]
        for s, _ in moves: self.paused[c][s] = True

    def plan_migrate(self, c, want=None):
        """the rebalance of the header: grow the destination paused where it is short, plan, migrate, shrink the source"""
        if self.host_only: return False
        r, t = self.rng, 1 - c
        active = int((~self.paused[c]).sum())
        if active < 3: return False
        want = want or int(r.integers(2, min(active - 1, 12) + 1))
        short = want - int(self.paused[t].sum())
        if short > 0:
            if self.S[t] + short > self.top: want -= short - (self.top - self.S[t]); short = self.top - self.S[t]
            if short > 0: self.grow(t, self.S[t] + short, paused=True, settle=False)
        moves = migration_pairing(self.paused[c], self.paused[t], want)
        if not moves: return False
        as_is = bool(r.random() < 0.3)
        self.apply_migration(c, moves, False)
        self.emit(op="plan_migrate", ctx=c, dst=t, want=want, moves=moves, as_is=as_is, paused=False)
        n = self.cuttable(c)
        if n < self.S[c]: self.shrink(c, n, by_compaction=False)
        if self.unenum[t].any(): self.enumerate(t)
        return True

    # -- grouping: the list is the library's; its postcondition is what the generator goes on with
    def group(self, c):
        if self.unenum[c].any(): self.enumerate(c)      # (the moves are not known here, so nothing that travels may be pending)
        A = int((~self.paused[c]).sum())
        self.paused[c][:A] = False; self.paused[c][A:] = True
        self.emit(op="group", ctx=c, one_way=bool(self.rng.random() < 0.5), as_is=bool(self.rng.random() < 0.3)); return True

    def pdm_fade(self, c, on=None):
        on = (not self.fmode[c]) if on is None else on
        if on == self.fmode[c]: return False
        self.fmode[c] = on
        self.emit(op="pdm_fade", ctx=c, on=on); return True

    # -- motifs of the new ops
    def swap(self, c, a, b):
        moves = [(a, b), (b, a)]
        self.apply_moves(c, moves)
        self.emit(op="move", ctx=c, moves=moves, as_is=bool(self.rng.random() < 0.3))

    def boot_raw(self, c, streams, settle=False):
        r = self.rng
        self.unenum[c][streams] = True
        self.emit(op="boot", ctx=c, streams=streams, dump=bool(r.random() < 0.6), as_is=bool(r.random() < 0.3))
        if settle: self.enumerate(c)

    def follow(self, c, what=None):
        """the call directly after a maintenance op: mixed depths, S/PDIF, or PDM words"""
        r = self.rng
        what = what or str(r.choice(["mixed", "spdif", "pdm", "any"], p=[0.45, 0.3, 0.15, 0.1]))
        if what == "spdif" and self.mode: return self.run(c, spdif=True)
        if what == "pdm": return self.pdm_run(c)
        if what == "any": return self.run(c)
        return self.run(c, form=str(r.choice(["mixed", "mixed_pdm"])), pattern=str(r.choice(["alternating", "random", "all_but_one", "lane_mates"])))

    def pdm_run(self, c):
        return self.run(c, form=str(self.rng.choice(["pdm", "mixed_pdm"])))

    def active_slot(self, c, lo=0):
        a = np.flatnonzero(~self.paused[c][lo:]) + lo
        if not len(a):
            first = int(self.rng.integers(lo, self.S[c]))
            self.resume(c, first, 1)
            return first
        return int(self.rng.choice(a))

    def sub_up(self, c, s=None):
        """the sub on (one stream or all) and a PDM call: the stream's modulator runs"""
        self.request(c, stream=s if self.rng.random() < 0.5 else None, kind="sub_on")
        self.pdm_run(c)

    def a_fade(self, c):
        """a stream of context c whose fade is in flight: the mode on, the sub on, a PDM call, the sub off, a PDM call (1 023 frames to go, less
        the call's).  Returns its slot."""
        if self.unenum[c].any(): self.enumerate(c)
        self.pdm_fade(c, True)
        s = self.active_slot(c)
        self.sub_up(c, s)
        self.request(c, stream=s, kind="sub_off")
        self.pdm_run(c)
        return s

    # the motifs go round, so that a few seeds hold each: (motif, the maintenance call it crosses)
    PLANS = ([(k, None) for k in range(8)] + [(8, w) for w in ("move", "migrate", "import_carry", "import_plain", "boot", "grow")]
             + [(9, w) for w in ("pause", "move", "migrate_on", "migrate_off", "boot", "shrink", "mode_off")]
             + [(10, w) for w in ("move", "migrate", "grow", "boot", "import", "resume", "migrate+spdif", "grow+spdif")])

    def motif(self):
        r = self.rng
        if self.host_only or r.random() < 0.12: return super().motif()
        c = self.ctx()
        S, R = self.S[c], self.R
        Sg = min(S, self.top)      # (a Q28 context may start above 3R + 1; it never grows back past it)
        k, what = self.PLANS[self.turn % len(self.PLANS)]
        self.turn += 1
        if k == 0:      # a grow that reallocates, then a call
            if not self.grow(c, how="realloc"): self.grow(c)
            self.follow(c)
        elif k == 1:    # a grow over columns that a shrink left dirty, the PDM words allocated
            self.sub_up(c)
            if S < 3: return
            n = max(1, Sg - int(r.integers(1, min(Sg, R + 2))))
            self.shrink(c, n, by_compaction=False)
            if r.random() < 0.5: self.run(c)
            self.grow(c, int(r.integers(n + 1, Sg + 1)), paused=False, settle=False)
            self.enumerate(c)
            self.request(c, stream=None, kind="sub_on")
            self.pdm_run(c)
        elif k == 2:    # a grown stream is moved into an older row, then plays
            old = self.S[c]
            if not self.grow(c, paused=False, settle=False): return
            a, b = int(r.integers(old, self.S[c])), int(r.integers(0, old))
            self.swap(c, a, b)
            self.follow(c)
            self.enumerate(c)
        elif k == 3:    # a stash, a resize that reallocates or cuts and regrows its range, then its import
            count = int(r.integers(1, min(5, Sg) + 1)); first = Sg - count - int(r.integers(0, min(3, Sg - count + 1)))
            first = max(0, first)
            self.export(c, first, count)
            stash = len(self.stashes) - 1
            if r.random() < 0.5 and first >= 1:
                self.shrink(c, first, by_compaction=False)
                if r.random() < 0.5: self.run(c)
                self.grow(c, Sg, settle=False); self.enumerate(c)
                if r.random() < 0.4: self.reserve(c, self.S[c])
            elif not self.grow(c, how="realloc"): return
            if r.random() < 0.5: self.run(c)
            self.import_(c=c, stash=stash, to=first)
            self.follow(c)
        elif k == 4:    # a device that no host has set up yet changes its context and is set up there
            t = 1 - c
            if r.random() < 0.5 or not self.grow(c, settle=False): self.boot_raw(c, [int(v) for v in r.permutation(S)[:int(r.integers(1, 4))]])
            srcs = [int(v) for v in np.flatnonzero(self.unenum[c])[:4]]
            self.due[c] = 0
            self.migrate(c, srcs=srcs, paused=False)
            self.due[t] = 0
            if r.random() < 0.5: self.follow(t)
            self.enumerate(t); self.enumerate(c)
            self.run(t)
        elif k == 5:    # a migration, a request to the arrival alone, the copy it left behind resumed
            t = 1 - c
            s = self.active_slot(c)
            if self.unenum[c][s]: self.enumerate(c)
            self.migrate(c, srcs=[s], paused=False)
            d = self.ops[-1]["moves"][0][1]
            self.request(t, stream=d, kind=str(r.choice(["load_bulk", "band", "load_slot", "preamp", "delay", "sub_on"])))
            self.follow(t)
            self.resume(c, s, 1); self.run(c)
        elif k == 6:    # the rebalance
            if not self.plan_migrate(c): return
            self.follow(1 - c); self.follow(c)
        elif k == 7:    # three parameter objects or more, grouped, then a call
            if S < 4: return
            for kind in ("load_bulk", "load_slot", "load_bulk", "preamp", "load_slot"):
                self.request(c, stream=self.active_slot(c), kind=kind)
            if r.random() < 0.4: self.pause(c, *self.range(c, cap=4))
            if r.random() < 0.5: self.follow(c, "mixed")
            self.group(c)
            self.follow(c, "mixed" if r.random() < 0.7 else None)
        elif k == 8:    # PDM words on both sides of a maintenance call
            self.sub_up(c)
            t = c
            if what == "move": ok = self.move(c, must_src=self.active_slot(c))
            elif what == "migrate":
                t = 1 - c
                a = self.active_slot(c)
                ok = self.migrate(c, srcs=[a] + [int(v) for v in r.permutation(S)[:2] if int(v) != a], paused=False)
                if r.random() < 0.5: self.request(t, stream=None, kind="sub_on")
            elif what in ("import_carry", "import_plain"):
                self.export(c, *self.range(c, cap=min(self.S)))
                if r.random() < 0.5: self.pdm_run(c)
                ok = self.import_(stash=len(self.stashes) - 1, carry=what == "import_carry")
                t = next(o for o in reversed(self.ops) if o["op"] == "import")["ctx"] if ok else c
            elif what == "boot":
                self.boot_raw(c, [int(v) for v in r.permutation(S)[:int(r.integers(1, 4))]], settle=True); ok = True
                if r.random() < 0.6: self.request(c, stream=None, kind="sub_on")
            else:
                ok = self.grow(c, settle=False)
                if ok: self.enumerate(c)
                if r.random() < 0.6: self.request(c, stream=None, kind="sub_on")
            self.pdm_run(t)
            if t != c: self.pdm_run(c)
        elif k == 9:    # a fade in flight goes through a maintenance call
            t = c
            if what == "shrink" and S < 3: return
            s = self.a_fade(c) if what != "shrink" else None
            if what == "shrink":      # the fading stream's slot is cut and comes back as a new device
                s = Sg - 1
                self.resume(c, s, 1)
                if self.unenum[c].any(): self.enumerate(c)
                self.pdm_fade(c, True)
                self.sub_up(c, s); self.request(c, stream=s, kind="sub_off"); self.pdm_run(c)
                self.shrink(c, Sg - int(r.integers(1, min(Sg - 1, 4) + 1)), by_compaction=False)
                self.pdm_run(c)
                self.grow(c, Sg, paused=False, settle=False); self.enumerate(c)
            elif what == "pause":
                self.pause(c, s, 1); self.pdm_run(c); self.resume(c, s, 1)
            elif what == "move":
                if not self.move(c, must_src=s): return
            elif what in ("migrate_on", "migrate_off"):
                t = 1 - c
                self.pdm_fade(t, what == "migrate_on")
                self.migrate(c, srcs=[s], paused=False)
            elif what == "boot": self.boot_raw(c, [s], settle=True)
            else: self.pdm_fade(c, False)
            self.pdm_run(t)
            if what == "mode_off": self.pdm_fade(c, True)
            if r.random() < 0.5: self.pdm_run(t)
        else:           # a call in mixed depths directly after a maintenance call
            spdif = what.endswith("+spdif")
            what = what.split("+")[0]
            if spdif: self.spdif_mode()
            t = c
            if what == "move": ok = self.move(c)
            elif what == "migrate": ok = self.migrate(c); t = 1 - c
            elif what == "grow": ok = self.grow(c, settle=False); self.due[c] = 1
            elif what == "boot": self.boot_raw(c, [int(v) for v in r.permutation(S)[:int(r.integers(1, 4))]]); self.due[c] = 1; ok = True
            elif what == "import":
                if not self.stashes: self.export(self.ctx())
                ok = self.import_(c=c if self.stashes[-1][2] <= S else None, stash=len(self.stashes) - 1)
                t = next(o for o in reversed(self.ops) if o["op"] == "import")["ctx"] if ok else c
            else:
                first, count = self.range(c, cap=6)
                self.pause(c, first, count); self.run(c)
                ok = self.resume(c, first, count)
            if ok: self.follow(t, "spdif" if spdif else "mixed")

    def single(self):
        r = self.rng
        if r.random() < 0.45: return super().single()
        kind = str(r.choice(["grow", "shrink", "reserve", "reserve", "migrate", "group", "pdm_fade", "request", "run", "compact", "old_request", "old_request", "old_request", "realign", "image_count", "plan_migrate", "plan_migrate"]))
        c = self.ctx()
        if self.host_only and kind == "migrate": kind = "reserve"
        return {"grow": lambda: self.grow(c), "shrink": lambda: self.shrink(c), "reserve": lambda: self.reserve(c), "migrate": lambda: self.migrate(c),
                "group": lambda: self.group(c), "pdm_fade": lambda: self.pdm_fade(c), "request": lambda: self.request(c, kind=str(r.choice(NEW_REQUESTS))),
                "run": lambda: self.run(c), "compact": lambda: self.compact_something(c), "old_request": lambda: super(WideGen, self).request(c),
                "realign": lambda: self.realign(c), "image_count": lambda: self.image_count(c), "plan_migrate": lambda: self.plan_migrate(c)}[kind]()


def wide_config(seed):
    """a configuration as schedule(seed)'s; flavour, layout, rate and starting size go round with the seed, so that few seeds hold them all"""
    rng = np.random.default_rng(83000 + seed)
    fl = ("f32", "fma", "q28")[(seed + seed // 3) % 3]
    layout = LAYOUTS[(seed // 3) % 3]
    fs, Bs = RATES[seed % 3]
    B = int(rng.choice(Bs)); depth = 16 if rng.random() < 0.5 else 24
    S = sizes(fl)[(seed + seed // 6) % 6]
    flavor = FLAVORS[fl]
    P = 4 if int(flavor) else 2
    blob, blob2 = random_blob(rng, int(flavor), fs), random_blob(rng, int(flavor), fs)
    blob["i2s_config"]["output_types"][1] = 1; blob2["i2s_config"]["output_types"][0] = 1
    for b in (blob, blob2):
        b["outputs"]["enabled"][:P] = 1; b["outputs"]["mute"][:2] = 0; b["crosspoints"]["enabled"][:, :2] = 1
    cfg = dict(seed=seed, flavor=fl, layout=layout, fs=fs, B=B, depth=depth, S=S, side=SIDE, R=row(fl), top=top(fl), blob=blob, blob2=blob2,
               vol=int(rng.choice([0, -5 * 256, -20 * 256])), vol_side=int(rng.choice([0, -9 * 256])), first_stream=int(rng.integers(0, 20)))
    return rng, cfg


def schedule_wide(seed):
    """(config, ops): a pure function of the seed"""
    rng, cfg = wide_config(seed)
    g = WideGen(rng, cfg["flavor"], (cfg["S"], SIDE))
    g.turn = 4 * seed
    warm = dict(n=WARM, mem="host", tiled=False, enabled_only=False, clip=True, i2s=False, spdif=False, form="process", pattern=None, depths=None, warm=True)
    g.emit(op="run", ctx=0, **warm); g.emit(op="run", ctx=1, **warm)
    if rng.random() < 0.55: g.spdif_mode()
    if rng.random() < 0.5: g.pdm_fade(int(rng.integers(0, 2)))
    target = len(g.ops) + int(rng.integers(22, 34))
    # (the weights are tuned against tests/test_lifecycle_wide_cpu.py::test_default_wide_seeds_contain_the_crossings)
    while len(g.ops) < target - 2:
        last = g.ops[-1]
        if g.mode and last["op"] in ("pause", "resume", "move", "boot", "import", "spdif_carry", "grow", "migrate") and rng.random() < 0.35:
            g.run(last["dst"] if last["op"] == "migrate" else last["ctx"], spdif=True)
        elif rng.random() < 0.62: g.motif()
        else: g.single()
    g.due = [0, 0]
    g.run(1); g.run(0)
    return cfg, g.ops


def host_schedule_wide(seed, fl, S, n_ops=50):
    """the wide generator on two host-only contexts of one flavour (context 0: S streams, context 1: SIDE): what such contexts do, and the calls
    they must refuse after validating them (`refused`)"""
    rng = np.random.default_rng(97000 + seed)
    g = WideGen(rng, fl, (S, SIDE))
    g.host_only = True      # (no audio: no runs, no snapshots; migrations are planned and refused)
    while len(g.ops) < n_ops:
        kind = str(rng.choice(["request", "request", "pause", "pause", "resume", "boot", "enumerate", "spdif_mode", "grow", "grow", "shrink", "reserve", "group", "plan",
                               "pdm_fade", "pdm_running", "mixed_bytes", "image_count", "refused", "refused"]))
        c = g.ctx()
        if kind == "request": g.request(c)
        elif kind == "pause": g.pause(c)
        elif kind == "resume": g.resume(c)
        elif kind == "boot": g.boot(c)
        elif kind == "enumerate": g.enumerate(c)
        elif kind == "spdif_mode": g.spdif_mode()
        elif kind == "grow": g.grow(c, how=str(rng.choice(["inside", "realloc", "any"])))
        elif kind == "shrink": g.shrink(c)
        elif kind == "reserve": g.reserve(c)
        elif kind == "group": g.emit(op="plan_group", ctx=c, one_way=bool(rng.random() < 0.5))
        elif kind == "plan": g.emit(op="plan", ctx=c, dst=1 - c, want=int(rng.integers(1, 40)))
        elif kind == "pdm_fade": g.pdm_fade(c)
        elif kind == "pdm_running":
            first, count = g.range(c)
            g.emit(op="pdm_running", ctx=c, first=first, values=[int(v) for v in rng.integers(0, 2, count)])
        elif kind == "mixed_bytes":
            g.emit(op="mixed_bytes", ctx=c, n=int(rng.integers(1, 4)), B=int(rng.choice([1, 44, 45, 48, 96])), depths=depth_vector(rng, str(rng.choice(PATTERNS)), g.S[c]))
        elif kind == "image_count": g.image_count(c)
        else:
            what = str(rng.choice(["migrate", "mixed", "pdm", "fade_state"]))
            moves = []
            if what == "migrate":
                k = int(rng.integers(1, 5))
                moves = list(zip([int(v) for v in rng.permutation(g.S[c])[:k]], g.free_slots(1 - c, k)))[:min(k, g.S[c])]
            if what == "fade_state": g.pdm_fade(c, True)
            first, count = g.range(c)
            g.emit(op="refused", ctx=c, what=what, moves=moves, first=first, count=count, depths=depth_vector(rng, str(rng.choice(PATTERNS)), g.S[c]))
    return g.ops[:n_ops]


def named(ops, final):
    """{context: every slot below the context's final size that an op of the list names}; a group's moves are those the executor noted"""
    out = M.named([op for op in ops if op["op"] in M.KINDS])
    for op in ops:
        k = op["op"]
        s = out.setdefault(op["ctx"], set())
        if k == "grow": s.update((op["old"], op["n"] - 1, op["old"] - 1))
        elif k == "shrink": s.add(op["n"] - 1)
        elif k in ("migrate", "plan_migrate"):
            s.update(a for a, _ in op["moves"]); out.setdefault(op["dst"], set()).update(b for _, b in op["moves"])
        elif k == "group": s.update(v for m in op.get("moves", ()) for v in m)
        elif k == "pdm_carry": s.update(range(op["to"], op["to"] + op["count"]))
    return {c: {v for v in s if 0 <= v < final[c]} for c, s in out.items()}


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def clone(m):
    """a FadeStream of its own with the same modulator words, byte, position and base"""
    n = FadeStream()
    C.memmove(n.o.st, m.o.st, C.sizeof(m.o.st))
    n.running, n.pos, n.base = m.running, m.pos, m.base
    return n


class WideLife(Life):
    """Life whose context changes its size, gives streams to another context and takes theirs, and makes its calls in four forms.  Per-slot
    records are kept for `room` slots from the start (ResizeSched's way).  pools: the input at 16 and 24 bit, one row per stream id;
    self.data[s] is the id of the stream in slot s (it travels as Life's data rows do)."""

    def __init__(self, d, flavor, fs, bases, home, ids, pools, depth, B, room, blob2=None, image=None):
        super().__init__(d, flavor, fs, bases, home, ids, depth, B, blob2=blob2, image=image)
        S = d.n_streams
        self.room, self.pools = room, pools
        self.pos = np.zeros(room, dtype=np.int64)
        self.parts += [[] for _ in range(room - S)]; self.hooks += [dict() for _ in range(room - S)]
        self.home += [home] * (room - S); self.pdm += [[] for _ in range(room - S)]
        self.m = [FadeStream() for _ in range(room)]
        self.fmode = False
        self.cap = rows_of(S, d.tile_streams())               # rows, where the header fixes it
        o = self.fresh(None); self.power_on = o.status(); o.close()
        self.now = dict(form="process", depths=None)          # the call that run() is making
        assert d.stream_capacity() == self.cap * d.tile_streams(), "after dspi_create the capacity is the rows in use"

    # -- requests
    def request(self, name, *args, stream=None, want=0):
        if name == "sub_on": return sub_setup(self, self.flavor, **({} if stream is None else dict(stream=stream)))
        if name == "sub_off": return self.vendor_set(W.REQ["SET_OUTPUT_ENABLE"], self.d.N - 1, b"\x00", **({} if stream is None else dict(stream=stream)))
        return super().request(name, *args, stream=stream, want=want)

    def vendor_set(self, req, wvalue, payload, stream=None):
        """(what sub_setup calls: a recorded request)"""
        super().request("vendor_set", req, wvalue, payload, stream=stream)

    def sub_on(self, s):
        return self.d.vendor_get(W.REQ["GET_CORE1_MODE"], 0, 1, stream=int(s)) == b"\x01"

    # -- the fade model follows what Life follows
    def relocate(self, moves):
        moves = [(int(s), int(d)) for s, d in moves if int(s) != int(d)]
        m = list(self.m)
        dsts = {d for _, d in moves}
        super().relocate(moves)
        for s, d in moves: self.m[d] = m[s]
        for s, _ in moves:
            if s not in dsts: self.m[s] = clone(m[s])      # "an open-end source keeps its value": the frozen copy

    def boot(self, streams, dump=None, as_is=False, want=48):
        super().boot(streams, dump, as_is, want)
        for s in streams: self.m[int(s)] = FadeStream()      # "dspi_boot_streams and new slots of a grow (0)"; "the listed slots go to 0"

    def export(self, first, count):
        st = super().export(first, count)
        d = self.d
        st.update(m=[clone(self.m[s]) for s in range(first, first + count)], running=d.pdm_running(first, count),
                  fade=d.pdm_fade_state(first, count) if self.fmode else None)
        return st

    def import_(self, to, stash, realign=False):
        super().import_(to, stash, realign)
        for k, m in enumerate(stash["m"]):      # "snapshots ... the byte does not travel and an import leaves the slot's byte alone"; "Snapshots are unchanged and carry neither"
            x = clone(m)
            x.running, x.pos, x.base = self.m[to + k].running, self.m[to + k].pos, self.m[to + k].base
            self.m[to + k] = x

    def pdm_carry(self, to, stash):
        """"carry it with dspi_pdm_running, get on the source context, set on the destination"; the fade word likewise where the destination
        keeps one (a source whose mode was off had none: word 0)"""
        d, n = self.d, len(stash["m"])
        assert np.array_equal(d.pdm_running(to, n, set=stash["running"]), stash["running"])
        words = None
        if self.fmode:
            words = stash["fade"] if stash["fade"] is not None else np.zeros(n, dtype=np.uint32)
            assert np.array_equal(d.pdm_fade_state(to, n, set=words), words)
        for k in range(n):
            x = self.m[to + k]
            x.running = int(stash["running"][k])
            if words is not None:
                x.pos = int(words[k]) & 0xFFFF
                x.base = int(np.int16(np.uint16(int(words[k]) >> 16)))

    def pdm_fade(self, on):
        assert self.d.pdm_fade(1 if on else 0) is bool(on)
        if self.fmode and not on:
            for x in self.m: x.stop_now()               # "disabling it ends every fade in flight at once: byte 0, no more words"
        if on and not self.fmode:
            for x in self.m: x.pos, x.base = 0, 0        # "Enabling the mode gives every stream base 0 and 'not fading'"
        self.fmode = bool(on)

    # -- sizes
    def grow(self, n, paused=False):
        d, old, R = self.d, self.d.n_streams, self.d.tile_streams()
        was = d.streams_paused().astype(bool)
        assert d.resize_streams(n, paused=paused) == n == d.n_streams == int(d.L.dspi_num_streams(d.h))
        now = d.streams_paused().astype(bool)
        assert np.array_equal(now[:old], was) and (now[old:] == paused).all(), "old slots keep their activity, new slots are active / arrive paused"
        if rows_of(n, R) > self.cap: self.cap = rows_of(n, R)      # "Past it, new arrays of exactly the rows needed are allocated"
        k = n - old
        self.last_clip = np.concatenate([self.last_clip, np.zeros(k, dtype=np.uint16)])
        self.paused = np.concatenate([self.paused, np.full(k, paused)])
        self.sp = np.concatenate([self.sp, np.zeros(k, dtype=np.int64)])      # "the new slots' positions are 0 and the old slots keep theirs"
        for s in range(old, n):
            self.booted[s] = None
            self.parts[s] = []; self.hooks[s] = {}; self.pos[s] = 0; self.pdm[s] = []
            self.m[s] = FadeStream()
            self.frozen.pop(s, None)
            if paused: self.frozen[s] = (self.power_on, 0)
        for s in sorted({old, n - 1, (old + n) // 2}):
            assert d.status(s) == self.power_on, f"new slot {s}: status bytes are not the power-on ones"

    def shrink(self, n):
        d, old = self.d, self.d.n_streams
        assert self.paused[n:].all(), "the generator left an active slot in the cut range"
        assert d.resize_streams(n) == n == d.n_streams == int(d.L.dspi_num_streams(d.h))
        self.last_clip, self.paused, self.sp = self.last_clip[:n].copy(), self.paused[:n].copy(), self.sp[:n].copy()
        for s in range(n, old):
            self.parts[s] = []; self.hooks[s] = {}; self.pos[s] = 0; self.pdm[s] = []
            self.frozen.pop(s, None); self.booted.pop(s, None)
            self.m[s] = FadeStream()

    def reserve(self, n):
        R = self.d.tile_streams()
        assert self.d.reserve_streams(n) == rows_of(n, R) * R
        self.cap = rows_of(n, R)

    # -- migration: relocate_across, extended by everything Life and this class add per slot
    def migrate_to(self, y, moves, as_is=False, paused=False):
        x = self
        moves = [(int(s), int(d)) for s, d in moves]
        assert x.d.migrate_streams(y.d, moves, as_is=as_is, paused=paused) == len(moves)
        relocate_across(x, y, moves, paused)
        both = x.fmode and y.fmode
        for s, d in moves:
            y.home[d] = x.home[s]; y.pdm[d] = list(x.pdm[s])
            y.booted.pop(d, None)
            if s in x.booted: y.booted[d] = x.booted[s]
            if x.mode: y.sp[d] = x.sp[s]      # "both contexts in per-stream mode: the stream's own position" (the mode is switched on in both at once)
            y.m[d] = x.m[s]; x.m[s] = clone(x.m[s])      # "the arrival takes the source's value (the source slot keeps its own, as a frozen copy)"
            if not both:      # "if either context has the mode off the position arrives as 0, the base is dropped, and a fade in flight has ended as an immediate stop, byte 0"
                y.m[d].stop_now(); y.m[d].pos = y.m[d].base = 0
            y.paused[d] = paused or x.paused[s]
            x.paused[s] = True

    # -- calls
    def row16(self, sid, p0, p1): return packets(self.pools[16][sid], 16, self.B, p0, p1)
    def row24(self, sid, p0, p1): return packets(self.pools[24][sid], 24, self.B, p0, p1)

    def input(self, n):
        d, B = self.d, self.B
        S = d.n_streams
        paused = d.streams_paused().astype(bool)
        depths = self.now["depths"] or [self.depth] * S
        assert len(depths) == S
        runs = []
        for s in range(S):
            if paused[s]: runs.append(self.rng.integers(0, 256, n * B * (6 if depths[s] == 24 else 4), dtype=np.uint8)); continue
            p0 = int(self.pos[s])
            r = self.row16(int(self.data[s]), p0, p0 + n) if depths[s] == 16 else self.row24(int(self.data[s]), p0, p0 + n)
            runs.append(np.ascontiguousarray(r).reshape(-1).view(np.uint8))
        if self.now["depths"] is not None:
            pcm = np.concatenate(runs)
            total, off = d.mixed_pcm_bytes(depths, n, B)
            assert total == pcm.nbytes and int(off[-1]) == total
            return pcm, paused
        pcm = np.stack(runs)
        return (pcm.view(np.int16).reshape(S, n * B, 2) if self.depth == 16 else pcm), paused

    def part_form(self, s):
        dp = self.now["depths"]
        return dict(depth=int(dp[s]) if dp is not None else self.depth, sub_on=self.now["sub_on"][s] if self.now.get("sub_on") is not None else None)

    def fed(self, s, p0, p1, form):
        return (self.row16(int(self.data[s]), p0, p1), 16) if form["depth"] == 16 else (self.row24(int(self.data[s]), p0, p1), 24)

    def at_part(self, o, s, form, at):
        if form["sub_on"] is not None:
            assert (o.vendor_get(W.REQ["GET_CORE1_MODE"], 0, 1) == b"\x01") == form["sub_on"], f"{at}: GET_CORE1_MODE said the sub was {'on' if form['sub_on'] else 'off'}; the replayed oracle says otherwise"

    def lib_call(self, pcm_ptr, n, out, words_ptr, bits):
        """dspi_process_pdm / dspi_process_mixed themselves: "the same flags with the same meanings and refusals" as dspi_process, so every flag
        bit the run drew is passed (dspi_amd.host's wrappers of these two calls pass only some of them)"""
        d, form = self.d, self.now["form"]
        if form == "pdm": rc = d.L.dspi_process_pdm(d.h, pcm_ptr, self.depth, n, self.B, C.byref(out), words_ptr, bits)
        else:
            dp = np.ascontiguousarray(self.now["depths"], dtype=np.uint8)
            assert dp.size == d.n_streams
            rc = d.L.dspi_process_mixed(d.h, pcm_ptr, dp.ctypes.data, n, self.B, C.byref(out), words_ptr, bits)
        assert rc == 0, f"dspi_process_{form}: {rc}: {d.L.dspi_last_error(d.h).decode()}"

    @staticmethod
    def flag_bits(tiled, enabled_only, i2s_slots, spdif, clip):
        return ((H.OUT_TILED if tiled else 0) | (H.OUT_ENABLED_ONLY if enabled_only else 0) | (H.OUT_I2S_SLOTS if i2s_slots else 0)
                | (H.OUT_SPDIF if spdif else 0) | (H.OUT_CLIP_FLAGS if clip else 0))

    def lib_host(self, pcm, n, tiled, enabled_only, i2s_slots, spdif, clip):
        d, B, form = self.d, self.B, self.now["form"]
        S, P, F, R = d.n_streams, d.P, n * B, d.tile_streams()
        if form == "process": return super().lib_host(pcm, n, tiled=tiled, enabled_only=enabled_only, i2s_slots=i2s_slots, spdif=spdif, clip=clip)
        nt = rows_of(S, R)
        pcm = np.ascontiguousarray(pcm)
        pairs = np.zeros((nt, 2 * P, F, R), dtype=np.int32) if tiled else np.zeros((S, P, F, 4), dtype=np.uint32) if spdif else np.zeros((S, P, F, 2), dtype=np.int32)
        sub = np.zeros((nt, F, R) if tiled else (S, F), dtype=np.int32)
        peaks = np.zeros((S, n, d.C), dtype=np.uint16)
        d.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        self.words = np.full((nt, F, 8, R) if tiled else (S, F, 8), SENT, dtype=np.uint32) if form in ("pdm", "mixed_pdm") else None
        out = H._Out(pairs.ctypes.data, sub.ctypes.data, peaks.ctypes.data, d.last_clip.ctypes.data if clip else None)
        self.lib_call(pcm.ctypes.data, n, out, self.words.ctypes.data if self.words is not None else None, self.flag_bits(tiled, enabled_only, i2s_slots, spdif, clip))
        return pairs, sub, peaks

    def lib_device(self, pcm_ptr, n, pairs_ptr, sub_ptr, peaks_ptr, tiled, enabled_only, i2s_slots, spdif, clip_ptr):
        import torch
        d, B, form = self.d, self.B, self.now["form"]
        S, F, R = d.n_streams, n * B, d.tile_streams()
        if form == "process": return super().lib_device(pcm_ptr, n, pairs_ptr, sub_ptr, peaks_ptr, tiled=tiled, enabled_only=enabled_only, i2s_slots=i2s_slots, spdif=spdif, clip_ptr=clip_ptr)
        self.t_words = None
        if form in ("pdm", "mixed_pdm"):
            self.t_words = torch.full((rows_of(S, R), F, 8, R) if tiled else (S, F, 8), SENT, dtype=torch.int32, device=torch.device("cuda", 0))
            torch.cuda.synchronize()
        out = H._Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self.lib_call(pcm_ptr, n, out, self.t_words.data_ptr() if self.t_words is not None else None, H.MEM_DEVICE | self.flag_bits(tiled, enabled_only, i2s_slots, spdif, bool(clip_ptr)))

    def call(self, pcm, n, mem, tiled, enabled_only, clip, i2s, spdif):
        d = self.d
        S, F, R = d.n_streams, n * self.B, d.tile_streams()
        with_words = self.now["form"] in ("pdm", "mixed_pdm")
        if with_words: self.now["sub_on"] = [bool(not self.paused[s] and self.sub_on(s)) for s in range(S)]      # (as the requests stand before the call)
        out = super().call(pcm, n, mem, tiled, enabled_only, clip, i2s, spdif)
        if not with_words: return out
        words = self.t_words.cpu().numpy().view(np.uint32) if mem == "device" else self.words
        unwritten = SENT if mem == "device" else 0
        if tiled:
            flat = words.transpose(0, 3, 1, 2).reshape(-1, F, 8)
            # (host buffers come back as whole tiles out of the library's staging area, as pairs and sub do in Life.call: only device columns keep their value)
            assert (flat[S:] == SENT).all() or mem == "host", "PDM words: columns past the last stream were written"
            words = flat[:S]
        sub = out[1]
        for s in range(S):
            if self.paused[s]:      # "A paused stream is not modulated either ... and its byte is left alone"
                assert (words[s] == unwritten).all(), f"paused stream {s}: its PDM words were written"
                continue
            x = self.m[s]
            was = (x.running, x.pos)
            want = x.call(self.now["sub_on"][s], sub[s], F, self.fmode)
            if want is None: assert (words[s] == unwritten).all(), f"stream {s} is not modulated (byte, fade position before the call: {was}), its PDM words were written"
            elif not np.array_equal(want, words[s]):
                raise AssertionError(f"stream {s} (sub {'on' if self.now['sub_on'][s] else 'off'}; byte, fade position before the call: {was}): PDM words differ from the model's from frame "
                                     f"{int(np.argwhere((want != words[s]).any(axis=1))[0][0])} of {F}")
        return out

    def run(self, n, form="process", depths=None, pattern=None, **kw):
        self.now = dict(form=form, depths=depths, sub_on=None)
        try: return super().run(n, **kw)
        finally: self.now = dict(form="process", depths=None, sub_on=None)

    def modulate(self, tiled=False):
        """dspi_pdm_modulate "runs EVERY active stream's modulator from the stored words" and "neither read[s] nor write[s] the byte" nor the fade
        word: the sub words of the context's last run, repeated or cut to its size of now"""
        # (after DSPI_OUT_ENABLED_ONLY on device buffers a silent sub holds the fill value: the words are only an input, to the library and to the model alike)
        S = self.d.n_streams
        sub = np.ascontiguousarray(self.last_sub[np.arange(S) % len(self.last_sub)])
        words = self.modulated(sub, tiled)
        for s in range(S):
            if self.paused[s]: assert not words[s].any(), f"paused stream {s}: PDM words written"
            else: assert np.array_equal(self.m[s].o.run(sub[s]), words[s]), f"stream {s}: dspi_pdm_modulate's words differ from its modulator's"

    # -- the cheap checks after every op
    def check_books(self, what):
        super().check_books(what)
        d, n = self.d, self.d.n_streams
        assert n == len(self.paused) == int(d.L.dspi_num_streams(d.h)), f"{what}: dspi_num_streams"
        assert d.stream_capacity() == self.cap * d.tile_streams(), f"{what}: dspi_stream_capacity is {d.stream_capacity()}, the header says {self.cap * d.tile_streams()}"
        assert d.pdm_running().tolist() == [x.running for x in self.m[:n]], f"{what}: dspi_pdm_running is not the model's"
        if self.fmode: assert d.pdm_fade_state().tolist() == [x.word() for x in self.m[:n]], f"{what}: dspi_pdm_fade_state is not the model's"


def new_lives_wide(cfg):
    """the two contexts of a configuration, their models and the shared input pools: [main, side]"""
    flavor, fs, B, depth = FLAVORS[cfg["flavor"]], cfg["fs"], cfg["B"], cfg["depth"]
    bases = [(cfg["blob"], cfg["vol"]), (cfg["blob2"], cfg["vol_side"])]
    image = M.preset_image(flavor, fs)
    room = max(cfg["top"], cfg["S"])      # (a Q28 context may start above 3R + 1)
    p16 = WL.synth_pcm16(2 * room, TOTAL * B, fs, first_stream=cfg["first_stream"])
    pools = {16: p16, 24: WL.pcm16_to_pcm24_bytes(p16, seed=1000 + cfg["seed"])}
    lives = []
    for home, S in enumerate((cfg["S"], cfg["side"])):
        ids = np.arange(home * room, (home + 1) * room, dtype=np.int64)
        lives.append(WideLife(context(flavor, S, fs, *bases[home]), flavor, fs, bases, home, ids, pools, depth, B, room, blob2=cfg["blob2"], image=image))
    return lives


def plan_moves(d, one_way):
    return [tuple(int(v) for v in m) for m in np.asarray(d.plan_grouping(one_way)).reshape(-1, 2).tolist()]


def group(x, one_way, as_is=False, what=""):
    """dspi_plan_grouping and dspi_move_streams on its list; what the header promises and a caller can see; returns the list"""
    moves = plan_moves(x.d, one_way)
    if moves: x.move(moves, as_is)      # "dspi_move_streams accepts the list in both modes"
    A = int((~x.paused).sum())
    got = x.d.streams_paused().astype(bool)
    assert not got[:A].any() and got[A:].all(), f"{what}: after the grouping move slots [0, {A}) are not the active ones"
    assert plan_moves(x.d, one_way) == [], f"{what}: planning again on the result does not return 0"
    return moves


def wide_step(op, lives, stashes, what):
    """lifecycle_model.execute's executor for the new kinds"""
    x, k = lives[op["ctx"]], op["op"]
    if k == "grow":
        realloc = rows_of(op["n"], x.d.tile_streams()) > x.cap
        assert realloc == op["realloc"], f"{what}: the generator's capacity is not the model's"
        x.grow(op["n"], op["paused"])
    elif k == "shrink": x.shrink(op["n"])
    elif k == "reserve": x.reserve(op["n"])
    elif k in ("migrate", "plan_migrate"):
        y = lives[op["dst"]]
        if k == "plan_migrate":
            plan = [tuple(m) for m in np.asarray(x.d.plan_migration(y.d, op["want"])).reshape(-1, 2).tolist()]
            assert plan == migration_pairing(x.paused, y.paused, op["want"]) == [tuple(m) for m in op["moves"]], f"{what}: dspi_plan_migration is not the documented pairing"
        x.migrate_to(y, op["moves"], op["as_is"], op["paused"])
    elif k == "group": op["moves"] = group(x, op["one_way"], op["as_is"], what)
    elif k == "pdm_fade": x.pdm_fade(op["on"])
    elif k == "pdm_carry": x.pdm_carry(op["to"], stashes[op["stash"]])
    else: return False
    return True


def execute_wide(cfg, ops, lives, stashes=None):
    return M.execute(cfg, ops, lives, stashes, step=wide_step)


def describe(cfg, ops):
    def tag(op):
        t = op["op"] + ("*" if op["ctx"] else "")
        if op["op"] == "run" and op["form"] != "process": t += ":" + op["form"]
        if op["op"] == "request" and op["kind"] in NEW_REQUESTS: t += ":" + op["kind"]
        return t
    return (f"wide lifecycle fuzz seed {cfg['seed']}: flavor {cfg['flavor']} layout {cfg['layout']} fs {cfg['fs']} B {cfg['B']} depth {cfg['depth']} S {cfg['S']} + {cfg['side']}, "
            f"ops: {' '.join(tag(op) for op in ops)}")
