"""The reference leg of the parity tests.  TEST INFRASTRUCTURE ONLY.

The GPU tests compare the HIP chain with A, the restatement (oracle/liborc_*.so) under the firmware's saturating float->int casts.  The
same hands wrote the kernels and the restatement, so a misreading both share passes.  oracle/_ref/libref_{f32,f32_fma,q28}.so are the
reference's own leaf sources compiled unmodified; an x86 build of them casts the x86 way, so for one checked stream the leg runs

    A = Oracle(flavor)                              what the test compares the GPU with, as before
    X = Oracle(flavor, x86_casts=True)              the restatement casting as the reference build does
    R = Oracle(flavor, ref=True, x86_casts=True)    the reference leaf build (the fma build for wire.F32_FMA)

in lockstep — the same setup, the same requests, the same packets, state carried across calls — and asserts

    X == R    always: every pair word, sub word, peak, clip flag and status byte, and every return code on the way;
    GPU == R  directly, wherever A == X held for that stream so far (no cast overflowed: the x86 build is then a valid checker of the
              firmware's words).  Nothing is deduced through A.

Where A != X a cast overflowed (the x86 conversion gives INT_MIN where the firmware saturates; the Q28 limiter does that on quiet samples,
leveller.c:366-383): the stream is left out of the direct assertion from then on, for good, and counted (`shares()`).  Without oracle/_ref
the leg is left out quietly; tests/test_gpu_parity.py::test_reference_leg_present is the test that fails then."""
from __future__ import annotations

import contextlib
import os

import numpy as np

import orclib
from orclib import Oracle

LEAF_LIBS = ("libref_f32.so", "libref_f32_fma.so", "libref_q28.so")

# methods that change (or may change) a device's state: forwarded to X and R, whose answers must agree
_LOCKSTEP = ("set_rate", "set_volume", "set_mute", "factory_defaults", "load_bulk", "load_slot", "load_flash_dump", "vendor_set", "vendor_get")

_counts: dict = {}      # test function -> [checks held, checks left out]
_notes: list = []       # (test function, stream label, where A and X first differed) of every stream that was left out
_named: list = []       # scope() in force


def available(flavor) -> bool:
    return orclib.ref_available(int(flavor), "ref", bool(getattr(flavor, "fma", False)))


def missing_libs():
    return [n for n in LEAF_LIBS if not (orclib.ORC_DIR / "_ref" / n).exists()]


def lib_name(flavor) -> str:
    return "oracle/_ref/" + orclib._ref_path(int(flavor), "ref", bool(getattr(flavor, "fma", False))).name


@contextlib.contextmanager
def scope(name: str):
    """count under this name (the CPU replay names the GPU test function it replays) instead of the running test's"""
    _named.append(name)
    try: yield
    finally: _named.pop()


def _scope() -> str:
    """the running test function, without its parameters"""
    if _named: return _named[-1]
    cur = os.environ.get("PYTEST_CURRENT_TEST", "")
    return cur.split(" ")[0].split("::")[-1].split("[")[0] or "?"


def _count(held: bool):
    _counts.setdefault(_scope(), [0, 0])[0 if held else 1] += 1


def shares() -> dict:
    """{test function: (checks held, checks left out)} of this process so far; a check is one stream over one process() call"""
    return {k: tuple(v) for k, v in _counts.items()}


def left_out() -> list:
    """(test function, stream label, the first words in which the saturating and the x86 casts differed) of every stream left out so far"""
    return list(_notes)


def _same(a, b) -> bool:
    """two process() results: (pairs, sub, peaks, clip)"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def _where(a, b) -> str:
    for name, x, y in zip(("pairs", "sub", "peaks"), a, b):
        if not np.array_equal(x, y): return f"{name} at {np.argwhere(x != y)[:3].tolist()}"
    return f"clip flags {a[3]:#x} / {b[3]:#x}"


class Leg:
    """A with X and R in lockstep: stands where a test had `Oracle(flavor, detmath=True)` and answers as A does.

    process() returns A's result and keeps R's; the test asserts GPU == A as it always did and then calls `hold()` with the GPU's words
    of the same call.  `held` says whether this stream can still be asserted directly."""

    def __init__(self, flavor, label: str = ""):
        self.a = Oracle(flavor, detmath=True)
        self.flavor, self.label = flavor, label
        self.on = available(flavor)
        self.held = self.on
        self.last = None                    # (R's process() result, R's status after it, A == X for this stream so far)
        if self.on:
            self.x = Oracle(flavor, detmath=True, x86_casts=True)
            self.r = Oracle(flavor, ref=True, detmath=True, x86_casts=True)

    def __getattr__(self, name):
        a = self.__dict__["a"]
        if name not in _LOCKSTEP or not self.__dict__.get("on"):
            return getattr(a, name)

        def call(*args, **kw):
            ra = getattr(a, name)(*args, **kw)
            rx = getattr(self.x, name)(*args, **kw)
            rr = getattr(self.r, name)(*args, **kw)
            assert rx == rr, f"{name}{args[:2]}: the restatement answers {rx!r}, {lib_name(self.flavor)} {rr!r} {self.label}"
            return ra
        return call

    def process(self, pcm, n_blocks, block_len, bit_depth=16, want_peaks=True):
        ra = self.a.process(pcm, n_blocks, block_len, bit_depth, want_peaks)
        if self.on:
            rx = self.x.process(pcm, n_blocks, block_len, bit_depth, want_peaks)
            rr = self.r.process(pcm, n_blocks, block_len, bit_depth, want_peaks)
            sx, sr = self.x.status(), self.r.status()
            assert _same(rx, rr), f"the restatement differs from {lib_name(self.flavor)} {self.label}: {_where(rx, rr)}"
            assert sx == sr, f"status: the restatement differs from {lib_name(self.flavor)} {self.label}"
            if self.held and not (_same(ra, rx) and self.a.status() == sx):
                self.held = False
                _notes.append((_scope(), self.label, _where(ra, rx) if not _same(ra, rx) else "status"))
            self.last = (rr, sr, self.held)
            _count(self.held)
        return ra

    def status(self) -> bytes:
        if self.on: assert self.x.status() == self.r.status(), f"status: the restatement differs from {lib_name(self.flavor)} {self.label}"
        return self.a.status()

    def hold(self, pairs=None, sub=None, peaks=None, status=None, clip=None, what: str = "", last=None, since=(0, 0)):
        """The GPU's words of the call that process() ran last (None: not requested from the GPU) against R's, where the stream is held.
        `last`: a kept `self.last` of an earlier call instead.  since = (frame, packet): the GPU's words are the end of that call, from
        there on (a test that fetched its last launch only)."""
        rr, sr, held = last if last is not None else (self.last or (None, None, False))
        if not held: return False
        rr = (rr[0][:, since[0]:], rr[1][since[0]:], rr[2][since[1]:], rr[3])
        lib = f"{lib_name(self.flavor)} {self.label} {what}"
        if pairs is not None: assert np.array_equal(rr[0], pairs), f"pairs differ from {lib}: {np.argwhere(rr[0] != pairs)[:3].tolist()}"
        if sub is not None: assert np.array_equal(rr[1], sub), f"sub differs from {lib}: {np.argwhere(rr[1] != sub)[:3].tolist()}"
        if peaks is not None: assert np.array_equal(rr[2], peaks), f"peaks differ from {lib}: {np.argwhere(rr[2] != peaks)[:3].tolist()}"
        if clip is not None: assert int(clip) == rr[3], f"clip flags differ from {lib}: {int(clip):#x} / {rr[3]:#x}"
        if status is not None: assert status == sr, f"status differs from {lib}"
        return True

    def close(self):
        self.a.close()
        if self.on: self.x.close(); self.r.close()
