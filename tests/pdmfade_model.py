"""The model of dspi_pdm_fade (include/dspi.h): one PdmOracle (tests/orclib.py) per stream plus the rule.

During the fade the firmware runs the loop body of a normal sample with target = v + 32768, v = (base * pos) >> 10
(pdm_generator.c:326-327, :366-397).  |base| <= 29500, so |v| <= 29500, and a fade sample is exactly the normal sample v << 14 seen by a
modulator whose fade-in is complete: >> 14 returns v and the limiter passes it.  So the model needs no modulator of its own:
  a fade frame        run([v << 14]) with the state's ninth word (the fade-in position) saved, held at 1024, and restored
  a cancel            that word := 1024 - pos
  the end of a fade   byte 0; restart() at the next enable (the RNG where the fade left it)
The base is computed from the `sub` words the caller hands in — the ones the call under test returned."""
import numpy as np

from orclib import PdmOracle

CLIP, FULL, FADE_IN_WORD = 29500, 1024, 8


def pcm_of(sub_word: int, fade_in: int) -> int:
    """pdm_generator.c:352-362: the limiter, then the fade-in scaling at position fade_in"""
    v = max(-CLIP, min(CLIP, int(sub_word) >> 14))
    return (v * fade_in) >> 10 if fade_in < FULL else v


def fade_samples(base: int, pos: int, n: int) -> np.ndarray:
    """the n synthetic samples of a fade that stands at `pos`: positions pos-1, pos-2, ... (n <= pos - 1)"""
    p = np.arange(pos - 1, pos - 1 - n, -1, dtype=np.int64)
    return (((base * p) >> 10) << 14).astype(np.int32)


class FadeStream:
    """one stream: its modulator, running byte, fade position and base"""

    def __init__(self):
        self.o, self.running, self.pos, self.base = PdmOracle(), 0, 0, 0

    def call(self, sub_on: bool, sub, frames: int, mode: bool = True):
        """one successful dspi_process_pdm call for an ACTIVE stream; returns its words uint32 [frames][8], or None where it is not modulated"""
        if not mode:
            if not sub_on: self.running = 0; return None
            if not self.running: self.o.restart(); self.running = 1
            return self.o.run(sub)
        if not sub_on:
            if not self.running: return None
            if not self.pos: self.pos = FULL
            n = min(frames, self.pos - 1)
            words = np.zeros((frames, 8), dtype=np.uint32)
            held = self.o.st[FADE_IN_WORD]
            self.o.st[FADE_IN_WORD] = FULL
            if n: words[:n] = self.o.run(fade_samples(self.base, self.pos, n))
            self.o.st[FADE_IN_WORD] = held
            self.pos -= n
            if self.pos == 1: self.pos, self.running = 0, 0
            return words
        if self.pos and self.running:      # cancel: no reset, state carried
            self.o.st[FADE_IN_WORD] = FULL - self.pos
        self.pos = 0
        if not self.running: self.o.restart(); self.running = 1
        met = min(int(self.o.st[FADE_IN_WORD]) + frames - 1, FULL)      # the fade-in position the last frame meets
        words = self.o.run(sub)
        self.base = pcm_of(sub[frames - 1], met)
        return words

    def stop_now(self):
        """the mode goes off, or the stream arrives where the mode is off: a fade in flight ends at once"""
        if self.pos: self.pos, self.running = 0, 0

    def word(self) -> int:
        """dspi_pdm_fade_state's word"""
        return self.pos | ((self.base & 0xFFFF) << 16)
