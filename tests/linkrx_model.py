"""Chained devices (include/dspi.h: dspi_wire_decode, dspi_process_linked) as a model in plain Python: where the words of a link lie, written
from the header's prose as four index formulas, the S/PDIF receiver of tests/spdifrx_model.py for an S/PDIF link and `>> 8` for an I2S link.
What dspi_amd/csrc/dspi_link.cpp (the CPU reader) and dspi_linkrx.hip (the kernels) are held to bit for bit.

Also the test buffers: `lay` writes lines into the two wire layouts the PRODUCER's way (by the shape of the regions, include/dspi.h "THE WIRE
LAYOUT" / "THE TILED WIRE LAYOUT"), so that the reader's formulas and the buffers they read are two statements of the layout, not one."""
import numpy as np

import spdifrx_model as M

NONE, SPDIF, I2S = 0, 1, 2
LINK = np.dtype([("line", "<u4"), ("kind", "<u4")])
GARBAGE = 0xDEADBEEF      # what no producer writes: I2S tails, the columns behind the last stream


# ---- the reader: the header's "THE WORDS OF A LINK" -------------------------------------------------------------------------------------------
def link_words(wire, P: int, R: int, F: int, line: int, kind: int) -> np.ndarray:
    """the words of one link, gathered from the flat uint32 buffer: S/PDIF uint32 [F][4], I2S uint32 [F][2]"""
    s, p = divmod(line, P)
    f = np.arange(F, dtype=np.int64)[:, None]
    if kind == SPDIF:
        j = np.arange(4, dtype=np.int64)[None, :]
        at = (line * F) * 4 + f * 4 + j if R == 0 else ((s // R * P + p) * F) * 4 * R + (f * 4 + j) * R + s % R
    else:
        k = np.arange(2, dtype=np.int64)[None, :]
        at = (line * F) * 4 + f * 2 + k if R == 0 else ((s // R * P + p) * F) * 4 * R + (k * F + f) * R + s % R
    return wire[at]


def decode(wire, P: int, R: int, F: int, line: int, kind: int, rx: dict | None) -> np.ndarray:
    """one link -> pairs int32 [F][2]; an S/PDIF link goes through the record rx (updated in place), an I2S link has none"""
    w = link_words(wire, P, R, F, line, kind)
    if kind == SPDIF: return M.receive(rx, w)
    return (w.astype(np.uint32).view(np.int32) >> 8).astype(np.int32)      # arithmetic: numpy shifts int32 that way


# ---- the buffers: the producer's side -------------------------------------------------------------------------------------------------------------
def words_of(S: int, P: int, R: int, F: int) -> int:
    return S * P * F * 4 if R == 0 else -(-S // R) * P * F * 4 * R


def lay(lines: dict, S: int, P: int, R: int, F: int) -> np.ndarray:
    """lines: {line: uint32 [F][4] (an S/PDIF slot) or uint32 [F][2] (an I2S slot)} -> the flat buffer; what no line writes holds GARBAGE"""
    wire = np.full(words_of(S, P, R, F), GARBAGE, dtype=np.uint32)
    if R == 0: regions = wire.reshape(S, P, 4 * F)
    else: tiles = wire.reshape(-(-S // R), P, 4 * F, R)
    for line, w in lines.items():
        s, p = divmod(line, P)
        w = np.asarray(w, dtype=np.uint32)
        assert w.shape in ((F, 4), (F, 2)) and s < S, (line, w.shape)
        if R == 0: regions[s, p, :w.size] = w.reshape(-1)                                  # [F][4], or [F][2] in the first half
        elif w.shape[1] == 4: tiles[s // R, p, :, s % R] = w.reshape(-1)                   # rows f * 4 + j
        else: tiles[s // R, p, :2 * F, s % R] = w.T.reshape(-1)                            # rows side * F + f
    return wire


def corrupt(w, kind: int, pos: int):
    """an S/PDIF line (from block position pos) with one family of trouble, by kind % 6; every index fits 135 frames"""
    F = len(w)
    kind %= 6
    if kind == 1:      # V, with and without its parity, and a run across a 64-frame boundary
        M.set_v(w, 0, 0); M.set_v(w, 5, 1, keep_parity=False)
        for f in range(62, 67): M.set_v(w, f, f & 1)
    elif kind == 2:      # flipped data cells (parity errors, one of them a C bit), cleared clock cells
        M.flip_data_cell(w, 20, 0, 9); M.flip_data_cell(w, 21, 1, 27); M.flip_data_cell(w, 100, 0, 30)
        M.clear_clock_cell(w, 40, 0, 12); M.clear_clock_cell(w, 90, 1, 31)
    elif kind == 3:      # bad preambles on either side, a misplaced Z (re-lock), Z twice
        M.set_preamble(w, 30, 0, M.Z); M.set_preamble(w, 70, 1, M.X); M.set_preamble(w, 71, 0, M.Y); M.set_preamble(w, 72, 0, 0x00)
        M.set_preamble(w, 110, 0, M.Z); M.set_preamble(w, 111, 0, M.Z)
    elif kind == 4:      # X where Z belongs: the lock is lost where the block starts; zero frames
        z = (192 - pos) % 192
        if z < F: M.set_preamble(w, z, 0, M.X)
        w[120:123] = 0
    elif kind == 5: w[:] = 0      # no signal at all
    return w


def build(S: int, P: int, F: int, seed: int):
    """every line of S streams x P pairs, F frames: types by (s + p) % 2 (1: an I2S slot), every S/PDIF line corrupted by its own kind.
    -> (lines {line: words}, kinds uint32 [S * P])"""
    rng = np.random.default_rng(seed)
    lines, kinds = {}, np.zeros(S * P, dtype=np.uint32)
    for line in range(S * P):
        s, p = divmod(line, P)
        pairs = M.random_pairs(rng, F)
        if (s + p) % 2:
            kinds[line] = I2S
            lines[line] = (pairs.astype(np.uint32) << 8) | np.uint32(line & 0xff)      # (the low byte is the reader's to ignore)
        else:
            kinds[line] = SPDIF
            pos = (37 * line) % 192
            lines[line] = corrupt(M.encode(pairs, pos, (44100, 48000, 96000)[line % 3]), line // 2, pos)
    return lines, kinds


def link_orders(kinds: np.ndarray) -> dict:
    """the link lists of the tests: identity, reversed, every line named twice, and holes"""
    n = len(kinds)
    def of(order, holes=False):
        l = np.zeros(len(order), dtype=LINK)
        l["line"] = order; l["kind"] = kinds[order]
        if holes:
            l["kind"][::3] = NONE
            l["line"][::6] = 0xffffffff      # (a hole's line means nothing)
        return l
    ident = np.arange(n)
    return {"identity": of(ident), "reversed": of(ident[::-1]), "twice": of(np.repeat(ident, 2)), "holes": of(ident, True)}
