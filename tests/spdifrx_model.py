"""The S/PDIF receiver of include/dspi.h ("S/PDIF input") as a sequential model, frame by frame, in plain Python integers: what the CPU
receiver (dspi_amd/csrc/dspi_spdifrx.cpp) and the kernel (dspi_spdifrx.hip) are held to bit for bit.  Also: the test inputs (the reference's
own encoder where oracle/_ref exists, else the restatement tests/test_oracle_spdif.py pins to it) and the corruptions the tests apply."""
import numpy as np

import orclib

Z, X, Y = 0x39, 0xC9, 0x69
RATES = {0x00: 44100, 0x02: 48000, 0x08: 88200, 0x0A: 96000, 0x0C: 176400, 0x0E: 192000}
# the record as numpy sees it: 40 bytes, include/dspi.h dspi_spdif_rx
RX = np.dtype([("state", "<u4"), ("sample_rate", "<u4"), ("parity_err_count", "<u4"), ("c_bits", "u1", (5,)), ("pad_", "u1", (3,)), ("hold", "<i4", (2,)),
               ("sync", "<u4"), ("held", "<u4"), ("coding_errors", "<u4")])
assert RX.itemsize == 40


def new_rx() -> dict:
    """a receiver just started: all zero"""
    return dict(state=0, sample_rate=0, parity_err_count=0, c_bits=[0] * 5, hold=[0, 0], sync=0, held=0, coding_errors=0)


def to_record(rx: dict) -> np.ndarray:
    r = np.zeros((), dtype=RX)
    for k in ("state", "sample_rate", "parity_err_count", "sync", "held", "coding_errors"): r[k] = rx[k] & 0xffffffff
    r["c_bits"] = rx["c_bits"]; r["hold"] = rx["hold"]
    return r


def records(rxs) -> np.ndarray:
    return np.array([to_record(r) for r in rxs], dtype=RX)


def data_cells(l: int, h: int) -> int:
    """the data cell of slot k at bit k: cells = h:l, slot k's data cell is bit 2k + 1"""
    cells = h << 32 | l
    return sum((cells >> (2 * k + 1) & 1) << k for k in range(32))


def well_formed(l: int, h: int, side: int) -> bool:
    pre = l & 0xff
    return (pre in (Z, X) if side == 0 else pre == Y) and (l & 0x55555500) == 0x55555500 and (h & 0x55555555) == 0x55555555


def receive(rx: dict, words) -> np.ndarray:
    """frames uint32 [n][4] through the record rx (updated in place) -> pairs int32 [n][2]"""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 4)
    out = np.zeros((len(words), 2), dtype=np.int32)
    any_ok = False

    def lose():
        rx["sync"] = 0; rx["sample_rate"] = 0

    for f, w in enumerate(words.tolist()):
        sub = ((w[0], w[1]), (w[2], w[3]))
        ok = [well_formed(*sub[0], 0), well_formed(*sub[1], 1)]
        data = [data_cells(*sub[0]), data_cells(*sub[1])]
        any_ok = any_ok or ok[0] or ok[1]
        # 1. sync
        if ok[0] and sub[0][0] & 0xff == Z:
            if rx["sync"] != 1: rx["parity_err_count"] = 0
            rx["sync"] = 1
        elif ok[0] and rx["sync"] == 1: lose()
        elif not ok[0]: lose()
        if not ok[1]: lose()
        # 2. each side
        for side in (0, 1):
            d = data[side]
            if not ok[side]:
                rx["coding_errors"] = (rx["coding_errors"] + 1) & 0xffffffff
                out[f, side] = rx["hold"][side]; rx["held"] = (rx["held"] + 1) & 0xffffffff
                continue
            if bin(d >> 4).count("1") & 1: rx["parity_err_count"] = (rx["parity_err_count"] + 1) & 0xffffffff
            if d >> 28 & 1:
                out[f, side] = rx["hold"][side]; rx["held"] = (rx["held"] + 1) & 0xffffffff
            else:
                s = d >> 4 & 0xffffff
                s -= (s & 0x800000) << 1
                out[f, side] = rx["hold"][side] = s
        # 3. the channel status
        if rx["sync"]:
            p = rx["sync"] - 1
            if p < 40: rx["c_bits"][p // 8] = (rx["c_bits"][p // 8] & ~(1 << p % 8)) | (data[0] >> 30 & 1) << p % 8
            if p == 31: rx["sample_rate"] = RATES.get(rx["c_bits"][3], 0)
            rx["sync"] = 1 + (p + 1) % 192
    rx["state"] = 2 if rx["sync"] else 1 if any_ok else 0
    return out


def pack24(pairs: np.ndarray) -> np.ndarray:
    """int32 [n][2] -> the 6 n bytes of 24-bit little-endian PCM"""
    u = np.asarray(pairs, dtype=np.int32).reshape(-1).astype(np.uint32)
    return np.stack([u & 0xff, u >> 8 & 0xff, u >> 16 & 0xff], axis=-1).astype(np.uint8).reshape(-1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def encode(pairs: np.ndarray, pos: int, fs: int) -> np.ndarray:
    """int32 [n][2] from block position pos at rate fs -> uint32 [n][4]: the reference's encoder where it is built, else its restatement"""
    words, _ = orclib.spdif_encode(np.ascontiguousarray(pairs, dtype=np.int32), pos, fs, ref=orclib.spdif_ref_available())
    return words


def random_pairs(rng, n: int) -> np.ndarray:
    return rng.integers(-(1 << 23), 1 << 23, (n, 2), dtype=np.int64).astype(np.int32)


# ---- corruptions, applied to encoded words in place ([n][4]; side 0 = left) ------------------------------------------------------------------
def flip_data_cell(words, f: int, side: int, slot: int):
    """flips the data cell of `slot` (4..31): one flip is a parity error"""
    bit = 2 * slot + 1
    words[f, 2 * side + (bit >> 5)] ^= np.uint32(1 << (bit & 31))


def set_v(words, f: int, side: int, keep_parity: bool = True):
    """sets V (slot 28); flips P (slot 31) with it unless a parity error is wanted"""
    if data_cells(int(words[f, 2 * side]), int(words[f, 2 * side + 1])) >> 28 & 1: return
    flip_data_cell(words, f, side, 28)
    if keep_parity: flip_data_cell(words, f, side, 31)


def clear_clock_cell(words, f: int, side: int, slot: int):
    bit = 2 * slot
    words[f, 2 * side + (bit >> 5)] &= np.uint32(~(1 << (bit & 31)) & 0xffffffff)


def set_preamble(words, f: int, side: int, pre: int):
    words[f, 2 * side] = (words[f, 2 * side] & np.uint32(0xffffff00)) | np.uint32(pre)
