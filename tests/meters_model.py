"""The meter bridge as include/dspi.h states it ("the meter bridge"), in numpy and plain Python: the update rule over a call's peaks, the alarm
list, the status block.  Written from the header's prose, not from the C++ or the kernels: the tests hold both against it."""
import numpy as np


def update(meters, peaks, hold_packets, decay_q15, active=None):
    """meters uint32 [S][C] (level | count << 16), peaks uint16 [S][K][C]; returns the new meters.  active: bool [S] or None = every stream;
    a paused stream's words stay as they are.  Vectorised over (stream, channel), sequential over the packets."""
    meters = np.asarray(meters, dtype=np.uint32)
    S, K, C = peaks.shape
    assert meters.shape == (S, C) and 0 <= hold_packets <= 65535 and 0 <= decay_q15 <= 32768
    level = (meters & 0xffff).astype(np.int64)
    count = (meters >> 16).astype(np.int64)
    for k in range(K):
        p = peaks[:, k, :].astype(np.int64)
        up = p >= level
        held = ~up & (count > 0)
        fall = ~up & ~held
        decayed = np.maximum(p, ((level * decay_q15) & 0xffffffff) >> 15)
        level = np.where(up, p, np.where(fall, decayed, level))
        count = np.where(up, hold_packets, np.where(held, count - 1, count))
    out = (level | count << 16).astype(np.uint32)
    if active is not None:
        out = np.where(np.asarray(active, dtype=bool)[:, None], out, meters)
    return out


def update_scalar(word, peaks, hold_packets, decay_q15):
    """one meter word through a sequence of peaks, the rule written out (the vectorised form above is checked against it)"""
    level, count = word & 0xffff, word >> 16
    for p in peaks:
        p = int(p)
        if p >= level:
            level, count = p, hold_packets
        elif count > 0:
            count -= 1
        else:
            level = max(p, ((level * decay_q15) & 0xffffffff) >> 15)
    return level | count << 16


def alarms(meters, clip, level_q15, cap):
    """meters uint32 [S][C] or None, clip uint16 [S] -> (streams [min(total, cap)], info, total): ascending; info = mask of the channels at or above
    the level | clip << 16"""
    clip = np.asarray(clip, dtype=np.uint32)
    S = len(clip)
    mask = np.zeros(S, dtype=np.uint32)
    if meters is not None:
        over = (np.asarray(meters, dtype=np.uint32) & 0xffff) >= level_q15
        for c in range(over.shape[1]): mask |= over[:, c].astype(np.uint32) << np.uint32(c)
    hit = (clip != 0) | (mask != 0)
    streams = np.nonzero(hit)[0].astype(np.uint32)
    info = (mask | clip << np.uint32(16))[streams].astype(np.uint32)
    return streams[:cap], info[:cap], len(streams)


def status_block(peaks, clip):
    """REQ_GET_STATUS wValue 9 of one stream: peaks[C] LE u16, two CPU-load bytes (0), clip LE u16"""
    return np.asarray(peaks, dtype="<u2").tobytes() + b"\0\0" + int(clip).to_bytes(2, "little")
