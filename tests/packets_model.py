"""The packet table (include/dspi.h: dspi_process_packets, dspi_packets_check) as a model in plain Python, written from the header's prose: when
an entry is legal, what a table is refused for and in which order, with the index of the first entry refused, and what an accepted table
describes — every stream's packets gathered and widened into the input of the dspi_process_mixed call that the call IS."""
import numpy as np

MAX_BLOCK_LEN = 192      # DSPI_MAX_BLOCK_LEN
MAX_ENTRIES = 2 ** 31 - 1


def frame_bytes(depth):
    return {16: 4, 24: 6}[depth]


def entry_ok(offset, depth, block_len, arena_bytes):
    """AN ENTRY IS LEGAL when it is even and offset + block_len * frame bytes <= arena_bytes"""
    return offset % 2 == 0 and offset + block_len * frame_bytes(depth) <= arena_bytes


def check(depths, table, n_blocks, block_len, arena_bytes, active=None, max_block_len=MAX_BLOCK_LEN):
    """refusals 2 to 5 behind the pointers: None, or ("lengths",), ("depth", s), ("overflow",), ("entry", s * n_blocks + k).  table: rows of
    n_blocks offsets, looked at only when the earlier refusals pass; active: one truth value per stream, or None."""
    n = len(depths)
    if n_blocks == 0 or block_len == 0 or block_len > max_block_len: return ("lengths",)
    for s, d in enumerate(depths):
        if d not in (16, 24): return ("depth", s)
    if n * n_blocks > MAX_ENTRIES: return ("overflow",)
    for s in range(n):
        if active is not None and not active[s]: continue      # entries of PAUSED streams are neither read nor checked
        for k in range(n_blocks):
            if not entry_ok(int(table[s][k]), depths[s], block_len, arena_bytes): return ("entry", s * n_blocks + k)
    return None


def widen(packet, depth):
    """one packet's bytes as packed 24 bit: a 16-bit sample s becomes s << 8 (00 lo hi), a 24-bit packet is what it is"""
    packet = np.asarray(packet, dtype=np.uint8)
    if depth == 24: return packet.copy()
    out = np.zeros((packet.size // 2, 3), dtype=np.uint8)
    out[:, 1:] = packet.reshape(-1, 2)
    return out.reshape(-1)


def gather(arena, row, depth, block_len):
    """one stream's run of len(row) * block_len frames, packed 24 bit: packet k is block_len frames at arena[row[k]:]"""
    n = block_len * frame_bytes(depth)
    parts = []
    for off in row:
        off = int(off)
        assert off + n <= len(arena)
        parts.append(widen(arena[off:off + n], depth))
    return np.concatenate(parts)


def mixed_input(arena, depths, table, block_len, active=None):
    """the pcm_in of the dspi_process_mixed call that a packet call IS: every stream's packets in order at the stream's own depth, streams back
    to back (a paused stream's run: zeros, which nobody reads)"""
    runs = []
    for s, d in enumerate(depths):
        n = block_len * frame_bytes(d)
        if active is not None and not active[s]: runs.append(np.zeros(n * len(table[s]), dtype=np.uint8)); continue
        runs.append(np.concatenate([np.asarray(arena[int(o):int(o) + n], dtype=np.uint8) for o in table[s]]))
    return np.concatenate(runs)
