"""The emit table (include/dspi.h: dspi_packets_emit, dspi_packets_emit_check) as a model in numpy, written from the header's prose: when an entry
is legal, what a table is refused for and in which order, with the index of the entry refused, which entries overlap, and what an accepted
table makes of a buffer of pair words, stream-major or tiled — the arena afterwards, byte for byte."""
import numpy as np

MAX_BLOCK_LEN = 192      # DSPI_MAX_BLOCK_LEN
MAX_ENTRIES = 2 ** 31 - 1
SKIP = 2 ** 64 - 1       # DSPI_PACKET_SKIP


def frame_bytes(fmt):
    return {24: 6, 32: 8}[fmt]


def entry_ok(offset, fmt, block_len, arena_bytes):
    """AN EMIT ENTRY IS LEGAL when it is DSPI_PACKET_SKIP, or when it is even and offset + block_len * frame bytes <= arena_bytes"""
    return offset == SKIP or (offset % 2 == 0 and offset + block_len * frame_bytes(fmt) <= arena_bytes)


def check(formats, table, n_pairs, n_blocks, block_len, arena_bytes, active=None, overlap=False, max_block_len=MAX_BLOCK_LEN):
    """refusals 2 to 5 behind the pointers, then the overlap rule when asked: None, or ("lengths",), ("format", s), ("overflow",), ("entry", i),
    ("overlap", i).  table: per stream n_pairs * n_blocks offsets, looked at only when the earlier refusals pass; active: one truth value per
    stream, or None."""
    n = len(formats)
    if n_blocks == 0 or block_len == 0 or block_len > max_block_len: return ("lengths",)
    for s, f in enumerate(formats):
        if f not in (24, 32): return ("format", s)
    if n * n_pairs * n_blocks > MAX_ENTRIES: return ("overflow",)
    per = n_pairs * n_blocks
    live = []
    for s in range(n):
        if active is not None and not active[s]: continue      # rows of PAUSED streams are neither read nor checked
        for i in range(per):
            o = int(table[s][i])
            if not entry_ok(o, formats[s], block_len, arena_bytes): return ("entry", s * per + i)
            if o != SKIP: live.append((s * per + i, o, o + block_len * frame_bytes(formats[s])))
    if overlap:      # the first entry, in table order, that shares a byte with another entry (every pair looked at: the model does not sort)
        for i, a, b in live:
            for j, c, d in live:
                if i != j and a < d and c < b: return ("overlap", i)
    return None


def packet(pairs, s, p, k, fmt, block_len, tile_streams=0):
    """the bytes of packet k of pair p of stream s.  pairs: int32 [stream][pair][F][2], or tiled [tile][output][F][R] with left = output 2p and
    right = output 2p + 1.  32: the two int32 LE words of each frame as they stand; 24: the low three bytes of each word, LE, L then R"""
    f = slice(k * block_len, (k + 1) * block_len)
    if tile_streams: words = np.stack([pairs[s // tile_streams, 2 * p, f, s % tile_streams], pairs[s // tile_streams, 2 * p + 1, f, s % tile_streams]], axis=1)
    else: words = pairs[s, p, f, :]
    b = np.ascontiguousarray(words.astype("<i4")).view(np.uint8).reshape(block_len, 2, 4)
    return (b if fmt == 32 else b[:, :, :3]).reshape(-1)


def emit(arena, pairs, formats, table, n_pairs, n_blocks, block_len, tile_streams=0, active=None):
    """the arena after the call (a copy): every entry of an active stream that is not SKIP holds its packet, every other byte is what it was.
    The entries must not overlap (the model asserts it: the result would be unspecified)."""
    out = np.array(arena, dtype=np.uint8, copy=True)
    written = np.zeros(len(out), dtype=bool)
    for s, fmt in enumerate(formats):
        if active is not None and not active[s]: continue
        for p in range(n_pairs):
            for k in range(n_blocks):
                o = int(table[s][p * n_blocks + k])
                if o == SKIP: continue
                b = packet(pairs, s, p, k, fmt, block_len, tile_streams)
                assert o + len(b) <= len(out) and not written[o:o + len(b)].any()
                out[o:o + len(b)] = b
                written[o:o + len(b)] = True
    return out
