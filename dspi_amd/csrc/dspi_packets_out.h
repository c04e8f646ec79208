// dspi_packets_out.h — the packet table of dspi_packets_emit (include/dspi.h): table[(s * n_pairs + p) * n_blocks + k] is the byte offset in the
// caller's arena where packet k of pair p of stream s GOES, block_len frames of 8 bytes (format 32: the two pair words as they stand) or 6
// (format 24: the low three bytes of each word, a 24-bit USB packet), or DSPI_PACKET_SKIP.  The source is a buffer of plain pair words that a
// process call wrote, stream-major [stream][pair][F][2] or tiled [tile][output][F][R].  Plain C++ (no HIP): dspi_capi.cpp includes it,
// tests/packets_out_driver.cpp exercises it without a GPU.  Here are the entry rule, the check in its order with the overlap check, one stream's
// row emitted on the CPU from either layout (packets_emit_cpu: the host path, and the model the kernels are held to), and THE ADDRESS
// ARITHMETIC OF THE TWO KERNELS (dspi_packettx.hip) as inline functions that the kernels and the driver's walker both include: for a
// (workgroup, lane group, lane, iteration) they give every source address that is read and every destination address and width that is
// written, so the walker proves without a GPU that nothing outside an active stream's source is read, that every byte of an entry is written
// exactly once and that no byte outside an entry is written.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dspi_packets.h"

#ifdef __HIP__
#include <hip/hip_runtime_api.h>
#endif

namespace dspi {

// ---- the entry rule and the check ----
constexpr uint64_t kPacketSkip = ~0ull;             // DSPI_PACKET_SKIP: the entry emits nothing
constexpr uint32_t kEmitCheckOverlap = 0x1u;        // DSPI_EMIT_CHECK_OVERLAP
DSPI_PK_HD inline uint32_t emit_frame_bytes(uint32_t format) { return format == 24u ? 6u : 8u; }
// an entry is legal when it is the skip word, or even with the packet's `bytes` ending inside the arena
constexpr bool emit_entry_ok(uint64_t offset, uint64_t bytes, uint64_t arena_bytes) { return offset == kPacketSkip || packet_entry_ok(offset, bytes, arena_bytes); }
// What a table is refused for, in the order of the call's refusals 2 to 5 (the pointers are the caller's to check): the lengths (n_blocks or
// block_len 0, block_len above max_block_len), a format that is neither 24 nor 32 (*at: the stream), n_streams * n_pairs * n_blocks above
// kPacketMaxEntries, the first illegal entry of an active stream in table order (*at: its index); then, `overlap` asked for, the first entry
// in table order that shares a byte with another one (*at: its index; found by sorting, n log n).  active: one byte per stream or null (every
// stream); a paused stream's entries are not looked at.
enum class EmitBad { Ok, Lengths, Format, Overflow, Entry, Overlap };
EmitBad packets_emit_check(const uint8_t *formats, const uint64_t *table, uint32_t n_streams, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len, uint32_t max_block_len,
                           uint64_t arena_bytes, const uint8_t *active, bool overlap, uint64_t *at);
// stream s's row of the table (n_pairs * n_blocks entries, legal) emitted into the arena from `pairs`, the whole source buffer: stream-major
// (tile_streams 0) or tiled in tiles of tile_streams columns.  Nothing but the entries' bytes is written.
void packets_emit_cpu(uint8_t *arena, const int32_t *pairs, const uint64_t *row, uint8_t format, uint32_t s, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len,
                      uint32_t tile_streams);

// ---- what the two kernels share (dspi_packettx.hip says why) ----
constexpr uint32_t kEmitLanes = 16;             // lanes that serve one packet (stream-major) or one column's piece of one (tiled): a quarter of a wave
constexpr uint32_t kEmitGroups = 16;            // lane groups of a workgroup
constexpr uint32_t kEmitThreads = kEmitLanes * kEmitGroups;

// What a lane group writes, as ADDRESSES (alignment mod 16 is a matter of addresses): destination bytes [a, b), a whole number of frames of fb
// bytes, through an LDS image whose byte 0 stands for address image0 <= a.
struct EmitSpan {
    uint64_t a, b, image0;
    uint32_t fb;
};
// frame f of the span (its two words l, r) stands in the image from byte emit_frame_at on (even), as emit_frame_words' 16-bit words:
// four of them (format 32: lo hi lo hi) or three (format 24: l0 l1 | l2 r0 | r1 r2)
DSPI_PK_HD inline uint32_t emit_frame_at(const EmitSpan &S, uint32_t f) { return (uint32_t)(S.a - S.image0) + S.fb * f; }
DSPI_PK_HD inline uint32_t emit_frame_words(uint32_t l, uint32_t r, uint32_t fb, uint16_t w[4]) {
    if (fb == 8u) { w[0] = (uint16_t)l; w[1] = (uint16_t)(l >> 16); w[2] = (uint16_t)r; w[3] = (uint16_t)(r >> 16); return 4u; }
    w[0] = (uint16_t)l; w[1] = (uint16_t)(((l >> 16) & 0xffu) | ((r & 0xffu) << 8)); w[2] = (uint16_t)(r >> 8); w[3] = 0;
    return 3u;
}
// destination side.  The lane's i-th piece at *p, cut on absolute 16-byte boundaries (false: none, nor for a larger i); *whole: the span covers
// all 16 bytes, one 16-byte store; else the piece is the span's first or last and only the 2-byte words inside [a, b) are stored, singly
DSPI_PK_HD inline bool emit_dst_piece(const EmitSpan &S, uint32_t lane, uint32_t i, uint64_t *p, bool *whole) {
    *p = (S.a & ~15ull) + 16ull * (lane + kEmitLanes * i);
    if (*p >= S.b) return false;
    *whole = *p >= S.a && *p + 16u <= S.b;
    return true;
}
// the table's entry of (stream, pair, packet)
DSPI_PK_HD inline uint64_t emit_entry_index(uint32_t s, uint32_t p, uint32_t k, uint32_t n_pairs, uint32_t n_blocks) { return ((uint64_t)s * n_pairs + p) * n_blocks + k; }

// ---- the stream-major kernel: a lane group serves an entry, a workgroup kEmitGroups neighbouring ones ----
constexpr uint32_t kEmitMajorPitch = 1792;      // LDS bytes per lane group: 14 + 8 * 192 bytes rounded up to a multiple of 256 (the bank arithmetic)
static_assert(kEmitMajorPitch % 256u == 0 && kEmitMajorPitch >= 16u + 8u * 192u, "a packet's image, whatever its alignment");
DSPI_PK_HD inline uint64_t emit_major_entry(uint32_t wg, uint32_t group) { return (uint64_t)wg * kEmitGroups + group; }
DSPI_PK_HD inline uint32_t emit_major_stream(uint64_t e, uint32_t n_pairs, uint32_t n_blocks) { return (uint32_t)(e / ((uint64_t)n_pairs * n_blocks)); }
// dst0: the arena's address
DSPI_PK_HD inline EmitSpan emit_major_span(uint64_t dst0, uint64_t offset, uint32_t format, uint32_t block_len) {
    EmitSpan S;
    S.fb = emit_frame_bytes(format);
    S.a = dst0 + offset; S.b = S.a + (uint64_t)S.fb * block_len; S.image0 = S.a & ~15ull;
    return S;
}
// source side: with F = n_blocks * block_len the run of entry e starts 8 * e * block_len bytes into the buffer.  The lane's i-th frame *f of
// the packet, an 8-byte load at *p (src0: the buffer's address); false: it has none, nor any for a larger i
DSPI_PK_HD inline bool emit_major_src(uint64_t src0, uint64_t e, uint32_t block_len, uint32_t lane, uint32_t i, uint32_t *f, uint64_t *p) {
    *f = lane + kEmitLanes * i;
    *p = src0 + 8ull * (e * block_len + *f);
    return *f < block_len;
}

// ---- the tiled kernel: a workgroup serves (tile, pair, packet, chunk of kEmitChunk frames), a lane group one column's piece at a time ----
constexpr uint32_t kEmitChunk = 32;             // frames: 6 and 8 times it are multiples of 16, so a chunk's span is aligned as its packet is
constexpr uint32_t kEmitTiledPitch = 65;        // LDS words per column: 2 + 8 * kEmitChunk bytes, odd (the bank arithmetic)
static_assert(kEmitChunk % 8u == 0 && kEmitTiledPitch % 2u == 1 && kEmitTiledPitch * 4u >= 2u + 8u * kEmitChunk, "a column's image of a chunk");
DSPI_PK_HD inline uint32_t emit_chunks(uint32_t block_len) { return (block_len + kEmitChunk - 1u) / kEmitChunk; }
struct EmitTiledJob {
    uint32_t tile, pair, k;      // the packets (tile * R + c, pair, k) of the tile's columns c
    uint32_t f0, nf;             // frames [f0, f0 + nf) of each
};
DSPI_PK_HD inline EmitTiledJob emit_tiled_job(uint64_t wg, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len) {
    const uint32_t chunks = emit_chunks(block_len);
    EmitTiledJob J;
    const uint32_t ch = (uint32_t)(wg % chunks); wg /= chunks;
    J.k = (uint32_t)(wg % n_blocks); wg /= n_blocks;
    J.pair = (uint32_t)(wg % n_pairs); J.tile = (uint32_t)(wg / n_pairs);
    J.f0 = ch * kEmitChunk;
    J.nf = block_len - J.f0 < kEmitChunk ? block_len - J.f0 : kEmitChunk;
    return J;
}
DSPI_PK_HD inline uint64_t emit_tiled_workgroups(uint32_t n_streams, uint32_t R, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len) {
    return (uint64_t)((n_streams + R - 1u) / R) * n_pairs * n_blocks * emit_chunks(block_len);
}
// the span of the column whose entry is `offset`: the chunk's frames of its packet; the image is aligned mod 4 like the destination
DSPI_PK_HD inline EmitSpan emit_tiled_span(uint64_t dst0, uint64_t offset, uint32_t format, const EmitTiledJob &J) {
    EmitSpan S;
    S.fb = emit_frame_bytes(format);
    S.a = dst0 + offset + (uint64_t)S.fb * J.f0; S.b = S.a + (uint64_t)S.fb * J.nf; S.image0 = S.a & ~3ull;
    return S;
}
// source side: thread tid's i-th row piece: frame *fr of the chunk, columns 4 *q .. 4 *q + 3, their left words at *pl and their right words
// at *pr (outputs 2 pair and 2 pair + 1 of [tile][2 n_pairs][F][R]); false: none, nor for a larger i.  The 16 bytes are ONE load where all
// four columns emit (emit_tiled_whole) and a 4-byte load per emitting column otherwise: a column that emits nothing is not read.
DSPI_PK_HD inline bool emit_tiled_src(uint64_t src0, const EmitTiledJob &J, uint32_t R, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len, uint32_t tid, uint32_t i,
                                      uint32_t *fr, uint32_t *q, uint64_t *pl, uint64_t *pr) {
    const uint32_t row_lanes = R / 4u;
    const uint64_t F = (uint64_t)n_blocks * block_len;
    *q = tid % row_lanes;
    *fr = tid / row_lanes + (kEmitThreads / row_lanes) * i;
    if (*fr >= J.nf) return false;
    *pl = src0 + 4ull * ((((uint64_t)J.tile * 2u * n_pairs + 2u * J.pair) * F + (uint64_t)J.k * block_len + J.f0 + *fr) * R + 4u * *q);
    *pr = *pl + 4ull * F * R;
    return true;
}
DSPI_PK_HD inline bool emit_tiled_whole(uint32_t mask) { return mask == 15u; }
// column side: the column lane group `group` serves in its i-th pass; false: none, nor for a larger i
DSPI_PK_HD inline bool emit_tiled_col(uint32_t R, uint32_t group, uint32_t i, uint32_t *c) { *c = group + kEmitGroups * i; return *c < R; }

#ifdef __HIP__
// (dspi_packettx.hip) one launch: every entry of an active stream that is not the skip word, from `pairs` — stream-major, or tiled in tiles of
// tile_streams columns — into the arena.  table [n_streams][n_pairs][n_blocks] and formats [n_streams] are device memory; active: the activity
// bitmap or null = every stream.  pairs is 16-byte aligned, the arena 2-byte.
hipError_t launch_packettx(const int32_t *pairs, uint32_t tile_streams, const uint64_t *table, const uint8_t *formats, const uint32_t *active, void *arena, uint32_t n_streams,
                           uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len, hipStream_t stream);
#endif

}  // namespace dspi
