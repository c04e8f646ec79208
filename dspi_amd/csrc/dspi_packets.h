// dspi_packets.h — the packet table of dspi_process_packets (include/dspi.h): table[s * n_blocks + k] is the byte offset in the caller's arena
// of packet k of stream s, block_len frames of 4 bytes (16 bit) or 6 (24 bit).  The call is dspi_process_mixed with every stream's frames taken
// packet by packet from where the table points; entries may be equal and may overlap in any way.  Plain C++ (no HIP): dspi_capi.cpp includes
// it, tests/packets_driver.cpp exercises it without a GPU.  Here are the entry rule, the check in its order, one stream's row gathered on the
// CPU (packets_gather_cpu: the model the kernel is held to), and THE ADDRESS ARITHMETIC OF THE KERNEL (dspi_packetrx.hip) as inline functions
// that the kernel and the driver's walker both include: for a (workgroup, lane group, lane, iteration) they give every source address that is read
// and every destination address that is written, so the walker proves without a GPU that nothing outside an entry is read and that every
// destination byte of an active stream is written exactly once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dspi_intake.h"

#ifdef __HIP__
#define DSPI_PK_HD __host__ __device__
#else
#define DSPI_PK_HD
#endif

namespace dspi {

// ---- the entry rule and the check ----
// an entry is legal when it is even and the packet's `bytes` end inside the arena
constexpr bool packet_entry_ok(uint64_t offset, uint64_t bytes, uint64_t arena_bytes) { return !(offset & 1u) && bytes <= arena_bytes && offset <= arena_bytes - bytes; }
// the table's entries are counted in 31 bits (one kernel job each)
constexpr uint64_t kPacketMaxEntries = 0x7fffffffull;
// What a table is refused for, in the order of the call's refusals 2 to 5 (the pointers are the caller's to check): the lengths (n_blocks or
// block_len 0, block_len above max_block_len), a depth that is neither 16 nor 24 (*at: the stream), n_streams * n_blocks above
// kPacketMaxEntries, the first illegal entry of an active stream in table order (*at: s * n_blocks + k).  active: one byte per stream or
// null (every stream); a paused stream's entries are not looked at.
enum class PacketsBad { Ok, Lengths, Depth, Overflow, Entry };
PacketsBad packets_check(const uint8_t *depths, const uint64_t *table, uint32_t n_streams, uint32_t n_blocks, uint32_t block_len, uint32_t max_block_len, uint64_t arena_bytes,
                         const uint8_t *active, uint64_t *at);
// one stream's row of the table (n_blocks entries, legal) as its packed 24-bit run of n_blocks * block_len frames: packet k through
// intake_widen_cpu into dst + 6 block_len k.  dst does not overlap the arena.
void packets_gather_cpu(uint8_t *dst, const uint8_t *arena, const uint64_t *row, uint8_t depth, uint32_t n_blocks, uint32_t block_len);

// ---- the kernel's geometry (dspi_packetrx.hip says why) ----
constexpr uint32_t kPacketLanes = 16;           // lanes that serve one job: a quarter of a wave
constexpr uint32_t kPacketJobsPerWg = 16;       // jobs of a workgroup, all at the same time: 256 threads, four jobs per wave
constexpr uint32_t kPacketTile = 1024;          // destination bytes of a job, cut on absolute 16-byte boundaries
constexpr uint32_t kPacketImage = kPacketTile + 16;      // LDS bytes per job: its source range, aligned mod 16 like the source

// a job is (stream, packet, tile); a packet has packet_tiles(block_len) tiles whatever its alignment (one up to 168 frames), of which the
// packet may not reach the last
DSPI_PK_HD inline uint32_t packet_tiles(uint32_t block_len) { return (uint32_t)((6ull * block_len + 14u) / kPacketTile + 1u); }
// the job of lane group `group` of workgroup `wg`: the groups of a workgroup work on neighbouring jobs
DSPI_PK_HD inline uint64_t packet_job_index(uint32_t wg, uint32_t group) { return (uint64_t)wg * kPacketJobsPerWg + group; }
DSPI_PK_HD inline void packet_job(uint64_t job, uint32_t n_blocks, uint32_t tiles, uint32_t *s, uint32_t *k, uint32_t *t) {
    const uint64_t sk = job / tiles;
    *t = (uint32_t)(job - sk * tiles);
    *s = (uint32_t)(sk / n_blocks);
    *k = (uint32_t)(sk - (uint64_t)*s * n_blocks);
}

// One job's ranges, all as ADDRESSES (alignment mod 16 is a matter of addresses): the tile's part of the packet's destination [ta, tb) and
// piece0, the 16-aligned address of the tile's first piece; the source bytes that part comes from [sa, sb) — all of them for a 24-bit packet,
// samples ra / 3 .. (rb - 1) / 3 for a 16-bit one —, of which [ha, hb) are whole aligned 16-byte pieces; image0: the address LDS byte 0 stands
// for; r0: the place of ta in its 3-byte sample.
struct PacketTile {
    uint64_t piece0, ta, tb;
    uint64_t sa, sb, ha, hb, image0;
    uint32_t r0;
};
// d0 / s0: the addresses of the packet's first destination / source byte.  False: the packet does not reach tile t.
DSPI_PK_HD inline bool packet_tile(uint64_t d0, uint64_t s0, uint32_t block_len, bool wide, uint32_t t, PacketTile *T) {
    const uint64_t d1 = d0 + 6ull * block_len;
    T->piece0 = (d0 & ~15ull) + (uint64_t)t * kPacketTile;
    T->ta = T->piece0 > d0 ? T->piece0 : d0;
    T->tb = T->piece0 + kPacketTile < d1 ? T->piece0 + kPacketTile : d1;
    if (T->ta >= T->tb) return false;
    const uint64_t ra = T->ta - d0, rb = T->tb - d0, k0 = ra / 3u;
    T->r0 = (uint32_t)(ra - 3u * k0);
    T->sa = s0 + (wide ? ra : 2u * k0);
    T->sb = s0 + (wide ? rb : 2u * ((rb - 1u) / 3u + 1u));
    T->image0 = T->sa & ~15ull;
    const uint64_t up = (T->sa + 15u) & ~15ull, down = T->sb & ~15ull;
    T->ha = up < T->sb ? up : T->sb;
    T->hb = T->ha > down ? T->ha : down;
    return true;
}
// source side.  The lane's i-th whole piece (a 16-byte load at *p); false: it has none, nor any for a larger i
DSPI_PK_HD inline bool packet_src_piece(const PacketTile &T, uint32_t lane, uint32_t i, uint64_t *p) { *p = T.ha + 16ull * (lane + kPacketLanes * i); return *p < T.hb; }
// ... the lane's 2-byte word in front of the first piece / behind the last (fewer than eight of each)
DSPI_PK_HD inline bool packet_src_head(const PacketTile &T, uint32_t lane, uint64_t *p) { *p = T.sa + 2ull * lane; return *p < T.ha; }
DSPI_PK_HD inline bool packet_src_tail(const PacketTile &T, uint32_t lane, uint64_t *p) { *p = T.hb + 2ull * lane; return *p < T.sb; }
// destination side.  The lane's i-th piece at *p (false: none, nor for a larger i); *whole: the packet covers all 16 bytes, one 16-byte store;
// else the piece is the packet's first or last, shared with a neighbour's run, and only the 2-byte words inside [ta, tb) are stored, singly
DSPI_PK_HD inline bool packet_dst_piece(const PacketTile &T, uint32_t lane, uint32_t i, uint64_t *p, bool *whole) {
    *p = T.piece0 + 16ull * (lane + kPacketLanes * i);
    if (*p >= T.tb) return false;
    *whole = *p >= T.ta && *p + 16u <= T.tb;
    return true;
}
// destination word j of the tile (at ta + 2j) is a function of ONE source word: its address, and *r, how it is made from it (packet_word_make)
DSPI_PK_HD inline uint64_t packet_word_src(const PacketTile &T, bool wide, uint32_t j, uint32_t *r) {
    if (wide) { *r = 1u; return T.sa + 2ull * j; }
    const uint32_t b = T.r0 + 2u * j, k = b / 3u;
    *r = b - 3u * k;
    return T.sa + 2ull * k;
}
// r = 1: the word itself (every 24-bit word; lo hi of a widened sample); r = 0: 00 lo; r = 2: hi 00
DSPI_PK_HD inline uint32_t packet_word_make(uint32_t v, uint32_t r) { return r == 0u ? (v & 0xffu) << 8 : r == 1u ? v : v >> 8; }

}  // namespace dspi
