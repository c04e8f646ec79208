// dspi_tablecheck.h — the entry check of a packet table that lies in DEVICE memory (include/dspi.h, "resident packet tables"): the lowest
// index i of an entry of an ACTIVE stream that the entry rule refuses, or kTableCheckNone.  One checker serves both table kinds: the input
// table of dspi_process_packets (dspi_packets.h: packet_entry_ok) and the emit table of dspi_packets_emit (dspi_packets_out.h: emit_entry_ok);
// the rule is theirs and is not restated here.  Plain C++ (no HIP): dspi_capi.cpp includes it, tests/tablecheck_driver.cpp exercises it without
// a GPU.  Here is THE ARITHMETIC OF THE KERNEL (dspi_tablecheck.hip) as inline functions that the kernel and the driver's walker both include:
// for a (workgroup, thread, iteration) they give every table index that is loaded, the width of the load, and every entry that the lane
// judges; tablecheck_lane is the lane's whole body with the loads behind a functor, so the driver runs the very loop the kernel runs and
// proves without a GPU that every entry is judged exactly once and that nothing outside the table's 8 * entries bytes is read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dspi_packets_out.h"

namespace dspi {

constexpr uint32_t kTableInput = 0, kTableEmit = 1;      // the table's kind
constexpr uint64_t kTableCheckNone = ~0ull;              // the answer when no entry is refused
constexpr uint32_t kTableCheckThreads = 256;             // a workgroup: four waves
constexpr uint32_t kTableCheckWave = 64;
constexpr uint32_t kTableCheckWaves = kTableCheckThreads / kTableCheckWave;
// the launch's default cap on the grid: four workgroups for each of 256 CUs, 16 waves per CU with a 16-byte load in flight each; a table of
// more than 2 * 256 * 1024 entries goes round the grid-stride loop
constexpr uint32_t kTableCheckDefaultWgs = 1024;

// What is checked: table[entries], entry i belonging to stream i / per_stream, whose kind byte (a depth, 16 / 24, or a format, 24 / 32; valid:
// the calls' refusal 3 came first) gives its packets' length
struct TableCheck {
    uint64_t entries;            // n_streams * per_stream, at most kPacketMaxEntries
    uint64_t arena_bytes;
    uint32_t per_stream;         // input: n_blocks; emit: n_pairs * n_blocks.  Not 0 where entries is not
    uint32_t block_len;
    uint32_t kind;               // kTableInput / kTableEmit
};

// ---- the rule, from the two tables' own headers ----
DSPI_PK_HD inline uint64_t tablecheck_packet_bytes(uint32_t kind, uint8_t stream_kind, uint32_t block_len) {
    return (uint64_t)block_len * (kind == kTableEmit ? emit_frame_bytes(stream_kind) : intake_frame_bytes(stream_kind));
}
DSPI_PK_HD inline bool tablecheck_entry_ok(uint32_t kind, uint64_t offset, uint64_t bytes, uint64_t arena_bytes) {
    return kind == kTableEmit ? emit_entry_ok(offset, bytes, arena_bytes) : packet_entry_ok(offset, bytes, arena_bytes);
}

// ---- which entries a lane loads ----
// the grid: a thread per PAIR of entries (one 16-byte load), at least one workgroup, at most max_workgroups
DSPI_PK_HD inline uint32_t tablecheck_workgroups(uint64_t entries, uint32_t max_workgroups) {
    const uint64_t want = (entries / 2u + kTableCheckThreads - 1u) / kTableCheckThreads;
    const uint64_t cap = max_workgroups ? max_workgroups : 1u;
    return (uint32_t)(want < 1u ? 1u : want > cap ? cap : want);
}
// the thread's it-th pair: entries *first and *first + 1, ONE 16-byte load at table + *first (*first is even, the table 16-byte aligned);
// false: it has none, nor any for a larger it
DSPI_PK_HD inline bool tablecheck_pair(uint64_t entries, uint32_t n_wgs, uint32_t wg, uint32_t tid, uint64_t it, uint64_t *first) {
    const uint64_t q = (it * n_wgs + wg) * kTableCheckThreads + tid;
    *first = 2u * q;
    return q < entries / 2u;
}
// the last entry of an odd count: ONE 8-byte load at table + *index, by the first thread of the first workgroup
DSPI_PK_HD inline bool tablecheck_tail(uint64_t entries, uint32_t wg, uint32_t tid, uint64_t *index) {
    *index = entries - 1u;
    return (entries & 1u) && wg == 0u && tid == 0u;
}
// the streams of the two entries of a pair: one division
DSPI_PK_HD inline void tablecheck_pair_streams(uint64_t first, uint32_t per_stream, uint32_t *s0, uint32_t *s1) {
    const uint32_t i = (uint32_t)first;      // (entries <= kPacketMaxEntries)
    *s0 = i / per_stream;
    *s1 = *s0 + (i - *s0 * per_stream + 1u == per_stream ? 1u : 0u);
}
DSPI_PK_HD inline uint64_t tablecheck_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- a lane's whole body ----
// M gives the memory:  M.pair(first, v)   v[0], v[1] = table[first], table[first + 1], one 16-byte load
//                      M.one(index)       table[index], one 8-byte load
//                      M.stream_kind(s)   the stream's depth or format byte
//                      M.active(s)        the stream's activity bit (true where there is no bitmap)
// An entry of a paused stream is loaded with its neighbour but not judged.  Returns the lowest refused index among the lane's entries.
template <class M> DSPI_PK_HD inline uint64_t tablecheck_judge(const TableCheck &a, M &m, uint64_t index, uint32_t s, uint64_t offset) {
    if (!m.active(s)) return kTableCheckNone;
    return tablecheck_entry_ok(a.kind, offset, tablecheck_packet_bytes(a.kind, m.stream_kind(s), a.block_len), a.arena_bytes) ? kTableCheckNone : index;
}
template <class M> DSPI_PK_HD inline uint64_t tablecheck_lane(const TableCheck &a, uint32_t n_wgs, uint32_t wg, uint32_t tid, M &m) {
    uint64_t lowest = kTableCheckNone, first;
    for (uint64_t it = 0; tablecheck_pair(a.entries, n_wgs, wg, tid, it, &first); it++) {
        uint64_t v[2];
        uint32_t s0, s1;
        m.pair(first, v);
        tablecheck_pair_streams(first, a.per_stream, &s0, &s1);
        lowest = tablecheck_min(lowest, tablecheck_judge(a, m, first, s0, v[0]));
        lowest = tablecheck_min(lowest, tablecheck_judge(a, m, first + 1u, s1, v[1]));
    }
    if (tablecheck_tail(a.entries, wg, tid, &first)) lowest = tablecheck_min(lowest, tablecheck_judge(a, m, first, (uint32_t)(first / a.per_stream), m.one(first)));
    return lowest;
}

// ---- the reduction: the kernel's steps, which the driver replays on arrays ----
// within a wave a butterfly: for off = 32, 16 .. 1 every lane takes tablecheck_min(own, lane ^ off's); then lane 0 of each wave leaves its value
// in LDS slot `wave`, the workgroup's thread 0 takes the minimum of the kTableCheckWaves slots and, where that is not kTableCheckNone, brings
// it into the answer word with one 64-bit atomic minimum.
constexpr uint32_t kTableCheckFirstStep = kTableCheckWave / 2u;

#ifdef __HIP__
// (dspi_tablecheck.hip) sets *answer to kTableCheckNone on `stream`, then one launch that leaves the lowest refused index there.  table
// [entries] (16-byte aligned), kinds [entries / per_stream] and answer (8-byte aligned) are device memory; active: the activity bitmap or
// null = every stream.  max_workgroups 0: kTableCheckDefaultWgs.
hipError_t launch_tablecheck(const TableCheck &a, const uint64_t *table, const uint8_t *kinds, const uint32_t *active, uint64_t *answer, uint32_t max_workgroups, hipStream_t stream);
#endif

}  // namespace dspi
