// dspi_packets_out.cpp — the packet table of dspi_packets_emit: the check in its order, the overlap check and the CPU path (dspi_packets_out.h).
#include "dspi_packets_out.h"

#include <string.h>

#include <algorithm>
#include <vector>

namespace dspi {

EmitBad packets_emit_check(const uint8_t *formats, const uint64_t *table, uint32_t n_streams, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len, uint32_t max_block_len,
                           uint64_t arena_bytes, const uint8_t *active, bool overlap, uint64_t *at) {
    if (n_blocks == 0 || block_len == 0 || block_len > max_block_len) return EmitBad::Lengths;
    for (uint32_t s = 0; s < n_streams; s++)
        if (formats[s] != 24 && formats[s] != 32) { if (at) *at = s; return EmitBad::Format; }
    if ((uint64_t)n_streams * n_pairs > kPacketMaxEntries || (uint64_t)n_streams * n_pairs * n_blocks > kPacketMaxEntries) return EmitBad::Overflow;
    const uint64_t row_len = (uint64_t)n_pairs * n_blocks;
    uint64_t live = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        if (active && !active[s]) continue;
        const uint64_t bytes = (uint64_t)block_len * emit_frame_bytes(formats[s]);
        const uint64_t *const row = table + s * row_len;
        for (uint64_t i = 0; i < row_len; i++) {
            if (!emit_entry_ok(row[i], bytes, arena_bytes)) { if (at) *at = s * row_len + i; return EmitBad::Entry; }
            live += row[i] != kPacketSkip;
        }
    }
    if (!overlap) return EmitBad::Ok;
    // Sorted by offset, an entry that shares a byte with a later one shares one with its successor, and one that shares a byte with an
    // earlier one starts before the furthest end seen so far: one sweep marks every entry that overlaps any other.
    struct Run { uint64_t a, b, index; };
    std::vector<Run> runs;
    runs.reserve(live);
    for (uint32_t s = 0; s < n_streams; s++) {
        if (active && !active[s]) continue;
        const uint64_t bytes = (uint64_t)block_len * emit_frame_bytes(formats[s]);
        for (uint64_t i = 0; i < row_len; i++) {
            const uint64_t o = table[s * row_len + i];
            if (o != kPacketSkip) runs.push_back(Run{o, o + bytes, s * row_len + i});
        }
    }
    std::sort(runs.begin(), runs.end(), [](const Run &x, const Run &y) { return x.a != y.a ? x.a < y.a : x.index < y.index; });
    uint64_t first = kPacketSkip, end = 0, end_index = 0;      // the furthest end so far and whose it is
    for (size_t i = 0; i < runs.size(); i++) {
        if (i && runs[i].a < end) first = std::min(first, std::min(runs[i].index, end_index));
        if (!i || runs[i].b > end) { end = runs[i].b; end_index = runs[i].index; }
    }
    if (first == kPacketSkip) return EmitBad::Ok;
    if (at) *at = first;
    return EmitBad::Overlap;
}

void packets_emit_cpu(uint8_t *arena, const int32_t *pairs, const uint64_t *row, uint8_t format, uint32_t s, uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len,
                      uint32_t tile_streams) {
    const uint64_t F = (uint64_t)n_blocks * block_len;
    const uint32_t fb = emit_frame_bytes(format);
    for (uint32_t p = 0; p < n_pairs; p++)
        for (uint32_t k = 0; k < n_blocks; k++) {
            const uint64_t o = row[(uint64_t)p * n_blocks + k];
            if (o == kPacketSkip) continue;
            uint8_t *d = arena + o;
            for (uint32_t f = 0; f < block_len; f++, d += fb) {
                const uint64_t frame = (uint64_t)k * block_len + f;
                uint32_t w[2];
                for (uint32_t side = 0; side < 2; side++) {
                    const uint64_t at = tile_streams ? (((uint64_t)(s / tile_streams) * 2u * n_pairs + 2u * p + side) * F + frame) * tile_streams + s % tile_streams
                                                     : ((((uint64_t)s * n_pairs + p) * F + frame) * 2u + side);
                    w[side] = (uint32_t)pairs[at];
                }
                if (fb == 8u) {
                    const uint8_t b[8] = {(uint8_t)w[0], (uint8_t)(w[0] >> 8), (uint8_t)(w[0] >> 16), (uint8_t)(w[0] >> 24), (uint8_t)w[1], (uint8_t)(w[1] >> 8), (uint8_t)(w[1] >> 16), (uint8_t)(w[1] >> 24)};
                    memcpy(d, b, 8);
                } else {
                    const uint8_t b[6] = {(uint8_t)w[0], (uint8_t)(w[0] >> 8), (uint8_t)(w[0] >> 16), (uint8_t)w[1], (uint8_t)(w[1] >> 8), (uint8_t)(w[1] >> 16)};
                    memcpy(d, b, 6);
                }
            }
        }
}

}  // namespace dspi
