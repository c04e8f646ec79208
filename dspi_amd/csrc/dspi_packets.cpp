// dspi_packets.cpp — the packet table of dspi_process_packets: the check in its order and the CPU gather (dspi_packets.h).
#include "dspi_packets.h"

namespace dspi {

PacketsBad packets_check(const uint8_t *depths, const uint64_t *table, uint32_t n_streams, uint32_t n_blocks, uint32_t block_len, uint32_t max_block_len, uint64_t arena_bytes,
                         const uint8_t *active, uint64_t *at) {
    if (n_blocks == 0 || block_len == 0 || block_len > max_block_len) return PacketsBad::Lengths;
    const uint32_t bad = intake_check_depths(depths, n_streams);
    if (bad < n_streams) { if (at) *at = bad; return PacketsBad::Depth; }
    if ((uint64_t)n_streams * n_blocks > kPacketMaxEntries) return PacketsBad::Overflow;
    for (uint32_t s = 0; s < n_streams; s++) {
        if (active && !active[s]) continue;
        const uint64_t bytes = (uint64_t)block_len * intake_frame_bytes(depths[s]);
        const uint64_t *const row = table + (uint64_t)s * n_blocks;
        for (uint32_t k = 0; k < n_blocks; k++)
            if (!packet_entry_ok(row[k], bytes, arena_bytes)) { if (at) *at = (uint64_t)s * n_blocks + k; return PacketsBad::Entry; }
    }
    return PacketsBad::Ok;
}

void packets_gather_cpu(uint8_t *dst, const uint8_t *arena, const uint64_t *row, uint8_t depth, uint32_t n_blocks, uint32_t block_len) {
    for (uint32_t k = 0; k < n_blocks; k++) intake_widen_cpu(dst + (uint64_t)kIntakeOutFrame * block_len * k, arena + row[k], depth, block_len);
}

}  // namespace dspi
