// dspi_packetrx.hip — the front end of dspi_process_packets: every stream's packets, from where the table (dspi_packets.h) points in the
// caller's arena, into the tight packed 24-bit array [stream][6F] that the chain kernels read.  Per (stream, packet) the job is the intake's
// (dspi_intake.hip) with the run being ONE packet: destination at 6F s + 6 block_len k, source at arena + table[s][k]; a 24-bit packet is
// copied, a 16-bit packet widened (sample s becomes 00 lo hi); a paused stream is skipped, neither its entries nor its bytes are read.
//
// The two sides of a packet are aligned differently mod 16 (an entry is any even offset; a destination packet starts at a multiple of 6
// block_len), so 16-byte accesses on both sides go through an LDS image of the source range that keeps the SOURCE's alignment, exactly as in
// the intake: whole aligned 16-byte source pieces as one load and one LDS store per lane, the up to seven 2-byte words in front and behind
// singly — nothing outside [offset, offset + length) of the entry is read —; then a lane gathers the eight words of an aligned destination piece
// from LDS and stores 16 bytes.  Neighbouring packets of a stream share a destination piece whenever 6 block_len is no multiple of 16 (44,
// 45 frames): a piece that the packet covers only in part is stored as 2-byte words, the packet's own only, so only disjoint 2-byte stores
// ever meet in a piece and nothing is read back.  All of that arithmetic is dspi_packets.h's (packet_tile and the lane functions), which
// tests/packets_driver.cpp walks on the CPU for every workgroup and lane.
//
// HOW MANY PACKETS A WORKGROUP CARRIES.  A packet is 288 to 576 bytes where streams are many, and a full-size call has 3.3 million of them.
// A job is (stream, packet, tile): a tile is kPacketTile = 1 KiB of the destination cut on absolute 16-byte boundaries, so a packet of up to
// 168 frames is one job and a longer one packet_tiles(block_len) jobs.  A job is served by kPacketLanes = 16 lanes, a quarter of a wave (a
// 288-byte packet is 18 or 19 pieces: two per lane), and a workgroup of 256 threads carries kPacketJobsPerWg = 16 jobs, all at the same time:
// 205 thousand workgroups at full size instead of 3.3 million, every lane of every wave busy, and ONE chain of dependent accesses (entry,
// source, LDS, destination) per workgroup.  The first design, which profiles/packets.md measured — one whole wave per job, four jobs per
// wave one after the other — left three quarters of the lanes idle and made four such chains in a row: config 5's front end took
// 0.75 ms with it and 0.58 ms with this one, of which the kernel is 0.16 ms.
// Jobs are numbered stream-major, packets of a stream next to each other, so the destination pieces that two packets share are written by
// neighbouring lane groups of one workgroup.  Each job has its own LDS image (kPacketImage bytes, 16.3 KiB per workgroup); the barrier only
// orders a group's own LDS stores and loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_packets.h"

namespace dspi {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct PacketRxArgs {
    const uint8_t *arena;        // the caller's bytes: packet k of stream s at arena + table[s * n_blocks + k]
    const uint64_t *table;       // [n_streams][n_blocks]
    const uint8_t *depths;       // [n_streams]: 16 or 24
    const uint32_t *active;      // one bit per stream, or null: every stream
    uint8_t *dst;                // [n_streams][6 n_blocks block_len]
    uint64_t jobs;               // n_streams * n_blocks * tiles
    uint32_t n_blocks, block_len, tiles;
};

__global__ __launch_bounds__(kPacketLanes * kPacketJobsPerWg) void packetrx_kernel(const PacketRxArgs a) {
    __shared__ u4 images[kPacketJobsPerWg][kPacketImage / 16];
    const uint32_t group = threadIdx.x / kPacketLanes, lane = threadIdx.x % kPacketLanes;
    u4 *const image4 = images[group];
    uint16_t *const image = reinterpret_cast<uint16_t *>(image4);
    // alignment is a matter of addresses; the accesses themselves go through the two argument pointers (global, not flat, instructions)
    const uint64_t src0 = reinterpret_cast<uintptr_t>(a.arena), dst0 = reinterpret_cast<uintptr_t>(a.dst);
    auto src_at = [&](uint64_t p) { return a.arena + (p - src0); };
    auto dst_at = [&](uint64_t p) { return a.dst + (p - dst0); };
    const uint64_t packet = 6ull * a.block_len, run = packet * a.n_blocks;

    // (everything that decides `on` is the group's, not the lane's)
    const uint64_t job = packet_job_index(blockIdx.x, group);
    bool on = job < a.jobs, wide = false;
    uint32_t s = 0, k = 0, t = 0;
    PacketTile T;
    if (on) {
        packet_job(job, a.n_blocks, a.tiles, &s, &k, &t);
        on = !a.active || (a.active[s >> 5] >> (s & 31u) & 1u);
    }
    if (on) {
        wide = a.depths[s] == 24;
        on = packet_tile(dst0 + run * s + packet * k, src0 + a.table[(uint64_t)s * a.n_blocks + k], a.block_len, wide, t, &T);
    }
    if (on) {      // source -> LDS
        uint64_t p;
        for (uint32_t i = 0; packet_src_piece(T, lane, i, &p); i++) image4[(p - T.image0) >> 4] = *reinterpret_cast<const u4 *>(src_at(p));
        if (packet_src_head(T, lane, &p)) image[(p - T.image0) / 2u] = *reinterpret_cast<const uint16_t *>(src_at(p));
        if (packet_src_tail(T, lane, &p)) image[(p - T.image0) / 2u] = *reinterpret_cast<const uint16_t *>(src_at(p));
    }
    __syncthreads();
    if (!on) return;
    // LDS -> destination.  word(j): the destination word 2j bytes behind ta
    auto word = [&](uint32_t j) -> uint32_t {
        uint32_t r;
        const uint64_t q = packet_word_src(T, wide, j, &r);
        return packet_word_make(image[(q - T.image0) / 2u], r);
    };
    uint64_t p;
    bool whole;
    for (uint32_t i = 0; packet_dst_piece(T, lane, i, &p, &whole); i++) {
        if (whole) {
            const uint32_t j = (uint32_t)(p - T.ta) / 2u;
            u4 v;
            v.x = word(j) | word(j + 1) << 16; v.y = word(j + 2) | word(j + 3) << 16;
            v.z = word(j + 4) | word(j + 5) << 16; v.w = word(j + 6) | word(j + 7) << 16;
            *reinterpret_cast<u4 *>(dst_at(p)) = v;
        } else {
            for (uint32_t w = 0; w < 8; w++) {
                const uint64_t q = p + 2u * w;
                if (q >= T.ta && q < T.tb) *reinterpret_cast<uint16_t *>(dst_at(q)) = (uint16_t)word((uint32_t)(q - T.ta) / 2u);
            }
        }
    }
}

}  // namespace

hipError_t launch_packetrx(const void *arena, const uint64_t *table, const uint8_t *depths, const uint32_t *active, void *dst, uint32_t n_streams, uint32_t n_blocks,
                           uint32_t block_len, hipStream_t stream) {
    if (!n_streams || !n_blocks || !block_len) return hipSuccess;
    const uint32_t tiles = packet_tiles(block_len);
    const uint64_t entries = (uint64_t)n_streams * n_blocks;
    if (entries > kPacketMaxEntries || entries * tiles / kPacketJobsPerWg >= 0x7fffffffull) return hipErrorInvalidValue;
    const uint64_t jobs = entries * tiles;
    PacketRxArgs a{static_cast<const uint8_t *>(arena), table, depths, active, static_cast<uint8_t *>(dst), jobs, n_blocks, block_len, tiles};
    hipLaunchKernelGGL(packetrx_kernel, dim3((uint32_t)((jobs + kPacketJobsPerWg - 1) / kPacketJobsPerWg)), dim3(kPacketLanes * kPacketJobsPerWg), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi

// The launcher by itself on raw device pointers, on the null stream, waited for: NOT part of include/dspi.h and no interface.  It exists for
// tests/test_gpu_packets.py, which holds the kernel to the model at packet lengths that the calls refuse (a packet of several tiles).
extern "C" int dspi_packetrx_launch_raw(const void *arena, const uint64_t *table, const uint8_t *depths, void *dst, uint32_t n_streams, uint32_t n_blocks, uint32_t block_len) {
    hipError_t e = dspi::launch_packetrx(arena, table, depths, nullptr, dst, n_streams, n_blocks, block_len, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return (int)e;
}
