// dspi_meterbridge.hip — the meter bridge on the device (dspi_meters.h: the words and the rules): meter ballistics over a call's peaks, the
// alarm list, the status blocks of a range and REQ_CLEAR_CLIPS for a list.  The consumers of what the chain kernels leave; no chain state
// but the clip slots (cleared on request) is written.
//
// UPDATE   peaks = uint16 [n][K][C], meters = uint32 [n][C].  A workgroup serves G = 256 / C consecutive streams: lane t holds word t of the
//          workgroup's G C contiguous meter words, i.e. (stream t / C, channel t % C).  The streams' peaks are one contiguous span (K C 2 bytes
//          per stream, back to back): it comes into LDS with 16-byte loads, kMeterStagePackets packets at a time, in pieces that keep the low
//          four bits of their global address (dspi_meters.h meter_piece: the arithmetic, shared with the CPU driver that checks every index);
//          the vectors a piece only partly covers (its odd start and end) go element by element.  Then every lane walks its packets in LDS
//          and stores its word once.  A paused stream's lanes do nothing and none of its peaks is loaded.
// ALARMS   one lane per stream: its word (dspi_meters.h alarm_info) from the four clip slots and its C meter words.  Three launches: ballot and
//          popcount per wave -> a count per workgroup; an exclusive scan of the counts (one workgroup) and the total; the same words again, each
//          alarmed lane storing at its workgroup's offset + its rank.  No atomic: the list is ascending by construction.
// STATUS   one lane per stream reads the C peak slots and the four clip slots (consecutive streams of a row: coalesced), the blocks go through
//          LDS and out as consecutive 16-bit words.  CLEAR: one lane per (entry, slot).  Both address the state like dspi_status.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_meters.h"

namespace dspi {

namespace {

constexpr uint32_t kT = kMeterLanes;      // lanes per workgroup, every kernel here

__device__ inline bool bit_of(const uint32_t *bits, uint32_t s) { return !bits || (bits[s >> 5] >> (s & 31u) & 1u); }

// ---- update (the staging arithmetic is dspi_meters.h's: meter_geom, meter_chunk, meter_piece) ---------------------------------------------------
template <int C>
__global__ __launch_bounds__(kT) void meters_update_kernel(const uint16_t *peaks, uint32_t n, uint32_t K, uint32_t hold, uint32_t decay, uint32_t *meters, const uint32_t *active) {
    constexpr MeterGeom geom = meter_geom(C);
    __shared__ __attribute__((aligned(16))) uint8_t lds[geom.lds_bytes];
    const uint32_t t = threadIdx.x;
    const uint32_t s0 = blockIdx.x * geom.G, g = min(geom.G, n - s0);
    const uint32_t sl = t / C, ch = t % C;
    const bool mine = sl < g && bit_of(active, s0 + sl);
    const size_t word_at = (size_t)s0 * C + t;
    uint32_t word = mine ? meters[word_at] : 0u;
    const uint8_t *const src = reinterpret_cast<const uint8_t *>(peaks);
    const uint64_t base = reinterpret_cast<uintptr_t>(peaks);
    uint32_t level = meter_level(word), count = meter_count(word);
    for (uint32_t k0 = 0; k0 < K; k0 += kMeterStagePackets) {
        const MeterChunk chunk = meter_chunk(C, s0, g, K, k0);
        const uint32_t L = meter_piece_lanes(chunk);
        for (uint32_t piece = t / L; piece < chunk.n_pieces; piece += kT / L) {
            const MeterPiece pc = meter_piece(chunk, geom, base, piece);
            const uint8_t *const from = src + pc.origin;      // (dereferenced from the piece's first byte on only)
            uint8_t *const to = lds + pc.dst;
            // vector v of the piece: a whole one is loaded into r (the caller stores it, with several in flight); the others are done here
            auto stage = [&](uint32_t v, uint4 &r) -> bool {
                if (v * 16u >= pc.end) return false;
                bool all = meter_vec_whole(pc, v);
                if (all && active)      // (streams are at least 14 bytes long: a vector touches three at the most)
                    for (uint32_t s = meter_stream_of(chunk, pc, v * 16u), last = meter_stream_of(chunk, pc, v * 16u + 14u); s <= last; s++) all = all && bit_of(active, s);
                if (all) { r = *reinterpret_cast<const uint4 *>(from + v * 16u); return true; }
                for (uint32_t e = 0; e < 8u; e++) {      // a piece's odd start or end, or a vector with a paused stream in it: element by element
                    const uint32_t rel = v * 16u + 2u * e;
                    if (rel >= pc.lead && rel < pc.end && bit_of(active, meter_stream_of(chunk, pc, rel)))
                        *reinterpret_cast<uint16_t *>(to + rel) = *reinterpret_cast<const uint16_t *>(from + rel);
                }
                return false;
            };
            for (uint32_t v = t % L; v * 16u < pc.end; v += 4u * L) {      // four vectors a lane in flight
                uint4 r0, r1, r2, r3;
                const bool w0 = stage(v, r0), w1 = stage(v + L, r1), w2 = stage(v + 2u * L, r2), w3 = stage(v + 3u * L, r3);
                if (w0) *reinterpret_cast<uint4 *>(to + v * 16u) = r0;
                if (w1) *reinterpret_cast<uint4 *>(to + (v + L) * 16u) = r1;
                if (w2) *reinterpret_cast<uint4 *>(to + (v + 2u * L) * 16u) = r2;
                if (w3) *reinterpret_cast<uint4 *>(to + (v + 3u * L) * 16u) = r3;
            }
        }
        __syncthreads();
        if (mine) {
            const uint8_t *p = lds + meter_walk_at(chunk, geom, base, sl, ch);
            const uint32_t kc = min(kMeterStagePackets, K - k0);
            uint32_t k = 0;
            for (; k + 8u <= kc; k += 8u) {      // eight peaks on their way from LDS before the first is used
                uint32_t q[8];
#pragma unroll
                for (uint32_t j = 0; j < 8u; j++) q[j] = *reinterpret_cast<const uint16_t *>(p + (k + j) * C * 2u);
#pragma unroll
                for (uint32_t j = 0; j < 8u; j++) meter_step_lc(level, count, q[j], hold, decay);
            }
            for (; k < kc; k++) meter_step_lc(level, count, *reinterpret_cast<const uint16_t *>(p + k * C * 2u), hold, decay);
        }
        __syncthreads();
    }
    word = meter_word(level, count);
    if (mine) meters[word_at] = word;
}

// ---- alarms -------------------------------------------------------------------------------------------------------------------------------
struct ClipAt { const uint32_t *state; uint32_t row, n_slots, clip_slot; };
__device__ inline uint32_t clip_of(const ClipAt &a, uint32_t s) {
    const uint32_t wg = s / a.row, col = s % a.row;
    const uint32_t *p = a.state + ((size_t)wg * a.n_slots + a.clip_slot) * a.row + col;      // consecutive streams of a row: coalesced
    return (p[0] | p[a.row] | p[2 * (size_t)a.row] | p[3 * (size_t)a.row]) & 0xffffu;
}
template <int C>
__device__ inline uint32_t alarm_word(const ClipAt &a, const uint32_t *meters, uint32_t level, uint32_t n) {
    const uint32_t s = blockIdx.x * kT + threadIdx.x;
    return s < n ? alarm_info(meters ? meters + (size_t)s * C : nullptr, C, level, clip_of(a, s)) : 0u;
}
// the alarmed lanes of the workgroup in front of this one (`rank`), and how many it has in all
__device__ inline uint32_t rank_in_workgroup(bool alarmed, uint32_t &count) {
    __shared__ uint32_t per_wave[kT / 64];
    const uint64_t ballot = __ballot(alarmed);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) per_wave[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    count = 0;
    for (uint32_t w = 0; w < kT / 64; w++) { if (w < wave) rank += per_wave[w]; count += per_wave[w]; }
    return rank;
}

template <int C>
__global__ __launch_bounds__(kT) void alarm_count_kernel(ClipAt a, const uint32_t *meters, uint32_t level, uint32_t n, uint32_t *counts) {
    uint32_t count;
    (void)rank_in_workgroup(alarm_word<C>(a, meters, level, n) != 0u, count);
    if (threadIdx.x == 0) counts[blockIdx.x] = count;
}

// offsets[i] = counts[0] + .. + counts[i - 1]; *total = the sum of all
__global__ __launch_bounds__(kT) void alarm_scan_kernel(const uint32_t *counts, uint32_t n_counts, uint32_t *offsets, uint32_t *total) {
    __shared__ uint32_t sum[2][kT];
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < n_counts; i0 += kT) {
        const uint32_t i = i0 + threadIdx.x, mine = i < n_counts ? counts[i] : 0u;
        uint32_t cur = 0;
        sum[0][threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < kT; d <<= 1, cur ^= 1u) {      // inclusive, doubling
            sum[cur ^ 1u][threadIdx.x] = sum[cur][threadIdx.x] + (threadIdx.x >= d ? sum[cur][threadIdx.x - d] : 0u);
            __syncthreads();
        }
        if (i < n_counts) offsets[i] = carry + sum[cur][threadIdx.x] - mine;
        carry += sum[cur][kT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int C>
__global__ __launch_bounds__(kT) void alarm_write_kernel(ClipAt a, const uint32_t *meters, uint32_t level, uint32_t n, const uint32_t *offsets, uint32_t *streams, uint32_t *info, uint32_t cap) {
    const uint32_t w = alarm_word<C>(a, meters, level, n);
    uint32_t count;
    const uint32_t rank = rank_in_workgroup(w != 0u, count);
    const uint64_t at = (uint64_t)offsets[blockIdx.x] + rank;
    if (w != 0u && at < cap) {
        streams[at] = blockIdx.x * kT + threadIdx.x;
        if (info) info[at] = w;
    }
}

// ---- status blocks and REQ_CLEAR_CLIPS by list ----------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kT) void status_gather_kernel(ClipAt a, uint32_t peaks_slot, uint32_t first, uint32_t count, uint8_t *out) {
    constexpr uint32_t W = C + 2;      // 16-bit words of a block
    __shared__ uint16_t blocks[kT * W];
    const uint32_t i0 = blockIdx.x * kT, i = i0 + threadIdx.x;
    if (i < count) {
        const uint32_t s = first + i, wg = s / a.row, col = s % a.row;
        const uint32_t *p = a.state + ((size_t)wg * a.n_slots + peaks_slot) * a.row + col;
        for (uint32_t c = 0; c < (uint32_t)C; c++) blocks[threadIdx.x * W + c] = (uint16_t)p[c * (size_t)a.row];
        blocks[threadIdx.x * W + C] = 0;      // cpu0_load / cpu1_load: no MCU here
        blocks[threadIdx.x * W + C + 1] = (uint16_t)clip_of(a, s);
    }
    __syncthreads();
    const uint32_t n_words = min(kT, count - i0) * W;
    uint8_t *const dst = out + (size_t)i0 * W * 2u;
    if (reinterpret_cast<uintptr_t>(out) & 1u)
        for (uint32_t j = threadIdx.x; j < n_words; j += kT) { dst[2 * j] = (uint8_t)(blocks[j] & 0xffu); dst[2 * j + 1] = (uint8_t)(blocks[j] >> 8); }
    else
        for (uint32_t j = threadIdx.x; j < n_words; j += kT) reinterpret_cast<uint16_t *>(dst)[j] = blocks[j];
}

__global__ __launch_bounds__(kT) void clip_clear_kernel(uint32_t *state, const uint32_t *list, uint32_t n_list, uint32_t row, uint32_t n_slots, uint32_t clip_slot) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= (uint64_t)n_list * 4u) return;
    const uint32_t s = list[i >> 2], k = (uint32_t)(i & 3u);
    state[((size_t)(s / row) * n_slots + clip_slot + k) * row + s % row] = 0u;
}

template <class F>
hipError_t for_channels(int n_ch, F f) {
    if (n_ch == 11) f(std::integral_constant<int, 11>{});
    else if (n_ch == 7) f(std::integral_constant<int, 7>{});
    else return hipErrorNotSupported;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_meters_update(int n_ch, const uint16_t *peaks, uint32_t n, uint32_t n_blocks, uint32_t hold, uint32_t decay, uint32_t *meters, const uint32_t *active, hipStream_t stream) {
    return for_channels(n_ch, [&](auto c) {
        constexpr int C = decltype(c)::value;
        hipLaunchKernelGGL(meters_update_kernel<C>, dim3((n + meter_geom(C).G - 1u) / meter_geom(C).G), dim3(kT), 0, stream, peaks, n, n_blocks, hold, decay, meters, active);
    });
}

hipError_t launch_meters_alarms(int n_ch, const uint32_t *state, uint32_t n, uint32_t row, uint32_t n_slots, uint32_t clip_slot, const uint32_t *meters, uint32_t level,
                                uint32_t *scratch, uint32_t *streams, uint32_t *info, uint32_t cap, uint32_t *total, hipStream_t stream) {
    const uint32_t n_wg = meters_alarm_workgroups(n);
    const ClipAt a{state, row, n_slots, clip_slot};
    return for_channels(n_ch, [&](auto c) {
        constexpr int C = decltype(c)::value;
        hipLaunchKernelGGL(alarm_count_kernel<C>, dim3(n_wg), dim3(kT), 0, stream, a, meters, level, n, scratch);
        hipLaunchKernelGGL(alarm_scan_kernel, dim3(1), dim3(kT), 0, stream, scratch, n_wg, scratch + n_wg, total);
        hipLaunchKernelGGL(alarm_write_kernel<C>, dim3(n_wg), dim3(kT), 0, stream, a, meters, level, n, scratch + n_wg, streams, info, cap);
    });
}

hipError_t launch_status_gather(int n_ch, const uint32_t *state, uint32_t first, uint32_t count, uint32_t row, uint32_t n_slots, uint32_t peaks_slot, uint32_t clip_slot, void *out,
                                hipStream_t stream) {
    const ClipAt a{state, row, n_slots, clip_slot};
    return for_channels(n_ch, [&](auto c) {
        constexpr int C = decltype(c)::value;
        hipLaunchKernelGGL(status_gather_kernel<C>, dim3((count + kT - 1u) / kT), dim3(kT), 0, stream, a, peaks_slot, first, count, static_cast<uint8_t *>(out));
    });
}

hipError_t launch_clip_clear(uint32_t *state, const uint32_t *list, uint32_t n_list, uint32_t row, uint32_t n_slots, uint32_t clip_slot, hipStream_t stream) {
    hipLaunchKernelGGL(clip_clear_kernel, dim3((uint32_t)(((uint64_t)n_list * 4u + kT - 1u) / kT)), dim3(kT), 0, stream, state, list, n_list, row, n_slots, clip_slot);
    return hipGetLastError();
}

}  // namespace dspi
