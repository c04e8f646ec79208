// dspi_wire_tiled.hip — the tiled wire encoder (dspi_wire.h: the tiled layout): the chain's TILED int24 pair words, [tile][output][F][R], into
// what each column's OWN driver shifts out, in the regions of the tiled subframes, [tile][pair][4 F rows][R]: IEC 60958 subframes for an
// S/PDIF slot (row f * 4 + j; dspi_spdif_dev.h, the encoder of dspi_spdif.hip) or left-justified I2S slot words for an I2S slot
// (pico_audio_i2s_multi/audio_i2s_multi.c:217-226; row side * F + f, the region's first half), by the output types of the column's own image.
//
// Mapping: workgroup = (tile, pair, slice of kFrameSlice frames), lane = column, as in dspi_spdif.hip's tiled encoder — every load and every
// store is one coalesced row of R words — but the workgroup is R lanes wide (64 for the Q28 tile: one full wave, no idle half).
// The type is per LANE: the lanes of a wave take different branches, each branch storing whole rows under its lanes' mask.  A lane loads its
// activity bit, its image index, its position and the words of its first frame in one group, then type and rate from the image (one dependent
// load), ONCE, and keeps them over its frame slice (profiles/wire.md §2 has what the stream-major kernel pays per lane for the same).
// Columns past the last stream and paused columns (rates.active) are neither read nor written.  With `zero_tails` (host-buffer paths) an I2S
// lane also stores zeros over rows 2 F .. 4 F - 1 of its column, two rows per frame.  No LDS, no scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_spdif_dev.h"

namespace dspi {

namespace {

constexpr uint32_t kFrameSlice = 32;
static_assert(kWireTiledMaxFrames == 65535u * kFrameSlice, "one frame slice per blockIdx.z");

// PS: per-stream positions as in dspi_spdif.hip — spos[absolute stream] mod 192 is added to block_pos.
template <uint32_t ROW, bool PS>
__global__ __launch_bounds__(ROW) void wire_tiled_kernel(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t block_pos,
                                                         uint32_t status_hi, SpdifRates rates, const uint32_t *spos, uint32_t zero_tails) {
    const uint32_t tile = blockIdx.x, pair = blockIdx.y, col = threadIdx.x;
    const uint32_t stream = tile * ROW + col;
    if (stream >= n_streams) return;
    const uint32_t s = rates.stream0 + stream;
    const size_t F = n_frames;
    const uint32_t f0 = blockIdx.z * kFrameSlice, f1 = min(n_frames, f0 + kFrameSlice);
    // outputs 2 * pair and 2 * pair + 1 are separate [frame][R] planes
    const int32_t *const inL = pairs + ((size_t)tile * (2 * n_pairs) + 2 * pair) * F * ROW + col, *const inR = inL + F * ROW;
    uint32_t *const region = out + ((size_t)tile * n_pairs + pair) * F * 4 * ROW + col;
    // one group of loads: whose column this is, and the words of its first frame (they stand at the same place whatever the type); the empty
    // asm statement keeps the words' loads beside the others instead of behind the wait for the image's line
    uint32_t act = rates.active ? rates.active[s >> 5] : ~0u, image = rates.stream_image[s], sp = PS ? spos[s] : 0u;
    uint32_t wl = (uint32_t)inL[(size_t)f0 * ROW], wr = (uint32_t)inR[(size_t)f0 * ROW];
    asm volatile("" : "+v"(act), "+v"(image), "+v"(sp), "+v"(wl), "+v"(wr));
    // a paused stream's words in the scratch are stale, and its column is not the call's to write
    if (!((act >> (s & 31u)) & 1u)) return;
    const DevImage &im = rates.img[image];
    const bool i2s = (im.i2s_pairs >> pair) & 1u;
    const uint32_t status_lo = spdif_status_lo(im.fs_hz);
    if (PS) block_pos += sp % 192u;
    uint32_t pos = (block_pos + f0) % 192u;
    for (uint32_t f = f0; f < f1; ++f) {
        const uint32_t l = wl, r = wr;
        if (f + 1 < f1) { wl = (uint32_t)inL[(size_t)(f + 1) * ROW]; wr = (uint32_t)inR[(size_t)(f + 1) * ROW]; }
        if (i2s) {
            region[(size_t)f * ROW] = l << 8;
            region[(F + f) * ROW] = r << 8;
            if (zero_tails) { uint32_t *const q = region + (2 * F + 2 * (size_t)f) * ROW; q[0] = 0u; q[ROW] = 0u; }
        } else {
            const spdif_u4 o = spdif_frame(l, r, pos, status_lo, status_hi);
            uint32_t *const q = region + (size_t)f * 4 * ROW;
            q[0] = o.x; q[ROW] = o.y; q[2 * ROW] = o.z; q[3 * ROW] = o.w;
        }
        pos = (pos + 1 == 192u) ? 0u : pos + 1;
    }
}

template <uint32_t ROW>
void launch(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t n_tiles, uint32_t block_pos, const SpdifRates &rates,
            const uint32_t *spos, bool zero_tails, hipStream_t stream) {
    const dim3 grid(n_tiles, n_pairs, (n_frames + kFrameSlice - 1) / kFrameSlice);
    if (spos) hipLaunchKernelGGL((wire_tiled_kernel<ROW, true>), grid, dim3(ROW), 0, stream, pairs, out, n_streams, n_pairs, n_frames, block_pos, kSpdifStatusHi, rates, spos, zero_tails ? 1u : 0u);
    else hipLaunchKernelGGL((wire_tiled_kernel<ROW, false>), grid, dim3(ROW), 0, stream, pairs, out, n_streams, n_pairs, n_frames, block_pos, kSpdifStatusHi, rates, spos, zero_tails ? 1u : 0u);
}

}  // namespace

hipError_t launch_wire_tiled(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t row, uint32_t n_tiles, uint32_t block_pos,
                             const SpdifRates &rates, bool zero_tails, hipStream_t stream, const uint32_t *stream_pos) {
    if (!rates.img || !rates.stream_image) return hipErrorInvalidValue;      // the types are each stream's own, as in launch_wire
    if (row != 64 && row != 128) return hipErrorInvalidValue;
    if ((uint64_t)n_streams > (uint64_t)n_tiles * row) return hipErrorInvalidValue;
    if (!n_streams || !n_pairs || !n_frames) return hipSuccess;
    if (n_frames > kWireTiledMaxFrames) return hipErrorInvalidValue;      // (the callers refuse such a call before anything runs)
    const uint32_t tiles = (n_streams + row - 1) / row;      // tiles behind the last stream hold nobody
    if (row == 64) launch<64>(pairs, out, n_streams, n_pairs, n_frames, tiles, block_pos, rates, stream_pos, zero_tails, stream);
    else launch<128>(pairs, out, n_streams, n_pairs, n_frames, tiles, block_pos, rates, stream_pos, zero_tails, stream);
    return hipGetLastError();
}

}  // namespace dspi
