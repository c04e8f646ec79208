// dspi_wire.hip — the wire encoder (dspi_wire.h: the layout): the chain's int24 pair words into what each pair's OWN driver shifts out,
// IEC 60958 subframes for an S/PDIF slot (dspi_spdif_dev.h, the encoder of dspi_spdif.hip) or left-justified I2S slot words
// (pico_audio_i2s_multi/audio_i2s_multi.c:217-226) for an I2S slot, by the output types of the stream's own image.
//
// Stream-major only; lane mapping of dspi_spdif.hip's stream-major encoders: one lane per frame pair (even frame counts) or per frame.
// The type is uniform over a (stream, pair) run of F/2 or F lanes, so a wave diverges at run boundaries only.  Every lane does one load
// (16 or 8 bytes) and, as an S/PDIF lane, stores 32 or 16 bytes of subframes; as an I2S lane 16 or 8 bytes of slot words at the START of
// the pair's region — contiguous over the run, as a DMA buffer wants them —, and only with `zero_tails` (host-buffer paths: the pinned
// area, a staged chunk's device buffer) zeros over its share of the region's second half.  No LDS, no scratch memory.
// The loads go out in two groups — the words, the stream's image index and its position; then type and rate from the image —, so the
// stores stand two round trips behind the launch, as in the S/PDIF encoder when it reads per-stream rates (profiles/wire.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_spdif_dev.h"

namespace dspi {

namespace {

typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// PS: per-stream positions as in dspi_spdif.hip — spos[absolute stream] mod 192 is added to block_pos.
// PAIR: two frames per lane; `lanes_per_run` = F / 2 then, else F.
template <bool PS, bool PAIR>
__device__ __forceinline__ void wire_lanes(const int32_t *pairs, uint32_t *out, uint64_t total, uint32_t lanes_per_run, uint32_t block_pos, uint32_t status_hi,
                                           const SpdifRates &rates, uint32_t n_pairs, const uint32_t *spos, uint32_t zero_tails) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;      // (stream * n_pairs + pair) * lanes_per_run + frame (pair)
    if (idx >= total) return;
    const uint64_t run = idx / lanes_per_run;                             // stream * n_pairs + pair
    const uint32_t k = (uint32_t)(idx - run * lanes_per_run);
    const uint32_t s = rates.stream0 + (uint32_t)(run / n_pairs), pair = (uint32_t)(run % n_pairs);
    // a paused stream's words in the scratch are stale, and its region is not the call's to write: nothing of it is read
    if (rates.active && !((rates.active[s >> 5] >> (s & 31u)) & 1u)) return;
    // The lane's words stand at the same place whatever the type, so their load is issued here, beside the stream's image index and its
    // position: the type and the rate then cost ONE dependent load (the image's line) behind them, not two in front of the words
    // (left alone the compiler sinks the words' load behind the wait for the index, and the rate's into the S/PDIF branch behind the type:
    //  three and four round trips in a row; the empty asm statements pin the two groups where they are written)
    uint32_t image = rates.stream_image[s], sp = PS ? spos[s] : 0u;
    u4 w;
    if (PAIR) w = *reinterpret_cast<const u4 *>(pairs + idx * 4);
    else { const u2 v = *reinterpret_cast<const u2 *>(pairs + idx * 2); w = u4{v.x, v.y, 0u, 0u}; }
    uint32_t w0 = w.x, w1 = w.y, w2 = w.z, w3 = w.w;
    asm volatile("" : "+v"(image), "+v"(sp), "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
    w = u4{w0, w1, w2, w3};
    if (PS) block_pos += sp % 192u;
    const DevImage &im = rates.img[image];
    uint32_t i2s_pairs = im.i2s_pairs, fs_hz = im.fs_hz;
    asm volatile("" : "+v"(i2s_pairs), "+v"(fs_hz));
    const uint32_t frames_per_lane = PAIR ? 2u : 1u;
    const uint64_t n_frames = (uint64_t)lanes_per_run * frames_per_lane;
    uint32_t *const region = out + run * n_frames * 4;                    // 16 bytes per frame
    if ((i2s_pairs >> pair) & 1u) {
        if (PAIR) {
            *reinterpret_cast<u4 *>(region + (size_t)k * 4) = u4{w.x << 8, w.y << 8, w.z << 8, w.w << 8};
            if (zero_tails) *reinterpret_cast<u4 *>(region + n_frames * 2 + (size_t)k * 4) = u4{0u, 0u, 0u, 0u};
        } else {
            *reinterpret_cast<u2 *>(region + (size_t)k * 2) = u2{w.x << 8, w.y << 8};
            if (zero_tails) *reinterpret_cast<u2 *>(region + n_frames * 2 + (size_t)k * 2) = u2{0u, 0u};
        }
        return;
    }
    const uint32_t status_lo = spdif_status_lo(fs_hz);
    const uint32_t f = k * frames_per_lane;
    if (PAIR) {
        const u4 o0 = spdif_frame(w.x, w.y, (block_pos + f) % 192u, status_lo, status_hi);
        const u4 o1 = spdif_frame(w.z, w.w, (block_pos + f + 1u) % 192u, status_lo, status_hi);
        *reinterpret_cast<u4 *>(region + (size_t)k * 8) = o0;
        *reinterpret_cast<u4 *>(region + (size_t)k * 8 + 4) = o1;
    } else {
        *reinterpret_cast<u4 *>(region + (size_t)k * 4) = spdif_frame(w.x, w.y, (block_pos + f) % 192u, status_lo, status_hi);
    }
}

template <bool PS, bool PAIR>
__global__ __launch_bounds__(256) void wire_kernel(const int32_t *pairs, uint32_t *out, uint64_t total, uint32_t lanes_per_run, uint32_t block_pos, uint32_t status_hi,
                                                   SpdifRates rates, uint32_t n_pairs, const uint32_t *spos, uint32_t zero_tails) {
    wire_lanes<PS, PAIR>(pairs, out, total, lanes_per_run, block_pos, status_hi, rates, n_pairs, spos, zero_tails);
}

template <bool PS, bool PAIR>
void launch(const int32_t *pairs, uint32_t *out, uint64_t total, uint32_t lanes_per_run, uint32_t block_pos, const SpdifRates &rates, uint32_t n_pairs, const uint32_t *spos,
            bool zero_tails, hipStream_t stream) {
    hipLaunchKernelGGL((wire_kernel<PS, PAIR>), dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, pairs, out, total, lanes_per_run, block_pos, kSpdifStatusHi, rates,
                       n_pairs, spos, zero_tails ? 1u : 0u);
}

}  // namespace

hipError_t launch_wire(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t block_pos, const SpdifRates &rates,
                       bool zero_tails, hipStream_t stream, const uint32_t *stream_pos) {
    if (!rates.img || !rates.stream_image) return hipErrorInvalidValue;      // the types are each stream's own: there is no "one image for everybody" form
    const uint64_t runs = (uint64_t)n_streams * n_pairs;
    if (!runs || !n_frames) return hipSuccess;
    if (n_frames % 2 == 0) {
        if (stream_pos) launch<true, true>(pairs, out, runs * (n_frames / 2), n_frames / 2, block_pos, rates, n_pairs, stream_pos, zero_tails, stream);
        else launch<false, true>(pairs, out, runs * (n_frames / 2), n_frames / 2, block_pos, rates, n_pairs, nullptr, zero_tails, stream);
    } else {
        if (stream_pos) launch<true, false>(pairs, out, runs * n_frames, n_frames, block_pos, rates, n_pairs, stream_pos, zero_tails, stream);
        else launch<false, false>(pairs, out, runs * n_frames, n_frames, block_pos, rates, n_pairs, nullptr, zero_tails, stream);
    }
    return hipGetLastError();
}

}  // namespace dspi
