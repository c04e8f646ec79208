// dspi_pdm.hip — DSPi's PDM sub output on the GPU: 256x oversampled 2nd-order sigma-delta modulator with noise-shaped
// dither, the consumer of the chain's Q28 sub channel (reference firmware/DSPi/pdm_generator.c).
//
// Per input sample (reference lines):  hard limiter :351-354, fade-in :356-360, target :363, then 8 chunks of
// { xorshift32 dither :62-68/:368, noise shaper :79-108/:369, 32 modulator steps MSB first :371-378 }, leaky
// integrators :396-397.  Integer arithmetic only, every add/sub/mul wrapping mod 2^32 like the Cortex-M code, so the
// words are bit-exact against the CPU restatement the tests use.  The DMA pacing and under-run recovery of the
// firmware loop are transport, not sample arithmetic, and are not modelled; its fade-out on disable (:223-237,
// :323-348) is dspi_process_pdm's in the dspi_pdm_fade mode (pdm_list_kernel<TILED, true> below).
//
// Mapping: one lane = one stream (the modulator is a 256-step serial recurrence per sample; the only parallelism is
// streams).  A workgroup is one tile row of the context (128 float / 64 Q28 streams): with the tiled layouts every
// access is one coalesced row ([tile][frame][R] in, [tile][frame][8][R] out).  VALU-issue bound: ~2 800 integer
// instructions per sample; 32 bytes out per 4 bytes in.
//
// Paused streams (dspi_pause_streams): a lane whose stream's bit in the activity bitmap is clear returns before it reads anything — its
// modulator state stays frozen, its `sub` is not read and its `words` are not written (both layouts).  No bitmap (null): every stream runs.
//
// dspi_process_pdm runs the same per-sample body over a LIST of streams (pdm_list_kernel): only the devices whose sub output is on cost lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_pdmfade.h"      // (the aux words' bits)

namespace dspi {

namespace {

constexpr int32_t kClip = 29500;          // PDM_CLIP_THRESH (config.h:64)
constexpr uint32_t kDitherMask = 0x1FF;   // PDM_DITHER_MASK (config.h:68)
constexpr int kLeak = 16;                 // PDM_LEAKAGE_SHIFT (config.h:71)
constexpr int kFadeShift = 10;            // PDM_FADE_IN_SHIFT (config.h:74)

__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
__device__ __forceinline__ int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

// 256 threads = four waves = one per SIMD of a CU, 256 / row tile rows per workgroup: with two-wave workgroups the
// dispatcher put both workgroups of a CU on the same two SIMDs and left the other two idle (measured: exactly 2x).
constexpr int kPdmThreads = 256;

// A modulator's nine words in registers, and the one statement of the per-sample arithmetic: both kernels below load the words, run
// pdm_samples over their stream's frames and store the words back.
struct PdmRegs {
    int32_t err, err2, x1, x2, y1, y2, err_acc;
    uint32_t rng, fade;
};
__device__ __forceinline__ PdmRegs pdm_load(const uint32_t *gs, uint32_t row) {
    return PdmRegs{(int32_t)gs[0 * row], (int32_t)gs[1 * row], (int32_t)gs[2 * row], (int32_t)gs[3 * row], (int32_t)gs[4 * row], (int32_t)gs[5 * row],
                   (int32_t)gs[6 * row], gs[7 * row], gs[8 * row]};
}
__device__ __forceinline__ void pdm_store(uint32_t *gs, uint32_t row, const PdmRegs &r) {
    gs[0 * row] = (uint32_t)r.err; gs[1 * row] = (uint32_t)r.err2;
    gs[2 * row] = (uint32_t)r.x1; gs[3 * row] = (uint32_t)r.x2; gs[4 * row] = (uint32_t)r.y1; gs[5 * row] = (uint32_t)r.y2; gs[6 * row] = (uint32_t)r.err_acc;
    gs[7 * row] = r.rng; gs[8 * row] = r.fade;
}

// Where a lane's samples come from.  The call's `sub` words: the stream's first sample, frames at stride `step` ...
struct PdmSubWords {
    const int32_t *in; size_t step;
    __device__ __forceinline__ int32_t operator()(uint32_t f) const { return in[(size_t)f * step]; }
};
// ... or, for a lane that fades out (dspi_pdm_fade; pdm_generator.c:326-327), the ramp itself: frame f plays position p - 1 - f of the base,
// v = (base * pos) >> 10, handed over as v << 14 — with |v| <= 29500 and the fade-in word held at 1024 the sample arithmetic below makes
// target = v + 32768 of it, the firmware's.  Such a lane reads no `sub`.  (A select per sample: fade and normal lanes share their waves.)
struct PdmFadeWords {
    const int32_t *in; size_t step; int32_t base; uint32_t p; bool fading;
    __device__ __forceinline__ int32_t operator()(uint32_t f) const {
        if (!fading) return in[(size_t)f * step];
        return (int32_t)((uint32_t)((base * (int32_t)(p - 1u - f)) >> kFadeShift) << 14);
    }
};

// `src(f)`: the stream's sample of frame f; `out`: its first word; TILED: the 8 words of a frame at stride row, frames at 8 rows
template <bool TILED, class Src>
__device__ __forceinline__ void pdm_samples_from(PdmRegs &r, const Src &src, uint32_t *out, uint32_t n_frames, uint32_t row) {
    int32_t err = r.err, err2 = r.err2, x1 = r.x1, x2 = r.x2, y1 = r.y1, y2 = r.y2, err_acc = r.err_acc;
    uint32_t rng = r.rng, fade = r.fade;
    const size_t out_step = TILED ? row : 1;

    int32_t next = n_frames ? src(0) : 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const int32_t sample = next;
        if (f + 1 < n_frames) next = src(f + 1);      // the next sample lands under 2 800 instructions
        int32_t pcm = sample >> 14;
        pcm = pcm > kClip ? kClip : pcm;
        pcm = pcm < -kClip ? -kClip : pcm;
        if (fade < (1u << kFadeShift)) { pcm = wmul(pcm, (int32_t)fade) >> kFadeShift; ++fade; }
        const int32_t target = pcm + 32768;
        uint32_t w[8];
#pragma unroll
        for (int chunk = 0; chunk < 8; ++chunk) {
            rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5;                         // fast_rand
            const int32_t raw = (int32_t)(rng & kDitherMask) - (int32_t)(kDitherMask >> 1);
            err_acc = wadd(wmul(err_acc, 248) >> 8, (err2 >> 8) >> 6);                   // noise_shaped_dither
            const int32_t input = wsub(raw, err_acc);
            int32_t acc = wmul(15778, input);
            acc = wadd(acc, wmul(-31556, x1));
            acc = wadd(acc, wmul(15778, x2));
            acc = wadd(acc, wmul(31531, y1));
            acc = wsub(acc, wmul(15580, y2));
            const int32_t dither = acc >> 14;
            x2 = x1; x1 = input; y2 = y1; y1 = dither;
            // 32 modulator steps (pdm_generator.c:371-378), five instructions each instead of the literal ten:
            //   fb = bit ? 65535 : 0;  err += target - fb;  err2 += err - fb;  bit = (err2 + dither >= 0)
            // with n = (err2 + dither) >> 31 (-1 for a 0 bit), fbn = n & 65535 = 65535 - fb, and the shifted variables
            // e = err - 65535, u = err2 + dither (dither is constant inside a chunk):
            //   e += (target - 65535) + fbn;   u += e + fbn;   word = 2*word + n   (= the bits minus 2^32-1, fixed up below)
            // Same values mod 2^32 at every step, so the words and the carried state are identical.
            const uint32_t tm = (uint32_t)target - 65535u;
            uint32_t e = (uint32_t)err - 65535u, u = (uint32_t)err2 + (uint32_t)dither, wacc = 0;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const uint32_t n = (uint32_t)((int32_t)u >> 31);
                const uint32_t fbn = n & 65535u;
                wacc = (wacc << 1) + n;
                e = e + tm + fbn;
                u = u + e + fbn;
            }
            const uint32_t word = wacc - 1u;
            err = (int32_t)(e + 65535u);
            err2 = (int32_t)(u - (uint32_t)dither);
            w[chunk] = word;
        }
        err = wsub(err, err >> kLeak);
        err2 = wsub(err2, err2 >> kLeak);
        uint32_t *o = out + (size_t)f * 8 * out_step;
        if (TILED) {
#pragma unroll
            for (int chunk = 0; chunk < 8; ++chunk) o[(size_t)chunk * row] = w[chunk];
        } else {
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<u4 *>(o) = u4{w[0], w[1], w[2], w[3]};
            *reinterpret_cast<u4 *>(o + 4) = u4{w[4], w[5], w[6], w[7]};
        }
    }
    r = PdmRegs{err, err2, x1, x2, y1, y2, err_acc, rng, fade};
}
// `in`: the stream's first sample; TILED: frames at stride row
template <bool TILED>
__device__ __forceinline__ void pdm_samples(PdmRegs &r, const int32_t *in, uint32_t *out, uint32_t n_frames, uint32_t row) {
    pdm_samples_from<TILED>(r, PdmSubWords{in, TILED ? (size_t)row : (size_t)1}, out, n_frames, row);
}

template <bool TILED>
__global__ __launch_bounds__(kPdmThreads) void pdm_kernel(uint32_t *state, const int32_t *sub, uint32_t *words, uint32_t n_streams, uint32_t n_frames,
                                                           uint32_t row, const uint32_t *active) {
    const uint32_t wg = blockIdx.x * (kPdmThreads / row) + threadIdx.x / row, col = threadIdx.x % row;
    const uint32_t stream = wg * row + col;
    if (stream >= n_streams) return;
    if (active && !((active[stream >> 5] >> (stream & 31u)) & 1u)) return;
    uint32_t *gs = state + (size_t)wg * kPdmStateWords * row + col;
    PdmRegs r = pdm_load(gs, row);
    const int32_t *in = TILED ? sub + (size_t)wg * n_frames * row + col : sub + (size_t)stream * n_frames;
    uint32_t *out = TILED ? words + (size_t)wg * n_frames * 8 * row + col : words + (size_t)stream * n_frames * 8;
    pdm_samples<TILED>(r, in, out, n_frames, row);
    pdm_store(gs, row, r);
}

// The modulator over a list (dspi_process_pdm; dspi_pdmlife.h): lane g of the grid serves the stream in list[g], so the launch costs the
// lanes of the streams that run their modulator, whatever the context's size.  Bit 31 of the word (kPdmListReset): the lane starts from
// the re-enable state (pdm_generator.c:241-252: the power-on words, the RNG running on) instead of the stored words — the reset is part
// of this launch.  The list is ascending, so the lanes of a fully listed row read and write whole rows as pdm_kernel's do.  `sub` and
// `words` are addressed by absolute stream in the call's layout; an unlisted stream's state, sub and words are not touched.
//
// FADE (dspi_pdm_fade on; dspi_pdmfade.h): lane g also loads its aux word and its stream's fade base.  A fade lane plays the ramp from
// (base, p) for as long as it lasts and writes zero words for the rest of the call; a cancel lane takes fade-in position 1024 - p first; every
// lane that modulated normally stores its new base — the pcm value of its last frame, after the limiter and the fade-in scaling
// (pdm_generator.c:352-362), from the call's last `sub` word and the fade-in position that frame met.  Without FADE the kernel takes an
// empty struct and is the kernel it was.
template <bool FADE> struct PdmFadeArgs {};
template <> struct PdmFadeArgs<true> {
    const uint32_t *aux;      // [n_list], beside `list`; null: every word is 0
    int32_t *base;            // [stream]
};
template <bool TILED, bool FADE>
__global__ __launch_bounds__(kPdmThreads) void pdm_list_kernel(uint32_t *state, const int32_t *sub, uint32_t *words, const uint32_t *list, uint32_t n_list,
                                                                uint32_t n_streams, uint32_t n_frames, uint32_t row, PdmFadeArgs<FADE> fx) {
    const uint32_t g = blockIdx.x * kPdmThreads + threadIdx.x;
    if (g >= n_list) return;
    const uint32_t word = list[g], stream = word & 0x7fffffffu;
    if (stream >= n_streams) return;
    const uint32_t wg = stream / row, col = stream % row;
    uint32_t *gs = state + (size_t)wg * kPdmStateWords * row + col;
    PdmRegs r = pdm_load(gs, row);
    if (word >> 31)      // (selects, not a branch: reset and carried lanes share their waves)
        r = PdmRegs{(int32_t)pdm_power_on_word(0), (int32_t)pdm_power_on_word(1), (int32_t)pdm_power_on_word(2), (int32_t)pdm_power_on_word(3),
                    (int32_t)pdm_power_on_word(4), (int32_t)pdm_power_on_word(5), (int32_t)pdm_power_on_word(6), r.rng, pdm_power_on_word(8)};
    const int32_t *in = TILED ? sub + (size_t)wg * n_frames * row + col : sub + (size_t)stream * n_frames;
    uint32_t *out = TILED ? words + (size_t)wg * n_frames * 8 * row + col : words + (size_t)stream * n_frames * 8;
    if constexpr (!FADE) {
        pdm_samples<TILED>(r, in, out, n_frames, row);
    } else {
        const uint32_t a = fx.aux ? fx.aux[g] : 0u, p = a & kPdmAuxPos;
        const bool fading = (a & kPdmAuxFade) != 0;
        const size_t step = TILED ? (size_t)row : (size_t)1;
        if (a & kPdmAuxCancel) r.fade = (1u << kFadeShift) - p;      // pdm_generator.c:233-237: the samples the fade has played are the fade-in's to come
        const uint32_t fade_in = r.fade;
        uint32_t n_run = n_frames;
        if (fading) {      // positions p-1 .. 1, the fade-in position untouched
            const uint32_t left = p ? p - 1u : 0u;
            n_run = left < n_frames ? left : n_frames;
            r.fade = 1u << kFadeShift;
        }
        pdm_samples_from<TILED>(r, PdmFadeWords{in, step, fx.base[stream], p, fading}, out, n_run, row);
        if (fading) {
            r.fade = fade_in;
            for (uint32_t f = n_run; f < n_frames; ++f) {      // the fade is over: the stream is listed, so nobody else zeroes these
                uint32_t *o = out + (size_t)f * 8 * step;
#pragma unroll
                for (int chunk = 0; chunk < 8; ++chunk) o[(size_t)chunk * step] = 0u;
            }
        } else {
            int32_t pcm = in[(size_t)(n_frames - 1u) * step] >> 14;
            pcm = pcm > kClip ? kClip : pcm;
            pcm = pcm < -kClip ? -kClip : pcm;
            const uint32_t full = 1u << kFadeShift;
            const uint32_t met = (fade_in >= full || n_frames - 1u >= full - fade_in) ? full : fade_in + (n_frames - 1u);      // the last frame's fade-in position
            if (met < full) pcm = wmul(pcm, (int32_t)met) >> kFadeShift;
            fx.base[stream] = pcm;
        }
    }
    pdm_store(gs, row, r);
}

// the fade bases of listed slots into a packed buffer, and a packed buffer (null: zeros) into listed slots: one thread per entry.  A base
// travels with its stream through the packed temporary, so swaps and cycles are safe.
__global__ void pdm_base_gather_kernel(const int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, int32_t *packed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i];
    packed[i] = s < n_streams ? base[s] : 0;
}
__global__ void pdm_base_scatter_kernel(int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, const int32_t *packed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i];
    if (s < n_streams) base[s] = packed ? packed[i] : 0;
}

// power-on (init != 0: pdm_power_on_word, dspi_kernels.h) or the re-enable path (pdm_generator.c:241-252: everything but the RNG)
__global__ void pdm_reset_kernel(uint32_t *state, uint32_t n_streams, uint32_t row, int32_t only_stream, int init) {
    const uint32_t wg = blockIdx.x, col = threadIdx.x;
    const uint32_t stream = wg * row + col;
    if (col >= row || stream >= n_streams || (only_stream >= 0 && stream != (uint32_t)only_stream)) return;
    uint32_t *gs = state + (size_t)wg * kPdmStateWords * row + col;
    for (int i = 0; i < kPdmStateWords; ++i)
        if (init || i != kPdmRngWord) gs[(size_t)i * row] = pdm_power_on_word(i);
}

}  // namespace

hipError_t launch_pdm(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, uint32_t n_streams, uint32_t n_frames, uint32_t row,
                      uint32_t n_wg, const uint32_t *active, hipStream_t stream) {
    const uint32_t per = kPdmThreads / row, blocks = (n_wg + per - 1) / per;
    if (tiled) hipLaunchKernelGGL(pdm_kernel<true>, dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, n_streams, n_frames, row, active);
    else hipLaunchKernelGGL(pdm_kernel<false>, dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, n_streams, n_frames, row, active);
    return hipGetLastError();
}

hipError_t launch_pdm_list(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, const uint32_t *list, uint32_t n_list, uint32_t n_streams,
                           uint32_t n_frames, uint32_t row, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    const uint32_t blocks = (n_list + kPdmThreads - 1) / kPdmThreads;
    const PdmFadeArgs<false> none{};
    if (tiled) hipLaunchKernelGGL((pdm_list_kernel<true, false>), dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, list, n_list, n_streams, n_frames, row, none);
    else hipLaunchKernelGGL((pdm_list_kernel<false, false>), dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, list, n_list, n_streams, n_frames, row, none);
    return hipGetLastError();
}

hipError_t launch_pdm_list_fade(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, const uint32_t *list, const uint32_t *aux, int32_t *base,
                                uint32_t n_list, uint32_t n_streams, uint32_t n_frames, uint32_t row, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    const uint32_t blocks = (n_list + kPdmThreads - 1) / kPdmThreads;
    const PdmFadeArgs<true> fx{aux, base};
    if (tiled) hipLaunchKernelGGL((pdm_list_kernel<true, true>), dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, list, n_list, n_streams, n_frames, row, fx);
    else hipLaunchKernelGGL((pdm_list_kernel<false, true>), dim3(blocks), dim3(kPdmThreads), 0, stream, state, sub, words, list, n_list, n_streams, n_frames, row, fx);
    return hipGetLastError();
}

hipError_t launch_pdm_base_gather(const int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, int32_t *packed, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pdm_base_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, base, slots, n, n_streams, packed);
    return hipGetLastError();
}

hipError_t launch_pdm_base_scatter(int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, const int32_t *packed, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pdm_base_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, base, slots, n, n_streams, packed);
    return hipGetLastError();
}

hipError_t launch_pdm_reset(uint32_t *state, uint32_t n_streams, uint32_t row, uint32_t n_wg, int32_t only_stream, int init, hipStream_t stream) {
    hipLaunchKernelGGL(pdm_reset_kernel, dim3(n_wg), dim3(128), 0, stream, state, n_streams, row, only_stream, init);
    return hipGetLastError();
}

}  // namespace dspi
