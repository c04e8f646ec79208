// dspi_spdifrx.cpp — S/PDIF input: the receiver for one line on the CPU and the layout of dspi_process_sources (dspi_spdifrx.h).
#include "dspi_spdifrx.h"

#include <string.h>

namespace dspi {

void spdifrx_line_cpu(SpdifRx *rx, const void *words, uint64_t frames, int32_t *pairs, uint8_t *packed) {
    const uint8_t *in = static_cast<const uint8_t *>(words);
    RxRegs r{rx->sync, rx->sample_rate, rx->parity_err_count, rx->held, rx->coding_errors, 0, rx->hold[0], rx->hold[1], false};
    memcpy(&r.cbits, rx->c_bits, 8);      // (the five status bytes and the padding behind them, which is kept)
    for (uint64_t f = 0; f < frames; f++) {
        uint32_t w[4];
        memcpy(w, in + f * kRxFrameBytes, sizeof w);
        int32_t out[2] = {0, 0};
        rx_frame(r, w[0], w[1], w[2], w[3], out[0], out[1]);
        if (pairs) { pairs[2 * f] = out[0]; pairs[2 * f + 1] = out[1]; }
        if (packed)
            for (int side = 0; side < 2; side++)
                for (int b = 0; b < 3; b++) packed[6 * f + 3 * side + b] = (uint8_t)((uint32_t)out[side] >> 8 * b);
    }
    rx->sync = r.sync; rx->sample_rate = r.rate; rx->parity_err_count = r.parity; rx->held = r.held; rx->coding_errors = r.coding;
    memcpy(rx->c_bits, &r.cbits, 8);
    rx->hold[0] = r.hold_l; rx->hold[1] = r.hold_r;
    rx->state = r.sync ? 2u : r.any_ok ? 1u : 0u;
}

uint32_t sources_check(const uint8_t *sources, uint32_t n) {
    for (uint32_t s = 0; s < n; s++)
        if (!source_frame_bytes(sources[s])) return s;
    return n;
}

bool sources_any_spdif(const uint8_t *sources, uint32_t n) {
    for (uint32_t s = 0; s < n; s++)
        if (sources[s] == kSrcSpdif) return true;
    return false;
}

bool sources_offsets(const uint8_t *sources, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets) {
    // (every run with 15 bytes in front of it still fits)
    if ((frames && (uint64_t)n > (UINT64_MAX - 15u * (uint64_t)n) / kRxFrameBytes / frames)) return false;
    uint64_t at = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (sources[s] == kSrcSpdif) at = (at + 15u) & ~(uint64_t)15;
        if (offsets) offsets[s] = at;
        at += frames * source_frame_bytes(sources[s]);
    }
    if (offsets) offsets[n] = at;
    if (total) *total = at;
    return true;
}

}  // namespace dspi
