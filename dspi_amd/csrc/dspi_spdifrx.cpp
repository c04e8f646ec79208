// dspi_spdifrx.cpp — S/PDIF input: the receiver for one line on the CPU and the layout of dspi_process_sources (dspi_spdifrx.h).
#include "dspi_spdifrx.h"

#include <string.h>

namespace dspi {

void spdifrx_line_cpu(SpdifRx *rx, const void *words, uint64_t frames, int32_t *pairs, uint8_t *packed) {
    const uint8_t *in = static_cast<const uint8_t *>(words);
    bool any_ok = false;
    auto lose = [&]() { rx->sync = 0; rx->sample_rate = 0; };
    for (uint64_t f = 0; f < frames; f++) {
        uint32_t w[4];
        memcpy(w, in + f * kRxFrameBytes, sizeof w);
        const bool ok[2] = {rx_left_ok(w[0], w[1]), rx_right_ok(w[2], w[3])};
        const uint32_t data[2] = {rx_data(w[0], w[1]), rx_data(w[2], w[3])};
        any_ok = any_ok || ok[0] || ok[1];
        // 1. sync
        if (ok[0] && (w[0] & 0xffu) == kPreZ) {
            if (rx->sync != 1) rx->parity_err_count = 0;      // a lock or a re-lock
            rx->sync = 1;
        } else if (!ok[0] || rx->sync == 1) lose();            // malformed, or X where Z is expected
        if (!ok[1]) lose();
        // 2. each side
        int32_t out[2];
        for (int side = 0; side < 2; side++) {
            if (!ok[side]) rx->coding_errors++;
            else if (rx_parity_fails(data[side])) rx->parity_err_count++;      // counted only: the sample passes
            if (!ok[side] || rx_v(data[side])) { out[side] = rx->hold[side]; rx->held++; }
            else out[side] = rx->hold[side] = rx_sample(data[side]);
        }
        // 3. the channel status
        if (rx->sync) {
            const uint32_t p = rx->sync - 1;
            if (p < kRxStatusBits) rx->c_bits[p / 8] = (uint8_t)((rx->c_bits[p / 8] & ~(1u << p % 8)) | (uint32_t)rx_c(data[0]) << p % 8);
            if (p == 31) rx->sample_rate = rx_rate(rx->c_bits[3]);
            rx->sync = 1 + (p + 1) % kRxBlock;
        }
        if (pairs) { pairs[2 * f] = out[0]; pairs[2 * f + 1] = out[1]; }
        if (packed)
            for (int side = 0; side < 2; side++)
                for (int b = 0; b < 3; b++) packed[6 * f + 3 * side + b] = (uint8_t)((uint32_t)out[side] >> 8 * b);
    }
    rx->state = rx->sync ? 2u : any_ok ? 1u : 0u;
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
