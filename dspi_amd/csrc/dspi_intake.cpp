// dspi_intake.cpp — the input layout of dspi_process_mixed (dspi_intake.h).
#include "dspi_intake.h"

#include <string.h>

#include <algorithm>

namespace dspi {

uint32_t intake_check_depths(const uint8_t *depths, uint32_t n) {
    for (uint32_t s = 0; s < n; s++)
        if (!intake_frame_bytes(depths[s])) return s;
    return n;
}

uint8_t intake_uniform_depth(const uint8_t *depths, uint32_t n) {
    if (!n) return 0;
    for (uint32_t s = 1; s < n; s++)
        if (depths[s] != depths[0]) return 0;
    return depths[0];
}

bool intake_offsets(const uint8_t *depths, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets) {
    if (frames && (uint64_t)n > UINT64_MAX / kIntakeOutFrame / frames) return false;
    uint64_t at = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (offsets) offsets[s] = at;
        at += frames * intake_frame_bytes(depths[s]);
    }
    if (offsets) offsets[n] = at;
    if (total) *total = at;
    return true;
}

void intake_row_range(const uint64_t *offsets, uint32_t n, uint32_t row, uint32_t r0, uint32_t r1, uint64_t *begin, uint64_t *end) {
    const uint64_t s0 = std::min<uint64_t>((uint64_t)r0 * row, n), s1 = std::min<uint64_t>((uint64_t)r1 * row, n);
    *begin = offsets[s0];
    *end = offsets[std::max(s0, s1)];
}

void intake_widen_cpu(uint8_t *dst, const uint8_t *src, uint8_t depth, uint64_t frames) {
    if (depth == 24) { memcpy(dst, src, (size_t)(frames * 6)); return; }
    for (uint64_t k = 0; k < 2 * frames; k++) {      // one sample (a channel of a frame) at a time
        dst[3 * k] = 0; dst[3 * k + 1] = src[2 * k]; dst[3 * k + 2] = src[2 * k + 1];
    }
}

}  // namespace dspi
