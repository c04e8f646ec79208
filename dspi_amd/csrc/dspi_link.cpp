// dspi_link.cpp — chained devices: what is refused about a view and its links, and the reader for one link on the CPU (dspi_link.h).
#include "dspi_link.h"

#include <vector>

namespace dspi {

uint64_t link_view_lines(const WireView &v) { return (uint64_t)v.n_streams * v.n_pairs; }

bool link_view_words(const WireView &v, uint64_t *words) {
    // stream-major: every line's region; tiled: every tile's regions, the last tile whole
    const uint64_t R = v.tile_streams, regions = R ? ((uint64_t)v.n_streams + R - 1) / R * v.n_pairs : link_view_lines(v);
    uint64_t w = 0;
    if (__builtin_mul_overflow(regions, (uint64_t)v.n_frames * 4u, &w) || (R && __builtin_mul_overflow(w, R, &w)) || w > UINT64_MAX / 4u) return false;
    if (words) *words = w;
    return true;
}

const char *link_view_why(const WireView &v, uint64_t frames, bool device) {
    if (!v.wire) return "the view's wire is NULL";
    if (device && reinterpret_cast<uintptr_t>(v.wire) % 16u) return "the view's wire is device memory and 16-byte aligned";
    if (v.n_pairs != 2 && v.n_pairs != 4) return "the view's n_pairs is 2 or 4";
    if (v.tile_streams != 0 && v.tile_streams != 64 && v.tile_streams != 128) return "the view's tile_streams is 0, 64 or 128";
    if (v.n_streams == 0) return "the view has no streams";
    if (frames ? v.n_frames != frames : v.n_frames == 0) return frames ? "the view's n_frames is not n_blocks * block_len" : "the view has no frames";
    if (!link_view_words(v, nullptr)) return "the view's size overflows";
    return nullptr;
}

uint32_t links_check(const Link *links, uint32_t n, uint64_t lines, const uint8_t *active, bool none_ok) {
    for (uint32_t i = 0; i < n; i++) {
        if (active && !active[i]) continue;
        const Link &l = links[i];
        if (l.kind == kLinkNone && none_ok) continue;
        if ((l.kind != kLinkSpdif && l.kind != kLinkI2s) || l.line >= lines) return i;
    }
    return n;
}

bool links_any(const Link *links, uint32_t n, const uint8_t *active, uint32_t kind) {
    for (uint32_t i = 0; i < n; i++)
        if ((!active || active[i]) && links[i].kind == kind) return true;
    return false;
}

void link_decode_cpu(const WireView &v, const Link &lk, SpdifRx *rx, int32_t *pairs, uint8_t *packed) {
    const uint64_t F = v.n_frames, L = lk.line;
    const uint32_t P = v.n_pairs, R = v.tile_streams, c = R ? link_column(L, P, R) : 0u;
    const uint32_t *const region = v.wire + (R ? link_region_tiled(L, P, R, F) : link_region(L, F));
    if (lk.kind == kLinkSpdif) {      // the line's frames where they lie, then the receiver as it is
        std::vector<uint32_t> line(4 * F);
        for (uint64_t f = 0; f < F; f++)
            for (uint32_t j = 0; j < 4; j++) line[4 * f + j] = region[R ? link_spdif_word_tiled(f, j, R, c) : link_spdif_word(f, j)];
        spdifrx_line_cpu(rx, line.data(), F, pairs, packed);
    } else if (lk.kind == kLinkI2s) {
        for (uint64_t f = 0; f < F; f++)
            for (uint32_t side = 0; side < 2; side++) {
                const int32_t x = link_i2s_sample(region[R ? link_i2s_word_tiled(f, side, F, R, c) : link_i2s_word(f, side)]);
                if (pairs) pairs[2 * f + side] = x;
                if (packed)
                    for (int b = 0; b < 3; b++) packed[6 * f + 3 * side + b] = (uint8_t)((uint32_t)x >> 8 * b);
            }
    }
}

}  // namespace dspi
