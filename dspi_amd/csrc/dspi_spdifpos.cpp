// dspi_spdifpos.cpp — per-stream S/PDIF block positions: see dspi_spdifpos.h.
#include "dspi_spdifpos.h"

namespace dspi {

void SpdifPos::enable(uint32_t n_streams, uint32_t pos) {
    if (on) return;
    on = true; dirty = true; clock = 0;
    word.assign(n_streams, pos % kSpdifBlock);      // T = 0: an offset and a frozen position are the same number
}

void SpdifPos::disable() {
    on = false; dirty = false; clock = 0;
    word.clear(); word.shrink_to_fit();
}

void SpdifPos::pause(uint32_t first, uint32_t count, const uint8_t *active) {
    for (uint32_t s = first; s < first + count; s++)
        if (is_active(s, active)) put(s, get(s, active), false);
}

void SpdifPos::resume(uint32_t first, uint32_t count, const uint8_t *active) {
    for (uint32_t s = first; s < first + count; s++)
        if (!is_active(s, active)) put(s, word[s], true);
}

void SpdifPos::move(const StreamMove *moves, uint32_t n, const uint8_t *active) {
    // every source is read before any slot is written
    struct Arrival { uint32_t pos; bool act; };
    std::vector<Arrival> in(n);
    std::vector<uint8_t> is_dst(word.size(), 0);
    for (uint32_t i = 0; i < n; i++) {
        in[i] = Arrival{get(moves[i].src, active), is_active(moves[i].src, active)};
        is_dst[moves[i].dst] = 1;
    }
    for (uint32_t i = 0; i < n; i++)
        if (moves[i].src != moves[i].dst && !is_dst[moves[i].src]) put(moves[i].src, in[i].pos, false);      // the open end: a frozen copy
    for (uint32_t i = 0; i < n; i++)
        if (moves[i].src != moves[i].dst) put(moves[i].dst, in[i].pos, in[i].act);
}

void SpdifPos::boot(const uint32_t *streams, uint32_t n, const uint8_t *active) {
    for (uint32_t i = 0; i < n; i++) set(streams[i], 0, active);
}

}  // namespace dspi
