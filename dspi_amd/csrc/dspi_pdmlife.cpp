// dspi_pdmlife.cpp — the PDM modulators' running bytes and the work list of a dspi_process_pdm call: see dspi_pdmlife.h.
#include "dspi_pdmlife.h"

#include <algorithm>

namespace dspi {

std::pair<size_t, size_t> PdmWork::range(uint32_t s0, uint32_t s1) const {
    auto below = [](uint32_t word, uint32_t s) { return (word & ~kPdmListReset) < s; };
    const size_t lo = (size_t)(std::lower_bound(list.begin(), list.end(), s0, below) - list.begin());
    const size_t hi = (size_t)(std::lower_bound(list.begin(), list.end(), s1, below) - list.begin());
    return {lo, hi};
}

const PdmWork &PdmLife::plan(const uint8_t *active, const std::function<bool(uint32_t)> &sub_on) {
    if (!dirty) return work;
    builds++;
    work = PdmWork();
    const uint32_t n = (uint32_t)running.size();
    for (uint32_t s = 0; s < n; s++) {
        const bool act = !active || active[s], on = act && sub_on(s);
        if (on) {
            work.list.push_back(running[s] ? s : s | kPdmListReset);
            if (!running[s]) work.resets = true;
            continue;
        }
        if (act && running[s]) work.stops.push_back(s);
        if (!work.unlisted.empty() && work.unlisted.back().second == s) work.unlisted.back().second = s + 1;
        else work.unlisted.emplace_back(s, s + 1);
    }
    dirty = false; uploaded = false;
    return work;
}

void PdmLife::commit() {
    for (uint32_t w : work.list) running[w & ~kPdmListReset] = 1;
    for (uint32_t s : work.stops) running[s] = 0;
    work.stops.clear();
    if (work.resets) mark_dirty();      // the next call's list has no such bits
}

void PdmLife::move(const StreamMove *moves, uint32_t n) {
    std::vector<uint8_t> in(n);      // every source is read before any slot is written
    for (uint32_t i = 0; i < n; i++) in[i] = running[moves[i].src];
    for (uint32_t i = 0; i < n; i++) running[moves[i].dst] = in[i];
    mark_dirty();
}

void PdmLife::boot(const uint32_t *streams, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) running[streams[i]] = 0;
    mark_dirty();
}

const char *PdmLife::set_get(uint32_t first, uint32_t count, const uint8_t *set, uint8_t *get) {
    if (count == 0 || (uint64_t)first + count > running.size()) return "stream range out of bounds";
    if (set) for (uint32_t k = 0; k < count; k++) if (set[k] > 1) return "a value is 0 or 1";
    if (set) { for (uint32_t k = 0; k < count; k++) running[first + k] = set[k]; mark_dirty(); }
    if (get) for (uint32_t k = 0; k < count; k++) get[k] = running[first + k];
    return nullptr;
}

}  // namespace dspi
