// dspi_boot.cpp — see dspi_boot.h.
#include "dspi_boot.h"

#include <algorithm>

namespace dspi {

const char *boot_validate(const uint32_t *streams, uint32_t n, uint32_t n_streams) {
    if (!streams || n == 0) return "empty stream list";
    std::vector<uint8_t> seen(n_streams, 0);
    const SlotCheck c = check_slots(streams, 1, n, seen);
    return c == SlotCheck::out_of_range ? "stream index out of range" : c == SlotCheck::duplicate ? "a slot is listed twice" : nullptr;
}

std::vector<BootRowItem> boot_row_items(const uint32_t *streams, uint32_t n, uint32_t n_streams, uint32_t row_streams, const uint8_t *active, bool power_on_positions) {
    std::vector<uint32_t> sorted(streams, streams + n);
    std::sort(sorted.begin(), sorted.end());
    std::vector<BootRowItem> items;
    if (sorted.empty()) return items;
    std::vector<uint8_t> listed(((size_t)sorted.back() / row_streams + 1) * row_streams, 0);      // (every touched row whole)
    for (uint32_t s : sorted) {
        listed[s] = 1;
        const uint32_t row = s / row_streams, col = s % row_streams;
        if (items.empty() || items.back().row != row) items.push_back(BootRowItem{row, 0u, 0u, kBootNone, {0u, 0u, 0u, 0u}});
        items.back().cols[col / 32] |= 1u << (col % 32);
    }
    for (BootRowItem &it : items) {
        for (uint32_t q = 0; q < row_streams / 4; q++) {
            const uint32_t four = (it.cols[q / 8] >> (4 * (q % 8))) & 15u;
            if (four) it.q_any |= 1u << q;
            if (four == 15u) it.q_all |= 1u << q;
        }
        if (!power_on_positions) it.target = row_lowest_resident(it.row, row_streams, n_streams, active, listed.data());
    }
    return items;
}

}  // namespace dspi
