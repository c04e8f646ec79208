// dspi_boot.cpp — see dspi_boot.h.
#include "dspi_boot.h"

#include <algorithm>

namespace dspi {

const char *boot_validate(const uint32_t *streams, uint32_t n, uint32_t n_streams) {
    if (!streams || n == 0) return "empty stream list";
    for (uint32_t i = 0; i < n; i++)
        if (streams[i] >= n_streams) return "stream index out of range";
    std::vector<uint8_t> mark(n_streams, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (mark[streams[i]]) return "a slot is listed twice";
        mark[streams[i]] = 1;
    }
    return nullptr;
}

std::vector<BootRowItem> boot_row_items(const uint32_t *streams, uint32_t n, uint32_t n_streams, uint32_t row_streams, const uint8_t *active, bool power_on_positions) {
    std::vector<uint32_t> sorted(streams, streams + n);
    std::sort(sorted.begin(), sorted.end());
    std::vector<BootRowItem> items;
    for (uint32_t s : sorted) {
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
        if (power_on_positions) continue;
        const uint64_t r0 = (uint64_t)it.row * row_streams, r1 = std::min<uint64_t>(r0 + row_streams, n_streams);
        for (uint64_t s = r0; s < r1 && it.target == kBootNone; s++) {
            const uint32_t col = (uint32_t)(s - r0);
            if (!((it.cols[col / 32] >> (col % 32)) & 1u) && (!active || active[s])) it.target = (uint32_t)s;
        }
    }
    return items;
}

}  // namespace dspi
