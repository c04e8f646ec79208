// dspi_migrate.cpp — see dspi_migrate.h.
#include "dspi_migrate.h"

namespace dspi {

const char *migrate_validate(const StreamMove *moves, uint32_t n, uint32_t n_src, uint32_t n_dst, const uint8_t *dst_active) {
    if (!moves || n == 0) return "empty move list";
    for (uint32_t i = 0; i < n; i++) {
        if (moves[i].src >= n_src) return "source index out of range";
        if (moves[i].dst >= n_dst) return "destination index out of range";
    }
    std::vector<uint8_t> is_src(n_src, 0), is_dst(n_dst, 0);
    if (check_slots(&moves->src, 2, n, is_src) == SlotCheck::duplicate) return "a slot is the source of two entries";
    if (check_slots(&moves->dst, 2, n, is_dst) == SlotCheck::duplicate) return "a slot is the destination of two entries";
    for (uint32_t i = 0; i < n; i++)
        if (!dst_active || dst_active[moves[i].dst]) return "a destination holds an active stream";
    return nullptr;
}

std::vector<StreamMove> migrate_plan(const uint8_t *src_active, uint32_t n_src, const uint8_t *dst_active, uint32_t n_dst, uint32_t want) {
    std::vector<StreamMove> out;
    if (!dst_active) return out;      // nothing paused at the destination: no room
    std::vector<uint32_t> from, to;
    for (uint32_t s = n_src; s-- > 0 && from.size() < want;)
        if (!src_active || src_active[s]) from.push_back(s);
    for (uint32_t s = 0; s < n_dst && to.size() < from.size(); s++)
        if (!dst_active[s]) to.push_back(s);
    const size_t k = to.size();      // (<= from.size(): the k highest sources are from's first k)
    for (size_t i = 0; i < k; i++) out.push_back(StreamMove{from[k - 1 - i], to[i]});
    return out;
}

std::vector<MoveBatch> migrate_batches(const StreamMove *moves, uint32_t n, uint32_t cap) {
    if (cap < 1) cap = 1;
    std::vector<MoveBatch> out;
    for (uint32_t first = 0; first < n; first += cap) {
        MoveBatch b;
        for (uint32_t k = 0; k < cap && first + k < n; k++) {
            b.gather.push_back(MoveRecord{moves[first + k].src, k});
            b.scatter.push_back(MoveRecord{moves[first + k].dst, k});
        }
        out.push_back(std::move(b));
    }
    return out;
}

}  // namespace dspi
