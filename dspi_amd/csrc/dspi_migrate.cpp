// dspi_migrate.cpp — see dspi_migrate.h.
#include "dspi_migrate.h"

#include <algorithm>
#include <unordered_map>

namespace dspi {

const char *migrate_validate(const StreamMove *moves, uint32_t n, uint32_t n_src, uint32_t n_dst, const uint8_t *dst_active) {
    if (!moves || n == 0) return "empty move list";
    for (uint32_t i = 0; i < n; i++) {
        if (moves[i].src >= n_src) return "source index out of range";
        if (moves[i].dst >= n_dst) return "destination index out of range";
    }
    std::vector<uint8_t> is_src(n_src, 0), is_dst(n_dst, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (is_src[moves[i].src]) return "a slot is the source of two entries";
        is_src[moves[i].src] = 1;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (is_dst[moves[i].dst]) return "a slot is the destination of two entries";
        is_dst[moves[i].dst] = 1;
    }
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

std::vector<MigrateTarget> migrate_targets(const StreamMove *moves, uint32_t n, uint32_t n_dst, uint32_t row_streams, const uint8_t *dst_active) {
    std::vector<MigrateTarget> out(n);
    struct RowTarget { uint32_t target, from_entry, lowest; };
    std::unordered_map<uint32_t, RowTarget> rows;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t row = moves[i].dst / row_streams;
        auto it = rows.find(row);
        if (it != rows.end()) {
            if (it->second.from_entry && moves[i].dst < it->second.lowest) { it->second.lowest = moves[i].dst; it->second.target = i; }
            continue;
        }
        const uint64_t r0 = (uint64_t)row * row_streams, r1 = std::min<uint64_t>(r0 + row_streams, n_dst);
        uint32_t resident = kMoveNone;
        for (uint64_t s = r0; s < r1 && resident == kMoveNone; s++)
            if (!dst_active || dst_active[s]) resident = (uint32_t)s;
        rows[row] = resident != kMoveNone ? RowTarget{resident, 0u, 0u} : RowTarget{i, 1u, moves[i].dst};
    }
    for (uint32_t i = 0; i < n; i++) {
        const RowTarget &t = rows[moves[i].dst / row_streams];
        out[i] = MigrateTarget{moves[i].dst, t.target, t.from_entry};
    }
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
