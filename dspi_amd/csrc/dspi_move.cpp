// dspi_move.cpp — see dspi_move.h.
#include "dspi_move.h"

#include <algorithm>
#include <unordered_map>

namespace dspi {

const char *move_validate(const StreamMove *moves, uint32_t n, uint32_t n_streams, const uint8_t *active) {
    if (!moves || n == 0) return "empty move list";
    for (uint32_t i = 0; i < n; i++)
        if (moves[i].src >= n_streams || moves[i].dst >= n_streams) return "stream index out of range";
    std::vector<uint8_t> mark(n_streams, 0);      // bit 0: a source, bit 1: a destination
    for (uint32_t i = 0; i < n; i++) {
        if (mark[moves[i].src] & 1u) return "a slot is the source of two entries";
        mark[moves[i].src] |= 1u;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (mark[moves[i].dst] & 2u) return "a slot is the destination of two entries";
        mark[moves[i].dst] |= 2u;
    }
    for (uint32_t i = 0; i < n; i++)
        if (!(mark[moves[i].dst] & 1u) && (!active || active[moves[i].dst])) return "a destination holds an active stream that the list does not move away";
    return nullptr;
}

std::vector<StreamMove> move_compaction(const uint8_t *active, uint32_t n_streams, bool one_way) {
    std::vector<StreamMove> out;
    if (!active) return out;
    uint32_t n_active = 0;
    for (uint32_t s = 0; s < n_streams; s++) n_active += active[s] ? 1u : 0u;
    uint32_t t = n_active;
    for (uint32_t h = 0; h < n_active; h++) {
        if (active[h]) continue;
        while (!active[t]) t++;      // (as many active slots at or above A as paused ones below it)
        out.push_back(StreamMove{t, h});
        if (!one_way) out.push_back(StreamMove{h, t});
        t++;
    }
    return out;
}

std::vector<MoveTarget> move_targets(const StreamMove *moves, uint32_t n, uint32_t n_streams, uint32_t row_streams, const uint8_t *active) {
    std::vector<uint8_t> moved(n_streams, 0);
    std::vector<MoveTarget> out;
    for (uint32_t i = 0; i < n; i++) {
        if (moves[i].src == moves[i].dst) continue;
        moved[moves[i].src] = moved[moves[i].dst] = 1;
        out.push_back(MoveTarget{moves[i].src, moves[i].dst, kMoveNone});
    }
    // per touched row: the lowest resident, else the source of the lowest destination
    std::unordered_map<uint32_t, uint32_t> row_target, row_lowest;      // row -> slot to read / lowest destination seen
    for (const MoveTarget &t : out) {
        const uint32_t row = t.dst / row_streams;
        if (row_target.count(row)) {
            auto lo = row_lowest.find(row);
            if (lo != row_lowest.end() && t.dst < lo->second) { lo->second = t.dst; row_target[row] = t.src; }
            continue;
        }
        const uint64_t r0 = (uint64_t)row * row_streams, r1 = std::min<uint64_t>(r0 + row_streams, n_streams);
        uint32_t resident = kMoveNone;
        for (uint64_t s = r0; s < r1 && resident == kMoveNone; s++)
            if (!moved[s] && (!active || active[s])) resident = (uint32_t)s;
        if (resident != kMoveNone) row_target[row] = resident;
        else { row_target[row] = t.src; row_lowest[row] = t.dst; }
    }
    for (MoveTarget &t : out) t.target = row_target[t.dst / row_streams];
    return out;
}

namespace {

struct Scheduler {
    explicit Scheduler(uint32_t c) : cap(c) {}
    uint32_t cap, used = 0;
    std::vector<MoveBatch> out;
    MoveBatch cur;
    void flush(uint32_t keep = 0) {
        if (!cur.gather.empty() || !cur.scatter.empty()) out.push_back(std::move(cur));
        cur = MoveBatch{};
        used = keep;
    }
    void add(uint32_t src, uint32_t dst, uint32_t keep = 0) {
        if (used == cap) flush(keep);
        cur.gather.push_back(MoveRecord{src, used});
        cur.scatter.push_back(MoveRecord{dst, used});
        used++;
    }
};

}  // namespace

std::vector<MoveBatch> move_schedule(const StreamMove *moves, uint32_t n, uint32_t cap) {
    if (cap < 2) cap = 2;
    std::unordered_map<uint32_t, uint32_t> to, from;      // src -> dst, dst -> src
    std::vector<uint32_t> order;                          // the sources, in list order
    for (uint32_t i = 0; i < n; i++) {
        if (moves[i].src == moves[i].dst) continue;
        to[moves[i].src] = moves[i].dst; from[moves[i].dst] = moves[i].src;
        order.push_back(moves[i].src);
    }
    std::unordered_map<uint32_t, uint8_t> done;
    std::vector<std::vector<uint32_t>> chains, cycles;      // slots in move order: slot k + 1 takes slot k's stream
    for (uint32_t s : order) {      // chains begin at a source that is no destination
        if (from.count(s)) continue;
        std::vector<uint32_t> c{s};
        for (auto it = to.find(s); it != to.end(); it = to.find(it->second)) { done[c.back()] = 1; c.push_back(it->second); }
        chains.push_back(std::move(c));
    }
    for (uint32_t s : order) {      // what is left closes on itself
        if (done.count(s)) continue;
        std::vector<uint32_t> c;
        for (uint32_t x = s; !done.count(x); x = to[x]) { done[x] = 1; c.push_back(x); }
        cycles.push_back(std::move(c));
    }
    Scheduler b(cap);
    for (const auto &c : cycles) {
        const uint32_t len = (uint32_t)c.size();
        if (len > cap) continue;
        if (b.used + len > cap) b.flush();
        for (uint32_t k = 0; k < len; k++) b.add(c[k], c[(k + 1) % len]);
    }
    for (const auto &c : cycles) {
        const uint32_t len = (uint32_t)c.size();
        if (len <= cap) continue;
        b.flush();
        b.cur.gather.push_back(MoveRecord{c[len - 1], 0});      // held until the cycle closes
        b.used = 1;
        for (uint32_t k = len - 1; k-- > 0;) b.add(c[k], c[k + 1], 1);
        b.cur.scatter.push_back(MoveRecord{c[0], 0});
        b.flush();
    }
    for (const auto &c : chains)
        for (size_t k = c.size() - 1; k-- > 0;) b.add(c[k], c[k + 1]);
    b.flush();
    return b.out;
}

void move_row_items(const std::vector<MoveRecord> &list, uint32_t row_streams, std::vector<MoveRowItem> &items, std::vector<uint32_t> &colrec) {
    std::vector<MoveRecord> sorted(list);
    std::sort(sorted.begin(), sorted.end(), [](const MoveRecord &a, const MoveRecord &b) { return a.slot < b.slot; });
    const size_t first = items.size();
    for (const MoveRecord &r : sorted) {
        const uint32_t row = r.slot / row_streams, col = r.slot % row_streams;
        if (items.size() == first || items.back().row != row) {
            items.push_back(MoveRowItem{row, 0u, 0u, 0u});
            colrec.insert(colrec.end(), row_streams, kMoveNone);
        }
        colrec[colrec.size() - row_streams + col] = r.record;
        items.back().q_any |= 1u << (col / 4);
    }
    for (size_t i = first; i < items.size(); i++) {
        const uint32_t *cr = colrec.data() + colrec.size() - (items.size() - i) * row_streams;
        for (uint32_t q = 0; q < row_streams / 4; q++)
            if (cr[4 * q] != kMoveNone && cr[4 * q + 1] != kMoveNone && cr[4 * q + 2] != kMoveNone && cr[4 * q + 3] != kMoveNone) items[i].q_all |= 1u << q;
    }
}

}  // namespace dspi
