// dspi_move.cpp — see dspi_move.h.
#include "dspi_move.h"

#include <algorithm>
#include <unordered_map>

namespace dspi {

const char *move_validate(const StreamMove *moves, uint32_t n, uint32_t n_streams, const uint8_t *active) {
    if (!moves || n == 0) return "empty move list";
    std::vector<uint8_t> is_src(n_streams, 0), is_dst(n_streams, 0);
    const SlotCheck src = check_slots(&moves->src, 2, n, is_src), dst = check_slots(&moves->dst, 2, n, is_dst);
    if (src == SlotCheck::out_of_range || dst == SlotCheck::out_of_range) return "stream index out of range";
    if (src == SlotCheck::duplicate) return "a slot is the source of two entries";
    if (dst == SlotCheck::duplicate) return "a slot is the destination of two entries";
    for (uint32_t i = 0; i < n; i++)
        if (!is_src[moves[i].dst] && (!active || active[moves[i].dst])) return "a destination holds an active stream that the list does not move away";
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

std::vector<ListTarget> list_targets(const StreamMove *moves, uint32_t n, uint32_t n_dst, uint32_t row_streams, const uint8_t *dst_active, const uint8_t *listed) {
    struct RowTarget { uint32_t target, from_entry; };
    std::unordered_map<uint32_t, RowTarget> rows;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t row = moves[i].dst / row_streams;
        auto it = rows.find(row);
        if (it == rows.end()) {
            const uint32_t resident = row_lowest_resident(row, row_streams, n_dst, dst_active, listed);
            rows[row] = resident != kMoveNone ? RowTarget{resident, 0u} : RowTarget{i, 1u};
        } else if (it->second.from_entry && moves[i].dst < moves[it->second.target].dst) it->second.target = i;
    }
    std::vector<ListTarget> out(n);
    for (uint32_t i = 0; i < n; i++) {
        const RowTarget &t = rows[moves[i].dst / row_streams];
        out[i] = ListTarget{moves[i].src, moves[i].dst, t.target, t.from_entry};
    }
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
