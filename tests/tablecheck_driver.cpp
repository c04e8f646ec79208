// tablecheck_driver.cpp — dspi_amd/csrc/dspi_tablecheck.h without a GPU, for tests/test_packets_resident_cpu.py: one command per line of stdin,
// one line of answer each.  The table of a command is allocated at exactly 8 * entries bytes, 16-byte aligned, so that a load past it is a
// sanitizer finding as well as a finding of the walker.
//   walk entries per_stream max_wgs       (max_wgs 0: the launch's default)
//         tablecheck_lane, the kernel's whole per-lane body, for every workgroup and thread of the grid the launcher would start, over a
//         recording memory  ->  "ok WORKGROUPS PAIR_LOADS TAIL_LOADS MAX_ITERATIONS" after asserting: every load inside [0, 8 * entries); every
//         pair load 16 bytes at a 16-byte aligned address; at most one single 8-byte load, of the last entry of an odd count; every index in
//         [0, entries) loaded exactly once and judged exactly once, with the stream index / per_stream; no index at or above `entries`
//         judged; else "FAIL why"
//   answer kind n P nb bl arena_bytes max_wgs  kinds[n]  active[n]  table[n * per]     (kind 0: input, P is 1; kind 1: emit; per = P * nb)
//         the kernel's per-lane arithmetic and ITS REDUCTION replayed lane by lane (the butterfly within each wave of 64, the four LDS slots,
//         thread 0's minimum, the atomic minimum into a word set to all ones), next to the host check on the same table
//         ->  "ANSWER VERDICT": ANSWER the word as a decimal number or "none"; VERDICT "ok" | "lengths" | "kind S" | "overflow" | "entry I" from
//         packets_check / packets_emit_check (`active` all ones is passed as null, like a context without pauses)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <deque>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_tablecheck.h"

using namespace dspi;

struct Table {      // exactly as long as it is said to be, aligned as the calls demand
    uint64_t *p = nullptr;
    uint64_t entries;
    explicit Table(uint64_t n) : entries(n) {
        if (posix_memalign(reinterpret_cast<void **>(&p), 16, n ? 8 * n : 16)) abort();
        for (uint64_t i = 0; i < n; i++) p[i] = 0;
    }
    ~Table() { free(p); }
};

// ---- the walker's memory: it records what is loaded and what is judged ----
struct Recorder {
    const Table &T;
    uint32_t per_stream;
    std::vector<uint32_t> loaded, judged;
    std::deque<uint64_t> pending;      // indices loaded and not judged yet, in the order the lane judges them
    uint64_t pair_loads = 0, tail_loads = 0;
    std::string why;
    Recorder(const Table &t, uint32_t per) : T(t), per_stream(per), loaded(t.entries, 0), judged(t.entries, 0) {}
    void fail(const std::string &w) { if (why.empty()) why = w; }
    void pair(uint64_t first, uint64_t v[2]) {
        v[0] = v[1] = 0;
        const uint64_t a = 8 * first;
        if (a + 16 > 8 * T.entries || first + 1 >= T.entries) return fail("a pair load outside the table");
        if ((reinterpret_cast<uintptr_t>(T.p) + a) % 16) return fail("a pair load is not 16-byte aligned");
        v[0] = T.p[first]; v[1] = T.p[first + 1];
        loaded[first]++; loaded[first + 1]++; pair_loads++;
        pending.push_back(first); pending.push_back(first + 1);
    }
    uint64_t one(uint64_t index) {
        if (index >= T.entries) { fail("a single load outside the table"); return 0; }
        if (!(T.entries & 1u) || index != T.entries - 1) { fail("a single load that is not the last entry of an odd count"); return 0; }
        loaded[index]++; tail_loads++;
        pending.push_back(index);
        return T.p[index];
    }
    bool active(uint32_t s) {      // (once per judged entry, first of all)
        if (pending.empty()) { fail("an entry is judged that was not loaded"); return false; }
        const uint64_t i = pending.front();
        pending.pop_front();
        if (i >= T.entries) { fail("an index at or above `entries` is judged"); return false; }
        if (s != i / per_stream) fail("an entry is judged with another stream than index / per_stream");
        judged[i]++;
        return true;
    }
    uint8_t stream_kind(uint32_t) { return 24; }
};

static std::string walk(uint64_t entries, uint32_t per_stream, uint32_t max_wgs) {
    Table T(entries);
    Recorder R(T, per_stream);
    const TableCheck a{entries, 1u << 20, per_stream, 45, kTableInput};
    const uint32_t n_wgs = tablecheck_workgroups(entries, max_wgs ? max_wgs : kTableCheckDefaultWgs);
    if (n_wgs < 1 || n_wgs > (max_wgs ? max_wgs : kTableCheckDefaultWgs)) return "FAIL the grid is not inside its cap";
    uint64_t max_it = 0;
    for (uint32_t wg = 0; wg < n_wgs; wg++)
        for (uint32_t tid = 0; tid < kTableCheckThreads; tid++) {
            const uint64_t before = R.pair_loads;
            if (tablecheck_lane(a, n_wgs, wg, tid, R) != kTableCheckNone) R.fail("a legal table is refused");
            if (!R.pending.empty()) R.fail("an entry is loaded and not judged");
            max_it = std::max(max_it, R.pair_loads - before);
        }
    for (uint64_t i = 0; i < entries && R.why.empty(); i++) {
        if (R.loaded[i] != 1) R.fail("entry " + std::to_string(i) + " is loaded " + std::to_string(R.loaded[i]) + " times");
        if (R.judged[i] != 1) R.fail("entry " + std::to_string(i) + " is judged " + std::to_string(R.judged[i]) + " times");
    }
    if (R.tail_loads != (entries & 1u)) R.fail("the single load of an odd count is missing, or there is one too many");
    if (!R.why.empty()) return "FAIL " + R.why;
    return "ok " + std::to_string(n_wgs) + " " + std::to_string(R.pair_loads) + " " + std::to_string(R.tail_loads) + " " + std::to_string(max_it);
}

// ---- the answer: real memory, the kernel's reduction replayed ----
struct Memory {
    const Table &T;
    const std::vector<uint8_t> &kinds;
    const std::vector<uint32_t> *bits;      // the activity bitmap as the kernels take it, or null
    void pair(uint64_t first, uint64_t v[2]) const { v[0] = T.p[first]; v[1] = T.p[first + 1]; }
    uint64_t one(uint64_t index) const { return T.p[index]; }
    uint8_t stream_kind(uint32_t s) const { return kinds.at(s); }
    bool active(uint32_t s) const { return !bits || ((*bits).at(s >> 5) >> (s & 31u) & 1u); }
};

static std::string answer(std::istringstream &in) {
    uint32_t kind, n, P, nb, bl, max_wgs;
    uint64_t ab;
    in >> kind >> n >> P >> nb >> bl >> ab >> max_wgs;
    const uint32_t per = P * nb;
    std::vector<uint8_t> kinds(n), active(n);
    Table T((uint64_t)n * per);
    uint64_t x;
    for (auto &k : kinds) { in >> x; k = (uint8_t)x; }
    for (auto &k : active) { in >> x; k = (uint8_t)x; }
    for (uint64_t i = 0; i < T.entries; i++) in >> T.p[i];
    if (!in) return "FAIL parse";
    const bool all = std::all_of(active.begin(), active.end(), [](uint8_t v) { return v != 0; });
    std::vector<uint32_t> bits((n + 31) / 32, 0u);
    for (uint32_t s = 0; s < n; s++) if (active[s]) bits[s >> 5] |= 1u << (s & 31u);

    // the host check
    uint64_t at = 0;
    std::string verdict;
    if (kind == kTableEmit) {
        switch (packets_emit_check(kinds.data(), T.p, n, P, nb, bl, 192, ab, all ? nullptr : active.data(), false, &at)) {
        case EmitBad::Ok: verdict = "ok"; break;
        case EmitBad::Lengths: verdict = "lengths"; break;
        case EmitBad::Format: verdict = "kind " + std::to_string(at); break;
        case EmitBad::Overflow: verdict = "overflow"; break;
        case EmitBad::Entry: verdict = "entry " + std::to_string(at); break;
        case EmitBad::Overlap: verdict = "overlap"; break;
        }
    } else {
        switch (packets_check(kinds.data(), T.p, n, nb, bl, 192, ab, all ? nullptr : active.data(), &at)) {
        case PacketsBad::Ok: verdict = "ok"; break;
        case PacketsBad::Lengths: verdict = "lengths"; break;
        case PacketsBad::Depth: verdict = "kind " + std::to_string(at); break;
        case PacketsBad::Overflow: verdict = "overflow"; break;
        case PacketsBad::Entry: verdict = "entry " + std::to_string(at); break;
        }
    }
    if (verdict != "ok" && verdict.compare(0, 5, "entry")) return "- " + verdict;      // (the calls refuse these before the checker runs)

    // the launch: the word set to all ones, then every workgroup
    const TableCheck a{T.entries, ab, per, bl, kind};
    Memory m{T, kinds, all ? nullptr : &bits};
    uint64_t word = kTableCheckNone;
    const uint32_t n_wgs = tablecheck_workgroups(a.entries, max_wgs ? max_wgs : kTableCheckDefaultWgs);
    for (uint32_t wg = 0; wg < n_wgs; wg++) {
        uint64_t lane[kTableCheckThreads], lds[kTableCheckWaves];
        for (uint32_t tid = 0; tid < kTableCheckThreads; tid++) lane[tid] = tablecheck_lane(a, n_wgs, wg, tid, m);
        for (uint32_t w = 0; w < kTableCheckWaves; w++) {      // the butterfly: every lane of the wave at once
            uint64_t *const v = lane + w * kTableCheckWave;
            for (uint32_t off = kTableCheckFirstStep; off; off >>= 1) {
                uint64_t next[kTableCheckWave];
                for (uint32_t l = 0; l < kTableCheckWave; l++) next[l] = tablecheck_min(v[l], v[l ^ off]);
                std::copy(next, next + kTableCheckWave, v);
            }
            lds[w] = v[0];
        }
        uint64_t lowest = lane[0];
        for (uint32_t w = 1; w < kTableCheckWaves; w++) lowest = tablecheck_min(lowest, lds[w]);
        if (lowest != kTableCheckNone) word = tablecheck_min(word, lowest);      // the atomic minimum
    }
    return (word == kTableCheckNone ? std::string("none") : std::to_string(word)) + " " + verdict;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        std::string out = "FAIL unknown command";
        if (cmd == "walk") {
            uint64_t entries; uint32_t per, max_wgs;
            in >> entries >> per >> max_wgs;
            out = in ? walk(entries, per, max_wgs) : "FAIL parse";
        } else if (cmd == "answer") out = answer(in);
        printf("%s\n", out.c_str());
    }
    return 0;
}
