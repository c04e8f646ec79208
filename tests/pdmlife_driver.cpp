// pdmlife_driver.cpp — dspi_amd/csrc/dspi_pdmlife.{h,cpp} without a GPU (tests/test_pdmlife_cpu.py): a script on stdin, one command per
// line, run against one PdmLife and what a context keeps beside it: the record of pauses (a pause belongs to the slot, a move carries it
// along, an open-end source becomes paused) and every stream's "sub on" (it belongs to the stream's parameters and travels with them).
// Whatever the context marks the book dirty for, the driver does too: a changed "sub on", a changed pause.
//   new N | sub S V | pause FIRST COUNT | resume FIRST COUNT | move S D [S D ...] | arrive S V ACTIVE SUB | boot S [S ...] | resize N
//   set FIRST V [V ...] | setnull FIRST COUNT | get
//   plan   the rule without the call's success (a failed call): prints  W <builds> <resets> L <words, rS = reset> U <first-end runs> S <stops>
//   call   the rule and the successful call, prints the same
//   range S0 S1   the current list's words of streams [S0, S1): prints  R lo hi
// and the layout of a dspi_process_pdm call (dspi_plan.h plan_call), launch_plan_driver.cpp's call record with one more input, pdm_words:
//   C n_streams n_wg row n_ch n_out n_pairs n_blocks block_len bit_depth flags pairs sub peaks clip no_direct all_latency pdm_words
//   prints  L frames mem spdif_two_pass two_pass_rows two_pass_bytes direct_bytes n_chunks rows_per_chunk, then per buffer (pcm pairs sub
//   peaks clip pdm_words sub_scratch): bytes per tile_cols off
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_pdmlife.h"
#include "../dspi_amd/csrc/dspi_plan.h"

using namespace dspi;

static void print_work(const PdmLife &pl, const PdmWork &w) {
    printf("W %llu %d L", (unsigned long long)pl.builds, (int)w.resets);
    for (uint32_t x : w.list) printf(x & kPdmListReset ? " r%u" : " %u", x & ~kPdmListReset);
    printf(" U");
    for (const auto &r : w.unlisted) printf(" %u-%u", r.first, r.second);
    printf(" S");
    for (uint32_t s : w.stops) printf(" %u", s);
    printf("\n");
}

static bool call_record(const std::vector<uint32_t> &v) {
    if (v.size() != 17) return false;
    CallInput in;
    in.n_streams = v[0]; in.n_wg = v[1]; in.row = v[2]; in.n_ch = v[3]; in.n_out = v[4]; in.n_pairs = v[5]; in.n_blocks = v[6]; in.block_len = v[7];
    in.bit_depth = v[8]; in.flags = v[9]; in.pairs = v[10]; in.sub = v[11]; in.peaks = v[12]; in.clip = v[13]; in.no_direct = v[14]; in.all_latency = v[15];
    in.pdm_words = v[16];
    const CallLayout L = plan_call(in);
    printf("L %zu %d %d %u %zu %zu %u %u", L.frames, (int)L.mem, (int)L.spdif_two_pass, L.two_pass_rows, L.two_pass_bytes, L.direct_bytes, L.n_chunks, L.rows_per_chunk);
    for (const CallBuffer *b : {&L.pcm, &L.pairs, &L.sub, &L.peaks, &L.clip, &L.pdm_words, &L.sub_scratch}) printf(" %zu %zu %d %zu", b->bytes, b->per, (int)b->tile_cols, b->off);
    printf("\n");
    return true;
}

int main() {
    PdmLife pl;
    std::vector<uint8_t> active, sub;
    uint32_t n_streams = 0;
    auto act = [&]() -> const uint8_t * {      // null while nothing is paused, as the context hands it over
        for (uint8_t a : active) if (!a) return active.data();
        return nullptr;
    };
    auto sub_on = [&](uint32_t s) { return sub[s] != 0; };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<uint32_t> v;
        for (uint64_t x; in >> x;) v.push_back((uint32_t)x);
        if (cmd == "C") { if (!call_record(v)) { printf("bad call record\n"); return 2; } }
        else if (cmd == "new" && v.size() == 1) { n_streams = v[0]; active.assign(n_streams, 1); sub.assign(n_streams, 0); pl = PdmLife(); pl.create(n_streams); }
        else if (cmd == "sub" && v.size() == 2 && v[0] < n_streams) { if (sub[v[0]] != (v[1] ? 1 : 0)) { sub[v[0]] = v[1] ? 1 : 0; pl.mark_dirty(); } }
        else if ((cmd == "pause" || cmd == "resume") && v.size() == 2 && (uint64_t)v[0] + v[1] <= n_streams) {
            for (uint32_t s = v[0]; s < v[0] + v[1]; s++) active[s] = cmd == "resume";
            pl.mark_dirty();
        } else if (cmd == "move" && !v.empty() && v.size() % 2 == 0) {
            std::vector<StreamMove> mv;
            for (size_t i = 0; i < v.size(); i += 2) mv.push_back(StreamMove{v[i], v[i + 1]});
            if (const char *why = move_validate(mv.data(), (uint32_t)mv.size(), n_streams, act())) { printf("refused: %s\n", why); return 2; }
            pl.move(mv.data(), (uint32_t)mv.size());
            std::vector<uint8_t> was(mv.size()), was_sub(mv.size()), is_dst(n_streams, 0);
            for (size_t i = 0; i < mv.size(); i++) { was[i] = active[mv[i].src]; was_sub[i] = sub[mv[i].src]; is_dst[mv[i].dst] = 1; }
            for (size_t i = 0; i < mv.size(); i++) { active[mv[i].dst] = was[i]; sub[mv[i].dst] = was_sub[i]; }
            for (size_t i = 0; i < mv.size(); i++) if (!is_dst[mv[i].src]) active[mv[i].src] = 0;
        } else if (cmd == "arrive" && v.size() == 4 && v[0] < n_streams) { pl.arrive(v[0], (uint8_t)v[1]); active[v[0]] = v[2] != 0; sub[v[0]] = v[3] != 0; }
        else if (cmd == "boot" && !v.empty()) { pl.boot(v.data(), (uint32_t)v.size()); for (uint32_t s : v) sub[s] = 0; }      // (factory defaults: the sub is off)
        else if (cmd == "resize" && v.size() == 1) { n_streams = v[0]; pl.resize(n_streams); active.resize(n_streams, 1); sub.resize(n_streams, 0); }
        else if ((cmd == "set" && v.size() >= 1) || (cmd == "setnull" && v.size() == 2)) {
            std::vector<uint8_t> vals, got(n_streams + 1, 0xee);
            for (size_t i = 1; i < v.size(); i++) vals.push_back((uint8_t)v[i]);
            const uint32_t count = cmd == "set" ? (uint32_t)vals.size() : v[1];
            const char *why = pl.set_get(v[0], count, cmd == "set" ? vals.data() : nullptr, got.data());
            if (why) { bool clean = true; for (uint8_t g : got) clean = clean && g == 0xee; printf("refused: %s%s\n", why, clean ? "" : " (get was written)"); }
            else { printf("ok"); for (uint32_t k = 0; k < count; k++) printf(" %u", got[k]); printf("\n"); }
        } else if (cmd == "get") {
            printf("B");
            for (uint8_t b : pl.running) printf(" %u", b);
            printf(pl.dirty ? " dirty\n" : " clean\n");
        } else if (cmd == "plan" || cmd == "call") {
            const PdmWork &w = pl.plan(act(), sub_on);
            print_work(pl, w);
            if (cmd == "call") pl.commit();
        } else if (cmd == "range" && v.size() == 2) {
            const auto r = pl.work.range(v[0], v[1]);
            printf("R %zu %zu\n", r.first, r.second);
        } else { printf("bad command: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
