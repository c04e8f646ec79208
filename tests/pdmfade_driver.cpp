// pdmfade_driver.cpp — dspi_amd/csrc/dspi_pdmfade.{h,cpp} without a GPU (tests/test_pdmfade_cpu.py): a script on stdin, one command per
// line, run against one PdmLife, one PdmFade and what a context keeps beside them (the record of pauses, every stream's "sub on"), wired
// as dspi_capi.cpp wires them: PdmLife::plan gets PdmFade::wants, then PdmFade::plan; a call is PdmLife::commit, then PdmFade::commit.
//   new N | mode V | sub S V | pause FIRST COUNT | resume FIRST COUNT | move S D [S D ...] | arrive S RUNNING POS ACTIVE SUB | boot S [S ...]
//   resize N | run FIRST V [V ...] (dspi_pdm_running's set) | pos S P (dspi_pdm_fade_state's set, the host half) | check FIRST W [W ...]
//   plan     the rule without the call's success: prints  W <builds> L <words, rS = reset> A <aux: 0 | fP | cP> U <first-end runs> any=<0|1>
//   call F   the rule and a successful call of F frames, prints the same
//   get      prints  B <running bytes> P <positions> mode=<0|1> <dirty|clean>
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_pdmfade.h"

using namespace dspi;

int main() {
    PdmLife pl;
    PdmFade fd;
    std::vector<uint8_t> active, sub;
    uint32_t n_streams = 0;
    auto act = [&]() -> const uint8_t * {
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
        if (cmd == "new" && v.size() == 1) { n_streams = v[0]; active.assign(n_streams, 1); sub.assign(n_streams, 0); pl = PdmLife(); pl.create(n_streams); fd = PdmFade(); fd.create(n_streams); }
        else if (cmd == "mode" && v.size() == 1) { if (v[0]) fd.enable(pl); else fd.disable(pl); }
        else if (cmd == "sub" && v.size() == 2 && v[0] < n_streams) { if (sub[v[0]] != (v[1] ? 1 : 0)) { sub[v[0]] = v[1] ? 1 : 0; pl.mark_dirty(); } }
        else if ((cmd == "pause" || cmd == "resume") && v.size() == 2 && (uint64_t)v[0] + v[1] <= n_streams) {
            for (uint32_t s = v[0]; s < v[0] + v[1]; s++) active[s] = cmd == "resume";
            pl.mark_dirty();
        } else if (cmd == "move" && !v.empty() && v.size() % 2 == 0) {
            std::vector<StreamMove> mv;
            for (size_t i = 0; i < v.size(); i += 2) mv.push_back(StreamMove{v[i], v[i + 1]});
            if (const char *why = move_validate(mv.data(), (uint32_t)mv.size(), n_streams, act())) { printf("refused: %s\n", why); return 2; }
            pl.move(mv.data(), (uint32_t)mv.size());
            fd.move(mv.data(), (uint32_t)mv.size());
            std::vector<uint8_t> was(mv.size()), was_sub(mv.size()), is_dst(n_streams, 0);
            for (size_t i = 0; i < mv.size(); i++) { was[i] = active[mv[i].src]; was_sub[i] = sub[mv[i].src]; is_dst[mv[i].dst] = 1; }
            for (size_t i = 0; i < mv.size(); i++) { active[mv[i].dst] = was[i]; sub[mv[i].dst] = was_sub[i]; }
            for (size_t i = 0; i < mv.size(); i++) if (!is_dst[mv[i].src]) active[mv[i].src] = 0;
        } else if (cmd == "arrive" && v.size() == 5 && v[0] < n_streams) { pl.arrive(v[0], (uint8_t)v[1]); fd.arrive(pl, v[0], v[2]); active[v[0]] = v[3] != 0; sub[v[0]] = v[4] != 0; }
        else if (cmd == "boot" && !v.empty()) { pl.boot(v.data(), (uint32_t)v.size()); fd.boot(v.data(), (uint32_t)v.size()); for (uint32_t s : v) sub[s] = 0; }
        else if (cmd == "resize" && v.size() == 1) { n_streams = v[0]; pl.resize(n_streams); fd.resize(n_streams); active.resize(n_streams, 1); sub.resize(n_streams, 0); }
        else if (cmd == "run" && v.size() >= 2) {
            std::vector<uint8_t> vals(v.begin() + 1, v.end());
            if (const char *why = pl.set_get(v[0], (uint32_t)vals.size(), vals.data(), nullptr)) printf("refused: %s\n", why);
        } else if (cmd == "pos" && v.size() == 2 && v[0] < n_streams) { fd.pos[v[0]] = (uint16_t)v[1]; pl.mark_dirty(); }
        else if (cmd == "check" && v.size() >= 1) {
            const char *why = fd.check(v[0], (uint32_t)v.size() - 1, v.data() + 1);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "get") {
            printf("B");
            for (uint8_t b : pl.running) printf(" %u", b);
            printf(" P");
            for (uint16_t p : fd.pos) printf(" %u", p);
            printf(" mode=%d %s\n", (int)fd.on, pl.dirty ? "dirty" : "clean");
        } else if (cmd == "plan" || (cmd == "call" && v.size() == 1)) {
            const PdmWork &w = pl.plan(act(), [&](uint32_t s) { return fd.wants(pl, s, sub_on(s)); });
            fd.plan(pl, sub_on);
            printf("W %llu L", (unsigned long long)pl.builds);
            for (uint32_t x : w.list) printf(x & kPdmListReset ? " r%u" : " %u", x & ~kPdmListReset);
            printf(" A");
            for (size_t i = 0; i < w.list.size(); i++) {
                const uint32_t a = i < fd.aux.size() ? fd.aux[i] : 0u;
                if (a & kPdmAuxFade) printf(" f%u", a & kPdmAuxPos);
                else if (a & kPdmAuxCancel) printf(" c%u", a & kPdmAuxPos);
                else printf(" %u", a);
            }
            printf(" U");
            for (const auto &r : w.unlisted) printf(" %u-%u", r.first, r.second);
            printf(" any=%d\n", (int)fd.any_aux);
            if (cmd == "call") { pl.commit(); fd.commit(pl, v[0]); }
        } else { printf("bad command: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
