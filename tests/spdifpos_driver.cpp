// spdifpos_driver.cpp — dspi_amd/csrc/dspi_spdifpos.{h,cpp} without a GPU (tests/test_spdif_pos_cpu.py): a script on stdin, one command per
// line, run against one SpdifPos and the record of pauses that a context would keep beside it (the rules of include/dspi.h: a pause
// belongs to the slot, a move carries it along, an open-end source becomes paused).  Every `get` prints one line.
//   new N | enable P | disable | advance F | pause FIRST COUNT | resume FIRST COUNT | move S D [S D ...] | boot S [S ...] | set S P | get
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_spdifpos.h"

using namespace dspi;

int main() {
    SpdifPos sp;
    std::vector<uint8_t> active;
    uint32_t n_streams = 0;
    auto act = [&]() -> const uint8_t * {      // null while nothing is paused, as the context hands it over
        for (uint8_t a : active) if (!a) return active.data();
        return nullptr;
    };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<uint32_t> v;
        for (uint64_t x; in >> x;) v.push_back((uint32_t)x);
        if (cmd == "new" && v.size() == 1) { n_streams = v[0]; active.assign(n_streams, 1); sp = SpdifPos(); }
        else if (cmd == "enable" && v.size() == 1) sp.enable(n_streams, v[0]);
        else if (cmd == "disable") sp.disable();
        else if (cmd == "advance" && v.size() == 1) { if (sp.on) sp.advance(v[0]); }
        else if ((cmd == "pause" || cmd == "resume") && v.size() == 2 && (uint64_t)v[0] + v[1] <= n_streams) {
            if (sp.on) { if (cmd == "pause") sp.pause(v[0], v[1], act()); else sp.resume(v[0], v[1], act()); }
            for (uint32_t s = v[0]; s < v[0] + v[1]; s++) active[s] = cmd == "resume";
        } else if (cmd == "move" && !v.empty() && v.size() % 2 == 0) {
            std::vector<StreamMove> mv;
            for (size_t i = 0; i < v.size(); i += 2) mv.push_back(StreamMove{v[i], v[i + 1]});
            if (const char *why = move_validate(mv.data(), (uint32_t)mv.size(), n_streams, act())) { printf("refused: %s\n", why); return 2; }
            if (sp.on) sp.move(mv.data(), (uint32_t)mv.size(), act());
            std::vector<uint8_t> was(mv.size()), is_dst(n_streams, 0);
            for (size_t i = 0; i < mv.size(); i++) { was[i] = active[mv[i].src]; is_dst[mv[i].dst] = 1; }
            for (size_t i = 0; i < mv.size(); i++) active[mv[i].dst] = was[i];
            for (size_t i = 0; i < mv.size(); i++) if (!is_dst[mv[i].src]) active[mv[i].src] = 0;
        } else if (cmd == "boot" && !v.empty()) { if (sp.on) sp.boot(v.data(), (uint32_t)v.size(), act()); }
        else if (cmd == "set" && v.size() == 2 && v[0] < n_streams) sp.set(v[0], v[1], act());
        else if (cmd == "get") {
            printf("%s", sp.on ? "on" : "off");
            if (sp.on) {
                for (uint32_t s = 0; s < n_streams; s++) printf(" %u", sp.get(s, act()));
                for (uint32_t w : sp.word) if (w >= kSpdifBlock) { printf(" word-out-of-range"); break; }
                if (sp.clock >= kSpdifBlock) printf(" clock-out-of-range");
            }
            printf("\n");
        } else { printf("bad command: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
