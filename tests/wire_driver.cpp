// wire_driver.cpp — drives dspi_amd/csrc/dspi_wire.{h,cpp} (the wire layout of dspi_process_wire / dspi_wire_encode) from
// tests/test_wire_cpu.py.  One command per input line, one answer per line:
//   flags process|encode WORD   -> 1 when the call accepts these flags, else 0
//   region S P NP F I2S         -> offset written tail_begin tail_end (bytes) of pair P of stream S, NP pairs, F frames
//   mask T...                   -> the I2S mask of a parameter object with these output types
//   scan N A... | I... | M...   -> N streams: their activity bytes (a single "-": no record, every stream active), their objects, the objects'
//                                  I2S masks; answers 1 when an active stream's object has an I2S slot (the wire route), else 0
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_wire.h"

using namespace dspi;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "flags") {
            std::string which; unsigned long word; in >> which >> word;
            printf("%d\n", (which == "process" ? wire_process_flags_ok((uint32_t)word) : wire_encode_flags_ok((uint32_t)word)) ? 1 : 0);
        } else if (cmd == "region") {
            unsigned long long s, p, np, f; int i2s; in >> s >> p >> np >> f >> i2s;
            const WireRegion r = wire_region(s, p, np, f, i2s != 0);
            printf("%llu %llu %llu %llu\n", (unsigned long long)r.offset, (unsigned long long)r.written, (unsigned long long)r.tail_begin, (unsigned long long)r.tail_end);
        } else if (cmd == "mask") {
            std::vector<uint8_t> t;
            for (unsigned v; in >> v;) t.push_back((uint8_t)v);
            printf("%u\n", wire_i2s_mask(t.data(), (uint32_t)t.size()));
        } else if (cmd == "scan") {
            uint32_t n; in >> n;
            std::vector<uint8_t> active; std::vector<int32_t> image; std::vector<uint32_t> masks;
            std::string tok;
            bool record = true;
            int part = 0;
            while (in >> tok) {
                if (tok == "|") { part++; continue; }
                if (part == 0) { if (tok == "-") record = false; else active.push_back((uint8_t)std::stoul(tok)); }
                else if (part == 1) image.push_back((int32_t)std::stol(tok));
                else masks.push_back((uint32_t)std::stoul(tok));
            }
            if ((record && active.size() != n) || image.size() != n) { printf("bad scan\n"); continue; }
            printf("%d\n", wire_any_i2s(image.data(), n, record ? active.data() : nullptr, masks.data()) ? 1 : 0);
        } else printf("unknown command\n");
    }
    return 0;
}
