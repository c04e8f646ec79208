// intake_driver.cpp — drives dspi_amd/csrc/dspi_intake.{h,cpp} (the input layout of dspi_process_mixed) from tests/test_intake_cpu.py.
// One command per input line, one answer per line:
//   check D...              -> the index of the first depth that is neither 16 nor 24, or the count; then the uniform depth (0: none)
//   off F D...              -> total, then the n + 1 offsets
//   rows F ROW K D...       -> the byte ranges "b-e" of K chunks of rows (rows per chunk = ceil(rows / K)), in chunk order
//   widen DEPTH F HEX       -> the run of F frames (hex bytes) as packed 24 bit, hex; the output buffer is exactly 6 F bytes
//   preamp WORD             -> 1 when a 16-bit stream with this binary32 preamp is refused, else 0
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_intake.h"

using namespace dspi;

static std::vector<uint8_t> depths_of(std::istringstream &in) {
    std::vector<uint8_t> d;
    for (unsigned v; in >> v;) d.push_back((uint8_t)v);
    return d;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "check") {
            const std::vector<uint8_t> d = depths_of(in);
            printf("%u %u\n", intake_check_depths(d.data(), (uint32_t)d.size()), (unsigned)intake_uniform_depth(d.data(), (uint32_t)d.size()));
        } else if (cmd == "off") {
            uint64_t frames; in >> frames;
            const std::vector<uint8_t> d = depths_of(in);
            std::vector<uint64_t> off(d.size() + 1);
            uint64_t total = 0, alone = 0;
            if (!intake_offsets(d.data(), (uint32_t)d.size(), frames, &total, off.data()) || !intake_offsets(d.data(), (uint32_t)d.size(), frames, &alone, nullptr) || alone != total) {
                printf("overflow\n");
                continue;
            }
            printf("%llu", (unsigned long long)total);
            for (uint64_t o : off) printf(" %llu", (unsigned long long)o);
            printf("\n");
        } else if (cmd == "rows") {
            uint64_t frames; uint32_t row, k; in >> frames >> row >> k;
            const std::vector<uint8_t> d = depths_of(in);
            const uint32_t n = (uint32_t)d.size(), rows = (n + row - 1) / row, per = (rows + k - 1) / k;
            std::vector<uint64_t> off(d.size() + 1);
            intake_offsets(d.data(), n, frames, nullptr, off.data());
            for (uint32_t r0 = 0; r0 < rows; r0 += per) {
                uint64_t b, e;
                intake_row_range(off.data(), n, row, r0, r0 + per < rows ? r0 + per : rows, &b, &e);
                printf("%s%llu-%llu", r0 ? " " : "", (unsigned long long)b, (unsigned long long)e);
            }
            printf("\n");
        } else if (cmd == "widen") {
            unsigned depth; uint64_t frames; std::string hex; in >> depth >> frames >> hex;
            std::vector<uint8_t> src(hex.size() / 2), dst((size_t)frames * 6);
            for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
            if (src.size() != frames * intake_frame_bytes((uint8_t)depth)) { printf("bad length\n"); continue; }
            intake_widen_cpu(dst.data(), src.data(), (uint8_t)depth, frames);
            for (uint8_t b : dst) printf("%02x", b);
            printf("\n");
        } else if (cmd == "preamp") {
            unsigned long word; in >> word;
            printf("%d\n", intake_preamp_breaks_widening((uint32_t)word) ? 1 : 0);
        } else printf("unknown command\n");
    }
    return 0;
}
