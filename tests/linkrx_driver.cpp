// linkrx_driver.cpp — dspi_amd/csrc/dspi_link.{h,cpp} (with dspi_spdifrx.cpp) without a GPU (tests/test_link_cpu.py).  One command per input
// line, one line of output each; buffers travel as files of raw little-endian words, each read into a heap block of exactly its size, so that
// a word read outside the view is the sanitizer's to report:
//   dec <wire file> <n_streams> <n_pairs> <tile_streams> <n_frames> <links file> <rx file> <out file>
//         link_decode_cpu for every link of the links file (dspi_link [n]) through the records of the rx file (dspi_spdif_rx [n]); the out file
//         takes the records, the pair words int32 [n][F][2] and the packed bytes uint8 [n][6 F], the last two filled with 0x5A beforehand.
//         Prints "ok", or what link_view_why / links_check refuse.
//   view <wire alignment> <n_streams> <n_pairs> <tile_streams> <n_frames> <frames> <device>      link_view_why: "ok" or the text
//   words <n_streams> <n_pairs> <tile_streams> <n_frames>                                         link_view_words: the count or "overflow"
//   check <lines> <none_ok> <line>:<kind>:<active> ...                                            "<links_check> <any S/PDIF> <any I2S>"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_link.h"

using namespace dspi;

// a file's bytes in a block of exactly that size, 16-byte aligned like the buffers of the calls
struct Block {
    std::unique_ptr<uint8_t[]> p;
    size_t n = 0;
    bool read(const std::string &path) {
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        if (!f) return false;
        n = (size_t)f.tellg();
        p.reset(new uint8_t[n ? n : 1]);
        f.seekg(0);
        f.read(reinterpret_cast<char *>(p.get()), (std::streamsize)n);
        return (bool)f;
    }
};

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string cmd;
        in >> cmd;
        if (cmd == "dec") {
            std::string wire_path, links_path, rx_path, out_path;
            WireView v{};
            in >> wire_path >> v.n_streams >> v.n_pairs >> v.tile_streams >> v.n_frames >> links_path >> rx_path >> out_path;
            Block wire, links, rx;
            if (!wire.read(wire_path) || !links.read(links_path) || !rx.read(rx_path)) { puts("cannot read"); continue; }
            v.wire = reinterpret_cast<const uint32_t *>(wire.p.get());
            const uint32_t n = (uint32_t)(links.n / sizeof(Link));
            const Link *const lk = reinterpret_cast<const Link *>(links.p.get());
            uint64_t words = 0;
            if (const char *why = link_view_why(v, 0, false)) { puts(why); continue; }
            if (!link_view_words(v, &words) || words * 4 != wire.n || rx.n != (size_t)n * sizeof(SpdifRx)) { puts("sizes disagree"); continue; }
            const uint32_t bad = links_check(lk, n, link_view_lines(v), nullptr, true);
            if (bad < n) { printf("link %u\n", bad); continue; }
            const size_t F = v.n_frames;
            std::vector<int32_t> pairs((size_t)n * 2 * F, 0x5A5A5A5A);
            std::vector<uint8_t> packed((size_t)n * 6 * F, 0x5A);
            SpdifRx *const recs = reinterpret_cast<SpdifRx *>(rx.p.get());
            for (uint32_t i = 0; i < n; i++) link_decode_cpu(v, lk[i], recs + i, pairs.data() + (size_t)i * 2 * F, packed.data() + (size_t)i * 6 * F);
            std::ofstream out(out_path, std::ios::binary);
            out.write(reinterpret_cast<const char *>(recs), (std::streamsize)rx.n);
            out.write(reinterpret_cast<const char *>(pairs.data()), (std::streamsize)(pairs.size() * 4));
            out.write(reinterpret_cast<const char *>(packed.data()), (std::streamsize)packed.size());
            puts(out ? "ok" : "cannot write");
        } else if (cmd == "view") {
            uintptr_t align;
            uint64_t frames;
            int device;
            WireView v{};
            in >> align >> v.n_streams >> v.n_pairs >> v.tile_streams >> v.n_frames >> frames >> device;
            v.wire = reinterpret_cast<const uint32_t *>(align);      // (never read: 0 is NULL, 16 is aligned, 8 is not)
            const char *why = link_view_why(v, frames, device != 0);
            puts(why ? why : "ok");
        } else if (cmd == "words") {
            WireView v{};
            uint64_t words = 0;
            in >> v.n_streams >> v.n_pairs >> v.tile_streams >> v.n_frames;
            if (link_view_words(v, &words)) printf("%llu\n", (unsigned long long)words);
            else puts("overflow");
        } else if (cmd == "check") {
            uint64_t lines;
            int none_ok;
            in >> lines >> none_ok;
            std::vector<Link> lk;
            std::vector<uint8_t> active;
            for (std::string item; in >> item;) {
                unsigned line, kind, on;
                if (sscanf(item.c_str(), "%u:%u:%u", &line, &kind, &on) != 3) break;
                lk.push_back(Link{line, kind}); active.push_back((uint8_t)on);
            }
            const uint32_t n = (uint32_t)lk.size();
            printf("%u %d %d\n", links_check(lk.data(), n, lines, active.data(), none_ok != 0), (int)links_any(lk.data(), n, active.data(), kLinkSpdif), (int)links_any(lk.data(), n, active.data(), kLinkI2s));
        } else puts("unknown command");
    }
    return 0;
}
