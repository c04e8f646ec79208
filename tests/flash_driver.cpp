// flash_driver.cpp — a stream's own flash (dspi_amd/csrc/dspi_flash.{h,cpp}) on the CPU, for tests/test_flash_cpu.py: the book and the sector
// rules.  Every mode reads its cases from standard input, one per line, and answers one line per case.  A case is a script of words:
//   flash_driver book      the book of a context ("main") and of a second one ("src", for migrations); every flash carries a TAG byte
//       n N                main: N streams sharing one fresh flash (tag 0)             sn N     the same for src
//       w S TAG            main: writable(S), then its tag := TAG (clone on write)     sw S TAG the same for src
//       mv a>b,c>d         main: move (all entries at once)
//       ar a>b,c>d         main: arrive from src (by value), src: leave
//       bt TAG s,s,s       main: boot the listed slots onto one new flash tagged TAG
//       rs N TAG           main: resize to N (new slots share one new flash tagged TAG)
//       drop               main: the mode goes off
//     -> "tags t t t | objs o o o | refs r r r | distinct k | src tags t t | src distinct k"   (refs: of the live objects, by index)
//   flash_driver pairs     "i,i,i f,f,f" (image and flash index per stream) -> "image:flash@first ... | pair per stream"
//   flash_driver sector    one flash
//       write SECTOR LEN V       a sector write of LEN bytes of value V                erase SECTOR
//       set HEX                  set_bytes: an erased area whose first bytes are HEX (the directory sector's)
//       legacy FLAVOR VERSION    a valid legacy sector (sector 11) whose data bytes are 1, 2, 3, ...
//       boot FLAVOR              boot_writes                      flush   dir_ensure + dir_flush                first FLAVOR POPULATED
//     -> "valid V | wrote W | dir HEX(344 bytes of sector 0) | cache HEX(cached directory from byte 12 to 24) | used u0 u1 ... u11" (bytes that are not 0xFF, per sector)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_flash.h"

using namespace dspi;

static const size_t kTagAt = 5000;

static std::vector<StreamMove> moves_of(const std::string &s) {
    std::vector<StreamMove> mv;
    std::istringstream in(s);
    std::string e;
    while (std::getline(in, e, ',')) {
        const size_t gt = e.find('>');
        StreamMove m; memset(&m, 0, sizeof m);
        m.src = (uint32_t)strtoul(e.substr(0, gt).c_str(), nullptr, 0); m.dst = (uint32_t)strtoul(e.substr(gt + 1).c_str(), nullptr, 0);
        mv.push_back(m);
    }
    return mv;
}
static std::vector<int32_t> ints_of(const std::string &s) {
    std::vector<int32_t> v;
    std::istringstream in(s);
    std::string e;
    while (std::getline(in, e, ',')) v.push_back((int32_t)strtol(e.c_str(), nullptr, 0));
    return v;
}
static std::unique_ptr<Flash> tagged(uint8_t tag) { auto f = std::make_unique<Flash>(); f->bytes[kTagAt] = tag; return f; }
static void start(FlashBook &b, uint32_t n) { b.drop(); b.enable(n); const int32_t o = b.add(tagged(0)); for (uint32_t s = 0; s < n; s++) b.assign(s, o); }
static void tags(std::ostringstream &out, const FlashBook &b) { for (uint32_t s = 0; s < b.index.size(); s++) out << " " << (int)b.readable(s).bytes[kTagAt]; }
static std::string hex(const uint8_t *p, size_t n) { static const char *d = "0123456789abcdef"; std::string s; for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; } return s; }

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        std::string w;
        if (cmd == "book") {
            FlashBook b, src;
            while (in >> w) {
                if (w == "n" || w == "sn") { uint32_t n; in >> n; start(w == "n" ? b : src, n); }
                else if (w == "w" || w == "sw") { uint32_t s; int t; in >> s >> t; (w == "w" ? b : src).writable(s)->bytes[kTagAt] = (uint8_t)t; }
                else if (w == "mv") { std::string l; in >> l; const auto mv = moves_of(l); b.move(mv.data(), (uint32_t)mv.size()); }
                else if (w == "ar") { std::string l; in >> l; const auto mv = moves_of(l); src.leave(mv.data(), (uint32_t)mv.size()); b.arrive(src, mv.data(), (uint32_t)mv.size()); }
                else if (w == "bt") { int t; std::string l; in >> t >> l; std::vector<uint32_t> s; for (int32_t v : ints_of(l)) s.push_back((uint32_t)v); b.boot(s.data(), (uint32_t)s.size(), b.add(tagged((uint8_t)t))); }
                else if (w == "rs") { uint32_t n; int t; in >> n >> t; b.resize(n, n > b.index.size() ? b.add(tagged((uint8_t)t)) : -1); }
                else if (w == "drop") b.drop();
                else { fprintf(stderr, "book: unknown word %s\n", w.c_str()); return 2; }
            }
            out << "tags"; tags(out, b);
            out << " | objs"; for (int32_t o : b.index) out << " " << o;
            out << " | refs"; for (size_t k = 0; k < b.objects.size(); k++) if (b.objects[k]) out << " " << b.refs[k];
            out << " | distinct " << b.distinct() << " | src tags"; tags(out, src);
            out << " | src distinct " << src.distinct();
        } else if (cmd == "pairs") {
            std::string a, f; in >> a >> f;
            std::vector<uint32_t> of;
            for (const FlashPair &p : flash_pairs(ints_of(a), ints_of(f), &of)) out << p.image << ":" << p.flash << "@" << p.first_stream << " ";
            out << "|"; for (uint32_t k : of) out << " " << k;
        } else if (cmd == "sector") {
            Flash f;
            bool wrote = false;
            while (in >> w) {
                if (w == "write") { int s; size_t n; int v; in >> s >> n >> v; std::vector<uint8_t> p(n, (uint8_t)v); f.write_sector(s, p.data(), n); }
                else if (w == "erase") { int s; in >> s; f.erase_sector(s); }
                else if (w == "set") {
                    std::string h; in >> h;
                    std::vector<uint8_t> img(kFlashDumpBytes, 0xFF);
                    for (size_t i = 0; i + 1 < h.size(); i += 2) img[i / 2] = (uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16);
                    memcpy(&img[kTagAt], &f.bytes[kTagAt], 1);
                    for (int s = 1; s < 12; s++) memcpy(&img[(size_t)s * kFlashSector], &f.bytes[(size_t)s * kFlashSector], kFlashSector);      // (only the directory sector is replaced)
                    f.set_bytes(img.data());
                } else if (w == "legacy") {
                    int flavor, version; in >> flavor >> version;
                    const StateMap m = make_state_map(flavor);
                    const size_t lb = 12 + (size_t)m.n_ch * kStoredBands * 16 + 4 + 4 + (size_t)m.n_ch * 4 + 12 + 4 + 4 + 8 + 4 + 8 + (size_t)2 * m.n_out * 8 + (size_t)m.n_out * 12 + 8;
                    std::vector<uint8_t> p(lb);
                    for (size_t i = 12; i < lb; i++) p[i] = (uint8_t)(i - 11);
                    const uint32_t magic = 0x44535031u, crc = flash_crc32(&p[12], lb - 12); const uint16_t v = (uint16_t)version, z = 0;
                    memcpy(&p[0], &magic, 4); memcpy(&p[4], &v, 2); memcpy(&p[6], &z, 2); memcpy(&p[8], &crc, 4);
                    f.write_sector(kSectorLegacy, p.data(), lb);
                } else if (w == "boot") { int flavor; in >> flavor; wrote = f.boot_writes(flavor); }
                else if (w == "flush") { f.dir_ensure(); f.dir_flush(); }
                else if (w == "first") { int flavor, pop; in >> flavor >> pop; f = *Flash::first_boot(flavor, pop != 0, nullptr); }
                else { fprintf(stderr, "sector: unknown word %s\n", w.c_str()); return 2; }
            }
            const PresetDir d = f.directory();
            out << "valid " << (int)f.dir_valid << " | wrote " << (wrote ? 1 : 0) << " | dir " << hex(f.bytes, sizeof(PresetDir))
                << " | cache " << hex(reinterpret_cast<const uint8_t *>(&d) + 12, 12) << " | used";
            for (int s = 0; s < 12; s++) { size_t u = 0; for (size_t i = 0; i < kFlashSector; i++) u += f.bytes[(size_t)s * kFlashSector + i] != 0xFF; out << " " << u; }
        } else {
            fprintf(stderr, "usage: flash_driver book | pairs | sector\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
