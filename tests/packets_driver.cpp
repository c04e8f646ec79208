// packets_driver.cpp — dspi_amd/csrc/dspi_packets.{h,cpp} without a GPU, for tests/test_packets_cpu.py: one command per line of stdin, one line of
// answer each.  The arena of a command is allocated at exactly arena_bytes, so that a read past an entry that ends with the arena is a
// sanitizer finding; its bytes are arena_byte(seed, i), which the Python side computes too.
//   check n nb bl max_bl arena_bytes  depths[n]  active[n]  table[n * nb]   ->  ok | lengths | depth S | overflow | entry I
//   gather depth nb bl arena_bytes seed  row[nb]                            ->  the run's bytes in hex
//   walk n nb bl arena_bytes seed src_res dst_res  depths[n]  active[n]  table[n * nb]
//         the kernel's address functions for every workgroup, lane group and lane, with the arena at an address of residue src_res mod 16 and
//         the destination at one of residue dst_res, through an emulated LDS image  ->  "ok " + the destination's bytes in hex (a paused
//         stream's stay cc), after asserting: every source address inside its own entry, every image byte that is read was stored, every
//         destination byte of an active stream written exactly once and no other, the bytes equal packets_gather_cpu's; else "FAIL why"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_packets.h"

using namespace dspi;

static uint8_t arena_byte(uint64_t seed, uint64_t i) { return (uint8_t)((i * 131u + seed * 17u + (i >> 8) * 7u + 1u) & 0xffu); }

static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; i++) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
    return s;
}

struct Arena {      // exactly `bytes` long
    uint8_t *p;
    uint64_t bytes;
    Arena(uint64_t n, uint64_t seed) : p(static_cast<uint8_t *>(malloc(n ? n : 1))), bytes(n) { for (uint64_t i = 0; i < n; i++) p[i] = arena_byte(seed, i); }
    ~Arena() { free(p); }
};

static std::string walk(uint32_t n, uint32_t nb, uint32_t bl, const Arena &ar, uint32_t src_res, uint32_t dst_res, const std::vector<uint8_t> &depths, const std::vector<uint8_t> &active,
                        const std::vector<uint64_t> &table) {
    const uint64_t src0 = 0x7f0000001000ull + src_res, dst0 = 0x7e0000002000ull + dst_res;      // (addresses only: nothing is read through them)
    const uint64_t packet = 6ull * bl, run = packet * nb;
    std::vector<uint8_t> dst(run * n, 0xcc);
    std::vector<uint32_t> writes(run * n, 0u);
    const uint32_t tiles = packet_tiles(bl);
    const uint64_t jobs = (uint64_t)n * nb * tiles;
    const uint32_t wgs = (uint32_t)((jobs + kPacketJobsPerWg - 1) / kPacketJobsPerWg);
    std::vector<uint8_t> image(kPacketImage), stored(kPacketImage);
    uint64_t seen_jobs = 0;
    for (uint32_t wg = 0; wg < wgs; wg++) {
        for (uint32_t group = 0; group < kPacketJobsPerWg; group++) {
            const uint64_t job = packet_job_index(wg, group);
            if (job >= jobs) continue;
            seen_jobs++;
            uint32_t s, k, t;
            packet_job(job, nb, tiles, &s, &k, &t);
            if (s >= n || k >= nb || t >= tiles) return "FAIL a job outside the table";
            if (!active[s]) continue;
            const bool wide = depths[s] == 24;
            const uint64_t e0 = src0 + table[(uint64_t)s * nb + k], e1 = e0 + (uint64_t)bl * intake_frame_bytes(depths[s]);      // the entry, as addresses
            PacketTile T;
            if (!packet_tile(dst0 + run * s + packet * k, e0, bl, wide, t, &T)) continue;
            if (T.sb - T.image0 > kPacketImage) return "FAIL the source range does not fit the image";
            std::fill(stored.begin(), stored.end(), 0);
            auto load = [&](uint64_t p, uint32_t bytes) -> bool {      // a load of `bytes` at address p into the image
                if (p % bytes || p < e0 || p + bytes > e1 || p < T.image0 || p + bytes - T.image0 > kPacketImage) return false;
                memcpy(&image[p - T.image0], ar.p + (p - src0), bytes);
                for (uint32_t b = 0; b < bytes; b++) { if (stored[p - T.image0 + b]) return false; stored[p - T.image0 + b] = 1; }
                return true;
            };
            for (uint32_t lane = 0; lane < kPacketLanes; lane++) {
                uint64_t p;
                for (uint32_t i = 0; packet_src_piece(T, lane, i, &p); i++) if (!load(p, 16)) return "FAIL a 16-byte source load outside its entry, misaligned or repeated";
                if (packet_src_head(T, lane, &p) && !load(p, 2)) return "FAIL a head word outside its entry, misaligned or repeated";
                if (packet_src_tail(T, lane, &p) && !load(p, 2)) return "FAIL a tail word outside its entry, misaligned or repeated";
            }
            bool bad = false;
            auto word = [&](uint32_t j) -> uint32_t {
                uint32_t r;
                const uint64_t q = packet_word_src(T, wide, j, &r);
                if (q < T.image0 || q + 2 - T.image0 > kPacketImage || !stored[q - T.image0] || !stored[q - T.image0 + 1]) { bad = true; return 0; }
                return packet_word_make((uint32_t)image[q - T.image0] | (uint32_t)image[q - T.image0 + 1] << 8, r);
            };
            auto store = [&](uint64_t q, uint32_t v) {      // a 2-byte store at address q
                if (q % 2 || q < dst0 + run * s + packet * k || q + 2 > dst0 + run * s + packet * (k + 1)) { bad = true; return; }
                dst[q - dst0] = (uint8_t)v; dst[q - dst0 + 1] = (uint8_t)(v >> 8);
                writes[q - dst0]++; writes[q - dst0 + 1]++;
            };
            for (uint32_t lane = 0; lane < kPacketLanes; lane++) {
                uint64_t p;
                bool whole;
                for (uint32_t i = 0; packet_dst_piece(T, lane, i, &p, &whole); i++) {
                    if (p % 16) return "FAIL a destination piece is not aligned";
                    for (uint32_t w = 0; w < 8; w++) {
                        const uint64_t q = p + 2u * w;
                        if (whole || (q >= T.ta && q < T.tb)) store(q, word((uint32_t)(q - T.ta) / 2u));
                    }
                }
            }
            if (bad) return "FAIL a destination word outside its packet, or made from an image word that was not stored";
        }
    }
    if (seen_jobs != jobs) return "FAIL the workgroups do not cover the jobs";
    std::vector<uint8_t> want(run);
    for (uint32_t s = 0; s < n; s++) {
        for (uint64_t b = 0; b < run; b++)
            if (writes[run * s + b] != (active[s] ? 1u : 0u)) return "FAIL a destination byte written " + std::to_string(writes[run * s + b]) + " times (stream " + std::to_string(s) + ", byte " + std::to_string(b) + ")";
        if (!active[s]) continue;
        packets_gather_cpu(want.data(), ar.p, &table[(uint64_t)s * nb], depths[s], nb, bl);
        if (memcmp(want.data(), &dst[run * s], run)) return "FAIL the bytes differ from packets_gather_cpu's (stream " + std::to_string(s) + ")";
    }
    return "ok " + hex(dst.data(), dst.size());
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        auto bytes = [&](size_t n) { std::vector<uint8_t> v(n); for (auto &x : v) { unsigned u; in >> u; x = (uint8_t)u; } return v; };
        auto words = [&](size_t n) { std::vector<uint64_t> v(n); for (auto &x : v) in >> x; return v; };
        if (cmd == "check") {
            uint32_t n, nb, bl, max_bl; uint64_t arena_bytes;
            in >> n >> nb >> bl >> max_bl >> arena_bytes;
            const std::vector<uint8_t> depths = bytes(n), active = bytes(n);
            // (a table that the check must refuse before it looks at it is not allocated: n * nb may be huge)
            const bool early = !nb || !bl || bl > max_bl || (uint64_t)n * nb > kPacketMaxEntries;
            const std::vector<uint64_t> table = words(early ? 0 : (size_t)n * nb);
            uint64_t at = ~0ull;
            switch (packets_check(depths.data(), table.data(), n, nb, bl, max_bl, arena_bytes, active.data(), &at)) {
            case PacketsBad::Ok: printf("ok\n"); break;
            case PacketsBad::Lengths: printf("lengths\n"); break;
            case PacketsBad::Depth: printf("depth %llu\n", (unsigned long long)at); break;
            case PacketsBad::Overflow: printf("overflow\n"); break;
            case PacketsBad::Entry: printf("entry %llu\n", (unsigned long long)at); break;
            }
        } else if (cmd == "gather") {
            unsigned depth; uint32_t nb, bl; uint64_t arena_bytes, seed;
            in >> depth >> nb >> bl >> arena_bytes >> seed;
            const std::vector<uint64_t> row = words(nb);
            const Arena ar(arena_bytes, seed);
            std::vector<uint8_t> dst((size_t)6 * bl * nb);
            packets_gather_cpu(dst.data(), ar.p, row.data(), (uint8_t)depth, nb, bl);
            printf("%s\n", hex(dst.data(), dst.size()).c_str());
        } else if (cmd == "walk") {
            uint32_t n, nb, bl, src_res, dst_res; uint64_t arena_bytes, seed;
            in >> n >> nb >> bl >> arena_bytes >> seed >> src_res >> dst_res;
            const std::vector<uint8_t> depths = bytes(n), active = bytes(n);
            const std::vector<uint64_t> table = words((size_t)n * nb);
            const Arena ar(arena_bytes, seed);
            printf("%s\n", walk(n, nb, bl, ar, src_res, dst_res, depths, active, table).c_str());
        } else {
            printf("?\n");
        }
        if (!in) { fprintf(stderr, "packets_driver: a short line: %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
