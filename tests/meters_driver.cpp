// meters_driver.cpp — dspi_amd/csrc/dspi_meters.{h,cpp} without a GPU (tests/test_meters_cpu.py).  One command per input line, one line of output
// each.  Every buffer is a heap block of exactly the size the interface states, so that a sanitized build sees any step outside it.
//   update <C> <n> <K> <hold> <decay> <active hex | -> <meters hex> <peaks hex>      meters_update_cpu: "<meters hex>"
//   stage  <C> <n> <K> <hold> <decay> <active hex | -> <meters hex> <peaks hex> <lead>  the same through the UPDATE KERNEL's arithmetic (meter_geom /
//                                            meter_chunk / meter_piece / meter_walk_at), a lane being an index of a loop, with `peaks` standing
//                                            <lead> bytes (even, 0..14) behind a 16-byte boundary: every global byte it loads must lie inside
//                                            peaks and belong to an active stream, whole vectors must be aligned, every LDS byte it writes must
//                                            lie inside the kernel's array, and every LDS byte a lane reads must have been written in this chunk:
//                                            "<meters hex>" or "fault: <what>"
//   alarms <C> <n> <level> <cap> <info 0|1> <meters hex | -> <clip hex | ->       meters_alarms_cpu: "<written> <total> <streams hex> <info hex>"
//   pack   <C> <clip> <peaks hex>                                                  status_pack: "<block hex>"
//   list   <n> <entry> ...                                                         clear_list_check: "<index>"
//   why_update <n> <C> <n_blocks> <hold> <decay> <flags> <peaks address> <meters address>   meters_update_why (nothing is dereferenced): the reason or "ok"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_meters.h"

using namespace dspi;

static std::vector<uint8_t> unhex(const std::string &s) {
    if (s == "-") return {};
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return v;
}
static std::string hex(const void *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; i++) { s[2 * i] = d[static_cast<const uint8_t *>(p)[i] >> 4]; s[2 * i + 1] = d[static_cast<const uint8_t *>(p)[i] & 15]; }
    return s;
}
template <class T>
static std::vector<T> as(const std::vector<uint8_t> &b) {
    std::vector<T> v(b.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}

// the update kernel (dspi_meterbridge.hip meters_update_kernel) with loops for its workgroups and lanes
static const char *update_by_stages(int C, uint32_t n, uint32_t K, uint32_t hold, uint32_t decay, const uint8_t *active, uint32_t *meters, const uint8_t *peaks, uint64_t base) {
    const MeterGeom geom = meter_geom(C);
    const uint64_t total = (uint64_t)n * K * (uint64_t)C * 2u;
    const auto on = [&](uint32_t s) { return !active || active[s]; };
    std::vector<uint8_t> lds(geom.lds_bytes);
    std::vector<uint8_t> written(geom.lds_bytes);
    for (uint32_t s0 = 0; s0 < n; s0 += geom.G) {
        const uint32_t g = n - s0 < geom.G ? n - s0 : geom.G;
        if (g * (uint32_t)C > kMeterLanes) return "more words than lanes";
        for (uint32_t k0 = 0; k0 < K; k0 += kMeterStagePackets) {
            const MeterChunk chunk = meter_chunk(C, s0, g, K, k0);
            std::fill(written.begin(), written.end(), (uint8_t)0);
            const uint32_t L = meter_piece_lanes(chunk);
            if (L == 0 || kMeterLanes % L) return "the lanes do not divide into pieces";
            for (uint32_t t = 0; t < kMeterLanes; t++)
                for (uint32_t piece = t / L; piece < chunk.n_pieces; piece += kMeterLanes / L) {
                    const MeterPiece pc = meter_piece(chunk, geom, base, piece);
                    const int64_t a0 = pc.origin + pc.lead, a1 = pc.origin + pc.end;      // the piece's bytes, from `peaks`
                    if (a0 < 0 || (uint64_t)a1 > total || (base + (uint64_t)a0) % 16u != pc.lead || pc.dst % 16u) return "a piece lies outside peaks, or its lead is not its address's";
                    if ((uint64_t)a0 != ((uint64_t)(s0 + piece) * K + k0) * (uint64_t)C * 2u || (uint64_t)(a1 - a0) != (uint64_t)(chunk.one ? g * K : (K - k0 < kMeterStagePackets ? K - k0 : kMeterStagePackets)) * C * 2u)
                        return "a piece is not its streams' packets";
                    for (uint32_t v = t % L; v * 16u < pc.end; v += L) {
                        if ((uint64_t)pc.dst + v * 16u + 16u > geom.lds_bytes) return "a vector lies outside the LDS array";
                        bool all = meter_vec_whole(pc, v);
                        if (all && active)
                            for (uint32_t s = meter_stream_of(chunk, pc, v * 16u), last = meter_stream_of(chunk, pc, v * 16u + 14u); s <= last; s++) all = all && on(s);
                        for (uint32_t e = 0; e < 8u; e++) {
                            const uint32_t rel = v * 16u + 2u * e;
                            const bool inside = rel >= pc.lead && rel < pc.end;
                            if (all ? !inside : !(inside && on(meter_stream_of(chunk, pc, rel)))) { if (all) return "a whole vector reaches outside its piece"; continue; }
                            const uint32_t s = meter_stream_of(chunk, pc, rel);
                            const uint64_t a = (uint64_t)(pc.origin + rel);
                            if (s >= n || !on(s) || a / ((uint64_t)K * (uint64_t)C * 2u) != s) return "a byte of the wrong stream is loaded";
                            if (written[pc.dst + rel]) return "an LDS element is written twice";
                            memcpy(&lds[pc.dst + rel], peaks + a, 2);
                            written[pc.dst + rel] = written[pc.dst + rel + 1u] = 1;
                        }
                    }
                }
            const uint32_t kc = K - k0 < kMeterStagePackets ? K - k0 : kMeterStagePackets;
            for (uint32_t t = 0; t < g * (uint32_t)C; t++) {
                const uint32_t sl = t / (uint32_t)C, ch = t % (uint32_t)C;
                if (!on(s0 + sl)) continue;
                const uint32_t at = meter_walk_at(chunk, geom, base, sl, ch);
                uint32_t word = meters[(size_t)s0 * C + t];
                for (uint32_t k = 0; k < kc; k++) {
                    const uint32_t o = at + k * (uint32_t)C * 2u;
                    if ((uint64_t)o + 2u > geom.lds_bytes || !written[o] || !written[o + 1u]) return "a lane reads LDS that was not written";
                    uint16_t p;
                    memcpy(&p, &lds[o], 2);
                    if (memcmp(&p, peaks + (((uint64_t)(s0 + sl) * K + k0 + k) * (uint64_t)C + ch) * 2u, 2)) return "a lane reads another element's peak";
                    word = meter_step(word, p, hold, decay);
                }
                meters[(size_t)s0 * C + t] = word;
            }
        }
    }
    return nullptr;
}

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string cmd;
        in >> cmd;
        if (cmd == "update" || cmd == "stage") {
            int C;
            uint32_t n, K, hold, decay, lead = 0;
            std::string active_hex, meters_hex, peaks_hex;
            in >> C >> n >> K >> hold >> decay >> active_hex >> meters_hex >> peaks_hex;
            if (cmd == "stage") in >> lead;
            const std::vector<uint8_t> active = unhex(active_hex), peaks = unhex(peaks_hex);
            std::vector<uint32_t> meters = as<uint32_t>(unhex(meters_hex));
            if ((C != 7 && C != 11) || meters.size() != (size_t)n * C || peaks.size() != (size_t)n * K * C * 2u || (!active.empty() && active.size() != n) || lead > 14u || lead % 2u) { puts("bad input"); continue; }
            if (cmd == "update") {
                // peaks as uint16 in a block of its own: exactly n K C elements
                std::vector<uint16_t> p = as<uint16_t>(peaks);
                meters_update_cpu(p.data(), n, K, C, hold, decay, meters.data(), active.empty() ? nullptr : active.data());
            } else if (const char *fault = update_by_stages(C, n, K, hold, decay, active.empty() ? nullptr : active.data(), meters.data(), peaks.data(), 4096u + lead)) {
                printf("fault: %s\n", fault);
                continue;
            }
            puts(hex(meters.data(), meters.size() * 4).c_str());
        } else if (cmd == "alarms") {
            int C, want_info;
            uint32_t n, level, cap, total = 0xdeadbeefu;
            std::string meters_hex, clip_hex;
            in >> C >> n >> level >> cap >> want_info >> meters_hex >> clip_hex;
            const std::vector<uint32_t> meters = as<uint32_t>(unhex(meters_hex));
            const std::vector<uint16_t> clip = as<uint16_t>(unhex(clip_hex));
            if ((!meters.empty() && meters.size() != (size_t)n * C) || (!clip.empty() && clip.size() != n)) { puts("bad input"); continue; }
            std::vector<uint32_t> streams(cap, 0xffffffffu), info(want_info ? cap : 0u, 0xffffffffu);
            const uint32_t w = meters_alarms_cpu(meters.empty() ? nullptr : meters.data(), clip.empty() ? nullptr : clip.data(), n, C, level, streams.data(),
                                                 want_info ? info.data() : nullptr, cap, &total);
            printf("%u %u %s- %s-\n", w, total, hex(streams.data(), (size_t)w * 4).c_str(), hex(info.data(), want_info ? (size_t)w * 4 : 0).c_str());
        } else if (cmd == "pack") {
            int C;
            unsigned clip;
            std::string peaks_hex;
            in >> C >> clip >> peaks_hex;
            const std::vector<uint16_t> peaks = as<uint16_t>(unhex(peaks_hex));
            if (peaks.size() != (size_t)C) { puts("bad input"); continue; }
            std::vector<uint8_t> block(status_block_bytes(C));
            status_pack(peaks.data(), (uint16_t)clip, C, block.data());
            puts(hex(block.data(), block.size()).c_str());
        } else if (cmd == "list") {
            uint32_t n;
            in >> n;
            std::vector<uint32_t> list;
            for (uint32_t v; in >> v;) list.push_back(v);
            printf("%u\n", clear_list_check(list.data(), (uint32_t)list.size(), n));
        } else if (cmd == "why_update") {
            int C;
            uint32_t n, n_blocks, hold, decay, flags;
            uint64_t peaks, meters;
            in >> n >> C >> n_blocks >> hold >> decay >> flags >> peaks >> meters;
            const char *why = meters_update_why(reinterpret_cast<const void *>(peaks), n_blocks, hold, decay, reinterpret_cast<const void *>(meters), flags, n, C);
            puts(why ? why : "ok");
        } else puts("unknown command");
    }
    return 0;
}
