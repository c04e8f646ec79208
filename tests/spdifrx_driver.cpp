// spdifrx_driver.cpp — dspi_amd/csrc/dspi_spdifrx.{h,cpp} without a GPU (tests/test_spdif_rx_cpu.py).  One command per input line, one line
// of output each:
//   line  <split> <record hex> <words hex>   the CPU receiver over the frames, in two calls cut at frame <split> (0 or >= frames: one call), the
//                                            record carried: "<record hex> <pairs hex> <packed hex>"
//   walk  <split> <record hex> <words hex>   the same through the KERNEL's arithmetic on the host: 64-frame chunks as bit masks, rx_walk for the
//                                            sync machine, popcounts for the counters, nearest-lower-good-frame for the hold
//   off   <frames> <source> ...              sources_offsets: "<total> <offset 0> ... <offset n>" or "overflow"
//   check <source> ...                       "<sources_check> <sources_any_spdif>"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_spdifrx.h"

using namespace dspi;

static std::vector<uint8_t> unhex(const std::string &s) {
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

// the kernel's way (dspi_spdifrx.hip), a lane being an index of a loop
static void line_by_chunks(SpdifRx *rx, const uint32_t *w, uint64_t frames, int32_t *pairs) {
    uint64_t cbits = 0;
    memcpy(&cbits, rx->c_bits, 8);
    bool any_ok = false;
    for (uint64_t base = 0; base < frames; base += 64) {
        const uint32_t nv = frames - base < 64 ? (uint32_t)(frames - base) : 64u;
        uint64_t bad[2] = {0, 0}, z = 0, c = 0, par[2] = {0, 0}, good[2] = {0, 0};
        int32_t smp[64][2];
        for (uint32_t i = 0; i < nv; i++) {
            const uint32_t *f = w + 4 * (base + i);
            const bool ok[2] = {rx_left_ok(f[0], f[1]), rx_right_ok(f[2], f[3])};
            const uint32_t d[2] = {rx_data(f[0], f[1]), rx_data(f[2], f[3])};
            if (ok[0] && (f[0] & 0xffu) == kPreZ) z |= 1ull << i;
            if (rx_c(d[0])) c |= 1ull << i;
            for (int s = 0; s < 2; s++) {
                if (!ok[s]) bad[s] |= 1ull << i;
                if (ok[s] && rx_parity_fails(d[s])) par[s] |= 1ull << i;
                if (ok[s] && !rx_v(d[s])) good[s] |= 1ull << i;
                smp[i][s] = rx_sample(d[s]);
            }
        }
        const uint64_t valid = rx_low_bits(nv);
        any_ok = any_ok || (valid & ~(bad[0] & bad[1]));
        RxWalk walk{rx->sync, rx->sample_rate, cbits, -1};
        rx_walk(walk, nv, bad[0], bad[1], z, c);
        rx->sync = walk.sync; rx->sample_rate = walk.rate; cbits = walk.cbits;
        const uint64_t counted = walk.lock_lane < 0 ? ~0ull : ~rx_low_bits((uint32_t)walk.lock_lane);
        rx->parity_err_count = (walk.lock_lane < 0 ? rx->parity_err_count : 0u) + (uint32_t)__builtin_popcountll(par[0] & counted) + (uint32_t)__builtin_popcountll(par[1] & counted);
        for (int s = 0; s < 2; s++) {
            rx->coding_errors += (uint32_t)__builtin_popcountll(bad[s]);
            rx->held += (uint32_t)__builtin_popcountll(valid & ~good[s]);
            for (uint32_t i = 0; i < nv; i++) {
                const uint64_t g = good[s] & rx_low_bits(i);
                pairs[2 * (base + i) + s] = (good[s] >> i & 1u) ? smp[i][s] : g ? smp[63 - __builtin_clzll(g)][s] : rx->hold[s];
            }
            if (good[s]) rx->hold[s] = smp[63 - __builtin_clzll(good[s])][s];
        }
    }
    memcpy(rx->c_bits, &cbits, 8);
    rx->state = rx->sync ? 2u : any_ok ? 1u : 0u;
}

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string cmd;
        in >> cmd;
        if (cmd == "line" || cmd == "walk") {
            uint64_t split;
            std::string rec_hex, words_hex;
            in >> split >> rec_hex >> words_hex;
            const std::vector<uint8_t> rec = unhex(rec_hex), words = unhex(words_hex);
            if (rec.size() != sizeof(SpdifRx) || words.size() % kRxFrameBytes) { puts("bad input"); continue; }
            SpdifRx rx;
            memcpy(&rx, rec.data(), sizeof rx);
            const uint64_t frames = words.size() / kRxFrameBytes;
            if (split > frames) split = frames;
            std::vector<int32_t> pairs(2 * frames);
            std::vector<uint8_t> packed(6 * frames);
            std::vector<uint32_t> w(4 * frames);
            memcpy(w.data(), words.data(), words.size());
            const uint64_t cut[3] = {0, split, frames};
            for (int k = 0; k < 2; k++) {
                const uint64_t a = cut[k], n = cut[k + 1] - a;
                if (!n) continue;
                if (cmd == "line") spdifrx_line_cpu(&rx, words.data() + a * kRxFrameBytes, n, pairs.data() + 2 * a, packed.data() + 6 * a);
                else line_by_chunks(&rx, w.data() + 4 * a, n, pairs.data() + 2 * a);
            }
            if (cmd == "walk")
                for (uint64_t k = 0; k < 2 * frames; k++)
                    for (int b = 0; b < 3; b++) packed[3 * k + b] = (uint8_t)((uint32_t)pairs[k] >> 8 * b);
            printf("%s %s %s\n", hex(&rx, sizeof rx).c_str(), hex(pairs.data(), pairs.size() * 4).c_str(), hex(packed.data(), packed.size()).c_str());
        } else if (cmd == "off") {
            uint64_t frames, total = 0;
            in >> frames;
            std::vector<uint8_t> src;
            for (unsigned v; in >> v;) src.push_back((uint8_t)v);
            std::vector<uint64_t> off(src.size() + 1, 0);
            if (!sources_offsets(src.data(), (uint32_t)src.size(), frames, &total, off.data())) { puts("overflow"); continue; }
            std::string s = std::to_string(total);
            for (uint64_t o : off) s += " " + std::to_string(o);
            puts(s.c_str());
        } else if (cmd == "check") {
            std::vector<uint8_t> src;
            for (unsigned v; in >> v;) src.push_back((uint8_t)v);
            printf("%u %d\n", sources_check(src.data(), (uint32_t)src.size()), (int)sources_any_spdif(src.data(), (uint32_t)src.size()));
        } else puts("unknown command");
    }
    return 0;
}
