// packets_out_driver.cpp — dspi_amd/csrc/dspi_packets_out.{h,cpp} without a GPU, for tests/test_packets_out_cpu.py: one command per line of stdin,
// one line of answer each.  The arena of a command is allocated at exactly arena_bytes and the source at exactly its layout's size, so that an
// access past either is a sanitizer finding; the arena's bytes are arena_byte(seed, i) and the source's words src_word(seed, i), which the
// Python side computes too.  R = 0: the stream-major source [n][P][F][2]; R > 0: the tiled one [tiles][2 P][F][R].
//   check n P nb bl max_bl arena_bytes overlap  formats[n]  active[n]  table[n * P * nb]   ->  ok | lengths | format S | overflow | entry I | overlap I
//   emit n P nb bl R arena_bytes seed  formats[n]  active[n]  table[n * P * nb]            ->  the arena after packets_emit_cpu for every active stream, in hex
//   walk n P nb bl R arena_bytes seed dst_res  formats[n]  active[n]  table[n * P * nb]
//         the kernel's address functions (R = 0: packettx_major_kernel, else packettx_tiled_kernel<R>) for every workgroup, lane group, lane
//         and iteration, with the arena at an address of residue dst_res mod 16, through emulated LDS images  ->  "ok " + the arena in hex,
//         after asserting: every source access aligned to its width, inside the source buffer and inside the frames of a packet that an
//         active stream emits; every image byte that is read was stored, and stored once; every 16-byte store aligned; every store inside
//         the entry of its own packet; every byte of an entry written exactly once and no other byte at all; the arena equal to
//         packets_emit_cpu's; else "FAIL why".  The table's entries must not overlap.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_packets_out.h"

using namespace dspi;

static uint8_t arena_byte(uint64_t seed, uint64_t i) { return (uint8_t)((i * 131u + seed * 17u + (i >> 8) * 7u + 1u) & 0xffu); }
static int32_t src_word(uint64_t seed, uint64_t i) { return (int32_t)(uint32_t)((i * 2654435761ull + seed * 40503ull + (i >> 7) * 97ull + 12345ull) & 0xffffffffull); }

static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; i++) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
    return s;
}

struct Buffers {      // exactly as long as they are said to be
    uint8_t *arena;
    int32_t *src;
    uint64_t arena_bytes, src_words;
    Buffers(uint64_t ab, uint64_t words, uint64_t seed) : arena(static_cast<uint8_t *>(malloc(ab ? ab : 1))), src(static_cast<int32_t *>(malloc(words ? words * 4 : 1))), arena_bytes(ab), src_words(words) {
        for (uint64_t i = 0; i < ab; i++) arena[i] = arena_byte(seed, i);
        for (uint64_t i = 0; i < words; i++) src[i] = src_word(seed, i);
    }
    ~Buffers() { free(arena); free(src); }
};

static uint64_t source_words(uint32_t n, uint32_t P, uint32_t nb, uint32_t bl, uint32_t R) {
    const uint64_t F = (uint64_t)nb * bl;
    return R ? (uint64_t)((n + R - 1) / R) * 2u * P * F * R : (uint64_t)n * P * F * 2u;
}

struct Walk {
    uint32_t n, P, nb, bl, R;
    const Buffers &B;
    const std::vector<uint8_t> &formats, &active;
    const std::vector<uint64_t> &table;
    uint64_t src0, dst0;
    std::vector<uint8_t> out;
    std::vector<uint32_t> writes;
    std::string why;

    bool fail(const std::string &w) { if (why.empty()) why = w; return false; }
    bool emits(uint32_t s, uint32_t p, uint32_t k) const { return s < n && active[s] && table[emit_entry_index(s, p, k, P, nb)] != kPacketSkip; }
    // a source load of `words` 4-byte words at address p, all of them words of frames [f_lo, f_hi) of packet (s, pair, k) — stream-major — or,
    // tiled, words of row `side` of frame f_lo of columns whose streams emit (pair, k)
    bool load_ok(uint64_t p, uint32_t words) {
        if (p % (4u * words)) return fail("a source load is not aligned to its width");
        if (p < src0 || p + 4ull * words > src0 + 4ull * B.src_words) return fail("a source load outside the buffer");
        return true;
    }
    // a destination store of `bytes` at address q, inside entry [e0, e1)
    bool store(uint64_t q, uint32_t bytes, const uint8_t *v, uint64_t e0, uint64_t e1) {
        if (q % bytes) return fail("a destination store is not aligned to its width");
        if (q < e0 || q + bytes > e1) return fail("a destination store outside its entry");
        if (q < dst0 || q + bytes > dst0 + B.arena_bytes) return fail("a destination store outside the arena");
        for (uint32_t b = 0; b < bytes; b++) { out[q - dst0 + b] = v[b]; writes[q - dst0 + b]++; }
        return true;
    }
    // a span out of its image (bytes, with what was stored), by the 16 lanes of a group
    bool span_out(const EmitSpan &S, const std::vector<uint8_t> &image, const std::vector<uint8_t> &stored, uint32_t read_width, uint64_t e0, uint64_t e1) {
        for (uint32_t lane = 0; lane < kEmitLanes; lane++) {
            uint64_t p;
            bool whole;
            for (uint32_t i = 0; emit_dst_piece(S, lane, i, &p, &whole); i++) {
                if (p % 16) return fail("a destination piece is not aligned");
                if (whole) {
                    const uint64_t at = p - S.image0;
                    if (p < S.image0 || at % read_width || at + 16 > image.size()) return fail("a whole piece is read outside the image or misaligned in it");
                    for (uint32_t b = 0; b < 16; b++) if (!stored[at + b]) return fail("a whole piece reads an image byte that was not stored");
                    if (!store(p, 16, &image[at], e0, e1)) return false;
                } else {
                    for (uint32_t w = 0; w < 8; w++) {
                        const uint64_t q = p + 2u * w;
                        if (q < S.a || q >= S.b) continue;
                        const uint64_t at = q - S.image0;
                        if (at + 2 > image.size() || !stored[at] || !stored[at + 1]) return fail("a partial piece reads an image word that was not stored");
                        if (!store(q, 2, &image[at], e0, e1)) return false;
                    }
                }
            }
        }
        return true;
    }
    // a frame into an image, as put_frame does
    bool put(const EmitSpan &S, std::vector<uint8_t> &image, std::vector<uint8_t> &stored, uint32_t f, uint32_t l, uint32_t r) {
        uint16_t w[4];
        const uint32_t nw = emit_frame_words(l, r, S.fb, w), at = emit_frame_at(S, f);
        if (at % 2 || at + 2u * nw > image.size()) return fail("a frame does not fit its image");
        for (uint32_t i = 0; i < nw; i++)
            for (uint32_t b = 0; b < 2; b++) {
                if (stored[at + 2 * i + b]) return fail("an image byte is stored twice");
                stored[at + 2 * i + b] = 1; image[at + 2 * i + b] = (uint8_t)(w[i] >> (8 * b));
            }
        return true;
    }

    bool major() {
        const uint64_t entries = (uint64_t)n * P * nb;
        const uint32_t wgs = (uint32_t)((entries + kEmitGroups - 1) / kEmitGroups);
        std::vector<uint8_t> image(kEmitMajorPitch), stored(kEmitMajorPitch);
        uint64_t seen = 0;
        for (uint32_t wg = 0; wg < wgs; wg++)
            for (uint32_t group = 0; group < kEmitGroups; group++) {
                const uint64_t e = emit_major_entry(wg, group);
                if (e >= entries) continue;
                seen++;
                const uint32_t s = emit_major_stream(e, P, nb);
                if (s >= n) return fail("an entry outside the table");
                if (!active[s] || table[e] == kPacketSkip) continue;
                const EmitSpan S = emit_major_span(dst0, table[e], formats[s], bl);
                const uint64_t e0 = dst0 + table[e], e1 = e0 + (uint64_t)bl * emit_frame_bytes(formats[s]);
                if (S.a != e0 || S.b != e1 || S.image0 > S.a || S.image0 % 16) return fail("the span is not the entry");
                const uint64_t run0 = src0 + 8ull * e * bl;      // the packet's own run: [stream][pair][F][2]
                std::fill(stored.begin(), stored.end(), 0);
                for (uint32_t lane = 0; lane < kEmitLanes; lane++) {
                    uint32_t f;
                    uint64_t p;
                    for (uint32_t i = 0; emit_major_src(src0, e, bl, lane, i, &f, &p); i++) {
                        if (!load_ok(p, 2)) return false;
                        if (p != run0 + 8ull * f || f >= bl) return fail("a source load outside the packet's own run");
                        const uint64_t at = (p - src0) / 4;
                        if (!put(S, image, stored, f, (uint32_t)B.src[at], (uint32_t)B.src[at + 1])) return false;
                    }
                }
                if (!span_out(S, image, stored, 16, e0, e1)) return false;
            }
        if (seen != entries) return fail("the workgroups do not cover the entries");
        return true;
    }

    bool tiled() {
        const uint64_t wgs = emit_tiled_workgroups(n, R, P, nb, bl), F = (uint64_t)nb * bl;
        std::vector<std::vector<uint8_t>> image(R, std::vector<uint8_t>(kEmitTiledPitch * 4)), stored(R, std::vector<uint8_t>(kEmitTiledPitch * 4));
        std::vector<uint64_t> info(R);
        std::vector<uint32_t> chunk_frames((size_t)((n + R - 1) / R) * P * nb, 0u);
        for (uint64_t wg = 0; wg < wgs; wg++) {
            const EmitTiledJob J = emit_tiled_job(wg, P, nb, bl);
            if (J.tile >= (n + R - 1) / R || J.pair >= P || J.k >= nb || J.f0 % kEmitChunk || J.f0 + J.nf > bl || !J.nf) return fail("a job outside the table");
            chunk_frames[((size_t)J.tile * P + J.pair) * nb + J.k] += J.nf;
            for (uint32_t c = 0; c < R; c++) {      // step 0, as the kernel does it
                const uint64_t s = (uint64_t)J.tile * R + c;
                info[c] = emits((uint32_t)(s < n ? s : n), J.pair, J.k) ? table[emit_entry_index((uint32_t)s, J.pair, J.k, P, nb)] | (formats[s] == 24 ? 1u : 0u) : kPacketSkip;
                std::fill(stored[c].begin(), stored[c].end(), 0);
            }
            auto span_of = [&](uint64_t word) { return emit_tiled_span(dst0, word & ~1ull, (word & 1u) ? 24u : 32u, J); };
            for (uint32_t tid = 0; tid < kEmitThreads; tid++) {      // step 1
                uint32_t fr, q;
                uint64_t pl, pr;
                for (uint32_t i = 0; emit_tiled_src(src0, J, R, P, nb, bl, tid, i, &fr, &q, &pl, &pr); i++) {
                    if (4 * q + 3 >= R || fr >= J.nf) return fail("a row piece outside the chunk");
                    uint32_t mask = 0;
                    for (uint32_t j = 0; j < 4; j++) mask |= (info[4 * q + j] != kPacketSkip) << j;
                    if (!mask) continue;
                    // where the words of this frame of these columns really are: [tile][2 pair + side][F][R]
                    const uint64_t frame = (uint64_t)J.k * bl + J.f0 + fr;
                    const uint64_t want_l = src0 + 4ull * ((((uint64_t)J.tile * 2 * P + 2 * J.pair) * F + frame) * R + 4 * q), want_r = want_l + 4ull * F * R;
                    if (pl != want_l || pr != want_r) return fail("a row piece is not the frame's words of its columns");
                    if (emit_tiled_whole(mask)) { if (mask != 15u || !load_ok(pl, 4) || !load_ok(pr, 4)) return fail("a 16-byte row load that covers a column which emits nothing, or is misaligned"); }
                    for (uint32_t j = 0; j < 4; j++) {
                        if (!(mask >> j & 1u)) continue;      // (not read: a column that emits nothing)
                        if (!emit_tiled_whole(mask) && (!load_ok(pl + 4 * j, 1) || !load_ok(pr + 4 * j, 1))) return false;
                        const uint32_t c = 4 * q + j;
                        if (!put(span_of(info[c]), image[c], stored[c], fr, (uint32_t)B.src[(pl - src0) / 4 + j], (uint32_t)B.src[(pr - src0) / 4 + j])) return false;
                    }
                }
            }
            std::vector<uint8_t> served(R, 0);
            for (uint32_t group = 0; group < kEmitGroups; group++) {      // step 2
                uint32_t c;
                for (uint32_t i = 0; emit_tiled_col(R, group, i, &c); i++) {
                    if (c >= R || served[c]++) return fail("a column served twice or outside the tile");
                    if (info[c] == kPacketSkip) continue;
                    const EmitSpan S = span_of(info[c]);
                    const uint32_t s = J.tile * R + c;
                    const uint64_t e0 = dst0 + table[emit_entry_index(s, J.pair, J.k, P, nb)], e1 = e0 + (uint64_t)bl * emit_frame_bytes(formats[s]);
                    if (S.a != e0 + (uint64_t)S.fb * J.f0 || S.b != S.a + (uint64_t)S.fb * J.nf || S.b > e1 || S.image0 > S.a || S.image0 % 4) return fail("the span is not the chunk's part of the entry");
                    if (!span_out(S, image[c], stored[c], 4, e0, e1)) return false;
                }
            }
            for (uint32_t c = 0; c < R; c++) if (!served[c]) return fail("a column is not served");
        }
        for (uint32_t f : chunk_frames) if (f != bl) return fail("the workgroups do not cover the packets' frames");
        return true;
    }

    std::string run() {
        out.assign(B.arena, B.arena + B.arena_bytes);
        writes.assign(B.arena_bytes, 0u);
        if (!(R ? tiled() : major())) return "FAIL " + why;
        // every byte of an entry exactly once, no other byte at all; the bytes packets_emit_cpu's
        std::vector<uint32_t> want_writes(B.arena_bytes, 0u);
        std::vector<uint8_t> want(B.arena, B.arena + B.arena_bytes);
        for (uint32_t s = 0; s < n; s++) {
            if (!active[s]) continue;
            for (uint64_t i = 0; i < (uint64_t)P * nb; i++) {
                const uint64_t o = table[(uint64_t)s * P * nb + i];
                if (o != kPacketSkip) for (uint64_t b = 0; b < (uint64_t)bl * emit_frame_bytes(formats[s]); b++) want_writes[o + b]++;
            }
            packets_emit_cpu(want.data(), B.src, &table[(uint64_t)s * P * nb], formats[s], s, P, nb, bl, R);
        }
        for (uint64_t b = 0; b < B.arena_bytes; b++)
            if (writes[b] != want_writes[b]) return "FAIL arena byte " + std::to_string(b) + " written " + std::to_string(writes[b]) + " times, " + std::to_string(want_writes[b]) + " entries cover it";
        if (memcmp(want.data(), out.data(), B.arena_bytes)) return "FAIL the bytes differ from packets_emit_cpu's";
        return "ok " + hex(out.data(), out.size());
    }
};

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        auto bytes = [&](size_t n) { std::vector<uint8_t> v(n); for (auto &x : v) { unsigned u; in >> u; x = (uint8_t)u; } return v; };
        auto words = [&](size_t n) { std::vector<uint64_t> v(n); for (auto &x : v) in >> x; return v; };
        if (cmd == "check") {
            uint32_t n, P, nb, bl, max_bl, overlap; uint64_t arena_bytes;
            in >> n >> P >> nb >> bl >> max_bl >> arena_bytes >> overlap;
            const std::vector<uint8_t> formats = bytes(n), active = bytes(n);
            // (a table that the check must refuse before it looks at it is not allocated: it may be huge)
            bool early = !nb || !bl || bl > max_bl || (uint64_t)n * P * nb > kPacketMaxEntries;
            for (uint8_t f : formats) early = early || (f != 24 && f != 32);
            const std::vector<uint64_t> table = words(early ? 0 : (size_t)n * P * nb);
            uint64_t at = ~0ull;
            switch (packets_emit_check(formats.data(), table.data(), n, P, nb, bl, max_bl, arena_bytes, active.data(), overlap != 0, &at)) {
            case EmitBad::Ok: printf("ok\n"); break;
            case EmitBad::Lengths: printf("lengths\n"); break;
            case EmitBad::Format: printf("format %llu\n", (unsigned long long)at); break;
            case EmitBad::Overflow: printf("overflow\n"); break;
            case EmitBad::Entry: printf("entry %llu\n", (unsigned long long)at); break;
            case EmitBad::Overlap: printf("overlap %llu\n", (unsigned long long)at); break;
            }
        } else if (cmd == "emit" || cmd == "walk") {
            uint32_t n, P, nb, bl, R, dst_res = 0; uint64_t arena_bytes, seed;
            in >> n >> P >> nb >> bl >> R >> arena_bytes >> seed;
            if (cmd == "walk") in >> dst_res;
            const std::vector<uint8_t> formats = bytes(n), active = bytes(n);
            const std::vector<uint64_t> table = words((size_t)n * P * nb);
            const Buffers B(arena_bytes, source_words(n, P, nb, bl, R), seed);
            if (cmd == "emit") {
                for (uint32_t s = 0; s < n; s++)
                    if (active[s]) packets_emit_cpu(B.arena, B.src, &table[(uint64_t)s * P * nb], formats[s], s, P, nb, bl, R);
                printf("%s\n", hex(B.arena, arena_bytes).c_str());
            } else {
                // (addresses only: nothing is read through them)
                Walk w{n, P, nb, bl, R, B, formats, active, table, 0x7f0000001000ull, 0x7e0000002000ull + dst_res, {}, {}, {}};
                printf("%s\n", w.run().c_str());
            }
        } else {
            printf("?\n");
        }
        if (!in) { fprintf(stderr, "packets_out_driver: a short line: %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
