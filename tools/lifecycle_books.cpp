// tools/lifecycle_books.cpp — a stand-alone program (its own main) that drives the parameter books of host-only contexts, for runs under
// AddressSanitizer + UBSan: `make -C dspi_amd/csrc lifecycle_books_asan && dspi_amd/csrc/lifecycle_books_asan [contexts] [ops] [seed]`.
// tests/test_lifecycle_cpu.py builds it against the plain library and runs it briefly; there the program's own checks are the test.
// It is a vehicle for the sanitizers, NOT tests/lifecycle_model.py's host_schedule in another language: it draws its own sequences (xorshift) over
// the same kinds of call, and it has no oracle, so its checks are weaker than tests/test_lifecycle_cpu.py::test_host_only_books, which compares
// every stream's parameters with an oracle's.
//
// Random legal sequences of requests (single stream and broadcast), pauses, resumes, boots, S/PDIF mode and positions, compaction plans, image
// counts and the calls a host-only context refuses after validating them, on contexts of 3, 131 and 300 streams of both flavours.  There is no
// oracle here; after every op the program checks what it can know by itself:
//   * a call addressed to one stream changes no other stream's dspi_collect_bulk; a refused call changes nobody's
//   * dspi_streams_paused and dspi_spdif_stream_pos are the program's own record
//   * dspi_plan_compaction is the documented pairing of H (paused slots below A) and T (active slots at or above A)
//   * dspi_debug_image_count lies between the number of distinct blobs and the number of streams
//   * booted streams all collect the same blob, the one a fresh context of one stream collects
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "dspi.h"

static uint64_t rng_state;
static uint32_t rnd() {      // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t below(uint32_t n) { return rnd() % n; }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) / 16777216.0f; }

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "lifecycle_books: seed %llu, op %d (%s): ", (unsigned long long)seed, op, what); fprintf(stderr, __VA_ARGS__); \
                                              fprintf(stderr, "\n"); return 1; } } while (0)

typedef std::string Blob;
static const size_t kBlob = 2896;      // what dspi_collect_bulk returns (include/dspi.h: REQ_GET_ALL_PARAMS)
enum { REQ_SET_EQ_PARAM = 0x42, REQ_SET_PREAMP = 0x44, REQ_SET_OUTPUT_DELAY = 0x78 };      // config.h:111-251, as dspi_amd/wire.py REQ names them

static Blob collect(dspi_ctx *c, int32_t s) {
    Blob b(kBlob, '\0');
    return dspi_collect_bulk(c, s, &b[0], kBlob) == (int)kBlob ? b : Blob();
}

static int one_context(uint64_t seed, int n_ops) {
    int op = -1; const char *what = "create";
    rng_state = 0x9E3779B97F4A7C15ull ^ (seed * 0xD1342543DE82EF95ull + 1);
    const int flavor = seed & 1 ? DSPI_FLAVOR_RP2350_F32_FMA : DSPI_FLAVOR_RP2040_Q28;
    const uint32_t sizes[3] = {3, 131, 300};
    const uint32_t S = sizes[(seed >> 1) % 3];
    const int n_out = (flavor & 0xFF) ? 9 : 5;
    dspi_ctx *c = nullptr, *fresh = nullptr;
    CHECK(dspi_create(&c, flavor, S, DSPI_DEVICE_NONE) == DSPI_OK && dspi_create(&fresh, flavor, 1, DSPI_DEVICE_NONE) == DSPI_OK, "dspi_create");
    const Blob power_on = collect(fresh, 0);
    std::vector<Blob> bulk(S);
    for (uint32_t s = 0; s < S; s++) bulk[s] = collect(c, s);
    CHECK(!power_on.empty() && bulk[0] == power_on, "a fresh context does not collect the power-on blob");
    std::vector<uint8_t> paused(S, 0), got_paused(S);
    std::vector<uint32_t> sp(S, 0), got_sp(S);
    bool mode = false;
    for (op = 0; op < n_ops; op++) {
        uint32_t first = below(S), count = 1 + below(S - first);
        if (rnd() & 1) count = count < 5 ? count : 1 + below(5);
        int32_t target = below(5) < 2 ? DSPI_ALL_STREAMS : (int32_t)below(S);
        bool refused = false;
        std::set<uint32_t> touched;      // streams whose parameters this op may change
        auto touch = [&](int32_t t) { if (t == DSPI_ALL_STREAMS) for (uint32_t s = 0; s < S; s++) touched.insert(s); else touched.insert((uint32_t)t); };
        switch (below(12)) {
        case 0: { what = "preamp"; float db = uniform(-12.f, 0.f); touch(target);
                  CHECK(dspi_vendor_set(c, target, REQ_SET_PREAMP, 0, &db, 4) == DSPI_OK, "%s", dspi_last_error(c)); break; }
        case 1: { what = "band"; touch(target);
                  struct { uint8_t ch, band, type, pad; float f, q, g; } p = {(uint8_t)below(2), (uint8_t)below(10), (uint8_t)(1 + below(3)), 0, uniform(100.f, 8000.f), uniform(0.5f, 2.f), uniform(-6.f, 6.f)};
                  CHECK(dspi_vendor_set(c, target, REQ_SET_EQ_PARAM, 0, &p, sizeof p) == DSPI_OK, "%s", dspi_last_error(c)); break; }
        case 2: { what = "output delay"; float ms = uniform(0.f, 9.f); touch(target);
                  CHECK(dspi_vendor_set(c, target, REQ_SET_OUTPUT_DELAY, (uint16_t)below(n_out), &ms, 4) == DSPI_OK, "%s", dspi_last_error(c)); break; }
        case 3: { what = "volume"; CHECK(dspi_set_host_volume(c, target, (int16_t)(-256 * (int)below(30))) == DSPI_OK, "%s", dspi_last_error(c)); break; }
        case 4: { what = "load_bulk of another stream's blob"; touch(target);
                  const Blob b = bulk[below(S)];
                  CHECK(dspi_load_bulk(c, target, b.data(), kBlob) == 0, "%s", dspi_last_error(c)); break; }
        case 5: { what = "pause"; CHECK(dspi_pause_streams(c, first, count) == (int)count, "%s", dspi_last_error(c));
                  for (uint32_t s = first; s < first + count; s++) paused[s] = 1;
                  break; }
        case 6: { what = "resume"; CHECK(dspi_resume_streams(c, first, count, rnd() & 1 ? DSPI_RESUME_AS_IS : 0) == (int)count, "%s", dspi_last_error(c));
                  for (uint32_t s = first; s < first + count; s++) paused[s] = 0;
                  break; }
        case 7: { what = "boot";
                  std::vector<uint32_t> list;
                  for (uint32_t s = first; s < first + count && list.size() < 8; s++) list.insert(list.begin() + below((uint32_t)list.size() + 1), s);
                  int sel = -1;
                  CHECK(dspi_boot_streams(c, list.data(), (uint32_t)list.size(), nullptr, 0, rnd() & 1 ? DSPI_BOOT_STREAMS_AS_IS : 0, &sel) == (int)list.size() && sel == 48, "%s", dspi_last_error(c));
                  for (uint32_t s : list) { touched.insert(s); sp[s] = 0; }
                  for (uint32_t s : list) CHECK(collect(c, (int32_t)s) == power_on, "booted stream %u does not collect the power-on blob", s);
                  break; }
        case 8: { what = "S/PDIF mode and positions";
                  if (!mode) { CHECK(dspi_spdif_per_stream(c, 1) == 1, "%s", dspi_last_error(c)); mode = true; }
                  std::vector<uint32_t> v(count);
                  for (auto &x : v) x = below(192);
                  CHECK(dspi_spdif_stream_pos(c, first, count, v.data(), nullptr) == (int)count, "%s", dspi_last_error(c));
                  for (uint32_t k = 0; k < count; k++) sp[first + k] = v[k];
                  break; }
        case 9: { what = "image count";
                  std::set<Blob> distinct(bulk.begin(), bulk.end());
                  const int n = dspi_debug_image_count(c);
                  CHECK(n >= (int)distinct.size() && n <= (int)S, "%d parameter objects for %zu distinct blobs on %u streams", n, distinct.size(), S);
                  break; }
        case 10: { what = "refused move";      // a swap of two slots is always legal
                  if (S < 2) break;
                  dspi_stream_move m[2]; m[0].src = m[1].dst = below(S); do m[0].dst = m[1].src = below(S); while (m[0].dst == m[0].src);
                  CHECK(dspi_move_streams(c, m, 2, rnd() & 1 ? DSPI_MOVE_AS_IS : 0) == DSPI_E_NODEVICE, "a host-only context took a move");
                  refused = true; break; }
        default: { what = "refused export / realign";
                  size_t hb = 0, sb = 0;
                  CHECK(dspi_snapshot_sizes(c, first, count, &hb, &sb) == DSPI_OK && hb >= 64 && sb % 16 == 0, "%s", dspi_last_error(c));
                  std::vector<uint8_t> head(hb), state(sb);
                  dspi_snapshot snap = {head.data(), hb, state.data(), sb};
                  CHECK(dspi_export_streams(c, first, count, &snap, 0) == DSPI_E_NODEVICE, "a host-only context exported");
                  CHECK(dspi_realign_streams(c, first, count) == DSPI_E_NODEVICE, "a host-only context realigned");
                  refused = true; break; }
        }
        CHECK(!refused || touched.empty(), "bookkeeping of the program itself");
        for (uint32_t s = 0; s < S; s++) {
            const Blob b = collect(c, (int32_t)s);
            CHECK(!b.empty(), "dspi_collect_bulk of stream %u: %s", s, dspi_last_error(c));
            CHECK(touched.count(s) || b == bulk[s], "the parameters of stream %u changed, which the call did not address", s);
            bulk[s] = b;
        }
        CHECK(dspi_streams_paused(c, 0, S, got_paused.data()) >= 0 && got_paused == paused, "dspi_streams_paused is not the program's record");
        if (mode) CHECK(dspi_spdif_stream_pos(c, 0, S, nullptr, got_sp.data()) == (int)S && got_sp == sp, "dspi_spdif_stream_pos is not the program's record");
        for (uint32_t one_way = 0; one_way < 2; one_way++) {
            uint32_t A = 0;
            for (uint32_t s = 0; s < S; s++) A += !paused[s];
            std::vector<uint32_t> H, T;
            for (uint32_t s = 0; s < A; s++) if (paused[s]) H.push_back(s);
            for (uint32_t s = A; s < S; s++) if (!paused[s]) T.push_back(s);
            std::vector<dspi_stream_move> want, got(2 * S + 1);
            for (size_t i = 0; i < H.size(); i++) { want.push_back({T[i], H[i]}); if (!one_way) want.push_back({H[i], T[i]}); }
            const int n = dspi_plan_compaction(c, got.data(), (uint32_t)got.size(), one_way ? DSPI_COMPACT_ONE_WAY : 0);
            CHECK(n == (int)want.size() && (n == 0 || !memcmp(got.data(), want.data(), (size_t)n * sizeof(dspi_stream_move))), "dspi_plan_compaction is not the documented pairing");
        }
    }
    dspi_destroy(fresh);
    dspi_destroy(c);
    return 0;
}

int main(int argc, char **argv) {
    const int contexts = argc > 1 ? atoi(argv[1]) : 30, n_ops = argc > 2 ? atoi(argv[2]) : 40;
    const uint64_t seed0 = argc > 3 ? strtoull(argv[3], nullptr, 0) : 0;
    for (int k = 0; k < contexts; k++)
        if (one_context(seed0 + (uint64_t)k, n_ops)) return 1;
    printf("lifecycle_books: %d contexts x %d ops, books consistent\n", contexts, n_ops);
    return 0;
}
