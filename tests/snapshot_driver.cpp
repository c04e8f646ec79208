// snapshot_driver.cpp — the stream snapshot format (dspi_amd/csrc/dspi_snapshot.{h,cpp}) on the CPU, for tests/test_snapshot_cpu.py.
//   snapshot_driver layout                 per flavour: the numbers the layout derives from, then every section's offset / len / span
//   snapshot_driver head COUNT IMAGES      head bytes, state bytes (both flavours)
//   snapshot_driver write FLAVOR FMA COUNT IMAGES FILE    a well-formed head (placeholder parameter objects) into FILE
//   snapshot_driver validate               a well-formed head, then one corruption at a time: "<case>: <verdict>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_params.h"
#include "../dspi_amd/csrc/dspi_snapshot.h"

using namespace dspi;

static std::vector<uint64_t> make_head(int flavor, bool fma, uint32_t count, uint32_t n_images) {
    std::vector<uint64_t> buf((snap_head_bytes(count, n_images) + 7) / 8, 0);
    unsigned char *head = reinterpret_cast<unsigned char *>(buf.data());
    const SnapHeader h = snap_make_header(flavor, fma, count, n_images, true);
    memcpy(head, &h, sizeof h);
    for (uint32_t i = 0; i < n_images; i++) {      // (the constructor lives in dspi_params.cpp; validation reads these two members only)
        Params *p = reinterpret_cast<Params *>(head + sizeof h + i * snap_params_stride());
        p->flavor = flavor; p->fma_contract = fma; p->freq = 48000 + i;
    }
    uint32_t *idx = reinterpret_cast<uint32_t *>(head + sizeof h + n_images * snap_params_stride());
    for (uint32_t k = 0; k < count; k++) idx[k] = k % n_images;
    snap_seal(head);
    return buf;
}

static void verdict(const char *name, const std::vector<uint64_t> &buf, size_t bytes, int flavor, bool fma) {
    const char *why = snap_validate_head(buf.data(), bytes, flavor, fma);
    printf("%s: %s\n", name, why ? why : "ok");
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "layout") {
        for (int flavor = 0; flavor < 2; flavor++) {
            const StateMap m = make_state_map(flavor);
            const SnapLayout l = make_snap_layout(flavor);
            printf("flavor %d n_slots %d n_out %d max_delay %d ring %d pdm %d row %d record_words %u params %zu stride %zu header %zu\n", flavor, m.n_slots, m.n_out,
                   m.max_delay, kRingLen, kPdmWords, m.row, l.record_words, snap_params_bytes(), snap_params_stride(), sizeof(SnapHeader));
            for (int s = 0; s < SEC_COUNT; s++) printf("section %d %u %u %u\n", s, l.sec[s].offset, l.sec[s].len, l.sec[s].span);
        }
        return 0;
    }
    if (cmd == "head" && argc == 4) {
        const uint32_t count = (uint32_t)strtoul(argv[2], nullptr, 0), images = (uint32_t)strtoul(argv[3], nullptr, 0);
        printf("%zu %zu %zu\n", snap_head_bytes(count, images), snap_state_bytes(0, count), snap_state_bytes(1, count));
        return 0;
    }
    if (cmd == "write" && argc == 7) {
        const uint32_t count = (uint32_t)strtoul(argv[4], nullptr, 0), images = (uint32_t)strtoul(argv[5], nullptr, 0);
        const std::vector<uint64_t> head = make_head(atoi(argv[2]), atoi(argv[3]) != 0, count, images);
        FILE *f = fopen(argv[6], "wb");
        if (!f || fwrite(head.data(), 1, snap_head_bytes(count, images), f) != snap_head_bytes(count, images) || fclose(f) != 0) return 1;
        return 0;
    }
    if (cmd == "validate") {
        const uint32_t count = 5, images = 2;
        const std::vector<uint64_t> good = make_head(1, true, count, images);
        const size_t bytes = snap_head_bytes(count, images);
        verdict("ok", good, bytes, 1, true);
        verdict("longer buffer", good, bytes + 8, 1, true);
        verdict("other flavour context", good, bytes, 0, false);
        verdict("other contract context", good, bytes, 1, false);
        verdict("truncated", good, bytes - 1, 1, true);
        verdict("shorter than header", good, sizeof(SnapHeader) - 1, 1, true);
        struct Case { const char *name; size_t field; uint32_t value; };      // a header word set to `value`, nothing resealed
        const Case cases[] = {{"magic", offsetof(SnapHeader, magic), 0x12345678u}, {"version", offsetof(SnapHeader, version), kSnapVersion + 1},
                              {"flavor", offsetof(SnapHeader, flavor), 0u}, {"contract", offsetof(SnapHeader, contract), 0u},
                              {"fingerprint", offsetof(SnapHeader, fingerprint), snap_fingerprint(1) ^ 1u}, {"params size", offsetof(SnapHeader, params_bytes), 8u},
                              {"record size", offsetof(SnapHeader, record_words), make_snap_layout(1).record_words + 4}, {"count", offsetof(SnapHeader, count), count + 1},
                              {"count zero", offsetof(SnapHeader, count), 0u}, {"image count", offsetof(SnapHeader, n_images), count + 1},
                              {"image count zero", offsetof(SnapHeader, n_images), 0u}, {"image count other", offsetof(SnapHeader, n_images), images + 1},
                              {"head size", offsetof(SnapHeader, head_bytes), 64u}, {"crc", offsetof(SnapHeader, crc), 0u}, {"flags", offsetof(SnapHeader, flags), 0u}};
        for (const Case &c : cases) {
            std::vector<uint64_t> bad = good;
            memcpy(reinterpret_cast<unsigned char *>(bad.data()) + c.field, &c.value, 4);
            verdict(c.name, bad, bytes, 1, true);
        }
        {   // a byte of a parameter object, of the index
            std::vector<uint64_t> bad = good;
            reinterpret_cast<unsigned char *>(bad.data())[sizeof(SnapHeader) + 100] ^= 0x40;
            verdict("body byte", bad, bytes, 1, true);
            bad = good;
            reinterpret_cast<unsigned char *>(bad.data())[bytes - 2] ^= 0x01;
            verdict("index byte", bad, bytes, 1, true);
        }
        {   // resealed, so that the checks behind the CRC are reached
            std::vector<uint64_t> bad = good;
            uint32_t *idx = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(bad.data()) + sizeof(SnapHeader) + images * snap_params_stride());
            idx[3] = images;
            snap_seal(bad.data());
            verdict("index out of range", bad, bytes, 1, true);
            bad = good;
            reinterpret_cast<Params *>(reinterpret_cast<unsigned char *>(bad.data()) + sizeof(SnapHeader) + snap_params_stride())->flavor = 0;
            snap_seal(bad.data());
            verdict("foreign parameter object", bad, bytes, 1, true);
        }
        return 0;
    }
    fprintf(stderr, "usage: snapshot_driver layout | head COUNT IMAGES | write FLAVOR FMA COUNT IMAGES FILE | validate\n");
    return 2;
}
