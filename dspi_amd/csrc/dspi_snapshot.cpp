// dspi_snapshot.cpp — sizes, header construction and validation of the stream snapshot format (dspi_snapshot.h).  Pure host code.
#include "dspi_snapshot.h"

#include <string.h>

#include <vector>

#include "dspi_params.h"

namespace dspi {

size_t snap_params_bytes() { return sizeof(Params); }
size_t snap_params_stride() { return (sizeof(Params) + 7u) & ~(size_t)7u; }

// the polynomial of the preset slots' CRC (flash_storage.c:282-291, dspi_params.cpp crc32_edb88320), byte-wise through a table: a head
// may carry tens of thousands of parameter objects
uint32_t snap_crc32(const void *data, size_t n, uint32_t crc) {
    struct Table {
        uint32_t t[256];
        Table() {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
                t[i] = c;
            }
        }
    };
    static const Table tab;      // (initialised once, thread-safely: contexts on different threads may export at the same time)
    const uint32_t *table = tab.t;
    const unsigned char *d = static_cast<const unsigned char *>(data);
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ d[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

// Everything the two sides of a hand-over must agree on beyond the header's own fields: the parameter object's size and the numbers the
// record layout is derived from.  (A library whose Params changed meaning without changing size must raise kSnapVersion.)
uint32_t snap_fingerprint(int flavor) {
    const StateMap m = make_state_map(flavor);
    const SnapLayout l = make_snap_layout(flavor);
    const uint32_t w[] = {(uint32_t)sizeof(Params), (uint32_t)sizeof(StateOps), (uint32_t)m.n_slots, (uint32_t)m.n_out, (uint32_t)m.max_delay, (uint32_t)m.row,
                          (uint32_t)kRingLen, (uint32_t)kPdmWords, (uint32_t)m.lds_slots, (uint32_t)m.widx, (uint32_t)m.clip, l.record_words};
    return snap_crc32(w, sizeof w);
}

size_t snap_head_bytes(uint32_t count, uint32_t n_images) { return sizeof(SnapHeader) + (size_t)n_images * snap_params_stride() + (size_t)count * 4u; }
size_t snap_state_bytes(int flavor, uint32_t count) { return (size_t)count * make_snap_layout(flavor).record_words * 4u; }

SnapHeader snap_make_header(int flavor, bool fma, uint32_t count, uint32_t n_images, bool audio_started) {
    SnapHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kSnapMagic; h.version = kSnapVersion;
    h.flavor = (uint32_t)flavor; h.contract = fma ? 1u : 0u;
    h.record_words = make_snap_layout(flavor).record_words;
    h.count = count; h.n_images = n_images;
    h.fingerprint = snap_fingerprint(flavor);
    h.params_bytes = (uint32_t)sizeof(Params);
    h.flags = audio_started ? kSnapAudioStarted : 0u;
    h.head_bytes = snap_head_bytes(count, n_images);
    return h;
}

static uint32_t head_crc(const void *head, size_t n) {
    SnapHeader h;
    memcpy(&h, head, sizeof h);
    h.crc = 0;
    return snap_crc32(static_cast<const unsigned char *>(head) + sizeof h, n - sizeof h, snap_crc32(&h, sizeof h));
}

void snap_seal(void *head) {
    SnapHeader h;
    memcpy(&h, head, sizeof h);
    h.crc = head_crc(head, (size_t)h.head_bytes);
    memcpy(head, &h, sizeof h);
}

const unsigned char *snap_params(const void *head, uint32_t image) {
    return static_cast<const unsigned char *>(head) + sizeof(SnapHeader) + (size_t)image * snap_params_stride();
}

const char *snap_validate_head(const void *head, size_t head_bytes, int flavor, bool fma) {
    if (!head || head_bytes < sizeof(SnapHeader)) return "snapshot head: shorter than its header";
    SnapHeader h;
    memcpy(&h, head, sizeof h);
    if (h.magic != kSnapMagic) return "snapshot head: wrong magic";
    if (h.version != kSnapVersion) return "snapshot head: unknown format version";
    if (h.flavor != (uint32_t)flavor) return "snapshot head: the streams are of the other flavour";
    if (h.contract != (fma ? 1u : 0u)) return "snapshot head: the streams are of the other float contract";
    if (h.fingerprint != snap_fingerprint(flavor) || h.params_bytes != (uint32_t)sizeof(Params)) return "snapshot head: internal layout fingerprint differs (another build of the library)";
    if (h.record_words != make_snap_layout(flavor).record_words) return "snapshot head: record size differs";
    if (h.count == 0) return "snapshot head: no streams";
    if (h.n_images == 0 || h.n_images > h.count) return "snapshot head: image count out of range";
    if (h.head_bytes != snap_head_bytes(h.count, h.n_images)) return "snapshot head: sizes do not add up";
    if (head_bytes < h.head_bytes) return "snapshot head: truncated";
    if (h.crc != head_crc(head, (size_t)h.head_bytes)) return "snapshot head: CRC mismatch";
    const unsigned char *idx = snap_params(head, h.n_images);
    for (uint32_t i = 0; i < h.count; i++) {
        uint32_t k;
        memcpy(&k, idx + (size_t)i * 4, 4);
        if (k >= h.n_images) return "snapshot head: image index out of range";
    }
    std::vector<uint64_t> buf(snap_params_stride() / 8);      // (the caller's head need not be aligned for a Params)
    for (uint32_t i = 0; i < h.n_images; i++) {      // a parameter object of this flavour and contract (the fields dspi_create fixes)
        memcpy(buf.data(), snap_params(head, i), sizeof(Params));
        const Params *p = reinterpret_cast<const Params *>(buf.data());
        if (p->flavor != flavor || p->fma_contract != (fma && flavor != 0)) return "snapshot head: a parameter object of another flavour or contract";
    }
    return nullptr;
}

}  // namespace dspi
