// dspi_snapshot.h — the hand-over format of dspi_export_streams / dspi_import_streams (include/dspi.h): what a snapshot's head holds,
// how one stream's run-time record is laid out, how both are sized, built and validated.  Plain C++ (no HIP): dspi_capi.cpp and
// dspi_snapshot.hip include it, tests/snapshot_driver.cpp exercises it without a GPU.
//
//   head   (host memory)   SnapHeader | n_images parameter objects (Params, as bytes, each padded to 8) | count x uint32 image index
//   state  (host / device) count records of record_words(flavor) 32-bit words, stream-major: record i is stream first + i
//
// One record is the stream's column of the context's four stream-minor arrays ([W][position][R]), section after
// section in the arrays' own position order; every section starts on a 16-byte boundary (its span is its length rounded up to four
// words, the pad words are zero), so that both sides of the transposition kernels move 16 bytes per lane:
//   SEC_STATE   StateMap::n_slots words            every state slot (filters, crossfeed, leveller, ring position, delay write index,
//                                                  mute envelope, last peaks, the four clip slots)
//   SEC_LINES   n_out * max_delay words            every delay line at full length, [output][position]
//   SEC_RING    2 * kRingLen words                 the leveller's two rings, [channel][position]
//   SEC_PDM     kPdmStateWords words               the PDM modulator (power-on values when the source never ran it)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "dspi_image.h"

namespace dspi {

constexpr int kPdmWords = 9;            // == kPdmStateWords (dspi_kernels.h; static_assert in dspi_snapshot.hip)
constexpr uint32_t kSnapMagic = 0x53505344u;      // "DSPS"
constexpr uint32_t kSnapVersion = 1;

enum SnapSection : int { SEC_STATE = 0, SEC_LINES, SEC_RING, SEC_PDM, SEC_COUNT };

struct SnapSectionInfo {
    uint32_t offset;      // first word of the section inside a record
    uint32_t len;         // words that carry state = positions per row of the section's device array
    uint32_t span;        // len rounded up to 4: the words the section occupies
};
struct SnapLayout {
    SnapSectionInfo sec[SEC_COUNT];
    uint32_t record_words;
    uint32_t row;         // StateMap::row
};

constexpr uint32_t snap_round4(uint32_t n) { return (n + 3u) & ~3u; }
constexpr SnapLayout make_snap_layout(int flavor) {
    const StateMap m = make_state_map(flavor);
    SnapLayout l{};
    const uint32_t lens[SEC_COUNT] = {(uint32_t)m.n_slots, (uint32_t)m.n_out * (uint32_t)m.max_delay, 2u * (uint32_t)kRingLen, (uint32_t)kPdmWords};
    uint32_t at = 0;
    for (int s = 0; s < SEC_COUNT; s++) {
        l.sec[s].offset = at; l.sec[s].len = lens[s]; l.sec[s].span = snap_round4(lens[s]);
        at += l.sec[s].span;
    }
    l.record_words = at;
    l.row = (uint32_t)m.row;
    return l;
}

// ---- realignment (DSPI_SNAP_REALIGN, dspi_realign_streams) ----
// A delay line and a leveller ring are circular and addressed only relative to the stream's one position slot (StateMap::widx,
// StateMap::ring_pos): a stream whose lines are rotated by d and whose position is advanced by d is the same stream.  A realigning
// write gives every stream it writes the positions of its destination row, so that the row's streams share one position again.
//
// The target rule: whose (widx, ring_pos) the streams written into row `row` take, for a call that writes streams [first, first +
// count) of a context of n_streams: the lowest-numbered stream of the row that is below n_streams and OUTSIDE the range — a resident
// neighbour, its positions read from the context's state array —, or, where the row has none, the first stream of the range that
// lands in the row, its positions read from its record.  (A range of whole rows therefore moves its rows' first streams by 0.)
struct SnapTarget {
    uint32_t stream;      // of the destination context
    bool resident;        // outside the range: read the state array; else read record `stream - first`
};
constexpr SnapTarget snap_row_target(uint32_t row, uint32_t row_streams, uint32_t n_streams, uint32_t first, uint32_t count) {
    const uint64_t r0 = (uint64_t)row * row_streams, r1 = r0 + row_streams < n_streams ? r0 + row_streams : n_streams, end = (uint64_t)first + count;
    if (r0 < first) return SnapTarget{(uint32_t)r0, true};            // the row begins below the range
    if (end < r1) return SnapTarget{(uint32_t)end, true};             // the range ends inside the row
    return SnapTarget{(uint32_t)r0, false};                           // the range covers what the context has of the row
}
// ... for dspi_resume_streams (include/dspi.h), which realigns in place the streams of [first, first + count) that were paused: `active` is
// the context's activity bitmap BEFORE the call (bit s % 32 of word s / 32: stream s takes part in dspi_process).  The row's target is its
// lowest-numbered stream below n_streams that is active — in the range or not: a stream of the range that was active is a resident and is
// not moved —, its positions read from the state array; a row without one takes the first stream of the range that lies in it (every
// stream of the range there is then one this call resumes), from its record.  With every stream outside the range active and every
// stream inside paused this is snap_row_target.
constexpr bool snap_stream_active(const uint32_t *active, uint64_t s) { return (active[s >> 5] >> (s & 31u)) & 1u; }
constexpr SnapTarget snap_row_target_active(uint32_t row, uint32_t row_streams, uint32_t n_streams, uint32_t first, uint32_t count, const uint32_t *active) {
    const uint64_t r0 = (uint64_t)row * row_streams, r1 = r0 + row_streams < n_streams ? r0 + row_streams : n_streams;
    for (uint64_t s = r0; s < r1; s++) if (snap_stream_active(active, s)) return SnapTarget{(uint32_t)s, true};
    const uint64_t lo = r0 > first ? r0 : first, end = (uint64_t)first + count, hi = end < r1 ? end : r1;
    for (uint64_t s = lo; s < hi; s++) if (!snap_stream_active(active, s)) return SnapTarget{(uint32_t)s, false};
    return SnapTarget{(uint32_t)lo, false};      // (the call resumes nobody in this row: never read)
}
// how far a stream at position `from` is rotated to stand at `to` (both masked; len a power of two); snap_shift_pair: both positions at once
constexpr uint32_t snap_shift(uint32_t from, uint32_t to, uint32_t len) { return (to - from) & (len - 1u); }
// A stream's masked (delay write index, ring position) pair, read at `p`, the stream's first state word, with the slots `stride` words
// apart: a column of the [W][slot][R] state array (snap_positions: stream s of the context, stride StateMap::row) or the state section of
// a record (stride 1).
struct SnapPos { uint32_t widx, ring_pos; };
constexpr SnapPos snap_positions_at(const StateMap &sm, const uint32_t *p, size_t stride) {
    return SnapPos{p[(size_t)sm.widx * stride] & ((uint32_t)sm.max_delay - 1u), p[(size_t)sm.ring_pos * stride] & ((uint32_t)kRingLen - 1u)};
}
constexpr SnapPos snap_positions(const StateMap &sm, const uint32_t *state, uint64_t s) {
    return snap_positions_at(sm, state + (size_t)(s / (uint32_t)sm.row) * sm.n_slots * sm.row + s % (uint32_t)sm.row, (size_t)sm.row);
}
constexpr SnapPos snap_shift_pair(const StateMap &sm, SnapPos from, SnapPos to) {
    return SnapPos{snap_shift(from.widx, to.widx, (uint32_t)sm.max_delay), snap_shift(from.ring_pos, to.ring_pos, (uint32_t)kRingLen)};
}
// the record position whose word lands at position p of a line or ring of `len` words rotated by d: line[(q + d) mod len] = record[q]
constexpr uint32_t snap_rot_source(uint32_t p, uint32_t d, uint32_t len) { return (p - d) & (len - 1u); }

// 64 bytes, little-endian like everything else the library exchanges
struct SnapHeader {
    uint32_t magic, version;
    uint32_t flavor;            // DSPI_FLAVOR_*
    uint32_t contract;          // 1: DSPI_FLOAT_CONTRACT_FMA
    uint32_t record_words;      // of one stream's record in `state`
    uint32_t count;             // streams
    uint32_t n_images;          // parameter objects that follow the header
    uint32_t fingerprint;       // snap_fingerprint(flavor): the internal layout both sides must share
    uint32_t params_bytes;      // sizeof(Params)
    uint32_t flags;             // kSnapAudioStarted
    uint64_t head_bytes;        // of the whole head
    uint32_t reserved[3];
    uint32_t crc;               // CRC-32 (the preset slots' polynomial) of the head with this field zero
};
static_assert(sizeof(SnapHeader) == 64, "SnapHeader is 64 bytes");
constexpr uint32_t kSnapAudioStarted = 1u;

size_t snap_params_bytes();                       // sizeof(Params)
size_t snap_params_stride();                      // ... padded to 8
uint32_t snap_fingerprint(int flavor);
uint32_t snap_crc32(const void *data, size_t n, uint32_t crc = 0);      // chainable: pass the previous result
size_t snap_head_bytes(uint32_t count, uint32_t n_images);
size_t snap_state_bytes(int flavor, uint32_t count);
// fills everything but the CRC; snap_seal computes it over the finished head
SnapHeader snap_make_header(int flavor, bool fma, uint32_t count, uint32_t n_images, bool audio_started);
void snap_seal(void *head);
const unsigned char *snap_params(const void *head, uint32_t image);      // object `image`; image = n_images: the stream index (uint32 per stream)

// nullptr = well formed for a context of (flavor, fma); else which check refused it.  Reads at most head_bytes bytes.
const char *snap_validate_head(const void *head, size_t head_bytes, int flavor, bool fma);

}  // namespace dspi
