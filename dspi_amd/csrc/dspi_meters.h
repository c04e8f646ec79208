// dspi_meters.h — the meter bridge (include/dspi.h "the meter bridge"): meter ballistics, alarms and status blocks for a whole context.
//
// The chain kernels leave two things per stream: the block peaks of every packet (dspi_out.peaks, uint16 [stream][block][C]; the last
// packet's also in the state slots REQ_GET_STATUS reads) and the sticky clip bits (four state slots, OR'd).  The reference's metering
// spec leaves ballistics to the host application; this module is that host's arithmetic for n devices at once.  Plain C++, no HIP: the
// argument rules, the CPU paths and the status block's layout; dspi_meterbridge.hip holds the kernels that compute the same words.
//
// METER WORD   uint32 = level | count << 16: the displayed level (a block peak's scale, 0..65535) and the packets its hold has left.
// UPDATE       per packet, with p the packet's peak:   p >= level: level = p, count = hold
//                                                      else count > 0: count--
//                                                      else level = max(p, (level * decay) >> 15)
//              Integer throughout, so a word is defined bit for bit and a call over K packets equals calls over any split of them.
// ALARM        a stream whose clip bits are non-zero, or (meters given) that has a channel with level >= the threshold;
//              info = mask of those channels | clip bits << 16.  Lists are ascending.
// STATUS BLOCK REQ_GET_STATUS wValue 9: peaks[C] LE u16, two CPU-load bytes (0 here), clip bits LE u16: 2 C + 4 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dspi {

constexpr uint32_t kMeterMemDevice = 0x1u;      // DSPI_MEM_DEVICE, the one flag of these calls (dspi_capi.cpp asserts the two equal)
constexpr uint32_t kMeterMaxHold = 65535u, kMeterMaxDecay = 32768u, kMeterMaxLevel = 65535u;

constexpr uint32_t meter_level(uint32_t word) { return word & 0xffffu; }
constexpr uint32_t meter_count(uint32_t word) { return word >> 16; }
constexpr uint32_t meter_word(uint32_t level, uint32_t count) { return level | count << 16; }
// one packet (the rule above; 32-bit unsigned product: 65535 * 32768 < 2^31), on a meter's two halves.  constexpr, like alarm_info: the kernels
// compile the same text
constexpr void meter_step_lc(uint32_t &level, uint32_t &count, uint32_t p, uint32_t hold, uint32_t decay) {
    const bool up = p >= level, held = count > 0;      // (written as selections: the kernel's lanes take different branches at every packet)
    const uint32_t d = ((level & 0xffffu) * (decay & 0xffffu)) >> 15;      // (the masks change nothing — level <= 65535, decay <= 32768 —; they let the kernel multiply at full rate)
    level = up ? p : held ? level : p > d ? p : d;
    count = up ? hold : held ? count - 1u : 0u;
}
constexpr uint32_t meter_step(uint32_t word, uint32_t p, uint32_t hold, uint32_t decay) {
    uint32_t level = meter_level(word), count = meter_count(word);
    meter_step_lc(level, count, p, hold, decay);
    return meter_word(level, count);
}

constexpr size_t status_block_bytes(int n_ch) { return (size_t)n_ch * 2u + 4u; }

// ---- the argument rules: why a call is refused with DSPI_E_INVAL (nullptr: it is not).  n / n_ch: the context's streams and channels.
// What follows them in every call is DSPI_E_NODEVICE for kMeterMemDevice on a host-only context.
const char *meters_update_why(const void *peaks, uint32_t n_blocks, uint32_t hold_packets, uint32_t decay_q15, const void *meters, uint32_t flags, uint32_t n, int n_ch);
const char *meters_alarms_why(const void *meters, uint32_t level_q15, const void *streams, const void *info, uint32_t cap, const void *total, uint32_t flags);
// (cap is looked at after these: DSPI_E_SHORT)
const char *status_all_why(uint32_t first, uint32_t count, const void *buf, uint32_t flags, uint32_t n);
// the first entry >= n, or count when there is none
uint32_t clear_list_check(const uint32_t *streams, uint32_t count, uint32_t n);

// ---- the CPU paths
// peaks uint16 [n][n_blocks][n_ch], meters uint32 [n][n_ch]; active: one byte per stream or null = every stream.  A paused stream's words are
// neither read nor written, and neither is its region of peaks.
void meters_update_cpu(const uint16_t *peaks, uint32_t n, uint32_t n_blocks, int n_ch, uint32_t hold_packets, uint32_t decay_q15, uint32_t *meters, const uint8_t *active);
// the info word of one stream (0: not in alarm).  meters: the stream's n_ch words or null.
constexpr uint32_t alarm_info(const uint32_t *meters, int n_ch, uint32_t level_q15, uint32_t clip) {
    uint32_t mask = 0;
    if (meters)
        for (int c = 0; c < n_ch; c++) mask |= (uint32_t)(meter_level(meters[c]) >= level_q15) << c;
    return mask | clip << 16;
}
// meters uint32 [n][n_ch] or null, clip uint16 [n] or null (no bits anywhere).  The lowest min(total, cap) alarmed streams into streams (and
// their info words into info, when given), ascending; *total: how many there are.  Returns the number written.
uint32_t meters_alarms_cpu(const uint32_t *meters, const uint16_t *clip, uint32_t n, int n_ch, uint32_t level_q15, uint32_t *streams, uint32_t *info, uint32_t cap, uint32_t *total);
// one status block from a stream's peaks (n_ch of them) and clip bits into status_block_bytes(n_ch) bytes
void status_pack(const uint16_t *peaks, uint16_t clip, int n_ch, uint8_t *out);

// ---- how the update kernel (dspi_meterbridge.hip) brings a workgroup's peaks into LDS: the arithmetic only, constexpr, so that the kernel and
// the stand-alone driver (tests/meters_driver.cpp, which walks it on the CPU with every index checked) compile the same text.
// A workgroup of kMeterLanes lanes serves G = kMeterLanes / C consecutive streams from s0, g of them present; lane t holds word t of their
// g C contiguous meter words.  Their peaks are one contiguous span, K C 2 bytes per stream.  It is staged kMeterStagePackets packets at a time:
// K <= that: the whole span is ONE PIECE; above: one piece per stream and chunk.  A piece lies in LDS at the low four bits of its global
// address, so that every aligned 16-byte vector inside it goes over as it is.  Lanes share the pieces without a division: with one piece all
// kMeterLanes lanes stride over its vectors, else each wave of 64 takes every fourth piece (meter_piece_lanes).
constexpr uint32_t kMeterLanes = 256;
constexpr uint32_t kMeterStagePackets = 64;
struct MeterGeom {
    uint32_t G;                // streams per workgroup
    uint32_t piece_stride;     // LDS bytes between two pieces: a piece of kMeterStagePackets packets and up to 14 bytes in front of it, in whole vectors
    uint32_t lds_bytes;
};
constexpr MeterGeom meter_geom(int n_ch) {
    const uint32_t G = kMeterLanes / (uint32_t)n_ch, piece = kMeterStagePackets * (uint32_t)n_ch * 2u;
    const uint32_t stride = (piece + 14u + 15u) / 16u * 16u, span = (G * piece + 14u + 15u) / 16u * 16u;
    return MeterGeom{G, stride, span > G * stride ? span : G * stride};
}
struct MeterChunk {
    bool one;                  // the workgroup's streams are one piece
    uint32_t s0, n_pieces, piece_bytes;
    uint64_t stream_bytes, first;                  // first: byte offset of the chunk's first packet within a stream
};
constexpr MeterChunk meter_chunk(int n_ch, uint32_t s0, uint32_t g, uint32_t K, uint32_t k0) {
    const bool one = K <= kMeterStagePackets;
    const uint32_t kc = K - k0 < kMeterStagePackets ? K - k0 : kMeterStagePackets;
    const uint32_t bytes = (one ? g * K : kc) * (uint32_t)n_ch * 2u;
    return MeterChunk{one, s0, one ? 1u : g, bytes, (uint64_t)K * (uint64_t)n_ch * 2u, (uint64_t)k0 * (uint64_t)n_ch * 2u};
}
constexpr uint32_t meter_piece_lanes(const MeterChunk &c) { return c.one ? kMeterLanes : 64u; }      // lane t: piece t / this (+ kMeterLanes / this, ...), vectors t % this (+ this, ...)
struct MeterPiece {
    int64_t origin;            // byte offset from `peaks` of the piece's vector 0: the piece's first byte less `lead` (so it may be negative, for stream 0)
    uint32_t lead;             // bytes of vector 0 in front of the piece (0..14): the low four bits of the piece's global address
    uint32_t end;              // lead + the piece's bytes: the piece is [lead, end) of its vectors' bytes
    uint32_t dst;              // where its vector 0 goes in LDS
    uint32_t piece;
};
// base: the address of `peaks` (its low four bits are all that is used)
constexpr MeterPiece meter_piece(const MeterChunk &c, const MeterGeom &g, uint64_t base, uint32_t piece) {
    const uint64_t a0 = (uint64_t)(c.s0 + piece) * c.stream_bytes + c.first;
    const uint32_t lead = (uint32_t)((base + a0) & 15u);
    return MeterPiece{(int64_t)a0 - (int64_t)lead, lead, lead + c.piece_bytes, piece * g.piece_stride, piece};
}
// vector v of a piece covers [16 v, 16 v + 16) of its vectors' bytes: there is one while 16 v < end, and it lies inside the piece when ...
constexpr bool meter_vec_whole(const MeterPiece &p, uint32_t v) { return v * 16u >= p.lead && v * 16u + 16u <= p.end; }
// the stream that owns byte `rel` of the piece's vectors' bytes (lead <= rel < end)
constexpr uint32_t meter_stream_of(const MeterChunk &c, const MeterPiece &p, uint32_t rel) {
    return c.one ? c.s0 + (rel - p.lead) / (uint32_t)c.stream_bytes : c.s0 + p.piece;
}
// where the chunk's first packet of (local stream sl, channel ch) lies in LDS; its later packets follow at n_ch * 2 bytes each
constexpr uint32_t meter_walk_at(const MeterChunk &c, const MeterGeom &g, uint64_t base, uint32_t sl, uint32_t ch) {
    const uint64_t a0 = (uint64_t)(c.s0 + (c.one ? 0u : sl)) * c.stream_bytes + c.first;
    return (uint32_t)((base + a0) & 15u) + (c.one ? sl * (uint32_t)c.stream_bytes : sl * g.piece_stride) + ch * 2u;
}

}  // namespace dspi
