// dspi_spdifrx.h — S/PDIF input (include/dspi.h: dspi_spdif_decode, dspi_process_sources): the subframe as the firmware's encoder writes it
// (pico_audio_spdif_multi: sample_encoding.h:27-47, audio_spdif.c:77-94, :101-113, :141-153) read back, the receiver record, the input layout
// of a call whose streams each name their source, and the receiver for one line on the CPU.  Plain C++ (no HIP): dspi_capi.cpp includes it,
// tests/spdifrx_driver.cpp exercises it without a GPU.  The kernel is dspi_spdifrx.hip; spdifrx_line_cpu below is the same rule, frame by
// frame (the direct path's decoder, and the model the kernel is held to).
//
// A frame is four words {l, h} left, {l, h} right.  With cells = h:l (64 bits) time slot k owns bit 2k (the clock cell, 1 for k >= 4) and bit
// 2k + 1 (the data cell).  l & 0xff is the preamble: Z 0x39 (left, block start), X 0xC9 (left), Y 0x69 (right).  Data cells: slots 4..27 the
// sample (slot 4 = LSB), 28 V, 29 U, 30 C, 31 P; parity holds when the XOR of the data cells of slots 4..31 is 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dspi {

// the record of include/dspi.h (dspi_spdif_rx), word for word: dspi_capi.cpp asserts the two agree
struct SpdifRx {
    uint32_t state;                 // 0 NO_SIGNAL, 1 ACQUIRING, 2 LOCKED: written at the end of every call
    uint32_t sample_rate;           // Hz from channel status byte 3, or 0
    uint32_t parity_err_count;      // since the last lock
    uint8_t c_bits[5], pad_[3];
    int32_t hold[2];                // last good sample, left / right
    uint32_t sync;                  // 0: not locked; 1 + p: the next frame is expected at block position p (0..191)
    uint32_t held;                  // subframes concealed
    uint32_t coding_errors;         // subframes that were not well-formed
};
static_assert(sizeof(SpdifRx) == 40, "the record is 40 bytes");
constexpr uint32_t kRxWords = 10;            // ... ten words: state rate parity c_bits[0..3] c_bits[4]+pad hold[0] hold[1] sync held coding_errors
constexpr uint32_t kRxBlock = 192;           // frames of a channel status block
constexpr uint32_t kRxStatusBits = 40;       // channel status bits kept (bytes 0-4)
constexpr uint32_t kRxFrameBytes = 16;

constexpr uint32_t kPreZ = 0x39, kPreX = 0xC9, kPreY = 0x69;
constexpr uint32_t kClockLo = 0x55555500u, kClockHi = 0x55555555u;

// ---- one subframe (constexpr: the kernel calls the same functions) ----
constexpr bool rx_clocks_ok(uint32_t l, uint32_t h) { return (l & kClockLo) == kClockLo && (h & kClockHi) == kClockHi; }
constexpr bool rx_left_ok(uint32_t l, uint32_t h) { return ((l & 0xffu) == kPreZ || (l & 0xffu) == kPreX) && rx_clocks_ok(l, h); }
constexpr bool rx_right_ok(uint32_t l, uint32_t h) { return (l & 0xffu) == kPreY && rx_clocks_ok(l, h); }
// the 16 odd bits of w, bit 2k + 1 to bit k
constexpr uint32_t rx_odd_bits(uint32_t w) {
    uint32_t x = (w >> 1) & 0x55555555u;
    x = (x | x >> 1) & 0x33333333u;
    x = (x | x >> 2) & 0x0f0f0f0fu;
    x = (x | x >> 4) & 0x00ff00ffu;
    return (x | x >> 8) & 0xffffu;
}
// the data cells of slots 0..31, slot k at bit k (slots 0..3 are the preamble's and mean nothing)
constexpr uint32_t rx_data(uint32_t l, uint32_t h) { return rx_odd_bits(h) << 16 | rx_odd_bits(l); }
constexpr int32_t rx_sample(uint32_t data) { return (int32_t)(data << 4) >> 8; }      // slots 4..27, sign-extended from bit 23
constexpr bool rx_v(uint32_t data) { return data >> 28 & 1u; }
constexpr bool rx_c(uint32_t data) { return data >> 30 & 1u; }
constexpr bool rx_parity_fails(uint32_t data) { return __builtin_popcount(data >> 4) & 1; }
// Hz for channel status byte 3, or 0
constexpr uint32_t rx_rate(uint32_t byte3) {
    return byte3 == 0x00 ? 44100u : byte3 == 0x02 ? 48000u : byte3 == 0x08 ? 88200u : byte3 == 0x0A ? 96000u : byte3 == 0x0C ? 176400u : byte3 == 0x0E ? 192000u : 0u;
}

// ---- one frame by the rule itself, steps 1-3 of include/dspi.h, on the record as registers hold it (constexpr: spdifrx_line_cpu runs it frame
// after frame, and so does every lane of dspi_linkrx.hip's tiled kernel: one text for the sequential rule) ----
struct RxRegs {
    uint32_t sync, rate, parity, held, coding;      // the record's sync (<= 192), sample_rate, parity_err_count, held, coding_errors
    uint64_t cbits;                                 // c_bits[0..4] in bits 0..39; above them the record's padding, kept
    int32_t hold_l, hold_r;
    bool any_ok;                                    // a well-formed subframe since the call began: what `state` is written from
};
constexpr void rx_lose(RxRegs &r) { r.sync = 0; r.rate = 0; }
constexpr int32_t rx_side(RxRegs &r, bool ok, uint32_t data, int32_t &hold) {
    // (sums and selects, no branch: the counters stay in registers on the device)
    const bool good = ok && !rx_v(data);
    r.coding += ok ? 0u : 1u;
    r.parity += ok && rx_parity_fails(data) ? 1u : 0u;      // counted only: the sample passes
    r.held += good ? 0u : 1u;
    hold = good ? rx_sample(data) : hold;
    return hold;
}
constexpr void rx_frame(RxRegs &r, uint32_t l0, uint32_t h0, uint32_t l1, uint32_t h1, int32_t &out_l, int32_t &out_r) {
    const bool ok_l = rx_left_ok(l0, h0), ok_r = rx_right_ok(l1, h1);
    const uint32_t data_l = rx_data(l0, h0), data_r = rx_data(l1, h1);
    r.any_ok = r.any_ok || ok_l || ok_r;
    // 1. sync
    if (ok_l && (l0 & 0xffu) == kPreZ) {
        if (r.sync != 1) r.parity = 0;      // a lock or a re-lock
        r.sync = 1;
    } else if (!ok_l || r.sync == 1) rx_lose(r);      // malformed, or X where Z is expected
    if (!ok_r) rx_lose(r);
    // 2. each side
    out_l = rx_side(r, ok_l, data_l, r.hold_l);
    out_r = rx_side(r, ok_r, data_r, r.hold_r);
    // 3. the channel status
    if (r.sync) {
        const uint32_t p = r.sync - 1;
        if (p < kRxStatusBits) r.cbits = (r.cbits & ~(1ull << p)) | (uint64_t)rx_c(data_l) << p;
        if (p == 31) r.rate = rx_rate((uint32_t)(r.cbits >> 24) & 0xffu);
        r.sync = 1 + (p + 1) % kRxBlock;
    }
}

// ---- the sync machine over up to 64 consecutive frames given as bit masks, bit i = frame i (the kernel's ballots; constexpr: the kernel
// and tests/spdifrx_driver.cpp run this one text).  Only three kinds of frame change the machine by more than a step: a left Z, a malformed
// subframe, and a left X where the position is 0; between two of them the position advances by one per frame.  So the walk goes from event
// to event: a run of ordinary frames is one shift-and-mask of the C mask into the channel status word.  X at position 0 can only happen
// where the run that enters a stretch wraps: one candidate frame per run.
struct RxWalk {
    uint32_t sync, rate;      // the record's, in and out
    uint64_t cbits;           // bits 0..39: the channel status, in and out (higher bits are kept)
    int lock_lane;            // out: the last frame that locked or re-locked (the parity count restarts WITH that frame), or -1
};
constexpr uint64_t rx_low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
// n: frames (1..64); bad_l / bad_r: the side is not well-formed; z: left well-formed with Z; c: the left subframe's C.  No bit at or above n.
constexpr void rx_walk(RxWalk &w, uint32_t n, uint64_t bad_l, uint64_t bad_r, uint64_t z, uint64_t c) {
    const uint64_t bad = bad_l | bad_r, stops = bad | z;
    w.lock_lane = -1;
    uint32_t at = 0;
    while (at < n) {
        uint32_t ev = n;      // the next frame that is handled singly
        if (w.sync == 0) {      // not locked: only a Z changes that; malformed frames in between clear the rate again
            const uint64_t zs = z & ~rx_low_bits(at);
            if (zs) ev = (uint32_t)__builtin_ctzll(zs);
            if (bad & ~rx_low_bits(at) & rx_low_bits(ev)) w.rate = 0;
        } else {                // locked at position p: ordinary frames up to the next Z, malformed frame, or the frame where the position is 0 again
            const uint32_t p = w.sync - 1;
            const uint64_t st = stops & ~rx_low_bits(at);
            const uint32_t stop = st ? (uint32_t)__builtin_ctzll(st) : n, wrap = at + (kRxBlock - p) % kRxBlock;
            ev = stop < wrap ? stop : wrap;
            if (ev > n) ev = n;
            const uint32_t len = ev - at;      // positions p .. p + len - 1, none past 191
            if (len) {
                if (p < kRxStatusBits) {
                    const uint32_t cnt = len < kRxStatusBits - p ? len : kRxStatusBits - p;
                    w.cbits = (w.cbits & ~(rx_low_bits(cnt) << p)) | ((c >> at & rx_low_bits(cnt)) << p);
                    if (p <= 31u && p + cnt > 31u) w.rate = rx_rate((uint32_t)(w.cbits >> 24) & 0xffu);
                }
                w.sync = 1u + (p + len) % kRxBlock;
            }
        }
        if (ev >= n) break;
        // the frame at ev, by the rule itself
        if (z >> ev & 1u) {
            if (w.sync != 1u) w.lock_lane = (int)ev;
            w.sync = 1u;
        } else if ((bad_l >> ev & 1u) || w.sync == 1u) { w.sync = 0; w.rate = 0; }
        if (bad_r >> ev & 1u) { w.sync = 0; w.rate = 0; }
        if (w.sync) {
            const uint32_t p = w.sync - 1;
            if (p < kRxStatusBits) w.cbits = (w.cbits & ~(1ull << p)) | (c >> ev & 1ull) << p;
            if (p == 31u) w.rate = rx_rate((uint32_t)(w.cbits >> 24) & 0xffu);
            w.sync = 1u + (p + 1u) % kRxBlock;
        }
        at = ev + 1u;
    }
}

// ---- the receiver for one line ----
// `frames` frames of four words at `words` (any alignment) through the record *rx, which is read and updated as include/dspi.h says
// (rx->sync <= 192).  Output, either or both: pairs = int32 [frames][2]; packed = 6 bytes per frame, the two samples as 24-bit little endian
// (what the chain reads at bit depth 24).
void spdifrx_line_cpu(SpdifRx *rx, const void *words, uint64_t frames, int32_t *pairs, uint8_t *packed);

// ---- the input layout of dspi_process_sources: dspi_intake.h's with a third kind of run ----
constexpr uint8_t kSrcSpdif = 1;      // DSPI_SRC_SPDIF; 16 and 24 are the PCM depths (DSPI_SRC_PCM16 / 24)
constexpr uint32_t source_frame_bytes(uint8_t src) { return src == 24 ? 6u : src == 16 ? 4u : src == kSrcSpdif ? kRxFrameBytes : 0u; }
// every entry a source?  Returns n when so, else the index of the first entry that is none.
uint32_t sources_check(const uint8_t *sources, uint32_t n);
bool sources_any_spdif(const uint8_t *sources, uint32_t n);
// offsets[s] = where stream s's run starts: behind its predecessor's, an S/PDIF run at the next multiple of 16; offsets[n] = the total.
// n + 1 values (offsets == nullptr: none written).  The sources are valid.  False when the size does not fit in 64 bits; nothing is written
// then.  Without an S/PDIF entry these are intake_offsets' values.
bool sources_offsets(const uint8_t *sources, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets);

}  // namespace dspi
