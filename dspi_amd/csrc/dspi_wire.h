// dspi_wire.h — the wire layout of dspi_process_wire / dspi_wire_encode (include/dspi.h): every pair in the words of the driver its slot
// belongs to, S/PDIF subframes or I2S slot words, by the stream's OWN output types.  Plain C++ (no HIP): dspi_capi.cpp includes it,
// tests/wire_driver.cpp exercises it without a GPU.  The kernel that writes the layout is dspi_wire.hip.
//
// The layout has the size and the regions of DSPI_OUT_SPDIF: pair p of stream s owns 16 F bytes at ((s * P + p) * F) * 16.
//   S/PDIF slot   uint32 [F][4], the subframes, the whole region
//   I2S slot      uint32 [F][2], word << 8, L then R, in the FIRST 8 F bytes; the last 8 F bytes (the tail) are never written in a caller's
//                 device buffer and come back as zeros in host buffers
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dspi.h"

namespace dspi {

// ---- the flag rule: what the two calls accept; everything else (DSPI_OUT_SPDIF, which is implied, DSPI_OUT_I2S_SLOTS, DSPI_OUT_TILED, every
// undefined bit) is refused before anything else is looked at
constexpr uint32_t kWireProcessFlags = DSPI_MEM_DEVICE | DSPI_OUT_ENABLED_ONLY | DSPI_OUT_CLIP_FLAGS;
constexpr uint32_t kWireEncodeFlags = DSPI_MEM_DEVICE;
constexpr bool wire_process_flags_ok(uint32_t flags) { return (flags & ~kWireProcessFlags) == 0; }
constexpr bool wire_encode_flags_ok(uint32_t flags) { return (flags & ~kWireEncodeFlags) == 0; }

// ---- the region arithmetic, in bytes from the start of the buffer
struct WireRegion {
    uint64_t offset;                  // of the region
    uint64_t written;                 // bytes from `offset` on that hold the pair's words: 16 F (S/PDIF) or 8 F (I2S)
    uint64_t tail_begin, tail_end;    // the bytes of the region behind them: empty (both = offset + 16 F) for an S/PDIF slot
};
constexpr uint64_t wire_region_bytes(uint64_t n_frames) { return 16 * n_frames; }
constexpr WireRegion wire_region(uint64_t stream, uint64_t pair, uint64_t n_pairs, uint64_t n_frames, bool i2s) {
    return WireRegion{(stream * n_pairs + pair) * wire_region_bytes(n_frames), (i2s ? 8u : 16u) * n_frames,
                      (stream * n_pairs + pair) * wire_region_bytes(n_frames) + (i2s ? 8u : 16u) * n_frames,
                      (stream * n_pairs + pair + 1) * wire_region_bytes(n_frames)};
}

// ---- the TILED wire layout of dspi_process_devices (with DSPI_OUT_TILED) / dspi_wire_encode_tiled: the regions of dspi_spdif_encode_v's
// tiled subframes.  R = streams per tile, tile t = stream / R, column c = stream % R.  Pair p of tile t owns 16 F R bytes, 4 F rows of R
// words, at word offset ((t * P + p) * F) * 4 * R; column c of every row belongs to one stream, whose type decides what stands there:
//   S/PDIF slot   row f * 4 + j: subframe word j of frame f — uint32 [F][4][R], the tiled subframes
//   I2S slot      row side * F + f, side 0 = L: word << 8 — uint32 [2][F][R] in the FIRST half of the region, what dspi_i2s_encode writes
//                 with DSPI_OUT_TILED for outputs 2p and 2p + 1; rows 2 F .. 4 F - 1 of the column (the tail) are never written in a
//                 caller's device buffer and come back as zeros in host buffers, like a paused stream's column and the columns past the
//                 context's last stream
// The flag rules of the two calls: everything else is refused before anything else is looked at, as above.
constexpr uint32_t kDevicesProcessFlags = DSPI_MEM_DEVICE | DSPI_OUT_TILED | DSPI_OUT_ENABLED_ONLY | DSPI_OUT_CLIP_FLAGS;
constexpr uint32_t kWireEncodeTiledFlags = DSPI_MEM_DEVICE;
constexpr bool devices_process_flags_ok(uint32_t flags) { return (flags & ~kDevicesProcessFlags) == 0; }
constexpr bool wire_encode_tiled_flags_ok(uint32_t flags) { return (flags & ~kWireEncodeTiledFlags) == 0; }
// the arithmetic, in WORDS from the start of the buffer
constexpr uint64_t wire_tiled_region_words(uint64_t n_frames, uint64_t row) { return 4 * n_frames * row; }
constexpr uint64_t wire_tiled_region(uint64_t tile, uint64_t pair, uint64_t n_pairs, uint64_t n_frames, uint64_t row) {
    return (tile * n_pairs + pair) * wire_tiled_region_words(n_frames, row);
}
constexpr uint64_t wire_tiled_spdif_word(uint64_t region, uint64_t row, uint64_t col, uint64_t frame, uint64_t j) {
    return region + (frame * 4 + j) * row + col;
}
constexpr uint64_t wire_tiled_i2s_word(uint64_t region, uint64_t n_frames, uint64_t row, uint64_t col, uint64_t side, uint64_t frame) {
    return region + (side * n_frames + frame) * row + col;
}
// one stream's column of a region: its words stand at first + k * row, k < written; the tail at tail_first + k * row, k < tail
struct WireTiledColumn { uint64_t first, written, tail_first, tail; };
constexpr WireTiledColumn wire_tiled_column(uint64_t stream, uint64_t pair, uint64_t n_pairs, uint64_t n_frames, uint64_t row, bool i2s) {
    return WireTiledColumn{wire_tiled_region(stream / row, pair, n_pairs, n_frames, row) + stream % row, (i2s ? 2u : 4u) * n_frames,
                           wire_tiled_region(stream / row, pair, n_pairs, n_frames, row) + stream % row + (i2s ? 2u : 4u) * n_frames * row,
                           (i2s ? 2u : 0u) * n_frames};
}

// ---- the types: bit p of a parameter object's mask = its slot p is an I2S slot (output_types[p] == 1, config.h:286-287) — DevImage::i2s_pairs
inline uint32_t wire_i2s_mask(const uint8_t *output_types, uint32_t n_pairs) {
    uint32_t m = 0;
    for (uint32_t p = 0; p < n_pairs; p++) if (output_types[p] == 1) m |= 1u << p;
    return m;
}
// does any ACTIVE stream's parameter object carry an I2S slot?  stream_image [n_streams]: the object of every stream; active: the context's
// record (one byte per stream, 1 = active; nullptr = every stream is); image_i2s [object]: wire_i2s_mask of each.
// false: dspi_process_wire IS dspi_process with DSPI_OUT_SPDIF, route and bytes; true: two passes with the wire encoder.
bool wire_any_i2s(const int32_t *stream_image, uint32_t n_streams, const uint8_t *active, const uint32_t *image_i2s);

}  // namespace dspi
