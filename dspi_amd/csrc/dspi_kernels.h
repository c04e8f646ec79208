// dspi_kernels.h — launch interface between the context (dspi_capi.cpp) and dspi_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>
#include "dspi_image.h"
#include "dspi_plan.h"

namespace dspi {

constexpr int kChunk = 16;   // frames per in-kernel chunk (divides the 48- and 96-frame packets)

struct KArgs {
    const DevImage *img;     // the context's image array; a workgroup uses img[item.image] (scalar loads: its lanes share it)
    const WgItem *items;     // workgroups of this launch: row, image, lane mask
    uint32_t *state;         // [n_wg][n_slots][64]
    uint32_t *dlines;        // [n_wg][n_out][max_delay][64]
    uint32_t *ring;          // [n_wg][kRingLen][2][64]
    const void *pcm;         // [stream][n_blocks*block_len] frames, 4 or 6 bytes each
    int32_t *pairs;          // [stream][pair][frames][2] or null
    int32_t *sub;            // [stream][frames] or null
    uint16_t *peaks;         // [stream][block][C] or null
    uint32_t n_streams, n_blocks, block_len, bit_depth;
    const uint32_t *stream_image;   // [n_streams] image index of every stream (float one-stream kernel: per-lane parameters)
    uint32_t tiled_out;      // DSPI_OUT_TILED: pairs = [tile][output][frames][row], sub = [tile][frames][row] (row = StateMap::row)
    uint32_t *xwords;        // packed float kernel, stream-major output: mini lines [n_wg][3][kMaxOut][kChunk][128] words — the rows of outputs that do not reach their pair's waves through the delay line (dspi_chain_pk.inc output_item_pk)
    const float *vals;       // packed float kernel, per-lane values: value tiles [n_wg][kPvTileFloats] (dspi_image.h) or null
    uint32_t pairs_stream0;  // stream-major `pairs` starts at this stream (0: the caller's whole buffer; the two-pass S/PDIF path hands the kernels a scratch buffer that
                             // holds a chunk of rows)
    uint32_t skip_silent;    // DSPI_OUT_ENABLED_ONLY: sample words of silent outputs (a disabled S/PDIF pair, the sub while it is off) need not be stored
    uint32_t i2s_slots;      // DSPI_OUT_I2S_SLOTS: pairs whose slot is an I2S slot (DevImage::i2s_pairs) carry left-justified I2S words (word << 8)
    uint32_t spdif;          // DSPI_OUT_SPDIF (latency layout only): `pairs` takes IEC 60958 subframes, uint32 [stream][pair][frame][4]
    uint32_t spdif_pos;      // position of the launch's first frame in the 192-frame block (the channel status follows each image's own fs_hz)
    uint32_t fma;            // float flavour: the context's contract is DSPI_FLOAT_CONTRACT_FMA (selects the kernel family at launch)
    uint32_t no_emit_lines;  // DSPI_NO_EMIT_LINES: the packed kernel's emitter wave keeps the row mapping everywhere (dspi_chain_pk.inc pair_lines_*)
};

size_t chain_lds_bytes(int flavor, int packed);
// the chain launch of one path of the launch plan (dspi_plan.h): args.items = its items (WgItem in dspi_image.h says what they mean)
hipError_t launch_chain(Path path, const KArgs &args, uint32_t n_items, hipStream_t stream);
hipError_t launch_state_ops(int flavor, const WgItem *items, uint32_t n_items, const StateOps &ops, uint32_t *state, uint32_t *dlines,
                            uint32_t *ring, uint32_t n_streams, hipStream_t stream);
// (re)build the value tiles of the listed rows from the images of their streams
// all_differ: development switch, every band is treated as different between the row's streams (the worst case, for timing)
// active: the context's activity bitmap or null = every stream: "which bands differ" is decided among the row's active streams
hipError_t launch_pv_build(const DevImage *img, const uint32_t *stream_image, const uint32_t *rows, uint32_t n_rows, float *vals, uint32_t n_streams, bool all_differ,
                           const uint32_t *active, hipStream_t stream);
hipError_t launch_state_init(int flavor, uint32_t *state, uint32_t n_wg, hipStream_t stream);
// debug: taps [kBands+1][n] after every band of EQ channel `ch` of *img (float flavour), other [kBands][n] = the other
// contract's one-step result from the same input and state
hipError_t launch_eq_taps(bool fma, const DevImage *img, int ch, const float *x, uint32_t n, float *taps, float *other, hipStream_t stream);

// ---- PDM sub output (dspi_pdm.hip): per-stream state [n_wg][kPdmStateWords][row]: err err2 x1 x2 y1 y2 err_acc rng fade_in_pos
constexpr int kPdmStateWords = 9;
constexpr int kPdmRngWord = 7;
// power-on word i of a modulator: zero except the dither RNG's seed (pdm_generator.c:63).  The one definition: the modulator's own
// initialiser (dspi_pdm.hip) and the power-on kernel (dspi_boot_streams, dspi_boot.hip) both write what it says.
constexpr uint32_t pdm_power_on_word(int i) { return i == kPdmRngWord ? 123456789u : 0u; }
// active: the context's activity bitmap (one bit per stream) or null = every stream; a paused stream's state and words are not touched
hipError_t launch_pdm(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, uint32_t n_streams, uint32_t n_frames, uint32_t row,
                      uint32_t n_wg, const uint32_t *active, hipStream_t stream);
// the same modulator over a work list in device memory (dspi_pdmlife.h: n_list words, ascending streams, bit 31 = start from the re-enable
// state): lane g serves list[g]; `sub` and `words` are the call's, addressed by absolute stream.  n_list == 0 launches nothing.
hipError_t launch_pdm_list(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, const uint32_t *list, uint32_t n_list, uint32_t n_streams,
                           uint32_t n_frames, uint32_t row, hipStream_t stream);
// ... in the fade mode (dspi_pdm_fade; dspi_pdmfade.h): `aux` holds one word per list entry (null: all zero), `base` the fade bases [stream]
hipError_t launch_pdm_list_fade(bool tiled, uint32_t *state, const int32_t *sub, uint32_t *words, const uint32_t *list, const uint32_t *aux, int32_t *base,
                                uint32_t n_list, uint32_t n_streams, uint32_t n_frames, uint32_t row, hipStream_t stream);
// the fade bases of the n listed slots into `packed`, and `packed` (null: zeros) into the n listed slots
hipError_t launch_pdm_base_gather(const int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, int32_t *packed, hipStream_t stream);
hipError_t launch_pdm_base_scatter(int32_t *base, const uint32_t *slots, uint32_t n, uint32_t n_streams, const int32_t *packed, hipStream_t stream);
hipError_t launch_pdm_reset(uint32_t *state, uint32_t n_streams, uint32_t row, uint32_t n_wg, int32_t only_stream, int init, hipStream_t stream);

// ---- S/PDIF subframe encoder (dspi_spdif.hip)
// The sample-rate byte of the channel status (audio_spdif.c:250-256) is a property of the DEVICE: streams of one context may run at
// different rates.  stream_image == nullptr: every stream at `fs`; else stream s reads img[stream_image[stream0 + s]].fs_hz.
// active (dspi_process's two-pass S/PDIF only, stream-major): the context's activity bitmap, indexed like stream_image; streams whose bit is
// clear are skipped — nothing of theirs is read or written.  null: every stream (dspi_spdif_encode is stateless per stream and knows no pauses).
struct SpdifRates { const DevImage *img; const uint32_t *stream_image; uint32_t stream0; const uint32_t *active = nullptr; };
// stream_pos (dspi_spdif_encode_v; dspi_process while dspi_spdif_per_stream is on): null = every stream starts at block_pos, the kernels of
// always; else one word per stream in device memory, indexed like stream_image (stream s reads stream_pos[stream0 + s]): the stream's first
// frame stands at (block_pos + stream_pos[..] mod 192) mod 192, block_pos < 192.
hipError_t launch_spdif(bool tiled, const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t row,
                        uint32_t n_wg, uint32_t block_pos, uint32_t fs, const SpdifRates &rates, hipStream_t stream, const uint32_t *stream_pos = nullptr);
// ---- the wire encoder (dspi_wire.hip; dspi_wire.h: the layout): launch_spdif's stream-major form with the TYPE of every pair taken from the
// stream's own image (DevImage::i2s_pairs, beside the fs_hz the encoder reads there): subframes for an S/PDIF slot, slot words (word << 8) in
// the first half of the region for an I2S slot.  rates.img and rates.stream_image are required; stream0, active and stream_pos as above.
// zero_tails (the host-buffer paths): I2S lanes also store zeros over the second half of their region; else nothing writes it.
hipError_t launch_wire(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t block_pos, const SpdifRates &rates,
                       bool zero_tails, hipStream_t stream, const uint32_t *stream_pos = nullptr);
// ---- the tiled wire encoder (dspi_wire_tiled.hip; dspi_wire.h: the tiled layout): launch_spdif's TILED form with the type of every pair taken
// from the column's own image.  pairs = [tile][output][n_frames][row] as the chain writes them with KArgs::tiled_out, out = [tile][pair][4 *
// n_frames][row]; n_streams columns from tile 0 on (n_streams <= n_tiles * row, the rest of the last tile holds nobody and is not touched);
// row = 64 or 128.  rates, stream_pos, zero_tails as for launch_wire; zero_tails zeroes rows 2 F .. 4 F - 1 of an I2S column.
constexpr uint32_t kWireTiledMaxFrames = 65535u * 32u;      // the frame slices ride on blockIdx.z
hipError_t launch_wire_tiled(const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t row, uint32_t n_tiles, uint32_t block_pos,
                             const SpdifRates &rates, bool zero_tails, hipStream_t stream, const uint32_t *stream_pos = nullptr);
// I2S slots (audio_i2s_multi.c:217-226): words << 8 for the pairs in pair_mask; same layouts as the pair words themselves
hipError_t launch_i2s(bool tiled, const int32_t *pairs, uint32_t *out, uint32_t n_streams, uint32_t n_pairs, uint32_t n_frames, uint32_t row,
                      uint32_t n_wg, uint32_t pair_mask, hipStream_t stream);

// ---- status at scale (dspi_status.hip): out[s] = OR of stream s's four sticky clip slots (state slots clip_slot .. clip_slot + 3)
hipError_t launch_detmath(int which, const float *a, const float *b, uint32_t n, float *out, hipStream_t stream);      // dspi_status.hip
hipError_t launch_clip_gather(const uint32_t *state, uint32_t n_streams, uint32_t row, uint32_t n_slots, uint32_t clip_slot, uint16_t *out, hipStream_t stream);

// ---- the meter bridge (dspi_meters.h: the words and the rules; dspi_meterbridge.hip: the kernels).  n_ch = 7 or 11; state / row / n_slots /
// clip_slot as for launch_clip_gather; everything else in device memory, 4-byte aligned.
// meters [n][n_ch] through the packets of peaks [n][n_blocks][n_ch], kMeterStagePackets (dspi_meters.h) of them in LDS at once; active: the activity bitmap or null = every stream (a paused stream's
// words and peaks are not touched)
hipError_t launch_meters_update(int n_ch, const uint16_t *peaks, uint32_t n, uint32_t n_blocks, uint32_t hold, uint32_t decay, uint32_t *meters, const uint32_t *active, hipStream_t stream);
// the alarm list of streams [0, n): three launches.  meters and info may be null; scratch: 2 * meters_alarm_workgroups(n) words.
constexpr uint32_t meters_alarm_workgroups(uint32_t n) { return (n + 255u) / 256u; }
hipError_t launch_meters_alarms(int n_ch, const uint32_t *state, uint32_t n, uint32_t row, uint32_t n_slots, uint32_t clip_slot, const uint32_t *meters, uint32_t level,
                                uint32_t *scratch, uint32_t *streams, uint32_t *info, uint32_t cap, uint32_t *total, hipStream_t stream);
// the status blocks (2 n_ch + 4 bytes each) of streams [first, first + count), back to back, into out (any alignment)
hipError_t launch_status_gather(int n_ch, const uint32_t *state, uint32_t first, uint32_t count, uint32_t row, uint32_t n_slots, uint32_t peaks_slot, uint32_t clip_slot, void *out,
                                hipStream_t stream);
// zero into the four clip slots of every listed stream (each < the context's streams; any order, duplicates allowed)
hipError_t launch_clip_clear(uint32_t *state, const uint32_t *list, uint32_t n_list, uint32_t row, uint32_t n_slots, uint32_t clip_slot, hipStream_t stream);

// ---- the context's four per-stream arrays, [W][position][R] each (dspi_snapshot.hip's and dspi_boot.hip's launchers take them as one) ----
struct StateArrays { uint32_t *state, *dlines, *ring, *pdm; };
// the one flavour ladder of their launchers (dspi_snapshot.hip, dspi_boot.hip; no chain file uses it): f(the flavour's row width as a
// compile-time constant)
template <class F>
void for_row_width(int flavor, F f) {
    if (flavor) f(std::integral_constant<uint32_t, 128>{});
    else f(std::integral_constant<uint32_t, 64>{});
}

// ---- stream snapshots (dspi_snapshot.hip): streams [first, first + count) of the four stream-minor arrays <-> stream-major records
// (dspi_snapshot.h), `records` = the record of stream `first`, 16-byte aligned.  import: records -> arrays, else arrays -> records.
hipError_t launch_snapshot(int flavor, bool import, const StateArrays &arr, uint32_t *records, uint32_t first, uint32_t count, hipStream_t stream);
// The realigning import (dspi_snapshot.h snap_row_target): two launches, the per-stream shifts into `shift` (2 words per stream of the range,
// 8-byte aligned device scratch), then the import rotated by them.  n_streams: the context's, for the rows' resident neighbours.
// `active` given (dspi_resume_streams): the same two launches under the activity-aware rule (dspi_snapshot.h snap_row_target_active).
// `active`: the bitmap before the call, one bit per stream; [r_first, r_first + r_count): the call's range, of which `records` hold the
// rows' chunk [first, first + count); streams the call does not resume are written back unrotated.
hipError_t launch_snapshot_realign(int flavor, const StateArrays &arr, uint32_t *records, uint32_t first, uint32_t count, uint32_t n_streams, uint32_t *shift, hipStream_t stream,
                                   const uint32_t *active = nullptr, uint32_t r_first = 0, uint32_t r_count = 0);

// ---- stream moves (dspi_move_streams; dspi_move.h: the lists; dspi_snapshot.hip: the kernels) ----
// The same transposition addressed by list: `items` = n_items MoveRowItem (one per touched row), `colrec` = per item one record index per
// column of the row (kMoveNone: the column is not listed and is neither read into a record nor written), both in device memory; `records`
// = record 0 of the scratch.  The gather reads listed columns into their records; the scatter writes records into listed columns, rotated
// by shift[destination stream] (two words per stream of the context, from launch_list_shifts) or, shift == nullptr, as they are.
hipError_t launch_move_gather(int flavor, const StateArrays &arr, uint32_t *records, const uint32_t *items, const uint32_t *colrec, uint32_t n_items, hipStream_t stream);
hipError_t launch_move_scatter(int flavor, const StateArrays &arr, uint32_t *records, const uint32_t *items, const uint32_t *colrec, uint32_t n_items, const uint32_t *shift,
                               hipStream_t stream);
// The shifts of a realigning list, one thread per entry, on the context that is written: shift[dst slot] from `targets` (n ListTarget,
// dspi_move.h) and `state`, that context's state array.  pos == nullptr (a move): every entry's own pair is read in place; else (a
// migration) `pos` holds the n pairs in list order, 8-byte aligned, that launch_migrate_positions wrote on the SOURCE context from its
// state array and the n source `slots` (there, or a copy of it).  All in device memory.
hipError_t launch_list_shifts(int flavor, const uint32_t *state, const uint32_t *targets, const uint32_t *pos, uint32_t n, uint32_t *shift, hipStream_t stream);
// ---- migration between two contexts (dspi_migrate_streams; dspi_migrate.h: the lists): the records go through launch_move_gather on the
// source context and launch_move_scatter on the destination context ----
hipError_t launch_migrate_positions(int flavor, const uint32_t *state, const uint32_t *slots, uint32_t n, uint32_t *pos, hipStream_t stream);

// ---- stream boots (dspi_boot_streams; dspi_boot.h: the list; dspi_boot.hip: the kernel) ----
// Power-on words into the listed columns of the four arrays (pdm may be null: a context that never ran the modulator has no array yet):
// `items` = n_items BootRowItem in device memory, one per touched row.  Reads nothing but the two position words of each item's target.
hipError_t launch_boot(int flavor, const StateArrays &arr, const uint32_t *items, uint32_t n_items, hipStream_t stream);

// ---- the intake of dspi_process_mixed (dspi_intake.h: the layout; dspi_intake.hip: the kernel) ----
// Streams [first, first + count) of the caller's mixed-depth bytes (stream s at src + offsets[s], depths[s] = 16 or 24; offsets [n_streams + 1]
// and depths [n_streams] in device memory, addressed by absolute stream like `active`, the activity bitmap or null) into dst + 6 frames s,
// packed 24 bit.  src and dst are 2-byte aligned; a paused stream is neither read nor written.
hipError_t launch_intake(const void *src, const uint64_t *offsets, const uint8_t *depths, const uint32_t *active, void *dst, uint64_t frames,
                         uint32_t first, uint32_t count, hipStream_t stream);

// ---- the S/PDIF receiver (dspi_spdifrx.h: the subframe, the record and the rule; dspi_spdifrx.hip: the kernel) ----
// Lines [first, first + count) of subframes, `frames` frames of 16 bytes each, through their records rx[line] (40 bytes each, device memory,
// read and written; a sync word above 192 is read as 0).  Line s stands at src + offsets[s] (offsets == nullptr: at src + 16 frames s), 16-byte
// aligned.  packed: dst + 6 frames s takes the packed 24-bit run the chain reads (2-byte aligned), as launch_intake writes it; else dst is
// int32 [line][frames][2], 8-byte aligned.  sources (null: every line): only lines whose entry is kSrcSpdif are served; active: the activity
// bitmap or null.  A line that is not served is neither read nor written, and neither is its record.  All indexed by absolute line.
hipError_t launch_spdifrx(bool packed, const void *src, const uint64_t *offsets, const uint8_t *sources, const uint32_t *active, void *rx, void *dst, uint64_t frames,
                          uint32_t first, uint32_t count, hipStream_t stream);

// ---- the link receivers (dspi_link.h: views, links, where a link's words lie; dspi_linkrx.hip: the kernels) ----
// Destinations [0, count): destination i takes links[i] (dspi::Link [count], device memory) of the wire buffer `wire` (n_pairs = 2 / 4, row = 0:
// the wire layout, 64 / 128: the tiled one; the links are valid for it) through its record rx[i] (S/PDIF links only; as for launch_spdifrx) into
// dst (packed: dst + 6 frames i, else int32 [count][frames][2]).  active: one bit per destination or null.  A destination whose link is
// kLinkNone or whose bit is clear is neither read nor written.  Stream-major views also need, for launch_spdifrx: offsets[i] = the byte offset
// of link i's region and kinds[i] = its kind as a byte (device memory).  any_spdif / any_i2s: what the links hold, as the host knows it.
hipError_t launch_linkrx(bool packed, const uint32_t *wire, const void *links, const uint64_t *offsets, const uint8_t *kinds, const uint32_t *active, void *rx, void *dst,
                         uint32_t frames, uint32_t n_pairs, uint32_t row, uint32_t count, bool any_spdif, bool any_i2s, hipStream_t stream);

// ---- the tiled receiver of dspi_process_patched (dspi_patch.h: the plan; dspi_patchrx.hip: the kernel) ----
// Destinations [0, count): destination i takes cols[i] (dspi::PatchCol [count], device memory, 16-byte aligned: the column of its line in whichever
// tiled view, resolved by the host) through its record rx[i] (S/PDIF patches only) into dst + 6 frames i, packed 24 bit.  A destination whose
// kind is kLinkNone is neither read nor written.  any_spdif: what the patches hold, as the host knows it.
hipError_t launch_patchrx(const void *cols, void *rx, void *dst, uint32_t frames, uint32_t count, bool any_spdif, hipStream_t stream);

// ---- the front end of dspi_process_packets (dspi_packets.h: the table and the address arithmetic; dspi_packetrx.hip: the kernel) ----
// Streams [0, n_streams): packet k of stream s (block_len frames at depths[s] = 16 or 24) from arena + table[s * n_blocks + k] into
// dst + 6 block_len (n_blocks s + k), packed 24 bit.  table [n_streams][n_blocks] and depths [n_streams] in device memory, the entries legal
// for the arena (dspi_packets.h) wherever `active`, the activity bitmap or null, has the stream's bit: a paused stream is neither read nor
// written, and neither are its entries.  arena and dst are 2-byte aligned.
hipError_t launch_packetrx(const void *arena, const uint64_t *table, const uint8_t *depths, const uint32_t *active, void *dst, uint32_t n_streams, uint32_t n_blocks,
                           uint32_t block_len, hipStream_t stream);

}  // namespace dspi
