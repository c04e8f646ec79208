// dspi_plan.h — which lanes of which workgroup run on which chain kernel (the launch plan of a context).
//
// Host only, no HIP: dspi_capi.cpp builds a PlanInput from the committed images at each rebuild, calls plan_launches and uploads
// the lists; tests/test_launch_plan_cpu.py drives plan_launches on the CPU.  What an item of each path means: WgItem, dspi_image.h.
// The layout of one dspi_process call (plan_call, below) lives here as well, under the same rule and the same test driver.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "dspi_image.h"

namespace dspi {

// One launcher call each (dspi_kernels.hip launch_chain), declared in launch order: dspi_process runs the non-empty ones in this
// order.  A path fixes what the plan decides; what each call decides (contract, 16/24 bit, ragged tail, tiled output, S/PDIF, the
// Q28 wave layout by size) stays at launch time.
enum class Path : uint8_t {
    F32Packed,          // packed kernel, lanes whose two streams share an image (dspi_chain_pk.inc)
    F32Skew1,           // latency layout (dspi_chain_skew.inc), shape 1: no output runs an EQ
    F32Skew2,           // ... shape 2: some output does
    F32Skew1PP,         // shape 1 with paired presets: the workgroup's slots hold different images of one ImageSig
    F32Skew2PP,         // shape 2 with paired presets
    F32PvBands,         // packed kernel with per-lane values, band coefficients per lane too
    F32PvShared,        // packed kernel with per-lane values, the row's filters shared
    F32OneStream,       // one stream per lane, every lane its own image (lanes the paths above leave)
    F32PackedLev,       // the same four packed paths with the leveller on ...
    F32Skew3,           // ... the latency layout's third shape (dspi_chain_skew_lev.inc)
    F32Skew3PP,
    F32PvBandsLev,
    F32PvSharedLev,
    Q28Uniform,         // Q28 chain, rows that hold one image: the image workgroup-uniform
    Q28PerLane,         // Q28 chain, rows that hold several: every lane its own image
};
constexpr int kNumPaths = 15;

// dspi_debug_launch_plan counts items by group (include/dspi.h): slots 0..5 in this order; slot 6 counts the paired latency items
enum class PathGroup : uint8_t { Q28Uniform, Packed, PerLaneImages, PvBands, PvShared, Latency };
struct PathInfo {
    Path path;
    PathGroup group;
    bool paired;        // latency layout with paired presets
};
constexpr PathInfo kPaths[kNumPaths] = {
    {Path::F32Packed, PathGroup::Packed, false},      {Path::F32Skew1, PathGroup::Latency, false},
    {Path::F32Skew2, PathGroup::Latency, false},      {Path::F32Skew1PP, PathGroup::Latency, true},
    {Path::F32Skew2PP, PathGroup::Latency, true},     {Path::F32PvBands, PathGroup::PvBands, false},
    {Path::F32PvShared, PathGroup::PvShared, false},  {Path::F32OneStream, PathGroup::PerLaneImages, false},
    {Path::F32PackedLev, PathGroup::Packed, false},   {Path::F32Skew3, PathGroup::Latency, false},
    {Path::F32Skew3PP, PathGroup::Latency, true},     {Path::F32PvBandsLev, PathGroup::PvBands, false},
    {Path::F32PvSharedLev, PathGroup::PvShared, false}, {Path::Q28Uniform, PathGroup::Q28Uniform, false},
    {Path::Q28PerLane, PathGroup::PerLaneImages, false},
};
constexpr bool paths_in_enum_order() {
    for (int p = 0; p < kNumPaths; p++) if ((int)kPaths[p].path != p) return false;
    return true;
}
static_assert(paths_in_enum_order(), "kPaths is indexed by Path");

// float flavour, per-lane VALUES: a row whose streams carry several presets of one structure runs the packed kernel with its numbers
// in a value tile (dspi_image.h); ImageSig = what has to agree for that (and for paired presets on the latency layout)
struct ImageSig {
    uint32_t flags, ch_bypassed, out_enabled, out_mute, fs_hz, mute_transition, mix_nz, i2s_pairs;
    int32_t delay[kMaxOut];
    uint8_t kinds[kPvBandSlots];
};
// two independent 64-bit hashes of an image's band coefficient words: rows whose images agree in both (and then word by word,
// PlanInput::same_filters) run the shared band loops, the rest of the numbers per lane
struct BandHash { uint64_t a, b; };

ImageSig make_sig(const DevImage &img);
BandHash hash_bands(const DevImage &img);
int skew_class(const ImageSig &g);

enum class F32Layout : uint8_t { Auto, Skew, Packed };      // DSPI_F32_LAYOUT: unset / skew / packed
uint32_t skew_pair_limit(int cls, uint32_t cus, F32Layout layout);

// per image, the rows that hold its streams in row order: WgItem{row, 0, lanes of the first stream, lanes of the second} (Q28:
// one stream per lane, mask1 = 0).  The state mutations run on these (dspi_capi.cpp commit_params).  `active` (one byte per stream, or
// null: every stream) leaves the streams out whose byte is 0: the launch plan's own rows (plan_launches), never the state mutations'.
std::vector<std::vector<WgItem>> image_rows(int flavor, uint32_t row, const int32_t *stream_image, uint32_t n_streams, size_t n_images,
                                            const uint8_t *active = nullptr);

struct PlanInput {
    int flavor = 1;                          // 0 = Q28, else float
    uint32_t n_streams = 0, row = 128;       // row: streams per workgroup (StateMap::row)
    std::vector<int32_t> stream_image;       // [n_streams]
    std::vector<uint32_t> refs;              // [image] streams that use it
    std::vector<uint8_t> active;             // [n_streams] 0: the stream is paused (dspi_pause_streams) and takes no part in a launch; empty: none is.
                                             // The plan is built from the active streams alone — rows, refs, every rule's lane counts
    std::vector<ImageSig> sig;               // [image] float only (ImageSig::flags: IF_LEVELLER_ON picks the leveller-on paths)
    std::vector<BandHash> bands;             // [image] float only
    uint32_t cus = 256;                      // compute units of the device
    F32Layout layout = F32Layout::Auto;
    bool paired = true;                      // DSPI_SKEW_PAIRED != 0
    std::function<bool(uint32_t, uint32_t)> same_filters;      // images a, b have the same band coefficient words
};

struct LaunchPlan {
    std::vector<WgItem> items[kNumPaths];    // per path, sorted by row
    uint32_t offset[kNumPaths] = {};         // of each list in one buffer of all of them, in Path order
    size_t total = 0;
    std::vector<uint8_t> row_pv;             // [row] 1 / 2: a per-lane-value row (F32PvBands / F32PvShared)
};

LaunchPlan plan_launches(const PlanInput &in);

// ---- one dspi_process call: the sizes of its buffers and how it moves them (dspi_capi.cpp dspi_process runs it) ----
struct CallInput {
    uint32_t n_streams = 0, n_wg = 0, row = 128;      // StateMap::row: streams per workgroup row, = per tile of DSPI_OUT_TILED
    uint32_t n_ch = 11, n_out = 9, n_pairs = 4;      // StateMap
    uint32_t n_blocks = 1, block_len = 1, bit_depth = 16;
    uint32_t flags = 0;                               // DSPI_MEM_DEVICE, DSPI_OUT_* (include/dspi.h)
    bool pairs = false, sub = false, peaks = false, clip = false;      // the outputs the caller passed (clip: with DSPI_OUT_CLIP_FLAGS)
    bool no_direct = false;                           // DSPI_NO_DIRECT
    bool all_latency = false;                         // float, and every non-empty path of the launch plan is on the latency layout
    bool pdm_words = false;                           // dspi_process_pdm: the caller's PDM words, beside the outputs above
    bool spdif_per_stream = false;                    // dspi_spdif_per_stream is on: the latency layout's fused encoder knows one position per launch
    bool wire_slots = false;                          // dspi_process_wire while an active stream has an I2S slot (dspi_wire.h wire_any_i2s): the fused encoder knows one type
    bool wire_tiled = false;                          // dspi_process_devices with DSPI_OUT_TILED: `pairs` is the wire layout, tiled (dspi_wire.h); sub and pdm_words tiled as ever
};

struct CallBuffer {
    size_t bytes = 0;          // 0: the caller did not pass it
    size_t per = 0;            // bytes per unit
    bool tile_cols = false;    // the unit: a tile column (DSPI_OUT_TILED words cover whole tiles) or a stream
    size_t off = 0;            // in the direct area
};

// the caller's device buffers; a pinned host area the kernels use directly (small host calls); device buffers, copies by row chunk
enum class CallMem : uint8_t { Device, Direct, Staged };

struct CallLayout {
    size_t frames = 0;
    CallBuffer pcm, pairs, sub, peaks, clip;
    CallBuffer pdm_words;                             // dspi_process_pdm (0 bytes: dspi_process): uint32 [unit][F][8], tiled [tile][F][8][R]
    CallBuffer sub_scratch;                           // ... when the caller passed no `sub`: the library's own Q28 sub words (device memory; `off` unused); staged: one chunk's
    bool spdif_two_pass = false;                      // DSPI_OUT_SPDIF off the latency layout, or with per-stream positions: the chain's pair words, then the encoder
    uint32_t two_pass_rows = 0; size_t two_pass_bytes = 0;      // rows per pass, their scratch of pair words
    bool wire_encoder = false;                        // ... and the second pass is the wire encoder (CallInput::wire_slots), not the subframe encoder
    bool wire_tiled = false;                          // ... its tiled form (CallInput::wire_tiled): the chain writes tiled pair words into the scratch
    CallMem mem = CallMem::Staged;
    size_t direct_bytes = 0;                          // the direct area: pcm, pairs, sub, peaks, clip, pdm_words at their `off`
    uint32_t n_chunks = 1, rows_per_chunk = 0;        // staged: chunk k = rows [k * rows_per_chunk, min(n_wg, (k + 1) * rows_per_chunk))
};

CallLayout plan_call(const CallInput &in);

}  // namespace dspi
