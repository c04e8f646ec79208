// dspi_patch.h — the patch bay (include/dspi.h: dspi_process_patched, dspi_patched_bytes): every stream of a call takes its frames from wherever
// it is plugged in — a run of `in` (dspi_spdifrx.h: PCM16, PCM24 or an S/PDIF run) or one line of one of up to kPatchMaxViews wire buffers
// (dspi_link.h: views, kinds and where a link's words lie).  Here: the byte layout of `in`, what the call refuses about its arguments, and the
// PLAN — everything the launches in front of the chain need, made on the host from the sources, the patches, the views and the activity bytes.
// Plain C++ (no HIP): dspi_capi.cpp includes it, tests/patch_driver.cpp exercises it without a GPU.  The kernels are dspi_intake.hip and
// dspi_spdifrx.hip as they are (the runs of `in`; the S/PDIF lines of a stream-major view), dspi_linkrx.hip's I2S kernel (the I2S lines of a
// stream-major view) and dspi_patchrx.hip (every tiled view of the call in one launch).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_link.h"
#include "dspi_spdifrx.h"

namespace dspi {

constexpr uint8_t kSrcLink = 2;             // DSPI_SRC_LINK: the stream's words are in somebody's wire buffer; it has no run in `in`
constexpr uint32_t kPatchMaxViews = 8;      // DSPI_MAX_VIEWS
struct Patch { uint32_t view, line, kind; };      // dspi_patch: line and kind as in Link, view < n_views
static_assert(sizeof(Patch) == 12, "a patch is three words");

// a tiled patch RESOLVED on the host: the kernel needs no table of views (one passed by value and indexed per lane would live in scratch
// memory).  col = the device address of the column's first word of the line's region; the words of the column are R apart, as
// link_spdif_word_tiled / link_i2s_word_tiled(…, c = 0) say.  An entry that is not served has kind kLinkNone and nothing else.
struct PatchCol { uint64_t col; uint32_t row, kind; };
static_assert(sizeof(PatchCol) == 16, "a resolved patch is 16 bytes");

constexpr bool patch_active(const uint8_t *active, uint32_t s) { return !active || active[s]; }
constexpr bool patch_source_ok(uint8_t src) { return src == kSrcLink || source_frame_bytes(src) != 0; }
constexpr uint32_t patch_frame_bytes(uint8_t src) { return src == kSrcLink ? 0u : source_frame_bytes(src); }

// ---- the layout of `in`: sources_offsets with one more rule, a LINK stream occupies no bytes (an S/PDIF run still starts at a multiple of 16)
// n + 1 values (offsets == nullptr: none written).  The sources are valid.  False when the size does not fit in 64 bits; nothing is written then.
bool patch_offsets(const uint8_t *sources, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets);

// ---- what the call refuses, one function per refusal (a text, or nullptr), in the call's order.  active: the host's activity bytes, or nullptr:
// every stream is active.  *at (may be null): the stream, or the view, the text speaks of. ----
const char *patch_sources_why(const uint8_t *sources, uint32_t n, uint32_t *at);                                            // 4
bool patch_any(const uint8_t *sources, uint32_t n, const uint8_t *active, uint8_t src);                                   // an ACTIVE stream of that source
const char *patch_views_why(const uint8_t *sources, uint32_t n, const uint8_t *active, const WireView *views, uint32_t n_views, const Patch *patches,
                            uint64_t frames, uint32_t *at);                                                                 // 5, when patch_any(.., kSrcLink)
bool patch_needs_in(const uint8_t *sources, uint32_t n, const uint8_t *active);                                           // an active stream has a run
bool patch_needs_rx(const uint8_t *sources, uint32_t n, const uint8_t *active, const Patch *patches);                     // ... is an S/PDIF run or link
const char *patch_in_why(const void *in, const uint8_t *sources, uint32_t n, const uint8_t *active);                      // 6
const char *patch_rx_why(const void *rx, const uint8_t *sources, uint32_t n, const uint8_t *active, const Patch *patches); // 7

// ---- the plan: ONE table for the device (uint64 words; every `at` below is an index into it), and what the host needs to know to launch ----
//   in_offsets   n + 1 byte offsets of the runs (patch_offsets)             } what launch_intake and launch_spdifrx over `in` read; an entry
//   in_kinds     n bytes: 16 / 24 / kSrcSpdif where the stream is served    } that is not served has kind 0
//   pcm_mask     one bit per stream: the intake's streams
//   per stream-major view that an active LINK stream names, what launch_linkrx (row 0) reads: n + 1 byte offsets of the regions, n Link, n kinds
//   cols         n PatchCol: every tiled view's patches together
// Not served: a paused stream, a stream of another source, a view of the other layout — kind NONE there, so no kernel looks at its line.
struct PatchPlan {
    std::vector<uint64_t> table;
    size_t in_offsets = 0, in_kinds = 0, pcm_mask = 0, cols = 0;
    bool any_pcm = false, any_spdif_in = false, any_tiled = false, tiled_spdif = false;      // tiled_spdif: a resolved patch is S/PDIF
    struct View { bool used = false, any_spdif = false, any_i2s = false; size_t offsets = 0, links = 0, kinds = 0; } view[kPatchMaxViews];
};
// Everything is valid by the refusals above (views and patches are looked at only where an active LINK stream needs them; they may be null when
// there is none).
void patch_plan(const uint8_t *sources, uint32_t n, const uint8_t *active, const WireView *views, uint32_t n_views, const Patch *patches, uint64_t frames, PatchPlan &p);

}  // namespace dspi
