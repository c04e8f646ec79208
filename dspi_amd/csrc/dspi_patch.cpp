// dspi_patch.cpp — the patch bay: the layout of `in`, the refusals and the plan of a dspi_process_patched call (dspi_patch.h).
#include "dspi_patch.h"

#include <string.h>

namespace dspi {

bool patch_offsets(const uint8_t *sources, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets) {
    // (every run with 15 bytes in front of it still fits: sources_offsets' bound, which a LINK stream only undercuts)
    if ((frames && (uint64_t)n > (UINT64_MAX - 15u * (uint64_t)n) / kRxFrameBytes / frames)) return false;
    uint64_t at = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (sources[s] == kSrcSpdif) at = (at + 15u) & ~(uint64_t)15;
        if (offsets) offsets[s] = at;
        at += frames * patch_frame_bytes(sources[s]);
    }
    if (offsets) offsets[n] = at;
    if (total) *total = at;
    return true;
}

const char *patch_sources_why(const uint8_t *sources, uint32_t n, uint32_t *at) {
    for (uint32_t s = 0; s < n; s++)
        if (!patch_source_ok(sources[s])) {
            if (at) *at = s;
            return "a source is none of DSPI_SRC_PCM16, DSPI_SRC_PCM24, DSPI_SRC_SPDIF, DSPI_SRC_LINK";
        }
    return nullptr;
}

bool patch_any(const uint8_t *sources, uint32_t n, const uint8_t *active, uint8_t src) {
    for (uint32_t s = 0; s < n; s++)
        if (sources[s] == src && patch_active(active, s)) return true;
    return false;
}

const char *patch_views_why(const uint8_t *sources, uint32_t n, const uint8_t *active, const WireView *views, uint32_t n_views, const Patch *patches,
                            uint64_t frames, uint32_t *at) {
    if (at) *at = 0;
    if (!views || !patches) return "an active DSPI_SRC_LINK stream needs views and patches";
    if (n_views == 0 || n_views > kPatchMaxViews) return "n_views is 1..DSPI_MAX_VIEWS";
    if (frames > 0xffffffffull) return "the view's n_frames is not n_blocks * block_len";
    for (uint32_t v = 0; v < n_views; v++)
        if (const char *why = link_view_why(views[v], frames, true)) {
            if (at) *at = v;
            return why;
        }
    for (uint32_t s = 0; s < n; s++) {
        if (sources[s] != kSrcLink || !patch_active(active, s)) continue;
        const Patch &p = patches[s];
        const char *const why = p.view >= n_views                               ? "a patch names no view of the call"
                                : p.kind != kLinkSpdif && p.kind != kLinkI2s    ? "a patch's kind is neither DSPI_LINK_SPDIF nor DSPI_LINK_I2S"
                                : p.line >= link_view_lines(views[p.view])      ? "a patch names no line of its view"
                                                                                : nullptr;
        if (why) {
            if (at) *at = s;
            return why;
        }
    }
    return nullptr;
}

bool patch_needs_in(const uint8_t *sources, uint32_t n, const uint8_t *active) {
    for (uint32_t s = 0; s < n; s++)
        if (sources[s] != kSrcLink && patch_active(active, s)) return true;
    return false;
}

bool patch_needs_rx(const uint8_t *sources, uint32_t n, const uint8_t *active, const Patch *patches) {
    for (uint32_t s = 0; s < n; s++)
        if (patch_active(active, s) && (sources[s] == kSrcSpdif || (sources[s] == kSrcLink && patches[s].kind == kLinkSpdif))) return true;
    return false;
}

const char *patch_in_why(const void *in, const uint8_t *sources, uint32_t n, const uint8_t *active) {
    if (!patch_needs_in(sources, n, active)) return nullptr;
    if (!in) return "an active stream with a run needs `in`";
    if (reinterpret_cast<uintptr_t>(in) % 16u) return "`in` is device memory and 16-byte aligned";
    return nullptr;
}

const char *patch_rx_why(const void *rx, const uint8_t *sources, uint32_t n, const uint8_t *active, const Patch *patches) {
    if (!patch_needs_rx(sources, n, active, patches)) return nullptr;
    if (!rx) return "an S/PDIF run or an S/PDIF link needs the receiver records (rx)";
    if (reinterpret_cast<uintptr_t>(rx) % 4u) return "device receiver records are 4-byte aligned";
    return nullptr;
}

void patch_plan(const uint8_t *sources, uint32_t n, const uint8_t *active, const WireView *views, uint32_t n_views, const Patch *patches, uint64_t frames, PatchPlan &p) {
    p = PatchPlan{};
    const size_t kind_words = ((size_t)n + 7) / 8, mask_words = ((size_t)n + 63) / 64;
    // who names what
    auto linked = [&](uint32_t s) { return sources[s] == kSrcLink && patch_active(active, s); };
    for (uint32_t s = 0; s < n; s++) {
        if (!linked(s)) continue;
        PatchPlan::View &pv = p.view[patches[s].view];
        pv.used = true;
        if (views[patches[s].view].tile_streams) { p.any_tiled = true; p.tiled_spdif = p.tiled_spdif || patches[s].kind == kLinkSpdif; }
        else (patches[s].kind == kLinkSpdif ? pv.any_spdif : pv.any_i2s) = true;
    }
    // the table's sections
    size_t words = 0;
    auto take = [&](size_t w) { const size_t at = words; words += w; return at; };
    p.in_offsets = take((size_t)n + 1); p.in_kinds = take(kind_words); p.pcm_mask = take(mask_words);
    for (uint32_t v = 0; v < n_views && v < kPatchMaxViews; v++)
        if (p.view[v].used && !views[v].tile_streams) { p.view[v].offsets = take((size_t)n + 1); p.view[v].links = take(n); p.view[v].kinds = take(kind_words); }
    words += words & 1u;      // (a resolved patch is one 16-byte load)
    p.cols = take(p.any_tiled ? 2 * (size_t)n : 0);
    p.table.assign(words, 0u);

    uint64_t *const t = p.table.data();
    patch_offsets(sources, n, frames, nullptr, t + p.in_offsets);
    uint8_t *const in_kinds = reinterpret_cast<uint8_t *>(t + p.in_kinds);
    uint32_t *const mask = reinterpret_cast<uint32_t *>(t + p.pcm_mask);
    PatchCol *const cols = reinterpret_cast<PatchCol *>(t + p.cols);
    for (uint32_t s = 0; s < n; s++) {
        if (!patch_active(active, s)) continue;
        if (sources[s] != kSrcLink) {
            in_kinds[s] = sources[s];
            if (sources[s] == kSrcSpdif) p.any_spdif_in = true;
            else { mask[s >> 5] |= 1u << (s & 31u); p.any_pcm = true; }
            continue;
        }
        const Patch &pt = patches[s];
        const WireView &v = views[pt.view];
        if (v.tile_streams) {
            const uint64_t word = link_region_tiled(pt.line, v.n_pairs, v.tile_streams, v.n_frames) + link_column(pt.line, v.n_pairs, v.tile_streams);
            cols[s] = PatchCol{(uint64_t)reinterpret_cast<uintptr_t>(v.wire) + word * 4u, v.tile_streams, pt.kind};
        } else {
            const PatchPlan::View &pv = p.view[pt.view];
            t[pv.offsets + s] = link_region(pt.line, v.n_frames) * 4u;
            const Link l{pt.line, pt.kind};
            memcpy(t + pv.links + s, &l, sizeof l);
            reinterpret_cast<uint8_t *>(t + pv.kinds)[s] = (uint8_t)pt.kind;
        }
    }
}

}  // namespace dspi
