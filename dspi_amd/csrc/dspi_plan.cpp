// dspi_plan.cpp — the launch plan: which lanes of which workgroup run on which chain kernel, and the layout of one call (dspi_plan.h).
#include "dspi_plan.h"

#include "../../include/dspi.h"

#include <string.h>

#include <algorithm>
#include <map>
#include <utility>

namespace dspi {

ImageSig make_sig(const DevImage &img) {
    ImageSig g;
    memset(&g, 0, sizeof g);
    g.flags = img.flags; g.ch_bypassed = img.ch_bypassed; g.out_enabled = img.out_enabled; g.out_mute = img.out_mute;
    g.fs_hz = img.fs_hz; g.mute_transition = img.mute_transition; g.i2s_pairs = img.i2s_pairs;
    for (int o = 0; o < kMaxOut; o++) {
        g.delay[o] = img.delay_samples[o];
        if (img.mix[0][o].f != 0.0f) g.mix_nz |= 1u << o;
        if (img.mix[1][o].f != 0.0f) g.mix_nz |= 1u << (kMaxOut + o);
    }
    for (int ch = 0; ch < kMaxCh; ch++) for (int b = 0; b < kBands; b++) g.kinds[ch * kBands + b] = (uint8_t)img.eq[ch][b].kind;
    g.kinds[kMaxCh * kBands] = (uint8_t)img.loud[0].kind; g.kinds[kMaxCh * kBands + 1] = (uint8_t)img.loud[1].kind;
    return g;
}

BandHash hash_bands(const DevImage &img) {
    uint64_t a = 0xcbf29ce484222325ull, b = 0x9e3779b97f4a7c15ull;      // FNV-1a and a multiply-xorshift mix over the same words
    auto feed = [&](uint32_t w) { a = (a ^ w) * 0x100000001b3ull; b = (b + w) * 0xff51afd7ed558ccdull; b ^= b >> 29; };
    for (int ch = 0; ch < kMaxCh; ch++) for (int k = 0; k < kBands; k++) for (int j = 0; j < 6; j++) feed(img.eq[ch][k].c[j].u);
    for (int k = 0; k < 2; k++) for (int j = 0; j < 6; j++) feed(img.loud[k].c[j].u);
    return BandHash{a, b};
}

// The latency layout of the float chain (dspi_chain_skew.inc) serves images with the leveller off.  Class 1: no output runs an EQ
// (disabled, muted, every band flat, or the sub in EQ-worker mode: exactly the cases in which output_item_pk skips the band loops) —
// eight stream pairs per workgroup, the outputs frame-parallel.  Class 2: some output does — two pairs per workgroup, every output a
// systolic row of its own.  Class 3: the leveller is on — the same two pairs and output rows, the groups of the workgroup passing frames
// through rings (dspi_chain_skew_lev.inc).
int skew_class(const ImageSig &g) {
    if (g.flags & IF_LEVELLER_ON) return 3;
    for (int o = 0; o < kMaxOut; o++) {
        const bool enabled = (g.out_enabled >> o) & 1u, muted = (g.out_mute >> o) & 1u, flat = (g.ch_bypassed >> (2 + o)) & 1u;
        const bool processed = o != kMaxOut - 1 || (g.flags & IF_SUB_ACTIVE);
        if (processed && enabled && !muted && !flat) return 2;
    }
    return 1;
}

// ... for launches that leave the chip underfilled: class 1 up to one of its eight-pair workgroups per CU (84 KB of LDS each), class 2
// up to two of its two-pair workgroups per CU (79 KB each); beyond that the packed kernel's throughput layout wins
// (tools/probe/probe8.hip, tools/bench_skew.py).  DSPI_F32_LAYOUT=skew|packed forces one (tests, development).
uint32_t skew_pair_limit(int cls, uint32_t cus, F32Layout layout) {
    if (layout == F32Layout::Skew) return 0xffffffffu;
    if (layout == F32Layout::Packed) return 0u;
    return (cls == 1 ? 8u : 4u) * cus;
}

std::vector<std::vector<WgItem>> image_rows(int flavor, uint32_t row, const int32_t *stream_image, uint32_t n_streams, size_t n_images,
                                            const uint8_t *active) {
    const bool two = flavor != 0;                 // float flavour: two streams per lane
    std::vector<std::vector<WgItem>> v(n_images);
    for (uint32_t s = 0; s < n_streams; s++) {
        if (active && !active[s]) continue;
        auto &l = v[(size_t)stream_image[s]];
        const uint32_t wg = s / row, col = s % row;
        if (l.empty() || l.back().wg != wg) l.push_back(WgItem{wg, 0u, 0ull, 0ull});
        if (two) { if (col & 1u) l.back().mask1 |= 1ull << (col >> 1); else l.back().mask |= 1ull << (col >> 1); }
        else l.back().mask |= 1ull << col;
    }
    return v;
}

namespace {

using ImageRows = std::vector<std::vector<WgItem>>;

struct RowAcc { uint64_t m0 = 0, m1 = 0; int n = 0; uint32_t first = 0; bool same = true, same_bands = true; };
using Rows = std::map<uint32_t, RowAcc>;      // row -> the images that hold its streams

// the context's last stream when the stream count is odd: a lane that holds one stream (cls 0: none, or a per-lane-value row)
struct OddLane { uint32_t row, lane, image; int cls; };

void sort_by_row(std::vector<WgItem> &v) {
    std::stable_sort(v.begin(), v.end(), [](const WgItem &x, const WgItem &y) { return x.wg < y.wg; });
}
bool leveller(const PlanInput &in, size_t image) { return (in.sig[image].flags & IF_LEVELLER_ON) != 0; }
uint32_t pairs_per_wg(int cls) { return cls == 1 ? 8u : 2u; }
Path latency_path(int cls, bool paired) {
    if (cls == 3) return paired ? Path::F32Skew3PP : Path::F32Skew3;
    if (cls == 2) return paired ? Path::F32Skew2PP : Path::F32Skew2;
    return paired ? Path::F32Skew1PP : Path::F32Skew1;
}
std::vector<WgItem> &list(LaunchPlan &p, Path path) { return p.items[(int)path]; }
uint32_t tag(uint32_t image, uint32_t part) { return image | (part << kSkPartShift); }

// Q28: rows with one image keep the workgroup-uniform path; rows with several run every lane on its own image, one item per row
void q28_lists(const std::vector<uint32_t> &refs, const ImageRows &rows_of, LaunchPlan &plan) {
    std::map<uint32_t, std::pair<uint64_t, int>> rows;      // row -> (lanes, images)
    for (size_t i = 0; i < rows_of.size(); i++)
        if (refs[i] > 0)
            for (const WgItem &it : rows_of[i]) { auto &r = rows[it.wg]; r.first |= it.mask; r.second++; }
    auto &uniform = list(plan, Path::Q28Uniform);
    for (size_t i = 0; i < rows_of.size(); i++)
        if (refs[i] > 0)
            for (WgItem it : rows_of[i])
                if (rows[it.wg].second == 1) { it.image = (uint32_t)i; uniform.push_back(it); }
    sort_by_row(uniform);
    for (const auto &r : rows)
        if (r.second.second > 1) list(plan, Path::Q28PerLane).push_back(WgItem{r.first, 0u, r.second.first, 0ull});
}

// Step 1 (float): rows holding several images of ONE structure are per-lane-value rows (packed kernel + value tile).  Row_pv 2 —
// identical filters: the kernel takes the band coefficients of the row's first image for every stream — is decided on two 64-bit
// hashes, then backed with the words themselves (same_filters) before it can cost bit-exactness.
Rows per_lane_value_rows(const PlanInput &in, const ImageRows &rows_of, std::vector<uint8_t> &row_pv) {
    Rows rows;
    for (size_t i = 0; i < rows_of.size(); i++)
        for (const WgItem &it : rows_of[i]) {
            RowAcc &r = rows[it.wg];
            if (r.n++ == 0) r.first = (uint32_t)i;
            else {
                if (memcmp(&in.sig[r.first], &in.sig[i], sizeof(ImageSig)) != 0) r.same = false;
                if (in.bands[r.first].a != in.bands[i].a || in.bands[r.first].b != in.bands[i].b) r.same_bands = false;
            }
            r.m0 |= it.mask; r.m1 |= it.mask1;
        }
    for (const auto &r : rows)
        if (r.second.n > 1 && r.second.same && (r.second.m0 & r.second.m1)) row_pv[r.first] = r.second.same_bands ? 2 : 1;
    for (size_t i = 0; i < rows_of.size(); i++)
        for (const WgItem &it : rows_of[i]) {
            if (row_pv[it.wg] != 2) continue;
            const uint32_t first = rows[it.wg].first;
            if (first != i && !in.same_filters(first, (uint32_t)i)) row_pv[it.wg] = 1;
        }
    return rows;
}

// Step 2 (float): lanes whose two streams share an image -> the packed kernel, one item per (row, image); per-lane-value rows -> one
// item per row, WgItem::image = the row's first image (read for the structure); every other lane -> the one-stream kernel, both lane
// components in one launch (WgItem::image = component), all images of a row in one item.  Leveller on / off: separate paths.
void shared_lists(const PlanInput &in, const std::vector<uint32_t> &refs, const ImageRows &rows_of, const Rows &rows, LaunchPlan &plan) {
    for (size_t i = 0; i < rows_of.size(); i++) {
        if (refs[i] == 0) continue;
        auto &dst = list(plan, leveller(in, i) ? Path::F32PackedLev : Path::F32Packed);
        for (const WgItem &it : rows_of[i]) {
            const uint64_t both = it.mask & it.mask1;
            if (both && !plan.row_pv[it.wg]) dst.push_back(WgItem{it.wg, (uint32_t)i, both, both});
        }
    }
    sort_by_row(list(plan, Path::F32Packed));
    sort_by_row(list(plan, Path::F32PackedLev));
    for (const auto &r : rows) {
        const uint8_t pv = plan.row_pv[r.first];
        if (!pv) continue;
        const bool lev = leveller(in, r.second.first);
        const Path p = pv == 1 ? (lev ? Path::F32PvBandsLev : Path::F32PvBands) : (lev ? Path::F32PvSharedLev : Path::F32PvShared);
        list(plan, p).push_back(WgItem{r.first, r.second.first, r.second.m0 & r.second.m1, 0ull});
    }
    auto &one = list(plan, Path::F32OneStream);
    for (uint32_t comp = 0; comp < 2; comp++) {
        std::map<uint32_t, uint64_t> lanes;      // row -> lanes whose stream `comp` alone is on an image
        auto only = [&](uint64_t m0, uint64_t m1) { return comp ? (m1 & ~m0) : (m0 & ~m1); };
        for (size_t i = 0; i < rows_of.size(); i++)
            if (refs[i] > 0)
                for (const WgItem &it : rows_of[i])      // (a per-lane-value row: only its half-filled lanes come here, below)
                    if (!plan.row_pv[it.wg] && only(it.mask, it.mask1)) lanes[it.wg] |= only(it.mask, it.mask1);
        for (const auto &r : rows)
            if (plan.row_pv[r.first] && only(r.second.m0, r.second.m1)) lanes[r.first] |= only(r.second.m0, r.second.m1);
        for (const auto &l : lanes) one.push_back(WgItem{l.first, comp, l.second, 0ull});
    }
    sort_by_row(one);
}

// The packed kernel leaves the last stream of an odd stream count to the one-stream kernel; the latency layout serves such a lane
// itself (its stores check the second stream) — a context of ONE stream is this case.  A paused last stream is in no list: no odd lane
// (and its image, which may be one that no active stream uses, is not read).
OddLane odd_lane(const PlanInput &in, const std::vector<uint8_t> &row_pv) {
    if (!(in.n_streams & 1u) || (!in.active.empty() && !in.active[in.n_streams - 1u])) return OddLane{0, 0, 0, 0};
    const uint32_t last = in.n_streams - 1u, row = last / in.row, image = (uint32_t)in.stream_image[last];
    return OddLane{row, (last % in.row) / 2u, image, row_pv[row] ? 0 : skew_class(in.sig[image])};
}

// Step 3, the all-small rule.  The whole context small — the lanes of every class within its limit: EVERY float lane takes the
// latency layout, whatever the presets: no per-lane-value tiles, no one-stream kernel, any mix of structures.  A workgroup = one part
// of a row (8 or 2 stream pairs).  The images that hold streams there: one -> a shared-preset item; several of ONE structure (ImageSig)
// -> one paired-preset item (the kernel reads every slot's numbers from its own image, args.stream_image; the item names the first
// image, for the structure); several structures -> one item per image, the other images' slots inactive (the kernels store per half).
// The limit counts lanes, a lane of the last kind once per image.  DSPI_SKEW_PAIRED=0 keeps to the last form (development, tests).
// Returns whether it placed the lanes.
bool all_small_rule(const PlanInput &in, const std::vector<uint32_t> &refs, const ImageRows &rows_of, LaunchPlan &plan) {
    auto limit = [&](int cls) { return (uint64_t)skew_pair_limit(cls, in.cus, in.layout); };
    uint64_t slots[4] = {0, 0, 0, 0};
    {   // a first bound: the lanes in use, whatever their images
        std::map<uint32_t, uint64_t> used[4];
        for (size_t i = 0; i < rows_of.size(); i++)
            if (refs[i] > 0)
                for (const WgItem &it : rows_of[i]) used[skew_class(in.sig[i])][it.wg] |= it.mask | it.mask1;
        for (int cls = 1; cls <= 3; cls++) for (const auto &u : used[cls]) slots[cls] += (uint64_t)__builtin_popcountll(u.second);
    }
    if (slots[1] + slots[2] + slots[3] == 0) return false;
    for (int cls = 1; cls <= 3; cls++) if (slots[cls] > limit(cls) * (cls == 2 ? 2u : 1u)) return false;      // (class 2: see below)
    struct Slot { uint32_t image; uint64_t m0, m1; };
    struct Cell { std::vector<Slot> v; bool same = false; };
    std::map<std::pair<uint32_t, uint32_t>, Cell> cells[4];      // [class]: (row, part) -> images
    for (size_t i = 0; i < rows_of.size(); i++) {
        if (refs[i] == 0) continue;
        const int cls = skew_class(in.sig[i]);
        const uint32_t ppw = pairs_per_wg(cls);
        for (const WgItem &it : rows_of[i])
            for (uint32_t part = 0; part < 64u / ppw; part++) {
                const uint64_t pm = ((1ull << ppw) - 1ull) << (part * ppw);
                if ((it.mask | it.mask1) & pm) cells[cls][{it.wg, part}].v.push_back(Slot{(uint32_t)i, it.mask & pm, it.mask1 & pm});
            }
    }
    for (int cls = 1; cls <= 3; cls++) {
        uint64_t n = 0;
        size_t paired = 0;
        for (auto &cell : cells[cls]) {
            const std::vector<Slot> &v = cell.second.v;
            bool same = in.paired && v.size() > 1;
            for (size_t j = 1; same && j < v.size(); j++)
                if (memcmp(&in.sig[v[0].image], &in.sig[v[j].image], sizeof(ImageSig)) != 0) same = false;
            cell.second.same = same;
            paired += same ? 1 : 0;
            uint64_t u = 0;
            for (const Slot &sl : v) { if (same) u |= sl.m0 | sl.m1; else n += (uint64_t)__builtin_popcountll(sl.m0 | sl.m1); }
            n += (uint64_t)__builtin_popcountll(u);
        }
        // Presets with output EQ and no leveller, mostly paired workgroups (every stream its own preset): the alternative is the packed
        // per-lane-filter kernel on an underfilled chip, and the layout wins up to twice its shared-preset limit (4 096 distinct
        // presets: 13.9 against 22.6 ms per 200 packets, profiles/r04_small_contexts_per_stream_leveller_off.jsonl).
        if (n > limit(cls) * ((cls == 2 && paired * 2 > cells[cls].size()) ? 2u : 1u)) return false;
    }
    for (int p = 0; p < kNumPaths; p++) if (kPaths[p].group != PathGroup::Latency) plan.items[p].clear();
    for (int cls = 1; cls <= 3; cls++)
        for (const auto &cell : cells[cls]) {      // (in (row, part) order: the lists come out sorted by row)
            const uint32_t row = cell.first.first, part = cell.first.second;
            const std::vector<Slot> &v = cell.second.v;
            if (cell.second.same) {
                uint64_t m0 = 0, m1 = 0;
                for (const Slot &sl : v) { m0 |= sl.m0; m1 |= sl.m1; }
                list(plan, latency_path(cls, true)).push_back(WgItem{row, tag(v[0].image, part), m0, m1});
            } else
                for (const Slot &sl : v) list(plan, latency_path(cls, false)).push_back(WgItem{row, tag(sl.image, part), sl.m0, sl.m1});
        }
    return true;
}

// Step 4, the size rule: shared-preset lanes whose image suits the latency layout move there, class by class, when the class's lanes
// leave the chip underfilled (take[cls]).  A latency-layout item is ONE workgroup: a row's item is cut into its non-empty parts; its
// masks stay the whole row's, the kernel reads the part's lanes only.
void size_rule(const PlanInput &in, LaunchPlan &plan, const bool (&take)[4]) {
    for (Path from : {Path::F32Packed, Path::F32PackedLev}) {
        std::vector<WgItem> keep;
        for (const WgItem &it : list(plan, from)) {
            const int cls = skew_class(in.sig[it.image]);
            if (!take[cls]) { keep.push_back(it); continue; }
            const uint32_t ppw = pairs_per_wg(cls);
            for (uint32_t part = 0; part < 64u / ppw; part++)
                if ((it.mask >> (part * ppw)) & ((1ull << ppw) - 1ull)) list(plan, latency_path(cls, false)).push_back(WgItem{it.wg, tag(it.image, part), it.mask, it.mask});
        }
        list(plan, from).swap(keep);
    }
}

// Step 5: the odd last stream follows its class to the latency layout: out of the one-stream item of its row, into the item of its
// image and part there (a new one if the part had none)
void odd_last_stream(const OddLane &odd, LaunchPlan &plan) {
    auto &one = list(plan, Path::F32OneStream);
    for (size_t i = 0; i < one.size(); i++) {
        if (one[i].wg != odd.row || one[i].image != 0u || !((one[i].mask >> odd.lane) & 1ull)) continue;      // (image = lane component, 0 = first stream)
        one[i].mask &= ~(1ull << odd.lane);
        if (one[i].mask == 0) one.erase(one.begin() + (long)i);
        auto &dst = list(plan, latency_path(odd.cls, false));
        const uint32_t t = tag(odd.image, odd.lane / pairs_per_wg(odd.cls));
        for (WgItem &d : dst) if (d.wg == odd.row && d.image == t) { d.mask |= 1ull << odd.lane; return; }
        dst.push_back(WgItem{odd.row, t, 1ull << odd.lane, 0ull});
        sort_by_row(dst);
        return;
    }
}

}  // namespace

LaunchPlan plan_launches(const PlanInput &in) {
    LaunchPlan plan;
    plan.row_pv.assign((in.n_streams + in.row - 1) / in.row, 0);
    // paused streams (PlanInput::active) are left out here, once: every list, rule and lane count below sees the active streams alone,
    // and an image counts the active streams on it
    const bool some_paused = !in.active.empty();
    const ImageRows rows_of = image_rows(in.flavor, in.row, in.stream_image.data(), in.n_streams, in.refs.size(), some_paused ? in.active.data() : nullptr);
    std::vector<uint32_t> active_refs;
    if (some_paused) {
        active_refs.assign(in.refs.size(), 0u);
        for (uint32_t s = 0; s < in.n_streams; s++) if (in.active[s]) active_refs[(size_t)in.stream_image[s]]++;
    }
    const std::vector<uint32_t> &refs = some_paused ? active_refs : in.refs;
    if (!in.flavor) q28_lists(refs, rows_of, plan);
    else {
        const Rows rows = per_lane_value_rows(in, rows_of, plan.row_pv);
        shared_lists(in, refs, rows_of, rows, plan);
        // the size rule's lanes per class: the shared-preset lanes, and the odd last stream
        const OddLane odd = odd_lane(in, plan.row_pv);
        uint64_t pairs[4] = {0, 0, 0, 0};
        for (Path p : {Path::F32Packed, Path::F32PackedLev})
            for (const WgItem &it : list(plan, p)) pairs[skew_class(in.sig[it.image])] += (uint64_t)__builtin_popcountll(it.mask);
        if (odd.cls) pairs[odd.cls]++;
        bool take[4] = {false, false, false, false};
        if (!all_small_rule(in, refs, rows_of, plan))
            for (int cls = 1; cls <= 3; cls++) take[cls] = pairs[cls] > 0 && pairs[cls] <= skew_pair_limit(cls, in.cus, in.layout);
        size_rule(in, plan, take);
        if (odd.cls && take[odd.cls]) odd_last_stream(odd, plan);
    }
    for (int p = 0; p < kNumPaths; p++) { plan.offset[p] = (uint32_t)plan.total; plan.total += plan.items[p].size(); }
    return plan;
}

CallLayout plan_call(const CallInput &in) {
    CallLayout L;
    const size_t F = L.frames = (size_t)in.n_blocks * in.block_len;
    // (the tiled wire layout is a tiled layout of subframe-sized regions, whatever the flags word says beside it)
    const bool tiled = (in.flags & DSPI_OUT_TILED) || in.wire_tiled, spdif = (in.flags & DSPI_OUT_SPDIF) || in.wire_tiled;
    auto buffer = [&](bool passed, bool tile_cols, size_t per) {
        return CallBuffer{passed ? (tile_cols ? (size_t)in.n_wg * in.row : (size_t)in.n_streams) * per : 0, per, tile_cols, 0};
    };
    L.pcm = buffer(true, false, F * (in.bit_depth == 24 ? 6 : 4));
    L.pairs = buffer(in.pairs, tiled, in.wire_tiled ? (size_t)in.n_pairs * F * 16 : tiled ? (size_t)(in.n_out - 1) * F * 4 : (size_t)in.n_pairs * F * (spdif ? 16 : 8));
    L.sub = buffer(in.sub, tiled, F * 4);
    L.peaks = buffer(in.peaks, false, (size_t)in.n_blocks * in.n_ch * 2);
    L.clip = buffer(in.clip, false, 2);
    L.pdm_words = buffer(in.pdm_words, tiled, F * 32);      // dspi_process_pdm: 8 words per frame, in the layout of the sub words

    // The latency layout's output waves encode the subframes themselves.  A launch with lanes on any other kernel (the flag is a property
    // of the output, not of the stream count) runs the chain into a scratch buffer of pair words, row chunk by row chunk, and the subframe
    // encoder from there into `pairs`: the same words, the block position carried the same way.  The scratch is capped by BYTES: ~1 GiB
    // worth of rows; one workgroup per CU (256 rows) only while that stays within 2 GiB; never less than one row.
    // With per-stream block positions (dspi_spdif_per_stream) every flagged call goes this way, the latency layout's launches too: its
    // kernels write plain pair words into the scratch (KArgs::pairs_stream0) and the encoder alone knows the streams' positions.
    // dspi_process_wire with an I2S slot on an active stream (CallInput::wire_slots) goes this way for the same reason: the type is the stream's.
    // The tiled wire layout (CallInput::wire_tiled) always goes this way, I2S slot or not: there is no fused tiled encoder.  The chain writes
    // TILED pair words into the scratch — a row of them is as large as a row of stream-major ones — and the tiled wire encoder runs from there.
    L.spdif_two_pass = spdif && in.pairs && (!in.all_latency || in.spdif_per_stream || in.wire_slots || in.wire_tiled);
    L.wire_encoder = L.spdif_two_pass && (in.wire_slots || in.wire_tiled);
    L.wire_tiled = L.spdif_two_pass && in.wire_tiled;
    if (L.spdif_two_pass) {
        const size_t row_b = (size_t)in.row * in.n_pairs * F * 8;
        size_t rows = std::max<size_t>(1, ((size_t)1 << 30) / row_b);
        if (rows < 256 && 256 * row_b <= ((size_t)2 << 30)) rows = 256;
        L.two_pass_rows = (uint32_t)std::min<size_t>(in.n_wg, rows);
        L.two_pass_bytes = L.two_pass_rows * row_b;
    }

    // the direct area: every buffer of the call at a 256-byte boundary, up to 2 MiB
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.pairs.off = up(L.pcm.bytes); L.sub.off = L.pairs.off + up(L.pairs.bytes); L.peaks.off = L.sub.off + up(L.sub.bytes);
    L.clip.off = L.peaks.off + up(L.peaks.bytes); L.pdm_words.off = L.clip.off + up(L.clip.bytes); L.direct_bytes = L.pdm_words.off + up(L.pdm_words.bytes);
    L.mem = (in.flags & DSPI_MEM_DEVICE) ? CallMem::Device : !in.no_direct && L.direct_bytes <= (2u << 20) ? CallMem::Direct : CallMem::Staged;

    // staged: from 32 MiB through the link, one chunk per 16 MiB, at most 8, and none without rows
    const size_t moved = L.pcm.bytes + L.pairs.bytes + L.sub.bytes + L.peaks.bytes + L.pdm_words.bytes;
    if (moved >= (32u << 20) && in.n_wg >= 2) L.n_chunks = (uint32_t)std::min<size_t>({(size_t)8, (size_t)in.n_wg, moved / (16u << 20)});
    L.rows_per_chunk = (in.n_wg + L.n_chunks - 1) / L.n_chunks;
    L.n_chunks = (in.n_wg + L.rows_per_chunk - 1) / L.rows_per_chunk;

    // dspi_process_pdm without out->sub: the chain's Q28 sub words go to a scratch of the library's, in device memory and in the call's
    // layout, and the modulator reads them there.  The whole call's — an eighth of the words buffer the caller passes anyway —, but on
    // the staged path one chunk's: the chain and the modulator of a chunk run back to back on one stream.
    if (in.pdm_words && !in.sub) {
        L.sub_scratch = buffer(true, tiled, F * 4);
        if (L.mem == CallMem::Staged) L.sub_scratch.bytes = (size_t)L.rows_per_chunk * in.row * L.sub_scratch.per;
    }
    return L;
}

}  // namespace dspi
