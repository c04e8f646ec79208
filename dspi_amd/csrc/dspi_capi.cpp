// dspi_capi.cpp — the C-ABI of libdspi_mi355x (include/dspi.h): context, device memory, launches.
//
// The context owns, per GPU: one state array, one delay-line array and one leveller ring for all
// streams (laid out per 64-stream workgroup, see dspi_image.h / DESIGN.md), plus a table of
// parameter images.  Streams reference images; a parameter call addressed to a single stream
// that shares its image clones the image first (copy-on-write), so "same preset on every
// stream" stays one broadcast image and per-stream presets still work — each distinct image is
// one launch over the workgroups (and lane masks) that use it.
#include <hip/hip_runtime.h>

#include <string.h>

#include <map>
#include <memory>
#include <new>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <type_traits>
#include <vector>
#include <thread>
#include <xmmintrin.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include "../../include/dspi_detmath.h"

#include "../../include/dspi.h"
#include "dspi_image.h"
#include "dspi_kernels.h"
#include "dspi_params.h"
#include "dspi_boot.h"
#include "dspi_devmem.h"
#include "dspi_flash.h"
#include "dspi_group.h"
#include "dspi_intake.h"
#include "dspi_link.h"
#include "dspi_meters.h"
#include "dspi_migrate.h"
#include "dspi_move.h"
#include "dspi_packets.h"
#include "dspi_packets_out.h"
#include "dspi_patch.h"
#include "dspi_pdmfade.h"
#include "dspi_pdmlife.h"
#include "dspi_plan.h"
#include "dspi_resize.h"
#include "dspi_snapshot.h"
#include "dspi_spdifpos.h"
#include "dspi_spdifrx.h"
#include "dspi_tablecheck.h"
#include "dspi_wire.h"

using namespace dspi;

struct dspi_ctx {
    int flavor = 1;
    bool fma = false;              // DSPI_FLOAT_CONTRACT_FMA: host design and kernels use the firmware build's fused multiply-adds
    uint32_t n_streams = 0, n_wg = 0;
    uint32_t cap_wg = 0;           // rows the persistent per-stream arrays (d_state, d_dlines, d_ring, d_pdm) are allocated for, >= n_wg (dspi_reserve_streams); no launch goes past n_wg
    int device = DSPI_DEVICE_NONE;
    StateMap sm{};
    DevMem mem;                    // every DevBuf / PinnedBuf below registers here; dspi_destroy releases through it (no member destructor makes a HIP call)
    std::vector<std::unique_ptr<Params>> images;
    std::vector<uint32_t> image_refs;
    std::vector<int32_t> stream_image;
    bool assignment_dirty = true;
    bool merge_hint = false;       // a broadcast call ran while several images were live: equal images fold back into one (merge_images)
    // per image, the rows that hold its streams (dspi_plan.h image_rows): the state mutations' work lists, uploaded to d_items
    std::vector<std::vector<WgItem>> image_rows;
    std::vector<uint32_t> image_rows_offset;
    // chain launches (dspi_plan.h): one list per kernel path, each covering every image, so a dspi_process is a handful of launches
    // however many presets are in play; uploaded to d_litems at plan.offset
    PlanInput plan_in;             // its sig / bands: per image, what the last upload built (commit_params)
    LaunchPlan plan;
    DevBuf<WgItem> d_litems{mem};
    DevBuf<uint32_t> d_stream_image{mem};   // image index per stream (per-lane parameter kernel)
    bool launch_dirty = true;
    uint32_t spdif_pos = 0;      // DSPI_OUT_SPDIF: block position of the next call's first frame
    // dspi_spdif_per_stream: while on, DSPI_OUT_SPDIF encodes stream s at its own position (dspi_spdifpos.h) and spdif_pos above only counts;
    // the device's copy of the per-stream words goes up behind the context's stream when a call has changed one (upload_spdif_pos)
    SpdifPos spdif_ps;
    DevBuf<uint32_t> d_spdif_ps{mem};
    DevBuf<uint32_t> d_spdif_vpos{mem};      // dspi_spdif_encode_v on host buffers: the caller's positions
    bool populated = false;      // DSPI_BOOT_POPULATED_FLASH: the streams are devices whose flash already holds a preset directory
    bool audio_started = false;  // a dspi_process has run: the devices are no longer booting (dspi_load_flash_dump)
    bool no_direct = false;      // DSPI_NO_DIRECT (development / tests, read once at dspi_create): the staged path for small host calls too
    bool no_emit_lines = false;  // DSPI_NO_EMIT_LINES (development / tests, read once at dspi_create): the emitter wave of the packed float kernel never takes its whole-line path
    // the leveller's alpha^count on the device is step 1 + a table that was generated for the firmware's 18 alphas (include/dspi_detmath.h); the
    // alphas this context has actually built into images, and the block length they were last checked with against the exact form
    std::vector<uint32_t> lv_alphas; uint32_t lv_checked_count = 0; size_t lv_checked_n = 0;
    uint32_t direct_spin_us = 0; // DSPI_DIRECT_SPIN_US (read once at dspi_create): how long a direct call polls its stream before the blocking wait; 0 = the call's own audio time (>= 300 us)
    uint64_t direct_stats[5] = {0, 0, 0, 0, 0};      // dspi_debug_direct_stats: calls, calls that fell back to the blocking wait, max enqueue ns, max wait ns, last spin budget ns
    // device
    hipStream_t hs = nullptr;
    // host-buffer dspi_process: H2D, kernels and D2H of consecutive row chunks overlap on three streams (created on first use)
    hipStream_t hs_in = nullptr, hs_out = nullptr;
    std::vector<hipEvent_t> pipe_events;
    DevBuf<uint32_t> d_state{mem}, d_dlines{mem}, d_ring{mem};
    DevBuf<uint32_t> d_xwords{mem};      // exchange area of the packed kernel's copy wave (stream-major output)
    DevBuf<DevImage> d_images{mem};
    std::vector<uint32_t> image_flags;             // DevImage::flags of each uploaded image (kernel variant selection)
    std::vector<uint8_t> image_touched;            // images uploaded since the tiles were last built
    DevBuf<float> d_vals{mem};
    DevBuf<uint32_t> d_pv_rows{mem};
    DevBuf<WgItem> d_items{mem};
    // staging buffers for host-memory dspi_process
    DevBuf<void> d_in{mem};
    DevBuf<int32_t> d_pairs{mem};
    DevBuf<int32_t> d_sub{mem};
    DevBuf<uint16_t> d_peaks{mem};
    DevBuf<uint16_t> d_clip{mem};          // DSPI_OUT_CLIP_FLAGS on host buffers
    // small calls on host buffers (one packet per call, the firmware's own rhythm): a pinned host area the kernels read and write directly
    PinnedBuf<char> h_direct{mem};      // (.device(): what the kernels address)
    // ... and a completion word of its own next to that area (round 6): the stream writes the call's sequence number there once the launches
    // have ended (hipStreamWriteValue32) and the host polls MEMORY instead of calling into the runtime (hipStreamQuery) thousands of times
    PinnedBuf<uint32_t> h_done{mem}; uint32_t direct_seq = 0; int direct_flag = -1;      // -1: untried, 0: not available / DSPI_DIRECT_POLL=query, 1: in use
    DevBuf<int32_t> d_spdif_words{mem};      // DSPI_OUT_SPDIF on launches the latency layout does not serve: the chain's pair words of one row chunk
    // PDM sub output (dspi_pdm.hip): modulator state per stream, allocated on first use; staging for host buffers
    DevBuf<uint32_t> d_pdm{mem};
    DevBuf<int32_t> d_pdm_in{mem};
    DevBuf<uint32_t> d_pdm_out{mem};
    // dspi_process_pdm (dspi_pdmlife.h): who runs their modulator, the device's copy of the call's work list (it goes up through h_move, behind
    // ev_move, when the list was rebuilt), and per parameter object the core1_mode it was last uploaded with (a change makes the list dirty)
    PdmLife pdm_life;
    DevBuf<uint32_t> d_pdm_list{mem};
    std::vector<int8_t> image_core1;
    // dspi_pdm_fade (dspi_pdmfade.h): the mode and the fade positions; the fade bases [cap_wg * row] (allocated when the mode is first enabled, they
    // follow the capacity like d_pdm); the packed temporary the bases travel through.  The call's aux words stand behind the list in d_pdm_list.
    PdmFade pdm_fade;
    DevBuf<int32_t> d_pdm_base{mem};
    DevBuf<int32_t> d_pdm_pack{mem};
    // the arrays that follow the row capacity cap_wg, in the order of their table (dspi_devmem.h kPersist): dspi_create, pdm_state, dspi_pdm_fade and the resizes walk it
    MemNode *const persist[kNumPersist] = {&d_state, &d_dlines, &d_ring, &d_pdm, &d_pdm_base};
    // The audio calls' front end (CallFront).  d_mixed: device buffers only — a scratch of n_streams * 6F bytes that the front end's kernels
    // (the intake, the receivers: every kind but Pcm) write and the chain reads, both on `hs`, asynchronously.  d_mixed_up: staged host buffers
    // only, mixed calls only — where a chunk's bytes go up as they are (on hs_in when the call has several chunks), the intake then writes
    // d_in.  THE RULE: whatever a stream other than `hs` touches (hs_in: d_in, d_mixed_up) belongs to the staged path alone, which ends
    // synchronised; nothing that an asynchronous call leaves in flight on `hs` is touched from another stream.  That is why the two paths do
    // not share one scratch.  d_mixed_tab: the device's table of the call's front end, whichever kind (a mixed call's: (n + 1) uint64 offsets
    // with the n depths behind them), read and written on `hs` only.  ONE owner: it goes up through upload_front_table alone (through h_move,
    // behind ev_move), which forgets what the table held.  A mixed call's table stays while the depths and the frame count repeat:
    // mixed_depths / mixed_frames say what it holds (0 frames: no mixed call's layout), and only intake_prepare sets them
    DevBuf<uint8_t> d_mixed{mem};
    DevBuf<uint8_t> d_mixed_up{mem};
    DevBuf<uint64_t> d_mixed_tab{mem};
    std::vector<uint8_t> mixed_depths; uint64_t mixed_frames = 0;
    // dspi_process_sources (dspi_spdifrx.h): a call with an S/PDIF source appends to the table the bitmap of the streams the INTAKE serves, the
    // active PCM streams (mixed_mask: what the table holds of it; empty: none); the receiver kernel reads the sources and the context's own
    // activity bitmap.  d_rx: the records of a host-memory call, on `hs` only, by calls that end synchronised (staged calls, dspi_spdif_decode)
    std::vector<uint32_t> mixed_mask;
    DevBuf<SpdifRx> d_rx{mem};
    DevBuf<int32_t> d_spdif_in{mem};
    DevBuf<uint32_t> d_spdif_out{mem};
    DevBuf<uint32_t> d_snap{mem};          // stream snapshots on host buffers: the records of one chunk of rows
    DevBuf<uint32_t> d_snap_shift{mem};      // realigning imports: two rotations per stream of a launch (dspi_snapshot.hip)
    // paused streams (dspi_pause_streams): a property of the SLOT.  `active` is the truth (one byte per stream, 1 = takes part in dspi_process;
    // empty until the first pause); the launch plan is built from it (PlanInput::active) and the kernels that walk every stream whatever the
    // plan says (PDM modulator, two-pass S/PDIF encoder, value-tile builder, the resume's target rule) read one bit per stream on the device,
    // uploaded when it has changed and something needs it (upload_activity)
    std::vector<uint8_t> active; uint32_t n_paused = 0;
    std::vector<std::pair<uint32_t, uint32_t>> paused_runs; bool paused_runs_dirty = false;      // [first, end) of consecutive paused streams: what the host-buffer paths zero
    DevBuf<uint32_t> d_active{mem}; bool active_dirty = false;
    // dspi_move_streams: records per batch (DSPI_MOVE_BATCH, read once at dspi_create; 0 = the snapshot chunk), and one call's work lists —
    // built in a pinned host area, copied up on the context's stream; the event says when the area may be rewritten
    uint32_t move_batch = 0;
    DevBuf<uint32_t> d_move{mem};
    PinnedBuf<char> h_move{mem}; hipEvent_t ev_move = nullptr;
    // dspi_migrate_streams: the transport (DSPI_MIGRATE_VIA, read once at dspi_create; the DESTINATION context's value decides), the listed
    // streams' positions (written on the source, read — there or as a copy here — on the destination), the host transport's pinned area,
    // and "my stream has come this far": recorded on this context's stream, waited for on the other's
    enum MigrateVia { kViaAuto = 0, kViaCopy = 1, kViaHost = 2 };
    int migrate_via = kViaAuto;
    DevBuf<uint32_t> d_mig_pos{mem};
    PinnedBuf<char> h_mig{mem};
    hipEvent_t ev_mig = nullptr;
    // dspi_process_linked: "the producer's stream has come this far": recorded on the PRODUCER's stream, waited for on this context's
    hipEvent_t ev_link = nullptr;
    // dspi_device_flash (dspi_flash.h): while on, every stream holds a flash of its own (shared until written) and the preset directory requests
    // are served from it.  Host memory only; consulted in request and maintenance paths, never by dspi_process.
    FlashBook flash;
    // the meter bridge (dspi_meters.h): no state of its own — the meters are the caller's.  Scratch on `hs` only: the alarm kernels' counts and
    // offsets, the uploaded list of dspi_clear_clips_list (through h_move, behind ev_move), and what a host-memory call brings down (every
    // stream's clip word, or the status blocks of a range) before it ends synchronised
    DevBuf<uint32_t> d_meter_scan{mem};
    DevBuf<uint32_t> d_meter_list{mem};
    DevBuf<uint8_t> d_meter_down{mem};
    // dspi_packets_emit (dspi_packets_out.h): no state — the device's copy of the call's table with the formats behind it, on `hs` only (it goes
    // up through h_move, behind ev_move).  Not d_mixed_tab: a process call's table stays what that call left.
    DevBuf<uint64_t> d_emit_tab{mem};
    // the resident packet tables' entry check (dspi_tablecheck.h): no state — the answer word, with the call's n depth / format bytes behind it
    // (they go up through h_move, behind ev_move), on `hs` only.  Not d_mixed_tab: a check leaves the front end's table what it was.
    DevBuf<uint64_t> d_tabcheck{mem};
    std::string err;
};

namespace {

int fail(dspi_ctx *c, int code, const std::string &msg) { if (c) c->err = msg; return code; }
// two refusals that many calls share, each text once: a call that needs the GPU on a context without one, and a call's lengths (`who`: the public call)
int refuse_host_only(dspi_ctx *c) { return fail(c, DSPI_E_NODEVICE, "host-only context: the HIP path is the only audio path"); }
int refuse_lengths(dspi_ctx *c, const char *who) { return fail(c, DSPI_E_INVAL, std::string(who) + ": 1 <= block_len <= 192, n_blocks >= 1"); }

#define HIPCK(c, call)                                                                                   \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail((c), DSPI_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

bool valid_stream(const dspi_ctx *c, int32_t s) { return s == DSPI_ALL_STREAMS || (s >= 0 && (uint32_t)s < c->n_streams); }

// The books of the parameter objects.  add_image appends one that no stream uses yet (the next commit uploads it) and returns its slot;
// assign_image points a stream at a slot.  An object that loses its last stream keeps its slot until the fold-back pass drops it
// (merge_images): a caller that can cause that asks for the pass (merge_hint).
int32_t add_image(dspi_ctx *c, std::unique_ptr<Params> p) {
    p->dirty = true;
    c->images.push_back(std::move(p)); c->image_refs.push_back(0);
    return (int32_t)c->images.size() - 1;
}
void assign_image(dspi_ctx *c, size_t stream, int32_t slot) {
    int32_t &si = c->stream_image[stream];
    c->image_refs[(size_t)si]--; si = slot; c->image_refs[(size_t)slot]++;
    c->assignment_dirty = true;
}

// parameter object to mutate for `stream` (copy-on-write when shared)
Params *writable(dspi_ctx *c, int32_t stream) {
    int32_t idx = c->stream_image[(size_t)stream];
    if (c->image_refs[(size_t)idx] > 1) {
        // a reference count never drops to zero (the last stream of an image keeps it), so clones always append
        const size_t slot = c->images.size();
        auto clone = std::make_unique<Params>(*c->images[(size_t)idx]);
        clone->dirty = true;
        c->images.push_back(std::move(clone)); c->image_refs.push_back(1);
        c->image_refs[(size_t)idx]--;
        c->stream_image[(size_t)stream] = (int32_t)slot;
        c->assignment_dirty = true;
        idx = (int32_t)slot;
    }
    return c->images[(size_t)idx].get();
}

// A broadcast call may make separate images equal again (the same whole state for everyone, or a request that removes the only
// difference): it asks for the fold-back pass at the next commit.  When that pass finds nothing to fold it leaves the images as they
// were — no re-upload, no rebuilt lists (merge_images) —, so a broadcast volume change on 65 536 distinct presets costs one hashing pass.
template <class F>
int for_targets(dspi_ctx *c, int32_t stream, F f) {
    if (!c) return DSPI_E_INVAL;
    if (!valid_stream(c, stream)) return fail(c, DSPI_E_INVAL, "stream index out of range");
    if (stream == DSPI_ALL_STREAMS) {
        int rc = 0;
        if (c->images.size() > 1) c->merge_hint = true;
        for (size_t i = 0; i < c->images.size(); i++)
            if (c->image_refs[i] > 0) { int r = f(*c->images[i]); if (r != 0) rc = r; }
        return rc;
    }
    return f(*writable(c, stream));
}

// Streams that were given presets of their own and then received the same whole state again (load_bulk / preset / factory reset
// with DSPI_ALL_STREAMS) hold equal parameter objects: fold them back into one image, so the rows return to the shared-parameter
// kernels and a commit is one upload again.  Params is trivially copyable and zero-filled before construction, so equal bytes
// <=> equal parameters, pending state operations included; unequal padding could only keep two images apart, never merge them.
static_assert(std::is_trivially_copyable<Params>::value, "merge_images compares parameter objects as bytes");
void merge_images(dspi_ctx *c) {
    c->merge_hint = false;
    const size_t ni = c->images.size();
    std::vector<size_t> live;
    for (size_t i = 0; i < ni; i++) if (c->image_refs[i] > 0) live.push_back(i);
    if (ni < 2) return;
    std::vector<uint8_t> was_dirty(ni, 0);
    for (size_t i : live) {
        Params &p = *c->images[i];
        was_dirty[i] = p.dirty ? 1 : 0;
        p.dirty = true;                                            // the flag is part of the bytes that are compared; restored below when nothing merges
        if (p.ops.reset_all_eq) memset(p.ops.reset_band, 0, sizeof p.ops.reset_band);      // the wipe covers every band (state_ops_kernel): which single bands a stream's history also marked does not matter
    }
    std::vector<uint64_t> h(ni, 0);
    auto hash = [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; k++) {
            const unsigned char *b = reinterpret_cast<const unsigned char *>(c->images[live[k]].get());
            uint64_t x = 0xcbf29ce484222325ull;
            for (size_t j = 0; j + 8 <= sizeof(Params); j += 8) { uint64_t w; memcpy(&w, b + j, 8); x = (x ^ w) * 0x100000001b3ull; x ^= x >> 29; }
            h[live[k]] = x;
        }
    };
    const size_t n = live.size();
    const size_t nt = n >= 512 ? std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), std::min<size_t>(32, n / 128)) : 1;
    if (nt > 1) {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; t++) th.emplace_back(hash, n * t / nt, n * (t + 1) / nt);
        for (auto &x : th) x.join();
    } else hash(0, n);
    std::unordered_map<uint64_t, std::vector<size_t>> seen;     // hash -> surviving images (old indices)
    std::vector<int32_t> remap(ni, -1);
    std::vector<size_t> keep;
    for (size_t i : live) {
        auto &cands = seen[h[i]];
        int32_t to = -1;
        for (size_t k : cands) if (memcmp(c->images[k].get(), c->images[i].get(), sizeof(Params)) == 0) { to = remap[k]; break; }
        if (to < 0) { to = (int32_t)keep.size(); keep.push_back(i); cands.push_back(i); }
        remap[i] = to;
    }
    if (keep.size() == ni) {                                      // nothing equal, nothing dead: nothing to upload that was not dirty already
        for (size_t i : live) c->images[i]->dirty = was_dirty[i] != 0;
        return;
    }
    std::vector<std::unique_ptr<Params>> images;
    for (size_t i : keep) images.push_back(std::move(c->images[i]));
    c->images = std::move(images);
    c->image_refs.assign(keep.size(), 0);
    for (auto &si : c->stream_image) { si = remap[(size_t)si]; c->image_refs[(size_t)si]++; }
    // per-image caches describe the old numbering: drop them, every image goes up again
    c->image_flags.clear(); c->plan_in.sig.clear(); c->plan_in.bands.clear(); c->image_touched.clear(); c->image_core1.clear();
    c->assignment_dirty = true; c->launch_dirty = true;
}

const Params &readable(const dspi_ctx *c, int32_t stream) {
    return *c->images[(size_t)c->stream_image[stream == DSPI_ALL_STREAMS ? 0 : (size_t)stream]];
}

// ---- the streams' own flashes (dspi_device_flash; the model and the book are dspi_flash.h) ----
// A request that may write the flash, for one stream (both objects clone on write) or for all: once per distinct (parameter object, flash
// object) pair, after an object that stands in several pairs got a clone per further pair, so that streams that shared both keep sharing
// both.  f(Params &, Flash &) answers like Params::vendor_get; a broadcast answers with stream 0's device.
template <class F>
int for_flash_targets(dspi_ctx *c, int32_t stream, F f) {
    if (stream != DSPI_ALL_STREAMS) { Params *p = writable(c, stream); return f(*p, *c->flash.writable((uint32_t)stream)); }
    std::vector<uint32_t> pair_of;
    const std::vector<FlashPair> pairs = flash_pairs(c->stream_image, c->flash.index, &pair_of);
    std::vector<int32_t> image(pairs.size()), obj(pairs.size());
    std::vector<uint8_t> image_seen(c->images.size(), 0), obj_seen(c->flash.objects.size(), 0);
    bool split = false;
    for (size_t k = 0; k < pairs.size(); k++) {
        image[k] = pairs[k].image; obj[k] = pairs[k].flash;
        if (image_seen[(size_t)pairs[k].image]) { image[k] = add_image(c, std::make_unique<Params>(*c->images[(size_t)pairs[k].image])); split = true; }
        if (obj_seen[(size_t)pairs[k].flash]) { obj[k] = c->flash.add(std::make_unique<Flash>(*c->flash.objects[(size_t)pairs[k].flash])); split = true; }
        image_seen[(size_t)pairs[k].image] = obj_seen[(size_t)pairs[k].flash] = 1;
    }
    if (split)
        for (uint32_t s = 0; s < c->n_streams; s++) {
            const uint32_t k = pair_of[s];
            if (image[k] != c->stream_image[s]) assign_image(c, s, image[k]);
            if (obj[k] != c->flash.index[s]) c->flash.assign(s, obj[k]);
        }
    if (c->images.size() > 1) c->merge_hint = true;
    int rc = 0;
    for (size_t k = pairs.size(); k-- > 0;) rc = f(*c->images[(size_t)image[k]], *c->flash.objects[(size_t)obj[k]]);      // (stream 0's pair last: its answer stands)
    return rc;
}

// The mirrors of the parameter objects of [first, first + count) follow their slots' directories: where they disagree (objects that came
// from elsewhere: an import), the streams of one (object, flash) pair move to one clone that agrees.
void flash_resync(dspi_ctx *c, const uint32_t *streams, uint32_t first, uint32_t count) {      // streams == nullptr: the range from `first`
    std::map<std::pair<int32_t, int32_t>, int32_t> fixed;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t s = streams ? streams[i] : first + i;
        const Flash &fl = c->flash.readable(s);
        const PresetDir d = fl.directory();
        const Params &r = *c->images[(size_t)c->stream_image[s]];
        if (r.dir_master_volume_mode == d.master_volume_mode && r.dir_include_pins == d.include_pins && memcmp(&r.dir_master_volume_db, &d.master_volume_db, 4) == 0) continue;
        const std::pair<int32_t, int32_t> key(c->stream_image[s], c->flash.index[s]);
        auto it = fixed.find(key);
        if (it == fixed.end()) {
            auto p = std::make_unique<Params>(r);
            flash_sync_mirrors(fl, *p);
            it = fixed.emplace(key, add_image(c, std::move(p))).first;
        }
        assign_image(c, s, it->second);
        c->merge_hint = true;
    }
}
void flash_resync(dspi_ctx *c, uint32_t first, uint32_t count) { flash_resync(c, nullptr, first, count); }

// one new flash object per distinct parameter object among the streams of [first, first + count): the first-boot flash with that object's
// mirrored master-volume fields (dspi_device_flash(1), arrivals from a context without the mode)
void flash_first_boot_range(dspi_ctx *c, uint32_t first, uint32_t count) {
    std::vector<int32_t> of_image(c->images.size(), -1);
    for (uint32_t s = first; s < first + count; s++) {
        int32_t &o = of_image[(size_t)c->stream_image[s]];
        if (o < 0) o = c->flash.add(Flash::first_boot(c->flavor, c->populated, c->images[(size_t)c->stream_image[s]].get()));
        c->flash.assign(s, o);
    }
    flash_resync(c, first, count);
}

// The allocator of dspi_devmem.h on HIP — the one place that allocates and frees.  hipFree and hipHostFree wait for the device, and growing
// a buffer that earlier asynchronous calls may still be using rests on that: no asynchronous, pooled or deferred free may take their place.
struct HipAlloc {
    hipError_t last = hipSuccess;      // what the call that failed answered
    bool ok(hipError_t e) { last = e; if (e != hipSuccess) (void)hipGetLastError(); return e == hipSuccess; }
    bool dev_alloc(void **p, size_t bytes) { return ok(hipMalloc(p, bytes)); }
    bool dev_free(void *p) { return ok(hipFree(p)); }
    bool dev_copy(void *dst, const void *src, size_t bytes) { return ok(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice)); }
    bool host_alloc(void **p, size_t bytes) { return ok(hipHostMalloc(p, bytes, hipHostMallocDefault)); }
    bool host_free(void *p) { return ok(hipHostFree(p)); }
    bool host_device_ptr(void **dp, void *hp) { return ok(hipHostGetDevicePointer(dp, hp, 0)); }
};
// scratch of one call: a DevMem on the stack, its buffers, then this — it goes first and takes their memory with it on every return path
struct ReleaseOnReturn { DevMem &m; ~ReleaseOnReturn() { HipAlloc a; devmem_release(a, m); } };

// what a refused or failed growth answers (`why`: the refused allocation's words)
int mem_fail(dspi_ctx *c, Mem m, const HipAlloc &a, const std::string &why) {
    if (m == Mem::AllocFailed) return fail(c, DSPI_E_NOMEM, why);
    return fail(c, DSPI_E_HIP, std::string(m == Mem::FreeFailed ? "hipFree(ptr): " : m == Mem::CopyFailed ? "hipMemcpy: " : "hipHostGetDevicePointer: ") + hipGetErrorString(a.last));
}
// device buffer b holds at least `bytes` (devmem_grow: contents are not kept)
int ensure(dspi_ctx *c, MemNode &b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    HipAlloc a;
    const Mem m = devmem_grow(a, b, bytes);
    return m == Mem::Ok ? 0 : mem_fail(c, m, a, "hipMalloc failed (" + std::to_string(bytes) + " bytes)");
}
// a pinned host area (h_move, h_mig) of at least `bytes`: one that is too small is replaced by one of `grow` bytes
int pinned_area(dspi_ctx *c, MemNode &area, size_t bytes, size_t grow, const char *why) {
    if (bytes <= area.cap) return 0;
    HipAlloc a;
    const Mem m = devmem_grow_pinned(a, area, bytes, grow, false);
    return m == Mem::Ok ? 0 : mem_fail(c, m, a, why);
}
// array k of the persistent per-stream arrays (dspi_devmem.h kPersist), every row of the capacity, where the context does not have it yet
int persist_alloc(dspi_ctx *c, int k, const char *why) {
    size_t b = 0;
    HipAlloc a;
    if (c->persist[k]->p) return 0;
    return persist_bytes(k, c->sm, c->cap_wg, &b) && devmem_grow(a, *c->persist[k], b) == Mem::Ok ? 0 : fail(c, DSPI_E_NOMEM, why);
}

// One call's words (`parts`, back to back) into device buffer dst, behind the context's earlier work: through the pinned area h_move and on
// the context's stream, so behind every launch that reads dst's old contents; ev_move says when the area may be rewritten.
int upload_via_move_area(dspi_ctx *c, MemNode &dst, const char *why, std::initializer_list<std::pair<const void *, size_t>> parts) {
    size_t bytes = 0, at = 0;
    for (const auto &p : parts) bytes += p.second;
    if (!c->ev_move) HIPCK(c, hipEventCreateWithFlags(&c->ev_move, hipEventDisableTiming));
    HIPCK(c, hipEventSynchronize(c->ev_move));      // the previous call's copy has left the area (long since, as a rule)
    int rc = pinned_area(c, c->h_move, bytes, bytes * 2, why);
    if (rc || (rc = ensure(c, dst, bytes))) return rc;
    for (const auto &p : parts) { if (p.second) memcpy(c->h_move + at, p.first, p.second); at += p.second; }
    HIPCK(c, hipMemcpyAsync(dst.p, c->h_move, bytes, hipMemcpyHostToDevice, c->hs));
    HIPCK(c, hipEventRecord(c->ev_move, c->hs));
    return 0;
}

// the device's activity bitmap as the host has it.  Behind a synchronisation (no kernel may still be reading the words): pauses are rare.
int upload_activity(dspi_ctx *c) {
    if (!c->active_dirty) return 0;
    std::vector<uint32_t> bits(((size_t)c->n_streams + 31) / 32, 0u);
    for (uint32_t s = 0; s < c->n_streams; s++) if (c->active[s]) bits[s >> 5] |= 1u << (s & 31u);
    int rc = ensure(c, c->d_active, bits.size() * 4);
    if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->hs));
    HIPCK(c, hipMemcpy(c->d_active, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
    c->active_dirty = false;
    return 0;
}
// The host-buffer paths hand back zeros in the paused streams' regions, which no kernel writes: the regions to clear, as runs of paused
// streams.  Empty = "clear the whole buffers" (more than kMaxPausedRuns runs: one large clear beats thousands of small ones).
constexpr size_t kMaxPausedRuns = 64;
const std::vector<std::pair<uint32_t, uint32_t>> &paused_runs(dspi_ctx *c) {
    if (c->paused_runs_dirty) {
        c->paused_runs.clear();
        for (uint32_t s = 0; s < c->n_streams && c->paused_runs.size() <= kMaxPausedRuns;) {
            if (c->active[s]) { s++; continue; }
            uint32_t e = s;
            while (e < c->n_streams && !c->active[e]) e++;
            c->paused_runs.emplace_back(s, e);
            s = e;
        }
        if (c->paused_runs.size() > kMaxPausedRuns) c->paused_runs.clear();
        c->paused_runs_dirty = false;
    }
    return c->paused_runs;
}
// the pieces of one buffer of a call that hold the streams of `runs` ([first, end), ascending): f(offset, bytes).  Tiled words: the whole
// tiles that hold one.
template <class F>
void for_run_regions(dspi_ctx *c, const CallBuffer &b, const std::vector<std::pair<uint32_t, uint32_t>> &runs, F f) {
    const size_t row = (size_t)c->sm.row;
    size_t done = 0;      // (tiles: runs in one tile are cleared once)
    for (const auto &r : runs) {
        size_t lo = r.first, hi = r.second;
        if (b.tile_cols) { lo = lo / row * row; hi = (hi + row - 1) / row * row; }
        lo = std::max(lo, done);
        if (hi > lo) f(lo * b.per, (hi - lo) * b.per);
        done = std::max(done, hi);
    }
}
// ... that hold paused streams
template <class F>
void for_paused_regions(dspi_ctx *c, const CallBuffer &b, F f) {
    if (!b.bytes) return;
    const auto &runs = paused_runs(c);
    if (runs.empty()) { f((size_t)0, b.bytes); return; }
    for_run_regions(c, b, runs, f);
}
// ... the tile of the tiled wire words (dspi_wire.h) that holds the columns behind the context's last stream — nothing, when the last tile
// is full.  The tiled wire encoder writes no word there, so the host-buffer paths clear that tile ahead of the launches, as they clear
// the paused streams' tiles: the ONE place where those columns become zeros.
template <class F>
void for_absent_columns(dspi_ctx *c, const CallBuffer &b, F f) {
    const size_t row = (size_t)c->sm.row;
    if (b.bytes && b.tile_cols && c->n_streams % row) f((size_t)(c->n_wg - 1) * row * b.per, row * b.per);
}
// ... of the PDM words that hold streams a dspi_process_pdm call does not list (nothing, while every stream is listed)
template <class F>
void for_unlisted_regions(dspi_ctx *c, const CallBuffer &b, const PdmWork &w, F f) {
    if (!b.bytes || w.unlisted.empty()) return;
    if (w.unlisted.size() > kMaxPausedRuns) { f((size_t)0, b.bytes); return; }
    for_run_regions(c, b, w.unlisted, f);
}
// what the kernels get: null while nothing is paused (they then do what they always did)
const uint32_t *activity(const dspi_ctx *c) { return c->n_paused ? c->d_active : nullptr; }
// who is paused, for the modules that keep per-stream books (dspi_move.h, dspi_boot.h, dspi_spdifpos.h); null: every slot is active
const uint8_t *host_activity(const dspi_ctx *c) { return c->n_paused ? c->active.data() : nullptr; }
// The books of the paused streams: set_active writes a slot's byte (`active` is allocated by the first pause) and keeps n_paused; after a
// call that changed one, activity_changed: the lists are rebuilt and the bitmap goes up at the next commit, the paused runs are found again.
void set_active(dspi_ctx *c, uint32_t s, bool on) {
    if ((c->active[s] != 0) == on) return;
    c->active[s] = on ? 1 : 0;
    if (on) c->n_paused--; else c->n_paused++;
}
void activity_changed(dspi_ctx *c) { c->launch_dirty = true; c->active_dirty = true; c->paused_runs_dirty = true; c->pdm_life.mark_dirty(); }
// the four per-stream arrays, for the launchers that address all of them (d_pdm: null until pdm_state has run)
StateArrays state_arrays(const dspi_ctx *c) { return StateArrays{c->d_state, c->d_dlines, c->d_ring, c->d_pdm}; }

// per-stream S/PDIF positions: the device's copy of the words as the host has them.  Like upload_activity, behind a synchronisation (no
// encoder may still be reading the words), and only after a call that changed one: sets, pauses, resumes, moves and boots are rare.
int upload_spdif_pos(dspi_ctx *c) {
    if (!c->spdif_ps.dirty && c->d_spdif_ps) return 0;
    int rc = ensure(c, c->d_spdif_ps, (size_t)c->n_streams * 4);
    if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->hs));
    HIPCK(c, hipMemcpy(c->d_spdif_ps, c->spdif_ps.word.data(), (size_t)c->n_streams * 4, hipMemcpyHostToDevice));
    c->spdif_ps.dirty = false;
    return 0;
}

int rebuild_assignment(dspi_ctx *c) {
    const size_t ni = c->images.size();
    c->image_rows = image_rows(c->flavor, (uint32_t)c->sm.row, c->stream_image.data(), c->n_streams, ni);
    c->image_rows_offset.assign(ni, 0);
    size_t total = 0;
    for (size_t i = 0; i < ni; i++) { c->image_rows_offset[i] = (uint32_t)total; total += c->image_rows[i].size(); }
    int rc = ensure(c, c->d_items, total * sizeof(WgItem));
    if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->hs));      // no state_ops launch may still be reading the list
    {   // one upload (per-stream presets: tens of thousands of one-item lists)
        std::vector<WgItem> all;
        all.reserve(total);
        for (const auto &v : c->image_rows) all.insert(all.end(), v.begin(), v.end());
        if (!all.empty()) HIPCK(c, hipMemcpy(c->d_items, all.data(), all.size() * sizeof(WgItem), hipMemcpyHostToDevice));
    }
    c->assignment_dirty = false;
    c->launch_dirty = true;
    c->pdm_life.mark_dirty();      // (which object a stream's "sub on" is read from)
    return 0;
}

int rebuild_launch_lists(dspi_ctx *c) {
    PlanInput &in = c->plan_in;
    in.flavor = c->flavor; in.n_streams = c->n_streams; in.row = (uint32_t)c->sm.row;
    in.stream_image = c->stream_image; in.refs = c->image_refs;
    if (c->n_paused) in.active = c->active; else in.active.clear();      // (nothing paused: the plan of a context that never paused, item for item)
    int cus = 0;
    if (c->device < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) cus = 256;
    in.cus = (uint32_t)cus;
    const char *layout = getenv("DSPI_F32_LAYOUT"), *paired = getenv("DSPI_SKEW_PAIRED");
    in.layout = layout && !strcmp(layout, "skew") ? F32Layout::Skew : layout && !strcmp(layout, "packed") ? F32Layout::Packed : F32Layout::Auto;
    in.paired = !(paired && !strcmp(paired, "0"));
    // the word-by-word check of "identical filters": the rows come image after image, the row's first image is built once per run
    std::unique_ptr<DevImage> ref(new DevImage), cur(new DevImage);
    uint32_t ref_image = 0xffffffffu;
    in.same_filters = [&](uint32_t a, uint32_t b) {
        if (ref_image != a) { c->images[a]->build_image(*ref); ref_image = a; }
        c->images[b]->build_image(*cur);
        return memcmp(ref->eq, cur->eq, sizeof ref->eq) == 0 && memcmp(ref->loud, cur->loud, sizeof ref->loud) == 0;
    };
    c->plan = plan_launches(in);
    in.same_filters = nullptr;
    int rc = ensure(c, c->d_litems, c->plan.total * sizeof(WgItem));
    if (rc) return rc;
    if ((rc = ensure(c, c->d_stream_image, (size_t)c->n_streams * 4))) return rc;
    HIPCK(c, hipStreamSynchronize(c->hs));      // no launch may still be reading the lists we overwrite
    for (int p = 0; p < kNumPaths; p++)
        if (!c->plan.items[p].empty())
            HIPCK(c, hipMemcpy(c->d_litems + c->plan.offset[p], c->plan.items[p].data(), c->plan.items[p].size() * sizeof(WgItem), hipMemcpyHostToDevice));
    HIPCK(c, hipMemcpy(c->d_stream_image, c->stream_image.data(), (size_t)c->n_streams * 4, hipMemcpyHostToDevice));
    // every per-lane-value row gets its tile rebuilt (commit_params)
    for (size_t i = 0; i < c->image_touched.size(); i++) c->image_touched[i] = 1;
    c->launch_dirty = false;
    return 0;
}

bool ops_pending(const StateOps &o) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&o);
    for (size_t i = 0; i < sizeof(StateOps) / 4; i++) if (w[i]) return true;
    return false;
}

// upload dirty images and run pending state mutations; everything is ordered on c->hs
int commit_params(dspi_ctx *c) {
    if (c->merge_hint) merge_images(c);
    if (c->assignment_dirty) { int rc = rebuild_assignment(c); if (rc) return rc; }
    const size_t ni = c->images.size();
    bool any_dirty = false;
    for (size_t i = 0; i < ni; i++) if (c->images[i]->dirty) any_dirty = true;
    if (any_dirty || ni * sizeof(DevImage) > c->d_images.cap) HIPCK(c, hipStreamSynchronize(c->hs));   // no launch may still be reading an image we overwrite
    if (ni * sizeof(DevImage) > c->d_images.cap) {      // the table grows with its images in it (a refusal leaves it as it was)
        HipAlloc a;
        const Mem m = devmem_grow_keep(a, c->d_images, (ni + 8) * sizeof(DevImage));
        if (m != Mem::Ok) return mem_fail(c, m, a, "hipMalloc failed (" + std::to_string((ni + 8) * sizeof(DevImage)) + " bytes)");
        for (auto &p : c->images) p->dirty = true;
    }
    // dirty images go up in contiguous runs (per-stream presets dirty thousands at once)
    if (c->image_flags.size() < ni) c->image_flags.resize(ni, 0u);
    if (c->image_core1.size() < ni) c->image_core1.resize(ni, -1);
    if (c->flavor && c->plan_in.sig.size() < ni) {
        ImageSig none; memset(&none, 0xff, sizeof none);
        c->plan_in.sig.resize(ni, none); c->plan_in.bands.resize(ni, BandHash{0, 0}); c->image_touched.resize(ni, 1); c->launch_dirty = true;
    }
    // a run of dirty images: built on all host threads when it is long (every stream its own preset: tens of thousands at once),
    // compared with what the launch lists were built from, uploaded with one copy
    std::vector<DevImage> run;
    std::vector<ImageSig> run_sig;
    std::vector<BandHash> run_bands;
    for (size_t i = 0; i < ni;) {
        if (!c->images[i]->dirty) { i++; continue; }
        size_t j = i;
        while (j < ni && c->images[j]->dirty) j++;
        const size_t n = j - i;
        run.resize(n);
        if (c->flavor) { run_sig.resize(n); run_bands.resize(n); }
        const unsigned csr = _mm_getcsr();      // the workers round and flush exactly like the calling thread
        auto build = [&](size_t k0, size_t k1) {
            _mm_setcsr(csr);
            for (size_t k = k0; k < k1; k++) {
                c->images[i + k]->build_image(run[k]);
                if (c->flavor) { run_sig[k] = make_sig(run[k]); run_bands[k] = hash_bands(run[k]); }
            }
        };
        const size_t nt = n >= 512 ? std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), std::min<size_t>(32, n / 128)) : 1;
        if (nt > 1) {
            std::vector<std::thread> th;
            for (size_t t = 0; t < nt; t++) th.emplace_back(build, n * t / nt, n * (t + 1) / nt);
            for (auto &x : th) x.join();
        } else build(0, n);
        for (size_t k = 0; k < n; k++) {
            const size_t ii = i + k;
            if ((c->image_flags[ii] ^ run[k].flags) & IF_LEVELLER_ON) c->launch_dirty = true;
            c->image_flags[ii] = run[k].flags;
            if (c->image_core1[ii] != (int8_t)c->images[ii]->core1_mode) { c->image_core1[ii] = (int8_t)c->images[ii]->core1_mode; c->pdm_life.mark_dirty(); }
            for (const float al : {run[k].lv_alpha_attack, run[k].lv_alpha_release}) {
                uint32_t bits; memcpy(&bits, &al, 4);
                if (std::find(c->lv_alphas.begin(), c->lv_alphas.end(), bits) == c->lv_alphas.end()) c->lv_alphas.push_back(bits);
            }
            if (c->flavor) {
                if (memcmp(&run_sig[k], &c->plan_in.sig[ii], sizeof(ImageSig)) != 0) { c->plan_in.sig[ii] = run_sig[k]; c->launch_dirty = true; }
                if (run_bands[k].a != c->plan_in.bands[ii].a || run_bands[k].b != c->plan_in.bands[ii].b) { c->plan_in.bands[ii] = run_bands[k]; c->launch_dirty = true; }
                c->image_touched[ii] = 1;
            }
            c->images[ii]->dirty = false;
        }
        HIPCK(c, hipMemcpy(c->d_images + i, run.data(), n * sizeof(DevImage), hipMemcpyHostToDevice));
        i = j;
    }
    // pending state mutations: consecutive images with the same mutation share one launch (their workgroup items are
    // consecutive in d_items)
    for (size_t i = 0; i < ni;) {
        Params &p = *c->images[i];
        if (!ops_pending(p.ops)) { i++; continue; }
        size_t j = i + 1;
        while (j < ni && memcmp(&c->images[j]->ops, &p.ops, sizeof(StateOps)) == 0) j++;
        const uint32_t first = c->image_rows_offset[i];
        const uint32_t count = (uint32_t)((j < ni ? c->image_rows_offset[j] : c->image_rows_offset[ni - 1] + (uint32_t)c->image_rows[ni - 1].size()) - first);
        if (count)
            HIPCK(c, launch_state_ops(c->flavor, c->d_items + first, count, p.ops, c->d_state, c->d_dlines, c->d_ring, c->n_streams, c->hs));
        for (size_t k = i; k < j; k++) c->images[k]->ops = StateOps{};
        i = j;
    }
    if (c->n_paused) { int rc = upload_activity(c); if (rc) return rc; }
    if (c->launch_dirty) { int rc = rebuild_launch_lists(c); if (rc) return rc; }
    if (c->flavor) {       // value tiles of the per-lane-value rows that hold an image uploaded above
        std::vector<uint32_t> rows;
        std::vector<uint8_t> seen(c->n_wg, 0);
        for (size_t i = 0; i < ni; i++) {
            if (!c->image_touched[i]) continue;
            c->image_touched[i] = 0;
            for (const WgItem &it : c->image_rows[i])
                if (c->plan.row_pv[it.wg] && !seen[it.wg]) { seen[it.wg] = 1; rows.push_back(it.wg); }
        }
        if (!rows.empty()) {
            int rc = ensure(c, c->d_vals, (size_t)c->n_wg * kPvTileFloats * sizeof(float));
            if (rc) return rc;
            if ((rc = ensure(c, c->d_pv_rows, (size_t)c->n_wg * 4))) return rc;
            HIPCK(c, hipStreamSynchronize(c->hs));      // no launch may still be reading the tiles or the row list
            HIPCK(c, hipMemcpy(c->d_pv_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
            static const bool all_differ = getenv("DSPI_DEBUG") && (strtoul(getenv("DSPI_DEBUG"), nullptr, 0) & 1u);      // development switch (timing of the worst case)
            HIPCK(c, launch_pv_build(c->d_images, c->d_stream_image, c->d_pv_rows, (uint32_t)rows.size(), c->d_vals, c->n_streams, all_differ, activity(c), c->hs));
        }
    }
    return 0;
}

int read_stream_words(dspi_ctx *c, uint32_t stream, int slot0, int count, uint32_t *out) {
    const uint32_t row = (uint32_t)c->sm.row, wg = stream / row, col = stream % row;
    const uint32_t *src = c->d_state + ((size_t)wg * c->sm.n_slots + slot0) * row + col;
    HIPCK(c, hipSetDevice(c->device));            // several contexts on different GPUs may share the process
    HIPCK(c, hipStreamSynchronize(c->hs));
    HIPCK(c, hipMemcpy2D(out, 4, src, (size_t)row * 4, 4, (size_t)count, hipMemcpyDeviceToHost));
    return 0;
}

int fetch_status(dspi_ctx *c, int32_t stream, uint16_t *peaks, uint16_t *clip) {
    for (int i = 0; i < kMaxCh; i++) peaks[i] = 0;
    *clip = 0;
    if (c->device == DSPI_DEVICE_NONE) return 0;
    const uint32_t s = stream == DSPI_ALL_STREAMS ? 0u : (uint32_t)stream;
    uint32_t w[kMaxCh + 4];
    int rc = read_stream_words(c, s, c->sm.peaks, c->sm.n_ch + 4, w);
    if (rc) return rc;
    for (int i = 0; i < c->sm.n_ch; i++) peaks[i] = (uint16_t)w[i];
    *clip = (uint16_t)(w[c->sm.n_ch] | w[c->sm.n_ch + 1] | w[c->sm.n_ch + 2] | w[c->sm.n_ch + 3]);
    return 0;
}

int zero_clips(dspi_ctx *c, int32_t stream) {
    if (c->device == DSPI_DEVICE_NONE) return 0;
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipStreamSynchronize(c->hs));
    const size_t row = (size_t)c->sm.row, pitch = (size_t)c->sm.n_slots * row * 4;
    if (stream == DSPI_ALL_STREAMS) {
        HIPCK(c, hipMemset2D(c->d_state + (size_t)c->sm.clip * row, pitch, 0, 4 * row * 4, c->n_wg));
    } else {
        const uint32_t wg = (uint32_t)stream / (uint32_t)row, col = (uint32_t)stream % (uint32_t)row;
        uint32_t z[4] = {0, 0, 0, 0};
        HIPCK(c, hipMemcpy2D(c->d_state + ((size_t)wg * c->sm.n_slots + c->sm.clip) * row + col, row * 4, z, 4, 4, 4, hipMemcpyHostToDevice));
    }
    return 0;
}

}  // namespace

extern "C" {

int dspi_abi_version(void) { return DSPI_ABI_VERSION; }

int dspi_create(dspi_ctx **out, int flavor, uint32_t n_streams, int hip_device) {
    const bool fma = (flavor & DSPI_FLOAT_CONTRACT_FMA) != 0, populated = (flavor & DSPI_BOOT_POPULATED_FLASH) != 0;
    flavor &= ~(DSPI_FLOAT_CONTRACT_FMA | DSPI_BOOT_POPULATED_FLASH);
    if (!out || (flavor != DSPI_FLAVOR_RP2040_Q28 && flavor != DSPI_FLAVOR_RP2350_F32) || n_streams == 0) return DSPI_E_INVAL;
    if (fma && flavor != DSPI_FLAVOR_RP2350_F32) return DSPI_E_INVAL;      // the RP2040 has no FPU: nothing to contract
    dspi_ctx *c = new (std::nothrow) dspi_ctx();
    if (!c) return DSPI_E_NOMEM;
    c->flavor = flavor;
    c->n_streams = n_streams;
    c->device = hip_device;
    c->sm = make_state_map(flavor);
    c->n_wg = (n_streams + (uint32_t)c->sm.row - 1) / (uint32_t)c->sm.row;
    c->cap_wg = c->n_wg;
    c->fma = fma;
    c->populated = populated;
    c->no_direct = getenv("DSPI_NO_DIRECT") != nullptr;
    c->no_emit_lines = getenv("DSPI_NO_EMIT_LINES") != nullptr;
    if (const char *e = getenv("DSPI_DIRECT_SPIN_US")) { const long v = atol(e); if (v > 0) c->direct_spin_us = (uint32_t)std::min<long>(v, 1000000L); }
    if (const char *e = getenv("DSPI_MOVE_BATCH")) { const long v = atol(e); if (v > 0) c->move_batch = (uint32_t)std::min<long>(std::max<long>(v, 2L), 65535L); }
    if (const char *e = getenv("DSPI_MIGRATE_VIA")) c->migrate_via = !strcmp(e, "copy") ? dspi_ctx::kViaCopy : !strcmp(e, "host") ? dspi_ctx::kViaHost : dspi_ctx::kViaAuto;
    c->images.push_back(std::make_unique<Params>(flavor, fma, !populated));
    c->image_refs.push_back(n_streams);
    c->stream_image.assign(n_streams, 0);
    c->pdm_life.create(n_streams);
    c->pdm_fade.create(n_streams);
    *out = c;
    if (hip_device == DSPI_DEVICE_NONE) return DSPI_OK;

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { *out = nullptr; delete c; return DSPI_E_NODEVICE; }
    auto bail = [&](int code) { dspi_destroy(c); *out = nullptr; return code; };
    if (hipSetDevice(hip_device) != hipSuccess) return bail(DSPI_E_NODEVICE);
    if (hipStreamCreateWithFlags(&c->hs, hipStreamNonBlocking) != hipSuccess) return bail(DSPI_E_HIP);
    for (int k = 0; k < kNumPersist; k++)
        if (kPersist[k].at_create && persist_alloc(c, k, "hipMalloc failed (per-stream arrays)")) return bail(DSPI_E_NOMEM);
    for (int k = 0; k < kNumPersist; k++)
        if (kPersist[k].at_create && hipMemsetAsync(c->persist[k]->p, 0, c->persist[k]->cap, c->hs) != hipSuccess) return bail(DSPI_E_HIP);
    if (launch_state_init(flavor, c->d_state, c->n_wg, c->hs) != hipSuccess || hipStreamSynchronize(c->hs) != hipSuccess) return bail(DSPI_E_HIP);
    return DSPI_OK;
}

void dspi_destroy(dspi_ctx *c) {
    if (!c) return;
    if (c->device != DSPI_DEVICE_NONE) {
        (void)hipSetDevice(c->device);
        if (c->hs) (void)hipStreamSynchronize(c->hs);
        HipAlloc a;
        devmem_release(a, c->mem);      // every buffer and pinned area, here: with the context's device current and its streams still alive
        if (c->ev_move) (void)hipEventDestroy(c->ev_move);
        if (c->ev_mig) (void)hipEventDestroy(c->ev_mig);
        if (c->ev_link) (void)hipEventDestroy(c->ev_link);
        for (hipEvent_t e : c->pipe_events) (void)hipEventDestroy(e);
        if (c->hs_in) (void)hipStreamDestroy(c->hs_in);
        if (c->hs_out) (void)hipStreamDestroy(c->hs_out);
        if (c->hs) (void)hipStreamDestroy(c->hs);
    }
    delete c;
}

const char *dspi_last_error(const dspi_ctx *c) { return c ? c->err.c_str() : "null context"; }
int dspi_num_channels(const dspi_ctx *c) { return c ? c->sm.n_ch : DSPI_E_INVAL; }
int dspi_num_outputs(const dspi_ctx *c) { return c ? c->sm.n_out : DSPI_E_INVAL; }
int dspi_num_pairs(const dspi_ctx *c) { return c ? c->sm.n_pairs : DSPI_E_INVAL; }
uint32_t dspi_num_streams(const dspi_ctx *c) { return c ? c->n_streams : 0; }
uint32_t dspi_tile_streams(const dspi_ctx *c) { return c ? (uint32_t)c->sm.row : 0; }
void *dspi_hip_stream(dspi_ctx *c) { return c ? (void *)c->hs : nullptr; }

int dspi_factory_defaults(dspi_ctx *c, int32_t stream) {
    return for_targets(c, stream, [](Params &p) { p.factory_reset(); return 0; });
}
int dspi_load_bulk(dspi_ctx *c, int32_t stream, const void *blob, size_t len) {
    if (!blob) return DSPI_E_INVAL;
    return for_targets(c, stream, [&](Params &p) { return p.load_bulk(blob, len); });
}
int dspi_collect_bulk(dspi_ctx *c, int32_t stream, void *blob, size_t cap) {
    if (!c || !blob || !valid_stream(c, stream)) return DSPI_E_INVAL;
    return readable(c, stream).collect_bulk(blob, cap);
}
int dspi_load_preset_slot(dspi_ctx *c, int32_t stream, const void *image, size_t len, int expect_slot) {
    if (!image) return DSPI_E_INVAL;
    return for_targets(c, stream, [&](Params &p) { return p.load_slot(image, len, expect_slot); });
}
int dspi_load_flash_dump(dspi_ctx *c, int32_t stream, const void *dump, size_t len) {
    if (!dump) return DSPI_E_INVAL;
    if (len < kFlashDumpBytes) return DSPI_E_SHORT;
    // A context of devices with a populated flash (DSPI_BOOT_POPULATED_FLASH) that has not processed audio yet BOOTS from the dump
    // (preset_boot_load -> apply_slot_to_live, flash_storage.c:1047-1082: no mute, no line zeroing): exact against the firmware from
    // frame 0.  Every other context is a running device that switches to the preset the dump selects (preset_load, :794-849).
    const bool as_boot = c->populated && !c->audio_started;
    const int rc = for_targets(c, stream, [&](Params &p) { return p.load_flash_dump(dump, len, as_boot); });
    // dspi_device_flash: the dump becomes the streams' flash (one shared object), with the writes of a boot over it (dspi_flash.h boot_writes)
    if (c && c->flash.on && valid_stream(c, stream)) {
        auto f = std::make_unique<Flash>();
        f->set_bytes(dump);
        f->boot_writes(c->flavor);
        const int32_t obj = c->flash.add(std::move(f));
        const uint32_t s0 = stream == DSPI_ALL_STREAMS ? 0u : (uint32_t)stream, n = stream == DSPI_ALL_STREAMS ? c->n_streams : 1u;
        for (uint32_t s = s0; s < s0 + n; s++) c->flash.assign(s, obj);
        flash_resync(c, s0, n);
    }
    return rc;
}
int dspi_flash_read_directory(const void *dump, size_t len, dspi_flash_dir *out) {
    if (!dump || !out) return DSPI_E_INVAL;
    FlashDirectory d;
    parse_flash_directory(dump, len, d);
    memset(out, 0, sizeof *out);
    out->valid = d.valid; out->version = d.version;
    out->startup_mode = d.startup_mode; out->default_slot = d.default_slot; out->last_active_slot = d.last_active_slot; out->include_pins = d.include_pins;
    out->slot_occupied = d.slot_occupied; out->master_volume_mode = d.master_volume_mode; out->master_volume_db = d.master_volume_db;
    memcpy(out->slot_names, d.slot_names, sizeof out->slot_names);
    return DSPI_OK;
}
int dspi_save_preset_slot(dspi_ctx *c, int32_t stream, void *image, size_t cap, int slot_index) {
    if (!c || !image || !valid_stream(c, stream)) return DSPI_E_INVAL;
    return readable(c, stream).save_slot(image, cap, slot_index);
}
int dspi_vendor_set(dspi_ctx *c, int32_t stream, uint8_t req, uint16_t wValue, const void *payload, uint16_t len) {
    if (len && !payload) return DSPI_E_INVAL;
    if (c && c->flash.on && flash_request_out(req)) {      // dspi_device_flash: the directory's setters write the stream's own flash
        if (!valid_stream(c, stream)) return fail(c, DSPI_E_INVAL, "stream index out of range");
        return for_flash_targets(c, stream, [&](Params &p, Flash &f) { return flash_vendor_set(f, p, req, wValue, payload, len); });
    }
    return for_targets(c, stream, [&](Params &p) { return p.vendor_set(req, wValue, payload, len); });
}
int dspi_vendor_get(dspi_ctx *c, int32_t stream, uint8_t req, uint16_t wValue, void *buf, uint16_t cap) {
    if (!c || !buf || !valid_stream(c, stream)) return DSPI_E_INVAL;
    if (c->flash.on && flash_request_in(req)) {      // dspi_device_flash: the preset directory, served from the stream's own flash
        if (!flash_request_writes(req)) return flash_vendor_read(c->flash.readable(stream == DSPI_ALL_STREAMS ? 0u : (uint32_t)stream), req, wValue, buf, cap);
        if (cap < 1) return DSPI_E_SHORT;
        return for_flash_targets(c, stream, [&](Params &p, Flash &f) { return flash_vendor_get(f, p, req, wValue, buf, cap); });
    }
    uint16_t peaks[kMaxCh], clip = 0;
    const bool needs_status = (req == 0x50 || req == 0x83);
    if (needs_status) { int rc = fetch_status(c, stream, peaks, &clip); if (rc) return rc; }
    const uint16_t before = clip;
    int n;
    if (req == 0x53) {   // REQ_FACTORY_RESET answers with a status byte and mutates state
        int rc = dspi_factory_defaults(c, stream);
        if (rc) return rc;
        if (cap < 1) return DSPI_E_SHORT;
        *(uint8_t *)buf = 0;
        return 1;
    }
    if (req == 0xC0) {   // REQ_SET_OUTPUT_TYPE: answered from a copy unless it really changes a slot's type (no clone, no mute for a no-op or a refusal)
        if (cap < 1) return DSPI_E_SHORT;
        const uint8_t slot = wValue & 0xFF, type = (wValue >> 8) & 0xFF;
        bool changes = false;
        for (size_t i = 0; i < c->images.size() && !changes; i++) {
            if (stream == DSPI_ALL_STREAMS ? c->image_refs[i] == 0 : (size_t)c->stream_image[(size_t)stream] != i) continue;
            const Params &r = *c->images[i];
            changes = slot < r.n_pairs && type <= 1 && type != r.output_types[slot];
        }
        if (!changes) { Params view = readable(c, stream); return view.vendor_get(req, wValue, buf, cap, peaks, &clip); }
    }
    if (req == 0xD6 || req == 0xC0) {   // REQ_SAVE_MASTER_VOLUME mutates the directory copy, REQ_SET_OUTPUT_TYPE the slot type (+ pipeline mute)
        return for_targets(c, stream, [&](Params &p) { int r = p.vendor_get(req, wValue, buf, cap, peaks, &clip); return r < 0 ? r : 0; }) == 0 ? 1 : DSPI_E_SHORT;
    }
    Params tmp_view = readable(c, stream);    // GETs never change parameters; work on a copy
    n = tmp_view.vendor_get(req, wValue, buf, cap, peaks, &clip);
    // REQ_CLEAR_CLIPS: with DSPI_ALL_STREAMS the answer carries stream 0's flags (one device answers one request), but every
    // stream's sticky bits are cleared whatever stream 0 held
    if (req == 0x83 && n >= 0 && (before != 0 || stream == DSPI_ALL_STREAMS)) { int rc = zero_clips(c, stream); if (rc) return rc; }
    return n;
}
int dspi_set_host_volume(dspi_ctx *c, int32_t stream, int16_t v) {
    return for_targets(c, stream, [&](Params &p) { p.set_volume(v); return 0; });
}
int dspi_set_mute(dspi_ctx *c, int32_t stream, int mute) {
    return for_targets(c, stream, [&](Params &p) { p.set_mute(mute != 0); return 0; });
}
int dspi_set_sample_rate(dspi_ctx *c, int32_t stream, uint32_t hz) {
    if (hz != 44100 && hz != 48000 && hz != 96000) return DSPI_E_INVAL;
    return for_targets(c, stream, [&](Params &p) { return p.set_rate(hz); });
}

int dspi_get_status(dspi_ctx *c, int32_t stream, void *buf, size_t cap) {
    if (!c || !buf || !valid_stream(c, stream)) return DSPI_E_INVAL;
    const int n = c->sm.n_ch * 2 + 4;
    if (cap < (size_t)n) return DSPI_E_SHORT;
    return dspi_vendor_get(c, stream, 0x50, 9, buf, (uint16_t)n);
}
int dspi_clear_clips(dspi_ctx *c, int32_t stream) {
    if (!c || !valid_stream(c, stream)) return DSPI_E_INVAL;
    uint16_t f = 0;
    int n = dspi_vendor_get(c, stream, 0x83, 0, &f, 2);
    return n < 0 ? n : (int)f;
}

int dspi_debug_image(dspi_ctx *c, int32_t stream, void *buf, size_t cap) {
    if (!c || !buf || !valid_stream(c, stream)) return DSPI_E_INVAL;
    if (cap < sizeof(DevImage)) return DSPI_E_SHORT;
    DevImage img;
    readable(c, stream).build_image(img);
    memcpy(buf, &img, sizeof(img));
    return (int)sizeof(img);
}

int dspi_debug_launch_plan(dspi_ctx *c, uint32_t *counts, size_t n_counts) {
    if (!c || !counts || n_counts < 5) return DSPI_E_INVAL;
    const int n = n_counts >= 8 ? 8 : n_counts >= 7 ? 7 : n_counts >= 6 ? 6 : 5;      // [0..5]: items per PathGroup, [6]: the latency layout's items with paired presets, [7]: DSPI_NO_EMIT_LINES
    uint32_t all[8] = {};
    all[7] = c->no_emit_lines ? 1u : 0u;
    for (const PathInfo &pi : kPaths) {
        const uint32_t k = (uint32_t)c->plan.items[(int)pi.path].size();
        all[(int)pi.group] += k;
        if (pi.paired) all[6] += k;
    }
    for (int k = 0; k < n; k++) counts[k] = all[k];
    return n;
}

int dspi_debug_direct_stats(dspi_ctx *c, uint64_t *out, size_t n) {
    if (!c || !out || n < 5) return DSPI_E_INVAL;
    for (int i = 0; i < 5; i++) out[i] = c->direct_stats[i];
    return 5;
}

int dspi_debug_image_count(dspi_ctx *c) {
    if (!c) return DSPI_E_INVAL;
    if (c->merge_hint) merge_images(c);
    return (int)c->images.size();
}

int dspi_debug_eq_taps(dspi_ctx *c, int32_t stream, int channel, const float *x, uint32_t n, float *taps, float *other) {
    if (!c || !x || !taps || !other || n == 0 || n > (1u << 20) || !valid_stream(c, stream) || stream < 0) return DSPI_E_INVAL;
    if (c->flavor != DSPI_FLAVOR_RP2350_F32 || channel < 0 || channel >= c->sm.n_ch) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    DevImage img;
    readable(c, stream).build_image(img);
    DevMem mem; DevBuf<DevImage> d_img{mem}; DevBuf<float> d_x{mem}, d_t{mem}, d_o{mem}; ReleaseOnReturn scratch{mem};
    HipAlloc a;
    const size_t nb = (size_t)n * sizeof(float);
    if (devmem_grow(a, d_img, sizeof img) != Mem::Ok || devmem_grow(a, d_x, nb) != Mem::Ok || devmem_grow(a, d_t, nb * (kBands + 1)) != Mem::Ok || devmem_grow(a, d_o, nb * kBands) != Mem::Ok)
        return fail(c, DSPI_E_NOMEM, "hipMalloc failed (EQ taps)");
    if (hipMemcpy(d_img, &img, sizeof img, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_x, x, nb, hipMemcpyHostToDevice) != hipSuccess ||
        launch_eq_taps(c->fma, d_img, channel, d_x, n, d_t, d_o, c->hs) != hipSuccess || hipStreamSynchronize(c->hs) != hipSuccess ||
        hipMemcpy(taps, d_t, nb * (kBands + 1), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(other, d_o, nb * kBands, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, DSPI_E_HIP, "EQ taps failed");
    return DSPI_OK;
}

int dspi_debug_detmath(dspi_ctx *c, int which, const float *a, const float *b, uint32_t n, float *out) {
    if (!c || !a || !out || ((which == 1 || which == 4) && !b) || n == 0 || n > (1u << 24) || which < 0 || which > 4) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    DevMem mem; DevBuf<float> d_a{mem}, d_b{mem}, d_o{mem}; ReleaseOnReturn scratch{mem};
    HipAlloc al;
    const size_t nb = (size_t)n * sizeof(float);
    if (devmem_grow(al, d_a, nb) != Mem::Ok || devmem_grow(al, d_b, nb) != Mem::Ok || devmem_grow(al, d_o, nb) != Mem::Ok) return fail(c, DSPI_E_NOMEM, "hipMalloc failed (detmath)");
    if (hipMemcpy(d_a, a, nb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_b, (which == 1 || which == 4) ? b : a, nb, hipMemcpyHostToDevice) != hipSuccess ||
        launch_detmath(which, d_a, d_b, n, d_o, c->hs) != hipSuccess || hipStreamSynchronize(c->hs) != hipSuccess ||
        hipMemcpy(out, d_o, nb, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, DSPI_E_HIP, "detmath kernel failed");
    return DSPI_OK;
}

// ---- PDM sub output: pdm_generator.c:351-397 per sample (dspi_pdm.hip) ----
static int pdm_state(dspi_ctx *c) {
    if (c->d_pdm) return 0;
    if (int rc = persist_alloc(c, kArrPdm, "hipMalloc failed (PDM state)")) return rc;      // (every row of the capacity, like the other arrays)
    HIPCK(c, hipMemsetAsync(c->d_pdm, 0, c->d_pdm.cap, c->hs));
    HIPCK(c, launch_pdm_reset(c->d_pdm, c->n_streams, (uint32_t)c->sm.row, c->n_wg, -1, 1, c->hs));
    return 0;
}

// host buffers of the stand-alone encoders (PDM, S/PDIF, I2S): the words come down from their staging buffer and the call waits for them
// (the way up stays each encoder's own: what goes up besides the input, and what is cleared, differs in every one)
static int stage_down(dspi_ctx *c, void *host, const void *staged, size_t bytes) {
    HIPCK(c, hipMemcpyAsync(host, staged, bytes, hipMemcpyDeviceToHost, c->hs));
    HIPCK(c, hipStreamSynchronize(c->hs));
    return 0;
}

int dspi_pdm_modulate(dspi_ctx *c, const int32_t *sub, uint32_t n_frames, uint32_t *words, uint32_t flags) {
    if (!c || !sub || !words || n_frames == 0) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    int rc = pdm_state(c);
    if (rc) return rc;
    if (c->n_paused && (rc = upload_activity(c))) return rc;
    const bool tiled = flags & DSPI_OUT_TILED, dev = flags & DSPI_MEM_DEVICE;
    const size_t cols = tiled ? (size_t)c->n_wg * c->sm.row : (size_t)c->n_streams;
    const size_t in_b = cols * n_frames * 4, out_b = in_b * 8;
    const int32_t *d_in = sub;
    uint32_t *d_out = words;
    if (!dev) {
        if ((rc = ensure(c, c->d_pdm_in, in_b)) || (rc = ensure(c, c->d_pdm_out, out_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_pdm_in, sub, in_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_pdm_in; d_out = c->d_pdm_out;
        if (c->n_paused) HIPCK(c, hipMemsetAsync(c->d_pdm_out, 0, out_b, c->hs));      // paused streams' words stay unwritten: the staging buffer goes back whole, with zeros there
    }
    HIPCK(c, launch_pdm(tiled, c->d_pdm, d_in, d_out, c->n_streams, n_frames, (uint32_t)c->sm.row, c->n_wg, activity(c), c->hs));
    return dev ? DSPI_OK : stage_down(c, words, c->d_pdm_out, out_b);
}

int dspi_pdm_restart(dspi_ctx *c, int32_t stream) {
    if (!c || !valid_stream(c, stream)) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return DSPI_E_NODEVICE;
    HIPCK(c, hipSetDevice(c->device));
    int rc = pdm_state(c);
    if (rc) return rc;
    HIPCK(c, launch_pdm_reset(c->d_pdm, c->n_streams, (uint32_t)c->sm.row, c->n_wg, stream == DSPI_ALL_STREAMS ? -1 : stream, 0, c->hs));
    return DSPI_OK;
}

// ---- stream snapshots (dspi_snapshot.h: the format; dspi_snapshot.hip: the transposition kernels) ----
static bool snap_range_ok(const dspi_ctx *c, uint32_t first, uint32_t count) { return count != 0 && (uint64_t)first + count <= c->n_streams; }

// the distinct images of streams [first, first + count) — or, `list` given, of its `count` sources — in order of first use, and every
// stream's index into that list
static void snap_images(const dspi_ctx *c, uint32_t first, uint32_t count, std::vector<int32_t> &used, std::vector<uint32_t> *index, const StreamMove *list = nullptr) {
    std::vector<int32_t> slot(c->images.size(), -1);
    if (index) index->resize(count);
    for (uint32_t k = 0; k < count; k++) {
        const int32_t im = c->stream_image[list ? (size_t)list[k].src : (size_t)first + k];
        if (slot[(size_t)im] < 0) { slot[(size_t)im] = (int32_t)used.size(); used.push_back(im); }
        if (index) (*index)[k] = (uint32_t)slot[(size_t)im];
    }
}

static uint32_t snap_chunk_rows(const dspi_ctx *c) { return c->flavor ? 2u : 8u; }
// host buffers go through device memory a chunk of rows at a time: streams [s, snap_chunk_end) end on a row boundary, 25 - 40 MB of records
static uint32_t snap_chunk_end(const dspi_ctx *c, uint32_t s, uint32_t end) {
    const uint32_t row = (uint32_t)c->sm.row, rows = snap_chunk_rows(c);
    return (uint32_t)std::min<uint64_t>(end, ((uint64_t)s / row + rows) * row);
}

// What a call that takes run-time state through the records does first: the context's device, the modulators' words (the records carry
// them out and back in; a context that never ran the modulator hands over its power-on words), scratch for `records` records and, for a
// call that rotates, the shift table — sized for the whole context once: a later, larger call never reallocates it under work in flight.
static int snap_prepare(dspi_ctx *c, size_t records, bool shifts) {
    HIPCK(c, hipSetDevice(c->device));
    int rc = pdm_state(c);
    if (rc || (rc = ensure(c, c->d_snap, records * snap_state_bytes(c->flavor, 1)))) return rc;
    return shifts ? ensure(c, c->d_snap_shift, (size_t)c->n_streams * 8) : 0;
}
// the context's arrays of streams [first, first + count) -> records, on its stream
static hipError_t snap_gather(dspi_ctx *c, uint32_t *records, uint32_t first, uint32_t count) {
    return launch_snapshot(c->flavor, false, state_arrays(c), records, first, count, c->hs);
}
// records -> the context's arrays on its stream, as they are or realigned to their rows (dspi_snapshot.h snap_row_target)
static hipError_t snap_scatter(dspi_ctx *c, bool realign, uint32_t *records, uint32_t first, uint32_t count) {
    if (realign) return launch_snapshot_realign(c->flavor, state_arrays(c), records, first, count, c->n_streams, c->d_snap_shift, c->hs);
    return launch_snapshot(c->flavor, true, state_arrays(c), records, first, count, c->hs);
}

int dspi_snapshot_sizes(const dspi_ctx *c, uint32_t first, uint32_t count, size_t *head_bytes, size_t *state_bytes) {
    if (!c || !snap_range_ok(c, first, count)) return DSPI_E_INVAL;
    std::vector<int32_t> used;
    snap_images(c, first, count, used, nullptr);
    if (head_bytes) *head_bytes = snap_head_bytes(count, (uint32_t)used.size());
    if (state_bytes) *state_bytes = snap_state_bytes(c->flavor, count);
    return DSPI_OK;
}

int dspi_export_streams(dspi_ctx *c, uint32_t first, uint32_t count, const dspi_snapshot *snap, uint32_t flags) {
    if (!c || !snap || !snap->head || !snap->state) return DSPI_E_INVAL;
    if (flags & ~DSPI_MEM_DEVICE) return fail(c, DSPI_E_INVAL, "dspi_export_streams: undefined flag bits");
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_export_streams: stream range out of bounds");
    const bool dev = flags & DSPI_MEM_DEVICE;
    if (dev && (reinterpret_cast<uintptr_t>(snap->state) & 15u)) return fail(c, DSPI_E_INVAL, "dspi_export_streams: device state buffer must be 16-byte aligned");
    std::vector<int32_t> used;
    std::vector<uint32_t> index;
    snap_images(c, first, count, used, &index);
    const size_t hb = snap_head_bytes(count, (uint32_t)used.size()), sb = snap_state_bytes(c->flavor, count);
    if (snap->head_bytes < hb || snap->state_bytes < sb) return fail(c, DSPI_E_SHORT, "dspi_export_streams: buffer too small (dspi_snapshot_sizes)");
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no run-time state to export");
    int rc = snap_prepare(c, 0, false);      // (host buffers: the chunks below size the scratch, each for itself)
    if (rc) return rc;
    // the head: header, the range's distinct parameter objects as they are (pending state operations included), the streams' indices
    unsigned char *const head = static_cast<unsigned char *>(snap->head);
    memset(head, 0, hb);
    const SnapHeader h = snap_make_header(c->flavor, c->fma, count, (uint32_t)used.size(), c->audio_started);
    memcpy(head, &h, sizeof h);
    for (size_t i = 0; i < used.size(); i++) memcpy(head + sizeof h + i * snap_params_stride(), c->images[(size_t)used[i]].get(), sizeof(Params));
    memcpy(head + sizeof h + used.size() * snap_params_stride(), index.data(), (size_t)count * 4);
    snap_seal(head);
    if (dev) {
        HIPCK(c, snap_gather(c, static_cast<uint32_t *>(snap->state), first, count));
        return (int)count;
    }
    const size_t rec = snap_state_bytes(c->flavor, 1);
    for (uint32_t s = first, end = first + count; s < end;) {
        const uint32_t e = snap_chunk_end(c, s, end);
        if ((rc = ensure(c, c->d_snap, (size_t)(e - s) * rec))) return rc;
        HIPCK(c, snap_gather(c, c->d_snap, s, e - s));
        HIPCK(c, hipMemcpyAsync(static_cast<char *>(snap->state) + (size_t)(s - first) * rec, c->d_snap, (size_t)(e - s) * rec, hipMemcpyDeviceToHost, c->hs));
        HIPCK(c, hipStreamSynchronize(c->hs));
        s = e;
    }
    return (int)count;
}

int dspi_import_streams(dspi_ctx *c, uint32_t first, const dspi_snapshot *snap, uint32_t flags) {
    if (!c || !snap || !snap->head || !snap->state) return DSPI_E_INVAL;
    if (flags & ~(DSPI_MEM_DEVICE | DSPI_SNAP_REALIGN)) return fail(c, DSPI_E_INVAL, "dspi_import_streams: undefined flag bits");
    // everything is validated before anything is written
    if (const char *why = snap_validate_head(snap->head, snap->head_bytes, c->flavor, c->fma)) return fail(c, DSPI_E_INVAL, why);
    SnapHeader h;
    memcpy(&h, snap->head, sizeof h);
    const uint32_t count = h.count;
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_import_streams: stream range out of bounds");
    if (snap->state_bytes < snap_state_bytes(c->flavor, count)) return fail(c, DSPI_E_SHORT, "dspi_import_streams: state buffer shorter than the head's stream count");
    const bool dev = flags & DSPI_MEM_DEVICE, realign = flags & DSPI_SNAP_REALIGN;
    if (dev && (reinterpret_cast<uintptr_t>(snap->state) & 15u)) return fail(c, DSPI_E_INVAL, "dspi_import_streams: device state buffer must be 16-byte aligned");
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no run-time state to import into");
    int rc = snap_prepare(c, dev ? 0 : snap_chunk_end(c, first, first + count) - first, realign);
    if (rc) return rc;
    const size_t rec = snap_state_bytes(c->flavor, 1);
    // parameters: the streams leave their images, the imported objects are appended dirty, and the fold-back pass (merge_images, at the
    // next commit) drops what nobody uses any more and folds equal objects — the imported ones among themselves and into images already
    // here.  Tiles, launch plan, alpha list and pending state operations follow from the ordinary commit.
    const size_t base = c->images.size();
    for (uint32_t i = 0; i < h.n_images; i++) {
        auto p = std::make_unique<Params>(*c->images[0]);
        memcpy(static_cast<void *>(p.get()), snap_params(snap->head, i), sizeof(Params));
        add_image(c, std::move(p));
    }
    const unsigned char *idx = snap_params(snap->head, h.n_images);
    for (uint32_t k = 0; k < count; k++) {
        uint32_t im;
        memcpy(&im, idx + (size_t)k * 4, 4);
        assign_image(c, (size_t)first + k, (int32_t)(base + im));
    }
    c->merge_hint = true;
    if (c->flash.on) flash_resync(c, first, count);      // (a snapshot carries no flash: the slots keep theirs, and the arrivals' directory mirrors follow it)
    if (h.flags & kSnapAudioStarted) c->audio_started = true;      // running devices arrived: dspi_load_flash_dump is no boot any more
    // run-time state, behind whatever the context's stream still has to do (a realigning import reads its rows' resident neighbours
    // there, on the device: their positions are what that work leaves)
    if (dev) {
        HIPCK(c, snap_scatter(c, realign, static_cast<uint32_t *>(snap->state), first, count));
        return (int)count;
    }
    for (uint32_t s = first, end = first + count; s < end;) {
        const uint32_t e = snap_chunk_end(c, s, end);
        if ((rc = ensure(c, c->d_snap, (size_t)(e - s) * rec))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_snap, static_cast<const char *>(snap->state) + (size_t)(s - first) * rec, (size_t)(e - s) * rec, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, snap_scatter(c, realign, c->d_snap, s, e - s));      // (chunks end on row boundaries: a row's target is the same in whichever chunk)
        HIPCK(c, hipStreamSynchronize(c->hs));
        s = e;
    }
    return (int)count;
}

int dspi_realign_streams(dspi_ctx *c, uint32_t first, uint32_t count) {
    if (!c) return DSPI_E_INVAL;
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_realign_streams: stream range out of bounds");
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no run-time state to realign");
    // scratch for a full chunk and the whole context's shifts, once, before anything is enqueued: the loop below never reallocates (a
    // hipFree would wait for the device) and the call stays asynchronous
    int rc = snap_prepare(c, (size_t)snap_chunk_rows(c) * (uint32_t)c->sm.row, true);
    if (rc) return rc;
    // run-time state only, chunk by chunk through the records' scratch, all on the context's stream: out as it is, back in rotated.  A
    // chunk holds whole rows of the range, so its rows' targets are those of the whole range.
    for (uint32_t s = first, end = first + count; s < end;) {
        const uint32_t e = snap_chunk_end(c, s, end);
        HIPCK(c, snap_gather(c, c->d_snap, s, e - s));
        HIPCK(c, snap_scatter(c, true, c->d_snap, s, e - s));
        s = e;
    }
    return (int)count;
}

// ---- paused streams: devices that receive no packet in a call (include/dspi.h) ----
int dspi_pause_streams(dspi_ctx *c, uint32_t first, uint32_t count) {
    if (!c) return DSPI_E_INVAL;
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_pause_streams: stream range out of bounds");
    if (c->spdif_ps.on) c->spdif_ps.pause(first, count, host_activity(c));      // (the S/PDIF position freezes; it is never realigned)
    if (c->active.empty()) c->active.assign(c->n_streams, 1);
    const uint32_t before = c->n_paused;
    for (uint32_t s = first; s < first + count; s++) set_active(c, s, false);
    if (c->n_paused != before) activity_changed(c);
    return (int)count;
}

int dspi_resume_streams(dspi_ctx *c, uint32_t first, uint32_t count, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (flags & ~DSPI_RESUME_AS_IS) return fail(c, DSPI_E_INVAL, "dspi_resume_streams: undefined flag bits");
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_resume_streams: stream range out of bounds");
    // the streams this call resumes lie in [lo, hi]; the others of the range are residents
    uint32_t lo = 0, hi = 0, n = 0;
    if (c->n_paused)
        for (uint32_t s = first; s < first + count; s++)
            if (!c->active[s]) { if (!n++) lo = s; hi = s; }
    if (!n) return (int)count;
    if (c->device != DSPI_DEVICE_NONE && !(flags & DSPI_RESUME_AS_IS)) {
        // Their rows went on while they stood still: rotate them onto their rows' positions (dspi_snapshot.h snap_row_target_active), run-time
        // state only, through the records' scratch like dspi_realign_streams — out as it is, back in rotated —, on the context's stream.  The
        // rule reads the bitmap as it stood BEFORE this call: when pauses or resumes were made since the last dspi_process the device's copy
        // is brought up to date first (that upload synchronises; otherwise the call only enqueues).
        // (Scratch for a full chunk, once, before anything is enqueued, as there.)
        int rc = snap_prepare(c, (size_t)snap_chunk_rows(c) * (uint32_t)c->sm.row, true);
        if (rc || (rc = upload_activity(c))) return rc;
        // Only rows that hold a stream to resume go through the scratch: a piece = [s, e) inside one scratch chunk, from the first such
        // stream to the end of the last such row of the chunk (cut at hi); rows between the pieces are not touched.
        const uint32_t row = (uint32_t)c->sm.row;
        for (uint32_t s = lo, end = hi + 1; s < end;) {
            while (s < end && c->active[s]) s++;
            if (s >= end) break;
            const uint32_t ce = snap_chunk_end(c, s, end);
            uint32_t e = s + 1;
            for (uint32_t t = s; t < ce; t++) if (!c->active[t]) e = std::min(ce, (t / row + 1) * row);
            HIPCK(c, snap_gather(c, c->d_snap, s, e - s));
            HIPCK(c, launch_snapshot_realign(c->flavor, state_arrays(c), c->d_snap, s, e - s, c->n_streams, c->d_snap_shift, c->hs, c->d_active, lo, hi - lo + 1));
            s = e;
        }
    }
    if (c->spdif_ps.on) c->spdif_ps.resume(lo, hi - lo + 1, host_activity(c));      // (... and continues from the frozen value)
    for (uint32_t s = lo; s <= hi; s++) set_active(c, s, true);
    activity_changed(c);
    return (int)count;
}

int dspi_streams_paused(const dspi_ctx *c, uint32_t first, uint32_t count, uint8_t *paused) {
    if (!c || !snap_range_ok(c, first, count)) return DSPI_E_INVAL;
    int n = 0;
    for (uint32_t k = 0; k < count; k++) {
        const bool p = c->n_paused && !c->active[(size_t)first + k];
        if (paused) paused[k] = p ? 1 : 0;
        n += p ? 1 : 0;
    }
    return n;
}

// ---- stream moves (dspi_move.h: validation, compaction rule, targets, batch schedule; dspi_snapshot.hip: the list-addressed kernels) ----
static_assert(sizeof(dspi_stream_move) == sizeof(StreamMove) && offsetof(dspi_stream_move, dst) == offsetof(StreamMove, dst), "dspi_stream_move is StreamMove");

static uint32_t move_batch_records(const dspi_ctx *c) { return c->move_batch ? c->move_batch : snap_chunk_rows(c) * (uint32_t)c->sm.row; }

// one call's work lists into device memory, behind the context's earlier work
static int move_upload(dspi_ctx *c, const std::vector<uint32_t> &words) {
    return upload_via_move_area(c, c->d_move, "hipHostMalloc failed (move lists)", {{words.data(), words.size() * 4}});
}

// row items and their columns' record indices, appended to a call's work lists: where they begin, in words
struct PackedItems { size_t items_at, colrec_at; };
static PackedItems pack_row_items(std::vector<uint32_t> &words, const std::vector<MoveRowItem> &items, const std::vector<uint32_t> &colrec) {
    const PackedItems at{words.size(), words.size() + items.size() * 4};
    words.resize(at.colrec_at + colrec.size());
    memcpy(words.data() + at.items_at, items.data(), items.size() * sizeof(MoveRowItem));
    memcpy(words.data() + at.colrec_at, colrec.data(), colrec.size() * 4);
    return at;
}
// ... and a call's targets at their head (four words per entry: what follows stays 16-byte aligned)
static void pack_targets(std::vector<uint32_t> &words, const std::vector<ListTarget> &t) {
    words.resize(t.size() * 4);
    memcpy(words.data(), t.data(), t.size() * sizeof(ListTarget));
}
// a planned list into the caller's buffer (moves == nullptr: its size only)
static int plan_out(const std::vector<StreamMove> &plan, dspi_stream_move *moves, uint32_t cap) {
    if (!moves) return (int)plan.size();
    if (plan.size() > cap) return DSPI_E_SHORT;
    if (!plan.empty()) memcpy(moves, plan.data(), plan.size() * sizeof(StreamMove));
    return (int)plan.size();
}
// a boot list's work items into device memory (move_upload)
// ... and behind them `slots` (dspi_boot_streams in the fade mode: the slots whose fade base becomes 0)
static int boot_upload(dspi_ctx *c, const std::vector<BootRowItem> &items, const uint32_t *slots = nullptr, uint32_t n_slots = 0) {
    std::vector<uint32_t> words(items.size() * (sizeof(BootRowItem) / 4));
    memcpy(words.data(), items.data(), items.size() * sizeof(BootRowItem));
    if (n_slots) words.insert(words.end(), slots, slots + n_slots);
    return move_upload(c, words);
}

int dspi_move_streams(dspi_ctx *c, const dspi_stream_move *moves, uint32_t n, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (flags & ~DSPI_MOVE_AS_IS) return fail(c, DSPI_E_INVAL, "dspi_move_streams: undefined flag bits");
    // everything is validated before anything is written
    const StreamMove *list = reinterpret_cast<const StreamMove *>(moves);
    if (const char *why = move_validate(list, n, c->n_streams, host_activity(c))) return fail(c, DSPI_E_INVAL, std::string("dspi_move_streams: ") + why);
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no run-time state to move");
    std::vector<StreamMove> mv;
    for (uint32_t i = 0; i < n; i++) if (list[i].src != list[i].dst) mv.push_back(list[i]);
    if (mv.empty()) return 0;
    const uint32_t nm = (uint32_t)mv.size(), row = (uint32_t)c->sm.row, cap = move_batch_records(c);
    const bool realign = !(flags & DSPI_MOVE_AS_IS);
    int rc = snap_prepare(c, cap, realign);
    if (rc) return rc;
    // the call's work lists, one upload: the targets (every shift is computed once, by one launch, before anything is written: batches
    // cannot disagree), then per batch the gather's and the scatter's row items and their columns' record indices
    const std::vector<MoveBatch> batches = move_schedule(mv.data(), nm, cap);
    std::vector<uint32_t> words;
    if (realign) {
        std::vector<uint8_t> listed(c->n_streams, 0);      // neither a source nor a destination is a resident
        for (const StreamMove &m : mv) listed[m.src] = listed[m.dst] = 1;
        pack_targets(words, list_targets(mv.data(), nm, c->n_streams, row, host_activity(c), listed.data()));
    }
    std::vector<MoveRowItem> items;
    std::vector<uint32_t> colrec;
    struct Span { size_t g0, g1, s1; };      // items [g0, g1): the batch's gather, [g1, s1): its scatter
    std::vector<Span> spans;
    for (const MoveBatch &b : batches) {
        Span sp{items.size(), 0, 0};
        move_row_items(b.gather, row, items, colrec); sp.g1 = items.size();
        move_row_items(b.scatter, row, items, colrec); sp.s1 = items.size();
        spans.push_back(sp);
    }
    const auto [items_at, colrec_at] = pack_row_items(words, items, colrec);
    // the fade mode's bases travel too (dspi_pdmfade.h): the sources, then the destinations, behind the other lists
    const bool bases = c->pdm_fade.on && c->d_pdm_base;
    const size_t slots_at = words.size();
    if (bases) {
        for (const StreamMove &m : mv) words.push_back(m.src);
        for (const StreamMove &m : mv) words.push_back(m.dst);
        if ((rc = ensure(c, c->d_pdm_pack, (size_t)nm * 4))) return rc;
    }
    if ((rc = move_upload(c, words))) return rc;
    if (bases) {      // (through the packed temporary: swaps and cycles are safe)
        HIPCK(c, launch_pdm_base_gather(c->d_pdm_base, c->d_move + slots_at, nm, c->n_streams, c->d_pdm_pack, c->hs));
        HIPCK(c, launch_pdm_base_scatter(c->d_pdm_base, c->d_move + slots_at + nm, nm, c->n_streams, c->d_pdm_pack, c->hs));
    }
    // run-time state, on the context's stream, behind whatever it still has to do
    if (realign) HIPCK(c, launch_list_shifts(c->flavor, c->d_state, c->d_move, nullptr, nm, c->d_snap_shift, c->hs));
    for (const Span &sp : spans) {
        HIPCK(c, launch_move_gather(c->flavor, state_arrays(c), c->d_snap, c->d_move + items_at + sp.g0 * 4, c->d_move + colrec_at + sp.g0 * row, (uint32_t)(sp.g1 - sp.g0), c->hs));
        HIPCK(c, launch_move_scatter(c->flavor, state_arrays(c), c->d_snap, c->d_move + items_at + sp.g1 * 4, c->d_move + colrec_at + sp.g1 * row, (uint32_t)(sp.s1 - sp.g1),
                                     realign ? c->d_snap_shift : nullptr, c->hs));
    }
    // parameters travel by reference, activity travels with the stream: all sources are read before any destination is written.  A
    // destination that is no source loses its occupant (one reference less); a source that is no destination keeps its own and becomes
    // a paused, frozen copy.  (Such entries exist only where something is paused: `active` is allocated then.)
    if (c->spdif_ps.on) c->spdif_ps.move(mv.data(), nm, host_activity(c));      // (the S/PDIF position is the device's own counter: it travels too)
    c->pdm_life.move(mv.data(), nm);      // (... and whether its modulator is running)
    c->pdm_fade.move(mv.data(), nm);      // (... and how far it has faded)
    if (c->flash.on) c->flash.move(mv.data(), nm);      // (... and its flash, by reference)
    const bool have_active = !c->active.empty();
    std::vector<int32_t> img(nm);
    std::vector<uint8_t> act(nm, 1), is_dst(c->n_streams, 0);
    for (uint32_t i = 0; i < nm; i++) { img[i] = c->stream_image[mv[i].src]; if (have_active) act[i] = c->active[mv[i].src]; is_dst[mv[i].dst] = 1; }
    bool one_way = false;
    for (uint32_t i = 0; i < nm; i++) {
        assign_image(c, mv[i].dst, img[i]);
        if (have_active) set_active(c, mv[i].dst, act[i] != 0);
    }
    for (uint32_t i = 0; i < nm; i++)
        if (!is_dst[mv[i].src]) { set_active(c, mv[i].src, false); one_way = true; }
    c->launch_dirty = true;
    if (have_active) activity_changed(c);
    if (one_way) c->merge_hint = true;      // an image may have lost its last stream: the fold-back pass drops it
    return (int)nm;
}

int dspi_plan_compaction(const dspi_ctx *c, dspi_stream_move *moves, uint32_t cap, uint32_t flags) {
    if (!c || (flags & ~DSPI_COMPACT_ONE_WAY)) return DSPI_E_INVAL;
    const std::vector<StreamMove> plan = move_compaction(host_activity(c), c->n_streams, flags & DSPI_COMPACT_ONE_WAY);
    return plan_out(plan, moves, cap);
}

// ---- migration between two contexts (dspi_migrate.h: validation, plan, batches; dspi_move.h: targets; dspi_snapshot.hip: the kernels) ----
// both contexts hear why (dspi_last_error on either)
static int migrate_fail(dspi_ctx *src, dspi_ctx *dst, int code, const std::string &msg) { fail(src, code, msg); return fail(dst, code, msg); }

// "my stream has come this far", and the other context's stream waiting for it: the event is recorded before the wait is enqueued (a wait
// on an event that was never recorded is no wait)
static int migrate_signal(dspi_ctx *from, dspi_ctx *to) {
    HIPCK(from, hipSetDevice(from->device));
    HIPCK(from, hipEventRecord(from->ev_mig, from->hs));
    HIPCK(to, hipSetDevice(to->device));
    HIPCK(to, hipStreamWaitEvent(to->hs, from->ev_mig, 0));
    return 0;
}

int dspi_migrate_streams(dspi_ctx *src, dspi_ctx *dst, const dspi_stream_move *moves, uint32_t n, uint32_t flags) {
    if (!src || !dst) { fail(src, DSPI_E_INVAL, "dspi_migrate_streams: null context"); return fail(dst, DSPI_E_INVAL, "dspi_migrate_streams: null context"); }
    // everything is validated in both contexts before anything is written in either
    if (src == dst) return fail(src, DSPI_E_INVAL, "dspi_migrate_streams: one context on both sides (dspi_move_streams)");
    if (src->flavor != dst->flavor || src->fma != dst->fma) return migrate_fail(src, dst, DSPI_E_INVAL, "dspi_migrate_streams: the contexts differ in flavour or float contract");
    if (flags & ~(DSPI_MIGRATE_AS_IS | DSPI_MIGRATE_PAUSED)) return migrate_fail(src, dst, DSPI_E_INVAL, "dspi_migrate_streams: undefined flag bits");
    const StreamMove *list = reinterpret_cast<const StreamMove *>(moves);
    if (const char *why = migrate_validate(list, n, src->n_streams, dst->n_streams, host_activity(dst))) return migrate_fail(src, dst, DSPI_E_INVAL, std::string("dspi_migrate_streams: ") + why);
    if (src->flash.on && !dst->flash.on) return migrate_fail(src, dst, DSPI_E_INVAL, "dspi_migrate_streams: the source's streams own flashes (dspi_device_flash), the destination's do not");
    if (src->device == DSPI_DEVICE_NONE || dst->device == DSPI_DEVICE_NONE) return migrate_fail(src, dst, DSPI_E_NODEVICE, "host-only context: no run-time state to migrate");
    const uint32_t row = (uint32_t)src->sm.row, cap = std::min(move_batch_records(src), move_batch_records(dst));
    const bool realign = !(flags & DSPI_MIGRATE_AS_IS);
    const int via = dst->migrate_via;
    const bool same_device = src->device == dst->device, staged = via != dspi_ctx::kViaAuto || !same_device;      // staged: the records pass through the destination's scratch
    const size_t rec = snap_state_bytes(src->flavor, 1);
    // scratch, shift table, position arrays, events and the host transport's area: all before anything is enqueued
    int rc = snap_prepare(src, cap, false);
    if (rc || (rc = snap_prepare(dst, staged ? cap : 0, realign))) return rc;
    for (dspi_ctx *c : {src, dst}) {
        HIPCK(c, hipSetDevice(c->device));
        if (!c->ev_mig) HIPCK(c, hipEventCreateWithFlags(&c->ev_mig, hipEventDisableTiming));
        if (realign && (c == src || staged) && (rc = ensure(c, c->d_mig_pos, (size_t)n * 8))) return rc;
    }
    if (via == dspi_ctx::kViaHost) {
        const size_t need = std::max((size_t)std::min(cap, n) * rec, (size_t)n * 8);
        if ((rc = pinned_area(dst, dst->h_mig, need, need, "hipHostMalloc failed (migration area)"))) return rc;
    }
    // the call's work lists, one upload per context through its own staging area: the source gets the listed slots (positions kernel) and
    // the batches' gather items, the destination the targets (every shift is computed once, before anything is written) and the scatter items
    const std::vector<MoveBatch> batches = migrate_batches(list, n, cap);
    struct Side { std::vector<uint32_t> words; std::vector<size_t> item0; PackedItems at{0, 0}; } ss, ds;
    if (realign) {
        ss.words.resize(((size_t)n + 3) & ~(size_t)3);
        for (uint32_t i = 0; i < n; i++) ss.words[i] = list[i].src;
        pack_targets(ds.words, list_targets(list, n, dst->n_streams, row, host_activity(dst), nullptr));
    }
    {
        std::vector<MoveRowItem> si, di;
        std::vector<uint32_t> sc, dc;
        for (const MoveBatch &b : batches) {
            ss.item0.push_back(si.size()); move_row_items(b.gather, row, si, sc);
            ds.item0.push_back(di.size()); move_row_items(b.scatter, row, di, dc);
        }
        ss.item0.push_back(si.size()); ds.item0.push_back(di.size());
        ss.at = pack_row_items(ss.words, si, sc); ds.at = pack_row_items(ds.words, di, dc);
    }
    // the fade mode's bases (dspi_pdmfade.h) travel while both contexts have the mode; with the mode at the destination only, the arrivals' bases are 0
    const bool base_to = dst->pdm_fade.on && dst->d_pdm_base, base_from = base_to && src->pdm_fade.on && src->d_pdm_base;
    const size_t src_slots_at = ss.words.size(), dst_slots_at = ds.words.size();
    if (base_from) for (uint32_t i = 0; i < n; i++) ss.words.push_back(list[i].src);
    if (base_to) for (uint32_t i = 0; i < n; i++) ds.words.push_back(list[i].dst);
    if (base_from) {
        HIPCK(src, hipSetDevice(src->device));
        if ((rc = ensure(src, src->d_pdm_pack, (size_t)n * 4))) return rc;
        HIPCK(dst, hipSetDevice(dst->device));
        if (staged && (rc = ensure(dst, dst->d_pdm_pack, (size_t)n * 4))) return rc;
    }
    HIPCK(src, hipSetDevice(src->device));
    if ((rc = move_upload(src, ss.words))) return rc;
    HIPCK(dst, hipSetDevice(dst->device));
    if ((rc = move_upload(dst, ds.words))) return rc;
    // the records of one batch from the source's scratch to where the destination scatters them from (on the destination's stream, behind
    // the source's gather), or the positions the same way
    auto carry = [&](uint32_t *to, const uint32_t *from, size_t bytes) -> int {
        if (via == dspi_ctx::kViaHost) {
            HIPCK(src, hipSetDevice(src->device));
            HIPCK(src, hipMemcpyAsync(dst->h_mig, from, bytes, hipMemcpyDeviceToHost, src->hs));
            HIPCK(src, hipStreamSynchronize(src->hs));
            HIPCK(dst, hipSetDevice(dst->device));
            HIPCK(dst, hipMemcpyAsync(to, dst->h_mig, bytes, hipMemcpyHostToDevice, dst->hs));
            return 0;
        }
        int r = migrate_signal(src, dst);
        if (r) return r;
        if (staged) HIPCK(dst, hipMemcpyPeerAsync(to, dst->device, from, src->device, bytes, dst->hs));
        return 0;
    };
    // the rotations: the sources' pairs on the source's stream, then the shifts on the destination's
    if (realign) {
        HIPCK(src, hipSetDevice(src->device));
        HIPCK(src, launch_migrate_positions(src->flavor, src->d_state, src->d_move, n, src->d_mig_pos, src->hs));
        if ((rc = carry(dst->d_mig_pos, src->d_mig_pos, (size_t)n * 8))) return rc;
        HIPCK(dst, hipSetDevice(dst->device));
        HIPCK(dst, launch_list_shifts(dst->flavor, dst->d_state, dst->d_move, staged ? dst->d_mig_pos : src->d_mig_pos, n, dst->d_snap_shift, dst->hs));
        if (via == dspi_ctx::kViaHost) HIPCK(dst, hipStreamSynchronize(dst->hs));      // (the pinned area is rewritten by the first batch)
    }
    // the fade bases, the same way and inside the same ordering: gathered on the source's stream, carried, scattered on the destination's (the
    // batches' closing signal covers the source's packed buffer as it covers its scratch)
    if (base_from) {
        HIPCK(src, hipSetDevice(src->device));
        HIPCK(src, launch_pdm_base_gather(src->d_pdm_base, src->d_move + src_slots_at, n, src->n_streams, src->d_pdm_pack, src->hs));
        if ((rc = carry(reinterpret_cast<uint32_t *>(dst->d_pdm_pack.get()), reinterpret_cast<const uint32_t *>(src->d_pdm_pack.get()), (size_t)n * 4))) return rc;
    }
    if (base_to) {
        HIPCK(dst, hipSetDevice(dst->device));
        HIPCK(dst, launch_pdm_base_scatter(dst->d_pdm_base, dst->d_move + dst_slots_at, n, dst->n_streams, !base_from ? nullptr : staged ? dst->d_pdm_pack : src->d_pdm_pack, dst->hs));
        if (base_from && via == dspi_ctx::kViaHost) HIPCK(dst, hipStreamSynchronize(dst->hs));      // (the pinned area is rewritten by the first batch)
    }
    // the batches: the source gathers, the destination takes the records and scatters, the source waits before it gathers over the same
    // scratch again — and once more at the end, so that dspi_sync / dspi_destroy of the source cover the destination's use of its scratch
    for (size_t b = 0; b < batches.size(); b++) {
        const uint32_t nb = (uint32_t)batches[b].gather.size();
        HIPCK(src, hipSetDevice(src->device));
        HIPCK(src, launch_move_gather(src->flavor, state_arrays(src), src->d_snap, src->d_move + ss.at.items_at + ss.item0[b] * 4, src->d_move + ss.at.colrec_at + ss.item0[b] * row,
                                      (uint32_t)(ss.item0[b + 1] - ss.item0[b]), src->hs));
        if ((rc = carry(dst->d_snap, src->d_snap, (size_t)nb * rec))) return rc;
        HIPCK(dst, hipSetDevice(dst->device));
        HIPCK(dst, launch_move_scatter(dst->flavor, state_arrays(dst), staged ? dst->d_snap : src->d_snap, dst->d_move + ds.at.items_at + ds.item0[b] * 4,
                                       dst->d_move + ds.at.colrec_at + ds.item0[b] * row, (uint32_t)(ds.item0[b + 1] - ds.item0[b]), realign ? dst->d_snap_shift : nullptr, dst->hs));
        if (via == dspi_ctx::kViaHost) HIPCK(dst, hipStreamSynchronize(dst->hs));
        else if ((rc = migrate_signal(dst, src))) return rc;
    }
    // parameters travel BY VALUE, through the books of an import: each distinct object among the listed streams is copied once, pending
    // state operations included, and appended to the destination's; the arrivals leave the former occupants' objects.  The fold-back pass
    // (merge_images, at the destination's next commit) drops what nobody uses any more and folds equal objects.
    std::vector<int32_t> used;
    std::vector<uint32_t> index;
    snap_images(src, 0, n, used, &index, list);
    const size_t base = dst->images.size();
    for (int32_t im : used) add_image(dst, std::make_unique<Params>(*src->images[(size_t)im]));
    for (uint32_t i = 0; i < n; i++) assign_image(dst, list[i].dst, (int32_t)(base + index[i]));
    dst->merge_hint = true; dst->launch_dirty = true;
    // the flashes travel by value too (dspi_flash.h); arrivals from a context without the mode get the flash a first boot leaves
    if (dst->flash.on) {
        if (src->flash.on) { src->flash.leave(list, n); dst->flash.arrive(src->flash, list, n); }
        else {
            std::vector<int32_t> fresh(used.size(), -1);
            for (uint32_t i = 0; i < n; i++) {
                int32_t &o = fresh[index[i]];
                if (o < 0) o = dst->flash.add(Flash::first_boot(dst->flavor, dst->populated, dst->images[base + index[i]].get()));
                dst->flash.assign(list[i].dst, o);
            }
        }
        std::vector<uint32_t> arrived(n);
        for (uint32_t i = 0; i < n; i++) arrived[i] = list[i].dst;
        flash_resync(dst, arrived.data(), 0, n);
    }
    if (src->audio_started) dst->audio_started = true;      // running devices arrived: dspi_load_flash_dump is no boot any more
    // the S/PDIF position is the device's own counter, the activity belongs to the stream: both arrive with it (DSPI_MIGRATE_PAUSED: it
    // arrives paused); every source slot stays behind as a paused, frozen copy, its position frozen with it
    const uint8_t *const sa = host_activity(src);
    std::vector<uint8_t> act(n, 1);
    for (uint32_t i = 0; i < n; i++) act[i] = (flags & DSPI_MIGRATE_PAUSED) ? 0 : (!sa || sa[list[i].src]) ? 1 : 0;
    if (dst->spdif_ps.on)
        for (uint32_t i = 0; i < n; i++) dst->spdif_ps.arrive(list[i].dst, src->spdif_ps.on ? src->spdif_ps.get(list[i].src, sa) : src->spdif_pos, act[i] != 0);
    if (src->spdif_ps.on)
        for (uint32_t i = 0; i < n; i++) src->spdif_ps.pause(list[i].src, 1, sa);
    for (uint32_t i = 0; i < n; i++) dst->pdm_life.arrive(list[i].dst, src->pdm_life.running[list[i].src]);      // (a running modulator arrives running)
    // ... and a fading one fading, where both contexts fade; else the position arrives as 0, and a fade in flight has ended as an immediate stop
    for (uint32_t i = 0; i < n; i++) dst->pdm_fade.arrive(dst->pdm_life, list[i].dst, src->pdm_fade.on ? src->pdm_fade.pos[list[i].src] : 0u);
    if (src->active.empty()) src->active.assign(src->n_streams, 1);
    for (uint32_t i = 0; i < n; i++) { set_active(dst, list[i].dst, act[i] != 0); set_active(src, list[i].src, false); }
    activity_changed(src); activity_changed(dst);
    return (int)n;
}

int dspi_plan_migration(const dspi_ctx *src, const dspi_ctx *dst, uint32_t want, dspi_stream_move *moves, uint32_t cap, uint32_t flags) {
    if (!src || !dst || flags || src->flavor != dst->flavor || src->fma != dst->fma) return DSPI_E_INVAL;
    const std::vector<StreamMove> plan = migrate_plan(host_activity(src), src->n_streams, host_activity(dst), dst->n_streams, want);
    return plan_out(plan, moves, cap);
}

// ---- grouping (dspi_group.h: the rule).  Bookkeeping like the compaction plan, but on the parameter objects as they stand folded: two
// devices that were given the same blob by separate calls are one group.
int dspi_plan_grouping(dspi_ctx *c, dspi_stream_move *moves, uint32_t cap, uint32_t flags) {
    if (!c || (flags & ~DSPI_GROUP_ONE_WAY)) return DSPI_E_INVAL;
    if (c->images.size() > 1) merge_images(c);
    const size_t ni = c->images.size();
    std::vector<uint32_t> cls;
    if (c->flavor && ni > 1) {
        // the structure of every object that holds an active stream: what the last upload built (plan_in.sig) where the object has not
        // changed since, else built here, on all host threads when there are many (every stream its own preset)
        std::vector<uint8_t> grouped(ni, 0);
        for (uint32_t s = 0; s < c->n_streams; s++) if (!c->n_paused || c->active[s]) grouped[(size_t)c->stream_image[s]] = 1;
        std::vector<ImageSig> sig(ni);
        memset(sig.data(), 0xff, ni * sizeof(ImageSig));      // (objects without an active stream form no group: their class is never read)
        std::vector<size_t> todo;
        for (size_t i = 0; i < ni; i++) {
            if (!grouped[i]) continue;
            if (!c->images[i]->dirty && i < c->plan_in.sig.size()) sig[i] = c->plan_in.sig[i];
            else todo.push_back(i);
        }
        const unsigned csr = _mm_getcsr();      // the workers round and flush exactly like the calling thread
        auto build = [&](size_t k0, size_t k1) {
            _mm_setcsr(csr);
            DevImage img;
            for (size_t k = k0; k < k1; k++) { c->images[todo[k]]->build_image(img); sig[todo[k]] = make_sig(img); }
        };
        const size_t n = todo.size();
        const size_t nt = n >= 512 ? std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), std::min<size_t>(32, n / 128)) : 1;
        if (nt > 1) {
            std::vector<std::thread> th;
            for (size_t t = 0; t < nt; t++) th.emplace_back(build, n * t / nt, n * (t + 1) / nt);
            for (auto &x : th) x.join();
        } else build(0, n);
        cls = group_classes(sig.data(), ni);
    }
    const std::vector<StreamMove> plan = group_plan(host_activity(c), c->stream_image.data(), cls.empty() ? nullptr : cls.data(), c->n_streams, flags & DSPI_GROUP_ONE_WAY);
    return plan_out(plan, moves, cap);
}

// ---- stream boots (dspi_boot.h: validation and the kernel's work items; dspi_boot.hip: the power-on kernel) ----
int dspi_boot_streams(dspi_ctx *c, const uint32_t *streams, uint32_t n, const void *dump, size_t len, uint32_t flags, int *selection) {
    if (!c) return DSPI_E_INVAL;
    if (flags & ~(DSPI_BOOT_STREAMS_AS_IS | DSPI_BOOT_STREAMS_OWN_FLASH)) return fail(c, DSPI_E_INVAL, "dspi_boot_streams: undefined flag bits");
    // everything is validated before anything is written
    if (const char *why = boot_validate(streams, n, c->n_streams)) return fail(c, DSPI_E_INVAL, std::string("dspi_boot_streams: ") + why);
    const bool own = (flags & DSPI_BOOT_STREAMS_OWN_FLASH) != 0;
    if (own && !c->flash.on) return fail(c, DSPI_E_INVAL, "dspi_boot_streams: DSPI_BOOT_STREAMS_OWN_FLASH needs dspi_device_flash");
    if (own && dump) return fail(c, DSPI_E_INVAL, "dspi_boot_streams: DSPI_BOOT_STREAMS_OWN_FLASH takes no dump");
    if (dump && len < kFlashDumpBytes) return fail(c, DSPI_E_SHORT, "dspi_boot_streams: dump shorter than DSPI_FLASH_DUMP_BYTES");
    // the device that has just been powered on: dspi_create's own, or one that boots from the dump's flash (first_boot = false, then
    // boot(dump): Params::load_flash_dump's boot path; sample rate, UAC1 volume and mute stay at their power-on values).  With
    // DSPI_BOOT_STREAMS_OWN_FLASH one such device per distinct flash object among the listed streams, booted from that flash.
    struct Group { std::unique_ptr<Params> p; int32_t flash = -1; int sel = 48; std::vector<uint32_t> members; };
    std::vector<Group> groups;
    if (own) {
        std::map<int32_t, size_t> of_flash;
        for (uint32_t i = 0; i < n; i++) {
            const auto it = of_flash.emplace(c->flash.index[streams[i]], groups.size());
            if (it.second) { groups.emplace_back(); groups.back().flash = it.first->first; }
            groups[it.first->second].members.push_back(streams[i]);
        }
        for (Group &g : groups) {
            g.p = std::make_unique<Params>(c->flavor, c->fma, false);
            g.sel = g.p->load_flash_dump(c->flash.objects[(size_t)g.flash]->bytes, kFlashDumpBytes, true);
        }
    } else {
        groups.emplace_back();
        groups[0].p = std::make_unique<Params>(c->flavor, c->fma, dump ? false : !c->populated);
        if (dump) groups[0].sel = groups[0].p->load_flash_dump(dump, len, true);
        groups[0].members.assign(streams, streams + n);
    }
    // run-time state, on the context's stream, behind whatever it still has to do (the kernel reads the rows' residents' positions there)
    if (c->device != DSPI_DEVICE_NONE) {
        HIPCK(c, hipSetDevice(c->device));
        const std::vector<BootRowItem> items = boot_row_items(streams, n, c->n_streams, (uint32_t)c->sm.row, host_activity(c), (flags & DSPI_BOOT_STREAMS_AS_IS) != 0);
        const bool bases = c->pdm_fade.on && c->d_pdm_base;
        int rc = boot_upload(c, items, streams, bases ? n : 0);
        if (rc) return rc;
        HIPCK(c, launch_boot(c->flavor, state_arrays(c), c->d_move, (uint32_t)items.size(), c->hs));
        if (bases) HIPCK(c, launch_pdm_base_scatter(c->d_pdm_base, c->d_move + items.size() * (sizeof(BootRowItem) / 4), n, c->n_streams, nullptr, c->hs));      // fade_base_pcm at power-on: 0
    }
    // the flash (dspi_device_flash): the dump with the boot's own writes, the flash a first boot leaves, or — own flash — the streams' flash
    // with the boot's writes (in place when every holder is listed, else in a copy the listed holders share)
    if (c->flash.on) {
        for (Group &g : groups) {
            std::unique_ptr<Flash> f;
            if (own) {
                if (c->flash.refs[(size_t)g.flash] == g.members.size()) { c->flash.objects[(size_t)g.flash]->boot_writes(c->flavor); continue; }
                f = std::make_unique<Flash>(*c->flash.objects[(size_t)g.flash]);
                f->boot_writes(c->flavor);
            } else if (dump) {
                f = std::make_unique<Flash>();
                f->set_bytes(dump);
                f->boot_writes(c->flavor);
            } else f = Flash::first_boot(c->flavor, c->populated, nullptr);
            g.flash = c->flash.add(std::move(f));
            c->flash.boot(g.members.data(), (uint32_t)g.members.size(), g.flash);
        }
        for (Group &g : groups) flash_sync_mirrors(*c->flash.objects[(size_t)g.flash], *g.p);
    }
    // parameters: the listed streams leave their objects (whose pending state operations never reach them) and share ONE new one (own
    // flash: one per distinct flash object), whose own pending operations the next commit applies over the power-on state, as after
    // dspi_create.  An object that lost its last stream is dropped, and a new object equal to one already here folded into it, by the
    // fold-back pass (merge_images).
    for (Group &g : groups) {
        const int32_t slot = add_image(c, std::move(g.p));
        for (uint32_t s : g.members) assign_image(c, s, slot);
    }
    c->launch_dirty = true; c->merge_hint = true;
    if (c->spdif_ps.on) c->spdif_ps.boot(streams, n, host_activity(c));      // a device that has just been powered on sends frame 0 of a block first
    c->pdm_life.boot(streams, n);      // ... and has never run its modulator
    c->pdm_fade.boot(streams, n);      // ... nor faded it
    if (selection) *selection = groups[0].sel;
    return (int)n;
}

// ---- the streams' own flashes (include/dspi.h "a stream's own flash"; dspi_flash.h) ----
int dspi_device_flash(dspi_ctx *c, int enable) {
    if (!c) return DSPI_E_INVAL;
    if (enable < 0 || (enable != 0) == c->flash.on) return c->flash.on ? 1 : 0;
    if (!enable) { c->flash.drop(); return 0; }
    c->flash.enable(c->n_streams);
    flash_first_boot_range(c, 0, c->n_streams);
    return 1;
}

int dspi_flash_read(dspi_ctx *c, uint32_t stream, void *dump, size_t cap) {
    if (!c || !dump) return DSPI_E_INVAL;
    if (!c->flash.on) return fail(c, DSPI_E_INVAL, "dspi_flash_read: the streams own no flash (dspi_device_flash)");
    if (stream >= c->n_streams) return fail(c, DSPI_E_INVAL, "dspi_flash_read: stream index out of range");
    if (cap < kFlashDumpBytes) return fail(c, DSPI_E_SHORT, "dspi_flash_read: buffer shorter than DSPI_FLASH_DUMP_BYTES");
    memcpy(dump, c->flash.readable(stream).bytes, kFlashDumpBytes);
    return (int)kFlashDumpBytes;
}

int dspi_flash_write(dspi_ctx *c, uint32_t first, uint32_t count, const void *dump, size_t len) {
    if (!c || !dump) return DSPI_E_INVAL;
    // everything is validated before anything is written
    if (!c->flash.on) return fail(c, DSPI_E_INVAL, "dspi_flash_write: the streams own no flash (dspi_device_flash)");
    if (count == 0 || (uint64_t)first + count > c->n_streams) return fail(c, DSPI_E_INVAL, "dspi_flash_write: stream range out of bounds");
    if (len < kFlashDumpBytes) return fail(c, DSPI_E_SHORT, "dspi_flash_write: dump shorter than DSPI_FLASH_DUMP_BYTES");
    auto f = std::make_unique<Flash>();
    f->set_bytes(dump);
    const int32_t obj = c->flash.add(std::move(f));
    for (uint32_t s = first; s < first + count; s++) c->flash.assign(s, obj);
    flash_resync(c, first, count);      // the mirrors follow the new directory (without a valid one: the fresh directory every request would see)
    return (int)count;
}

// ---- resizing (dspi_resize.h: validation, row arithmetic, the new slots' work items; dspi_boot.hip: the power-on kernel) ----
// The persistent per-stream arrays are row-outermost, so a context of other rows is a prefix copy.  New arrays of `rows` rows, ALL of them
// allocated before anything else happens (a refusal leaves the context as it was); the first `copy` rows come over device to device on the
// context's stream, behind its earlier work; then the stream is waited for, once, and the old arrays are freed.
static int resize_reallocate(dspi_ctx *c, uint32_t rows, uint32_t copy) {
    HipAlloc a;
    hipError_t e = hipSuccess;
    // (d_pdm before the modulator's first run and d_pdm_base before the fade mode's first enable are absent, and stay so)
    const Mem m = persist_reallocate(a, c->persist, c->sm, rows, c->cap_wg, [&](void *const *fresh) {
        for (int k = 0; k < kNumPersist && e == hipSuccess; k++)
            if (fresh[k] && copy) e = hipMemcpyAsync(fresh[k], c->persist[k]->p, (size_t)copy * kPersist[k].row_bytes(c->sm), hipMemcpyDeviceToDevice, c->hs);
        if (e == hipSuccess) e = hipStreamSynchronize(c->hs);
        return e == hipSuccess;
    });
    if (m == Mem::AllocFailed) return fail(c, DSPI_E_NOMEM, "hipMalloc failed (resized arrays, " + std::to_string(rows) + " rows)");
    if (m != Mem::Ok) return fail(c, DSPI_E_HIP, std::string("resized arrays: ") + hipGetErrorString(e));
    return 0;
}
// a row count no array's byte size can express is refused with the other rules, before anything is written
static bool resize_rows_fit(const dspi_ctx *c, uint32_t rows) { return persist_rows_fit(c->sm, rows); }

// Every per-stream book of the context, extended to or cut at n_new (beside the maintenance books above: stream_image / image_refs,
// active / n_paused / paused_runs, spdif_ps, and through the dirty flags the device's copies of activity, stream images and S/PDIF
// positions, the assignment and the launch plan).  Growing: the new slots reference `slot`, a parameter object added for them.
static void resize_books(dspi_ctx *c, uint32_t n_new, int32_t slot, bool arrive_paused) {
    const uint32_t n_old = c->n_streams;
    if (n_new < n_old) {
        for (uint32_t s = n_new; s < n_old; s++) c->image_refs[(size_t)c->stream_image[s]]--;
        c->n_paused -= n_old - n_new;      // (every cut slot was paused: resize_validate)
        c->active.resize(n_new);
    } else {
        c->image_refs[(size_t)slot] += n_new - n_old;
        if (arrive_paused && c->active.empty()) c->active.assign(n_old, 1);
        if (!c->active.empty()) c->active.resize(n_new, arrive_paused ? 0 : 1);
        if (arrive_paused) c->n_paused += n_new - n_old;
    }
    c->stream_image.resize(n_new, slot);
    c->n_streams = n_new;
    c->n_wg = resize_rows_of(n_new, (uint32_t)c->sm.row);
    if (c->spdif_ps.on) {      // old slots keep their positions; a device that has just been powered on sends frame 0 of a block first
        c->spdif_ps.word.resize(n_new, 0u);
        c->spdif_ps.dirty = true;
        for (uint32_t s = n_old; s < n_new; s++) c->spdif_ps.set(s, 0, host_activity(c));
    }
    c->pdm_life.resize(n_new);      // (new slots: never ran)
    c->pdm_fade.resize(n_new);      // (... never faded)
    if (c->flash.on) {              // (... and share the flash a first boot leaves; a shrink releases the cut slots')
        c->flash.resize(n_new, n_new > n_old ? c->flash.add(Flash::first_boot(c->flavor, c->populated, nullptr)) : -1);
        if (n_new > n_old) flash_resync(c, n_old, n_new - n_old);
    }
    c->assignment_dirty = true; c->merge_hint = true;      // (an object may have lost its last stream, or the new one equal one already here: the fold-back pass)
    activity_changed(c);
}

int dspi_resize_streams(dspi_ctx *c, uint32_t n_streams, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    // everything is validated before anything is written
    if (const char *why = resize_validate(c->n_streams, n_streams, flags, host_activity(c))) return fail(c, DSPI_E_INVAL, std::string("dspi_resize_streams: ") + why);
    const uint32_t n_old = c->n_streams, row = (uint32_t)c->sm.row;
    const ResizeRows r = resize_rows(n_old, n_streams, c->cap_wg, row);
    if (!resize_rows_fit(c, r.capacity) || n_streams > 0x7fffffffu) return fail(c, DSPI_E_INVAL, "dspi_resize_streams: the arrays' byte sizes overflow");      // (stream indices are int32_t)
    if (n_streams == n_old) return (int)n_old;
    if (n_streams < n_old) { resize_books(c, n_streams, -1, false); return (int)n_streams; }      // no allocation, no free, no wait: the capacity stays
    if (c->device != DSPI_DEVICE_NONE) {
        HIPCK(c, hipSetDevice(c->device));
        // the new slots' work items go up first (scratch of the call, no state of the context), so that nothing can fail between the
        // reallocation and the power-on launch
        const std::vector<BootRowItem> items = resize_row_items(n_old, n_streams, row, host_activity(c));
        int rc = boot_upload(c, items);
        if (rc || (r.reallocate && (rc = resize_reallocate(c, r.capacity, r.copy)))) return rc;
        // power-on state into EVERY new slot, whatever its column held (padding columns are dirty after a shrink, new rows unwritten),
        // behind the context's earlier work: the kernel reads the grown row's resident's positions there
        HIPCK(c, launch_boot(c->flavor, state_arrays(c), c->d_move, (uint32_t)items.size(), c->hs));
        if (c->d_pdm_base) HIPCK(c, hipMemsetAsync(c->d_pdm_base + n_old, 0, (size_t)(n_streams - n_old) * 4, c->hs));      // (... and fade base 0)
    } else c->cap_wg = r.capacity;
    // parameters: the boot's own half with a NULL dump — ONE new object for all new slots, dspi_create's device on this context
    const int32_t slot = add_image(c, std::make_unique<Params>(c->flavor, c->fma, !c->populated));
    resize_books(c, n_streams, slot, (flags & DSPI_RESIZE_PAUSED) != 0);
    return (int)n_streams;
}

int dspi_reserve_streams(dspi_ctx *c, uint32_t n_streams) {
    if (!c) return DSPI_E_INVAL;
    if (const char *why = reserve_validate(c->n_streams, n_streams)) return fail(c, DSPI_E_INVAL, std::string("dspi_reserve_streams: ") + why);
    const uint32_t row = (uint32_t)c->sm.row;
    const ResizeRows r = reserve_rows(c->n_streams, n_streams, c->cap_wg, row);
    if (!resize_rows_fit(c, r.capacity) || (uint64_t)r.capacity * row > 0x7fffffffull) return fail(c, DSPI_E_INVAL, "dspi_reserve_streams: the arrays' byte sizes overflow");
    if (r.reallocate) {
        if (c->device == DSPI_DEVICE_NONE) c->cap_wg = r.capacity;
        else {
            HIPCK(c, hipSetDevice(c->device));
            int rc = resize_reallocate(c, r.capacity, r.copy);
            if (rc) return rc;
        }
    }
    return (int)(c->cap_wg * row);
}

uint32_t dspi_stream_capacity(const dspi_ctx *c) { return c ? c->cap_wg * (uint32_t)c->sm.row : 0; }

int dspi_debug_stream_positions(dspi_ctx *c, uint32_t first, uint32_t count, uint32_t *widx, uint32_t *ring_pos) {
    if (!c || !widx || !ring_pos) return DSPI_E_INVAL;
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_debug_stream_positions: stream range out of bounds");
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no run-time state");
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipStreamSynchronize(c->hs));
    // the two slots' rows of every touched row of the state array ([row][slot][lane])
    const uint32_t row = (uint32_t)c->sm.row, r0 = first / row, rows = (first + count - 1) / row - r0 + 1;
    std::vector<uint32_t> w((size_t)rows * row), r((size_t)rows * row);
    const size_t pitch = (size_t)c->sm.n_slots * row * 4;
    HIPCK(c, hipMemcpy2D(w.data(), (size_t)row * 4, c->d_state + ((size_t)r0 * c->sm.n_slots + c->sm.widx) * row, pitch, (size_t)row * 4, rows, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy2D(r.data(), (size_t)row * 4, c->d_state + ((size_t)r0 * c->sm.n_slots + c->sm.ring_pos) * row, pitch, (size_t)row * 4, rows, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < count; k++) {
        const size_t at = (size_t)first + k - (size_t)r0 * row;
        widx[k] = w[at] & ((uint32_t)c->sm.max_delay - 1u);
        ring_pos[k] = r[at] & ((uint32_t)kRingLen - 1u);
    }
    return (int)count;
}

// ---- S/PDIF subframes: pico_audio_spdif_multi sample_encoding.h:27-47 + audio_spdif.c:76-116 (dspi_spdif.hip) ----
// the sample-rate byte of the channel status is each device's own (audio_spdif.c:250-256): one word for everybody (fs) while every live
// image runs at one rate, else per stream from the committed images (rates)
static int spdif_rates(dspi_ctx *c, uint32_t &fs, SpdifRates &rates) {
    fs = readable(c, DSPI_ALL_STREAMS).freq;
    rates = SpdifRates{nullptr, nullptr, 0u};
    bool one_rate = true;
    for (size_t i = 0; i < c->images.size(); i++) if (c->image_refs[i] > 0 && c->images[i]->freq != fs) one_rate = false;
    if (one_rate) return 0;
    int rc = commit_params(c);
    if (!rc) rates = SpdifRates{c->d_images, c->d_stream_image, 0u};
    return rc;
}

int dspi_spdif_encode(dspi_ctx *c, const int32_t *pairs, uint32_t n_frames, uint32_t block_pos, uint32_t *subframes, uint32_t flags) {
    if (!c || !pairs || !subframes || n_frames == 0 || block_pos >= 192) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    const bool tiled = flags & DSPI_OUT_TILED, dev = flags & DSPI_MEM_DEVICE;
    const size_t cols = tiled ? (size_t)c->n_wg * c->sm.row : (size_t)c->n_streams;
    const size_t in_b = cols * c->sm.n_pairs * n_frames * 8, out_b = in_b * 2;
    const int32_t *d_in = pairs;
    uint32_t *d_out = subframes;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_in, in_b)) || (rc = ensure(c, c->d_spdif_out, out_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_in, pairs, in_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_spdif_in; d_out = c->d_spdif_out;
    }
    uint32_t fs;
    SpdifRates rates;
    if ((rc = spdif_rates(c, fs, rates))) return rc;
    HIPCK(c, launch_spdif(tiled, d_in, d_out, c->n_streams, (uint32_t)c->sm.n_pairs, n_frames, (uint32_t)c->sm.row, c->n_wg, block_pos, fs, rates, c->hs));
    if (!dev && (rc = stage_down(c, subframes, c->d_spdif_out, out_b))) return rc;
    return (int)((block_pos + n_frames) % 192u);
}

// ---- I2S slots: pico_audio_i2s_multi/audio_i2s_multi.c:217-226 (dspi_spdif.hip) ----
int dspi_i2s_encode(dspi_ctx *c, const int32_t *pairs, uint32_t n_frames, uint32_t pair_mask, uint32_t *words, uint32_t flags) {
    if (!c || !pairs || !words || n_frames == 0 || (pair_mask >> c->sm.n_pairs) != 0) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    if (pair_mask == DSPI_I2S_PAIRS_BY_TYPE) {          // the slots whose output type is I2S (output_types[], REQ_SET_OUTPUT_TYPE)
        const Params &p = readable(c, DSPI_ALL_STREAMS);
        for (int i = 0; i < c->sm.n_pairs; i++) if (p.output_types[i] == 1) pair_mask |= 1u << i;
        if (pair_mask == 0) return 0;
    }
    const bool tiled = flags & DSPI_OUT_TILED, dev = flags & DSPI_MEM_DEVICE;
    const size_t cols = tiled ? (size_t)c->n_wg * c->sm.row : (size_t)c->n_streams;
    const size_t bytes = cols * c->sm.n_pairs * n_frames * 8;
    const int32_t *d_in = pairs;
    uint32_t *d_out = words;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_in, bytes)) || (rc = ensure(c, c->d_spdif_out, bytes))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_in, pairs, bytes, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, hipMemcpyAsync(c->d_spdif_out, words, bytes, hipMemcpyHostToDevice, c->hs));     // pairs outside the mask keep the caller's words
        d_in = c->d_spdif_in; d_out = c->d_spdif_out;
    }
    HIPCK(c, launch_i2s(tiled, d_in, d_out, c->n_streams, (uint32_t)c->sm.n_pairs, n_frames, (uint32_t)c->sm.row, c->n_wg, pair_mask, c->hs));
    if (!dev && (rc = stage_down(c, words, c->d_spdif_out, bytes))) return rc;
    return (int)pair_mask;
}

int dspi_spdif_block_pos(dspi_ctx *c, int32_t set) {
    if (!c || set >= 192) return DSPI_E_INVAL;
    if (set >= 0) c->spdif_pos = (uint32_t)set;
    return (int)c->spdif_pos;
}

// ---- per-stream block positions (dspi_spdifpos.h) ----
int dspi_spdif_per_stream(dspi_ctx *c, int enable) {
    if (!c) return DSPI_E_INVAL;
    if (enable > 0) c->spdif_ps.enable(c->n_streams, c->spdif_pos);
    else if (enable == 0) c->spdif_ps.disable();
    return c->spdif_ps.on ? 1 : 0;
}

int dspi_spdif_stream_pos(dspi_ctx *c, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get) {
    if (!c) return DSPI_E_INVAL;
    if (!c->spdif_ps.on) return fail(c, DSPI_E_INVAL, "dspi_spdif_stream_pos: per-stream positions are off (dspi_spdif_per_stream)");
    if (!snap_range_ok(c, first, count)) return fail(c, DSPI_E_INVAL, "dspi_spdif_stream_pos: stream range out of bounds");
    // everything is validated before anything is written
    if (set) for (uint32_t k = 0; k < count; k++) if (set[k] >= kSpdifBlock) return fail(c, DSPI_E_INVAL, "dspi_spdif_stream_pos: a position is 0..191");
    if (set) for (uint32_t k = 0; k < count; k++) c->spdif_ps.set(first + k, set[k], host_activity(c));
    if (get) for (uint32_t k = 0; k < count; k++) get[k] = c->spdif_ps.get(first + k, host_activity(c));
    return (int)count;
}

int dspi_spdif_encode_v(dspi_ctx *c, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos, uint32_t *subframes, uint32_t flags) {
    if (!c || !pairs || !subframes || !block_pos || n_frames == 0) return DSPI_E_INVAL;
    if (flags & ~(DSPI_MEM_DEVICE | DSPI_OUT_TILED)) return fail(c, DSPI_E_INVAL, "dspi_spdif_encode_v: undefined flag bits");
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    const bool tiled = flags & DSPI_OUT_TILED, dev = flags & DSPI_MEM_DEVICE;
    // host positions are validated before anything is launched; device positions are the kernels' to reduce modulo 192
    if (!dev) for (uint32_t s = 0; s < c->n_streams; s++) if (block_pos[s] >= kSpdifBlock) return fail(c, DSPI_E_INVAL, "dspi_spdif_encode_v: a position is 0..191");
    HIPCK(c, hipSetDevice(c->device));
    const size_t cols = tiled ? (size_t)c->n_wg * c->sm.row : (size_t)c->n_streams;
    const size_t in_b = cols * c->sm.n_pairs * n_frames * 8, out_b = in_b * 2, pos_b = (size_t)c->n_streams * 4;
    const int32_t *d_in = pairs;
    uint32_t *d_out = subframes;
    const uint32_t *d_pos = block_pos;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_in, in_b)) || (rc = ensure(c, c->d_spdif_out, out_b)) ||
            (rc = ensure(c, c->d_spdif_vpos, pos_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_in, pairs, in_b, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, hipMemcpyAsync(c->d_spdif_vpos, block_pos, pos_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_spdif_in; d_out = c->d_spdif_out; d_pos = c->d_spdif_vpos;
    }
    uint32_t fs;
    SpdifRates rates;
    if ((rc = spdif_rates(c, fs, rates))) return rc;
    HIPCK(c, launch_spdif(tiled, d_in, d_out, c->n_streams, (uint32_t)c->sm.n_pairs, n_frames, (uint32_t)c->sm.row, c->n_wg, 0u, fs, rates, c->hs, d_pos));
    return dev ? DSPI_OK : stage_down(c, subframes, c->d_spdif_out, out_b);
}

int dspi_sync(dspi_ctx *c) {
    if (!c) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return DSPI_E_NODEVICE;
    HIPCK(c, hipStreamSynchronize(c->hs));
    return DSPI_OK;
}

// ---- dspi_process: the call's layout (dspi_plan.h plan_call), then one of three memory paths ----

// alpha^count (leveller.c:200) on the device = step 1 of include/dspi_detmath.h's powf + its exception table; proven equal to the exact form
// for the firmware's alphas and every block length by tools/gen_detmath_tables.c — and checked here for the alphas this context has built
// into its images (every one it ever built, leveller on or off), once per block length and set of alphas
static int check_leveller_alphas(dspi_ctx *c, uint32_t block_len) {
    if (c->lv_checked_count == block_len && c->lv_checked_n == c->lv_alphas.size()) return 0;
    for (const uint32_t bits : c->lv_alphas) {
        float al; memcpy(&al, &bits, 4);
        const float t = dspi_det_powf_tab(al, (float)block_len), e = dspi_det_powf(al, (float)block_len);
        if (memcmp(&t, &e, 4) != 0) return fail(c, DSPI_E_UNSUPPORTED, "leveller alpha^count: this (alpha, block length) is not covered by the device's exception table (include/dspi_detmath_tables.h)");
    }
    c->lv_checked_count = block_len; c->lv_checked_n = c->lv_alphas.size();
    return 0;
}

// the chain launches for the rows [r0, r1): every non-empty path of the plan, in launch order (the lists are sorted by row)
static int launch_paths(dspi_ctx *c, KArgs &a, uint32_t r0, uint32_t r1) {
    for (const PathInfo &pi : kPaths) {
        const auto &items = c->plan.items[(int)pi.path];
        if (items.empty()) continue;
        auto by_row = [](const WgItem &it, uint32_t r) { return it.wg < r; };
        const size_t lo = (size_t)(std::lower_bound(items.begin(), items.end(), r0, by_row) - items.begin());
        const size_t hi = (size_t)(std::lower_bound(items.begin(), items.end(), r1, by_row) - items.begin());
        if (hi == lo) continue;
        a.items = c->d_litems + c->plan.offset[(int)pi.path] + lo;
        hipError_t e = launch_chain(pi.path, a, (uint32_t)(hi - lo), c->hs);
        if (e == hipErrorNotSupported) return fail(c, DSPI_E_UNSUPPORTED, "this flavour has no HIP kernel yet");
        if (e != hipSuccess) return fail(c, DSPI_E_HIP, std::string("chain kernel launch: ") + hipGetErrorString(e));
        c->audio_started = true;      // only now: a call refused for its arguments, or one that could not allocate, leaves a booting device booting (dspi_load_flash_dump)
    }
    return 0;
}

// ... of a call (a: its arguments, a.pairs the caller's words).  Two-pass S/PDIF: L.two_pass_rows rows at a time into the scratch of pair
// words, then the subframe encoder from there into a.pairs.  Paused streams: the chain leaves their words in the scratch stale, and the
// ENCODER SKIPS them (SpdifRates::active) — the scratch is not zeroed —, so that in the caller's device buffer their subframes stay unwritten.
// dspi_process_wire with an I2S slot in play (L.wire_encoder): the same route with the wire encoder (dspi_wire.hip) as the second pass; on the
// host-buffer paths it also zeroes the I2S regions' second halves, which no word of the call reaches.
// dspi_process_devices with DSPI_OUT_TILED (L.wire_tiled): the same route once more, the chain writing TILED pair words into the scratch and
// the tiled wire encoder (dspi_wire_tiled.hip) reading them there
static int launch_rows(dspi_ctx *c, KArgs a, const CallLayout &L, uint32_t r0, uint32_t r1) {
    if (!L.spdif_two_pass) return launch_paths(c, a, r0, r1);
    char *const subframes = reinterpret_cast<char *>(a.pairs);
    const uint32_t row = (uint32_t)c->sm.row;
    for (uint32_t q0 = r0; q0 < r1; q0 += L.two_pass_rows) {
        const uint32_t q1 = std::min(r1, q0 + L.two_pass_rows);
        const size_t s0 = (size_t)q0 * row, s1 = std::min((size_t)q1 * row, (size_t)c->n_streams);
        a.pairs = c->d_spdif_words; a.pairs_stream0 = (uint32_t)s0;      // the kernels index by absolute stream: stream s0 lands at the scratch's start
        // ... and tiled words by absolute row: row q0's tile lands at the scratch's start (rows below q0 are not launched, nothing below it is touched)
        if (L.wire_tiled) { a.pairs = c->d_spdif_words - (size_t)q0 * row * c->sm.n_pairs * L.frames * 2; a.pairs_stream0 = 0u; }
        int rc = launch_paths(c, a, q0, q1);
        if (rc) return rc;
        uint32_t *const dst = reinterpret_cast<uint32_t *>(subframes + s0 * L.pairs.per);
        const uint32_t pos = c->spdif_ps.on ? c->spdif_ps.clock : c->spdif_pos;
        const SpdifRates rates{c->d_images, c->d_stream_image, (uint32_t)s0, activity(c)};
        const uint32_t *const stream_pos = c->spdif_ps.on ? c->d_spdif_ps : nullptr;
        hipError_t e = L.wire_tiled ? launch_wire_tiled(c->d_spdif_words, dst, (uint32_t)(s1 - s0), (uint32_t)c->sm.n_pairs, (uint32_t)L.frames, row, q1 - q0, pos, rates,
                                                        L.mem != CallMem::Device, c->hs, stream_pos)
                     : L.wire_encoder ? launch_wire(c->d_spdif_words, dst, (uint32_t)(s1 - s0), (uint32_t)c->sm.n_pairs, (uint32_t)L.frames, pos, rates, L.mem != CallMem::Device,
                                                    c->hs, stream_pos)
                                      : launch_spdif(false, c->d_spdif_words, dst, (uint32_t)(s1 - s0), (uint32_t)c->sm.n_pairs, (uint32_t)L.frames, row, q1 - q0, pos, 0u, rates,
                                                     c->hs, stream_pos);
        if (e != hipSuccess) return fail(c, DSPI_E_HIP, std::string(L.wire_encoder ? "wire encoder launch: " : "spdif encoder launch: ") + hipGetErrorString(e));
    }
    return 0;
}

// sticky clip flags of every stream (global_status.clip_flags, usb_audio.c:2427-2443), after the chain on the same stream
static int gather_clip(dspi_ctx *c, uint16_t *dst) {
    hipError_t e = launch_clip_gather(c->d_state, c->n_streams, (uint32_t)c->sm.row, (uint32_t)c->sm.n_slots, (uint32_t)c->sm.clip, dst, c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("clip gather launch: ") + hipGetErrorString(e));
}

// ---- dspi_process_pdm: the PDM words of a call (null in the three paths below: dspi_process) ----
struct PdmCall {
    uint32_t *words;          // the caller's
    const PdmWork *work;      // the call's work list (dspi_pdmlife.h); its device copy is c->d_pdm_list
};
// the work list as the rule gives it for this call, and its device copy: built and uploaded only when something has changed it.  The
// words go up through the move calls' pinned area, behind its event, and on the context's stream: behind every launch that reads the old copy.
static int pdm_prepare(dspi_ctx *c, PdmCall &pc) {
    int rc = pdm_state(c);
    if (rc) return rc;
    // (in the fade mode a stream that fades, or is about to, stays listed: dspi_pdmfade.h says beside the list what its lane does)
    const auto sub_on = [c](uint32_t s) { return c->images[(size_t)c->stream_image[s]]->core1_mode == 1; };
    const PdmWork &w = c->pdm_life.plan(host_activity(c), [c, &sub_on](uint32_t s) { return c->pdm_fade.wants(c->pdm_life, s, sub_on(s)); });
    c->pdm_fade.plan(c->pdm_life, sub_on);
    pc.work = &w;
    if (c->pdm_life.uploaded || w.list.empty()) return 0;
    const bool aux = c->pdm_fade.any_aux;      // the aux words go up behind the list, only when one of them says anything
    if ((rc = upload_via_move_area(c, c->d_pdm_list, "hipHostMalloc failed (PDM work list)", {{w.list.data(), w.list.size() * 4}, {c->pdm_fade.aux.data(), aux ? w.list.size() * 4 : 0}}))) return rc;
    c->pdm_life.uploaded = true;
    return 0;
}
// the ONE modulator launch over the listed streams of [s0, s1), behind the chain launches of those rows; `sub` and `words` are addressed
// by absolute stream.  Nobody listed there: no launch.
static int launch_pdm_streams(dspi_ctx *c, const PdmCall &pc, const CallLayout &L, bool tiled, const int32_t *sub, uint32_t *words, size_t s0, size_t s1) {
    const std::pair<size_t, size_t> r = pc.work->range((uint32_t)s0, (uint32_t)s1);
    hipError_t e;
    if (c->pdm_fade.on)      // (each chunk of the staged path gets its slice of both arrays)
        e = launch_pdm_list_fade(tiled, c->d_pdm, sub, words, c->d_pdm_list + r.first, c->pdm_fade.any_aux ? c->d_pdm_list + pc.work->list.size() + r.first : nullptr, c->d_pdm_base,
                                 (uint32_t)(r.second - r.first), c->n_streams, (uint32_t)L.frames, (uint32_t)c->sm.row, c->hs);
    else e = launch_pdm_list(tiled, c->d_pdm, sub, words, c->d_pdm_list + r.first, (uint32_t)(r.second - r.first), c->n_streams, (uint32_t)L.frames, (uint32_t)c->sm.row, c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("pdm modulator launch: ") + hipGetErrorString(e));
}
// where the chain leaves the Q28 sub words of a dspi_process_pdm call whose caller passed no `sub`: the library's scratch (device memory)
static int pdm_sub_scratch(dspi_ctx *c, const CallLayout &L) { return ensure(c, c->d_sub, L.sub_scratch.bytes); }

// ---- where the chain's input comes from: the front end of an audio call, built on the public call's stack ----
// Whatever the kind, the call is planned as the PCM call it becomes (24 bit; plan_call knows nothing of the kinds); only the way its `pcm` area
// is filled differs.  Pcm: the caller's buffer as it stands.  Every other kind fills d_mixed on the device route; Mixed alone has host routes too.
struct CallFront {
    enum Kind : uint8_t { Pcm, Mixed, Linked, Patched, Packets };
    Kind kind = Pcm;
    bool wire = false;                     // out->pairs in the wire layout (process_call)
    const char *who = "dspi_process";      // the public call, for messages
    SpdifRx *rx = nullptr;                 // the records of the S/PDIF streams [n_streams], or null when none is served.  Mixed: in the call's memory; Linked, Patched: device memory
    const uint8_t *depths = nullptr;       // Mixed: 16 / 24, and in a dspi_process_sources call kSrcSpdif; Packets: 16 / 24.  The caller's, validated, like all that follows
    const uint64_t *offsets = nullptr;     // Mixed: [n_streams + 1] (dspi_intake.h; with S/PDIF runs dspi_spdifrx.h)
    const WireView *views = nullptr; uint32_t n_views = 0;      // Linked: the one view; Patched: [n_views], validated where an active LINK stream names them.  Wire words in device memory
    const Link *links = nullptr;           // Linked: [n_streams], host memory, validated for the entries that are served
    const PatchPlan *plan = nullptr;       // Patched (dspi_patch.h)
    const uint64_t *table = nullptr; uint32_t n_blocks = 0, block_len = 0;      // Packets: [n_streams][n_blocks], host memory, validated for the active streams
    bool table_on_device = false;          // Packets: the table is DEVICE memory (dspi_process_packets_resident), checked there or warranted by the caller
    bool host_capable() const { return kind == Pcm || kind == Mixed; }      // the others: the device route only
    bool reads_pcm_in() const { return kind != Linked && kind != Patched; }      // (Patched: `in` may be null, when no active stream has a run; Packets: the arena)
};
static bool rx_stream(const dspi_ctx *c, const CallFront &f, uint32_t s) { return f.depths[s] == kSrcSpdif && (!c->n_paused || c->active[s]); }

// THE owner of d_mixed_tab: every front end's table goes up here (through the pinned move area: the caller may reuse its own when the call
// returns), and what goes up is no mixed call's layout until intake_prepare, the one other writer of the cache's key, says that it is
static int upload_front_table(dspi_ctx *c, const char *why, std::initializer_list<std::pair<const void *, size_t>> parts) {
    c->mixed_frames = 0;
    return upload_via_move_area(c, c->d_mixed_tab, why, parts);
}
// Mixed: the path's scratch (d_mixed or d_mixed_up) and the device's table, which stays while the depths, the frame count and the intake's streams repeat
static int intake_prepare(dspi_ctx *c, const CallFront &f, uint64_t frames, DevBuf<uint8_t> &scratch, size_t scratch_bytes) {
    int rc = ensure(c, scratch, scratch_bytes);
    if (rc) return rc;
    const size_t n = c->n_streams;
    std::vector<uint32_t> mask;      // S/PDIF sources in the call: the intake's streams, behind the depths (padded to a word)
    if (f.rx) {
        mask.assign((n + 31) / 32, 0u);
        for (uint32_t s = 0; s < n; s++) if (f.depths[s] != kSrcSpdif && (!c->n_paused || c->active[s])) mask[s >> 5] |= 1u << (s & 31u);
    }
    if (c->mixed_frames == frames && c->mixed_depths.size() == n && !memcmp(c->mixed_depths.data(), f.depths, n) && c->mixed_mask == mask) return 0;
    const uint32_t pad = 0;
    if ((rc = upload_front_table(c, "hipHostMalloc failed (mixed input table)", {{f.offsets, (n + 1) * 8}, {f.depths, n}, {&pad, (4 - n % 4) % 4}, {mask.data(), mask.size() * 4}}))) return rc;
    c->mixed_depths.assign(f.depths, f.depths + n); c->mixed_frames = frames; c->mixed_mask.swap(mask);
    return 0;
}
// the intake launch for streams [s0, s1): `src` holds the caller's bytes at their offsets, `dst` is what the chain reads
// rx (a call with an S/PDIF source): the records in DEVICE memory; the intake then serves the PCM streams and the receiver kernel the others
static int launch_intake_streams(dspi_ctx *c, uint64_t frames, const void *src, void *dst, size_t s0, size_t s1, SpdifRx *rx) {
    const uint8_t *const depths = reinterpret_cast<const uint8_t *>(c->d_mixed_tab + c->n_streams + 1);
    const uint32_t *const pcm_streams = reinterpret_cast<const uint32_t *>(depths + ((size_t)c->n_streams + 3) / 4 * 4);
    // (a call whose every active stream is an S/PDIF source has nothing for the intake)
    const bool any_pcm = !rx || std::any_of(c->mixed_mask.begin(), c->mixed_mask.end(), [](uint32_t w) { return w != 0; });
    hipError_t e = any_pcm ? launch_intake(src, c->d_mixed_tab, depths, rx ? pcm_streams : activity(c), dst, frames, (uint32_t)s0, (uint32_t)(s1 - s0), c->hs) : hipSuccess;
    if (e == hipSuccess && rx) e = launch_spdifrx(true, src, c->d_mixed_tab, depths, activity(c), rx, dst, frames, (uint32_t)s0, (uint32_t)(s1 - s0), c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("intake launch: ") + hipGetErrorString(e));
}

// ---- Linked, and dspi_wire_decode (dspi_link.h): the call's links ----
// the device's table of a call's links: n + 1 offsets (what launch_spdifrx reads for the S/PDIF lines of a stream-major view), the n links, the n
// kinds as bytes; an entry that is not served (a paused stream, a hole) has kind NONE there, so no kernel looks at its line
struct LinkTab { const uint64_t *offsets; const Link *links; const uint8_t *kinds; bool any_spdif, any_i2s; };
static int link_table(dspi_ctx *c, const WireView &v, const Link *links, uint32_t n, const uint8_t *active, LinkTab &t) {
    std::vector<uint64_t> offsets((size_t)n + 1, 0u);
    std::vector<Link> dl(n);
    std::vector<uint8_t> kinds(((size_t)n + 7) / 8 * 8, 0u);
    t.any_spdif = t.any_i2s = false;
    for (uint32_t i = 0; i < n; i++) {
        const bool on = (!active || active[i]) && links[i].kind != kLinkNone;
        dl[i] = on ? links[i] : Link{0u, kLinkNone};
        kinds[i] = (uint8_t)dl[i].kind;
        if (on && !v.tile_streams) offsets[i] = link_region(links[i].line, v.n_frames) * 4u;
        t.any_spdif = t.any_spdif || dl[i].kind == kLinkSpdif;
        t.any_i2s = t.any_i2s || dl[i].kind == kLinkI2s;
    }
    if (int rc = upload_front_table(c, "hipHostMalloc failed (link table)", {{offsets.data(), offsets.size() * 8}, {dl.data(), (size_t)n * 8}, {kinds.data(), kinds.size()}})) return rc;
    t.offsets = c->d_mixed_tab;
    t.links = reinterpret_cast<const Link *>(c->d_mixed_tab + n + 1);
    t.kinds = reinterpret_cast<const uint8_t *>(c->d_mixed_tab + 2 * (size_t)n + 1);
    return 0;
}
// what this context's stream does from here on runs behind what the producer of a view has queued so far (a view without one, the context's
// own, a host-only producer: nothing to wait for).  "The producer's stream has come this far": recorded there, waited for here
static int wait_for_producer(dspi_ctx *c, const WireView &v) {
    dspi_ctx *const prod = static_cast<dspi_ctx *>(v.producer);
    if (!prod || prod == c || prod->device == DSPI_DEVICE_NONE) return 0;
    if (!c->ev_link) HIPCK(c, hipEventCreateWithFlags(&c->ev_link, hipEventDisableTiming));
    HIPCK(c, hipEventRecord(c->ev_link, prod->hs));
    HIPCK(c, hipStreamWaitEvent(c->hs, c->ev_link, 0));
    return 0;
}
// Linked: the link receivers from another call's wire buffer, behind the producer's work
static int launch_links(dspi_ctx *c, const CallFront &f, uint64_t frames) {
    const WireView &v = *f.views;
    LinkTab t;
    int rc = link_table(c, v, f.links, c->n_streams, host_activity(c), t);
    if (rc || (rc = wait_for_producer(c, v))) return rc;
    const hipError_t e = launch_linkrx(true, v.wire, t.links, t.offsets, t.kinds, nullptr, f.rx, c->d_mixed, (uint32_t)frames, v.n_pairs, v.tile_streams, c->n_streams, t.any_spdif, t.any_i2s, c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("link receiver launch: ") + hipGetErrorString(e));
}

// Patched (dspi_patch.h), the union of the two: at most one intake launch, one receiver launch over `in` (device memory, or null when no active
// stream has a run), two launches per stream-major view and one for all tiled views; each view's kernels behind its producer's work
static int launch_patched(dspi_ctx *c, const CallFront &f, const void *in, uint64_t frames) {
    const PatchPlan &p = *f.plan;
    int rc = upload_front_table(c, "hipHostMalloc failed (patch table)", {{p.table.data(), p.table.size() * 8}});
    if (rc) return rc;
    const uint64_t *const tab = c->d_mixed_tab;
    const uint8_t *const in_kinds = reinterpret_cast<const uint8_t *>(tab + p.in_kinds);
    hipError_t e = hipSuccess;
    if (p.any_pcm) e = launch_intake(in, tab + p.in_offsets, in_kinds, reinterpret_cast<const uint32_t *>(tab + p.pcm_mask), c->d_mixed, frames, 0u, c->n_streams, c->hs);
    if (e == hipSuccess && p.any_spdif_in) e = launch_spdifrx(true, in, tab + p.in_offsets, in_kinds, nullptr, f.rx, c->d_mixed, frames, 0u, c->n_streams, c->hs);
    if (e != hipSuccess) return fail(c, DSPI_E_HIP, std::string("intake launch: ") + hipGetErrorString(e));
    // one wait per DISTINCT producer that an active LINK stream's view names, all of them before the first kernel that reads a view
    for (uint32_t v = 0; v < f.n_views; v++) {
        bool seen = !p.view[v].used;      // (an unused view's producer is nobody's business)
        for (uint32_t u = 0; u < v; u++) seen = seen || (p.view[u].used && f.views[u].producer == f.views[v].producer);
        if (!seen && (rc = wait_for_producer(c, f.views[v]))) return rc;
    }
    for (uint32_t v = 0; v < f.n_views && e == hipSuccess; v++) {
        const PatchPlan::View &pv = p.view[v];
        if (!pv.used || f.views[v].tile_streams) continue;
        e = launch_linkrx(true, f.views[v].wire, tab + pv.links, tab + pv.offsets, reinterpret_cast<const uint8_t *>(tab + pv.kinds), nullptr, f.rx, c->d_mixed, (uint32_t)frames,
                          f.views[v].n_pairs, 0u, c->n_streams, pv.any_spdif, pv.any_i2s, c->hs);
    }
    if (e == hipSuccess && p.any_tiled) e = launch_patchrx(tab + p.cols, f.rx, c->d_mixed, (uint32_t)frames, c->n_streams, p.tiled_spdif, c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("patch receiver launch: ") + hipGetErrorString(e));
}

// Packets (dspi_packets.h): the table with the depths behind it, then the packet receiver over the caller's arena (device memory)
static int launch_packets(dspi_ctx *c, const CallFront &f, const void *arena) {
    // (a table on the device stays where it lies: only the depths go up)
    const size_t entries = (size_t)c->n_streams * f.n_blocks, up = f.table_on_device ? 0 : entries;
    if (int rc = upload_front_table(c, "hipHostMalloc failed (packet table)", {{f.table, up * 8}, {f.depths, c->n_streams}})) return rc;
    const uint64_t *const tab = c->d_mixed_tab;
    const hipError_t e = launch_packetrx(arena, f.table_on_device ? f.table : tab, reinterpret_cast<const uint8_t *>(tab + up), activity(c), c->d_mixed, c->n_streams, f.n_blocks, f.block_len, c->hs);
    return e == hipSuccess ? 0 : fail(c, DSPI_E_HIP, std::string("packet receiver launch: ") + hipGetErrorString(e));
}

// ---- the device route's front end, in two steps (process_call and process_device; the dspi_debug_*_intake calls run the same two) ----
// what must exist before the first launch, so that a call which cannot have it runs nothing: Mixed, the path's scratch and the table (on the
// direct path the CPU widens into the pinned area: nothing); the other kinds, the scratch their receivers write
static int front_prepare(dspi_ctx *c, const CallFront &f, CallMem mem, uint64_t frames, size_t pcm_bytes) {
    if (f.kind == CallFront::Pcm || mem == CallMem::Direct) return 0;
    if (f.kind != CallFront::Mixed) return ensure(c, c->d_mixed, pcm_bytes);
    return mem == CallMem::Device ? intake_prepare(c, f, frames, c->d_mixed, pcm_bytes) : intake_prepare(c, f, frames, c->d_mixed_up, (size_t)f.offsets[c->n_streams]);
}
// the launches that fill d_mixed from `pcm_in` (Pcm: none); *chain_pcm: what the chain then reads
static int front_launch(dspi_ctx *c, const CallFront &f, const void *pcm_in, uint64_t frames, const void **chain_pcm) {
    *chain_pcm = f.kind == CallFront::Pcm ? pcm_in : c->d_mixed.get();
    switch (f.kind) {
    case CallFront::Pcm: break;
    case CallFront::Mixed: return launch_intake_streams(c, frames, pcm_in, c->d_mixed, 0, c->n_streams, f.rx);
    case CallFront::Linked: return launch_links(c, f, frames);
    case CallFront::Patched: return launch_patched(c, f, pcm_in, frames);
    case CallFront::Packets: return launch_packets(c, f, pcm_in);
    }
    return 0;
}

// ---- device buffers: the caller's own, asynchronous on the context's stream ----
static int process_device(dspi_ctx *c, const CallLayout &L, KArgs &a, const void *pcm_in, const dspi_out *out, uint16_t *clip_out, const PdmCall *pc, const CallFront &front) {
    a.pairs = out->pairs; a.sub = out->sub; a.peaks = out->peaks;
    int rc = 0;
    if (pc && !out->sub) { if ((rc = pdm_sub_scratch(c, L))) return rc; a.sub = c->d_sub; }
    if (L.spdif_two_pass && (rc = ensure(c, c->d_spdif_words, L.two_pass_bytes))) return rc;
    if ((rc = front_launch(c, front, pcm_in, L.frames, &a.pcm)) || (rc = launch_rows(c, a, L, 0, c->n_wg))) return rc;
    if (pc && (rc = launch_pdm_streams(c, *pc, L, a.tiled_out != 0, a.sub, pc->words, 0, c->n_streams))) return rc;
    return clip_out ? gather_clip(c, clip_out) : DSPI_OK;
}

// ---- small calls on host buffers: the drop-in as the firmware's main loop makes it, ONE packet per call (usb_audio_drain_ring,
// usb_audio.c:1326-1332).  Staged copies would cost four DMA round trips (~100 us) for a few KB; instead the kernels read the packet
// from, and write their words to, a pinned host area directly (fine-grained, GPU-visible: hipHostMalloc), so the call is two memcpys on
// the CPU, the launches, and a spin on the stream: its latency is the kernel's. ----
static int direct_area(dspi_ctx *c, size_t bytes) {
    if (bytes <= c->h_direct.cap) return 0;
    if (c->h_direct) HIPCK(c, hipStreamSynchronize(c->hs));      // (no launch may still be using the area that is about to be freed)
    HipAlloc a;
    const Mem m = devmem_grow_pinned(a, c->h_direct, bytes, std::max<size_t>(bytes, 64u << 10), true);
    return m == Mem::Ok ? 0 : mem_fail(c, m, a, "hipHostMalloc failed (direct host area)");
}

// What a direct call polls (round 6): a word in pinned host memory that the stream itself sets to the call's sequence number behind the
// launches (hipStreamWriteValue32) — a load per poll, no call into the runtime while waiting; hipStreamQuery where that is not available
// (DSPI_DIRECT_POLL=query forces it).  Allocated by the first direct call.
static void completion_word(dspi_ctx *c) {
    const char *e = getenv("DSPI_DIRECT_POLL");
    c->direct_flag = 0;
    if (e && !strcmp(e, "query")) return;
    HipAlloc a;
    if (devmem_grow_pinned(a, c->h_done, 64, 64, true) == Mem::Ok) { *c->h_done = 0u; c->direct_flag = 1; }
}

static int process_direct(dspi_ctx *c, const CallLayout &L, KArgs &a, const void *pcm_in, const dspi_out *out, uint16_t *clip_out, uint32_t flags,
                          std::chrono::steady_clock::time_point call_t0, const PdmCall *pc, const CallFront &front) {
    int rc = direct_area(c, L.direct_bytes);
    if (rc) return rc;
    char *const h = c->h_direct, *const d = c->h_direct.device();
    std::vector<std::pair<uint32_t, SpdifRx>> rx_after;      // the records of the call's S/PDIF streams as the call leaves them: the caller's change when it succeeds
    if (front.kind == CallFront::Mixed) {      // the copy widens, or decodes, as it copies (a paused stream's bytes are not read, and nobody reads its run of the area)
        for (uint32_t s = 0; s < c->n_streams; s++) {
            if (c->n_paused && !c->active[s]) continue;
            uint8_t *const run = reinterpret_cast<uint8_t *>(h) + (size_t)s * L.pcm.per;
            const uint8_t *const src = static_cast<const uint8_t *>(pcm_in) + front.offsets[s];
            if (front.depths[s] == kSrcSpdif) {
                rx_after.emplace_back(s, front.rx[s]);
                spdifrx_line_cpu(&rx_after.back().second, src, L.frames, nullptr, run);
            } else intake_widen_cpu(run, src, front.depths[s], L.frames);
        }
    } else memcpy(h, pcm_in, L.pcm.bytes);
    a.pcm = d;
    if (out->pairs) a.pairs = reinterpret_cast<int32_t *>(d + L.pairs.off);
    if (out->sub) a.sub = reinterpret_cast<int32_t *>(d + L.sub.off);
    if (out->peaks) a.peaks = reinterpret_cast<uint16_t *>(d + L.peaks.off);
    if (pc && !out->sub) { if ((rc = pdm_sub_scratch(c, L))) return rc; a.sub = c->d_sub; }
    if (pc) for_unlisted_regions(c, L.pdm_words, *pc->work, [&](size_t at, size_t n) { memset(h + L.pdm_words.off + at, 0, n); });      // (unlisted streams' words stay unwritten: zeros, there only)
    if (flags & DSPI_OUT_ENABLED_ONLY) {      // (silent parts stay unwritten by the kernels: the caller finds zeros, the firmware's own fill)
        if (out->pairs) memset(h + L.pairs.off, 0, L.pairs.bytes);
        if (out->sub) memset(h + L.sub.off, 0, L.sub.bytes);
    }
    if (c->n_paused) {      // (paused streams' regions stay unwritten likewise: zeros, there only)
        if (out->pairs && !(flags & DSPI_OUT_ENABLED_ONLY)) for_paused_regions(c, L.pairs, [&](size_t at, size_t n) { memset(h + L.pairs.off + at, 0, n); });
        if (out->sub && !(flags & DSPI_OUT_ENABLED_ONLY)) for_paused_regions(c, L.sub, [&](size_t at, size_t n) { memset(h + L.sub.off + at, 0, n); });
        if (out->peaks) for_paused_regions(c, L.peaks, [&](size_t at, size_t n) { memset(h + L.peaks.off + at, 0, n); });
    }
    if (L.wire_tiled) for_absent_columns(c, L.pairs, [&](size_t at, size_t n) { memset(h + L.pairs.off + at, 0, n); });
    if ((L.spdif_two_pass && (rc = ensure(c, c->d_spdif_words, L.two_pass_bytes))) || (rc = launch_rows(c, a, L, 0, c->n_wg)) ||
        (pc && (rc = launch_pdm_streams(c, *pc, L, a.tiled_out != 0, a.sub, reinterpret_cast<uint32_t *>(d + L.pdm_words.off), 0, c->n_streams))) ||
        (clip_out && (rc = gather_clip(c, reinterpret_cast<uint16_t *>(d + L.clip.off))))) return rc;
    // the launches take tens of microseconds: polling answers within a microsecond of their end, a blocking wait adds a wake-up — but only
    // for as long as such launches can take: past the budget the call falls back to the blocking wait (a hung queue, or a host running
    // many contexts, must not pin a core).  The budget: the audio time the call carries (a caller in the firmware's rhythm has exactly
    // that long per call), never less than 300 us, never more than 50 ms; DSPI_DIRECT_SPIN_US (read at dspi_create) overrides it.
    // (The rare 0.5-10 ms calls — BENCH_r05 had one — are not this loop's: its clock check does not fire during them, the thread is off
    //  its core; profiles/r06_realtime_polling.md.)
    if (c->direct_flag < 0) completion_word(c);
    bool flagged = false;
    if (c->direct_flag == 1) {
        ++c->direct_seq;
        if (hipStreamWriteValue32(c->hs, c->h_done.device(), c->direct_seq, 0) == hipSuccess) flagged = true;
        else { (void)hipGetLastError(); c->direct_flag = 0; }      // (this runtime / device cannot: the stream is polled from here on)
    }
    hipError_t q = hipSuccess;
    const auto spin_t0 = std::chrono::steady_clock::now();
    const uint64_t audio_us = (uint64_t)L.frames * 1000000u / 44100u;      // (the slowest rate the firmware runs: an upper bound of the packet's time)
    const auto budget = std::chrono::microseconds(c->direct_spin_us ? (uint64_t)c->direct_spin_us : std::min<uint64_t>(50000u, std::max<uint64_t>(300u, audio_us)));
    uint32_t polls = 0;
    bool fell_back = false;
    if (flagged) {
        volatile const uint32_t *done = c->h_done;
        const uint32_t want = c->direct_seq;
        while (*done != want) {
            __builtin_ia32_pause();
            if ((++polls & 1023u) == 0 && std::chrono::steady_clock::now() - spin_t0 > budget) { q = hipStreamSynchronize(c->hs); fell_back = true; break; }
        }
        std::atomic_thread_fence(std::memory_order_acquire);      // the words the kernels wrote are read after the flag
    } else {
        while ((q = hipStreamQuery(c->hs)) == hipErrorNotReady) {
            if ((++polls & 63u) == 0 && std::chrono::steady_clock::now() - spin_t0 > budget) { q = hipStreamSynchronize(c->hs); fell_back = true; break; }
        }
    }
    {
        const auto t_end = std::chrono::steady_clock::now();
        const uint64_t enq = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(spin_t0 - call_t0).count();
        const uint64_t wait = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t_end - spin_t0).count();
        c->direct_stats[0]++;
        if (c->direct_stats[0] > 8) {      // (the context's first calls allocate the pinned area, build the launch lists, load the code objects: not the steady state)
            c->direct_stats[1] += fell_back ? 1u : 0u;
            c->direct_stats[2] = std::max(c->direct_stats[2], enq); c->direct_stats[3] = std::max(c->direct_stats[3], wait);
        }
        c->direct_stats[4] = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(budget).count();
    }
    if (q != hipSuccess) return fail(c, DSPI_E_HIP, std::string("stream: ") + hipGetErrorString(q));
    if (out->pairs) memcpy(out->pairs, h + L.pairs.off, L.pairs.bytes);
    if (out->sub) memcpy(out->sub, h + L.sub.off, L.sub.bytes);
    if (out->peaks) memcpy(out->peaks, h + L.peaks.off, L.peaks.bytes);
    if (clip_out) memcpy(clip_out, h + L.clip.off, L.clip.bytes);
    if (pc) memcpy(pc->words, h + L.pdm_words.off, L.pdm_words.bytes);
    for (const auto &r : rx_after) front.rx[r.first] = r.second;
    return DSPI_OK;
}

// ---- host buffers (the caller of usb_audio.c:1326-1332 is a host feeding packets): staged through device buffers.  The link moves
// 4 + 36 bytes per frame, the chain 100 times that, so the call is link-bound; what can be saved is the serialisation: the rows are
// cut into chunks and chunk i's D2H runs while chunk i+1 computes and chunk i+2 uploads (three streams, events).  The caller's
// buffers are pinned for the duration of the call (hipHostRegister: ~8 ms per GiB) so that the copies are asynchronous DMA; when
// that is refused (already registered, read-only mapping ...) the copies still work, just synchronously. ----
static int process_staged(dspi_ctx *c, const CallLayout &L, KArgs &a, const void *pcm_in, const dspi_out *out, uint16_t *clip_out, uint32_t flags, const PdmCall *pc, const CallFront &front) {
    const bool mixed = front.kind == CallFront::Mixed;
    int rc;
    if ((rc = ensure(c, c->d_in, L.pcm.bytes))) return rc;
    a.pcm = c->d_in;
    if (out->pairs) { if ((rc = ensure(c, c->d_pairs, L.pairs.bytes))) return rc; a.pairs = c->d_pairs; }
    if (out->sub) { if ((rc = ensure(c, c->d_sub, L.sub.bytes))) return rc; a.sub = c->d_sub; }
    if (out->peaks) { if ((rc = ensure(c, c->d_peaks, L.peaks.bytes))) return rc; a.peaks = c->d_peaks; }
    if (clip_out && (rc = ensure(c, c->d_clip, L.clip.bytes))) return rc;
    // dspi_process_pdm: the words' staging buffer is dspi_pdm_modulate's; without `sub` from the caller the chain writes one chunk's Q28 words
    // into the scratch (set per chunk, below: the kernels index by absolute stream)
    if (pc && ((rc = ensure(c, c->d_pdm_out, L.pdm_words.bytes)) || (!out->sub && (rc = pdm_sub_scratch(c, L))))) return rc;
    // DSPI_OUT_ENABLED_ONLY leaves the silent parts of pairs / sub unwritten: the staging buffers are copied back whole, so what the
    // caller finds there is zeros (the firmware's own fill), not stale staging memory
    if (flags & DSPI_OUT_ENABLED_ONLY) {
        if (a.pairs) HIPCK(c, hipMemsetAsync(a.pairs, 0, L.pairs.bytes, c->hs));
        if (a.sub) HIPCK(c, hipMemsetAsync(a.sub, 0, L.sub.bytes, c->hs));
    }
    // ... and the same for the regions of paused streams, which no kernel writes (peaks too): those regions only
    if (c->n_paused) {
        hipError_t me = hipSuccess;
        auto clear = [&](void *base) { return [&, base](size_t at, size_t n) { if (me == hipSuccess) me = hipMemsetAsync(static_cast<char *>(base) + at, 0, n, c->hs); }; };
        if (a.pairs && !(flags & DSPI_OUT_ENABLED_ONLY)) for_paused_regions(c, L.pairs, clear(a.pairs));
        if (a.sub && !(flags & DSPI_OUT_ENABLED_ONLY)) for_paused_regions(c, L.sub, clear(a.sub));
        if (a.peaks) for_paused_regions(c, L.peaks, clear(a.peaks));
        HIPCK(c, me);
    }
    if (L.wire_tiled) {
        hipError_t me = hipSuccess;
        for_absent_columns(c, L.pairs, [&](size_t at, size_t n) { me = hipMemsetAsync(reinterpret_cast<char *>(a.pairs) + at, 0, n, c->hs); });
        HIPCK(c, me);
    }
    if (pc) {      // ... and for the words of the streams the call does not list
        hipError_t me = hipSuccess;
        for_unlisted_regions(c, L.pdm_words, *pc->work, [&](size_t at, size_t n) { if (me == hipSuccess) me = hipMemsetAsync(reinterpret_cast<char *>(c->d_pdm_out.get()) + at, 0, n, c->hs); });
        HIPCK(c, me);
    }
    if (L.spdif_two_pass && (rc = ensure(c, c->d_spdif_words, L.two_pass_bytes))) return rc;
    // dspi_process_sources: the records of the call's S/PDIF streams go up ahead of the first launch and come down behind the last one (the
    // other entries of the caller's array are neither read nor written: zeros go up in their place)
    std::vector<SpdifRx> rx_stage;
    if (mixed && front.rx) {
        rx_stage.assign(c->n_streams, SpdifRx{});
        for (uint32_t s = 0; s < c->n_streams; s++) if (rx_stream(c, front, s)) rx_stage[s] = front.rx[s];
        if ((rc = ensure(c, c->d_rx, rx_stage.size() * sizeof(SpdifRx)))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_rx, rx_stage.data(), rx_stage.size() * sizeof(SpdifRx), hipMemcpyHostToDevice, c->hs));
    }
    const uint32_t n_chunks = L.n_chunks, row = (uint32_t)c->sm.row;
    // the caller's buffers and the staging buffers: a row range is one contiguous piece of each (tiled words: whole tiles; else streams)
    // (dspi_process_mixed: the caller's PCM is as long as its depths make it, and a chunk's piece of it goes up to the same place of d_mixed_up)
    CallBuffer pcm_b = L.pcm;
    if (mixed) pcm_b.bytes = (size_t)front.offsets[c->n_streams];
    struct Buf { void *host; void *dev; const CallBuffer &b; const char *what; bool pinned; };
    Buf bufs[5] = {{const_cast<void *>(pcm_in), mixed ? (void *)c->d_mixed_up : c->d_in, pcm_b, "H2D", false}, {out->pairs, a.pairs, L.pairs, "D2H pairs", false},
                   {out->sub, a.sub, L.sub, "D2H sub", false}, {out->peaks, a.peaks, L.peaks, "D2H peaks", false},
                   {pc ? pc->words : nullptr, c->d_pdm_out, L.pdm_words, "D2H pdm words", false}};
    if (n_chunks > 1)
        for (Buf &bf : bufs)
            if (bf.host && bf.b.bytes >= (1u << 20)) {
                bf.pinned = hipHostRegister(bf.host, bf.b.bytes, hipHostRegisterDefault) == hipSuccess;
                if (!bf.pinned) (void)hipGetLastError();
            }
    // (error paths too: no copy or kernel may still be in flight on memory that is about to be unregistered)
    auto unpin = [&]() {
        if (c->hs_in) (void)hipStreamSynchronize(c->hs_in);
        (void)hipStreamSynchronize(c->hs);
        if (c->hs_out) (void)hipStreamSynchronize(c->hs_out);
        for (Buf &bf : bufs) if (bf.pinned) { (void)hipHostUnregister(bf.host); bf.pinned = false; }
    };
    if (n_chunks > 1 && !c->hs_in) {
        if (hipStreamCreateWithFlags(&c->hs_in, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&c->hs_out, hipStreamNonBlocking) != hipSuccess) {
            unpin(); return fail(c, DSPI_E_HIP, "stream creation for the host-buffer pipeline failed");
        }
    }
    while (n_chunks > 1 && c->pipe_events.size() < 2 * (size_t)n_chunks) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { unpin(); return fail(c, DSPI_E_HIP, "event creation failed"); }
        c->pipe_events.push_back(e);
    }
    auto fail_hip = [&](hipError_t e, const char *what) { unpin(); return fail(c, DSPI_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
    hipError_t he;
    for (uint32_t ch = 0; ch < n_chunks; ch++) {
        const uint32_t r0 = ch * L.rows_per_chunk, r1 = std::min(c->n_wg, r0 + L.rows_per_chunk);
        const size_t s0 = (size_t)r0 * row, s1 = std::min((size_t)r1 * row, (size_t)c->n_streams);      // streams of the chunk
        auto copy = [&](const Buf &bf, hipMemcpyKind kind, hipStream_t s) {      // the chunk's piece of a buffer
            const size_t at = s0 * bf.b.per, n = ((bf.b.tile_cols ? (size_t)r1 * row : s1) - s0) * bf.b.per;
            char *h = static_cast<char *>(bf.host) + at, *d = static_cast<char *>(bf.dev) + at;
            return kind == hipMemcpyHostToDevice ? hipMemcpyAsync(d, h, n, kind, s) : hipMemcpyAsync(h, d, n, kind, s);
        };
        hipStream_t sin = n_chunks > 1 ? c->hs_in : c->hs, sout = n_chunks > 1 ? c->hs_out : c->hs;
        if (mixed) {
            uint64_t b0, b1;
            intake_row_range(front.offsets, c->n_streams, row, r0, r1, &b0, &b1);
            he = hipMemcpyAsync(c->d_mixed_up + b0, static_cast<const char *>(pcm_in) + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, sin);
        } else he = copy(bufs[0], hipMemcpyHostToDevice, sin);
        if (he != hipSuccess) return fail_hip(he, bufs[0].what);
        if (n_chunks > 1) {
            if ((he = hipEventRecord(c->pipe_events[2 * ch], sin)) != hipSuccess || (he = hipStreamWaitEvent(c->hs, c->pipe_events[2 * ch], 0)) != hipSuccess) return fail_hip(he, "event");
        }
        if (pc && !out->sub) a.sub = c->d_sub - s0 * L.frames;      // (the chunk's first stream or tile stands at the scratch's start, in both layouts)
        if (mixed && (rc = launch_intake_streams(c, L.frames, c->d_mixed_up, c->d_in, s0, s1, front.rx ? c->d_rx.get() : nullptr))) { unpin(); return rc; }
        if ((rc = launch_rows(c, a, L, r0, r1)) || (pc && (rc = launch_pdm_streams(c, *pc, L, a.tiled_out != 0, a.sub, c->d_pdm_out, s0, s1)))) { unpin(); return rc; }
        if (n_chunks > 1) {
            if ((he = hipEventRecord(c->pipe_events[2 * ch + 1], c->hs)) != hipSuccess || (he = hipStreamWaitEvent(sout, c->pipe_events[2 * ch + 1], 0)) != hipSuccess) return fail_hip(he, "event");
        }
        for (int k = 1; k < 5; k++)
            if (bufs[k].host && (he = copy(bufs[k], hipMemcpyDeviceToHost, sout)) != hipSuccess) return fail_hip(he, bufs[k].what);
    }
    if (clip_out) {
        if ((rc = gather_clip(c, c->d_clip))) { unpin(); return rc; }
        if ((he = hipMemcpyAsync(clip_out, c->d_clip, L.clip.bytes, hipMemcpyDeviceToHost, c->hs)) != hipSuccess) return fail_hip(he, "D2H clip flags");
    }
    if (!rx_stage.empty() && (he = hipMemcpyAsync(rx_stage.data(), c->d_rx, rx_stage.size() * sizeof(SpdifRx), hipMemcpyDeviceToHost, c->hs)) != hipSuccess) return fail_hip(he, "D2H receiver records");
    if (n_chunks > 1) {
        if ((he = hipStreamSynchronize(c->hs_out)) != hipSuccess) return fail_hip(he, "sync");
        if ((he = hipStreamSynchronize(c->hs_in)) != hipSuccess) return fail_hip(he, "sync");
    }
    if ((he = hipStreamSynchronize(c->hs)) != hipSuccess) return fail_hip(he, "sync");
    unpin();
    for (uint32_t s = 0; s < (uint32_t)rx_stage.size(); s++) if (rx_stream(c, front, s)) front.rx[s] = rx_stage[s];
    return DSPI_OK;
}

// ---- what the audio calls refuse, each rule in one place.  The rules are building blocks: every public call applies them in the order its
// own contract in include/dspi.h numbers, which the CPU tests pin ----
// The flags, two rules.  process_call applies them where dspi_process always has (the bits first of all, the combinations behind the
// host-only context's refusal: tests/test_capi.py pins that order); dspi_process_mixed applies both ahead of its own refusals, as its
// contract orders them.  A new flag rule goes INTO one of the two.
static int check_flag_bits(dspi_ctx *c, uint32_t flags) {
    // undefined flag bits are refused, not ignored: a later ABI may give them a meaning that reads further members of dspi_out
    constexpr uint32_t kKnownFlags = DSPI_MEM_DEVICE | DSPI_OUT_TILED | DSPI_OUT_ENABLED_ONLY | DSPI_OUT_I2S_SLOTS | DSPI_OUT_SPDIF | DSPI_OUT_CLIP_FLAGS;
    return (flags & ~kKnownFlags) ? fail(c, DSPI_E_INVAL, "dspi_process: undefined flag bits") : 0;
}
static int check_flag_combinations(dspi_ctx *c, uint32_t flags) {
    if ((flags & DSPI_OUT_SPDIF) && (flags & (DSPI_OUT_TILED | DSPI_OUT_I2S_SLOTS))) return fail(c, DSPI_E_INVAL, "DSPI_OUT_SPDIF goes with neither DSPI_OUT_TILED nor DSPI_OUT_I2S_SLOTS");
    return 0;
}
// does an active stream's parameter object carry an I2S slot (dspi_wire.h)?  From the host's objects and its record of pauses: no commit needed
static bool wire_slots_in_play(const dspi_ctx *c) {
    std::vector<uint32_t> image_i2s(c->images.size(), 0u);
    for (size_t i = 0; i < c->images.size(); i++) if (c->images[i]) image_i2s[i] = wire_i2s_mask(c->images[i]->output_types, (uint32_t)c->sm.n_pairs);
    return wire_any_i2s(c->stream_image.data(), c->n_streams, host_activity(c), image_i2s.data());
}
// The flag preamble of the calls that take DSPI_OUT_WIRE as a flag: *wire and the flags process_call gets (DSPI_OUT_WIRE stripped; with it
// DSPI_OUT_SPDIF, which the wire layout implies, and the flags held to dspi_process_devices' rule).  device_only (dspi_process_linked,
// _patched, _packets): DSPI_MEM_DEVICE is required, refused first of all, and the two rules above follow at once.  dspi_process_sources takes
// host memory too, and leaves the two rules to mixed_call, which applies them behind its own argument refusals
static int front_flags(dspi_ctx *c, const char *who, uint32_t *flags, bool *wire, bool device_only) {
    if (device_only && !(*flags & DSPI_MEM_DEVICE)) return fail(c, DSPI_E_INVAL, std::string(who) + ": DSPI_MEM_DEVICE is required");
    *wire = *flags & DSPI_OUT_WIRE;
    *flags &= ~DSPI_OUT_WIRE;
    if (*wire && !devices_process_flags_ok(*flags))
        return fail(c, DSPI_E_INVAL, std::string(who) + ": with DSPI_OUT_WIRE the flags are DSPI_MEM_DEVICE, DSPI_OUT_TILED, DSPI_OUT_ENABLED_ONLY and DSPI_OUT_CLIP_FLAGS");
    int rc;
    if (device_only && ((rc = check_flag_bits(c, *flags)) || (!*wire && (rc = check_flag_combinations(c, *flags))))) return rc;
    if (*wire) *flags |= DSPI_OUT_SPDIF;
    return 0;
}
// The lengths of a call
static int check_lengths(dspi_ctx *c, const char *who, uint32_t n_blocks, uint32_t block_len) {
    return (n_blocks == 0 || block_len == 0 || block_len > DSPI_MAX_BLOCK_LEN) ? refuse_lengths(c, who) : 0;
}
// The one case in which a 16-bit sample and its widened twin part ways (dspi_intake.h), refused, not approximated: an active stream whose
// entry of `kinds` is 16 with a preamp below 2^-103 on the float chain
static int check_widening(dspi_ctx *c, const char *who, const uint8_t *kinds, const uint8_t *active) {
    if (!c->flavor) return 0;
    for (uint32_t s = 0; s < c->n_streams; s++) {
        if (kinds[s] != 16 || (active && !active[s])) continue;
        for (const float p : readable(c, (int32_t)s).preamp_linear) {
            uint32_t w; memcpy(&w, &p, 4);
            if (intake_preamp_breaks_widening(w))
                return fail(c, DSPI_E_UNSUPPORTED, std::string(who) + ": stream " + std::to_string(s) + " takes 16-bit input with a preamp below 2^-103, where widening to 24 bit is not exact");
        }
    }
    return 0;
}

// ---- the one body of every audio call ----
// pcm_in: what the front end reads (front.reads_pcm_in(): required exactly then), at bit_depth where the front is Pcm; every other kind is the
// 24-bit call it becomes.  pdm_words: dspi_process_pdm's words, or null.  front: where the chain's input comes from (CallFront; its public call
// has refused what it refuses about its own arguments) and front.wire: out->pairs in the wire layout, the flags carrying DSPI_OUT_SPDIF, which
// that layout implies; with DSPI_OUT_TILED beside it (the callers have applied their own flag rule, dspi_wire.h) in the tiled wire layout
static int process_call(dspi_ctx *c, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags, const CallFront &front) {
    if (!c || !out || (!pcm_in && front.reads_pcm_in())) return DSPI_E_INVAL;
    int rc = check_flag_bits(c, flags);
    if (rc) return rc;
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    if ((bit_depth != 16 && bit_depth != 24) || n_blocks == 0 || block_len == 0 || block_len > DSPI_MAX_BLOCK_LEN)
        return fail(c, DSPI_E_INVAL, "bit_depth must be 16/24, 1 <= block_len <= 192, n_blocks >= 1");
    const auto call_t0 = std::chrono::steady_clock::now();
    HIPCK(c, hipSetDevice(c->device));
    if ((rc = commit_params(c)) || (rc = check_leveller_alphas(c, block_len))) return rc;

    // DSPI_OUT_CLIP_FLAGS: the caller's dspi_out has the ABI-7 member `clip_flags`
    uint16_t *const clip_out = (flags & DSPI_OUT_CLIP_FLAGS) ? out->clip_flags : nullptr;
    CallInput in;
    in.n_streams = c->n_streams; in.n_wg = c->n_wg; in.row = (uint32_t)c->sm.row; in.n_ch = (uint32_t)c->sm.n_ch; in.n_out = (uint32_t)c->sm.n_out;
    in.n_pairs = (uint32_t)c->sm.n_pairs; in.n_blocks = n_blocks; in.block_len = block_len; in.bit_depth = (uint32_t)bit_depth; in.flags = flags;
    in.pairs = out->pairs; in.sub = out->sub; in.peaks = out->peaks; in.clip = clip_out; in.no_direct = c->no_direct;
    in.all_latency = c->flavor != 0; in.spdif_per_stream = c->spdif_ps.on; in.pdm_words = pdm_words != nullptr;
    const bool tiled = flags & DSPI_OUT_TILED, spdif = flags & DSPI_OUT_SPDIF;
    in.wire_tiled = front.wire && tiled;                           // always two passes: there is no fused tiled encoder
    in.wire_slots = front.wire && !tiled && wire_slots_in_play(c);      // none in play: the call IS the DSPI_OUT_SPDIF call, route and bytes
    for (const PathInfo &pi : kPaths)
        if (pi.group != PathGroup::Latency && !c->plan.items[(int)pi.path].empty()) in.all_latency = false;
    const CallLayout L = plan_call(in);
    if (!front.wire && (rc = check_flag_combinations(c, flags))) return rc;
    if (L.wire_tiled && L.frames > kWireTiledMaxFrames) return fail(c, DSPI_E_UNSUPPORTED, "dspi_process_devices: a tiled call carries at most 2 097 120 frames");
    if (L.spdif_two_pass && c->spdif_ps.on && (rc = upload_spdif_pos(c))) return rc;
    PdmCall pdm{pdm_words, nullptr};
    const PdmCall *const pc = pdm_words ? &pdm : nullptr;
    if (pc && (rc = pdm_prepare(c, pdm))) return rc;
    if (L.mem != CallMem::Device && !front.host_capable()) return fail(c, DSPI_E_INVAL, std::string(front.who) + ": device memory only");
    if ((rc = front_prepare(c, front, L.mem, L.frames, L.pcm.bytes))) return rc;

    KArgs a{};
    a.img = c->d_images; a.stream_image = c->d_stream_image; a.vals = c->d_vals;
    a.state = c->d_state; a.dlines = c->d_dlines; a.ring = c->d_ring;
    a.n_streams = c->n_streams; a.n_blocks = n_blocks; a.block_len = block_len; a.bit_depth = (uint32_t)bit_depth;
    a.tiled_out = tiled ? 1u : 0u;
    a.fma = c->fma ? 1u : 0u;
    a.no_emit_lines = c->no_emit_lines ? 1u : 0u;
    // (two-pass S/PDIF: the encoder reads the WHOLE scratch chunk, so the chain must write the silent pairs' zero words there as well)
    a.skip_silent = ((flags & DSPI_OUT_ENABLED_ONLY) && !L.spdif_two_pass) ? 1u : 0u;
    a.i2s_slots = (flags & DSPI_OUT_I2S_SLOTS) ? 1u : 0u;
    if (spdif && !in.wire_tiled) { a.spdif = L.spdif_two_pass ? 0u : 1u; a.spdif_pos = c->spdif_pos; }      // (the fused encoder is stream-major)
    if (c->flavor && !tiled) {      // stream-major layout, packed kernel: the mini lines of the outputs whose rows do not reach the emit wave through their delay line (dspi_chain_pk.inc)
        const size_t xb = (size_t)c->n_wg * 3 * kMaxOut * kChunk * c->sm.row * 4;
        if ((rc = ensure(c, c->d_xwords, xb))) return rc;
        a.xwords = c->d_xwords;
    }

    switch (L.mem) {
    case CallMem::Device: rc = process_device(c, L, a, pcm_in, out, clip_out, pc, front); break;
    case CallMem::Direct: rc = process_direct(c, L, a, pcm_in, out, clip_out, flags, call_t0, pc, front); break;
    case CallMem::Staged: rc = process_staged(c, L, a, pcm_in, out, clip_out, flags, pc, front); break;
    }
    if (rc == DSPI_OK && pc) { c->pdm_life.commit(); c->pdm_fade.commit(c->pdm_life, (uint32_t)L.frames); }      // a failed call leaves the running bytes and the fade positions alone
    if (rc == DSPI_OK && spdif) {      // a failed call leaves the block positions alone
        c->spdif_pos = (uint32_t)((c->spdif_pos + L.frames) % 192u);
        if (c->spdif_ps.on) c->spdif_ps.advance(L.frames);      // every stream that was active in the call; the paused ones hold their own
    }
    return rc;
}

int dspi_process(dspi_ctx *c, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t flags) {
    return process_call(c, pcm_in, bit_depth, n_blocks, block_len, out, nullptr, flags, CallFront{});
}

int dspi_process_pdm(dspi_ctx *c, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags) {
    if (!c || !pdm_words) return DSPI_E_INVAL;
    return process_call(c, pcm_in, bit_depth, n_blocks, block_len, out, pdm_words, flags, CallFront{});
}

// ---- S/PDIF and I2S slots in one call, per device (dspi_wire.h: the layout and the rules; dspi_wire.hip: the encoder) ----
int dspi_process_wire(dspi_ctx *c, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (!wire_process_flags_ok(flags)) return fail(c, DSPI_E_INVAL, "dspi_process_wire: the flags are DSPI_MEM_DEVICE, DSPI_OUT_ENABLED_ONLY and DSPI_OUT_CLIP_FLAGS");
    return process_call(c, pcm_in, bit_depth, n_blocks, block_len, out, pdm_words, flags | DSPI_OUT_SPDIF, CallFront{CallFront::Pcm, true});
}

int dspi_wire_encode(dspi_ctx *c, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos, uint32_t *wire, uint32_t flags) {
    if (!c || !pairs || !wire || !block_pos || n_frames == 0) return DSPI_E_INVAL;
    if (!wire_encode_flags_ok(flags)) return fail(c, DSPI_E_INVAL, "dspi_wire_encode: the only flag is DSPI_MEM_DEVICE");
    const bool dev = flags & DSPI_MEM_DEVICE;
    // host positions are validated before anything is launched; device positions are the kernel's to reduce modulo 192
    if (!dev) for (uint32_t s = 0; s < c->n_streams; s++) if (block_pos[s] >= kSpdifBlock) return fail(c, DSPI_E_INVAL, "dspi_wire_encode: a position is 0..191");
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    const size_t in_b = (size_t)c->n_streams * c->sm.n_pairs * n_frames * 8, out_b = in_b * 2, pos_b = (size_t)c->n_streams * 4;
    const int32_t *d_in = pairs;
    uint32_t *d_out = wire;
    const uint32_t *d_pos = block_pos;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_in, in_b)) || (rc = ensure(c, c->d_spdif_out, out_b)) ||
            (rc = ensure(c, c->d_spdif_vpos, pos_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_in, pairs, in_b, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, hipMemcpyAsync(c->d_spdif_vpos, block_pos, pos_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_spdif_in; d_out = c->d_spdif_out; d_pos = c->d_spdif_vpos;
    }
    // every stream's types and rate are its own image's: committed first (unaware of pauses, like dspi_spdif_encode_v)
    if ((rc = commit_params(c))) return rc;
    // (host buffers: the staging buffer comes back whole, so the encoder zeroes the I2S regions' second halves there)
    HIPCK(c, launch_wire(d_in, d_out, c->n_streams, (uint32_t)c->sm.n_pairs, n_frames, 0u, SpdifRates{c->d_images, c->d_stream_image, 0u}, !dev, c->hs, d_pos));
    return dev ? DSPI_OK : stage_down(c, wire, c->d_spdif_out, out_b);
}

// ---- 16- and 24-bit devices in one call (dspi_intake.h: the layout and why widening is exact; dspi_intake.hip: the kernel) ----
// what both calls refuse about their arguments, in dspi_process's words
// sources: the entries are those of dspi_process_sources (dspi_spdifrx.h), DSPI_SRC_SPDIF among them
static int mixed_check(dspi_ctx *c, const uint8_t *depths, uint32_t n_blocks, uint32_t block_len, const char *who, bool sources = false) {
    const uint32_t bad = sources ? sources_check(depths, c->n_streams) : intake_check_depths(depths, c->n_streams);
    if (bad < c->n_streams && sources) return fail(c, DSPI_E_INVAL, std::string(who) + ": the source of stream " + std::to_string(bad) + " is none of DSPI_SRC_PCM16, DSPI_SRC_PCM24, DSPI_SRC_SPDIF");
    if (bad < c->n_streams) return fail(c, DSPI_E_INVAL, std::string(who) + ": the depth of stream " + std::to_string(bad) + " is neither 16 nor 24");
    return check_lengths(c, who, n_blocks, block_len);
}

int dspi_mixed_pcm_bytes(const dspi_ctx *c, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len, uint64_t *total_bytes, uint64_t *offsets) {
    if (!c || !bit_depths) return DSPI_E_INVAL;
    int rc = mixed_check(const_cast<dspi_ctx *>(c), bit_depths, n_blocks, block_len, "dspi_mixed_pcm_bytes");
    if (rc) return rc;
    if (!intake_offsets(bit_depths, c->n_streams, (uint64_t)n_blocks * block_len, total_bytes, offsets)) return fail(const_cast<dspi_ctx *>(c), DSPI_E_INVAL, "dspi_mixed_pcm_bytes: the buffer's size overflows");
    return DSPI_OK;
}

// the one body of dspi_process_mixed, (wire: out->pairs in the wire layout, the flags already held to its own rule) dspi_process_devices and
// (sources: bit_depths holds sources, rx the caller's records) dspi_process_sources, which without an S/PDIF entry is one of the two
static int mixed_call(dspi_ctx *c, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags,
                      const char *who, bool wire, bool sources = false, dspi_spdif_rx *rx = nullptr) {
    if (!c || !pcm_in || !bit_depths || !out) return DSPI_E_INVAL;
    int rc = mixed_check(c, bit_depths, n_blocks, block_len, who, sources);
    if (rc) return rc;
    const bool spdif_in = sources && sources_any_spdif(bit_depths, c->n_streams);
    // every entry equal: the call IS dspi_process / dspi_process_pdm / dspi_process_wire at that depth (which refuses a bad flag bit and a host-only context itself)
    if (const uint8_t depth = spdif_in ? 0 : intake_uniform_depth(bit_depths, c->n_streams))
        return process_call(c, pcm_in, depth, n_blocks, block_len, out, pdm_words, flags, CallFront{CallFront::Pcm, wire});
    if ((rc = check_flag_bits(c, flags)) || (!wire && (rc = check_flag_combinations(c, flags)))) return rc;
    std::vector<uint64_t> offsets((size_t)c->n_streams + 1);
    CallFront mx{CallFront::Mixed, wire, who, nullptr, bit_depths, offsets.data()};
    if (spdif_in) {      // what an S/PDIF source asks of the call's arguments
        if (!rx) return fail(c, DSPI_E_INVAL, std::string(who) + ": an S/PDIF source needs the receiver records (rx)");
        mx.rx = reinterpret_cast<SpdifRx *>(rx);
        if (flags & DSPI_MEM_DEVICE) {
            if (reinterpret_cast<uintptr_t>(pcm_in) % 16u) return fail(c, DSPI_E_INVAL, std::string(who) + ": with an S/PDIF source a device input is 16-byte aligned");
            if (reinterpret_cast<uintptr_t>(rx) % 4u) return fail(c, DSPI_E_INVAL, std::string(who) + ": device receiver records are 4-byte aligned");
        } else
            for (uint32_t s = 0; s < c->n_streams; s++)
                if (rx_stream(c, mx, s) && mx.rx[s].sync > kRxBlock) return fail(c, DSPI_E_INVAL, std::string(who) + ": the record of stream " + std::to_string(s) + " has sync > 192");
    }
    if (!(sources ? sources_offsets(bit_depths, c->n_streams, (uint64_t)n_blocks * block_len, nullptr, offsets.data())
                  : intake_offsets(bit_depths, c->n_streams, (uint64_t)n_blocks * block_len, nullptr, offsets.data()))) return fail(c, DSPI_E_INVAL, std::string(who) + ": the buffer's size overflows");
    if ((rc = check_widening(c, who, bit_depths, host_activity(c)))) return rc;
    return process_call(c, pcm_in, 24, n_blocks, block_len, out, pdm_words, flags, mx);
}

int dspi_process_mixed(dspi_ctx *c, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags) {
    return mixed_call(c, pcm_in, bit_depths, n_blocks, block_len, out, pdm_words, flags, "dspi_process_mixed", false);
}

// ---- every property of a device its host decides, in one call: depth vector, wire words, either layout (dspi_wire.h: the tiled wire layout
// and the flag rule; dspi_wire_tiled.hip: its encoder) ----
int dspi_process_devices(dspi_ctx *c, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (!devices_process_flags_ok(flags)) return fail(c, DSPI_E_INVAL, "dspi_process_devices: the flags are DSPI_MEM_DEVICE, DSPI_OUT_TILED, DSPI_OUT_ENABLED_ONLY and DSPI_OUT_CLIP_FLAGS");
    return mixed_call(c, pcm_in, bit_depths, n_blocks, block_len, out, pdm_words, flags | DSPI_OUT_SPDIF, "dspi_process_devices", true);
}

// ---- S/PDIF input (dspi_spdifrx.h: the subframe, the record, the rule and the layout; dspi_spdifrx.hip: the receiver kernel) ----
static_assert(sizeof(dspi_spdif_rx) == sizeof(SpdifRx) && offsetof(dspi_spdif_rx, c_bits) == offsetof(SpdifRx, c_bits) && offsetof(dspi_spdif_rx, hold) == offsetof(SpdifRx, hold) &&
              offsetof(dspi_spdif_rx, sync) == offsetof(SpdifRx, sync) && offsetof(dspi_spdif_rx, coding_errors) == offsetof(SpdifRx, coding_errors), "include/dspi.h and dspi_spdifrx.h: one record");
static_assert(DSPI_SRC_SPDIF == kSrcSpdif && DSPI_SRC_PCM16 == 16 && DSPI_SRC_PCM24 == 24, "include/dspi.h and dspi_spdifrx.h: one set of sources");

int dspi_sources_bytes(const dspi_ctx *c, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len, uint64_t *total_bytes, uint64_t *offsets) {
    if (!c || !sources) return DSPI_E_INVAL;
    int rc = mixed_check(const_cast<dspi_ctx *>(c), sources, n_blocks, block_len, "dspi_sources_bytes", true);
    if (rc) return rc;
    if (!sources_offsets(sources, c->n_streams, (uint64_t)n_blocks * block_len, total_bytes, offsets)) return fail(const_cast<dspi_ctx *>(c), DSPI_E_INVAL, "dspi_sources_bytes: the buffer's size overflows");
    return DSPI_OK;
}

int dspi_process_sources(dspi_ctx *c, const void *in, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words, dspi_spdif_rx *rx, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    bool wire;
    if (int rc = front_flags(c, "dspi_process_sources", &flags, &wire, false)) return rc;
    return mixed_call(c, in, sources, n_blocks, block_len, out, pdm_words, flags, "dspi_process_sources", wire, true, rx);
}

int dspi_spdif_decode(dspi_ctx *c, const uint32_t *subframes, uint32_t n_lines, uint32_t n_frames, dspi_spdif_rx *rx, int32_t *pairs, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (!subframes || !rx || !pairs || n_lines == 0 || n_frames == 0) return fail(c, DSPI_E_INVAL, "dspi_spdif_decode: a NULL pointer or a zero count");
    size_t in_b, rx_b;
    if (n_lines > 0x7fffffffu || __builtin_mul_overflow((size_t)n_lines * kRxFrameBytes, (size_t)n_frames, &in_b) || __builtin_mul_overflow((size_t)n_lines, sizeof(SpdifRx), &rx_b))
        return fail(c, DSPI_E_INVAL, "dspi_spdif_decode: the buffers' sizes overflow");
    if (flags & ~DSPI_MEM_DEVICE) return fail(c, DSPI_E_INVAL, "dspi_spdif_decode: the only flag is DSPI_MEM_DEVICE");
    const bool dev = flags & DSPI_MEM_DEVICE;
    SpdifRx *const recs = reinterpret_cast<SpdifRx *>(rx);
    if (dev) {
        if (reinterpret_cast<uintptr_t>(subframes) % 16u || reinterpret_cast<uintptr_t>(rx) % 16u || reinterpret_cast<uintptr_t>(pairs) % 16u)
            return fail(c, DSPI_E_INVAL, "dspi_spdif_decode: device pointers are 16-byte aligned");
    } else
        for (uint32_t l = 0; l < n_lines; l++) if (recs[l].sync > kRxBlock) return fail(c, DSPI_E_INVAL, "dspi_spdif_decode: the record of line " + std::to_string(l) + " has sync > 192");
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    const size_t out_b = in_b / 2;
    const void *d_in = subframes;
    void *d_out = pairs, *d_rx = rx;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_out, in_b)) || (rc = ensure(c, c->d_spdif_in, out_b)) || (rc = ensure(c, c->d_rx, rx_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_out, subframes, in_b, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, hipMemcpyAsync(c->d_rx, rx, rx_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_spdif_out; d_out = c->d_spdif_in; d_rx = c->d_rx;      // (the encoders' staging buffers the other way round: subframes in the larger one)
    }
    HIPCK(c, launch_spdifrx(false, d_in, nullptr, nullptr, nullptr, d_rx, d_out, n_frames, 0u, n_lines, c->hs));
    if (dev) return DSPI_OK;
    // the records come down into the library's own memory first: the caller's change only when every copy has succeeded
    std::vector<SpdifRx> after(n_lines);
    HIPCK(c, hipMemcpyAsync(after.data(), c->d_rx, rx_b, hipMemcpyDeviceToHost, c->hs));
    if ((rc = stage_down(c, pairs, c->d_spdif_in, out_b))) return rc;
    memcpy(recs, after.data(), rx_b);
    return DSPI_OK;
}

// ---- chained devices (dspi_link.h: views, links, the refusals and the reader on the CPU; dspi_linkrx.hip: the link receivers) ----
static_assert(sizeof(dspi_wire_view) == sizeof(WireView) && offsetof(dspi_wire_view, wire) == offsetof(WireView, wire) && offsetof(dspi_wire_view, n_streams) == offsetof(WireView, n_streams) &&
              offsetof(dspi_wire_view, n_pairs) == offsetof(WireView, n_pairs) && offsetof(dspi_wire_view, tile_streams) == offsetof(WireView, tile_streams) &&
              offsetof(dspi_wire_view, n_frames) == offsetof(WireView, n_frames) && offsetof(dspi_wire_view, producer) == offsetof(WireView, producer), "include/dspi.h and dspi_link.h: one view");
static_assert(sizeof(dspi_link) == sizeof(Link) && offsetof(dspi_link, kind) == offsetof(Link, kind), "include/dspi.h and dspi_link.h: one link");
static_assert(DSPI_LINK_NONE == kLinkNone && DSPI_LINK_SPDIF == kLinkSpdif && DSPI_LINK_I2S == kLinkI2s && DSPI_LINK_SPDIF == DSPI_SRC_SPDIF, "include/dspi.h and dspi_link.h: one set of kinds");

int dspi_wire_view_of(const dspi_ctx *p, const uint32_t *wire, uint32_t n_frames, uint32_t flags, dspi_wire_view *view) {
    if (!p || !view) return DSPI_E_INVAL;
    if (flags & ~DSPI_OUT_TILED) return fail(const_cast<dspi_ctx *>(p), DSPI_E_INVAL, "dspi_wire_view_of: the only flag is DSPI_OUT_TILED");
    *view = dspi_wire_view{wire, p->n_streams, (uint32_t)p->sm.n_pairs, (flags & DSPI_OUT_TILED) ? (uint32_t)p->sm.row : 0u, n_frames, const_cast<dspi_ctx *>(p)};
    return DSPI_OK;
}

int dspi_link_kinds(const dspi_ctx *p, dspi_link *links, uint32_t n) {
    if (!p || (!links && n)) return DSPI_E_INVAL;
    const uint32_t P = (uint32_t)p->sm.n_pairs;
    for (uint32_t i = 0; i < n; i++)
        if (links[i].line >= (uint64_t)p->n_streams * P) return fail(const_cast<dspi_ctx *>(p), DSPI_E_INVAL, "dspi_link_kinds: link " + std::to_string(i) + " names no line of the producer");
    for (uint32_t i = 0; i < n; i++) links[i].kind = readable(p, (int32_t)(links[i].line / P)).output_types[links[i].line % P] == 1 ? DSPI_LINK_I2S : DSPI_LINK_SPDIF;
    return DSPI_OK;
}

int dspi_wire_decode(dspi_ctx *c, const dspi_wire_view *view, const dspi_link *links, uint32_t n_links, dspi_spdif_rx *rx, int32_t *pairs, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (!view || !links || !pairs || n_links == 0) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: a NULL pointer or no link");
    if (flags & ~DSPI_MEM_DEVICE) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: the only flag is DSPI_MEM_DEVICE");
    const bool dev = flags & DSPI_MEM_DEVICE;
    const WireView &v = *reinterpret_cast<const WireView *>(view);
    const Link *const lk = reinterpret_cast<const Link *>(links);
    SpdifRx *const recs = reinterpret_cast<SpdifRx *>(rx);
    if (const char *why = link_view_why(v, 0, dev)) return fail(c, DSPI_E_INVAL, std::string("dspi_wire_decode: ") + why);
    const uint32_t bad = links_check(lk, n_links, link_view_lines(v), nullptr, true);
    if (bad < n_links) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: link " + std::to_string(bad) + " has a kind that is none of DSPI_LINK_*, or names no line of the view");
    const bool any_spdif = links_any(lk, n_links, nullptr, kLinkSpdif);
    const uint64_t F = v.n_frames;
    size_t out_b, rx_b;
    if (n_links > 0x7fffffffu || __builtin_mul_overflow((size_t)n_links * 8u, (size_t)F, &out_b) || __builtin_mul_overflow((size_t)n_links, sizeof(SpdifRx), &rx_b))
        return fail(c, DSPI_E_INVAL, "dspi_wire_decode: the buffers' sizes overflow");
    if (any_spdif && !rx) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: an S/PDIF link needs the receiver records (rx)");
    if (dev) {
        if ((any_spdif && reinterpret_cast<uintptr_t>(rx) % 16u) || reinterpret_cast<uintptr_t>(pairs) % 16u) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: device pointers are 16-byte aligned");
    } else
        for (uint32_t i = 0; i < n_links; i++)
            if (lk[i].kind == kLinkSpdif && recs[i].sync > kRxBlock) return fail(c, DSPI_E_INVAL, "dspi_wire_decode: the record of link " + std::to_string(i) + " has sync > 192");
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    WireView dv = v;
    void *d_out = pairs, *d_rx = rx;
    uint64_t words = 0;
    int rc;
    if (!dev) {
        link_view_words(v, &words);
        if ((rc = ensure(c, c->d_spdif_out, (size_t)words * 4)) || (rc = ensure(c, c->d_spdif_in, out_b)) || (any_spdif && (rc = ensure(c, c->d_rx, rx_b)))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_out, v.wire, (size_t)words * 4, hipMemcpyHostToDevice, c->hs));
        if (any_spdif) HIPCK(c, hipMemcpyAsync(c->d_rx, rx, rx_b, hipMemcpyHostToDevice, c->hs));
        dv.wire = c->d_spdif_out; d_out = c->d_spdif_in; d_rx = any_spdif ? c->d_rx.get() : nullptr;
    }
    LinkTab t;
    if ((rc = link_table(c, dv, lk, n_links, nullptr, t))) return rc;
    HIPCK(c, launch_linkrx(false, dv.wire, t.links, t.offsets, t.kinds, nullptr, d_rx, d_out, v.n_frames, v.n_pairs, v.tile_streams, n_links, t.any_spdif, t.any_i2s, c->hs));
    if (dev) return DSPI_OK;
    // everything comes down into the library's own memory first: the caller's buffers change only when every copy has succeeded, and only
    // where a link wrote (a hole's pair words and every record that is no S/PDIF link's stay the caller's)
    std::vector<int32_t> got(out_b / 4);
    std::vector<SpdifRx> after(any_spdif ? n_links : 0);
    if (any_spdif) HIPCK(c, hipMemcpyAsync(after.data(), c->d_rx, rx_b, hipMemcpyDeviceToHost, c->hs));
    if ((rc = stage_down(c, got.data(), c->d_spdif_in, out_b))) return rc;
    for (uint32_t i = 0; i < n_links; i++) {
        if (lk[i].kind == kLinkNone) continue;
        memcpy(pairs + (size_t)i * 2 * F, got.data() + (size_t)i * 2 * F, (size_t)F * 8);
        if (lk[i].kind == kLinkSpdif) recs[i] = after[i];
    }
    return DSPI_OK;
}

int dspi_process_linked(dspi_ctx *c, const dspi_wire_view *view, const dspi_link *links, uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words,
                        dspi_spdif_rx *rx, uint32_t flags) {
    if (!c || !view || !links || !out) return DSPI_E_INVAL;
    // 2. the flags
    bool wire;
    int rc = front_flags(c, "dspi_process_linked", &flags, &wire, true);
    // 3. the lengths
    if (rc || (rc = check_lengths(c, "dspi_process_linked", n_blocks, block_len))) return rc;
    // 4. the view
    const WireView &v = *reinterpret_cast<const WireView *>(view);
    const Link *const lk = reinterpret_cast<const Link *>(links);
    const uint64_t F = (uint64_t)n_blocks * block_len;
    if (F > 0xffffffffull) return fail(c, DSPI_E_INVAL, "dspi_process_linked: the view's n_frames is not n_blocks * block_len");
    if (const char *why = link_view_why(v, F, true)) return fail(c, DSPI_E_INVAL, std::string("dspi_process_linked: ") + why);
    // 5. the links of the active streams
    const uint32_t bad = links_check(lk, c->n_streams, link_view_lines(v), host_activity(c), false);
    if (bad < c->n_streams) return fail(c, DSPI_E_INVAL, "dspi_process_linked: the link of stream " + std::to_string(bad) + " is neither DSPI_LINK_SPDIF nor DSPI_LINK_I2S, or names no line of the view");
    // 6. the records
    const bool any_spdif = links_any(lk, c->n_streams, host_activity(c), kLinkSpdif);
    if (any_spdif && !rx) return fail(c, DSPI_E_INVAL, "dspi_process_linked: an S/PDIF link needs the receiver records (rx)");
    if (any_spdif && reinterpret_cast<uintptr_t>(rx) % 4u) return fail(c, DSPI_E_INVAL, "dspi_process_linked: device receiver records are 4-byte aligned");
    // 7. the producer
    if (view->producer && view->producer->device != DSPI_DEVICE_NONE && view->producer->device != c->device) return fail(c, DSPI_E_INVAL, "dspi_process_linked: the view's producer is on another HIP device");
    CallFront in{CallFront::Linked, wire, "dspi_process_linked", any_spdif ? reinterpret_cast<SpdifRx *>(rx) : nullptr};
    in.views = &v; in.n_views = 1; in.links = lk;
    return process_call(c, nullptr, 24, n_blocks, block_len, out, pdm_words, flags, in);
}

// ---- the patch bay (dspi_patch.h: the layout, the refusals and the plan; dspi_patchrx.hip: the tiled receiver) ----
static_assert(sizeof(dspi_patch) == sizeof(Patch) && offsetof(dspi_patch, line) == offsetof(Patch, line) && offsetof(dspi_patch, kind) == offsetof(Patch, kind), "include/dspi.h and dspi_patch.h: one patch");
static_assert(DSPI_SRC_LINK == kSrcLink && DSPI_MAX_VIEWS == kPatchMaxViews, "include/dspi.h and dspi_patch.h: one set of sources");

int dspi_patched_bytes(const dspi_ctx *c, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len, uint64_t *total_bytes, uint64_t *offsets) {
    if (!c || !sources) return DSPI_E_INVAL;
    dspi_ctx *const m = const_cast<dspi_ctx *>(c);
    uint32_t at = 0;
    if (const char *why = patch_sources_why(sources, c->n_streams, &at)) return fail(m, DSPI_E_INVAL, "dspi_patched_bytes: stream " + std::to_string(at) + ": " + why);
    if (int rc = check_lengths(m, "dspi_patched_bytes", n_blocks, block_len)) return rc;
    if (!patch_offsets(sources, c->n_streams, (uint64_t)n_blocks * block_len, total_bytes, offsets)) return fail(m, DSPI_E_INVAL, "dspi_patched_bytes: the buffer's size overflows");
    return DSPI_OK;
}

// refusals 3 to 10 of dspi_process_patched, in their order (dspi_debug_patched_intake shares them), for f.who; and for a call that has passed
// them its plan, with the descriptor's members that name it (f.rx: null unless an active stream is an S/PDIF run or link)
static int patched_front(dspi_ctx *c, CallFront &f, PatchPlan &plan, const void *in, const uint8_t *sources, const dspi_wire_view *views, uint32_t n_views, const dspi_patch *patches,
                         uint32_t n_blocks, uint32_t block_len, dspi_spdif_rx *rx) {
    const std::string w = std::string(f.who) + ": ";
    const uint32_t n = c->n_streams;
    const uint8_t *const act = host_activity(c);
    const WireView *const vs = reinterpret_cast<const WireView *>(views);
    const Patch *const ps = reinterpret_cast<const Patch *>(patches);
    uint32_t at = 0;
    int rc = check_lengths(c, f.who, n_blocks, block_len);
    if (rc) return rc;
    const uint64_t F = (uint64_t)n_blocks * block_len;
    if (const char *why = patch_sources_why(sources, n, &at)) return fail(c, DSPI_E_INVAL, w + "stream " + std::to_string(at) + ": " + why);
    const bool any_link = patch_any(sources, n, act, kSrcLink);
    if (any_link)
        if (const char *why = patch_views_why(sources, n, act, vs, n_views, ps, F, &at)) return fail(c, DSPI_E_INVAL, w + why + " (view or stream " + std::to_string(at) + ")");
    if (const char *why = patch_in_why(in, sources, n, act)) return fail(c, DSPI_E_INVAL, w + why);
    if (const char *why = patch_rx_why(rx, sources, n, act, ps)) return fail(c, DSPI_E_INVAL, w + why);
    uint64_t out_bytes = 0;
    if (!patch_offsets(sources, n, F, nullptr, nullptr) || __builtin_mul_overflow((uint64_t)n * kIntakeOutFrame, F, &out_bytes)) return fail(c, DSPI_E_INVAL, w + "the buffer's size overflows");
    if ((rc = check_widening(c, f.who, sources, act))) return rc;
    if (any_link)
        for (uint32_t s = 0; s < n; s++) {
            if (sources[s] != kSrcLink || (act && !act[s])) continue;
            const dspi_ctx *const prod = views[ps[s].view].producer;
            if (prod && prod->device != DSPI_DEVICE_NONE && prod->device != c->device) return fail(c, DSPI_E_INVAL, w + "the producer of view " + std::to_string(ps[s].view) + " is on another HIP device");
        }
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    f.views = vs; f.n_views = n_views; f.plan = &plan; f.rx = patch_needs_rx(sources, n, act, ps) ? reinterpret_cast<SpdifRx *>(rx) : nullptr;
    patch_plan(sources, n, act, vs, n_views, ps, F, plan);
    return 0;
}

int dspi_process_patched(dspi_ctx *c, const void *in, const uint8_t *sources, const dspi_wire_view *views, uint32_t n_views, const dspi_patch *patches, uint32_t n_blocks, uint32_t block_len,
                         const dspi_out *out, uint32_t *pdm_words, dspi_spdif_rx *rx, uint32_t flags) {
    if (!c || !sources || !out) return DSPI_E_INVAL;
    // 2. the flags
    bool wire;
    int rc = front_flags(c, "dspi_process_patched", &flags, &wire, true);
    // 3. to 11.
    PatchPlan plan;
    CallFront pt{CallFront::Patched, wire, "dspi_process_patched"};
    if (rc || (rc = patched_front(c, pt, plan, in, sources, views, n_views, patches, n_blocks, block_len, rx))) return rc;
    return process_call(c, in, 24, n_blocks, block_len, out, pdm_words, flags, pt);
}

int dspi_wire_encode_tiled(dspi_ctx *c, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos, uint32_t *wire, uint32_t flags) {
    if (!c || !pairs || !wire || !block_pos || n_frames == 0) return DSPI_E_INVAL;
    if (!wire_encode_tiled_flags_ok(flags)) return fail(c, DSPI_E_INVAL, "dspi_wire_encode_tiled: the only flag is DSPI_MEM_DEVICE");
    if (n_frames > kWireTiledMaxFrames) return fail(c, DSPI_E_INVAL, "dspi_wire_encode_tiled: at most 2 097 120 frames per call");
    const bool dev = flags & DSPI_MEM_DEVICE;
    // host positions are validated before anything is launched; device positions are the kernel's to reduce modulo 192
    if (!dev) for (uint32_t s = 0; s < c->n_streams; s++) if (block_pos[s] >= kSpdifBlock) return fail(c, DSPI_E_INVAL, "dspi_wire_encode_tiled: a position is 0..191");
    if (c->device == DSPI_DEVICE_NONE) return refuse_host_only(c);
    HIPCK(c, hipSetDevice(c->device));
    const uint32_t row = (uint32_t)c->sm.row;
    const size_t tile_in_b = (size_t)row * c->sm.n_pairs * n_frames * 8, in_b = c->n_wg * tile_in_b, out_b = in_b * 2, pos_b = (size_t)c->n_streams * 4;
    const int32_t *d_in = pairs;
    uint32_t *d_out = wire;
    const uint32_t *d_pos = block_pos;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_spdif_in, in_b)) || (rc = ensure(c, c->d_spdif_out, out_b)) ||
            (rc = ensure(c, c->d_spdif_vpos, pos_b))) return rc;
        HIPCK(c, hipMemcpyAsync(c->d_spdif_in, pairs, in_b, hipMemcpyHostToDevice, c->hs));
        HIPCK(c, hipMemcpyAsync(c->d_spdif_vpos, block_pos, pos_b, hipMemcpyHostToDevice, c->hs));
        d_in = c->d_spdif_in; d_out = c->d_spdif_out; d_pos = c->d_spdif_vpos;
        // (the staging buffer comes back whole: the encoder zeroes the I2S tails there, and the columns behind the last stream, which it
        //  does not write, are cleared with their tile as the audio calls clear them)
        hipError_t me = hipSuccess;
        for_absent_columns(c, CallBuffer{out_b, (size_t)c->sm.n_pairs * n_frames * 16, true, 0}, [&](size_t at, size_t n) { me = hipMemsetAsync(reinterpret_cast<char *>(d_out) + at, 0, n, c->hs); });
        HIPCK(c, me);
    }
    // every stream's types and rate are its own image's: committed first (unaware of pauses, like dspi_wire_encode)
    if ((rc = commit_params(c))) return rc;
    HIPCK(c, launch_wire_tiled(d_in, d_out, c->n_streams, (uint32_t)c->sm.n_pairs, n_frames, row, c->n_wg, 0u, SpdifRates{c->d_images, c->d_stream_image, 0u}, !dev, c->hs, d_pos));
    return dev ? DSPI_OK : stage_down(c, wire, c->d_spdif_out, out_b);
}

// ---- the front end of a device-buffer call alone, into the context's scratch: what the tools/bench_* of the input calls time (no chain, nothing
// advanced).  Each call's own argument checks, then the route's own two steps on the call's descriptor.  (upload_pauses: the activity bitmap goes
// up as commit_params sends it up in the real call; a patched call's kernels read the plan's masks, built from the host's record, instead) ----
static int debug_front(dspi_ctx *c, const CallFront &f, const void *in, uint64_t frames, bool upload_pauses = true) {
    HIPCK(c, hipSetDevice(c->device));
    int rc;
    if (upload_pauses && c->n_paused && (rc = upload_activity(c))) return rc;
    if ((rc = front_prepare(c, f, CallMem::Device, frames, (size_t)c->n_streams * kIntakeOutFrame * frames))) return rc;
    const void *chain_pcm;
    return front_launch(c, f, in, frames, &chain_pcm);
}

// ... of a dspi_process_mixed call, the intake (tools/bench_mixed.py), and (sources) of a dspi_process_sources call, the intake for the PCM
// streams and the receiver for the S/PDIF streams (tools/bench_spdif_in.py)
static int debug_mixed_intake(dspi_ctx *c, const char *who, const void *in, const uint8_t *kinds, uint32_t n_blocks, uint32_t block_len, bool sources, dspi_spdif_rx *rx) {
    if (!c || !in || !kinds) return DSPI_E_INVAL;
    int rc = mixed_check(c, kinds, n_blocks, block_len, who, sources);
    if (rc) return rc;
    const bool spdif_in = sources && sources_any_spdif(kinds, c->n_streams);
    if (spdif_in && (!rx || reinterpret_cast<uintptr_t>(in) % 16u || reinterpret_cast<uintptr_t>(rx) % 4u)) return fail(c, DSPI_E_INVAL, std::string(who) + ": rx is required and the input 16-byte aligned");
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no intake");
    const uint64_t frames = (uint64_t)n_blocks * block_len;
    std::vector<uint64_t> offsets((size_t)c->n_streams + 1);
    uint64_t out_bytes = 0;
    if (!(sources ? sources_offsets(kinds, c->n_streams, frames, nullptr, offsets.data()) : intake_offsets(kinds, c->n_streams, frames, nullptr, offsets.data())) ||
        __builtin_mul_overflow((uint64_t)c->n_streams * kIntakeOutFrame, frames, &out_bytes)) return fail(c, DSPI_E_INVAL, std::string(who) + ": the buffer's size overflows");
    return debug_front(c, CallFront{CallFront::Mixed, false, who, spdif_in ? reinterpret_cast<SpdifRx *>(rx) : nullptr, kinds, offsets.data()}, in, frames);
}
int dspi_debug_intake(dspi_ctx *c, const void *in, const uint8_t *depths, uint32_t n_blocks, uint32_t block_len) { return debug_mixed_intake(c, "dspi_debug_intake", in, depths, n_blocks, block_len, false, nullptr); }
int dspi_debug_sources_intake(dspi_ctx *c, const void *in, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len, dspi_spdif_rx *rx) {
    return debug_mixed_intake(c, "dspi_debug_sources_intake", in, sources, n_blocks, block_len, true, rx);
}

// ... of a dspi_process_patched call: the intake, the receiver over `in`, the link receivers and the patch receiver (tools/bench_patched.py)
int dspi_debug_patched_intake(dspi_ctx *c, const void *in, const uint8_t *sources, const dspi_wire_view *views, uint32_t n_views, const dspi_patch *patches, uint32_t n_blocks, uint32_t block_len,
                              dspi_spdif_rx *rx) {
    if (!c || !sources) return DSPI_E_INVAL;
    PatchPlan plan;
    CallFront pt{CallFront::Patched, false, "dspi_debug_patched_intake"};
    if (int rc = patched_front(c, pt, plan, in, sources, views, n_views, patches, n_blocks, block_len, rx)) return rc;
    return debug_front(c, pt, in, (uint64_t)n_blocks * block_len, false);
}

// ---- input from a packet table (dspi_packets.h: the entry rule, the check and the address arithmetic; dspi_packetrx.hip: the kernel) ----
// refusal 5's code and text (the host check's and the device check's)
static int refuse_packet_entry(dspi_ctx *c, const char *who, uint64_t at, uint32_t n_blocks, uint64_t *bad_entry) {
    if (bad_entry) *bad_entry = at;
    return fail(c, DSPI_E_INVAL, std::string(who) + ": entry " + std::to_string(at) + " (stream " + std::to_string(at / n_blocks) + ", packet " + std::to_string(at % n_blocks) + ") is odd or its packet does not end inside the arena");
}
// refusals 2 to 5 of dspi_process_packets behind the pointers, in their order (dspi_packets_check and dspi_debug_packets_intake share them).
// host_table false (the resident calls): the table is device memory, so every stream counts as paused here and no entry is looked at:
// refusals 2 to 4 alone, the table pointer never dereferenced
static int packets_refusals(dspi_ctx *c, const char *who, const uint8_t *depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, uint64_t *bad_entry,
                            bool host_table = true) {
    const std::string w = std::string(who) + ": ";
    uint64_t at = 0;
    const std::vector<uint8_t> nobody(host_table ? 0 : c->n_streams, 0u);
    switch (packets_check(depths, table, c->n_streams, n_blocks, block_len, DSPI_MAX_BLOCK_LEN, arena_bytes, host_table ? host_activity(c) : nobody.data(), &at)) {
    case PacketsBad::Ok: return 0;
    case PacketsBad::Lengths: return refuse_lengths(c, who);
    case PacketsBad::Depth: return fail(c, DSPI_E_INVAL, w + "the depth of stream " + std::to_string(at) + " is neither 16 nor 24");
    case PacketsBad::Overflow: return fail(c, DSPI_E_INVAL, w + "the table has more than 2^31 - 1 entries");
    case PacketsBad::Entry: break;
    }
    return refuse_packet_entry(c, who, at, n_blocks, bad_entry);
}

static CallFront packets_front(const char *who, bool wire, const uint8_t *depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len) {
    CallFront pk{CallFront::Packets, wire, who};
    pk.depths = depths; pk.table = table; pk.n_blocks = n_blocks; pk.block_len = block_len;
    return pk;
}

int dspi_packets_check(const dspi_ctx *c, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, uint64_t *bad_entry) {
    if (!c || !table || !bit_depths) return DSPI_E_INVAL;
    return packets_refusals(const_cast<dspi_ctx *>(c), "dspi_packets_check", bit_depths, table, n_blocks, block_len, arena_bytes, bad_entry);
}

int dspi_process_packets(dspi_ctx *c, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, const dspi_out *out,
                         uint32_t *pdm_words, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    // 1. the flags
    bool wire;
    int rc = front_flags(c, "dspi_process_packets", &flags, &wire, true);
    if (rc) return rc;
    // 2. to 5.
    if (!arena || !table || !bit_depths || !out) return fail(c, DSPI_E_INVAL, "dspi_process_packets: arena, table, bit_depths and out are required");
    if ((rc = packets_refusals(c, "dspi_process_packets", bit_depths, table, n_blocks, block_len, arena_bytes, nullptr))) return rc;
    // 6. the preamp rule
    if ((rc = check_widening(c, "dspi_process_packets", bit_depths, host_activity(c)))) return rc;
    // 7. (process_call refuses the host-only context)
    return process_call(c, arena, 24, n_blocks, block_len, out, pdm_words, flags, packets_front("dspi_process_packets", wire, bit_depths, table, n_blocks, block_len));
}

// the front end of a dspi_process_packets call alone, into the context's scratch: what tools/bench_packets.py times (no chain, nothing advanced)
int dspi_debug_packets_intake(dspi_ctx *c, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len) {
    if (!c || !arena || !table || !bit_depths) return DSPI_E_INVAL;
    int rc = packets_refusals(c, "dspi_debug_packets_intake", bit_depths, table, n_blocks, block_len, arena_bytes, nullptr);
    if (rc) return rc;
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no intake");
    return debug_front(c, packets_front("dspi_debug_packets_intake", false, bit_depths, table, n_blocks, block_len), arena, (uint64_t)n_blocks * block_len);
}

// ---- outputs to a packet table (dspi_packets_out.h: the entry rule, the checks, the CPU path and the address arithmetic; dspi_packettx.hip: the kernels) ----
static_assert(DSPI_PACKET_SKIP == kPacketSkip && DSPI_EMIT_CHECK_OVERLAP == kEmitCheckOverlap, "include/dspi.h and dspi_packets_out.h: one skip word, one flag");
// refusal 5's code and text, and the overlap's (the host check's and the device check's)
static int refuse_emit_entry(dspi_ctx *c, const char *who, uint64_t at, uint32_t n_blocks, bool overlaps, uint64_t *bad_entry) {
    if (bad_entry) *bad_entry = at;
    const uint64_t per = (uint64_t)c->sm.n_pairs * n_blocks;
    const std::string which = "entry " + std::to_string(at) + " (stream " + std::to_string(at / per) + ", pair " + std::to_string(at % per / n_blocks) + ", packet " + std::to_string(at % n_blocks) + ")";
    return fail(c, DSPI_E_INVAL, std::string(who) + ": " + which + (overlaps ? " overlaps another entry" : " is odd or its packet does not end inside the arena"));
}
// refusals 2 to 5 of dspi_packets_emit behind the pointers, in their order, and the overlap rule when asked (dspi_packets_emit_check shares them).
// host_table false: as in packets_refusals
static int emit_refusals(dspi_ctx *c, const char *who, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, bool overlap,
                         uint64_t *bad_entry, bool host_table = true) {
    const std::string w = std::string(who) + ": ";
    uint64_t at = 0;
    const std::vector<uint8_t> nobody(host_table ? 0 : c->n_streams, 0u);
    const EmitBad bad = packets_emit_check(formats, table, c->n_streams, (uint32_t)c->sm.n_pairs, n_blocks, block_len, DSPI_MAX_BLOCK_LEN, arena_bytes,
                                           host_table ? host_activity(c) : nobody.data(), overlap, &at);
    switch (bad) {
    case EmitBad::Ok: return 0;
    case EmitBad::Lengths: return refuse_lengths(c, who);
    case EmitBad::Format: return fail(c, DSPI_E_INVAL, w + "the format of stream " + std::to_string(at) + " is neither 24 nor 32");
    case EmitBad::Overflow: return fail(c, DSPI_E_INVAL, w + "the table has more than 2^31 - 1 entries");
    case EmitBad::Entry: case EmitBad::Overlap: break;
    }
    return refuse_emit_entry(c, who, at, n_blocks, bad == EmitBad::Overlap, bad_entry);
}

int dspi_packets_emit_check(const dspi_ctx *c, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, uint32_t check_flags,
                            uint64_t *bad_entry) {
    if (!c) return DSPI_E_INVAL;
    dspi_ctx *const m = const_cast<dspi_ctx *>(c);
    if (check_flags & ~DSPI_EMIT_CHECK_OVERLAP) return fail(m, DSPI_E_INVAL, "dspi_packets_emit_check: check_flags is 0 or DSPI_EMIT_CHECK_OVERLAP");
    if (!formats || !table) return fail(m, DSPI_E_INVAL, "dspi_packets_emit_check: formats and table are required");
    return emit_refusals(m, "dspi_packets_emit_check", formats, table, n_blocks, block_len, arena_bytes, check_flags & DSPI_EMIT_CHECK_OVERLAP, bad_entry);
}

int dspi_packets_emit(dspi_ctx *c, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats, const uint64_t *table, void *arena, uint64_t arena_bytes,
                      uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    // 1. the flags
    if (flags & ~(DSPI_MEM_DEVICE | DSPI_OUT_TILED)) return fail(c, DSPI_E_INVAL, "dspi_packets_emit: the flags are DSPI_MEM_DEVICE and DSPI_OUT_TILED");
    // 2. to 5.
    if (!pairs || !formats || !table || !arena) return fail(c, DSPI_E_INVAL, "dspi_packets_emit: pairs, formats, table and arena are required");
    int rc = emit_refusals(c, "dspi_packets_emit", formats, table, n_blocks, block_len, arena_bytes, false, nullptr);
    if (rc) return rc;
    const uint32_t P = (uint32_t)c->sm.n_pairs, R = (flags & DSPI_OUT_TILED) ? (uint32_t)c->sm.row : 0u;
    if (!(flags & DSPI_MEM_DEVICE)) {      // the CPU path: the activity is the context's at the time of the call, as on the device
        const uint8_t *const act = host_activity(c);
        for (uint32_t s = 0; s < c->n_streams; s++)
            if (!act || act[s]) packets_emit_cpu(static_cast<uint8_t *>(arena), pairs, table + (uint64_t)s * P * n_blocks, formats[s], s, P, n_blocks, block_len, R);
        return DSPI_OK;
    }
    // 6.
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "dspi_packets_emit: a host-only context has no device memory");
    if ((reinterpret_cast<uintptr_t>(pairs) & 15u) || (reinterpret_cast<uintptr_t>(arena) & 1u))
        return fail(c, DSPI_E_INVAL, "dspi_packets_emit: device pairs are 16-byte aligned (every hipMalloc is) and the arena 2-byte");
    if (R && emit_tiled_workgroups(c->n_streams, R, P, n_blocks, block_len) > 0x7fffffffull) return fail(c, DSPI_E_INVAL, "dspi_packets_emit: more than 2^31 - 1 workgroups");
    HIPCK(c, hipSetDevice(c->device));
    if (c->n_paused && (rc = upload_activity(c))) return rc;
    const size_t entries = (size_t)c->n_streams * P * n_blocks;
    if ((rc = upload_via_move_area(c, c->d_emit_tab, "hipHostMalloc failed (emit table)", {{table, entries * 8}, {formats, c->n_streams}}))) return rc;
    const uint64_t *const tab = c->d_emit_tab;
    const hipError_t e = launch_packettx(pairs, R, tab, reinterpret_cast<const uint8_t *>(tab + entries), activity(c), arena, c->n_streams, P, n_blocks, block_len, c->hs);
    return e == hipSuccess ? DSPI_OK : fail(c, DSPI_E_HIP, std::string("packetiser launch: ") + hipGetErrorString(e));
}

// the one launch of a dspi_packets_emit call alone, the table and the formats already in device memory: what tools/bench_packets_out.py times
// (no upload; NOTHING is checked but the pointers and the lengths — the table must be one that dspi_packets_emit_check accepts)
int dspi_debug_packets_emit_launch(dspi_ctx *c, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats, const uint64_t *table, void *arena, uint32_t flags) {
    if (!c || !pairs || !formats || !table || !arena || !n_blocks || !block_len || block_len > DSPI_MAX_BLOCK_LEN || (flags & ~(DSPI_MEM_DEVICE | DSPI_OUT_TILED)) || !(flags & DSPI_MEM_DEVICE) ||
        (reinterpret_cast<uintptr_t>(pairs) & 15u) || (reinterpret_cast<uintptr_t>(arena) & 1u))
        return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no packetiser");
    HIPCK(c, hipSetDevice(c->device));
    if (c->n_paused) { int rc = upload_activity(c); if (rc) return rc; }
    const hipError_t e = launch_packettx(pairs, (flags & DSPI_OUT_TILED) ? (uint32_t)c->sm.row : 0u, table, formats, activity(c), arena, c->n_streams, (uint32_t)c->sm.n_pairs, n_blocks, block_len, c->hs);
    return e == hipSuccess ? DSPI_OK : fail(c, DSPI_E_HIP, std::string("packetiser launch: ") + hipGetErrorString(e));
}

// ---- resident packet tables: both packet calls on a table that lies in DEVICE memory (dspi_tablecheck.h: the checker's arithmetic;
// dspi_tablecheck.hip: its kernel).  Only the table moves: the depths / formats stay host memory, refusals 2 to 4 and the preamp rule stay on the
// host, and refusal 5 is the checker's answer, waited for — or the caller's warrant (DSPI_TABLE_CHECKED), and then nothing waits ----
static_assert(DSPI_TABLE_CHECKED == 0x1u, "include/dspi.h");
static TableCheck resident_table(const dspi_ctx *c, uint32_t kind, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes) {
    const uint32_t per = kind == kTableEmit ? (uint32_t)c->sm.n_pairs * n_blocks : n_blocks;      // (refusal 4 came first: no overflow)
    return TableCheck{(uint64_t)c->n_streams * per, arena_bytes, per, block_len, kind};
}
// what stands between refusal 4 and refusal 5 in all four calls (audio: the text every audio call refuses a host-only context with)
static int resident_device_refusals(dspi_ctx *c, const char *who, const uint64_t *table, bool audio = false) {
    if (c->device == DSPI_DEVICE_NONE) return audio ? refuse_host_only(c) : fail(c, DSPI_E_NODEVICE, std::string(who) + ": a host-only context has no device memory");
    if (reinterpret_cast<uintptr_t>(table) & 15u) return fail(c, DSPI_E_INVAL, std::string(who) + ": a device table is 16-byte aligned (every hipMalloc is)");
    return 0;
}
// The checker on the context's stream, waited for: the answer word with the n kind bytes behind it goes up through the pinned area, the one
// launch follows, and the 8 bytes come back.  *answer: the lowest refused index of an active stream, or kTableCheckNone.
static int resident_check(dspi_ctx *c, const TableCheck &t, const uint8_t *kinds, const uint64_t *table, uint64_t *answer) {
    HIPCK(c, hipSetDevice(c->device));
    int rc;
    if (c->n_paused && (rc = upload_activity(c))) return rc;
    const uint64_t none = kTableCheckNone;
    if ((rc = upload_via_move_area(c, c->d_tabcheck, "hipHostMalloc failed (table check)", {{&none, 8}, {kinds, c->n_streams}}))) return rc;
    const hipError_t e = launch_tablecheck(t, table, reinterpret_cast<const uint8_t *>(c->d_tabcheck + 1), activity(c), c->d_tabcheck, 0u, c->hs);
    if (e != hipSuccess) return fail(c, DSPI_E_HIP, std::string("table check launch: ") + hipGetErrorString(e));
    HIPCK(c, hipMemcpyAsync(answer, c->d_tabcheck, 8, hipMemcpyDeviceToHost, c->hs));
    HIPCK(c, hipStreamSynchronize(c->hs));
    return 0;
}
// refusals 2 to 4, the device's two, then 5 unless the caller warrants it (`checked`), of the input kind ...
static int resident_packets_refusals(dspi_ctx *c, const char *who, const uint8_t *depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, bool audio,
                                     bool checked, uint64_t *bad_entry) {
    int rc = packets_refusals(c, who, depths, table, n_blocks, block_len, arena_bytes, nullptr, false);
    if (rc || (rc = resident_device_refusals(c, who, table, audio)) || checked) return rc;
    uint64_t at = kTableCheckNone;
    if ((rc = resident_check(c, resident_table(c, kTableInput, n_blocks, block_len, arena_bytes), depths, table, &at))) return rc;
    return at == kTableCheckNone ? 0 : refuse_packet_entry(c, who, at, n_blocks, bad_entry);
}
// ... and 2 to 5 of the emit kind, as the check call applies them (dspi_packets_emit_resident has its pointers' alignments in between)
static int resident_emit_refusals(dspi_ctx *c, const char *who, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes,
                                  uint64_t *bad_entry) {
    int rc = emit_refusals(c, who, formats, table, n_blocks, block_len, arena_bytes, false, nullptr, false);
    if (rc || (rc = resident_device_refusals(c, who, table))) return rc;
    uint64_t at = kTableCheckNone;
    if ((rc = resident_check(c, resident_table(c, kTableEmit, n_blocks, block_len, arena_bytes), formats, table, &at))) return rc;
    return at == kTableCheckNone ? 0 : refuse_emit_entry(c, who, at, n_blocks, false, bad_entry);
}

int dspi_packets_check_resident(dspi_ctx *c, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, uint64_t *bad_entry) {
    if (!c || !table || !bit_depths) return DSPI_E_INVAL;
    return resident_packets_refusals(c, "dspi_packets_check_resident", bit_depths, table, n_blocks, block_len, arena_bytes, false, false, bad_entry);
}

int dspi_packets_emit_check_resident(dspi_ctx *c, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes, uint32_t check_flags,
                                     uint64_t *bad_entry) {
    if (!c) return DSPI_E_INVAL;
    if (check_flags) return fail(c, DSPI_E_INVAL, "dspi_packets_emit_check_resident: check_flags is 0 (overlap detection stays with host tables)");
    if (!formats || !table) return fail(c, DSPI_E_INVAL, "dspi_packets_emit_check_resident: formats and table are required");
    return resident_emit_refusals(c, "dspi_packets_emit_check_resident", formats, table, n_blocks, block_len, arena_bytes, bad_entry);
}

int dspi_process_packets_resident(dspi_ctx *c, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len,
                                  const dspi_out *out, uint32_t *pdm_words, uint32_t flags, uint32_t table_flags) {
    static const char who[] = "dspi_process_packets_resident";
    if (!c) return DSPI_E_INVAL;
    // 1. the flags
    bool wire;
    int rc = front_flags(c, who, &flags, &wire, true);
    if (rc) return rc;
    if (table_flags & ~DSPI_TABLE_CHECKED) return fail(c, DSPI_E_INVAL, std::string(who) + ": table_flags is 0 or DSPI_TABLE_CHECKED");
    // 2. to 4., the device's two, 5. on the device
    if (!arena || !table || !bit_depths || !out) return fail(c, DSPI_E_INVAL, std::string(who) + ": arena, table, bit_depths and out are required");
    if ((rc = resident_packets_refusals(c, who, bit_depths, table, n_blocks, block_len, arena_bytes, true, table_flags & DSPI_TABLE_CHECKED, nullptr))) return rc;
    // 6. the preamp rule
    if ((rc = check_widening(c, who, bit_depths, host_activity(c)))) return rc;
    CallFront pk = packets_front(who, wire, bit_depths, table, n_blocks, block_len);
    pk.table_on_device = true;
    return process_call(c, arena, 24, n_blocks, block_len, out, pdm_words, flags, pk);
}

int dspi_packets_emit_resident(dspi_ctx *c, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats, const uint64_t *table, void *arena, uint64_t arena_bytes,
                               uint32_t flags, uint32_t table_flags) {
    static const char who[] = "dspi_packets_emit_resident";
    if (!c) return DSPI_E_INVAL;
    // 1. the flags
    if (flags & ~(DSPI_MEM_DEVICE | DSPI_OUT_TILED)) return fail(c, DSPI_E_INVAL, std::string(who) + ": the flags are DSPI_MEM_DEVICE and DSPI_OUT_TILED");
    if (!(flags & DSPI_MEM_DEVICE)) return fail(c, DSPI_E_INVAL, std::string(who) + ": DSPI_MEM_DEVICE is required");
    if (table_flags & ~DSPI_TABLE_CHECKED) return fail(c, DSPI_E_INVAL, std::string(who) + ": table_flags is 0 or DSPI_TABLE_CHECKED");
    // 2. to 4.
    if (!pairs || !formats || !table || !arena) return fail(c, DSPI_E_INVAL, std::string(who) + ": pairs, formats, table and arena are required");
    int rc = emit_refusals(c, who, formats, table, n_blocks, block_len, arena_bytes, false, nullptr, false);
    if (rc || (rc = resident_device_refusals(c, who, table))) return rc;
    const uint32_t P = (uint32_t)c->sm.n_pairs, R = (flags & DSPI_OUT_TILED) ? (uint32_t)c->sm.row : 0u;
    if ((reinterpret_cast<uintptr_t>(pairs) & 15u) || (reinterpret_cast<uintptr_t>(arena) & 1u))
        return fail(c, DSPI_E_INVAL, std::string(who) + ": device pairs are 16-byte aligned (every hipMalloc is) and the arena 2-byte");
    if (R && emit_tiled_workgroups(c->n_streams, R, P, n_blocks, block_len) > 0x7fffffffull) return fail(c, DSPI_E_INVAL, std::string(who) + ": more than 2^31 - 1 workgroups");
    // 5. on the device
    if (!(table_flags & DSPI_TABLE_CHECKED)) {
        uint64_t at = kTableCheckNone;
        if ((rc = resident_check(c, resident_table(c, kTableEmit, n_blocks, block_len, arena_bytes), formats, table, &at))) return rc;
        if (at != kTableCheckNone) return refuse_emit_entry(c, who, at, n_blocks, false, nullptr);
    }
    HIPCK(c, hipSetDevice(c->device));
    if (c->n_paused && (rc = upload_activity(c))) return rc;
    // (the table stays where it lies: only the formats go up)
    if ((rc = upload_via_move_area(c, c->d_emit_tab, "hipHostMalloc failed (emit formats)", {{formats, c->n_streams}}))) return rc;
    const hipError_t e = launch_packettx(pairs, R, table, reinterpret_cast<const uint8_t *>(c->d_emit_tab.get()), activity(c), arena, c->n_streams, P, n_blocks, block_len, c->hs);
    return e == hipSuccess ? DSPI_OK : fail(c, DSPI_E_HIP, std::string("packetiser launch: ") + hipGetErrorString(e));
}

// the checker's one launch alone, asynchronous on the context's stream, the answer left in the context's word and not read: what
// tools/bench_packets_resident.py times.  kind 0: an input table, 1: an emit table; kinds (the depths / formats) and table are DEVICE memory
int dspi_debug_table_check_launch(dspi_ctx *c, uint32_t kind, const uint8_t *kinds, const uint64_t *table, uint32_t n_blocks, uint32_t block_len, uint64_t arena_bytes) {
    if (!c || kind > kTableEmit || !kinds || !table || !n_blocks || !block_len || block_len > DSPI_MAX_BLOCK_LEN || (reinterpret_cast<uintptr_t>(table) & 15u)) return DSPI_E_INVAL;
    if ((uint64_t)c->n_streams * (kind == kTableEmit ? (uint64_t)c->sm.n_pairs : 1u) * n_blocks > kPacketMaxEntries) return DSPI_E_INVAL;
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no table check");
    HIPCK(c, hipSetDevice(c->device));
    int rc;
    if ((c->n_paused && (rc = upload_activity(c))) || (rc = ensure(c, c->d_tabcheck, 8))) return rc;
    const hipError_t e = launch_tablecheck(resident_table(c, kind, n_blocks, block_len, arena_bytes), table, kinds, activity(c), c->d_tabcheck, 0u, c->hs);
    return e == hipSuccess ? DSPI_OK : fail(c, DSPI_E_HIP, std::string("table check launch: ") + hipGetErrorString(e));
}

int dspi_pdm_running(dspi_ctx *c, uint32_t first, uint32_t count, const uint8_t *set, uint8_t *get) {
    if (!c) return DSPI_E_INVAL;
    if (const char *why = c->pdm_life.set_get(first, count, set, get)) return fail(c, DSPI_E_INVAL, std::string("dspi_pdm_running: ") + why);
    return (int)count;
}

// ---- the fade-out on disable (dspi_pdmfade.h: the mode, the positions, the aux words; dspi_pdm.hip: the FADE kernels and the bases' travel) ----
int dspi_pdm_fade(dspi_ctx *c, int enable) {
    if (!c) return DSPI_E_INVAL;
    if (enable > 0 && !c->pdm_fade.on) {
        if (c->device != DSPI_DEVICE_NONE) {      // every stream: base 0
            HIPCK(c, hipSetDevice(c->device));
            if (int rc = persist_alloc(c, kArrPdmBase, "hipMalloc failed (PDM fade bases)")) return rc;
            HIPCK(c, hipMemsetAsync(c->d_pdm_base, 0, c->d_pdm_base.cap, c->hs));
        }
        c->pdm_fade.enable(c->pdm_life);
    } else if (enable == 0) c->pdm_fade.disable(c->pdm_life);
    return c->pdm_fade.on ? 1 : 0;
}

int dspi_pdm_fade_state(dspi_ctx *c, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get) {
    if (!c) return DSPI_E_INVAL;
    if (!c->pdm_fade.on) return fail(c, DSPI_E_INVAL, "dspi_pdm_fade_state: the fade mode is off (dspi_pdm_fade)");
    // everything is validated before anything is written
    if (const char *why = c->pdm_fade.check(first, count, set)) return fail(c, DSPI_E_INVAL, std::string("dspi_pdm_fade_state: ") + why);
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "host-only context: no fade bases");
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipStreamSynchronize(c->hs));
    std::vector<int32_t> base(count);
    if (set) {
        for (uint32_t k = 0; k < count; k++) base[k] = (int16_t)(uint16_t)(set[k] >> 16);
        HIPCK(c, hipMemcpy(c->d_pdm_base + first, base.data(), (size_t)count * 4, hipMemcpyHostToDevice));
        for (uint32_t k = 0; k < count; k++) c->pdm_fade.pos[first + k] = (uint16_t)(set[k] & 0xffffu);
        c->pdm_life.mark_dirty();
    } else if (get) HIPCK(c, hipMemcpy(base.data(), c->d_pdm_base + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    if (get) for (uint32_t k = 0; k < count; k++) get[k] = (uint32_t)c->pdm_fade.pos[first + k] | (uint32_t)(uint16_t)base[k] << 16;
    return (int)count;
}

// ---- the meter bridge (dspi_meters.h: the words, the rules and the CPU paths; dspi_meterbridge.hip: the kernels) ----
static_assert(DSPI_MEM_DEVICE == kMeterMemDevice, "include/dspi.h and dspi_meters.h: one flag");

int dspi_meters_update(dspi_ctx *c, const uint16_t *peaks, uint32_t n_blocks, uint32_t hold_packets, uint32_t decay_q15, uint32_t *meters, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (const char *why = meters_update_why(peaks, n_blocks, hold_packets, decay_q15, meters, flags, c->n_streams, c->sm.n_ch)) return fail(c, DSPI_E_INVAL, std::string("dspi_meters_update: ") + why);
    if (!(flags & DSPI_MEM_DEVICE)) {      // the activity is the context's at the time of the call, on either path
        meters_update_cpu(peaks, c->n_streams, n_blocks, c->sm.n_ch, hold_packets, decay_q15, meters, host_activity(c));
        return DSPI_OK;
    }
    if (c->device == DSPI_DEVICE_NONE) return fail(c, DSPI_E_NODEVICE, "dspi_meters_update: a host-only context has no device memory");
    HIPCK(c, hipSetDevice(c->device));
    if (c->n_paused) { int rc = upload_activity(c); if (rc) return rc; }
    HIPCK(c, launch_meters_update(c->sm.n_ch, peaks, c->n_streams, n_blocks, hold_packets, decay_q15, meters, activity(c), c->hs));
    return DSPI_OK;
}

int dspi_meters_alarms(dspi_ctx *c, const uint32_t *meters, uint32_t level_q15, uint32_t *streams, uint32_t *info, uint32_t cap, uint32_t *total, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (const char *why = meters_alarms_why(meters, level_q15, streams, info, cap, total, flags)) return fail(c, DSPI_E_INVAL, std::string("dspi_meters_alarms: ") + why);
    const bool dev = flags & DSPI_MEM_DEVICE;
    if (c->device == DSPI_DEVICE_NONE) {
        if (dev) return fail(c, DSPI_E_NODEVICE, "dspi_meters_alarms: a host-only context has no device memory");
        return (int)meters_alarms_cpu(meters, nullptr, c->n_streams, c->sm.n_ch, level_q15, streams, info, cap, total);      // no chain has run: no clip bit
    }
    HIPCK(c, hipSetDevice(c->device));
    const uint32_t row = (uint32_t)c->sm.row, n_slots = (uint32_t)c->sm.n_slots, clip_slot = (uint32_t)c->sm.clip;
    int rc;
    if (dev) {
        if ((rc = ensure(c, c->d_meter_scan, (size_t)meters_alarm_workgroups(c->n_streams) * 2u * 4u))) return rc;
        HIPCK(c, launch_meters_alarms(c->sm.n_ch, c->d_state, c->n_streams, row, n_slots, clip_slot, meters, level_q15, c->d_meter_scan, streams, info, cap, total, c->hs));
        return DSPI_OK;
    }
    // host memory: every stream's clip word comes down (one launch, one copy), the scan runs on the CPU
    std::vector<uint16_t> clip(c->n_streams);
    if ((rc = ensure(c, c->d_meter_down, (size_t)c->n_streams * 2u))) return rc;
    HIPCK(c, launch_clip_gather(c->d_state, c->n_streams, row, n_slots, clip_slot, reinterpret_cast<uint16_t *>(c->d_meter_down.p), c->hs));
    if ((rc = stage_down(c, clip.data(), c->d_meter_down.p, (size_t)c->n_streams * 2u))) return rc;
    return (int)meters_alarms_cpu(meters, clip.data(), c->n_streams, c->sm.n_ch, level_q15, streams, info, cap, total);
}

int dspi_status_all(dspi_ctx *c, uint32_t first, uint32_t count, void *buf, size_t cap, uint32_t flags) {
    if (!c) return DSPI_E_INVAL;
    if (const char *why = status_all_why(first, count, buf, flags, c->n_streams)) return fail(c, DSPI_E_INVAL, std::string("dspi_status_all: ") + why);
    const size_t block = status_block_bytes(c->sm.n_ch), bytes = (size_t)count * block;
    if (cap < bytes) return fail(c, DSPI_E_SHORT, "dspi_status_all: the buffer is too small");
    const bool dev = flags & DSPI_MEM_DEVICE;
    if (c->device == DSPI_DEVICE_NONE) {
        if (dev) return fail(c, DSPI_E_NODEVICE, "dspi_status_all: a host-only context has no device memory");
        const uint16_t no_peaks[kMaxCh] = {};      // (as fetch_status answers there)
        for (uint32_t i = 0; i < count; i++) status_pack(no_peaks, 0, c->sm.n_ch, static_cast<uint8_t *>(buf) + i * block);
        return (int)count;
    }
    HIPCK(c, hipSetDevice(c->device));
    void *dst = buf;
    int rc;
    if (!dev) {
        if ((rc = ensure(c, c->d_meter_down, bytes))) return rc;
        dst = c->d_meter_down.p;
    }
    HIPCK(c, launch_status_gather(c->sm.n_ch, c->d_state, first, count, (uint32_t)c->sm.row, (uint32_t)c->sm.n_slots, (uint32_t)c->sm.peaks, (uint32_t)c->sm.clip, dst, c->hs));
    if (!dev && (rc = stage_down(c, buf, dst, bytes))) return rc;
    return (int)count;
}

int dspi_clear_clips_list(dspi_ctx *c, const uint32_t *streams, uint32_t n) {
    if (!c) return DSPI_E_INVAL;
    if (!streams && n) return fail(c, DSPI_E_INVAL, "dspi_clear_clips_list: a NULL list");
    const uint32_t bad = clear_list_check(streams, n, c->n_streams);
    if (bad < n) return fail(c, DSPI_E_INVAL, "dspi_clear_clips_list: entry " + std::to_string(bad) + " names no stream of the context");
    if (c->device == DSPI_DEVICE_NONE || n == 0) return (int)n;      // (host-only: no chain has run, nothing to clear)
    HIPCK(c, hipSetDevice(c->device));
    int rc = upload_via_move_area(c, c->d_meter_list, "hipHostMalloc failed (clip clear list)", {{streams, (size_t)n * 4u}});
    if (rc) return rc;
    HIPCK(c, launch_clip_clear(c->d_state, c->d_meter_list, n, (uint32_t)c->sm.row, (uint32_t)c->sm.n_slots, (uint32_t)c->sm.clip, c->hs));
    return (int)n;
}

}  // extern "C"
