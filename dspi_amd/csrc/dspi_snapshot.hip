// dspi_snapshot.hip — stream snapshots on the GPU: the transposition between the context's stream-minor arrays and stream-major records
// (dspi_snapshot.h).  Export gathers, import scatters; both are one launch over every section of the record.
//
// The arrays are [W][position][R] (one 512- / 256-byte row per position, column = stream), a record is [position] per stream.  A
// one-thread-per-stream copy would touch 4 bytes of every row; instead one workgroup of 256 threads takes a tile of TP positions x TC
// columns of a row and turns it in LDS:
//   array side    a lane moves 16 bytes = 4 columns of one position; TC/4 lanes cover the tile's piece of a row
//   record side   a lane moves 16 bytes = 4 positions of one column; TP/4 lanes cover the tile's run of one stream (4 TP bytes)
//   LDS           uint32 [TP][TC + 1].  With the odd pitch P, word j of record-side lane (k, c) sits in bank (4k + j) P + c and word j
//                 of array-side lane (r, q) in bank r P + 4q + j (mod 64).  (The odd pitch rules out 16-byte LDS accesses; four 4-byte
//                 ones per lane it is.)  Lanes k and k + 16 of the record side would meet in one bank (4 x 16 = 64), so a lane touches
//                 its four words in the order j + rot, rot = (k / 16) x (columns per wave): the lanes that share 4k mod 64 then sit
//                 1, 2 or 3 banks (P = 1 mod 64) or 33, 2, 35 banks (P = 33) apart, the columns of a wave fill the gaps: conflict-free.
// The tile shape is the one thing measured rather than derived (profiles/snapshot.md): what decides the time is the length of the
// record side's runs when they are WRITTEN — export: 10.0 / 6.9 / 5.7 / 4.8 ms per 10.3 GB with runs of 128 / 256 / 512 / 1 024 bytes;
// the import, which reads them, does not care (3.8 - 4.1 ms with any shape).  Hence
//   export  256 positions x 32 columns   1 024-byte runs, 128-byte row pieces; 33.8 KB of LDS; a record-side wave is one column, its
//                                        64 k's in four groups of 16: conflict-free with the rotation; array side (8 q's x 8 rows per
//                                        wave, bank 33 r + 4q + j) 2-way
//   import  128 positions x 64 columns   512-byte runs, 256-byte row pieces; 33.3 KB of LDS; a record-side wave is two columns x 32 k's:
//                                        conflict-free with the rotation; array side (16 q's x 4 rows per wave) conflict-free
// A row that the range covers only in part takes the same kernel: the record side loops over the covered columns only, the import's
// array side stores whole 16-byte groups where all four columns are covered and single words elsewhere, so foreign streams' words are
// never written.  Positions past a section's length (the tile grid rounds up) are never read from or written to the arrays; a
// section's pad words (dspi_snapshot.h) are exported as zeros and ignored by the import.
//
// The REALIGNING import (DSPI_SNAP_REALIGN, dspi_realign_streams; the rule and the index arithmetic are in dspi_snapshot.h) rotates every
// delay line and ring on this pass: position p of a line of column c takes the record's position (p - d_c) mod length, d_c from a
// per-stream shift table that snapshot_targets_kernel wrote just before (one workgroup per touched row, one thread per stream: the row's
// target positions minus the record's own), and the two position slots of the state section are advanced by the same d_c.  The array
// side is the plain import's.  The record side can no longer move 16 bytes per lane — the run that maps onto the tile starts at
// (p0 - d_c) mod length, aligned to 4 bytes only, and wraps once per line — so it reads single words, and with single words a wave is
// free to read them in run order:
//   record side   load j (of 4) of lane (k, h) of wave w reads position 32 j + k of column c = w + 4 i + 32 h in pass i (of 8): a half
//                 wave reads 128 consecutive bytes of one record (two pieces at the wrap), a workgroup's four loads 512 bytes per column
//   LDS           the word goes to tile[32 j + k][c]: bank (32 j + k) P + c = 32 j + k + w + 4 i + 32 h (mod 64; P = 65): for one
//                 instruction j, i and w are fixed and k + 32 h runs over all 64 banks: conflict-free.  (Two ADJACENT columns per wave,
//                 as on the plain path, would put lanes (k + 1, c) and (k, c + 1) into one bank: hence the half waves 32 columns apart.)
//
// The LIST-ADDRESSED kernels (dspi_move_streams; the lists: dspi_move.h) are the same three code paths with another answer to "which columns
// of which row": blockIdx.y is a work item — a touched row, a record index per column (kMoveNone: not listed) and two masks over the row's
// groups of four columns, "any listed" and "all listed" — instead of a row of a range.  Tiles, LDS pitch, lane mappings and bank arithmetic
// are unchanged.  A tile without a listed column returns at once; the record side skips unlisted columns (their LDS words are never
// filled on the gather and never read on the scatter); the scatter's array side stores 16 bytes where all four columns are listed and
// single words elsewhere, so a touched row's unlisted columns are never written.  The realigning scatter looks its shifts up by destination
// stream; list_shifts_kernel wrote them, once per call, before the first scatter.
//
// BETWEEN TWO CONTEXTS (dspi_migrate_streams; the lists: dspi_migrate.h) the gather runs on the source context's arrays and the scatter on the
// destination's, both unchanged; the shifts need both sides' positions, which no one kernel can read when the contexts sit on two devices:
// migrate_positions_kernel, on the source, writes every listed stream's pair into an array in list order; that array travels like the
// records; list_shifts_kernel, on the destination, writes shift[destination slot] from it and from the destination's own state array.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_move.h"
#include "dspi_snapshot.h"

namespace dspi {

static_assert(kPdmWords == kPdmStateWords, "the snapshot's PDM section is the modulator's state");
static_assert(sizeof(MoveRowItem) == 16 && sizeof(ListTarget) == 16, "the lists' work items go up as 32-bit words");

namespace {

constexpr uint32_t kSnapThreads = 256;
constexpr uint32_t kExportPos = 256, kExportCols = 32, kImportPos = 128, kImportCols = 64;      // tile shapes (see above)
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct SnapKArgs {
    uint32_t *arr[SEC_COUNT];          // [W][len][ROW]
    uint32_t len[SEC_COUNT], off[SEC_COUNT], span[SEC_COUNT];
    uint32_t tile0[SEC_COUNT];         // blockIdx.x of the section's first tile
    uint32_t *rec;                     // record of stream `first`
    uint32_t record_words, first, count, row0;
};

struct SnapRealignArgs : SnapKArgs {
    const uint2 *shift;                // per stream of [first, first + count): {delay lines' rotation, rings' rotation}
};
// the list-addressed kernels (dspi_move_streams): blockIdx.y is a work item, a touched row with a record index per column
struct SnapListArgs : SnapKArgs {
    const MoveRowItem *items;
    const uint32_t *colrec;            // [item][ROW]: the record of each column, kMoveNone = not listed
    const uint2 *shift;                // realigning scatter: per stream of the CONTEXT, indexed by the destination slot
};
template <bool REALIGN, bool LIST> struct SnapArgsOf { typedef SnapKArgs type; };
template <> struct SnapArgsOf<true, false> { typedef SnapRealignArgs type; };
template <bool REALIGN> struct SnapArgsOf<REALIGN, true> { typedef SnapListArgs type; };

// word i of four, i known at run time only: selects, so that the four stay in registers
__device__ __forceinline__ uint32_t pick(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) { return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3; }

template <uint32_t ROW, bool IMPORT, bool REALIGN = false, bool LIST = false>
__global__ __launch_bounds__(kSnapThreads) void snapshot_kernel(const typename SnapArgsOf<REALIGN, LIST>::type a) {
    static_assert(IMPORT || !REALIGN, "only the import realigns");
    constexpr uint32_t kTilePos = IMPORT ? kImportPos : kExportPos, kCols = IMPORT ? kImportCols : kExportCols;
    static_assert(ROW % kCols == 0 && kCols % 4 == 0 && kTilePos % 4 == 0 && kSnapThreads % (kCols / 4) == 0 && kSnapThreads % (kTilePos / 4) == 0, "tile shape");
    constexpr uint32_t kPitch = kCols + 1, kRowLanes = kCols / 4, kRowsPerPass = kSnapThreads / kRowLanes, kRunLanes = kTilePos / 4, kColsPerPass = kSnapThreads / kRunLanes;
    __shared__ uint32_t tile[kTilePos * kPitch];
    // the tile's section (constant indices only: a run-time index into the argument block would put it in scratch)
    uint32_t *base = a.arr[0];
    uint32_t len = a.len[0], span = a.span[0], off = a.off[0], t0 = 0;
    [[maybe_unused]] int sec = 0;
#pragma unroll
    for (int i = 1; i < SEC_COUNT; i++)
        if (blockIdx.x >= a.tile0[i]) { base = a.arr[i]; len = a.len[i]; span = a.span[i]; off = a.off[i]; t0 = a.tile0[i]; sec = i; }
    const uint32_t p0 = (blockIdx.x - t0) * kTilePos, col0 = blockIdx.z * kCols;
    const uint32_t tid = threadIdx.x;
    const uint32_t q = tid % kRowLanes, r0 = tid / kRowLanes;       // array side: columns 4q .. 4q + 3 of position p0 + r
    const uint32_t k = tid % kRunLanes, cc0 = tid / kRunLanes;      // record side: positions p0 + 4k .. + 3 of column c
    // the tile's columns: those inside [first, first + count) — or, LIST, those of the work item's row that carry a record index
    uint32_t wg, c_lo = 0, c_hi = kCols;      // relative to col0
    bool q_any, q_all;
    [[maybe_unused]] uint64_t b0 = 0;
    [[maybe_unused]] uint32_t *rec = nullptr;          // column c_lo's run
    [[maybe_unused]] const uint32_t *cr = nullptr;     // LIST: the tile's columns' record indices
    if constexpr (LIST) {
        const MoveRowItem it = a.items[blockIdx.y];
        const uint32_t any = it.q_any >> (col0 / 4), all = it.q_all >> (col0 / 4);
        if (!(any & ((1u << kRowLanes) - 1u))) return;
        wg = it.row;
        cr = a.colrec + (size_t)blockIdx.y * ROW + col0;
        q_any = (any >> q) & 1u; q_all = (all >> q) & 1u;
    } else {
        wg = a.row0 + blockIdx.y;
        const uint64_t s0 = (uint64_t)wg * ROW, lo = a.first > s0 + col0 ? a.first : s0 + col0, end = (uint64_t)a.first + a.count, hi = end < s0 + col0 + kCols ? end : s0 + col0 + kCols;
        b0 = s0 + col0;
        if (hi <= lo) return;
        c_lo = (uint32_t)(lo - b0); c_hi = (uint32_t)(hi - b0);
        rec = a.rec + (size_t)(b0 + c_lo - a.first) * a.record_words + off + p0;
        q_any = 4 * q + 4 > c_lo && 4 * q < c_hi; q_all = 4 * q >= c_lo && 4 * q + 4 <= c_hi;
    }
    uint32_t *const arr = base + ((size_t)wg * len + p0) * ROW + col0;
    // column c's run of the tile on the record side (LIST: null where the column is not listed)
    auto run_of = [&](uint32_t c) -> uint32_t * {
        if constexpr (LIST) { const uint32_t ri = cr[c]; return ri == kMoveNone ? nullptr : a.rec + (size_t)ri * a.record_words + off + p0; }
        else return rec + (size_t)(c - c_lo) * a.record_words;
    };
    // record side: a lane touches its four positions in the order rot, rot + 1, ... (mod 4), see the bank arithmetic at the top
    const uint32_t rot = ((k >> 4) * (64u / kRunLanes)) & 3u;

    if (!IMPORT) {
        if (q_any)
            for (uint32_t r = r0; r < kTilePos; r += kRowsPerPass) {
                u4 v = u4{0u, 0u, 0u, 0u};
                if (p0 + r < len) v = *reinterpret_cast<const u4 *>(arr + (size_t)r * ROW + 4 * q);
                uint32_t *t = tile + r * kPitch + 4 * q;
                t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
            }
        __syncthreads();
        if (p0 + 4 * k < span)
            for (uint32_t c = c_lo + cc0; c < c_hi; c += kColsPerPass) {
                const uint32_t *t = tile + 4 * k * kPitch + c;
                const uint32_t w0 = t[rot * kPitch], w1 = t[((rot + 1) & 3u) * kPitch], w2 = t[((rot + 2) & 3u) * kPitch], w3 = t[((rot + 3) & 3u) * kPitch];
                const u4 v = u4{pick(w0, w1, w2, w3, (0u - rot) & 3u), pick(w0, w1, w2, w3, (1u - rot) & 3u), pick(w0, w1, w2, w3, (2u - rot) & 3u), pick(w0, w1, w2, w3, (3u - rot) & 3u)};
                uint32_t *const run = run_of(c);
                if (LIST && !run) continue;
                *reinterpret_cast<u4 *>(run + 4 * k) = v;
            }
    } else {
        if constexpr (REALIGN) {
            static_assert(kTilePos == 128 && kCols == 64 && kSnapThreads == 256, "the realigning record side's lane mapping");
            constexpr StateMap sm = make_state_map(ROW == 128 ? 1 : 0);
            constexpr uint32_t kLine = (uint32_t)sm.max_delay, kRing = (uint32_t)kRingLen;
            static_assert((kLine & (kLine - 1)) == 0 && kLine % kTilePos == 0 && kRing % kTilePos == 0, "a tile lies inside one line / ring");
            // the tile's plane: a line, a ring — or the whole section (state, PDM: d = 0, and a mask of all ones, "length 2^32", keeps p)
            const uint32_t pmask = sec == SEC_LINES ? kLine - 1u : sec == SEC_RING ? kRing - 1u : ~0u;
            const uint32_t kk = tid & 31u, c_lane = (tid >> 6) + 32u * ((tid >> 5) & 1u);
            for (uint32_t i = 0; i < kCols / 8; i++) {
                const uint32_t c = c_lane + 4u * i;
                if (c < c_lo || c >= c_hi) continue;
                size_t k_str, k_shift;      // column c's record, and its entry of the shift table
                if constexpr (LIST) { if (cr[c] == kMoveNone) continue; k_str = cr[c]; k_shift = (size_t)wg * ROW + col0 + c; }
                else k_str = k_shift = (size_t)(b0 + c - a.first);
                const uint2 sh = a.shift[k_shift];
                const uint32_t d = sec == SEC_LINES ? sh.x : sec == SEC_RING ? sh.y : 0u;
                const uint32_t *rc = a.rec + k_str * a.record_words + off;      // column c's section
                // (four loads in flight, then four LDS writes: a position past the section's span — the tile grid rounds up — reads the
                // section's word 0 instead, and the array side never looks at it)
                uint32_t v[4];
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t p = p0 + 32u * j + kk;
                    v[j] = rc[p < span ? (p & ~pmask) | snap_rot_source(p, d, pmask + 1u) : 0u];
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t pos = 32u * j + kk, p = p0 + pos;
                    if (sec == SEC_STATE) {      // the two position slots move with their lines
                        if (p == (uint32_t)sm.widx) v[j] = (v[j] + sh.x) & (kLine - 1u);
                        if (p == (uint32_t)sm.ring_pos) v[j] = (v[j] + sh.y) & (kRing - 1u);
                    }
                    tile[pos * kPitch + c] = v[j];
                }
            }
        } else if (p0 + 4 * k < span)
            for (uint32_t c = c_lo + cc0; c < c_hi; c += kColsPerPass) {
                const uint32_t *const run = run_of(c);
                if (LIST && !run) continue;
                const u4 v = *reinterpret_cast<const u4 *>(run + 4 * k);
                uint32_t *t = tile + 4 * k * kPitch + c;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) { const uint32_t i = (j + rot) & 3u; t[i * kPitch] = pick(v.x, v.y, v.z, v.w, i); }
            }
        __syncthreads();
        if (q_any)
            for (uint32_t r = r0; r < kTilePos; r += kRowsPerPass) {
                if (p0 + r >= len) break;
                const uint32_t *t = tile + r * kPitch + 4 * q;
                uint32_t *g = arr + (size_t)r * ROW + 4 * q;
                if (q_all) *reinterpret_cast<u4 *>(g) = u4{t[0], t[1], t[2], t[3]};
                else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) if (LIST ? cr[4 * q + j] != kMoveNone : 4 * q + j >= c_lo && 4 * q + j < c_hi) g[j] = t[j];
                }
            }
    }
}

// The records of streams [first, first + count) and where the shifts of their realigning import come from and go to: what both target rules'
// kernels take (one workgroup per touched row from row0 on, one thread per stream)
struct SnapTargetArgs {
    const uint32_t *state, *rec;
    uint32_t record_words, state_off, first, count, n_streams, row0;
    uint2 *shift;                      // per stream of [first, first + count)
};

__device__ __forceinline__ uint2 as_uint2(SnapPos p) { return make_uint2(p.widx, p.ring_pos); }

// How far the record of stream s is rotated to stand at target t's two positions: the target's (a resident neighbour's, from the state
// array as the stream's earlier work left it, or a stream of the records', from its record) minus the record's own.
template <uint32_t ROW>
__device__ __forceinline__ uint2 snap_shift_onto(const SnapTargetArgs &a, const SnapTarget t, uint64_t s) {
    constexpr StateMap sm = make_state_map(ROW == 128 ? 1 : 0);
    auto recorded = [&](uint64_t k) { return snap_positions_at(sm, a.rec + (size_t)(k - a.first) * a.record_words + a.state_off, 1); };
    return as_uint2(snap_shift_pair(sm, recorded(s), t.resident ? snap_positions(sm, a.state, t.stream) : recorded(t.stream)));
}

// The plain rule (dspi_snapshot.h snap_row_target): every stream of the range moves onto its row's target; nothing is written for threads
// outside the range.
template <uint32_t ROW>
__global__ __launch_bounds__(ROW) void snapshot_targets_kernel(const SnapTargetArgs a) {
    const uint32_t row = a.row0 + blockIdx.x;
    const uint64_t s = (uint64_t)row * ROW + threadIdx.x;
    if (s < a.first || s >= (uint64_t)a.first + a.count) return;
    a.shift[s - a.first] = snap_shift_onto<ROW>(a, snap_row_target(row, ROW, a.n_streams, a.first, a.count), s);
}

// ... for dspi_resume_streams: the activity-aware rule (dspi_snapshot.h snap_row_target_active) on the bitmap as it stood before the call.
// Only the streams the call resumes — in the call's range [r_first, r_first + r_count) and paused — move; every other stream of the
// records [first, first + count) (a chunk of the range's rows) gets the shift (0, 0) and is written back as it is.
template <uint32_t ROW>
__global__ __launch_bounds__(ROW) void snapshot_targets_active_kernel(const SnapTargetArgs a, const uint32_t *active, uint32_t r_first, uint32_t r_count) {
    const uint32_t row = a.row0 + blockIdx.x;
    const uint64_t s = (uint64_t)row * ROW + threadIdx.x;
    if (s < a.first || s >= (uint64_t)a.first + a.count) return;
    uint2 d = make_uint2(0u, 0u);
    // (a target from the records lies in this chunk: chunks hold the range's rows whole)
    if (s >= r_first && s < (uint64_t)r_first + r_count && !snap_stream_active(active, s))
        d = snap_shift_onto<ROW>(a, snap_row_target_active(row, ROW, a.n_streams, r_first, r_count, active), s);
    a.shift[s - a.first] = d;
}

// the snapshot_kernel instance of a flavour, launched
template <bool IMPORT, bool REALIGN, bool LIST>
void snap_launch(int flavor, dim3 grid, const typename SnapArgsOf<REALIGN, LIST>::type &a, hipStream_t stream) {
    for_row_width(flavor, [&](auto row) { hipLaunchKernelGGL((snapshot_kernel<decltype(row)::value, IMPORT, REALIGN, LIST>), grid, dim3(kSnapThreads), 0, stream, a); });
}

struct SnapGrid { dim3 grid; uint32_t rows; };
SnapGrid snap_kargs(SnapKArgs &a, int flavor, bool import, const StateArrays &arr, uint32_t *records, uint32_t first, uint32_t count) {
    const SnapLayout l = make_snap_layout(flavor);
    uint32_t *const arrs[SEC_COUNT] = {arr.state, arr.dlines, arr.ring, arr.pdm};
    const uint32_t pos = import ? kImportPos : kExportPos, cols = import ? kImportCols : kExportCols;
    uint32_t tiles = 0;
    for (int s = 0; s < SEC_COUNT; s++) {
        a.arr[s] = arrs[s]; a.len[s] = l.sec[s].len; a.off[s] = l.sec[s].offset; a.span[s] = l.sec[s].span;
        a.tile0[s] = tiles;
        tiles += (l.sec[s].span + pos - 1) / pos;
    }
    a.rec = records; a.record_words = l.record_words; a.first = first; a.count = count;
    a.row0 = first / l.row;
    const uint32_t rows = (uint32_t)(((uint64_t)first + count - 1) / l.row) - a.row0 + 1;
    return SnapGrid{dim3(tiles, rows, l.row / cols), rows};
}

// One thread per entry of a migration list, on the SOURCE context: the pair of the stream in slot slots[i], as the source's earlier work
// left it, into pos[i].
template <uint32_t ROW>
__global__ __launch_bounds__(kSnapThreads) void migrate_positions_kernel(const uint32_t *state, const uint32_t *slots, uint32_t n, uint2 *pos) {
    constexpr StateMap sm = make_state_map(ROW == 128 ? 1 : 0);
    const uint32_t i = blockIdx.x * kSnapThreads + threadIdx.x;
    if (i < n) pos[i] = as_uint2(snap_positions(sm, state, slots[i]));
}

// One thread per entry of a move or migration list (dspi_move.h list_targets), on the context that is written: how far the stream of entry i
// is rotated to stand at its row's target — a resident's pair, or another entry's.  An entry's own pair is pos[i] (a migration: the
// source's pairs, in list order) or, pos == nullptr (a move), read in place from slot `src`; a resident's is read from `state`; all as the
// context's earlier work left them and before any scatter of the call writes.
template <uint32_t ROW>
__global__ __launch_bounds__(kSnapThreads) void list_shifts_kernel(const uint32_t *state, const ListTarget *t, const uint2 *pos, uint32_t n, uint2 *shift) {
    constexpr StateMap sm = make_state_map(ROW == 128 ? 1 : 0);
    const uint32_t i = blockIdx.x * kSnapThreads + threadIdx.x;
    if (i >= n) return;
    const ListTarget e = t[i];
    auto entry = [&](uint32_t k) {
        if (!pos) return snap_positions(sm, state, t[k].src);
        const uint2 p = pos[k];
        return SnapPos{p.x, p.y};
    };
    shift[e.dst] = as_uint2(snap_shift_pair(sm, entry(i), e.from_entry ? entry(e.target) : snap_positions(sm, state, e.target)));
}

dim3 snap_list_kargs(SnapListArgs &a, int flavor, bool import, const StateArrays &arr, uint32_t *records, const uint32_t *items, const uint32_t *colrec, uint32_t n_items) {
    dim3 grid = snap_kargs(a, flavor, import, arr, records, 0, 1).grid;
    a.first = 0; a.count = 0; a.row0 = 0;
    a.items = reinterpret_cast<const MoveRowItem *>(items); a.colrec = colrec; a.shift = nullptr;
    grid.y = n_items;
    return grid;
}

}  // namespace

hipError_t launch_migrate_positions(int flavor, const uint32_t *state, const uint32_t *slots, uint32_t n, uint32_t *pos, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kSnapThreads - 1) / kSnapThreads);
    for_row_width(flavor, [&](auto row) { hipLaunchKernelGGL((migrate_positions_kernel<decltype(row)::value>), grid, dim3(kSnapThreads), 0, stream, state, slots, n, reinterpret_cast<uint2 *>(pos)); });
    return hipGetLastError();
}

hipError_t launch_list_shifts(int flavor, const uint32_t *state, const uint32_t *targets, const uint32_t *pos, uint32_t n, uint32_t *shift, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kSnapThreads - 1) / kSnapThreads);
    const ListTarget *t = reinterpret_cast<const ListTarget *>(targets);
    for_row_width(flavor, [&](auto row) {
        hipLaunchKernelGGL((list_shifts_kernel<decltype(row)::value>), grid, dim3(kSnapThreads), 0, stream, state, t, reinterpret_cast<const uint2 *>(pos), n, reinterpret_cast<uint2 *>(shift));
    });
    return hipGetLastError();
}

hipError_t launch_move_gather(int flavor, const StateArrays &arr, uint32_t *records, const uint32_t *items, const uint32_t *colrec, uint32_t n_items, hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    SnapListArgs a{};
    const dim3 grid = snap_list_kargs(a, flavor, false, arr, records, items, colrec, n_items);
    snap_launch<false, false, true>(flavor, grid, a, stream);
    return hipGetLastError();
}

hipError_t launch_move_scatter(int flavor, const StateArrays &arr, uint32_t *records, const uint32_t *items, const uint32_t *colrec, uint32_t n_items, const uint32_t *shift,
                               hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    SnapListArgs a{};
    const dim3 grid = snap_list_kargs(a, flavor, true, arr, records, items, colrec, n_items);
    a.shift = reinterpret_cast<const uint2 *>(shift);
    if (shift) snap_launch<true, true, true>(flavor, grid, a, stream);
    else snap_launch<true, false, true>(flavor, grid, a, stream);
    return hipGetLastError();
}

hipError_t launch_snapshot(int flavor, bool import, const StateArrays &arr, uint32_t *records, uint32_t first, uint32_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    SnapKArgs a{};
    const dim3 grid = snap_kargs(a, flavor, import, arr, records, first, count).grid;
    if (import) snap_launch<true, false, false>(flavor, grid, a, stream);
    else snap_launch<false, false, false>(flavor, grid, a, stream);
    return hipGetLastError();
}

// the shifts of the records' streams under the plain target rule or, `active` given, under the resume's, then the import rotated by them
hipError_t launch_snapshot_realign(int flavor, const StateArrays &arr, uint32_t *records, uint32_t first, uint32_t count, uint32_t n_streams, uint32_t *shift, hipStream_t stream,
                                   const uint32_t *active, uint32_t r_first, uint32_t r_count) {
    if (count == 0) return hipSuccess;
    SnapRealignArgs a{};
    const SnapGrid g = snap_kargs(a, flavor, true, arr, records, first, count);
    a.shift = reinterpret_cast<const uint2 *>(shift);
    const SnapTargetArgs t{arr.state, records, a.record_words, a.off[SEC_STATE], first, count, n_streams, a.row0, reinterpret_cast<uint2 *>(shift)};
    for_row_width(flavor, [&](auto row) {
        constexpr uint32_t ROW = decltype(row)::value;
        if (active) hipLaunchKernelGGL((snapshot_targets_active_kernel<ROW>), dim3(g.rows), dim3(ROW), 0, stream, t, active, r_first, r_count);
        else hipLaunchKernelGGL((snapshot_targets_kernel<ROW>), dim3(g.rows), dim3(ROW), 0, stream, t);
    });
    snap_launch<true, true, false>(flavor, g.grid, a, stream);
    return hipGetLastError();
}

}  // namespace dspi
