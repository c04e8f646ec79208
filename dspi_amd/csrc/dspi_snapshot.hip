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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_snapshot.h"

namespace dspi {

static_assert(kPdmWords == kPdmStateWords, "the snapshot's PDM section is the modulator's state");

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

// word i of four, i known at run time only: selects, so that the four stay in registers
__device__ __forceinline__ uint32_t pick(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) { return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3; }

template <uint32_t ROW, bool IMPORT>
__global__ __launch_bounds__(kSnapThreads) void snapshot_kernel(const SnapKArgs a) {
    constexpr uint32_t kTilePos = IMPORT ? kImportPos : kExportPos, kCols = IMPORT ? kImportCols : kExportCols;
    static_assert(ROW % kCols == 0 && kCols % 4 == 0 && kTilePos % 4 == 0 && kSnapThreads % (kCols / 4) == 0 && kSnapThreads % (kTilePos / 4) == 0, "tile shape");
    constexpr uint32_t kPitch = kCols + 1, kRowLanes = kCols / 4, kRowsPerPass = kSnapThreads / kRowLanes, kRunLanes = kTilePos / 4, kColsPerPass = kSnapThreads / kRunLanes;
    __shared__ uint32_t tile[kTilePos * kPitch];
    // the tile's section (constant indices only: a run-time index into the argument block would put it in scratch)
    uint32_t *base = a.arr[0];
    uint32_t len = a.len[0], span = a.span[0], off = a.off[0], t0 = 0;
#pragma unroll
    for (int i = 1; i < SEC_COUNT; i++)
        if (blockIdx.x >= a.tile0[i]) { base = a.arr[i]; len = a.len[i]; span = a.span[i]; off = a.off[i]; t0 = a.tile0[i]; }
    const uint32_t wg = a.row0 + blockIdx.y, p0 = (blockIdx.x - t0) * kTilePos, col0 = blockIdx.z * kCols;
    // the tile's columns inside [first, first + count)
    const uint64_t s0 = (uint64_t)wg * ROW, b0 = s0 + col0, lo = a.first > b0 ? a.first : b0, end = (uint64_t)a.first + a.count, hi = end < b0 + kCols ? end : b0 + kCols;
    if (hi <= lo) return;
    const uint32_t c_lo = (uint32_t)(lo - b0), c_hi = (uint32_t)(hi - b0);      // relative to col0
    uint32_t *const arr = base + ((size_t)wg * len + p0) * ROW + col0;
    uint32_t *const rec = a.rec + (size_t)(b0 + c_lo - a.first) * a.record_words + off + p0;      // column c_lo's run
    const uint32_t tid = threadIdx.x;
    const uint32_t q = tid % kRowLanes, r0 = tid / kRowLanes;       // array side: columns 4q .. 4q + 3 of position p0 + r
    const uint32_t k = tid % kRunLanes, cc0 = tid / kRunLanes;      // record side: positions p0 + 4k .. + 3 of column c
    const bool q_any = 4 * q + 4 > c_lo && 4 * q < c_hi, q_all = 4 * q >= c_lo && 4 * q + 4 <= c_hi;
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
                *reinterpret_cast<u4 *>(rec + (size_t)(c - c_lo) * a.record_words + 4 * k) = v;
            }
    } else {
        if (p0 + 4 * k < span)
            for (uint32_t c = c_lo + cc0; c < c_hi; c += kColsPerPass) {
                const u4 v = *reinterpret_cast<const u4 *>(rec + (size_t)(c - c_lo) * a.record_words + 4 * k);
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
                    for (uint32_t j = 0; j < 4; j++) if (4 * q + j >= c_lo && 4 * q + j < c_hi) g[j] = t[j];
                }
            }
    }
}

}  // namespace

hipError_t launch_snapshot(int flavor, bool import, uint32_t *state, uint32_t *dlines, uint32_t *ring, uint32_t *pdm, uint32_t *records, uint32_t first,
                           uint32_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const SnapLayout l = make_snap_layout(flavor);
    SnapKArgs a{};
    uint32_t *const arrs[SEC_COUNT] = {state, dlines, ring, pdm};
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
    const dim3 grid(tiles, rows, l.row / cols);
    if (flavor) {
        if (import) hipLaunchKernelGGL((snapshot_kernel<128, true>), grid, dim3(kSnapThreads), 0, stream, a);
        else hipLaunchKernelGGL((snapshot_kernel<128, false>), grid, dim3(kSnapThreads), 0, stream, a);
    } else {
        if (import) hipLaunchKernelGGL((snapshot_kernel<64, true>), grid, dim3(kSnapThreads), 0, stream, a);
        else hipLaunchKernelGGL((snapshot_kernel<64, false>), grid, dim3(kSnapThreads), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace dspi
