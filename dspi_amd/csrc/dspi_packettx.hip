// dspi_packettx.hip — dspi_packets_emit on the GPU: the pair words a process call left, stream-major or tiled, into the caller's arena as one
// packet per (stream, pair, packet), each where the table (dspi_packets_out.h) points: block_len frames of 8 bytes (format 32: the words as
// they stand) or 6 (format 24: the low three bytes of each, a USB packet).  A paused stream and a skip entry are neither read nor written.
//
// THE DESTINATION SIDE is dspi_packetrx.hip's, turned round, and both kernels share it.  An entry is any even offset, so a packet starts
// anywhere in a 16-byte piece of the arena and its neighbours in the arena are other packets, or bytes that are not the call's at all.  A lane
// group (kEmitLanes = 16 lanes) owns a SPAN of destination bytes [a, b) — a packet, or a chunk of one — and cuts it on ABSOLUTE 16-byte
// boundaries: a piece that lies inside the span is one 16-byte store, the span's first and last piece are stored as the 2-byte words inside
// [a, b) only.  Nothing is read back and no store is wider than what the span owns, so nothing outside the union of the entries is ever
// written, whatever the table holds; where two entries overlap, each byte of the overlap takes one of the two stores that meet there.
// The bytes come from an LDS image of the span that keeps the DESTINATION's alignment: frame f of the span stands at (a - image0) + fb f,
// narrowed already (emit_frame_words: four 16-bit words for format 32, three for format 24), so a whole piece is read from LDS as it goes out.
//
// STREAM-MAJOR SOURCE (packettx_major_kernel).  With F = n_blocks block_len the run of entry e = (s n_pairs + p) n_blocks + k starts 8 e
// block_len bytes into the buffer: the entries in table order ARE the source in memory order.  A lane group serves an entry, a workgroup of
// 256 threads kEmitGroups = 16 neighbouring ones at the same time (one chain of dependent accesses — entry, source, LDS, destination — per
// workgroup, as in the receiver); a lane loads a frame (8 bytes: runs start at multiples of 8 block_len, which are not multiples of 16 when
// block_len is odd) and puts its three or four words into the group's image, image0 = a & ~15.  LDS: kEmitMajorPitch = 1 792 bytes per group
// (14 + 8 x 192 rounded up to a multiple of 256), 28 KiB per workgroup.  The pitch is a multiple of 256 bytes so that piece i of every
// group's image starts in bank 4 i mod 64: the 16 lanes that one cycle of a 16-byte LDS read serves (8 + 8 lanes of two neighbouring
// groups: pieces 0-3 and 12-15 of one with 4-11 of the other) then touch 64 different banks.
//
// TILED SOURCE (packettx_tiled_kernel<R>).  [tile][output][F][R]: a column's words lie R x 4 bytes apart, which is how they must not be
// read.  A workgroup takes (tile, pair, packet, chunk of kEmitChunk = 32 frames) and
//   0. looks up its R columns' entries: info[c] = offset | (format == 24), or the skip word for a column that emits nothing (past n_streams,
//      paused, a skip entry);
//   1. loads the chunk's rows of outputs 2 pair and 2 pair + 1 whole: a thread takes 4 columns of one frame, 16 bytes of the left row and
//      16 of the right, both in flight, R / 4 threads per row and 8 (R = 128) or 16 (R = 64) frames per pass; where one of its four columns
//      emits nothing it loads the others' words singly, so a paused column is not read; and puts each column's frame into THAT COLUMN'S
//      image (the transposition), narrowed;
//   2. writes each column's span from its image: a lane group per column, 16 columns per pass.
// A chunk of 32 frames is 192 or 256 bytes of every packet — multiples of 16, so a chunk's span is aligned like its packet and only a
// packet that is itself misaligned pays 2-byte stores at chunk boundaries (a halo of three frames per chunk would remove them; not built).
// LDS: a column's image is kEmitTiledPitch = 65 words (2 + 8 x 32 bytes), image0 = a & ~3: R x 260 bytes = 32.5 / 16.3 KiB, and 1 / 0.5 KiB
// of info.  The pitch is ODD (so no 16-byte LDS access: four 4-byte ones per piece, as dspi_snapshot.hip's record side), P = 1 mod 32:
//   step 1  the lanes of one LDS cycle (32) are 32 column quads q of one frame (R = 128) or 16 quads of two frames (R = 64); column 4q + j's
//           word sits in bank 4q + j + const (mod 32), eight banks four times over for one j — so a lane takes its columns in the order
//           j + q / 8: quads 8 apart then sit 1, 2, 3 banks apart, 32 different banks (R = 64: 16, the second frame two words on: 32);
//   step 2  the lanes of one cycle are two neighbouring columns' groups; word w of piece i of column c sits in bank c + 4i + w (mod 32), lanes
//           i and i + 8 of a column would meet — so a lane takes its four words in the order w + 2 (lane / 8): the two halves of columns c and
//           c + 1 sit 0, 2, 1, 3 banks on: 32 different banks.
// Both hold where the columns of a cycle agree in format and alignment (a fleet of like devices laid out regularly); where they do not the
// kernel is as correct and pays conflicts.  All the address arithmetic is dspi_packets_out.h's, which tests/packets_out_driver.cpp walks on
// the CPU for every workgroup, lane group, lane and iteration of both kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_kernels.h"
#include "dspi_packets_out.h"

namespace dspi {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct PacketTxArgs {
    const int32_t *pairs;        // the source, either layout
    const uint64_t *table;       // [n_streams][n_pairs][n_blocks]
    const uint8_t *formats;      // [n_streams]: 24 or 32
    const uint32_t *active;      // one bit per stream, or null: every stream
    uint8_t *arena;
    uint64_t entries;            // n_streams * n_pairs * n_blocks
    uint32_t n_streams, n_pairs, n_blocks, block_len;
};

// word i of four, i known at run time only: selects, so that the four stay in registers
__device__ __forceinline__ uint32_t pick(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) { return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3; }

__device__ __forceinline__ uint64_t pick64(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t i) { return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3; }

__device__ __forceinline__ bool stream_active(const uint32_t *active, uint32_t s) { return !active || (active[s >> 5] >> (s & 31u) & 1u); }

// a frame into an image (image16: the image's 16-bit words)
__device__ __forceinline__ void put_frame(uint16_t *image16, const EmitSpan &S, uint32_t f, uint32_t l, uint32_t r) {
    uint16_t w[4];
    const uint32_t n = emit_frame_words(l, r, S.fb, w), at = emit_frame_at(S, f) / 2u;
    image16[at] = w[0]; image16[at + 1] = w[1]; image16[at + 2] = w[2];
    if (n == 4u) image16[at + 3] = w[3];
}

// a partial piece at p: the 2-byte words inside the span, singly
__device__ __forceinline__ void store_partial(uint8_t *arena, uint64_t dst0, const uint16_t *image16, const EmitSpan &S, uint64_t p) {
    for (uint32_t w = 0; w < 8; w++) {
        const uint64_t q = p + 2u * w;
        if (q >= S.a && q < S.b) *reinterpret_cast<uint16_t *>(arena + (q - dst0)) = image16[(q - S.image0) / 2u];
    }
}

__global__ __launch_bounds__(kEmitThreads) void packettx_major_kernel(const PacketTxArgs a) {
    __shared__ u4 images[kEmitGroups][kEmitMajorPitch / 16];
    const uint32_t group = threadIdx.x / kEmitLanes, lane = threadIdx.x % kEmitLanes;
    u4 *const image4 = images[group];
    uint16_t *const image16 = reinterpret_cast<uint16_t *>(image4);
    // alignment is a matter of addresses; the accesses themselves go through the two argument pointers (global, not flat, instructions)
    const uint64_t src0 = reinterpret_cast<uintptr_t>(a.pairs), dst0 = reinterpret_cast<uintptr_t>(a.arena);
    const uint8_t *const src = reinterpret_cast<const uint8_t *>(a.pairs);

    // (everything that decides `on` is the group's, not the lane's)
    const uint64_t e = emit_major_entry(blockIdx.x, group);
    bool on = e < a.entries;
    uint32_t s = 0;
    uint64_t offset = kPacketSkip;
    if (on) { s = emit_major_stream(e, a.n_pairs, a.n_blocks); on = stream_active(a.active, s); }
    if (on) { offset = a.table[e]; on = offset != kPacketSkip; }
    EmitSpan S{};
    if (on) {      // source -> LDS
        S = emit_major_span(dst0, offset, a.formats[s], a.block_len);
        uint32_t f;
        uint64_t p;
        for (uint32_t i = 0; emit_major_src(src0, e, a.block_len, lane, i, &f, &p); i++) {
            const u2 v = *reinterpret_cast<const u2 *>(src + (p - src0));
            put_frame(image16, S, f, v.x, v.y);
        }
    }
    __syncthreads();
    if (!on) return;
    uint64_t p;
    bool whole;
    for (uint32_t i = 0; emit_dst_piece(S, lane, i, &p, &whole); i++) {
        if (whole) *reinterpret_cast<u4 *>(a.arena + (p - dst0)) = image4[(p - S.image0) >> 4];
        else store_partial(a.arena, dst0, image16, S, p);
    }
}

template <uint32_t R>
__global__ __launch_bounds__(kEmitThreads) void packettx_tiled_kernel(const PacketTxArgs a) {
    static_assert(R % kEmitGroups == 0 && R <= kEmitThreads && kEmitThreads % (R / 4) == 0, "the tile's lane mappings");
    __shared__ uint32_t images[R * kEmitTiledPitch];
    __shared__ uint64_t info[R];
    const uint32_t tid = threadIdx.x;
    const uint64_t src0 = reinterpret_cast<uintptr_t>(a.pairs), dst0 = reinterpret_cast<uintptr_t>(a.arena);
    const uint8_t *const src = reinterpret_cast<const uint8_t *>(a.pairs);
    const EmitTiledJob J = emit_tiled_job(blockIdx.x, a.n_pairs, a.n_blocks, a.block_len);
    auto span_of = [&](uint64_t word) { return emit_tiled_span(dst0, word & ~1ull, (word & 1u) ? 24u : 32u, J); };
    auto image16_of = [&](uint32_t c) { return reinterpret_cast<uint16_t *>(images + c * kEmitTiledPitch); };

    // 0. the columns' entries
    if (tid < R) {
        const uint64_t s = (uint64_t)J.tile * R + tid;
        uint64_t word = kPacketSkip;
        if (s < a.n_streams && stream_active(a.active, (uint32_t)s)) {
            const uint64_t offset = a.table[emit_entry_index((uint32_t)s, J.pair, J.k, a.n_pairs, a.n_blocks)];
            if (offset != kPacketSkip) word = offset | (a.formats[s] == 24 ? 1u : 0u);
        }
        info[tid] = word;
    }
    __syncthreads();
    // 1. rows -> the columns' images
    {
        uint32_t fr, q;
        uint64_t pl, pr;
        if (emit_tiled_src(src0, J, R, a.n_pairs, a.n_blocks, a.block_len, tid, 0, &fr, &q, &pl, &pr)) {
            const uint64_t w0 = info[4 * q], w1 = info[4 * q + 1], w2 = info[4 * q + 2], w3 = info[4 * q + 3];
            const uint32_t mask = (w0 != kPacketSkip) | (w1 != kPacketSkip) << 1 | (w2 != kPacketSkip) << 2 | (w3 != kPacketSkip) << 3;
            const uint32_t rot = (q >> 3) & 3u;
            if (mask)
                for (uint32_t i = 0; emit_tiled_src(src0, J, R, a.n_pairs, a.n_blocks, a.block_len, tid, i, &fr, &q, &pl, &pr); i++) {
                    u4 l = u4{0u, 0u, 0u, 0u}, r = l;
                    const uint32_t *const gl = reinterpret_cast<const uint32_t *>(src + (pl - src0)), *const gr = reinterpret_cast<const uint32_t *>(src + (pr - src0));
                    if (emit_tiled_whole(mask)) {
                        l = *reinterpret_cast<const u4 *>(gl); r = *reinterpret_cast<const u4 *>(gr);
                    } else {
                        if (mask & 1u) { l.x = gl[0]; r.x = gr[0]; }
                        if (mask & 2u) { l.y = gl[1]; r.y = gr[1]; }
                        if (mask & 4u) { l.z = gl[2]; r.z = gr[2]; }
                        if (mask & 8u) { l.w = gl[3]; r.w = gr[3]; }
                    }
#pragma unroll
                    for (uint32_t jj = 0; jj < 4; jj++) {
                        const uint32_t j = (jj + rot) & 3u;
                        if (!(mask >> j & 1u)) continue;
                        put_frame(image16_of(4 * q + j), span_of(pick64(w0, w1, w2, w3, j)), fr, pick(l.x, l.y, l.z, l.w, j), pick(r.x, r.y, r.z, r.w, j));
                    }
                }
        }
    }
    __syncthreads();
    // 2. the columns' images -> their spans
    const uint32_t group = tid / kEmitLanes, lane = tid % kEmitLanes, rot = 2u * (lane >> 3);
    uint32_t c;
    for (uint32_t i = 0; emit_tiled_col(R, group, i, &c); i++) {
        const uint64_t word = info[c];
        if (word == kPacketSkip) continue;
        const EmitSpan S = span_of(word);
        const uint32_t *const image = images + c * kEmitTiledPitch;
        uint64_t p;
        bool whole;
        for (uint32_t n = 0; emit_dst_piece(S, lane, n, &p, &whole); n++) {
            if (whole) {
                const uint32_t *const t = image + ((p - S.image0) >> 2);
                const uint32_t v0 = t[rot & 3u], v1 = t[(rot + 1u) & 3u], v2 = t[(rot + 2u) & 3u], v3 = t[(rot + 3u) & 3u];
                *reinterpret_cast<u4 *>(a.arena + (p - dst0)) = u4{pick(v0, v1, v2, v3, (0u - rot) & 3u), pick(v0, v1, v2, v3, (1u - rot) & 3u), pick(v0, v1, v2, v3, (2u - rot) & 3u),
                                                                   pick(v0, v1, v2, v3, (3u - rot) & 3u)};
            } else store_partial(a.arena, dst0, reinterpret_cast<const uint16_t *>(image), S, p);
        }
    }
}

}  // namespace

hipError_t launch_packettx(const int32_t *pairs, uint32_t tile_streams, const uint64_t *table, const uint8_t *formats, const uint32_t *active, void *arena, uint32_t n_streams,
                           uint32_t n_pairs, uint32_t n_blocks, uint32_t block_len, hipStream_t stream) {
    if (!n_streams || !n_pairs || !n_blocks || !block_len) return hipSuccess;
    const uint64_t entries = (uint64_t)n_streams * n_pairs * n_blocks;
    if (entries > kPacketMaxEntries || block_len * 8u + 16u > kEmitMajorPitch) return hipErrorInvalidValue;
    const PacketTxArgs a{pairs, table, formats, active, static_cast<uint8_t *>(arena), entries, n_streams, n_pairs, n_blocks, block_len};
    if (!tile_streams) {
        hipLaunchKernelGGL(packettx_major_kernel, dim3((uint32_t)((entries + kEmitGroups - 1) / kEmitGroups)), dim3(kEmitThreads), 0, stream, a);
        return hipGetLastError();
    }
    if (tile_streams != 128u && tile_streams != 64u) return hipErrorInvalidValue;
    const uint64_t wgs = emit_tiled_workgroups(n_streams, tile_streams, n_pairs, n_blocks, block_len);
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    if (tile_streams == 128u) hipLaunchKernelGGL((packettx_tiled_kernel<128>), dim3((uint32_t)wgs), dim3(kEmitThreads), 0, stream, a);
    else hipLaunchKernelGGL((packettx_tiled_kernel<64>), dim3((uint32_t)wgs), dim3(kEmitThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi
