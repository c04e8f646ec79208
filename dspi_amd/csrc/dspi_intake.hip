// dspi_intake.hip — the intake of dspi_process_mixed: the caller's runs of 16- and 24-bit frames (dspi_intake.h) into the tight packed
// 24-bit array [stream][6F] that the chain kernels read.  A 24-bit run is copied, a 16-bit run is widened (sample s becomes 00 lo hi:
// s << 8); a paused stream is skipped, nothing of it is read or written.  Pure data movement: 4 or 6 bytes read and 6 written per frame.
//
// Both sides are byte arrays whose runs start on 2-byte boundaries only (a 24-bit run of an odd frame count is 6 mod 16 bytes long, and so
// is every destination run), so the two sides of a run are, as a rule, aligned differently.  16-byte accesses on both sides therefore go
// through LDS:
//   grid          one workgroup per (stream, tile); blockIdx.x = (stream - first) * tiles + tile.  A tile is kTile = 4 KiB of the
//                 DESTINATION, cut on absolute 16-byte boundaries (tile t of a stream starts at floor16(the run's first address) + t kTile
//                 and is clipped to the run), so every destination piece below is one aligned 16 bytes.  tiles = (6F + 14) / kTile + 1
//                 covers the worst alignment; a tile that the run does not reach returns at once.
//   workgroup     one wave of 64 lanes.  Runs are short where streams are many (288 bytes at 48 frames): a larger workgroup would idle,
//                 and a wave needs no barrier partner.  A lane serves pieces lane, lane + 64, ...: up to four of each kind.
//   source side   the bytes the tile needs — [ra, rb) of a 24-bit run; samples ra / 3 .. (rb - 1) / 3 of a 16-bit run, i.e. two thirds as
//                 many bytes — go to LDS at (address mod 16) + 16 i: the aligned 16-byte pieces inside that range as one 16-byte load and
//                 one 16-byte LDS store per lane, the up to seven 2-byte words in front of the first and behind the last piece singly.
//                 Nothing outside the range is read: a neighbour's bytes may belong to a paused stream, or lie outside the caller's buffer.
//   LDS           kTile + 16 bytes, an image of the source range that keeps its alignment mod 16.
//   destination   every destination 2-byte word is a function of ONE source word: copied (24 bit), or with b = its byte offset in the run,
//                 k = b / 3 the sample, r = b mod 3: (lo << 8, the word, hi) for r = (0, 1, 2) — 00 lo | lo hi | hi 00.  A lane gathers the
//                 eight words of a piece from LDS (2-byte reads: the image is aligned like the source, not like the piece) and stores 16
//                 bytes; a piece that the run covers only in part — its first and last, which it may share with the neighbours' runs — is
//                 stored as 2-byte words, the run's own only.
// The 2-byte LDS reads of neighbouring lanes are 16 (24 bit) or 10 2/3 (16 bit) bytes apart: lanes l and l + 16 of a half wave meet in one
// bank, a 2-way conflict, on a kernel that moves 10 bytes per frame and waits for memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_intake.h"
#include "dspi_kernels.h"

namespace dspi {

namespace {

constexpr uint32_t kIntakeLanes = 64;
constexpr uint32_t kIntakeTile = 4096;      // destination bytes per workgroup
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct IntakeArgs {
    const uint8_t *src;          // the caller's bytes: stream s at src + offsets[s]
    const uint64_t *offsets;     // [n_streams + 1]
    const uint8_t *depths;       // [n_streams]: 16 or 24
    const uint32_t *active;      // one bit per stream, or null: every stream
    uint8_t *dst;                // [n_streams][run]
    uint64_t run;                // 6F: bytes of a destination run
    uint32_t first, tiles;
};

__global__ __launch_bounds__(kIntakeLanes) void intake_kernel(const IntakeArgs a) {
    __shared__ u4 image4[kIntakeTile / 16 + 1];
    uint16_t *const image = reinterpret_cast<uint16_t *>(image4);
    const uint32_t lane = threadIdx.x;
    // alignment is a matter of addresses; the accesses themselves go through the two argument pointers (global, not flat, instructions)
    const uintptr_t src0 = reinterpret_cast<uintptr_t>(a.src), dst0 = reinterpret_cast<uintptr_t>(a.dst);
    auto src_at = [&](uintptr_t p) { return a.src + (p - src0); };
    auto dst_at = [&](uintptr_t p) { return a.dst + (p - dst0); };
    const uint32_t s = a.first + blockIdx.x / a.tiles, t = blockIdx.x % a.tiles;
    if (a.active && !(a.active[s >> 5] >> (s & 31u) & 1u)) return;
    const bool wide = a.depths[s] == 24;

    // the tile's part of the destination run, as addresses: [ta, tb)
    const uintptr_t d0 = dst0 + a.run * s, d1 = d0 + a.run;
    const uintptr_t piece0 = (d0 & ~(uintptr_t)15) + (uintptr_t)t * kIntakeTile;
    const uintptr_t ta = piece0 > d0 ? piece0 : d0, tb = piece0 + kIntakeTile < d1 ? piece0 + kIntakeTile : d1;
    if (ta >= tb) return;
    // ... as byte offsets in the run [ra, rb), and the source bytes they come from [sa, sb) (addresses); r0: ra's place in its sample
    const uint64_t ra = ta - d0, rb = tb - d0;
    const uint64_t k0 = ra / 3u;
    const uint32_t r0 = (uint32_t)(ra - 3u * k0);
    const uintptr_t s0 = src0 + a.offsets[s];
    const uintptr_t sa = s0 + (wide ? ra : 2u * k0), sb = s0 + (wide ? rb : 2u * ((rb - 1u) / 3u + 1u));
    const uintptr_t image0 = sa & ~(uintptr_t)15;      // the address LDS byte 0 stands for

    // source -> LDS: whole 16-byte pieces [ha, hb), single words in front [sa, ha) and behind [hb, sb)
    const uintptr_t up = (sa + 15u) & ~(uintptr_t)15;
    const uintptr_t ha = up < sb ? up : sb, hb = ha > (sb & ~(uintptr_t)15) ? ha : (sb & ~(uintptr_t)15);
    for (uintptr_t p = ha + 16u * lane; p < hb; p += 16u * kIntakeLanes)
        image4[(p - image0) >> 4] = *reinterpret_cast<const u4 *>(src_at(p));
    if (sa + 2u * lane < ha) image[(sa - image0) / 2u + lane] = *reinterpret_cast<const uint16_t *>(src_at(sa + 2u * lane));
    if (hb + 2u * lane < sb) image[(hb - image0) / 2u + lane] = *reinterpret_cast<const uint16_t *>(src_at(hb + 2u * lane));
    __syncthreads();

    // LDS -> destination.  word(j): the destination word 2j bytes behind ta
    const uint32_t base = (uint32_t)(sa - image0) / 2u;
    auto word = [&](uint32_t j) -> uint32_t {
        if (wide) return image[base + j];
        const uint32_t b = r0 + 2u * j, k = b / 3u, r = b - 3u * k;
        const uint32_t v = image[base + k];
        return r == 0 ? (v & 0xffu) << 8 : r == 1 ? v : v >> 8;
    };
    for (uintptr_t p = piece0 + 16u * lane; p < tb; p += 16u * kIntakeLanes) {
        if (p >= ta && p + 16u <= tb) {
            const uint32_t j = (uint32_t)(p - ta) / 2u;
            u4 v;
            v.x = word(j) | word(j + 1) << 16; v.y = word(j + 2) | word(j + 3) << 16;
            v.z = word(j + 4) | word(j + 5) << 16; v.w = word(j + 6) | word(j + 7) << 16;
            *reinterpret_cast<u4 *>(dst_at(p)) = v;
        } else {
            for (uint32_t i = 0; i < 8; i++) {
                const uintptr_t q = p + 2u * i;
                if (q >= ta && q < tb) *reinterpret_cast<uint16_t *>(dst_at(q)) = (uint16_t)word((uint32_t)(q - ta) / 2u);
            }
        }
    }
}

}  // namespace

hipError_t launch_intake(const void *src, const uint64_t *offsets, const uint8_t *depths, const uint32_t *active, void *dst, uint64_t frames,
                         uint32_t first, uint32_t count, hipStream_t stream) {
    if (!count || !frames) return hipSuccess;
    const uint64_t run = frames * kIntakeOutFrame;
    const uint64_t tiles = (run + 14u) / kIntakeTile + 1u;
    if (tiles * count > 0x7fffffffull) return hipErrorInvalidValue;
    IntakeArgs a{static_cast<const uint8_t *>(src), offsets, depths, active, static_cast<uint8_t *>(dst), run, first, (uint32_t)tiles};
    hipLaunchKernelGGL(intake_kernel, dim3((uint32_t)(tiles * count)), dim3(kIntakeLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi
