// dspi_linkrx.hip — the link receivers (dspi_link.h: views, links and where a link's words lie; dspi_spdifrx.h: the receiver's rule): the lines
// of another call's wire buffer, WHERE THEY LIE, into pair words (dspi_wire_decode) or into the packed 24-bit runs the chain reads
// (dspi_process_linked).  Destination i takes links[i]; a destination whose link is kLinkNone, or whose stream is paused, reads and writes
// nothing, its record included.
//
//   tiled view          one LANE per destination, 64 destinations per workgroup (one wave), the kind per lane — dspi_wire_tiled.hip read
//                       backwards.  A lane walks its link's column frame by frame (dspi_colwalk.h: the walk, shared with dspi_patchrx.hip).  An S/PDIF lane carries its record in registers, runs
//                       rx_frame (dspi_spdifrx.h, the sequential rule itself) per frame and writes the record back once; an I2S lane has
//                       none.  The row loads of a wave coalesce where neighbouring destinations link neighbouring columns of one region;
//                       any other map is as correct and slower.  At 65 536 destinations this is one wave per SIMD, so a lane keeps a GROUP
//                       of frames in flight: the 4 (S/PDIF) or 2 (I2S) row loads of the next kGroup frames are issued as one group before
//                       the walk over the group that has arrived.  Frames are not sliced over the grid: the receiver is sequential in F.
//   stream-major view   the S/PDIF links go through launch_spdifrx as it is (a wave per line, its offsets naming the lines); the I2S links take
//                       linkrx_i2s_kernel here: a wave per link, lanes over frames, one 8-byte load and 8 or 6 bytes stored.
// A packed run is only 2-byte aligned (6 F bytes per destination): three 2-byte stores per frame, as in dspi_spdifrx.hip.  No LDS, no scratch
// memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_colwalk.h"
#include "dspi_intake.h"
#include "dspi_kernels.h"
#include "dspi_link.h"

namespace dspi {

namespace {

struct LinkArgs {
    const uint32_t *wire;
    const Link *links;           // [count]
    const uint32_t *active;      // one bit per destination, or null: every one
    uint32_t *rx;                // [count] records of kRxWords words; null only when no link is S/PDIF
    void *dst;                   // kPacked: uint8 [count][6 frames]; else int32 [count][frames][2]
    uint32_t frames, n_pairs, row, count;
};

__device__ inline bool served(const LinkArgs &a, uint32_t i) { return !a.active || (a.active[i >> 5] >> (i & 31u) & 1u); }

template <bool kPacked>
__global__ __launch_bounds__(kLinkLanes) void linkrx_tiled_kernel(const LinkArgs a) {
    const uint32_t i = blockIdx.x * kLinkLanes + threadIdx.x;
    if (i >= a.count) return;
    const Link lk = a.links[i];
    if ((lk.kind != kLinkSpdif && lk.kind != kLinkI2s) || !served(a, i)) return;
    const uint32_t *const col = a.wire + link_region_tiled(lk.line, a.n_pairs, a.row, a.frames) + link_column(lk.line, a.n_pairs, a.row);
    walk_column<kPacked>(col, lk.kind, a.row, a.frames, a.rx + (size_t)i * kRxWords, a.dst, i);
}

// a frame's two slot words are one 8-byte word of the region's first half
static_assert(link_i2s_word(1, 0) == 2 && link_i2s_word(0, 1) == 1, "uint2 per frame");

template <bool kPacked>
__global__ __launch_bounds__(kLinkLanes) void linkrx_i2s_kernel(const LinkArgs a) {
    const uint32_t i = blockIdx.x;
    const Link lk = a.links[i];
    if (lk.kind != kLinkI2s || !served(a, i)) return;
    const uint2 *const in = reinterpret_cast<const uint2 *>(a.wire + link_region(lk.line, a.frames));      // (16 F bytes per line: 16-byte aligned)
    for (uint64_t f = threadIdx.x; f < a.frames; f += kLinkLanes) {
        const uint2 w = in[f];
        put<kPacked>(a.dst, i, a.frames, f, link_i2s_sample(w.x), link_i2s_sample(w.y));
    }
}

}  // namespace

hipError_t launch_linkrx(bool packed, const uint32_t *wire, const void *links, const uint64_t *offsets, const uint8_t *kinds, const uint32_t *active, void *rx, void *dst,
                         uint32_t frames, uint32_t n_pairs, uint32_t row, uint32_t count, bool any_spdif, bool any_i2s, hipStream_t stream) {
    if (!count || !frames || (!any_spdif && !any_i2s)) return hipSuccess;
    if (count > 0x7fffffffu || (row != 0 && row != 64 && row != 128) || (n_pairs != 2 && n_pairs != 4) || (any_spdif && !rx)) return hipErrorInvalidValue;
    const LinkArgs a{wire, static_cast<const Link *>(links), active, static_cast<uint32_t *>(rx), dst, frames, n_pairs, row, count};
    if (row) {
        const dim3 grid((count + kLinkLanes - 1) / kLinkLanes);
        if (packed) hipLaunchKernelGGL(linkrx_tiled_kernel<true>, grid, dim3(kLinkLanes), 0, stream, a);
        else hipLaunchKernelGGL(linkrx_tiled_kernel<false>, grid, dim3(kLinkLanes), 0, stream, a);
        return hipGetLastError();
    }
    if (any_spdif) {
        const hipError_t e = launch_spdifrx(packed, wire, offsets, kinds, active, rx, dst, frames, 0u, count, stream);
        if (e != hipSuccess) return e;
    }
    if (any_i2s) {
        if (packed) hipLaunchKernelGGL(linkrx_i2s_kernel<true>, dim3(count), dim3(kLinkLanes), 0, stream, a);
        else hipLaunchKernelGGL(linkrx_i2s_kernel<false>, dim3(count), dim3(kLinkLanes), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace dspi
