// dspi_patchrx.hip — the tiled receiver of dspi_process_patched (dspi_patch.h: the plan and the resolved patches; dspi_colwalk.h: the walk):
// every tiled view of a call in ONE launch, whatever their tile sizes (64 and 128 mixed) and pair counts.
//   grid          one LANE per destination stream, 64 per workgroup (one wave), as dspi_linkrx.hip's tiled kernel.
//   lane          loads its 16-byte resolved patch {column, R, kind}: the host has turned (view, line) into the device address of the column's
//                 first word, so the kernel holds no table of views — one passed by value and indexed per lane would live in scratch memory.  A
//                 lane whose kind is NONE (a paused stream, a stream of another source, a patch into a stream-major view) reads and writes
//                 nothing more, its record included.  The others run walk_column, the one receiver dspi_linkrx.hip runs: kGroup frames of row
//                 loads in flight, rx_frame per frame, the record in registers written back once, the packed 24-bit run the chain reads.
//   R             per lane here (per launch there): the row stride of the loads is a vector register.  Neighbouring lanes that patch
//                 neighbouring columns of one region still coalesce; any other map is as correct and slower.
// The column pointer is made from an integer; it is given the global address space by hand so that the loads are global, not flat, loads as
// they are in dspi_linkrx.hip.  No LDS, no scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_colwalk.h"
#include "dspi_kernels.h"
#include "dspi_patch.h"

namespace dspi {

namespace {

typedef const __attribute__((address_space(1))) uint32_t *GlobalWords;

struct PatchArgs {
    const PatchCol *cols;      // [count]
    uint32_t *rx;              // [count] records of kRxWords words; null only when no patch is S/PDIF
    void *dst;                 // uint8 [count][6 frames]
    uint32_t frames, count;
};

__global__ __launch_bounds__(kLinkLanes) void patchrx_kernel(const PatchArgs a) {
    const uint32_t i = blockIdx.x * kLinkLanes + threadIdx.x;
    if (i >= a.count) return;
    const PatchCol pc = a.cols[i];
    if (pc.kind != kLinkSpdif && pc.kind != kLinkI2s) return;
    walk_column<true>((GlobalWords)pc.col, pc.kind, pc.row, a.frames, a.rx + (size_t)i * kRxWords, a.dst, i);
}

}  // namespace

hipError_t launch_patchrx(const void *cols, void *rx, void *dst, uint32_t frames, uint32_t count, bool any_spdif, hipStream_t stream) {
    if (!count || !frames) return hipSuccess;
    if (count > 0x7fffffffu || (any_spdif && !rx) || reinterpret_cast<uintptr_t>(cols) % 16u) return hipErrorInvalidValue;
    const PatchArgs a{static_cast<const PatchCol *>(cols), static_cast<uint32_t *>(rx), dst, frames, count};
    hipLaunchKernelGGL(patchrx_kernel, dim3((count + kLinkLanes - 1) / kLinkLanes), dim3(kLinkLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi
