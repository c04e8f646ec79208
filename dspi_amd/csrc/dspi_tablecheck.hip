// dspi_tablecheck.hip — the entry check of a packet table in device memory: ONE kernel for the input table of dspi_process_packets and the emit
// table of dspi_packets_emit, which answers with the lowest index of an entry of an active stream that the entry rule refuses, or all ones.
// Everything that decides which bytes are loaded and which entry a lane judges is dspi_tablecheck.h's (tablecheck_lane and the functions under
// it), which tests/tablecheck_driver.cpp walks on the CPU for every workgroup and thread; this file supplies the loads and the reduction.
//
// THE SHAPE.  The kernel only reads: 8 bytes per entry, the stream's kind byte and its activity word (both a few KB, cache hits).  A thread
// takes two neighbouring entries with one 16-byte load (the table is 16-byte aligned; the last entry of an odd count is read singly by one
// thread), workgroups of 256 threads walk the table in a grid-stride loop, and the grid is capped (kTableCheckDefaultWgs: four workgroups per
// CU) so that a table of millions of entries costs a thousand workgroups, not tens of thousands.  The stream of an entry is index /
// per_stream: one 32-bit division per pair.
//
// THE REDUCTION.  Each lane keeps the minimum of the indices it refused; a butterfly of __shfl_xor brings the wave's minimum to every lane,
// lane 0 of each of the four waves leaves it in LDS, and thread 0 of the workgroup brings the workgroup's minimum into the answer word.
// ONE 64-BIT ATOMIC MINIMUM (global_atomic_umin_x2, a vector memory instruction, relaxed, agent scope), NOT a slot array with a second pass:
// a workgroup that refused nothing issues no atomic at all, so the table that matters — a legal one, every call of a running fleet — costs
// none, and a refused table costs at most one per workgroup, a thousand on one word, once, on the way to an error return.  A slot array
// would add a second dependent launch (or an in-launch hand-off with its fences) to every call in order to save atomics that the good case
// never issues.  The answer is a minimum of integers: whatever order the atomics arrive in, the word ends the same.  The launch sets the word
// to all ones on the same stream beforehand; nothing else is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_tablecheck.h"

namespace dspi {

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct TableCheckArgs {
    TableCheck c;
    const uint64_t *table;       // [c.entries], 16-byte aligned
    const uint8_t *kinds;        // [c.entries / c.per_stream]
    const uint32_t *active;      // one bit per stream, or null: every stream
    uint64_t *answer;
};

// the kernel's memory behind tablecheck_lane
struct TableCheckLoads {
    const TableCheckArgs &a;
    __device__ void pair(uint64_t first, uint64_t v[2]) const {
        const u64x2 w = *reinterpret_cast<const u64x2 *>(a.table + first);
        v[0] = w.x; v[1] = w.y;
    }
    __device__ uint64_t one(uint64_t index) const { return a.table[index]; }
    __device__ uint8_t stream_kind(uint32_t s) const { return a.kinds[s]; }
    __device__ bool active(uint32_t s) const { return !a.active || (a.active[s >> 5] >> (s & 31u) & 1u); }
};

__global__ __launch_bounds__(kTableCheckThreads) void tablecheck_kernel(const TableCheckArgs a) {
    __shared__ uint64_t wave_min[kTableCheckWaves];
    TableCheckLoads m{a};
    uint64_t lowest = tablecheck_lane(a.c, gridDim.x, blockIdx.x, threadIdx.x, m);
    for (uint32_t off = kTableCheckFirstStep; off; off >>= 1) lowest = tablecheck_min(lowest, (uint64_t)__shfl_xor((unsigned long long)lowest, (int)off, (int)kTableCheckWave));
    if (threadIdx.x % kTableCheckWave == 0) wave_min[threadIdx.x / kTableCheckWave] = lowest;
    __syncthreads();
    if (threadIdx.x) return;
    for (uint32_t w = 1; w < kTableCheckWaves; w++) lowest = tablecheck_min(lowest, wave_min[w]);
    if (lowest != kTableCheckNone) __hip_atomic_fetch_min(a.answer, lowest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_tablecheck(const TableCheck &c, const uint64_t *table, const uint8_t *kinds, const uint32_t *active, uint64_t *answer, uint32_t max_workgroups, hipStream_t stream) {
    if (c.entries > kPacketMaxEntries || (c.entries && !c.per_stream) || (reinterpret_cast<uintptr_t>(table) & 15u) || (reinterpret_cast<uintptr_t>(answer) & 7u)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(answer, 0xff, 8, stream);
    if (e != hipSuccess || !c.entries) return e;
    TableCheckArgs a{c, table, kinds, active, answer};
    hipLaunchKernelGGL(tablecheck_kernel, dim3(tablecheck_workgroups(c.entries, max_workgroups ? max_workgroups : kTableCheckDefaultWgs)), dim3(kTableCheckThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi

// The launcher by itself on raw device pointers, on the null stream, waited for, the answer brought to *answer (host memory): NOT part of
// include/dspi.h and no interface.  It exists for tests/test_gpu_packets_resident.py, which drives loop iterations and tails at small sizes
// through max_workgroups.  scratch: 8 bytes of device memory, 8-byte aligned.  It reads nothing but the table, the kinds and the bitmap.
extern "C" int dspi_tablecheck_launch_raw(uint32_t kind, const uint64_t *table, const uint8_t *kinds, const uint32_t *active, uint64_t entries, uint32_t per_stream, uint32_t block_len,
                                          uint64_t arena_bytes, uint32_t max_workgroups, uint64_t *scratch, uint64_t *answer) {
    if (!table || !kinds || !scratch || !answer || kind > dspi::kTableEmit) return (int)hipErrorInvalidValue;
    const dspi::TableCheck c{entries, arena_bytes, per_stream, block_len, kind};
    hipError_t e = dspi::launch_tablecheck(c, table, kinds, active, scratch, max_workgroups, nullptr);
    if (e == hipSuccess) e = hipMemcpy(answer, scratch, 8, hipMemcpyDeviceToHost);
    return (int)e;
}
