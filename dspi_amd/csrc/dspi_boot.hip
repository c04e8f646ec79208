// dspi_boot.hip — power-on state for listed streams of a running context (dspi_boot_streams, include/dspi.h; the list: dspi_boot.h).
//
// The arrays are stacks of R-word rows, one row per position, column = stream ([W][position][R]: state slots, delay lines, leveller rings,
// PDM words), and the positions of one workgroup row lie one after the other.  Nothing is transposed and nothing is read: every listed
// column of every position gets a constant, so the kernel is the array side of the list-addressed scatter (dspi_snapshot.hip) without a
// record side.
//   work      blockIdx.x = a touched row (BootRowItem), blockIdx.y = one of kBootParts parts: each part takes a contiguous run of the
//             row's delay-line positions and one of its ring positions; part 0 also writes the state slots and the PDM words
//   lanes     R / 4 lanes cover one position, lane q its columns 4q .. 4q + 3; a workgroup covers 256 / (R / 4) consecutive positions per
//             pass, a wave 1 024 consecutive bytes
//   stores    16 bytes where all four columns of the group are listed — a fully listed row is written in whole 512- / 256-byte lines —,
//             single words for the listed columns of a partial group, none for a group without a listed column: no column that is not
//             listed is written
//   words     zero, except the state slots and PDM words that state_power_on_word (dspi_image.h) and pdm_power_on_word (dspi_kernels.h)
//             name, and the two write positions: the row's target's (one resident stream's delay write index and ring position, the only
//             words this kernel reads — the target is not listed, so no workgroup of the launch writes them), or (0, 0) for kBootNone
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_boot.h"
#include "dspi_kernels.h"
#include "dspi_snapshot.h"

namespace dspi {

static_assert(sizeof(BootRowItem) == 32, "the boot list's work items go up as 32-bit words");

namespace {

constexpr uint32_t kBootThreads = 256, kBootParts = 64;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct BootKArgs {
    uint32_t *state, *dlines, *ring, *pdm;      // pdm: null when the context has no modulator array
    const BootRowItem *items;
};

template <uint32_t ROW>
__global__ __launch_bounds__(kBootThreads) void boot_kernel(const BootKArgs a) {
    constexpr int kFlavor = ROW == 128 ? 1 : 0;
    constexpr StateMap sm = make_state_map(kFlavor);
    static_assert((uint32_t)sm.row == ROW && ROW % 4 == 0 && ROW <= 128 && kBootThreads % (ROW / 4) == 0, "row shape");
    constexpr uint32_t kGroups = ROW / 4, kPosPerPass = kBootThreads / kGroups;
    constexpr uint32_t kLines = (uint32_t)sm.n_out * (uint32_t)sm.max_delay, kRing = 2u * (uint32_t)kRingLen;
    const BootRowItem &it = a.items[blockIdx.x];
    const uint32_t q = threadIdx.x % kGroups, r = threadIdx.x / kGroups, part = blockIdx.y;
    if (!((it.q_any >> q) & 1u)) return;
    const bool all = (it.q_all >> q) & 1u;
    const uint32_t four = (it.cols[q / 8] >> (4 * (q % 8))) & 15u;      // which of the group's columns are listed (read per lane: no run-time index into a register copy of the item)
    const uint32_t row = it.row, target = it.target;
    // word w into the group's listed columns of the position whose row begins at `line`
    auto put = [&](uint32_t *line, uint32_t w) {
        uint32_t *g = line + 4 * q;
        if (all) *reinterpret_cast<u4 *>(g) = u4{w, w, w, w};
        else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) if ((four >> j) & 1u) g[j] = w;
        }
    };
    // this part's share of a section of `len` positions
    auto zero = [&](uint32_t *sec, uint32_t len) {
        const uint32_t chunk = (len + kBootParts - 1) / kBootParts, p0 = part * chunk, p1 = p0 + chunk < len ? p0 + chunk : len;
        for (uint32_t p = p0 + r; p < p1; p += kPosPerPass) put(sec + (size_t)p * ROW, 0u);
    };
    zero(a.dlines + (size_t)row * kLines * ROW, kLines);
    zero(a.ring + (size_t)row * kRing * ROW, kRing);
    if (part != 0) return;
    uint32_t widx = 0, ring_pos = 0;
    if (target != kBootNone) {
        const SnapPos t = snap_positions(sm, a.state, target);
        widx = t.widx; ring_pos = t.ring_pos;
    }
    uint32_t *const st = a.state + (size_t)row * sm.n_slots * ROW;
    for (uint32_t p = r; p < (uint32_t)sm.n_slots; p += kPosPerPass)
        put(st + (size_t)p * ROW, p == (uint32_t)sm.widx ? widx : p == (uint32_t)sm.ring_pos ? ring_pos : state_power_on_word(kFlavor, (int)p));
    if (a.pdm)
        for (uint32_t p = r; p < (uint32_t)kPdmStateWords; p += kPosPerPass) put(a.pdm + ((size_t)row * kPdmStateWords + p) * ROW, pdm_power_on_word((int)p));
}

}  // namespace

hipError_t launch_boot(int flavor, const StateArrays &arr, const uint32_t *items, uint32_t n_items, hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    const BootKArgs a{arr.state, arr.dlines, arr.ring, arr.pdm, reinterpret_cast<const BootRowItem *>(items)};
    const dim3 grid(n_items, kBootParts);
    for_row_width(flavor, [&](auto row) { hipLaunchKernelGGL((boot_kernel<decltype(row)::value>), grid, dim3(kBootThreads), 0, stream, a); });
    return hipGetLastError();
}

}  // namespace dspi
