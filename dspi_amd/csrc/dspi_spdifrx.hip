// dspi_spdifrx.hip — the S/PDIF receiver on the device (dspi_spdifrx.h: the subframe, the record, the rule on the CPU): a line of subframes
// into pair words (dspi_spdif_decode) or into the packed 24-bit run the chain reads (dspi_process_sources, beside dspi_intake.hip, which
// keeps serving the PCM streams of such a call).
//   grid          one workgroup per line, blockIdx.x = line - first; a line that is no S/PDIF source, or paused, returns at once.
//   workgroup     one wave of 64 lanes over 64 consecutive frames, chunk after chunk: the record is carried in wave-uniform registers and
//                 written back once, by lane 0.  A lane takes one 16-byte load (a frame) and stores 8 bytes of pair words or 6 of packed PCM.
//   the samples   per side, good = well-formed and V clear, as a ballot.  A lane that conceals takes the sample of the nearest lower good
//                 lane (one shuffle), else the record's hold; the highest good lane leaves the new hold.
//   the sync      wave-uniform: rx_walk (dspi_spdifrx.h) goes over the chunk's ballots from event to event, not over its frames.
//   the counters  popcounts of the ballots; the parity count behind the chunk's last lock event, which is what resets it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_intake.h"
#include "dspi_kernels.h"
#include "dspi_spdifrx.h"

namespace dspi {

namespace {

constexpr uint32_t kRxLanes = 64;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct RxArgs {
    const uint8_t *src;          // line s at src + offsets[s], or (offsets == null) at src + 16 frames s
    const uint64_t *offsets;     // [n + 1] or null
    const uint8_t *sources;      // [n]: only lines whose entry is kSrcSpdif are served; null: every line
    const uint32_t *active;      // one bit per line, or null: every line
    uint32_t *rx;                // [n] records of kRxWords words
    void *dst;                   // kPacked: uint8 [n][6 frames]; else int32 [n][frames][2]
    uint64_t frames;
    uint32_t first;
};

constexpr uint64_t low_bits(uint32_t n) { return rx_low_bits(n); }
__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

template <bool kPacked>
__global__ __launch_bounds__(kRxLanes) void spdifrx_kernel(const RxArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t s = a.first + blockIdx.x;
    if (a.sources && a.sources[s] != kSrcSpdif) return;
    if (a.active && !(a.active[s >> 5] >> (s & 31u) & 1u)) return;
    const u4 *const in = reinterpret_cast<const u4 *>(a.src + (a.offsets ? a.offsets[s] : (uint64_t)s * kRxFrameBytes * a.frames));
    uint32_t *const rec = a.rx + (size_t)s * kRxWords;

    // the record, wave-uniform
    uint32_t rate = uni(rec[1]), parity = uni(rec[2]);
    uint64_t cbits = (uint64_t)uni(rec[4]) << 32 | uni(rec[3]);      // bits 0..39: the channel status; above: the record's padding, kept
    int32_t hold_l = (int32_t)uni(rec[5]), hold_r = (int32_t)uni(rec[6]);
    uint32_t sync = uni(rec[7]), held = uni(rec[8]), coding = uni(rec[9]);
    if (sync > kRxBlock) sync = 0;
    bool any_ok = false;

    for (uint64_t base = 0; base < a.frames; base += kRxLanes) {
        const uint32_t nv = a.frames - base < kRxLanes ? (uint32_t)(a.frames - base) : kRxLanes;
        const bool valid = lane < nv;
        u4 w = {0u, 0u, 0u, 0u};
        if (valid) w = in[base + lane];
        const uint32_t dl = rx_data(w.x, w.y), dr = rx_data(w.z, w.w);
        const bool ok_l = valid && rx_left_ok(w.x, w.y), ok_r = valid && rx_right_ok(w.z, w.w);
        const int32_t smp_l = rx_sample(dl), smp_r = rx_sample(dr);
        const uint64_t m_valid = low_bits(nv);
        const uint64_t m_bad_l = m_valid & ~__ballot(ok_l), m_bad_r = m_valid & ~__ballot(ok_r);
        const uint64_t m_z = __ballot(ok_l && (w.x & 0xffu) == kPreZ), m_c = __ballot(valid && rx_c(dl));
        const uint64_t m_par_l = __ballot(ok_l && rx_parity_fails(dl)), m_par_r = __ballot(ok_r && rx_parity_fails(dr));
        const uint64_t m_good_l = __ballot(ok_l && !rx_v(dl)), m_good_r = __ballot(ok_r && !rx_v(dr));
        any_ok = any_ok || (m_valid & ~(m_bad_l & m_bad_r)) != 0;

        // ---- the sync machine: from event to event (scalar; every value is the wave's) ----
        RxWalk walk{sync, rate, cbits, -1};
        rx_walk(walk, nv, m_bad_l, m_bad_r, m_z, m_c);
        sync = walk.sync; rate = walk.rate; cbits = walk.cbits;
        const int lock_lane = walk.lock_lane;

        // ---- the counters ----
        const uint64_t counted = lock_lane < 0 ? ~0ull : ~low_bits((uint32_t)lock_lane);
        parity = (lock_lane < 0 ? parity : 0u) + (uint32_t)__builtin_popcountll(m_par_l & counted) + (uint32_t)__builtin_popcountll(m_par_r & counted);
        coding += (uint32_t)__builtin_popcountll(m_bad_l) + (uint32_t)__builtin_popcountll(m_bad_r);
        held += (uint32_t)__builtin_popcountll(m_valid & ~m_good_l) + (uint32_t)__builtin_popcountll(m_valid & ~m_good_r);

        // ---- the samples: concealed lanes take the nearest lower good lane's, else the hold ----
        const uint64_t below = low_bits(lane);
        const uint64_t gl = m_good_l & below, gr = m_good_r & below;
        const int32_t near_l = __shfl(smp_l, gl ? 63 - __builtin_clzll(gl) : 0), near_r = __shfl(smp_r, gr ? 63 - __builtin_clzll(gr) : 0);
        const int32_t out_l = (m_good_l >> lane & 1u) ? smp_l : gl ? near_l : hold_l;
        const int32_t out_r = (m_good_r >> lane & 1u) ? smp_r : gr ? near_r : hold_r;
        const int32_t last_l = __shfl(smp_l, m_good_l ? 63 - __builtin_clzll(m_good_l) : 0), last_r = __shfl(smp_r, m_good_r ? 63 - __builtin_clzll(m_good_r) : 0);
        if (m_good_l) hold_l = last_l;
        if (m_good_r) hold_r = last_r;

        if (valid) {
            if (kPacked) {      // a run is only 2-byte aligned: three 2-byte words per frame
                uint16_t *const d = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(a.dst) + (uint64_t)s * kIntakeOutFrame * a.frames) + 3u * (base + lane);
                d[0] = (uint16_t)out_l;
                d[1] = (uint16_t)(((uint32_t)out_l >> 16 & 0xffu) | ((uint32_t)out_r & 0xffu) << 8);
                d[2] = (uint16_t)((uint32_t)out_r >> 8);
            } else {
                int2 *const d = reinterpret_cast<int2 *>(a.dst) + (uint64_t)s * a.frames + base + lane;
                *d = make_int2(out_l, out_r);
            }
        }
    }

    if (lane == 0) {
        rec[0] = sync ? 2u : any_ok ? 1u : 0u;
        rec[1] = rate; rec[2] = parity; rec[3] = (uint32_t)cbits; rec[4] = (uint32_t)(cbits >> 32);
        rec[5] = (uint32_t)hold_l; rec[6] = (uint32_t)hold_r; rec[7] = sync; rec[8] = held; rec[9] = coding;
    }
}

}  // namespace

hipError_t launch_spdifrx(bool packed, const void *src, const uint64_t *offsets, const uint8_t *sources, const uint32_t *active, void *rx, void *dst, uint64_t frames,
                          uint32_t first, uint32_t count, hipStream_t stream) {
    if (!count || !frames) return hipSuccess;
    if (count > 0x7fffffffu) return hipErrorInvalidValue;
    RxArgs a{static_cast<const uint8_t *>(src), offsets, sources, active, static_cast<uint32_t *>(rx), dst, frames, first};
    if (packed) hipLaunchKernelGGL(spdifrx_kernel<true>, dim3(count), dim3(kRxLanes), 0, stream, a);
    else hipLaunchKernelGGL(spdifrx_kernel<false>, dim3(count), dim3(kRxLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dspi
