// dspi_colwalk.h — the tiled link receiver's walk over ONE column (device code; included by dspi_linkrx.hip, whose tiled kernel gives every lane
// the column of its link in the one view of the call, and by dspi_patchrx.hip, whose lanes bring a column each of any view): a lane walks its
// column frame by frame.  An S/PDIF lane carries its record in registers, runs rx_frame (dspi_spdifrx.h, the sequential rule itself) per frame
// and writes the record back once; an I2S lane has none.  A lane keeps a GROUP of frames in flight: the 4 (S/PDIF) or 2 (I2S) row loads of the
// next kGroup frames are issued as one group before the walk over the group that has arrived.  Frames are not sliced over the grid: the
// receiver is sequential in F.  A packed run is only 2-byte aligned (6 F bytes per destination): three 2-byte stores per frame, as in
// dspi_spdifrx.hip.  No LDS, no scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dspi_intake.h"
#include "dspi_link.h"

namespace dspi {

namespace {

constexpr uint32_t kLinkLanes = 64;
constexpr uint32_t kGroup = 8;      // frames a lane requests at once: 32 (S/PDIF) or 16 (I2S) row loads in flight while it walks the group before

template <bool kPacked>
__device__ inline void put(void *dst, uint32_t i, uint32_t frames, uint64_t f, int32_t l, int32_t r) {
    if (kPacked) {
        uint16_t *const d = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(dst) + (uint64_t)i * kIntakeOutFrame * frames) + 3u * f;
        d[0] = (uint16_t)l;
        d[1] = (uint16_t)(((uint32_t)l >> 16 & 0xffu) | ((uint32_t)r & 0xffu) << 8);
        d[2] = (uint16_t)((uint32_t)r >> 8);
    } else {
        reinterpret_cast<int2 *>(dst)[(uint64_t)i * frames + f] = make_int2(l, r);
    }
}

// the row loads of the kGroup frames from `base` of a column, all of them inside the line (w: registers, every index a constant)
// Col: a pointer to the column's first word (const uint32_t *, or the same in the global address space)
template <class Col>
__device__ inline void load_spdif(uint32_t (&w)[kGroup][4], Col col, uint64_t base, uint32_t row) {
#pragma unroll
    for (uint32_t g = 0; g < kGroup; g++)
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) w[g][j] = col[link_spdif_word_tiled(base + g, j, row, 0u)];
}
template <class Col>
__device__ inline void load_i2s(uint32_t (&w)[kGroup][2], Col col, uint64_t base, uint32_t frames, uint32_t row) {
#pragma unroll
    for (uint32_t g = 0; g < kGroup; g++)
#pragma unroll
        for (uint32_t side = 0; side < 2; side++) w[g][side] = col[link_i2s_word_tiled(base + g, side, frames, row, 0u)];
}

// destination i takes the F frames of the column `col` (rows of R words) of kind kLinkSpdif — through the record rec, kRxWords words — or kLinkI2s
template <bool kPacked, class Col>
__device__ inline void walk_column(Col col, uint32_t kind, uint32_t R, uint32_t F, uint32_t *rec, void *dst, uint32_t i) {
    const uint64_t whole = F - F % kGroup;      // the frames of whole groups; the rest, fewer than kGroup, go one by one
    if (kind == kLinkSpdif) {
        RxRegs r{rec[7], rec[1], rec[2], rec[8], rec[9], (uint64_t)rec[4] << 32 | rec[3], (int32_t)rec[5], (int32_t)rec[6], false};
        if (r.sync > kRxBlock) r.sync = 0;
        uint32_t cur[kGroup][4], nxt[kGroup][4];
        if (whole) load_spdif(cur, col, 0u, R);
        for (uint64_t base = 0; base < whole; base += kGroup) {
            const bool more = base + kGroup < whole;
            if (more) load_spdif(nxt, col, base + kGroup, R);      // in flight during the walk
#pragma unroll
            for (uint32_t g = 0; g < kGroup; g++) {
                int32_t out_l = 0, out_r = 0;
                rx_frame(r, cur[g][0], cur[g][1], cur[g][2], cur[g][3], out_l, out_r);
                put<kPacked>(dst, i, F, base + g, out_l, out_r);
            }
            if (more) {
#pragma unroll
                for (uint32_t g = 0; g < kGroup; g++)
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) cur[g][j] = nxt[g][j];
            }
        }
        for (uint64_t f = whole; f < F; f++) {
            int32_t out_l = 0, out_r = 0;
            rx_frame(r, col[link_spdif_word_tiled(f, 0, R, 0u)], col[link_spdif_word_tiled(f, 1, R, 0u)], col[link_spdif_word_tiled(f, 2, R, 0u)], col[link_spdif_word_tiled(f, 3, R, 0u)], out_l, out_r);
            put<kPacked>(dst, i, F, f, out_l, out_r);
        }
        rec[0] = r.sync ? 2u : r.any_ok ? 1u : 0u;
        rec[1] = r.rate; rec[2] = r.parity; rec[3] = (uint32_t)r.cbits; rec[4] = (uint32_t)(r.cbits >> 32);
        rec[5] = (uint32_t)r.hold_l; rec[6] = (uint32_t)r.hold_r; rec[7] = r.sync; rec[8] = r.held; rec[9] = r.coding;
    } else {
        uint32_t cur[kGroup][2], nxt[kGroup][2];
        if (whole) load_i2s(cur, col, 0u, F, R);
        for (uint64_t base = 0; base < whole; base += kGroup) {
            const bool more = base + kGroup < whole;
            if (more) load_i2s(nxt, col, base + kGroup, F, R);
#pragma unroll
            for (uint32_t g = 0; g < kGroup; g++) put<kPacked>(dst, i, F, base + g, link_i2s_sample(cur[g][0]), link_i2s_sample(cur[g][1]));
            if (more) {
#pragma unroll
                for (uint32_t g = 0; g < kGroup; g++) { cur[g][0] = nxt[g][0]; cur[g][1] = nxt[g][1]; }
            }
        }
        for (uint64_t f = whole; f < F; f++)
            put<kPacked>(dst, i, F, f, link_i2s_sample(col[link_i2s_word_tiled(f, 0, F, R, 0u)]), link_i2s_sample(col[link_i2s_word_tiled(f, 1, F, R, 0u)]));
    }
}

}  // namespace

}  // namespace dspi
