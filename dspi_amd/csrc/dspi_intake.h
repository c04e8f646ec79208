// dspi_intake.h — the input layout of dspi_process_mixed (include/dspi.h): every stream's run of F frames at its own frame size, 4 bytes
// (16 bit) or 6 (24 bit), runs back to back.  Plain C++ (no HIP): dspi_capi.cpp includes it, tests/intake_driver.cpp exercises it without
// a GPU.  The kernel that turns such a buffer into the packed 24-bit array the chain reads is dspi_intake.hip; intake_widen_cpu below is the
// same rule for one stream on the CPU (the direct path's copy into the pinned area, and the model the kernel is held to).
//
// Why widening is all a mixed call needs (usb_audio.c): a 16-bit sample s and the 24-bit sample s << 8 go through the same arithmetic.
//   float  (:601-603 against :680-681)   the gains are 2^-23 p and 2^-15 p; (float)(s << 8) = 256 (float)s exactly, so both products are
//                                        roundings of the same real number — while both gains are exact, i.e. while 2^-23 p is a normal
//                                        binary32: p >= 2^-103.  A smaller positive preamp (update_preamp, :244-250, does not clamp) is the
//                                        one case the identity fails in: intake_preamp_breaks_widening, and the call refuses it.
//   Q28    (:1001-1002 against :1010-1011) the 24-bit route is (s24 << 8) >> 2; with s24 = s16 << 8 that is s16 << 14, the 16-bit route.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dspi {

// bytes per frame of a stream of this depth (two channels); 0: not a depth
constexpr uint32_t intake_frame_bytes(uint8_t depth) { return depth == 24 ? 6u : depth == 16 ? 4u : 0u; }
// bytes per frame of the array the chain reads
constexpr uint32_t kIntakeOutFrame = 6;

// every entry 16 or 24?  Returns n when so, else the index of the first entry that is neither.
uint32_t intake_check_depths(const uint8_t *depths, uint32_t n);
// what the depths have in common: 16 or 24 when every entry is that (n >= 1), else 0
uint8_t intake_uniform_depth(const uint8_t *depths, uint32_t n);
// offsets[0] = 0, offsets[s + 1] = offsets[s] + frames * frame bytes of s: n + 1 values (offsets == nullptr: none written); returns the total.
// The depths are valid (intake_check_depths).  False when n * frames * 6 does not fit in 64 bits; nothing is written then.
bool intake_offsets(const uint8_t *depths, uint32_t n, uint64_t frames, uint64_t *total, uint64_t *offsets);
// the bytes of the caller's buffer that hold the streams of rows [r0, r1) (`row` streams each, the last row ragged): [*begin, *end), from
// the n + 1 offsets.  Consecutive row ranges give consecutive byte ranges: the staged path uploads a chunk's rows as one piece.
void intake_row_range(const uint64_t *offsets, uint32_t n, uint32_t row, uint32_t r0, uint32_t r1, uint64_t *begin, uint64_t *end);
// the float preamp (its binary32 word) for which a 16-bit sample and its widened twin may differ: 0 < p < 2^-103
constexpr uint32_t kIntakePreampLimitWord = 24u << 23;      // 2^-103
constexpr bool intake_preamp_breaks_widening(uint32_t word) { return word != 0u && word < kIntakePreampLimitWord; }
// one stream's run of `frames` frames as packed 24 bit: a 16-bit word pair L, R becomes the six bytes 00 Llo Lhi 00 Rlo Rhi, a 24-bit run
// is copied.  src: frames * intake_frame_bytes(depth) bytes, dst: frames * 6; they do not overlap.
void intake_widen_cpu(uint8_t *dst, const uint8_t *src, uint8_t depth, uint64_t frames);

}  // namespace dspi
