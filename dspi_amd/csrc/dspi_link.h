// dspi_link.h — chained devices (include/dspi.h: dspi_wire_decode, dspi_process_linked): a VIEW of a buffer some call wrote in the wire layout
// or the tiled wire layout (dspi_wire.h), LINKS that name one line of it each, where the words of a link lie in the four cases (two layouts,
// two word formats), what the calls refuse about a view and its links, and the reader for one link on the CPU.  Plain C++ (no HIP):
// dspi_capi.cpp includes it, tests/linkrx_driver.cpp exercises it without a GPU.  The kernels are dspi_linkrx.hip (a tiled view, and the I2S
// lines of a stream-major one) and dspi_spdifrx.hip as it is (the S/PDIF lines of a stream-major view); they call the index functions below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dspi_spdifrx.h"

namespace dspi {

constexpr uint32_t kLinkNone = 0, kLinkSpdif = 1, kLinkI2s = 2;      // DSPI_LINK_*; kLinkSpdif == kSrcSpdif: a link's kind is launch_spdifrx's source byte
static_assert(kLinkSpdif == kSrcSpdif, "an S/PDIF link is an S/PDIF source");

// dspi_wire_view of include/dspi.h, member for member (dspi_capi.cpp asserts the two agree); `producer` is the C-ABI's business
struct WireView {
    const uint32_t *wire;
    uint32_t n_streams, n_pairs, tile_streams, n_frames;
    void *producer;
};
struct Link { uint32_t line, kind; };      // dspi_link: line = producer stream * n_pairs + pair
static_assert(sizeof(Link) == 8, "a link is two words");

// ---- where the words of a link lie (constexpr: the kernels call the same functions).  L = the line, P = n_pairs, F = n_frames, R = tile_streams;
// s = L / P, p = L % P.  Word offsets from view.wire; a region is 4 F words (stream-major) or 4 F rows of R words (tiled). ----
constexpr uint64_t link_region(uint64_t L, uint64_t F) { return L * F * 4u; }
constexpr uint64_t link_spdif_word(uint64_t f, uint32_t j) { return f * 4u + j; }                      // frame f, word j of {l, h, l, h}
constexpr uint64_t link_i2s_word(uint64_t f, uint32_t side) { return f * 2u + side; }                   // the region's first half
constexpr uint64_t link_region_tiled(uint64_t L, uint32_t P, uint32_t R, uint64_t F) { return ((L / P / R * P + L % P) * F) * 4u * R; }
constexpr uint32_t link_column(uint64_t L, uint32_t P, uint32_t R) { return (uint32_t)(L / P % R); }
constexpr uint64_t link_spdif_word_tiled(uint64_t f, uint32_t j, uint32_t R, uint32_t c) { return (f * 4u + j) * R + c; }
constexpr uint64_t link_i2s_word_tiled(uint64_t f, uint32_t side, uint64_t F, uint32_t R, uint32_t c) { return (side * F + f) * R + c; }
constexpr int32_t link_i2s_sample(uint32_t word) { return (int32_t)word >> 8; }                         // the low byte is ignored

// ---- what the calls refuse, one function per refusal (a text, or nullptr) ----
// the view: `frames` is the F the call carries (0: any non-zero n_frames); device: view.wire is device memory and 16-byte aligned
const char *link_view_why(const WireView &v, uint64_t frames, bool device);
uint64_t link_view_lines(const WireView &v);                      // n_streams * n_pairs
bool link_view_words(const WireView &v, uint64_t *words);       // the buffer's size in words; false when the size in bytes does not fit in 64 bits
// the links: entry i is looked at when active == nullptr or active[i] != 0.  none_ok: kLinkNone is a hole (dspi_wire_decode), else every entry
// looked at is S/PDIF or I2S.  Returns n when all hold, else the index of the first that does not.
uint32_t links_check(const Link *links, uint32_t n, uint64_t lines, const uint8_t *active, bool none_ok);
bool links_any(const Link *links, uint32_t n, const uint8_t *active, uint32_t kind);

// ---- the reader for one link on host memory ----
// F = view.n_frames frames of link `lk` (valid by the rules above; kLinkNone: nothing is read or written).  An I2S link: word >> 8, no record
// is read or written.  An S/PDIF link: the receiver of dspi_spdifrx.h through *rx (rx->sync <= 192).  Output, either or both: pairs = int32 [F][2];
// packed = 6 bytes per frame, 24-bit little endian (what the chain reads at bit depth 24).
void link_decode_cpu(const WireView &view, const Link &lk, SpdifRx *rx, int32_t *pairs, uint8_t *packed);

}  // namespace dspi
