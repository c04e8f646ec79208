// wire_tiled_driver.cpp — drives the tiled wire layout of dspi_amd/csrc/dspi_wire.h (dspi_process_devices / dspi_wire_encode_tiled) from
// tests/test_wire_tiled_cpu.py.  One command per input line, one answer per line; offsets are in WORDS from the start of the buffer:
//   flags devices|encode WORD       -> 1 when the call accepts these flags, else 0
//   spdif T P NP F R C FR J         -> the word of subframe word J of frame FR, column C, pair P of tile T (NP pairs, F frames, R columns)
//   i2s T P NP F R C SIDE FR        -> the word of the slot word (SIDE, FR) of the same column
//   column S P NP F R I2S           -> first written tail_first tail of stream S's column of pair P: its words stand at first + k * R,
//                                      k < written, its tail at tail_first + k * R, k < tail
//   region T P NP F R               -> the region's first word and its length in words
#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../dspi_amd/csrc/dspi_wire.h"

using namespace dspi;
typedef unsigned long long ull;

// the rules stand beside the ones they extend, which keep their values
static_assert(kWireProcessFlags == (DSPI_MEM_DEVICE | DSPI_OUT_ENABLED_ONLY | DSPI_OUT_CLIP_FLAGS) && kWireEncodeFlags == DSPI_MEM_DEVICE, "the stream-major calls' rules");
static_assert(kDevicesProcessFlags == (kWireProcessFlags | DSPI_OUT_TILED) && kWireEncodeTiledFlags == kWireEncodeFlags, "the new calls' rules");
// constexpr and free of HIP: usable at compile time
static_assert(wire_tiled_region(1, 1, 4, 48, 128) == 5ull * 48 * 4 * 128 && wire_tiled_column(129, 0, 4, 48, 128, true).tail == 96, "constexpr arithmetic");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "flags") {
            std::string which; unsigned long word; in >> which >> word;
            printf("%d\n", (which == "devices" ? devices_process_flags_ok((uint32_t)word) : wire_encode_tiled_flags_ok((uint32_t)word)) ? 1 : 0);
        } else if (cmd == "spdif") {
            ull t, p, np, f, r, c, fr, j; in >> t >> p >> np >> f >> r >> c >> fr >> j;
            printf("%llu\n", (ull)wire_tiled_spdif_word(wire_tiled_region(t, p, np, f, r), r, c, fr, j));
        } else if (cmd == "i2s") {
            ull t, p, np, f, r, c, side, fr; in >> t >> p >> np >> f >> r >> c >> side >> fr;
            printf("%llu\n", (ull)wire_tiled_i2s_word(wire_tiled_region(t, p, np, f, r), f, r, c, side, fr));
        } else if (cmd == "column") {
            ull s, p, np, f, r; int i2s; in >> s >> p >> np >> f >> r >> i2s;
            const WireTiledColumn w = wire_tiled_column(s, p, np, f, r, i2s != 0);
            printf("%llu %llu %llu %llu\n", (ull)w.first, (ull)w.written, (ull)w.tail_first, (ull)w.tail);
        } else if (cmd == "region") {
            ull t, p, np, f, r; in >> t >> p >> np >> f >> r;
            printf("%llu %llu\n", (ull)wire_tiled_region(t, p, np, f, r), (ull)wire_tiled_region_words(f, r));
        } else printf("unknown command\n");
    }
    return 0;
}
