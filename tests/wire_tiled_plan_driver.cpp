// wire_tiled_plan_driver.cpp — plan_call (dspi_amd/csrc/dspi_plan.cpp) with CallInput::wire_tiled, for tests/test_wire_tiled_cpu.py.  The
// records and answers are tests/wire_plan_driver.cpp's with one more field each:
// in, per call:  C n_streams n_wg row n_ch n_out n_pairs n_blocks block_len bit_depth flags pairs sub peaks clip no_direct all_latency wire_slots
//                wire_tiled
// out, per call: L frames mem spdif_two_pass two_pass_rows two_pass_bytes direct_bytes n_chunks rows_per_chunk, per buffer (pcm pairs sub peaks
//                clip): bytes per tile_cols off, then wire_encoder wire_tiled
#include <stdio.h>
#include <string.h>

#include "../dspi_amd/csrc/dspi_plan.h"

using namespace dspi;

int main() {
    char tok[16];
    while (scanf("%15s", tok) == 1) {
        if (strcmp(tok, "C")) return 1;
        CallInput in;
        unsigned pairs, sub, peaks, clip, no_direct, all_latency, wire_slots, wire_tiled;
        if (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", &in.n_streams, &in.n_wg, &in.row, &in.n_ch, &in.n_out, &in.n_pairs, &in.n_blocks, &in.block_len,
                  &in.bit_depth, &in.flags, &pairs, &sub, &peaks, &clip, &no_direct, &all_latency, &wire_slots, &wire_tiled) != 18)
            return 1;
        in.pairs = pairs; in.sub = sub; in.peaks = peaks; in.clip = clip; in.no_direct = no_direct; in.all_latency = all_latency; in.wire_slots = wire_slots;
        in.wire_tiled = wire_tiled;
        const CallLayout L = plan_call(in);
        printf("L %zu %d %d %u %zu %zu %u %u", L.frames, (int)L.mem, (int)L.spdif_two_pass, L.two_pass_rows, L.two_pass_bytes, L.direct_bytes, L.n_chunks, L.rows_per_chunk);
        for (const CallBuffer *b : {&L.pcm, &L.pairs, &L.sub, &L.peaks, &L.clip}) printf(" %zu %zu %d %zu", b->bytes, b->per, (int)b->tile_cols, b->off);
        printf(" %d %d\n", (int)L.wire_encoder, (int)L.wire_tiled);
    }
    return 0;
}
