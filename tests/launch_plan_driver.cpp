// Driver of tests/test_launch_plan_cpu.py: runs plan_launches and plan_call (dspi_amd/csrc/dspi_plan.cpp) on records read from stdin
// and prints the plans and layouts.  Built with g++ alone: the planner needs no HIP.
//
// in, per scenario:  flavor n_streams n_images cus layout(0 auto, 1 skew, 2 packed) paired(0/1)
//                    n_streams image indices
//                    per image: flags out_enabled out_mute ch_bypassed variant band filters
//   ImageSig = {flags, ch_bypassed, out_enabled, out_mute, fs_hz = variant}; BandHash from `band`; two images have the same filter
//   words when their `filters` agree.
// out, per scenario: R <row_pv of every row>, then per non-empty path P <path> <items> and one line per item: wg image mask mask1
//
// in, per call:  C n_streams n_wg row n_ch n_out n_pairs n_blocks block_len bit_depth flags pairs sub peaks clip no_direct all_latency
// out, per call: L frames mem(0 device, 1 direct, 2 staged) spdif_two_pass two_pass_rows two_pass_bytes direct_bytes n_chunks
//                rows_per_chunk, then per buffer (pcm pairs sub peaks clip): bytes per tile_cols off
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../dspi_amd/csrc/dspi_plan.h"

using namespace dspi;

static bool call_record() {
    CallInput in;
    unsigned pairs, sub, peaks, clip, no_direct, all_latency;
    if (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", &in.n_streams, &in.n_wg, &in.row, &in.n_ch, &in.n_out, &in.n_pairs, &in.n_blocks,
              &in.block_len, &in.bit_depth, &in.flags, &pairs, &sub, &peaks, &clip, &no_direct, &all_latency) != 16)
        return false;
    in.pairs = pairs; in.sub = sub; in.peaks = peaks; in.clip = clip; in.no_direct = no_direct; in.all_latency = all_latency;
    const CallLayout L = plan_call(in);
    printf("L %zu %d %d %u %zu %zu %u %u", L.frames, (int)L.mem, (int)L.spdif_two_pass, L.two_pass_rows, L.two_pass_bytes, L.direct_bytes, L.n_chunks,
           L.rows_per_chunk);
    for (const CallBuffer *b : {&L.pcm, &L.pairs, &L.sub, &L.peaks, &L.clip}) printf(" %zu %zu %d %zu", b->bytes, b->per, (int)b->tile_cols, b->off);
    printf("\n");
    return true;
}

int main() {
    char tok[16];
    while (scanf("%15s", tok) == 1) {
        if (!strcmp(tok, "C")) { if (!call_record()) return 1; continue; }
        const int flavor = atoi(tok);
        int layout, paired;
        unsigned n_streams, n_images, cus;
        if (scanf("%u %u %u %d %d", &n_streams, &n_images, &cus, &layout, &paired) != 5) return 1;
        PlanInput in;
        in.flavor = flavor; in.n_streams = n_streams; in.row = flavor ? 128u : 64u;
        in.cus = cus; in.layout = (F32Layout)layout; in.paired = paired != 0;
        in.stream_image.resize(n_streams);
        in.refs.assign(n_images, 0u);
        for (unsigned s = 0; s < n_streams; s++) { if (scanf("%d", &in.stream_image[s]) != 1) return 1; in.refs[(size_t)in.stream_image[s]]++; }
        std::vector<unsigned> filters(n_images);
        for (unsigned i = 0; i < n_images; i++) {
            ImageSig g;
            memset(&g, 0, sizeof g);
            unsigned long long band;
            if (scanf("%u %u %u %u %u %llu %u", &g.flags, &g.out_enabled, &g.out_mute, &g.ch_bypassed, &g.fs_hz, &band, &filters[i]) != 7) return 1;
            in.sig.push_back(g);
            in.bands.push_back(BandHash{band, band * 0x9e3779b97f4a7c15ull + 1});
        }
        in.same_filters = [&](uint32_t a, uint32_t b) { return filters[a] == filters[b]; };
        const LaunchPlan plan = plan_launches(in);
        printf("R");
        for (uint8_t v : plan.row_pv) printf(" %u", v);
        printf("\n");
        for (int p = 0; p < kNumPaths; p++) {
            if (plan.items[p].empty()) continue;
            printf("P %d %zu\n", p, plan.items[p].size());
            for (const WgItem &it : plan.items[p]) printf("%u %u %llu %llu\n", it.wg, it.image, (unsigned long long)it.mask, (unsigned long long)it.mask1);
        }
        printf("E\n");
    }
    return 0;
}
