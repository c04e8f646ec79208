// Driver of tests/test_launch_plan_cpu.py: runs plan_launches (dspi_amd/csrc/dspi_plan.cpp) on scenarios read from stdin and prints
// the plans.  Built with g++ alone: the planner needs no HIP.
//
// in, per scenario:  flavor n_streams n_images cus layout(0 auto, 1 skew, 2 packed) paired(0/1)
//                    n_streams image indices
//                    per image: flags out_enabled out_mute ch_bypassed variant band filters
//   ImageSig = {flags, ch_bypassed, out_enabled, out_mute, fs_hz = variant}; BandHash from `band`; two images have the same filter
//   words when their `filters` agree.
// out, per scenario: R <row_pv of every row>, then per non-empty path P <path> <items> and one line per item: wg image mask mask1
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dspi_amd/csrc/dspi_plan.h"

using namespace dspi;

int main() {
    int flavor, layout, paired;
    unsigned n_streams, n_images, cus;
    while (scanf("%d %u %u %u %d %d", &flavor, &n_streams, &n_images, &cus, &layout, &paired) == 6) {
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
