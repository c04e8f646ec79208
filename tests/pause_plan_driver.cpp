// Driver of tests/test_pause_cpu.py: plan_launches (dspi_amd/csrc/dspi_plan.cpp) with an activity vector, and the activity-aware target
// rule of dspi_resume_streams (dspi_amd/csrc/dspi_snapshot.h).  Built with g++ alone.
//
//   pause_plan_driver                 scenarios on stdin, in the records of tests/launch_plan_driver.cpp, each followed by one activity record:
//                                       0                      PlanInput::active left empty (the field's default)
//                                       n_streams a_0 a_1 ...  one 0 / 1 per stream (0 = paused)
//                                     out: what launch_plan_driver prints for a scenario (R ..., P ..., items, E)
//   pause_plan_driver target ROW_STREAMS N_STREAMS FIRST COUNT BITS
//                                     BITS: N_STREAMS characters 0 / 1, the activity before the call.  Per touched row:
//                                     "row <row> stream <target> resident <0|1> plain <snap_row_target's stream> <its resident>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_plan.h"
#include "../dspi_amd/csrc/dspi_snapshot.h"

using namespace dspi;

static int target(int argc, char **argv) {
    if (argc != 7) return 2;
    const uint32_t R = (uint32_t)strtoul(argv[2], nullptr, 0), n = (uint32_t)strtoul(argv[3], nullptr, 0), first = (uint32_t)strtoul(argv[4], nullptr, 0),
                   count = (uint32_t)strtoul(argv[5], nullptr, 0);
    const std::string bits = argv[6];
    if (bits.size() != n || count == 0 || (uint64_t)first + count > n) return 2;
    std::vector<uint32_t> active((n + 31) / 32, 0u);
    for (uint32_t s = 0; s < n; s++) if (bits[s] == '1') active[s >> 5] |= 1u << (s & 31u);
    for (uint32_t row = first / R; row <= (first + count - 1) / R; row++) {
        const SnapTarget t = snap_row_target_active(row, R, n, first, count, active.data()), p = snap_row_target(row, R, n, first, count);
        printf("row %u stream %u resident %d plain %u %d\n", row, t.stream, t.resident ? 1 : 0, p.stream, p.resident ? 1 : 0);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return !strcmp(argv[1], "target") ? target(argc, argv) : 2;
    int flavor;
    while (scanf("%d", &flavor) == 1) {
        int layout, paired;
        unsigned n_streams, n_images, cus;
        if (scanf("%u %u %u %d %d", &n_streams, &n_images, &cus, &layout, &paired) != 5) return 1;
        PlanInput in;
        in.flavor = flavor; in.n_streams = n_streams; in.row = flavor ? 128u : 64u;
        in.cus = cus; in.layout = (F32Layout)layout; in.paired = paired != 0;
        in.stream_image.resize(n_streams);
        in.refs.assign(n_images, 0u);      // all streams, paused or not, as the context counts them
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
        unsigned n_active;
        if (scanf("%u", &n_active) != 1 || (n_active != 0 && n_active != n_streams)) return 1;
        in.active.resize(n_active);
        for (unsigned s = 0; s < n_active; s++) { unsigned a; if (scanf("%u", &a) != 1) return 1; in.active[s] = a ? 1 : 0; }
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
