// patch_driver.cpp — the plan of dspi_amd/csrc/dspi_patch.cpp without a GPU and outside Python: tests/test_patch_cpu.py builds this with its own
// main (under AddressSanitizer and UBSan where the compiler has them), feeds it cases on stdin and compares what it prints with
// tests/patch_model.py.  A case:
//   case N V F
//   V lines    wire n_streams n_pairs tile_streams n_frames          (wire: an address as a number; nothing is dereferenced)
//   N lines    source active view line kind
// The answer: the refusals 4 to 8 as texts ("ok": none), then the plan's flags and, section by section, the device table.  The views and the
// patches are copied into exactly sized heap arrays, so a read behind them is the sanitizer's to find.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dspi_amd/csrc/dspi_patch.h"

using namespace dspi;

static void why(const char *name, const char *text, uint32_t at) { printf("%s %" PRIu32 " %s\n", name, at, text ? text : "ok"); }

int main() {
    uint32_t n, V;
    uint64_t F;
    while (scanf(" case %" SCNu32 " %" SCNu32 " %" SCNu64, &n, &V, &F) == 3) {
        std::vector<WireView> views(V);
        for (WireView &v : views) {
            uint64_t wire;
            if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &wire, &v.n_streams, &v.n_pairs, &v.tile_streams, &v.n_frames) != 5) return 2;
            v.wire = reinterpret_cast<const uint32_t *>(static_cast<uintptr_t>(wire));
            v.producer = nullptr;
        }
        std::vector<uint8_t> sources(n), active(n);
        std::vector<Patch> patches(n);
        bool all_active = true;
        for (uint32_t s = 0; s < n; s++) {
            uint32_t src, act;
            if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &src, &act, &patches[s].view, &patches[s].line, &patches[s].kind) != 5) return 2;
            sources[s] = (uint8_t)src; active[s] = (uint8_t)act;
            all_active = all_active && act;
        }
        const uint8_t *const act = all_active ? nullptr : active.data();      // (as the library passes it: null when nobody is paused)
        uint32_t at = 0;
        const char *bad = patch_sources_why(sources.data(), n, &at);
        why("sources", bad, at);
        if (bad) { printf("end\n"); continue; }
        const bool any_link = patch_any(sources.data(), n, act, kSrcLink);
        at = 0;
        bad = any_link ? patch_views_why(sources.data(), n, act, V ? views.data() : nullptr, V, patches.data(), F, &at) : nullptr;
        why("views", bad, at);
        uint64_t total = 0;
        std::vector<uint64_t> off(n + 1);
        const bool fits = patch_offsets(sources.data(), n, F, &total, off.data());
        printf("bytes %s %" PRIu64 "\n", fits ? "ok" : "overflow", total);
        printf("needs %d %d\n", (int)patch_needs_in(sources.data(), n, act), bad ? 0 : (int)patch_needs_rx(sources.data(), n, act, patches.data()));
        if (bad || !fits) { printf("end\n"); continue; }
        PatchPlan p;
        patch_plan(sources.data(), n, act, views.data(), V, patches.data(), F, p);
        const uint64_t *const t = p.table.data();
        printf("flags %d %d %d %d\n", (int)p.any_pcm, (int)p.any_spdif_in, (int)p.any_tiled, (int)p.tiled_spdif);
        printf("in_offsets");
        for (uint32_t s = 0; s <= n; s++) printf(" %" PRIu64, t[p.in_offsets + s]);
        printf("\nin_kinds");
        for (uint32_t s = 0; s < n; s++) printf(" %u", reinterpret_cast<const uint8_t *>(t + p.in_kinds)[s]);
        printf("\npcm_mask");
        for (uint32_t s = 0; s < n; s++) printf(" %u", reinterpret_cast<const uint32_t *>(t + p.pcm_mask)[s >> 5] >> (s & 31u) & 1u);
        printf("\n");
        for (uint32_t v = 0; v < V; v++) {
            const PatchPlan::View &pv = p.view[v];
            printf("view %" PRIu32 " %d %d %d\n", v, (int)pv.used, (int)pv.any_spdif, (int)pv.any_i2s);
            if (!pv.used || views[v].tile_streams) continue;
            printf("offsets");
            for (uint32_t s = 0; s <= n; s++) printf(" %" PRIu64, t[pv.offsets + s]);
            printf("\nlinks");
            for (uint32_t s = 0; s < n; s++) {
                Link l;
                memcpy(&l, t + pv.links + s, sizeof l);
                printf(" %" PRIu32 ":%" PRIu32, l.line, l.kind);
            }
            printf("\nkinds");
            for (uint32_t s = 0; s < n; s++) printf(" %u", reinterpret_cast<const uint8_t *>(t + pv.kinds)[s]);
            printf("\n");
        }
        if (p.any_tiled) {
            printf("cols %d", (int)(p.cols % 2 == 0));
            for (uint32_t s = 0; s < n; s++) {
                PatchCol c;
                memcpy(&c, t + p.cols + 2 * (size_t)s, sizeof c);
                printf(" %" PRIu64 ":%" PRIu32 ":%" PRIu32, c.col, c.row, c.kind);
            }
            printf("\n");
        }
        printf("end\n");
    }
    return 0;
}
