// realign_driver.cpp — the realignment rule and index arithmetic of dspi_amd/csrc/dspi_snapshot.h on the CPU, for tests/test_realign_cpu.py.
//   realign_driver target ROW_STREAMS N_STREAMS FIRST COUNT    per touched row: "row <row> stream <target stream> resident <0|1>"
//   realign_driver rotate LEN W_S W_T P...                     "shift <d>" (d = the rotation from W_S to W_T); per P: "src <P> <record position that lands on P>";
//                                                              "lands <position the record's W_S lands on>"; "bijection <0|1>" over all LEN positions
//   realign_driver sweep LEN                                   every d in [0, LEN) at p in {0, 1, LEN - 1}: "ok" or the first failure
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_snapshot.h"

using namespace dspi;

static uint32_t num(const char *s) { return (uint32_t)strtoul(s, nullptr, 0); }

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "target" && argc == 6) {
        const uint32_t R = num(argv[2]), n = num(argv[3]), first = num(argv[4]), count = num(argv[5]);
        for (uint32_t row = first / R; row <= (first + count - 1) / R; row++) {
            const SnapTarget t = snap_row_target(row, R, n, first, count);
            printf("row %u stream %u resident %d\n", row, t.stream, t.resident ? 1 : 0);
        }
        return 0;
    }
    if (cmd == "rotate" && argc >= 5) {
        const uint32_t len = num(argv[2]), w_s = num(argv[3]), w_t = num(argv[4]), d = snap_shift(w_s, w_t, len);
        printf("shift %u\n", d);
        for (int i = 5; i < argc; i++) printf("src %u %u\n", num(argv[i]), snap_rot_source(num(argv[i]), d, len));
        std::vector<int> hit(len, 0);
        uint32_t lands = len;
        for (uint32_t p = 0; p < len; p++) {
            const uint32_t q = snap_rot_source(p, d, len);
            if (q < len) hit[q]++;
            if (q == w_s) lands = p;
        }
        bool bij = true;
        for (uint32_t q = 0; q < len; q++) bij = bij && hit[q] == 1;
        printf("lands %u\nbijection %d\n", lands, bij ? 1 : 0);
        return 0;
    }
    if (cmd == "sweep" && argc == 3) {
        // for every rotation d: the map p -> source is a bijection of [0, len), consecutive array positions read consecutive record positions
        // (mod len), and with w_t = (w_s + d) mod len the record's write position w_s lands on w_t — checked through p in {0, 1, len - 1}
        const uint32_t len = num(argv[2]);
        std::vector<uint32_t> seen(len);
        for (uint32_t d = 0; d < len; d++) {
            for (uint32_t q = 0; q < len; q++) seen[q] = 0;
            for (uint32_t p = 0; p < len; p++) {
                const uint32_t q = snap_rot_source(p, d, len);
                if (q >= len || seen[q]++) { printf("d %u: not a bijection at p %u\n", d, p); return 0; }
            }
            const uint32_t ps[3] = {0u, 1u, len - 1u};
            for (uint32_t p : ps) {
                const uint32_t w_s = snap_rot_source(p, d, len);      // the record position that lands on p ...
                if (((w_s + d) & (len - 1u)) != p) { printf("d %u p %u: source %u + d is not p\n", d, p, w_s); return 0; }
                const uint32_t w_t = p;                                 // ... so a record written at w_s continues at w_t = p
                if (snap_shift(w_s, w_t, len) != d) { printf("d %u p %u: snap_shift(%u, %u) is not d\n", d, p, w_s, w_t); return 0; }
            }
        }
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: realign_driver target ROW_STREAMS N_STREAMS FIRST COUNT | rotate LEN W_S W_T P... | sweep LEN\n");
    return 2;
}
