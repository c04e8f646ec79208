// group_driver.cpp — the grouping rule (dspi_amd/csrc/dspi_group.{h,cpp}) on the CPU, for tests/test_group_cpu.py.  Every mode reads its cases
// from standard input, one per line, and answers one line per case.  ACTIVE is a string of 0 / 1, one character per slot, or "-" (every slot
// active).
//   group_driver plan ONE_WAY      ACTIVE K class[0..K) object[0..n)   -> "src dst src dst ... | VERDICT": the list, and what move_validate says
//                                                                         of it on that population ("ok", also for an empty list).  K = 0: no
//                                                                         class table (one class, the Q28 flavour); n = the remaining numbers
//   group_driver classes           "flags delay0 kind0  flags delay0 kind0 ..." -> the class id of every ImageSig built from a triple
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_group.h"

using namespace dspi;

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const uint32_t arg = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 0) : 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        if (cmd == "plan") {
            std::string act; uint32_t k = 0;
            in >> act >> k;
            std::vector<uint8_t> a;
            if (act != "-") for (char ch : act) a.push_back(ch == '1');
            std::vector<uint32_t> cls(k);
            for (uint32_t &c : cls) in >> c;
            std::vector<int32_t> obj;
            int32_t o;
            while (in >> o) obj.push_back(o);
            const uint32_t n = (uint32_t)obj.size();
            if (!a.empty() && a.size() != n) { fprintf(stderr, "group_driver: %zu activity flags for %u slots\n", a.size(), n); return 2; }
            const std::vector<StreamMove> m = group_plan(a.empty() ? nullptr : a.data(), obj.data(), k ? cls.data() : nullptr, n, arg != 0);
            for (const StreamMove &e : m) out << e.src << " " << e.dst << " ";
            const char *why = m.empty() ? nullptr : move_validate(m.data(), (uint32_t)m.size(), n, a.empty() ? nullptr : a.data());
            out << "| " << (why ? why : "ok");
        } else if (cmd == "classes") {
            std::vector<ImageSig> sig;
            uint32_t flags; int32_t delay; uint32_t kind;
            while (in >> flags >> delay >> kind) {
                ImageSig g;
                memset(&g, 0, sizeof g);
                g.flags = flags; g.delay[0] = delay; g.kinds[0] = (uint8_t)kind;
                sig.push_back(g);
            }
            for (uint32_t c : group_classes(sig.data(), sig.size())) out << c << " ";
        } else {
            fprintf(stderr, "usage: group_driver plan ONE_WAY | classes\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
