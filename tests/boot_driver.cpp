// boot_driver.cpp — stream boots (dspi_amd/csrc/dspi_boot.{h,cpp}) on the CPU, for tests/test_boot_cpu.py.  Every mode reads its cases from
// standard input, one per line, and answers one line per case.  ACTIVE is a string of 0 / 1, one character per slot, or "-" (every slot
// active); a list is "stream stream ...", "null" the null pointer.
//   boot_driver validate            N list                  -> "ok" or the refusal
//   boot_driver items ROW           N ACTIVE AS_IS list     -> per row item "I ROW Q_ANY Q_ALL TARGET col col ..." (TARGET: -1 = kBootNone)
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_boot.h"

using namespace dspi;

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const uint32_t arg = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 0) : 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        uint32_t n = 0;
        in >> n;
        if (cmd == "validate") {
            std::vector<uint32_t> l;
            std::string tok;
            bool null = false;
            while (in >> tok) { if (tok == "null") null = true; else l.push_back((uint32_t)strtoul(tok.c_str(), nullptr, 0)); }
            // (a null list with a count of 3, an empty list with a valid pointer)
            static const uint32_t none = 0;
            const char *why = null ? boot_validate(nullptr, 3, n) : boot_validate(l.empty() ? &none : l.data(), (uint32_t)l.size(), n);
            out << (why ? why : "ok");
        } else if (cmd == "items" && arg) {
            std::string act; int as_is = 0;
            in >> act >> as_is;
            std::vector<uint8_t> a;
            if (act != "-") for (char ch : act) a.push_back(ch == '1');
            std::vector<uint32_t> l;
            uint32_t s;
            while (in >> s) l.push_back(s);
            for (const BootRowItem &it : boot_row_items(l.data(), (uint32_t)l.size(), n, arg, a.empty() ? nullptr : a.data(), as_is != 0)) {
                out << "I " << it.row << " " << it.q_any << " " << it.q_all << " " << (it.target == kBootNone ? -1 : (int64_t)it.target) << " ";
                for (uint32_t c = 0; c < arg; c++) if ((it.cols[c / 32] >> (c % 32)) & 1u) out << c << " ";
            }
        } else {
            fprintf(stderr, "usage: boot_driver validate | items ROW\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
