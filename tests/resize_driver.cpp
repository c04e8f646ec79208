// resize_driver.cpp — resizing (dspi_amd/csrc/dspi_resize.{h,cpp}) on the CPU, for tests/test_resize_cpu.py.  Every mode reads its cases
// from standard input, one per line, and answers one line per case.  ACTIVE is a string of 0 / 1, one character per slot below N_OLD, or
// "-" (every slot active).
//   resize_driver validate          N_OLD N_NEW FLAGS ACTIVE     -> "ok" or the refusal
//   resize_driver reserve           N N_RESERVE                  -> "ok" or the refusal
//   resize_driver rows ROW          N_OLD N_NEW CAPACITY_ROWS    -> "BEFORE AFTER CAPACITY COPY REALLOCATE"
//   resize_driver reserve_rows ROW  N N_RESERVE CAPACITY_ROWS    -> the same
//   resize_driver bytes             ROWS ROW_BYTES               -> the product, or "overflow"
//   resize_driver items ROW         N_OLD N_NEW ACTIVE           -> "S first count" (the new slots), then per row item
//                                                                   "I ROW Q_ANY Q_ALL TARGET col col ..." (TARGET: -1 = kBootNone)
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_resize.h"

using namespace dspi;

static std::vector<uint8_t> activity(const std::string &act) {
    std::vector<uint8_t> a;
    if (act != "-") for (char ch : act) a.push_back(ch == '1');
    return a;
}

static void put_rows(std::ostringstream &out, const ResizeRows &r) {
    out << r.before << " " << r.after << " " << r.capacity << " " << r.copy << " " << (r.reallocate ? 1 : 0);
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const uint32_t arg = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 0) : 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        if (cmd == "validate") {
            uint32_t n_old = 0, n_new = 0; std::string flags, act;
            in >> n_old >> n_new >> flags >> act;
            const std::vector<uint8_t> a = activity(act);
            const char *why = resize_validate(n_old, n_new, (uint32_t)strtoul(flags.c_str(), nullptr, 0), a.empty() ? nullptr : a.data());
            out << (why ? why : "ok");
        } else if (cmd == "reserve") {
            uint32_t n = 0, want = 0;
            in >> n >> want;
            const char *why = reserve_validate(n, want);
            out << (why ? why : "ok");
        } else if ((cmd == "rows" || cmd == "reserve_rows") && arg) {
            uint32_t n_old = 0, n_new = 0, cap = 0;
            in >> n_old >> n_new >> cap;
            put_rows(out, cmd == "rows" ? resize_rows(n_old, n_new, cap, arg) : reserve_rows(n_old, n_new, cap, arg));
        } else if (cmd == "bytes") {
            uint32_t rows = 0; unsigned long long row_bytes = 0;
            in >> rows >> row_bytes;
            size_t b = 0;
            if (resize_bytes(rows, (size_t)row_bytes, &b)) out << b; else out << "overflow";
        } else if (cmd == "items" && arg) {
            uint32_t n_old = 0, n_new = 0; std::string act;
            in >> n_old >> n_new >> act;
            const std::vector<uint8_t> a = activity(act);
            const std::vector<uint32_t> l = resize_new_slots(n_old, n_new);
            out << "S " << (l.empty() ? 0u : l.front()) << " " << l.size() << " ";
            for (size_t i = 1; i < l.size(); i++) if (l[i] != l[i - 1] + 1) out << "unordered ";
            for (const BootRowItem &it : resize_row_items(n_old, n_new, arg, a.empty() ? nullptr : a.data())) {
                out << "I " << it.row << " " << it.q_any << " " << it.q_all << " " << (it.target == kBootNone ? -1 : (int64_t)it.target) << " ";
                for (uint32_t c = 0; c < arg; c++) if ((it.cols[c / 32] >> (c % 32)) & 1u) out << c << " ";
            }
        } else {
            fprintf(stderr, "usage: resize_driver validate | reserve | rows ROW | reserve_rows ROW | bytes | items ROW\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
