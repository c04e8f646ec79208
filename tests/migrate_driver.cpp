// migrate_driver.cpp — migration between two contexts (dspi_amd/csrc/dspi_migrate.{h,cpp}) on the CPU, for tests/test_migrate_cpu.py.  Every
// mode reads its cases from standard input, one per line, and answers one line per case.  ACTIVE is a string of 0 / 1, one character per
// slot, or "-" (every slot active); a list is "src dst src dst ...".
//   migrate_driver validate            N_SRC N_DST DST_ACTIVE list   -> "ok" or the refusal
//   migrate_driver plan WANT           SRC_ACTIVE DST_ACTIVE         -> the list ("-" as SRC_ACTIVE / DST_ACTIVE: "-N", N active slots)
//   migrate_driver targets ROW         N_DST DST_ACTIVE list         -> "dst target from_entry ..." per entry
//   migrate_driver batches CAP         list                          -> "B g SLOT REC ... s SLOT REC ... B ..." (B begins a batch)
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_migrate.h"

using namespace dspi;

// "0110" -> bytes; "-N" -> empty (every one of N slots active), n = N
static std::vector<uint8_t> activity(const std::string &s, uint32_t &n) {
    std::vector<uint8_t> a;
    if (s[0] == '-') { n = (uint32_t)strtoul(s.c_str() + 1, nullptr, 0); return a; }
    for (char ch : s) a.push_back(ch == '1');
    n = (uint32_t)a.size();
    return a;
}
static std::vector<StreamMove> list_of(std::istringstream &in) {
    std::vector<StreamMove> m;
    uint32_t s, d;
    while (in >> s >> d) m.push_back(StreamMove{s, d});
    return m;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const uint32_t arg = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 0) : 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        if (cmd == "validate") {
            uint32_t n_src = 0, n_dst = 0, ignored = 0; std::string act;
            in >> n_src >> n_dst >> act;
            const std::vector<uint8_t> a = activity(act == "-" ? "-0" : act, ignored);
            const std::vector<StreamMove> m = list_of(in);
            const char *why = migrate_validate(m.empty() ? nullptr : m.data(), (uint32_t)m.size(), n_src, n_dst, a.empty() ? nullptr : a.data());
            out << (why ? why : "ok");
        } else if (cmd == "plan") {
            std::string sa, da;
            in >> sa >> da;
            uint32_t n_src = 0, n_dst = 0;
            const std::vector<uint8_t> s = activity(sa, n_src), d = activity(da, n_dst);
            for (const StreamMove &m : migrate_plan(s.empty() ? nullptr : s.data(), n_src, d.empty() ? nullptr : d.data(), n_dst, arg)) out << m.src << " " << m.dst << " ";
        } else if (cmd == "targets") {
            uint32_t n_dst = 0, ignored = 0; std::string act;
            in >> n_dst >> act;
            const std::vector<uint8_t> a = activity(act == "-" ? "-0" : act, ignored);
            const std::vector<StreamMove> m = list_of(in);
            for (const MigrateTarget &t : migrate_targets(m.data(), (uint32_t)m.size(), n_dst, arg, a.empty() ? nullptr : a.data())) out << t.dst << " " << t.target << " " << t.from_entry << " ";
        } else if (cmd == "batches") {
            const std::vector<StreamMove> m = list_of(in);
            for (const MoveBatch &b : migrate_batches(m.data(), (uint32_t)m.size(), arg)) {
                out << "B ";
                for (const MoveRecord &r : b.gather) out << "g " << r.slot << " " << r.record << " ";
                for (const MoveRecord &r : b.scatter) out << "s " << r.slot << " " << r.record << " ";
            }
        } else {
            fprintf(stderr, "usage: migrate_driver validate | plan WANT | targets ROW | batches CAP\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
