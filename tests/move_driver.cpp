// move_driver.cpp — stream moves (dspi_amd/csrc/dspi_move.{h,cpp}) on the CPU, for tests/test_move_cpu.py.  Every mode reads its cases from
// standard input, one per line, and answers one line per case.  ACTIVE is a string of 0 / 1, one character per slot, or "-" (every slot
// active); a list is "src dst src dst ...".
//   move_driver schedule CAP               list                -> "B g SLOT REC ... s SLOT REC ... B ..." (B begins a batch)
//   move_driver validate                   N ACTIVE list       -> "ok" or the refusal
//   move_driver compact ONE_WAY            ACTIVE              -> the compaction list
//   move_driver targets ROW                N ACTIVE list       -> "src dst target ..." per applied entry
//   move_driver list_targets ROW           N ACTIVE LISTED list -> "src dst target from_entry ..." per entry, list_targets as it is (LISTED like ACTIVE, "-": null)
//   move_driver items ROW                  "slot rec ..."      -> per row item "I ROW Q_ANY Q_ALL colrec..." (colrec: -1 = not listed)
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_move.h"

using namespace dspi;

static std::vector<uint8_t> activity(const std::string &s) {
    std::vector<uint8_t> a;
    if (s != "-") for (char ch : s) a.push_back(ch == '1');
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
        if (cmd == "schedule") {
            const std::vector<StreamMove> m = list_of(in);
            for (const MoveBatch &b : move_schedule(m.data(), (uint32_t)m.size(), arg)) {
                out << "B ";
                for (const MoveRecord &r : b.gather) out << "g " << r.slot << " " << r.record << " ";
                for (const MoveRecord &r : b.scatter) out << "s " << r.slot << " " << r.record << " ";
            }
        } else if (cmd == "validate" || cmd == "targets") {
            uint32_t n = 0; std::string act;
            in >> n >> act;
            const std::vector<uint8_t> a = activity(act);
            const std::vector<StreamMove> m = list_of(in);
            if (cmd == "validate") {
                const char *why = move_validate(m.empty() ? nullptr : m.data(), (uint32_t)m.size(), n, a.empty() ? nullptr : a.data());
                out << (why ? why : "ok");
            } else
                for (const MoveTarget &t : move_targets(m.data(), (uint32_t)m.size(), n, arg, a.empty() ? nullptr : a.data())) out << t.src << " " << t.dst << " " << t.target << " ";
        } else if (cmd == "list_targets") {
            uint32_t n = 0; std::string act, lst;
            in >> n >> act >> lst;
            const std::vector<uint8_t> a = activity(act), l = activity(lst);
            const std::vector<StreamMove> m = list_of(in);
            for (const ListTarget &t : list_targets(m.data(), (uint32_t)m.size(), n, arg, a.empty() ? nullptr : a.data(), l.empty() ? nullptr : l.data()))
                out << t.src << " " << t.dst << " " << t.target << " " << t.from_entry << " ";
        } else if (cmd == "compact") {
            std::string act;
            in >> act;
            const std::vector<uint8_t> a = activity(act);
            for (const StreamMove &m : move_compaction(a.empty() ? nullptr : a.data(), (uint32_t)a.size(), arg != 0)) out << m.src << " " << m.dst << " ";
        } else if (cmd == "items") {
            std::vector<MoveRecord> l;
            uint32_t s, r;
            while (in >> s >> r) l.push_back(MoveRecord{s, r});
            std::vector<MoveRowItem> items; std::vector<uint32_t> colrec;
            move_row_items(l, arg, items, colrec);
            for (size_t i = 0; i < items.size(); i++) {
                out << "I " << items[i].row << " " << items[i].q_any << " " << items[i].q_all << " ";
                for (uint32_t c = 0; c < arg; c++) out << (int64_t)(colrec[i * arg + c] == kMoveNone ? -1 : (int64_t)colrec[i * arg + c]) << " ";
            }
        } else {
            fprintf(stderr, "usage: move_driver schedule CAP | validate | compact ONE_WAY | targets ROW | list_targets ROW | items ROW\n");
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
