// devmem_driver.cpp — the owner of the context's device memory (dspi_amd/csrc/dspi_devmem.{h,cpp}) on the CPU, for tests/test_devmem_cpu.py,
// against an allocator that really allocates (malloc: a sanitized build sees every leak, double free and overrun) and records its calls:
//   A<bytes>=<id> device allocation    X<bytes> refused allocation (it leaves garbage in *p)    F<id> device free    C<to>,<from>,<bytes> copy
//   HA / HX / HF: the same for pinned host memory    HD<id> the device's address of a pinned area
// Every mode reads its cases from standard input, one per line, and answers one line per case.
//   devmem_driver grow | keep      REQ REQ ...       one device buffer; REQ = BYTES or !BYTES (this request's allocation is refused)
//                                                    -> per request "[calls] present cap" (keep: + "kept" / "lost": the bytes written so far)
//   devmem_driver pinned           BYTES:GROW:DEV .. one pinned area (! as above)   -> per request "[calls] present cap dev"
//   devmem_driver release          SIZE SIZE ...     one registry; SIZE = 0 (never grown), BYTES (device) or pBYTES (pinned)
//                                                    -> "order ok|bad [calls of the release] [calls of a second release] live"
//   devmem_driver table FLAVOR     (one empty line)  -> per array "name=row_bytes/at_create"
//   devmem_driver fit              ROWS N_SLOTS N_OUT MAX_DELAY ROW   -> per array its bytes or "overflow", then "fit" / "refused"
//   devmem_driver realloc FLAVOR   ROWS0 ROWS1 REFUSE_AT PDM BASE COPY_OK   -> "[calls] same|moved x5 cap_rows rows_kept|rows_lost"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../dspi_amd/csrc/dspi_devmem.h"

using namespace dspi;

struct Fake {
    std::ostringstream log;
    std::map<void *, int> id;
    int next = 1, refuse_in = 0;      // refuse_in = n: the n-th allocation from now is refused
    bool refused() { return refuse_in && --refuse_in == 0; }
    bool alloc(const char *tag, void **p, size_t n) {
        if (refused()) { log << tag << "X" << n << " "; *p = reinterpret_cast<void *>(0x10); return false; }
        *p = malloc(n ? n : 1);
        id[*p] = next;
        log << tag << "A" << n << "=" << next++ << " ";
        return true;
    }
    bool release(const char *tag, void *p) {
        if (!id.count(p)) { log << tag << "F? "; return false; }
        log << tag << "F" << id[p] << " ";
        id.erase(p); free(p);
        return true;
    }
    bool dev_alloc(void **p, size_t n) { return alloc("", p, n); }
    bool dev_free(void *p) { return release("", p); }
    bool dev_copy(void *dst, const void *src, size_t n) {
        log << "C" << id[dst] << "," << id[const_cast<void *>(src)] << "," << n << " ";
        memcpy(dst, src, n);
        return true;
    }
    bool host_alloc(void **p, size_t n) { return alloc("H", p, n); }
    bool host_free(void *p) { return release("H", p); }
    bool host_device_ptr(void **dp, void *hp) { log << "HD" << id[hp] << " "; *dp = hp; return true; }
    std::string take() { std::string s = log.str(); log.str(""); if (!s.empty()) s.pop_back(); return "[" + s + "]"; }
};

static const char *word(Mem m) { return m == Mem::Ok ? "ok" : m == Mem::FreeFailed ? "free-failed" : m == Mem::AllocFailed ? "refused" : m == Mem::CopyFailed ? "copy-failed" : "no-device-ptr"; }
static unsigned char mark(size_t i) { return (unsigned char)(i * 7 + 3); }

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const int arg = argc > 2 ? atoi(argv[2]) : 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        Fake a;
        std::string tok;
        if (cmd == "grow" || cmd == "keep") {
            DevMem mem; DevBuf<unsigned char> b(mem);
            size_t written = 0;
            while (in >> tok) {
                const bool refuse = tok[0] == '!';
                const size_t bytes = strtoull(tok.c_str() + refuse, nullptr, 0);
                a.refuse_in = refuse ? 1 : 0;
                const Mem m = cmd == "grow" ? devmem_grow(a, b, bytes) : devmem_grow_keep(a, b, bytes);
                a.refuse_in = 0;
                out << word(m) << a.take() << (b.p ? "p" : "-") << b.cap;
                if (cmd == "keep") {      // what was written before is still there; then the whole buffer is written
                    bool kept = true;
                    for (size_t i = 0; i < written && i < b.cap; i++) kept = kept && b[i] == mark(i);
                    for (size_t i = 0; i < b.cap; i++) b.get()[i] = mark(i);
                    written = b.cap;
                    out << (kept ? "kept" : "lost");
                }
                out << " ";
            }
            devmem_release(a, mem);
        } else if (cmd == "pinned") {
            DevMem mem; PinnedBuf<char> b(mem);
            while (in >> tok) {
                const bool refuse = tok[0] == '!';
                unsigned long long bytes = 0, grow = 0; int dev = 0;
                sscanf(tok.c_str() + refuse, "%llu:%llu:%d", &bytes, &grow, &dev);
                a.refuse_in = refuse ? 1 : 0;
                const Mem m = devmem_grow_pinned(a, b, (size_t)bytes, (size_t)grow, dev != 0);
                a.refuse_in = 0;
                out << word(m) << a.take() << (b.p ? "p" : "-") << b.cap << (b.device() ? (b.device() == b.get() ? "d" : "?") : "-") << " ";
            }
            devmem_release(a, mem);
        } else if (cmd == "release") {
            DevMem mem;
            std::deque<DevBuf<char>> bufs;
            std::deque<PinnedBuf<char>> areas;
            std::vector<MemNode *> made;      // in construction order
            while (in >> tok) {
                const bool pin = tok[0] == 'p';
                const size_t bytes = strtoull(tok.c_str() + pin, nullptr, 0);
                if (pin) { areas.emplace_back(mem); made.push_back(&areas.back()); } else { bufs.emplace_back(mem); made.push_back(&bufs.back()); }
                if (bytes && (pin ? devmem_grow_pinned(a, *made.back(), bytes, bytes, false) : devmem_grow(a, *made.back(), bytes)) != Mem::Ok) out << "?";
            }
            bool order = true;
            size_t k = 0;
            for (MemNode *n = mem.first; n; n = n->next, k++) order = order && k < made.size() && n == made[k];
            a.take();
            out << "order " << (order && k == made.size() ? "ok" : "bad") << " ";
            devmem_release(a, mem);
            out << a.take() << " ";
            devmem_release(a, mem);
            out << a.take() << " " << a.id.size();
        } else if (cmd == "table") {
            const StateMap sm = make_state_map(arg);
            for (int k = 0; k < kNumPersist; k++) out << kPersist[k].name << "=" << kPersist[k].row_bytes(sm) << "/" << (kPersist[k].at_create ? 1 : 0) << ";";
        } else if (cmd == "fit") {
            unsigned long long rows = 0;
            StateMap sm{};
            in >> rows >> sm.n_slots >> sm.n_out >> sm.max_delay >> sm.row;
            for (int k = 0; k < kNumPersist; k++) {
                size_t b = 0;
                if (persist_bytes(k, sm, (uint32_t)rows, &b)) out << b << " "; else out << "overflow ";
            }
            out << (persist_rows_fit(sm, (uint32_t)rows) ? "fit" : "refused");
        } else if (cmd == "realloc") {
            const StateMap sm = make_state_map(arg);
            uint32_t rows0 = 0, rows1 = 0, cap_rows = 0; int refuse_at = 0, pdm = 0, base = 0, copy_ok = 1;
            in >> rows0 >> rows1 >> refuse_at >> pdm >> base >> copy_ok;
            DevMem mem; DevBuf<unsigned char> b0(mem), b1(mem), b2(mem), b3(mem), b4(mem);
            MemNode *const arr[kNumPersist] = {&b0, &b1, &b2, &b3, &b4};
            cap_rows = rows0;
            for (int k = 0; k < kNumPersist; k++) {      // every row starts with its number and the array's
                size_t b = 0;
                if (!(kPersist[k].at_create || (k == kArrPdm ? pdm : base))) continue;
                if (!persist_bytes(k, sm, rows0, &b) || devmem_grow(a, *arr[k], b) != Mem::Ok) out << "?";
                for (uint32_t r = 0; r < rows0; r++) static_cast<unsigned char *>(arr[k]->p)[(size_t)r * kPersist[k].row_bytes(sm)] = (unsigned char)(r * 5 + k);
            }
            a.take();
            void *was[kNumPersist];
            for (int k = 0; k < kNumPersist; k++) was[k] = arr[k]->p;
            const uint32_t copy = rows0 < rows1 ? rows0 : rows1;
            a.refuse_in = refuse_at;
            const Mem m = persist_reallocate(a, arr, sm, rows1, cap_rows, [&](void *const *fresh) {
                for (int k = 0; k < kNumPersist; k++) if (fresh[k]) memcpy(fresh[k], arr[k]->p, (size_t)copy * kPersist[k].row_bytes(sm));
                a.log << "copied ";
                return copy_ok != 0;
            });
            a.refuse_in = 0;
            out << word(m) << a.take() << " ";
            bool rows_kept = true;
            for (int k = 0; k < kNumPersist; k++) {
                out << (!arr[k]->p ? "absent" : arr[k]->p == was[k] ? "same" : "moved") << arr[k]->cap << " ";
                for (uint32_t r = 0; arr[k]->p && r < (m == Mem::Ok ? copy : rows0); r++)
                    rows_kept = rows_kept && static_cast<unsigned char *>(arr[k]->p)[(size_t)r * kPersist[k].row_bytes(sm)] == (unsigned char)(r * 5 + k);
            }
            out << cap_rows << (rows_kept ? " rows_kept" : " rows_lost");
            devmem_release(a, mem);
        } else {
            fprintf(stderr, "usage: devmem_driver grow | keep | pinned | release | table FLAVOR | fit | realloc FLAVOR\n");
            return 2;
        }
        if (!a.id.empty() && cmd != "release") out << " LEAK";
        std::cout << out.str() << "\n";
    }
    return 0;
}
