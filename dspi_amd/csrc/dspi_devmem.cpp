// dspi_devmem.cpp — see dspi_devmem.h.
#include "dspi_devmem.h"

#include "dspi_resize.h"
#include "dspi_snapshot.h"

namespace dspi {

// [rows][positions][row streams] 32-bit words; the positions per row are the snapshot record's sections (dspi_snapshot.h), the fade base is one word
const PersistInfo kPersist[kNumPersist] = {
    {"state", [](const StateMap &m) { return (size_t)m.n_slots * (size_t)m.row * 4; }, true},
    {"delay lines", [](const StateMap &m) { return (size_t)m.n_out * (size_t)m.max_delay * (size_t)m.row * 4; }, true},
    {"leveller ring", [](const StateMap &m) { return (size_t)kRingLen * 2 * (size_t)m.row * 4; }, true},
    {"PDM state", [](const StateMap &m) { return (size_t)kPdmWords * (size_t)m.row * 4; }, false},
    {"PDM fade bases", [](const StateMap &m) { return (size_t)m.row * 4; }, false},
};

bool persist_bytes(int k, const StateMap &sm, uint32_t rows, size_t *bytes) { return resize_bytes(rows, kPersist[k].row_bytes(sm), bytes); }

bool persist_rows_fit(const StateMap &sm, uint32_t rows) {
    size_t b = 0;
    for (int k = 0; k < kNumPersist; k++) if (!persist_bytes(k, sm, rows, &b)) return false;
    return true;
}

}  // namespace dspi
