// dspi_resize.cpp — see dspi_resize.h.
#include "dspi_resize.h"

namespace dspi {

const char *resize_validate(uint32_t n_old, uint32_t n_new, uint32_t flags, const uint8_t *active) {
    if (n_new == 0) return "a context holds at least one stream";
    if (flags & ~kResizePaused) return "undefined flag bits";
    for (uint32_t s = n_new; s < n_old; s++)
        if (!active || active[s]) return "a slot of the cut range is active";
    return nullptr;
}

const char *reserve_validate(uint32_t n_streams, uint32_t n_reserve) {
    if (n_reserve == 0) return "a context holds at least one stream";
    if (n_reserve < n_streams) return "fewer streams than the context holds";
    return nullptr;
}

bool resize_bytes(uint32_t rows, size_t row_bytes, size_t *bytes) {
    if (row_bytes && rows > (size_t)-1 / row_bytes) return false;
    *bytes = (size_t)rows * row_bytes;
    return true;
}

ResizeRows resize_rows(uint32_t n_old, uint32_t n_new, uint32_t capacity_rows, uint32_t row_streams) {
    ResizeRows r{resize_rows_of(n_old, row_streams), resize_rows_of(n_new, row_streams), capacity_rows, 0u, false};
    if (r.after > capacity_rows) { r.reallocate = true; r.capacity = r.after; r.copy = r.before; }
    return r;
}

ResizeRows reserve_rows(uint32_t n_streams, uint32_t n_reserve, uint32_t capacity_rows, uint32_t row_streams) {
    const uint32_t used = resize_rows_of(n_streams, row_streams), want = resize_rows_of(n_reserve, row_streams);
    ResizeRows r{used, used, capacity_rows, 0u, false};
    if (want != capacity_rows) { r.reallocate = true; r.capacity = want; r.copy = used; }
    return r;
}

std::vector<uint32_t> resize_new_slots(uint32_t n_old, uint32_t n_new) {
    std::vector<uint32_t> l;
    for (uint32_t s = n_old; s < n_new; s++) l.push_back(s);
    return l;
}

std::vector<BootRowItem> resize_row_items(uint32_t n_old, uint32_t n_new, uint32_t row_streams, const uint8_t *active) {
    const std::vector<uint32_t> l = resize_new_slots(n_old, n_new);
    // (n_streams = n_old: nobody at or past it is a resident, and `active` has n_old entries)
    return boot_row_items(l.data(), (uint32_t)l.size(), n_old, row_streams, active, false);
}

}  // namespace dspi
