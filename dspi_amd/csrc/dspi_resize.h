// dspi_resize.h — resizing a context (dspi_resize_streams / dspi_reserve_streams, include/dspi.h): what a new stream count must satisfy,
// the row arithmetic of the persistent per-stream arrays, and the new slots of a grow as work items of the power-on kernel
// (dspi_boot.hip).  Plain C++ (no HIP): dspi_capi.cpp includes it, tests/resize_driver.cpp exercises it without a GPU.
//
// The arrays (state slots, delay lines, rings, PDM words) are stacks of rows of R streams, row-outermost: a context holds `capacity` rows
// of each and uses the first rows(n_streams) of them.  A resize inside the capacity changes no allocation; one past it, and every
// dspi_reserve_streams that changes the capacity, allocates arrays of exactly the rows wanted and copies the rows in use.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_boot.h"

namespace dspi {

constexpr uint32_t kResizePaused = 0x1u;      // DSPI_RESIZE_PAUSED

constexpr uint32_t resize_rows_of(uint32_t n_streams, uint32_t row_streams) { return n_streams / row_streams + (n_streams % row_streams ? 1u : 0u); }

// ---- validation ----
// nullptr = a context of n_old streams whose slot s is active where active[s] != 0 (active == nullptr: every slot is) may be resized to
// n_new; else which rule refuses it: a count of 0, an undefined flag bit, a slot of the cut range [n_new, n_old) that is active.
const char *resize_validate(uint32_t n_old, uint32_t n_new, uint32_t flags, const uint8_t *active);
// ... may reserve room for n_reserve streams; else: a count of 0, a count below the streams in use.
const char *reserve_validate(uint32_t n_streams, uint32_t n_reserve);
// the bytes of `rows` rows of `row_bytes` each; false where the product does not fit a size_t (the caller refuses the call)
bool resize_bytes(uint32_t rows, size_t row_bytes, size_t *bytes);

// ---- row arithmetic ----
// before / after: the rows in use; capacity: the rows allocated after the call; reallocate: new arrays of `capacity` rows are made and the
// first `copy` rows of the old ones copied into them (copy = 0 without a reallocation)
struct ResizeRows { uint32_t before, after, capacity, copy; bool reallocate; };
// dspi_resize_streams: a grow past the capacity reallocates to exactly the rows needed; everything else keeps the capacity
ResizeRows resize_rows(uint32_t n_old, uint32_t n_new, uint32_t capacity_rows, uint32_t row_streams);
// dspi_reserve_streams: the capacity becomes rows(n_reserve), whichever way; nothing happens where it has that value already
ResizeRows reserve_rows(uint32_t n_streams, uint32_t n_reserve, uint32_t capacity_rows, uint32_t row_streams);

// ---- the new slots of a grow ----
// [n_old, n_new), ascending
std::vector<uint32_t> resize_new_slots(uint32_t n_old, uint32_t n_new);
// ... as the power-on kernel's work items (boot_row_items): the residents are the ACTIVE streams below n_old, so the partial row that
// is grown takes the positions of its lowest-numbered active stream, and a row without one — every whole new row — has no target
std::vector<BootRowItem> resize_row_items(uint32_t n_old, uint32_t n_new, uint32_t row_streams, const uint8_t *active);

}  // namespace dspi
