// dspi_boot.h — power-cycling streams inside a running context (dspi_boot_streams, include/dspi.h): what a stream list must satisfy, and
// the work items of the kernel that writes power-on state into the listed columns (dspi_boot.hip).  Plain C++ (no HIP): dspi_capi.cpp and
// dspi_boot.hip include it, tests/boot_driver.cpp exercises it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_move.h"

namespace dspi {

constexpr uint32_t kBootNone = kMoveNone;      // a row's target: nobody's, the booted streams keep the power-on write positions (0, 0)

// ---- validation ----
// nullptr = the list may be applied to a context of n_streams; else which rule refuses it: an empty or null list, an index at or past
// n_streams, a slot listed twice.  The list may be in any order.
const char *boot_validate(const uint32_t *streams, uint32_t n, uint32_t n_streams);

// ---- work items of the power-on kernel (dspi_boot.hip) ----
// One item per touched row (rows ascending): the listed columns (bit c % 32 of cols[c / 32]; row_streams <= 128), per group of four
// columns whether any / all of them are listed (bit q = columns 4q .. 4q + 3, as MoveRowItem has them), and whose (delay write index,
// ring position) the row's booted streams take.  Zero lines and rings are zero under every rotation, so a booted stream simply TAKES the
// pair of its row and the row stays on the kernels' one-access path: `target` names the row's lowest-numbered resident (the row-target
// rule, dspi_move.h row_lowest_resident, with the list as `listed`), whose two position words the device reads behind the context's
// earlier work; kBootNone where the row has no resident, and everywhere with power_on_positions (DSPI_BOOT_STREAMS_AS_IS).
struct BootRowItem { uint32_t row, q_any, q_all, target, cols[4]; };
std::vector<BootRowItem> boot_row_items(const uint32_t *streams, uint32_t n, uint32_t n_streams, uint32_t row_streams, const uint8_t *active, bool power_on_positions);

}  // namespace dspi
