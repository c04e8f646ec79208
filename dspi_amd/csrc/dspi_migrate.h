// dspi_migrate.h — moving streams between slots of TWO contexts (dspi_migrate_streams / dspi_plan_migration, include/dspi.h): what a list
// must satisfy in both contexts, which list rebalances, and how the list goes through a scratch of `cap` records.  Plain C++ (no HIP):
// dspi_capi.cpp includes it, tests/migrate_driver.cpp exercises it without a GPU.  In every entry `src` is a slot of the source context
// and `dst` a slot of the destination context.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_move.h"

namespace dspi {

// ---- validation ----
// nullptr = the list may be applied between a source context of n_src streams and a destination context of n_dst streams whose slot s is
// active where dst_active[s] != 0 (dst_active == nullptr: every slot is); else which rule refuses it: an empty or null list, a source at
// or past n_src, a destination at or past n_dst, a slot named twice as a source, a slot named twice as a destination, an active
// destination (a migration never overwrites an active stream).
const char *migrate_validate(const StreamMove *moves, uint32_t n, uint32_t n_src, uint32_t n_dst, const uint8_t *dst_active);

// ---- the rebalancing list ----
// k = min(want, active slots of the source, paused slots of the destination) entries: the sources are the k HIGHEST active slots of the
// source context (a compact source stays compact, its top becomes cuttable), the destinations the k LOWEST paused slots of the destination
// context; entry i pairs the i-th lowest source with the i-th lowest destination.  (nullptr: every slot is active.)
std::vector<StreamMove> migrate_plan(const uint8_t *src_active, uint32_t n_src, const uint8_t *dst_active, uint32_t n_dst, uint32_t want);

// ---- realignment ----
// Whose (delay write index, ring position) an arriving stream takes: the row-target rule and list_targets (dspi_move.h), with
// listed = nullptr — every destination is paused, so none is a resident.
// For the CPU driver only (tests/migrate_driver.cpp, unchanged since before list_targets): that call without the sources.  Header-only:
// nothing of it is in the library, and no rule of its own.
struct MigrateTarget { uint32_t dst, target, from_entry; };
inline std::vector<MigrateTarget> migrate_targets(const StreamMove *moves, uint32_t n, uint32_t n_dst, uint32_t row_streams, const uint8_t *dst_active) {
    std::vector<MigrateTarget> out;
    for (const ListTarget &t : list_targets(moves, n, n_dst, row_streams, dst_active, nullptr)) out.push_back(MigrateTarget{t.dst, t.target, t.from_entry});
    return out;
}

// ---- the batches ----
// Two contexts have no cycles and no chains: no slot is read after it was written.  The batches are consecutive pieces of the list of at
// most `cap` (>= 1) entries; entry first + k of a piece goes through record k: gathered from its source slot in the source context,
// scattered into its destination slot in the destination context.  The row items of either side come from move_row_items (dspi_move.h).
std::vector<MoveBatch> migrate_batches(const StreamMove *moves, uint32_t n, uint32_t cap);

}  // namespace dspi
