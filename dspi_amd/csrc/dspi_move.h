// dspi_move.h — moving streams between slots of one context (dspi_move_streams / dspi_plan_compaction, include/dspi.h): what a move list
// must satisfy, which list compacts a context, whose write positions a stream written by ANY list-addressed call takes (the row-target
// rule, stated here once), and in which order a list of any shape goes through a scratch of `cap` records.  Plain C++ (no HIP):
// dspi_capi.cpp and dspi_snapshot.hip include it (dspi_migrate.h and dspi_boot.h build on it), tests/move_driver.cpp
// exercises it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dspi {

struct StreamMove { uint32_t src, dst; };      // == dspi_stream_move: slot dst takes the stream that slot src holds
constexpr uint32_t kMoveNone = 0xffffffffu;    // a column of a touched row that the list does not name

// ---- validation ----
// What every list validator asks first of the n slots slots[0], slots[stride], ...: all below seen.size() (decided over the whole list
// before anything else), none named twice.  `seen`: one zero byte per slot; the slots are marked in it (all of them when the answer is ok).
enum class SlotCheck { ok, out_of_range, duplicate };
inline SlotCheck check_slots(const uint32_t *slots, size_t stride, uint32_t n, std::vector<uint8_t> &seen) {
    for (uint32_t i = 0; i < n; i++) if (slots[i * stride] >= seen.size()) return SlotCheck::out_of_range;
    for (uint32_t i = 0; i < n; i++) if (seen[slots[i * stride]]++) return SlotCheck::duplicate;
    return SlotCheck::ok;
}
// nullptr = the list may be applied to a context of n_streams whose slot s is active where active[s] != 0 (active == nullptr: every
// slot is); else which rule refuses it: an empty or null list, an index at or past n_streams, a slot that is the source of two
// entries, a slot that is the destination of two entries, a destination that is active and not itself moved away by the list.
// Entries with src == dst take part in the duplicate rules (the slot is then a source and a destination) and are otherwise dropped.
const char *move_validate(const StreamMove *moves, uint32_t n, uint32_t n_streams, const uint8_t *active);

// ---- compaction ----
// The shortest list after which slots [0, A) are active and [A, n_streams) paused, A = the number of active slots: H = the paused slots
// below A, T = the active slots at or above A, both ascending (|H| == |T|); pair i is the swap {T[i] -> H[i]}, {H[i] -> T[i]}, or, one_way
// (the caller treats paused slots as free), {T[i] -> H[i]} alone.
std::vector<StreamMove> move_compaction(const uint8_t *active, uint32_t n_streams, bool one_way);

// ---- realignment: THE ROW-TARGET RULE of every list-addressed call (moves, migrations, boots, resizes) ----
// A stream written into a row takes the (delay write index, ring position) of the row's lowest-numbered RESIDENT — a slot below n_streams
// that is active (active == nullptr: every slot is) and not marked in `listed` (one byte per slot, may be null) —, read from the state
// array AS IT STANDS BEFORE THE CALL; where the row has none, those of the ARRIVAL at the row's lowest destination.  (include/dspi.h
// says the same to the caller.)  kMoveNone: the row has no resident.
inline uint32_t row_lowest_resident(uint32_t row, uint32_t row_streams, uint32_t n_streams, const uint8_t *active, const uint8_t *listed) {
    const uint64_t r0 = (uint64_t)row * row_streams, r1 = r0 + row_streams < n_streams ? r0 + row_streams : n_streams;
    for (uint64_t s = r0; s < r1; s++)
        if ((!active || active[s]) && !(listed && listed[s])) return (uint32_t)s;
    return kMoveNone;
}
// One per entry, in list order, for destinations in a context of n_dst streams: from_entry == 0: `target` is the resident's slot;
// from_entry == 1: `target` is the INDEX of the entry whose destination is the row's lowest, whose stream's positions are read where it
// stands before the call.  A move inside one context passes its list without identities and `listed` = that list's sources and
// destinations; a migration passes listed = nullptr (its destinations are paused: none is a resident).  The device
// (dspi_snapshot.hip list_shifts_kernel) reads both positions behind the context's earlier work and rotates the stream by their difference.
struct ListTarget { uint32_t src, dst, target, from_entry; };
std::vector<ListTarget> list_targets(const StreamMove *moves, uint32_t n, uint32_t n_dst, uint32_t row_streams, const uint8_t *dst_active, const uint8_t *listed);

// ---- for the CPU drivers of earlier commits only (tests/move_driver.cpp as it stood before list_targets): the move's call of list_targets
// with a SLOT per applied entry.  Header-only: nothing of it is in the library, and no rule of its own. ----
struct MoveTarget { uint32_t src, dst, target; };
inline std::vector<MoveTarget> move_targets(const StreamMove *moves, uint32_t n, uint32_t n_streams, uint32_t row_streams, const uint8_t *active) {
    std::vector<StreamMove> mv;
    std::vector<uint8_t> listed(n_streams, 0);
    for (uint32_t i = 0; i < n; i++)
        if (moves[i].src != moves[i].dst) { mv.push_back(moves[i]); listed[moves[i].src] = listed[moves[i].dst] = 1; }
    std::vector<MoveTarget> out;
    for (const ListTarget &t : list_targets(mv.data(), (uint32_t)mv.size(), n_streams, row_streams, active, listed.data()))
        out.push_back(MoveTarget{t.src, t.dst, t.from_entry ? mv[t.target].src : t.target});
    return out;
}

// ---- the batch schedule ----
// The scratch holds `cap` (>= 2) records.  A batch gathers some slots' columns into records, then scatters records into slots; the
// batches run in order.  Within a batch every gather precedes every scatter, so a swap or a whole cycle inside one batch needs nothing
// more.  Across batches no slot is written before its own old content was gathered, unless the list discards that content:
//   chains   a -> b -> ... -> z (z a destination only: its occupant is discarded) go tail first, z's entry first: every destination was
//            a source in an earlier or the same batch, so a chain may be cut anywhere
//   cycles   of at most cap entries go into one batch whole (a new batch is begun when the current one has not enough room left)
//   a cycle longer than cap is broken: its last slot's content goes into record 0 and is HELD there while the rest of the cycle runs as
//            a chain, tail first, through records 1 .. cap - 1; the batch that ends the chain also scatters record 0 into the cycle's
//            first slot.  No other group shares these batches.
// A record index below cap appears at most once among a batch's gathers and is only scattered after it was gathered (in this batch or,
// for the held record, an earlier one).
struct MoveRecord { uint32_t slot, record; };
struct MoveBatch { std::vector<MoveRecord> gather, scatter; };
std::vector<MoveBatch> move_schedule(const StreamMove *moves, uint32_t n, uint32_t cap);

// ---- work items of the list-addressed kernels (dspi_snapshot.hip) ----
// One item per touched row: which record each of its columns goes to / comes from (colrec, row_streams words per item, kMoveNone = not
// listed), and per group of four columns whether any / all of them are listed (bit q = columns 4q .. 4q + 3; row_streams <= 128).
struct MoveRowItem { uint32_t row, q_any, q_all, pad; };
// appends the items of `list` (rows ascending) and their colrec words
void move_row_items(const std::vector<MoveRecord> &list, uint32_t row_streams, std::vector<MoveRowItem> &items, std::vector<uint32_t> &colrec);

}  // namespace dspi
