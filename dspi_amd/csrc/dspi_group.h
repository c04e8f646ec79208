// dspi_group.h — which move list puts the active streams of every parameter object into one run of slots, runs of one structure side by
// side (dspi_plan_grouping, include/dspi.h): the launch plan (dspi_plan.h) picks the kernel by who sits beside whom, and this is the list
// after which neighbours share what it asks for.  Plain C++ (no HIP): dspi_capi.cpp includes it, tests/group_driver.cpp exercises it
// without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_move.h"
#include "dspi_plan.h"

namespace dspi {

// ---- structure classes ----
// out[i] = the lowest j with sig[j] == sig[i], byte for byte: images of one class may share a row of the per-lane-value kernels.
std::vector<uint32_t> group_classes(const ImageSig *sig, size_t n);

// ---- the grouping rule ----
// active[s] != 0: slot s is active (nullptr: every slot is); stream_object[s]: the parameter object slot s refers to, equal objects already
// folded; object_class[o]: the structure class of object o (nullptr: one class, the Q28 flavour).  A = the number of active slots.
//   groups     a group is the set of active streams of one object.  first(g) = its lowest slot, first(class) = the minimum over the
//              class's groups; groups are ordered by (first(class), first(g))
//   runs       in that order group g gets the next |g| slots of [0, A)
//   residents  a stream of g that already sits inside g's run stays
//   movers     the other streams of g, ascending by slot, take the run's remaining slots, ascending
//   paused     H = the paused slots below A, T = the slots at or above A that hold an active stream, both ascending (|H| == |T|): entry i
//              is {H[i] -> T[i]}; one_way (the caller treats paused slots as free) leaves these entries out
//   output     no identities; ascending by dst
// The list is legal for move_validate in both modes, no shorter list reaches this layout (its length is the active streams outside their
// run, plus |H| without one_way), and on a context it has been applied to the rule returns nothing.
std::vector<StreamMove> group_plan(const uint8_t *active, const int32_t *stream_object, const uint32_t *object_class, uint32_t n_streams, bool one_way);

}  // namespace dspi
