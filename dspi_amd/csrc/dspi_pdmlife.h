// dspi_pdmlife.h — which streams' PDM modulators run in a dspi_process_pdm call (include/dspi.h): one byte per stream, *running*, the
// rule that turns it, the host's record of pauses and the devices' own "sub on" into the call's work list, and what the stream
// maintenance calls do to the byte.  Plain C++ (no HIP): dspi_capi.cpp includes it, tests/pdmlife_driver.cpp exercises it without a GPU.
//
// The rule, for every ACTIVE stream of a successful call (a paused one is not modulated and its byte is left alone):
//   sub on, not running   listed with kPdmListReset: modulated after the re-enable reset (pdm_generator.c:239-252); the byte becomes 1
//   sub on, running       listed: modulated, its state carried over
//   sub off               not listed; the byte becomes 0
// `plan` builds the list and changes no byte; `commit` is the successful call: it writes the bytes the list stands for.  A list without
// reset bits stays valid until something that can change it happens (`dirty`): plan then builds nothing.
// Who is paused is the context's record (`active`: one byte per stream, 1 = active; nullptr = every stream is): every function that takes
// it takes it AS IT STANDS BEFORE the context applies the call it belongs to.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <utility>
#include <vector>

#include "dspi_move.h"

namespace dspi {

constexpr uint32_t kPdmListReset = 1u << 31;      // a work-list word: the stream in bits 0..30; this bit: the re-enable reset first

struct PdmWork {
    std::vector<uint32_t> list;                               // the listed streams, ascending
    std::vector<std::pair<uint32_t, uint32_t>> unlisted;      // [first, end) of consecutive unlisted streams, ascending
    std::vector<uint32_t> stops;                              // active streams whose sub is off while their byte is 1
    bool resets = false;                                      // some word carries kPdmListReset
    // the words of streams [s0, s1): [first, second) into `list`
    std::pair<size_t, size_t> range(uint32_t s0, uint32_t s1) const;
};

struct PdmLife {
    std::vector<uint8_t> running;      // [n_streams]
    bool dirty = true;                 // `work` may no longer be what the rule gives
    bool uploaded = false;             // the device's copy of work.list is the list (the context's flag: cleared whenever the list is built)
    uint64_t builds = 0;               // how often the rule has run
    PdmWork work;

    void create(uint32_t n_streams) { running.assign(n_streams, 0); mark_dirty(); }
    void mark_dirty() { dirty = true; }
    // the rule.  sub_on(s): stream s's device has its sub output on (Params::core1_mode == 1)
    const PdmWork &plan(const uint8_t *active, const std::function<bool(uint32_t)> &sub_on);
    // the call that `plan` was made for has succeeded
    void commit();
    // dspi_move_streams (a validated list): running[dst] := old running[src] for all entries at once; an open-end source keeps its value
    void move(const StreamMove *moves, uint32_t n);
    // dspi_migrate_streams, the destination context's side: slot s takes a stream whose byte is `value`
    void arrive(uint32_t s, uint8_t value) { running[s] = value ? 1 : 0; mark_dirty(); }
    // dspi_boot_streams: a device that has just been powered on has never run its modulator
    void boot(const uint32_t *streams, uint32_t n);
    // dspi_resize_streams: cut at n_streams, or extended with zeros
    void resize(uint32_t n_streams) { running.resize(n_streams, 0); mark_dirty(); }
    // dspi_pdm_running: nullptr, or why the call is refused (nothing is written then); `set` and `get` may each be null
    const char *set_get(uint32_t first, uint32_t count, const uint8_t *set, uint8_t *get);
};

}  // namespace dspi
