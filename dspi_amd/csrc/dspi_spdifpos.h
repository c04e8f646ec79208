// dspi_spdifpos.h — per-stream S/PDIF block positions (dspi_spdif_per_stream / dspi_spdif_stream_pos, include/dspi.h): where in the
// 192-frame channel-status block each stream's next DSPI_OUT_SPDIF frame stands, through pauses, resumes, moves and boots.  Plain C++
// (no HIP): dspi_capi.cpp includes it, tests/spdifpos_driver.cpp exercises it without a GPU.
//
// Representation: the context keeps a clock T (mod 192) that every successful DSPI_OUT_SPDIF call advances by its frames, and one word per
// stream: an ACTIVE stream holds an offset, its position is (T + word) mod 192; a PAUSED stream holds its frozen position itself.  So a
// call costs one addition whatever the stream count, the device's copy of the words (the encoder adds the launch's T to them) changes
// only when a pause, resume, set, move or boot rewrote one, and `dirty` says that it has.
// Who is paused is the context's record (`active`: one byte per stream, 1 = active; nullptr = every stream is): every function takes it
// AS IT STANDS BEFORE the context applies the call it belongs to.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspi_move.h"

namespace dspi {

constexpr uint32_t kSpdifBlock = 192;      // frames per channel-status block

struct SpdifPos {
    bool on = false;
    bool dirty = false;              // a word changed since the device's copy was made
    uint32_t clock = 0;              // T
    std::vector<uint32_t> word;      // [n_streams] while on: offset (active) or frozen position (paused), both below kSpdifBlock

    // on: every stream's position becomes `pos` (the context's own) — already on: nothing changes.  off: the words are dropped.
    void enable(uint32_t n_streams, uint32_t pos);
    void disable();
    // a successful DSPI_OUT_SPDIF call of `frames` frames: every active stream moves on, no paused one does
    void advance(uint64_t frames) { clock = (uint32_t)((clock + frames) % kSpdifBlock); }
    uint32_t get(uint32_t s, const uint8_t *active) const { return is_active(s, active) ? (clock + word[s]) % kSpdifBlock : word[s]; }
    void set(uint32_t s, uint32_t pos, const uint8_t *active) { put(s, pos, is_active(s, active)); }
    // dspi_pause_streams / dspi_resume_streams on [first, first + count): the streams that change freeze at / continue from their position
    void pause(uint32_t first, uint32_t count, const uint8_t *active);
    void resume(uint32_t first, uint32_t count, const uint8_t *active);
    // dspi_move_streams (a validated list): pos[dst] := old pos[src] for all entries at once, the activity travelling with the stream; a
    // source that is no destination keeps its position as a frozen copy (it becomes paused)
    void move(const StreamMove *moves, uint32_t n, const uint8_t *active);
    // dspi_migrate_streams, the destination context's side: slot s takes a stream that stands at `pos` and is active or paused as `act` says,
    // whatever the slot was before
    void arrive(uint32_t s, uint32_t pos, bool act) { put(s, pos % kSpdifBlock, act); }
    // dspi_boot_streams: the listed slots' next frame is frame 0 of a block; a paused slot stays paused
    void boot(const uint32_t *streams, uint32_t n, const uint8_t *active);

private:
    static bool is_active(uint32_t s, const uint8_t *active) { return !active || active[s]; }
    void put(uint32_t s, uint32_t pos, bool act) { word[s] = act ? (pos + kSpdifBlock - clock) % kSpdifBlock : pos; dirty = true; }
};

}  // namespace dspi
