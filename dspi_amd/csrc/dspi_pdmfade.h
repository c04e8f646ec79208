// dspi_pdmfade.h — the PDM fade-out on disable (dspi_pdm_fade, include/dspi.h; pdm_generator.c:223-237, :323-348): the mode, one fade
// position per stream, and what they make of a dspi_process_pdm call's work list.  Plain C++ (no HIP): dspi_capi.cpp includes it,
// tests/pdmfade_driver.cpp exercises it without a GPU.  PdmLife (dspi_pdmlife.h) stays what it is: the context hands its rule a "sub on"
// that is also true for a stream that fades or is about to (wants), so those streams stay ordinary listed entries, and this book says
// beside the list, one AUX WORD PER LIST ENTRY, what each lane does instead of a normal call:
//   0                         as without the mode
//   kPdmAuxFade | p           fade out from position p (2..1024; 1024: the fade starts with this call): frame f plays position p - 1 - f
//                             while that is >= 1, `sub` is not read; the frames after position 1 are zero words
//   kPdmAuxCancel | p         the sub came on again while fading at p: fade-in position := 1024 - p, no reset, then a normal call
// `plan` builds the words and changes no position; `commit` is the successful call: it advances the positions by the call's frames, ends
// the fades that have played position 1 (their running bytes go to 0 through PdmLife::set_get, dspi_pdm_running's own path) and keeps
// PdmLife dirty for as long as any word was non-zero.  With the mode off no word is ever non-zero and nothing here costs a call anything.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "dspi_move.h"
#include "dspi_pdmlife.h"

namespace dspi {

constexpr uint32_t kPdmAuxFade = 1u << 30, kPdmAuxCancel = 1u << 31, kPdmAuxPos = 0x7ffu;
constexpr uint32_t kPdmFadeStart = 1024;      // fade_out_pos of a disable (pdm_generator.c:227); the first sample plays 1023
constexpr uint32_t kPdmFadeMaxHeld = 1023;    // the largest position a stream holds between two calls
constexpr int32_t kPdmBaseMax = 29500;        // |fade_base_pcm| <= PDM_CLIP_THRESH: it is a limited sample

struct PdmFade {
    bool on = false;
    std::vector<uint16_t> pos;       // [n_streams]; 0: not fading
    std::vector<uint32_t> aux;       // one word per entry of the PdmWork list `plan` was called for (empty: all zero)
    bool any_aux = false;            // some word is non-zero: `aux` goes up beside the list
    uint64_t planned = ~0ull;        // PdmLife::builds the words stand for

    void create(uint32_t n_streams) { pos.assign(n_streams, 0); aux.clear(); any_aux = false; planned = ~0ull; }
    // dspi_pdm_fade.  Enabling: every stream "not fading" (the caller zeroes the bases).  Disabling: every fade in flight ends at once,
    // byte 0.  Either way the next call plans anew.
    void enable(PdmLife &life);
    void disable(PdmLife &life);
    // what the context hands PdmLife::plan as sub_on(s), given the device's own
    bool wants(const PdmLife &life, uint32_t s, bool sub_on) const { return sub_on || (on && life.running[s] != 0); }
    // the aux words for `life.work` (PdmLife::plan has just run); sub_on(s) is the device's own.  Nothing is rebuilt while the list stands.
    void plan(const PdmLife &life, const std::function<bool(uint32_t)> &sub_on);
    // the call that `plan` was made for has succeeded (after PdmLife::commit), `frames` frames long
    void commit(PdmLife &life, uint32_t frames);
    // the position travels where the running byte does
    void move(const StreamMove *moves, uint32_t n);                       // all entries at once; an open-end source keeps its value
    // a migration's destination side, after PdmLife::arrive: `value` is what the source held (0 when the source has the mode off).  With
    // the mode off here nothing is held: a fade in flight ends as an immediate stop, byte 0.
    void arrive(PdmLife &life, uint32_t s, uint32_t value);
    void boot(const uint32_t *streams, uint32_t n);                       // 0
    void resize(uint32_t n_streams) { pos.resize(n_streams, 0); planned = ~0ull; }
    // dspi_pdm_fade_state's host half: nullptr, or why the call is refused.  A word is pos | (uint16_t)base << 16.
    const char *check(uint32_t first, uint32_t count, const uint32_t *set) const;
};

}  // namespace dspi
