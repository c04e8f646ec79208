// dspi_pdmfade.cpp — the PDM fade-out's mode, positions and aux words: see dspi_pdmfade.h.
#include "dspi_pdmfade.h"

namespace dspi {

namespace {
void stop(PdmLife &life, uint32_t s) {      // the running byte to 0, through dspi_pdm_running's own path
    const uint8_t zero = 0;
    (void)life.set_get(s, 1, &zero, nullptr);
}
}  // namespace

void PdmFade::enable(PdmLife &life) {
    if (on) return;
    on = true;
    pos.assign(life.running.size(), 0);
    life.mark_dirty();
}

void PdmFade::disable(PdmLife &life) {
    if (!on) return;
    on = false;
    for (uint32_t s = 0; s < (uint32_t)pos.size(); s++)
        if (pos[s]) { pos[s] = 0; stop(life, s); }
    life.mark_dirty();
}

void PdmFade::plan(const PdmLife &life, const std::function<bool(uint32_t)> &sub_on) {
    if (planned == life.builds) return;
    planned = life.builds;
    aux.clear(); any_aux = false;
    if (!on) return;
    const std::vector<uint32_t> &list = life.work.list;
    aux.assign(list.size(), 0u);
    for (size_t i = 0; i < list.size(); i++) {
        const uint32_t s = list[i] & ~kPdmListReset;
        if (list[i] & kPdmListReset) continue;      // a modulator that comes up through the reset fades nothing (commit drops a stale position)
        if (sub_on(s)) { if (pos[s]) aux[i] = kPdmAuxCancel | pos[s]; }
        else aux[i] = kPdmAuxFade | (pos[s] ? (uint32_t)pos[s] : kPdmFadeStart);
        if (aux[i]) any_aux = true;
    }
}

void PdmFade::commit(PdmLife &life, uint32_t frames) {
    if (!on || (!any_aux && !life.work.resets)) return;
    const std::vector<uint32_t> &list = life.work.list;
    for (size_t i = 0; i < list.size() && i < aux.size(); i++) {
        const uint32_t s = list[i] & ~kPdmListReset, a = aux[i], p = a & kPdmAuxPos;
        if ((list[i] & kPdmListReset) || (a & kPdmAuxCancel)) pos[s] = 0;
        else if (a & kPdmAuxFade) {
            if (p - 1 <= frames) { pos[s] = 0; stop(life, s); }      // position 1 has been played: the fade is over
            else pos[s] = (uint16_t)(p - frames);
        }
    }
    life.mark_dirty();      // the next call's words differ
}

void PdmFade::move(const StreamMove *moves, uint32_t n) {
    std::vector<uint16_t> in(n);      // every source is read before any slot is written
    for (uint32_t i = 0; i < n; i++) in[i] = pos[moves[i].src];
    for (uint32_t i = 0; i < n; i++) pos[moves[i].dst] = in[i];
}

void PdmFade::arrive(PdmLife &life, uint32_t s, uint32_t value) {
    if (on) { pos[s] = (uint16_t)value; return; }
    pos[s] = 0;
    if (value) stop(life, s);
}

void PdmFade::boot(const uint32_t *streams, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) pos[streams[i]] = 0;
}

const char *PdmFade::check(uint32_t first, uint32_t count, const uint32_t *set) const {
    if (count == 0 || (uint64_t)first + count > pos.size()) return "stream range out of bounds";
    if (set) for (uint32_t k = 0; k < count; k++) {
        const int32_t base = (int16_t)(uint16_t)(set[k] >> 16);
        if ((set[k] & 0xffffu) > kPdmFadeMaxHeld) return "a fade position is 0..1023";
        if (base > kPdmBaseMax || base < -kPdmBaseMax) return "a base is within +-29500";
    }
    return nullptr;
}

}  // namespace dspi
