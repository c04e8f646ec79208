// dspi_meters.cpp — the meter bridge on the CPU: the argument rules, the update, the alarm scan and the status block (dspi_meters.h).
#include "dspi_meters.h"

#include <initializer_list>

namespace dspi {

const char *meters_update_why(const void *peaks, uint32_t n_blocks, uint32_t hold_packets, uint32_t decay_q15, const void *meters, uint32_t flags, uint32_t n, int n_ch) {
    if (!peaks || !meters) return "a NULL pointer";
    if (n_blocks == 0) return "n_blocks is 0";
    if (hold_packets > kMeterMaxHold) return "hold_packets above 65535";
    if (decay_q15 > kMeterMaxDecay) return "decay_q15 above 32768";
    if (flags & ~kMeterMemDevice) return "the only flag is DSPI_MEM_DEVICE";
    size_t b;
    if (__builtin_mul_overflow((size_t)n * (size_t)n_ch * 2u, (size_t)n_blocks, &b)) return "the size of peaks overflows";
    if ((flags & kMeterMemDevice) && (reinterpret_cast<uintptr_t>(peaks) % 4u || reinterpret_cast<uintptr_t>(meters) % 4u)) return "device pointers are 4-byte aligned";
    return nullptr;
}

const char *meters_alarms_why(const void *meters, uint32_t level_q15, const void *streams, const void *info, uint32_t cap, const void *total, uint32_t flags) {
    if (!streams || !total) return "a NULL pointer (streams, total)";
    if (cap == 0) return "cap is 0";
    if (level_q15 > kMeterMaxLevel) return "level_q15 above 65535";
    if (flags & ~kMeterMemDevice) return "the only flag is DSPI_MEM_DEVICE";
    if (flags & kMeterMemDevice)
        for (const void *p : {meters, streams, info, total})
            if (reinterpret_cast<uintptr_t>(p) % 4u) return "device pointers are 4-byte aligned";
    return nullptr;
}

const char *status_all_why(uint32_t first, uint32_t count, const void *buf, uint32_t flags, uint32_t n) {
    if (!buf) return "a NULL pointer";
    if (count == 0) return "count is 0";
    if (first >= n || count > n - first) return "stream range out of bounds";
    if (flags & ~kMeterMemDevice) return "the only flag is DSPI_MEM_DEVICE";
    return nullptr;
}

uint32_t clear_list_check(const uint32_t *streams, uint32_t count, uint32_t n) {
    for (uint32_t i = 0; i < count; i++)
        if (streams[i] >= n) return i;
    return count;
}

void meters_update_cpu(const uint16_t *peaks, uint32_t n, uint32_t n_blocks, int n_ch, uint32_t hold_packets, uint32_t decay_q15, uint32_t *meters, const uint8_t *active) {
    const size_t C = (size_t)n_ch;
    for (uint32_t s = 0; s < n; s++) {
        if (active && !active[s]) continue;
        const uint16_t *p = peaks + (size_t)s * n_blocks * C;
        uint32_t *m = meters + (size_t)s * C;
        for (size_t c = 0; c < C; c++) {
            uint32_t w = m[c];
            for (size_t k = 0; k < n_blocks; k++) w = meter_step(w, p[k * C + c], hold_packets, decay_q15);
            m[c] = w;
        }
    }
}

uint32_t meters_alarms_cpu(const uint32_t *meters, const uint16_t *clip, uint32_t n, int n_ch, uint32_t level_q15, uint32_t *streams, uint32_t *info, uint32_t cap, uint32_t *total) {
    uint32_t found = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t w = alarm_info(meters ? meters + (size_t)s * (size_t)n_ch : nullptr, n_ch, level_q15, clip ? clip[s] : 0u);
        if (!w) continue;
        if (found < cap) { streams[found] = s; if (info) info[found] = w; }
        found++;
    }
    *total = found;
    return found < cap ? found : cap;
}

void status_pack(const uint16_t *peaks, uint16_t clip, int n_ch, uint8_t *out) {
    for (int i = 0; i < n_ch; i++) { out[2 * i] = (uint8_t)(peaks[i] & 0xff); out[2 * i + 1] = (uint8_t)(peaks[i] >> 8); }
    out[2 * n_ch] = 0; out[2 * n_ch + 1] = 0;      // cpu0_load / cpu1_load: no MCU here
    out[2 * n_ch + 2] = (uint8_t)(clip & 0xff); out[2 * n_ch + 3] = (uint8_t)(clip >> 8);
}

}  // namespace dspi
