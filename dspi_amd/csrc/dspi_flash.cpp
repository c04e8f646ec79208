// dspi_flash.cpp — a stream's own flash: sector rules, the preset directory, the preset API over (flash, parameters), the book
// (dspi_flash.h).  Line numbers cite firmware/DSPi/flash_storage.c unless another file is named.
#include "dspi_flash.h"

#include <string.h>

#include <algorithm>
#include <map>

namespace dspi {

namespace {
constexpr uint32_t kDirMagic = 0x44535032u, kSlotMagic = 0x44535033u, kLegacyMagic = 0x44535031u;      // :66-68
constexpr uint16_t kDirVersion = 2;                                                                    // :133
constexpr float kMasterDefaultDb = -20.0f;                                                             // MASTER_VOL_DEFAULT_DB, config.h
constexpr size_t kDirV1Bytes = 340;                                                                    // PresetDirectory_v1, :95-110
constexpr size_t kDirHeader = 12;

PresetDir fresh_dir(const char *name0, uint16_t occupied) {      // dir_ensure's (:445-455) and migrate_legacy's (:1029-1038) directory
    PresetDir d;
    memset(&d, 0, sizeof d);
    d.include_pins = 1;
    d.master_volume_db = kMasterDefaultDb;
    d.slot_occupied = occupied;
    strncpy(d.slot_names[0], name0, kPresetNameLen - 1);
    return d;
}

size_t slot_bytes(int flavor) { return flavor ? 2864 : 1840; }      // sizeof(PresetSlot), == Params::slot_size()
size_t legacy_bytes(int flavor) {                                   // sizeof(LegacyFlashStorage): the slot's layout up to the pin section
    const StateMap m = make_state_map(flavor);
    return 12 + (size_t)m.n_ch * kStoredBands * 16 + 4 + 4 + (size_t)m.n_ch * 4 + 12 + 4 + 4 + 8 + 4 + 8 + (size_t)2 * m.n_out * 8 + (size_t)m.n_out * 12 + 8;
}
template <class V> V rd_at(const uint8_t *p, size_t off) { V v; memcpy(&v, p + off, sizeof v); return v; }

}  // namespace

uint32_t flash_crc32(const uint8_t *d, size_t n) {
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        crc ^= d[i];
        for (int j = 0; j < 8; j++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sectors and the directory
// ---------------------------------------------------------------------------------------------------------------------------------
void Flash::erase_all() { memset(bytes, 0xFF, sizeof bytes); memset(&dir, 0, sizeof dir); dir_valid = 0; }
void Flash::erase_sector(int sector) { memset(bytes + (size_t)sector * kFlashSector, 0xFF, kFlashSector); }
void Flash::write_sector(int sector, const void *payload, size_t len) {      // :315-357
    erase_sector(sector);
    memcpy(bytes + (size_t)sector * kFlashSector, payload, std::min(len, kFlashSector));
}

bool Flash::dir_load(bool persist, bool *wrote) {      // :370-419
    if (wrote) *wrote = false;
    dir_valid = 0;
    if (rd_at<uint32_t>(bytes, 0) != kDirMagic) return false;
    const uint16_t version = rd_at<uint16_t>(bytes, 4);
    const uint32_t crc = rd_at<uint32_t>(bytes, 8);
    if (version == kDirVersion) {
        if (flash_crc32(bytes + kDirHeader, sizeof(PresetDir) - kDirHeader) != crc) return false;
        memcpy(&dir, bytes, sizeof dir);
        dir_valid = 1;
        return true;
    }
    if (version == 1) {      // :390-414: startup bytes and the occupied mask stand where they do in version 2, the names 4 bytes earlier
        if (flash_crc32(bytes + kDirHeader, kDirV1Bytes - kDirHeader) != crc) return false;
        memset(&dir, 0, sizeof dir);
        dir.startup_mode = bytes[12]; dir.default_slot = bytes[13]; dir.last_active_slot = bytes[14]; dir.include_pins = bytes[15];
        dir.slot_occupied = rd_at<uint16_t>(bytes, 16);
        dir.master_volume_mode = bytes[18] ? 1 : 0;
        dir.master_volume_db = kMasterDefaultDb;
        memcpy(dir.slot_names, bytes + 20, sizeof dir.slot_names);
        dir_valid = 1;
        if (persist) { dir_flush(); if (wrote) *wrote = true; }
        return true;
    }
    return false;      // an unknown later version
}

void Flash::dir_ensure() {      // :440-457
    if (dir_valid) return;
    if (dir_load(true)) return;
    dir = fresh_dir("Default", 0);
    dir_valid = 1;
}

void Flash::dir_flush() {      // :423-436
    dir.magic = kDirMagic; dir.version = kDirVersion; dir.reserved = 0;
    dir.crc32 = flash_crc32(reinterpret_cast<const uint8_t *>(&dir) + kDirHeader, sizeof dir - kDirHeader);
    write_sector(kSectorDir, &dir, sizeof dir);
}

PresetDir Flash::directory() const {
    // (a sector that holds a valid directory is in the cache from the moment the bytes arrived: set_bytes, boot_writes)
    return dir_valid ? dir : fresh_dir("Default", 0);
}

void Flash::set_bytes(const void *dump) {
    memcpy(bytes, dump, sizeof bytes);
    memset(&dir, 0, sizeof dir);
    dir_load(false);
}

bool Flash::boot_writes(int flavor) {      // preset_boot_load, :1047-1102, the flash's side (Params::boot is the parameters')
    bool wrote = false;
    dir_valid = 0;      // power-on: nothing is cached
    if (dir_load(true, &wrote)) {
        uint8_t target = dir.startup_mode == 1 ? dir.last_active_slot : dir.default_slot;
        if (target >= kPresetSlots) { target = dir.default_slot; if (target >= kPresetSlots) target = 0; }
        dir.last_active_slot = target;      // (:1080, the cache only)
        return wrote;
    }
    // migrate_legacy (:997-1045)
    const uint8_t *lg = bytes + (size_t)kSectorLegacy * kFlashSector;
    const size_t lb = legacy_bytes(flavor), sb = slot_bytes(flavor);
    if (rd_at<uint32_t>(lg, 0) == kLegacyMagic && flash_crc32(lg + 12, lb - 12) == rd_at<uint32_t>(lg, 8)) {
        std::vector<uint8_t> slot(sb, 0);
        const uint32_t magic = kSlotMagic; const uint16_t version = rd_at<uint16_t>(lg, 4), idx = 0;
        memcpy(&slot[0], &magic, 4); memcpy(&slot[4], &version, 2); memcpy(&slot[6], &idx, 2);
        memcpy(&slot[12], lg + 12, lb - 12);
        const uint32_t crc = flash_crc32(&slot[12], sb - 12);
        memcpy(&slot[8], &crc, 4);
        write_sector(slot_sector(0), slot.data(), sb);
        dir = fresh_dir("Migrated", 0x0001);
        dir_valid = 1;
        dir_flush();
        return true;
    }
    dir_ensure();      // first boot, no legacy data (:1097-1100)
    dir_flush();
    return true;
}

std::unique_ptr<Flash> Flash::first_boot(int flavor, bool populated, const Params *p) {
    auto f = std::make_unique<Flash>();
    if (!populated) f->boot_writes(flavor); else f->dir_ensure();
    if (p && (f->dir.master_volume_mode != p->dir_master_volume_mode || memcmp(&f->dir.master_volume_db, &p->dir_master_volume_db, 4) != 0)) {
        f->dir.master_volume_mode = p->dir_master_volume_mode; f->dir.master_volume_db = p->dir_master_volume_db;
        if (!populated) f->dir_flush();
    }
    return f;
}

void flash_sync_mirrors(const Flash &f, Params &p) {
    const PresetDir d = f.directory();
    p.dir_master_volume_mode = d.master_volume_mode; p.dir_include_pins = d.include_pins; p.dir_master_volume_db = d.master_volume_db;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the preset API
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
// a sector write inside an operation: flash_write_sector's own re-arm of the mute (:346-348)
void write_and_hold(Flash &f, Params &p, int sector, const void *payload, size_t len) { f.write_sector(sector, payload, len); p.flash_mute(p.flash_hold_samples()); }
void flush_and_hold(Flash &f, Params &p) { f.dir_flush(); p.flash_mute(p.flash_hold_samples()); }
// prepare_flash_write_operation (main.c:553-572)
void prepare_flash_write(Params &p) { p.flash_mute(p.flash_premute_samples()); }

uint8_t save_inner(Flash &f, Params &p, uint8_t slot) {      // preset_save proper (:765-792)
    if (slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;
    f.dir_ensure();
    std::vector<uint8_t> image((size_t)p.slot_size());
    p.save_slot(image.data(), image.size(), slot);           // collect_live_state
    p.flash_mute(p.flash_hold_samples());                    // (:775-776)
    write_and_hold(f, p, slot_sector(slot), image.data(), image.size());
    f.dir.slot_occupied |= (uint16_t)(1u << slot);
    f.dir.last_active_slot = slot;
    flush_and_hold(f, p);
    return PRESET_OK;
}
}  // namespace

uint8_t preset_save(Flash &f, Params &p, uint8_t slot) {
    if (slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;      // (refused by the request itself, usb_audio.c:2698-2700: nothing is deferred)
    prepare_flash_write(p);
    const uint8_t rc = save_inner(f, p, slot);
    flash_sync_mirrors(f, p);
    return rc;
}

uint8_t preset_load(Flash &f, Params &p, uint8_t slot, bool main_loop) {
    if (slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;
    f.dir_ensure();
    flash_sync_mirrors(f, p);      // include_pins and the master-volume mode the slot is applied with are the directory's (:809-810)
    // an occupied slot goes through validate_slot (:750-759: magic, index, CRC — Params::slot_to_live's own test) into the live parameters; a
    // failure drops the mute it armed (:805-808) and leaves the directory alone
    const uint8_t *image = (f.dir.slot_occupied & (1u << slot)) ? f.bytes + (size_t)slot_sector(slot) * kFlashSector : nullptr;
    if (p.preset_apply(image, slot, main_loop) != 0) return PRESET_ERR_CRC;
    f.dir.last_active_slot = slot;      // (:845-846; the mute of this flush is armed inside preset_apply, before the type switch's)
    f.dir_flush();
    return PRESET_OK;
}

uint8_t preset_delete(Flash &f, Params &p, uint8_t slot) {
    if (slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;
    uint8_t old_types[4]; memcpy(old_types, p.output_types, 4);      // main.c:1023-1024
    prepare_flash_write(p);
    f.dir_ensure();
    f.erase_sector(slot_sector(slot));
    p.flash_mute(p.flash_hold_samples());                            // (:874-875)
    f.dir.slot_occupied &= (uint16_t)~(1u << slot);
    memset(f.dir.slot_names[slot], 0, kPresetNameLen);
    flush_and_hold(f, p);
    if (slot == f.dir.last_active_slot) {                            // (:882-904)
        p.preset_deleted_active();
        if (memcmp(old_types, p.output_types, (size_t)p.n_pairs) != 0) p.flash_mute(256);      // process_type_switches, main.c:1038-1048, :279
    }
    p.main_loop_pass();
    flash_sync_mirrors(f, p);
    return PRESET_OK;
}

uint8_t preset_set_name(Flash &f, Params &p, uint8_t slot, const void *payload, size_t len) {
    if (len == 0) return PRESET_OK;      // usb_audio.c:1961: nothing is deferred
    char name[kPresetNameLen];
    memset(name, 0, sizeof name);
    memcpy(name, payload, std::min(len, (size_t)kPresetNameLen - 1));
    prepare_flash_write(p);
    if (slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;      // (:917: after the pre-mute, which stands)
    f.dir_ensure();
    memset(f.dir.slot_names[slot], 0, kPresetNameLen);
    for (int i = 0; i < kPresetNameLen - 1 && name[i]; i++) f.dir.slot_names[slot][i] = name[i];      // strncpy(.., name, PRESET_NAME_LEN - 1): up to the first NUL
    flush_and_hold(f, p);
    flash_sync_mirrors(f, p);
    return PRESET_OK;
}

uint8_t preset_set_startup(Flash &f, Params &p, uint8_t mode, uint8_t default_slot) {
    prepare_flash_write(p);
    if (mode > 1 || default_slot >= kPresetSlots) return PRESET_ERR_INVALID_SLOT;      // (:943-944: silently, the pre-mute stands)
    f.dir_ensure();
    f.dir.startup_mode = mode; f.dir.default_slot = default_slot;
    flush_and_hold(f, p);
    flash_sync_mirrors(f, p);
    return PRESET_OK;
}

void preset_set_include_pins(Flash &f, Params &p, uint8_t include) {
    prepare_flash_write(p);
    f.dir_ensure();
    f.dir.include_pins = include ? 1 : 0;
    flush_and_hold(f, p);
    flash_sync_mirrors(f, p);
}

void preset_set_master_volume_mode(Flash &f, Params &p, uint8_t mode) {
    if (mode > 1) mode = 0;
    prepare_flash_write(p);
    f.dir_ensure();
    f.dir.master_volume_mode = mode;
    flush_and_hold(f, p);
    flash_sync_mirrors(f, p);
}

uint8_t preset_save_master_volume(Flash &f, Params &p) {
    prepare_flash_write(p);
    f.dir_ensure();
    f.dir.master_volume_db = p.master_db;
    flush_and_hold(f, p);
    flash_sync_mirrors(f, p);
    return PRESET_OK;
}

int flash_save_params(Flash &f, Params &p) {
    prepare_flash_write(p);
    f.dir_ensure();
    uint8_t slot = f.dir.last_active_slot;
    if (slot >= kPresetSlots) slot = 0;
    const uint8_t rc = save_inner(f, p, slot);
    flash_sync_mirrors(f, p);
    return rc == PRESET_OK ? FLASH_OK : FLASH_ERR_WRITE;
}

int flash_load_params(Flash &f, Params &p) {
    f.dir_ensure();
    uint8_t slot = f.dir.last_active_slot;
    if (slot >= kPresetSlots) slot = 0;
    const uint8_t rc = preset_load(f, p, slot, false);
    return rc == PRESET_OK ? FLASH_OK : rc == PRESET_ERR_CRC ? FLASH_ERR_CRC : FLASH_ERR_WRITE;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the vendor requests (usb_audio.c:1957-2005 OUT, :2473-2489, :2692-2844 IN)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
enum : uint8_t {
    REQ_SAVE_PARAMS = 0x51, REQ_LOAD_PARAMS = 0x52,
    REQ_PRESET_SAVE = 0x90, REQ_PRESET_LOAD, REQ_PRESET_DELETE, REQ_PRESET_GET_NAME, REQ_PRESET_SET_NAME, REQ_PRESET_GET_DIR, REQ_PRESET_SET_STARTUP,
    REQ_PRESET_GET_STARTUP, REQ_PRESET_SET_INCLUDE_PINS, REQ_PRESET_GET_INCLUDE_PINS, REQ_PRESET_GET_ACTIVE,
    REQ_SET_MASTER_VOLUME_MODE = 0xD4, REQ_SAVE_MASTER_VOLUME = 0xD6,
};
}

bool flash_request_in(uint8_t req) {
    switch (req) {
        case REQ_SAVE_PARAMS: case REQ_LOAD_PARAMS: case REQ_PRESET_SAVE: case REQ_PRESET_LOAD: case REQ_PRESET_DELETE: case REQ_PRESET_GET_NAME:
        case REQ_PRESET_GET_DIR: case REQ_PRESET_GET_STARTUP: case REQ_PRESET_GET_INCLUDE_PINS: case REQ_PRESET_GET_ACTIVE: case REQ_SAVE_MASTER_VOLUME: return true;
        default: return false;
    }
}
bool flash_request_out(uint8_t req) {
    return req == REQ_PRESET_SET_NAME || req == REQ_PRESET_SET_STARTUP || req == REQ_PRESET_SET_INCLUDE_PINS || req == REQ_SET_MASTER_VOLUME_MODE;
}
bool flash_request_writes(uint8_t req) {
    return !(req == REQ_PRESET_GET_NAME || req == REQ_PRESET_GET_DIR || req == REQ_PRESET_GET_STARTUP || req == REQ_PRESET_GET_INCLUDE_PINS || req == REQ_PRESET_GET_ACTIVE);
}

int flash_vendor_read(const Flash &f, uint8_t req, uint16_t wValue, void *buf, uint16_t cap) {
    const uint8_t slot = (uint8_t)wValue;
    uint8_t r[kPresetNameLen];
    int n = 1;
    if (req == REQ_PRESET_GET_NAME) { if (slot >= kPresetSlots) return -14; n = kPresetNameLen; }
    else if (req == REQ_PRESET_GET_DIR) n = 7;
    else if (req == REQ_PRESET_GET_STARTUP) n = 3;
    if (cap < n) return -15;
    const PresetDir d = f.directory();
    switch (req) {
        case REQ_PRESET_GET_NAME: memcpy(r, d.slot_names[slot], kPresetNameLen); break;
        case REQ_PRESET_GET_DIR:
            r[0] = (uint8_t)(d.slot_occupied & 0xFF); r[1] = (uint8_t)(d.slot_occupied >> 8); r[2] = d.startup_mode; r[3] = d.default_slot;
            r[4] = d.last_active_slot; r[5] = d.include_pins; r[6] = d.master_volume_mode;
            break;
        case REQ_PRESET_GET_STARTUP: r[0] = d.startup_mode; r[1] = d.default_slot; r[2] = d.last_active_slot; break;
        case REQ_PRESET_GET_INCLUDE_PINS: r[0] = d.include_pins; break;
        case REQ_PRESET_GET_ACTIVE: r[0] = d.last_active_slot; break;
        default: return -14;
    }
    memcpy(buf, r, (size_t)n);
    return n;
}

int flash_vendor_get(Flash &f, Params &p, uint8_t req, uint16_t wValue, void *buf, uint16_t cap) {
    if (!flash_request_writes(req)) return flash_vendor_read(f, req, wValue, buf, cap);
    const uint8_t slot = (uint8_t)wValue;
    uint8_t r[1];
    const int n = 1;
    if (cap < n) return -15;
    switch (req) {
        case REQ_SAVE_PARAMS: flash_save_params(f, p); r[0] = FLASH_OK; break;                           // "accepted" (usb_audio.c:2473-2480)
        case REQ_LOAD_PARAMS: r[0] = (uint8_t)flash_load_params(f, p); break;                            // the result itself (:2482-2489)
        case REQ_PRESET_SAVE: r[0] = slot >= kPresetSlots ? PRESET_ERR_INVALID_SLOT : PRESET_OK; if (slot < kPresetSlots) preset_save(f, p, slot); break;
        case REQ_PRESET_LOAD: r[0] = slot >= kPresetSlots ? PRESET_ERR_INVALID_SLOT : PRESET_OK; if (slot < kPresetSlots) preset_load(f, p, slot, true); break;
        case REQ_PRESET_DELETE: r[0] = slot >= kPresetSlots ? PRESET_ERR_INVALID_SLOT : PRESET_OK; if (slot < kPresetSlots) preset_delete(f, p, slot); break;
        case REQ_SAVE_MASTER_VOLUME: preset_save_master_volume(f, p); r[0] = PRESET_OK; break;
        default: return -14;
    }
    memcpy(buf, r, (size_t)n);
    return n;
}

int flash_vendor_set(Flash &f, Params &p, uint8_t req, uint16_t wValue, const void *payload, uint16_t len) {
    if (len == 0 || len > 64) return -14;      // no data stage / more than vendor_rx_buf holds: the setup packet stalls (usb_audio.c:2260-2264)
    const uint8_t *b = static_cast<const uint8_t *>(payload);
    switch (req) {
        case REQ_PRESET_SET_NAME: preset_set_name(f, p, (uint8_t)(wValue & 0xFF), b, len); return 0;
        case REQ_PRESET_SET_STARTUP: if (len >= 2) preset_set_startup(f, p, b[0], b[1]); return 0;
        case REQ_PRESET_SET_INCLUDE_PINS: preset_set_include_pins(f, p, b[0]); return 0;
        case REQ_SET_MASTER_VOLUME_MODE: preset_set_master_volume_mode(f, p, b[0]); return 0;
        default: return -14;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the book
// ---------------------------------------------------------------------------------------------------------------------------------
int32_t FlashBook::add(std::unique_ptr<Flash> f) {
    if (!free_slots.empty()) {
        const int32_t k = free_slots.back(); free_slots.pop_back();
        objects[(size_t)k] = std::move(f); refs[(size_t)k] = 0;
        return k;
    }
    objects.push_back(std::move(f)); refs.push_back(0);
    return (int32_t)objects.size() - 1;
}

void FlashBook::release(int32_t obj) {
    if (obj < 0) return;
    if (--refs[(size_t)obj] == 0) { objects[(size_t)obj].reset(); free_slots.push_back(obj); }
}

void FlashBook::assign(uint32_t s, int32_t obj) {
    refs[(size_t)obj]++;      // (first: assigning a stream its own object must not free it)
    release(index[s]);
    index[s] = obj;
}

Flash *FlashBook::writable(uint32_t s) {
    const int32_t k = index[s];
    if (refs[(size_t)k] > 1) assign(s, add(std::make_unique<Flash>(*objects[(size_t)k])));
    return objects[(size_t)index[s]].get();
}

size_t FlashBook::distinct() const {
    size_t n = 0;
    for (const auto &o : objects) if (o) n++;
    return n;
}

void FlashBook::move(const StreamMove *moves, uint32_t n) {
    std::vector<int32_t> from(n);
    for (uint32_t i = 0; i < n; i++) { from[i] = index[moves[i].src]; refs[(size_t)from[i]]++; }      // all sources are read (and held) before any destination is written
    for (uint32_t i = 0; i < n; i++) { release(index[moves[i].dst]); index[moves[i].dst] = from[i]; }
}

void FlashBook::arrive(const FlashBook &from, const StreamMove *moves, uint32_t n) {
    std::map<int32_t, int32_t> copy;      // the source's object -> its copy here
    for (uint32_t i = 0; i < n; i++) {
        const int32_t k = from.index[moves[i].src];
        auto it = copy.find(k);
        if (it == copy.end()) it = copy.emplace(k, add(std::make_unique<Flash>(*from.objects[(size_t)k]))).first;
        assign(moves[i].dst, it->second);
    }
}

void FlashBook::boot(const uint32_t *streams, uint32_t n, int32_t obj) {
    for (uint32_t i = 0; i < n; i++) assign(streams[i], obj);
}

void FlashBook::resize(uint32_t n_new, int32_t obj) {
    const uint32_t n_old = (uint32_t)index.size();
    for (uint32_t s = n_new; s < n_old; s++) release(index[s]);
    index.resize(n_new, -1);
    for (uint32_t s = n_old; s < n_new; s++) assign(s, obj);
}

std::vector<FlashPair> flash_pairs(const std::vector<int32_t> &stream_image, const std::vector<int32_t> &stream_flash, std::vector<uint32_t> *pair_of_stream) {
    std::map<std::pair<int32_t, int32_t>, uint32_t> seen;
    std::vector<FlashPair> out;
    if (pair_of_stream) pair_of_stream->resize(stream_image.size());
    for (uint32_t s = 0; s < (uint32_t)stream_image.size(); s++) {
        const auto it = seen.emplace(std::make_pair(stream_image[s], stream_flash[s]), (uint32_t)out.size());
        if (it.second) out.push_back(FlashPair{stream_image[s], stream_flash[s], s});
        if (pair_of_stream) (*pair_of_stream)[s] = it.first->second;
    }
    return out;
}

}  // namespace dspi
