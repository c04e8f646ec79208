// dspi_flash.h — a stream's own flash (dspi_device_flash, include/dspi.h): the 48 KB preset area of one DSPi device as bytes, the preset
// directory requests of the firmware over it, and the context's book of who holds which flash.  Plain C++ (no HIP, no kernel): dspi_capi.cpp
// includes it, tests/flash_driver.cpp exercises it without a GPU.
//
// The area (DSPI_FLASH_DUMP_BYTES, flash_storage.c:4-15, :50-58): sector 0 the preset directory, sectors 1..10 the ten preset slots, sector 11
// the legacy sector.  A sector WRITE leaves the payload followed by 0xFF to the end of the sector (flash_write_sector, :315-357: erase, then
// program the page-rounded buffer, which is 0xFF behind the payload); an ERASE leaves 0xFF.
//
// The directory the requests see is the firmware's dir_cache (:261-264): read from sector 0 when the device boots or when the bytes are
// replaced (dspi_flash_write), validated (magic, version, CRC-32 over everything after the 12-byte header), a version 1 converted; where the
// sector holds none it is dir_ensure's fresh one (:440-457), which reaches the flash with the next flush.  Every change goes through
// dir_flush, so between two requests the cache and a valid sector differ only where the firmware's do: in last_active_slot after a boot
// (preset_boot_load sets it without a flush, :1080).  Nothing of the directory lives in Params: its three mirrors there
// (dir_master_volume_mode, dir_include_pins, dir_master_volume_db) are set from the directory after every operation (flash_sync_mirrors).
//
// Cost: one Flash is 48 KB + 346 bytes of host memory, and the book holds one per DISTINCT flash: streams share an object until one of them
// writes (clone on write, as the parameter objects do).  65 536 distinct flashes are 3.2 GB.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "dspi_move.h"
#include "dspi_params.h"

namespace dspi {

constexpr size_t kFlashSector = 4096;
constexpr int kPresetSlots = 10, kPresetNameLen = 32;      // config.h:254-255
constexpr int kSectorDir = 0, kSectorLegacy = 11;
constexpr int slot_sector(int slot) { return 1 + slot; }
enum : uint8_t { PRESET_OK = 0, PRESET_ERR_INVALID_SLOT = 1, PRESET_ERR_SLOT_EMPTY = 2, PRESET_ERR_CRC = 3, PRESET_ERR_FLASH_WRITE = 4 };      // config.h:262-266
enum : uint8_t { FLASH_OK = 0, FLASH_ERR_WRITE = 1, FLASH_ERR_NO_DATA = 2, FLASH_ERR_CRC = 3 };                                              // flash_storage.h:9-12

#pragma pack(push, 1)
struct PresetDir {      // == PresetDirectory (version 2), flash_storage.c:113-131
    uint32_t magic;
    uint16_t version, reserved;
    uint32_t crc32;
    uint8_t startup_mode, default_slot, last_active_slot, include_pins;
    uint16_t slot_occupied;
    uint8_t master_volume_mode, padding;
    float master_volume_db;
    char slot_names[kPresetSlots][kPresetNameLen];
};
#pragma pack(pop)
static_assert(sizeof(PresetDir) == 344, "PresetDirectory is 344 bytes");

uint32_t flash_crc32(const uint8_t *d, size_t n);      // flash_storage.c:282-291

struct Flash {
    uint8_t bytes[kFlashDumpBytes];
    PresetDir dir;            // dir_cache
    uint8_t dir_valid;        // dir_cache_valid

    Flash() { erase_all(); }
    void erase_all();                                               // a flash nothing was ever written to; no directory cached
    void erase_sector(int sector);
    void write_sector(int sector, const void *payload, size_t len);
    // dir_load_cache (:370-419).  persist: a version 1 directory is flushed as version 2 (a boot does; dspi_flash_write does not).
    // Returns whether the sector held a valid directory; *wrote says whether the flash was written.
    bool dir_load(bool persist, bool *wrote = nullptr);
    void dir_ensure();                                              // :440-457
    void dir_flush();                                               // :423-436
    PresetDir directory() const;                                    // what a GET request sees: the cache, or dir_ensure's fresh one
    void set_bytes(const void *dump);                               // dspi_flash_write: the bytes replaced, the cache read again, nothing written
    // the writes of a power-on over these bytes (preset_boot_load, :1047-1102): a version 1 directory persisted as version 2; without a
    // directory the legacy sector migrated into slot 0 (migrate_legacy, :997-1045) or a fresh directory flushed; last_active_slot of the
    // cache set to the selected slot.  Returns whether anything was written.
    bool boot_writes(int flavor);
    // the flash a device's first boot leaves (an erased area, then boot_writes) — or, `populated`, an erased area whose fresh directory
    // stands in the cache only —, with the mirrored master-volume mode and saved master volume of `p` (may be nullptr) in the directory.
    // include_pins is dir_ensure's 1 whatever `p` says: a parameter object's mirror of it is 0 until a directory has been loaded into it,
    // which is how the library models "no directory" without the mode, not a setting of the device; the caller syncs the mirror afterwards.
    static std::unique_ptr<Flash> first_boot(int flavor, bool populated, const Params *p);
};

void flash_sync_mirrors(const Flash &f, Params &p);

// ---- the preset API over (flash, parameters): each call is the request AND the main-loop pass that serves it, so the pipeline mute that
// stands afterwards is the one the firmware leaves: flash_mute_hold_samples() after a sector write (:347-348), PRESET_MUTE_SAMPLES after
// the delete of the active slot (:884) or a type switch (main.c:279), the pre-mute of prepare_flash_write_operation (main.c:553-572: 120 ms,
// at least PRESET_MUTE_SAMPLES) where a deferred setter was refused before it wrote.  The 30 ms settle wait of that function passes no audio.
uint8_t preset_save(Flash &f, Params &p, uint8_t slot);                                      // :765-792 under main.c:992-1007
uint8_t preset_load(Flash &f, Params &p, uint8_t slot, bool main_loop);                      // :794-849 under main.c:926-976 (main_loop) or inside REQ_LOAD_PARAMS
uint8_t preset_delete(Flash &f, Params &p, uint8_t slot);                                    // :851-907 under main.c:1009-1052
uint8_t preset_set_name(Flash &f, Params &p, uint8_t slot, const void *payload, size_t len); // usb_audio.c:1957-1971, main.c:749-767, :916-928
uint8_t preset_set_startup(Flash &f, Params &p, uint8_t mode, uint8_t default_slot);         // :942-953 under main.c:769-786
void preset_set_include_pins(Flash &f, Params &p, uint8_t include);                          // :955-959 under main.c:788-799
void preset_set_master_volume_mode(Flash &f, Params &p, uint8_t mode);                       // :961-966 under main.c:801-812
uint8_t preset_save_master_volume(Flash &f, Params &p);                                      // :972-977 under main.c:814-822
int flash_save_params(Flash &f, Params &p);                                                  // :1108-1124 under main.c:978-990
int flash_load_params(Flash &f, Params &p);                                                  // :1126-1140, inside the request (usb_audio.c:2482-2489)

// the vendor requests served from the flash.  flash_request_in / _out: is `req` one of them, in that direction?  The two calls answer like
// Params::vendor_get / vendor_set: bytes written (IN), 0 (OUT), -14 for a stall, -15 for a buffer that is too small (checked before anything
// is written).  flash_request_writes: false for the getters, which neither write the flash nor change the parameters.
bool flash_request_in(uint8_t req);
bool flash_request_out(uint8_t req);
bool flash_request_writes(uint8_t req);
int flash_vendor_read(const Flash &f, uint8_t req, uint16_t wValue, void *buf, uint16_t cap);      // the getters
int flash_vendor_get(Flash &f, Params &p, uint8_t req, uint16_t wValue, void *buf, uint16_t cap);
int flash_vendor_set(Flash &f, Params &p, uint8_t req, uint16_t wValue, const void *payload, uint16_t len);

// ---- the book: refcounted flash objects and one index per stream, kept like the parameter objects' (add_image, image_refs, writable).
// An object that loses its last reference is freed at once and its slot reused.  One entry point per maintenance call.
struct FlashBook {
    bool on = false;
    std::vector<std::unique_ptr<Flash>> objects;
    std::vector<uint32_t> refs;
    std::vector<int32_t> index;      // [n_streams] while on

    void enable(uint32_t n_streams) { on = true; index.assign(n_streams, -1); }
    void drop() { on = false; objects.clear(); refs.clear(); index.clear(); free_slots.clear(); }
    int32_t add(std::unique_ptr<Flash> f);                    // an object nobody holds yet; it must be assigned before the call ends
    void assign(uint32_t s, int32_t obj);
    const Flash &readable(uint32_t s) const { return *objects[(size_t)index[s]]; }
    Flash *writable(uint32_t s);                              // clone on write
    size_t distinct() const;                                  // live objects
    // dspi_move_streams (a validated list): index[dst] := old index[src] for all entries at once; a source that is no destination (an
    // open end) keeps its reference, a destination that is no source loses its occupant's
    void move(const StreamMove *moves, uint32_t n);
    // dspi_migrate_streams, the destination's side: the flashes arrive BY VALUE from a source whose mode is on, each distinct object among
    // the listed sources copied once.  (From a source without the mode the context gives the arrivals first-boot flashes: add + assign.)
    // The source's side is leave(): its slots stay behind as frozen copies and KEEP their references, as they keep their parameter
    // objects — the entry point exists so that the rule stands in one place and is tested.
    void arrive(const FlashBook &from, const StreamMove *moves, uint32_t n);
    void leave(const StreamMove *moves, uint32_t n) { (void)moves; (void)n; }
    // dspi_boot_streams: the listed slots hold `obj`
    void boot(const uint32_t *streams, uint32_t n, int32_t obj);
    // dspi_resize_streams: a shrink releases the cut slots' references, a grow gives the new slots `obj` (unused on a shrink)
    void resize(uint32_t n_new, int32_t obj);

private:
    std::vector<int32_t> free_slots;
    void release(int32_t obj);
};

// a broadcast request: the distinct (parameter object, flash object) pairs among the streams in order of their first stream, and (optional)
// each stream's pair.  The context applies the request once per pair, after giving a parameter object that stands in several pairs a clone
// per further pair and a flash object likewise, so that streams that shared both keep sharing both.
struct FlashPair { int32_t image, flash; uint32_t first_stream; };
std::vector<FlashPair> flash_pairs(const std::vector<int32_t> &stream_image, const std::vector<int32_t> &stream_flash, std::vector<uint32_t> *pair_of_stream = nullptr);

}  // namespace dspi
