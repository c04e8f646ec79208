/*
 * dspi.h — C-ABI of libdspi_mi355x: the DSPi per-sample DSP chain on AMD Instinct MI355X.
 *
 * Drop-in boundary.  The reference firmware exposes no plugin/FFI interface: its chain is the
 * static function process_audio_packet(const uint8_t *data, uint16_t data_len)
 * (firmware/DSPi/usb_audio.c:500) reading ~40 file-scope globals that the USB control plane
 * writes.  What is frozen here is therefore the firmware's DATA interface:
 *
 *   audio in        interleaved little-endian stereo PCM, 16-bit or packed 24-bit, in packets
 *                   of block_len frames                 usb_audio.c:528-530, :591-686, :997-1015
 *   audio out       per S/PDIF pair int32 L,R words carrying a 24-bit sample; PDM sub as int32 Q28
 *                                                        usb_audio.c:926-955, :1244-1271
 *   whole state     WireBulkParams (2896 B, v2..v6)      bulk_params.h:42-205, bulk_params.c:178-377
 *                   PresetSlot v<=12 (+CRC-32)           flash_storage.c:136-189, :597-742
 *   parameters      EP0 vendor requests bRequest/wValue/payload
 *                                                        config.h:111-251, usb_audio.c:1632-2021 (SET), :2241-2688 (GET)
 *   UAC1 controls   volume (1/256 dB), mute, sample rate usb_audio.c:428-440, :1477-1499
 *   status          REQ_GET_STATUS wValue 9 byte layout  usb_audio.c:2427-2443
 *
 * One context drives `n_streams` independent DSPi devices ("streams") on one GPU.  Every
 * stream owns its filter state, delay lines and meters; parameters live in images shared by
 * any number of streams (all streams start on one image = factory defaults).
 *
 * Numerics: DSPI_FLAVOR_RP2040_Q28 is bit-exact integer arithmetic; DSPI_FLAVOR_RP2350_F32
 * is IEEE binary32 with flush-to-zero, either with no contraction or (DSPI_FLOAT_CONTRACT_FMA) with
 * exactly the fused multiply-adds GCC gives the firmware.  All match oracle/ bit-for-bit (tests/).
 * ONE boundary is defined by this repository rather than by the reference: the leveller calls
 * log10f once and powf twice per packet (leveller.c:178, :200, :206), the firmware links them from
 * an unpinned newlib / pico-float, and no libm agrees with another in the last bit.  The definition
 * here is one anyone can reproduce: the IEEE-754 CORRECTLY ROUNDED binary32 value (round to nearest,
 * ties to even) of log10(x) and of a^b — for every binary32 argument of log10f and of 10^y, and for
 * a^count on the firmware's eighteen smoothing coefficients (leveller.c:37-89) with count 1..192,
 * which are all the calls the leveller makes (results above e^88 clamp there, below e^-103 flush to 0).
 * include/dspi_detmath.h computes it (binary64 with a proven bound, double-double where the bound does
 * not decide; the kernels: the same floats through exception tables from an exhaustive walk,
 * include/dspi_detmath_tables.h); tests compare it with binary128 (libquadmath): 0 mismatches over
 * 10^7 arguments per function and over every argument the first step does not prove.  The product
 * and the oracle both use it, and the reference build used for pinning is compiled with
 * oracle/ref_math_hook.h (-include), which routes leveller.c's log10f / powf to the same header — the
 * reference build is MODIFIED at exactly this boundary and nowhere else.  glibc's own log10f / powf
 * differ from the correctly rounded value in ~2 % of calls, by at most 2 ulp; one golden vector
 * crosses the boundary: tests/golden/f32_full_96k_libm.npz (the reference with glibc's own libm,
 * BASELINE config 3's preset) is reproduced word for word by the oracle and by the GPU.
 * The float-to-int casts saturate as on both MCUs (vcvt.s32.f32 / the RP2040 bootrom's
 * float2int_z); an x86 build of the same C gives INT_MIN instead — for Q28 the one place this
 * shows in normal operation is the limiter quotient (leveller.c:376), where "bit-exact" rests on
 * that restated rule, not on executed reference code.
 *
 * Threading: a context is single-threaded.  Parameter calls take effect at the next
 * dspi_process() (= at a packet boundary, as in the firmware's main loop, main.c:826-894).
 * All functions return 0 / a non-negative count on success or a negative DSPI_E_* code; no
 * exceptions cross the boundary.
 */
#ifndef DSPI_H
#define DSPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSPI_ABI_VERSION 8   /* 2: DSPI_OUT_TILED, dspi_tile_streams, dspi_pdm_*, dspi_spdif_encode; 3: DSPI_FLOAT_CONTRACT_FMA,
                              * dspi_debug_eq_taps; 4: dspi_i2s_encode, vendor requests 0xC0 / 0xC1,
                              * dspi_debug_launch_plan, dspi_debug_image_count; 5: DSPI_OUT_ENABLED_ONLY, DSPI_OUT_I2S_SLOTS, DSPI_BOOT_POPULATED_FLASH, dspi_debug_launch_plan counts[5];
                              * 6: DSPI_OUT_SPDIF, dspi_spdif_block_pos; 7: dspi_out.clip_flags behind DSPI_OUT_CLIP_FLAGS, DSPI_OUT_SPDIF on every
                              * context, (additions only: a v6 caller's three-member dspi_out is never read past `peaks`);
                              * 8: dspi_debug_direct_stats, dspi_debug_detmath, the direct path polls a completion word for the call's own audio time (DSPI_DIRECT_SPIN_US, DSPI_DIRECT_POLL);
                              * 8 + snapshots: detect by symbol (dspi_snapshot_sizes, dspi_export_streams, dspi_import_streams; additions only);
                              * 8 + realignment: detect by symbol (dspi_realign_streams; with it DSPI_SNAP_REALIGN and dspi_debug_stream_positions; additions only);
                              * 8 + paused streams: detect by symbol (dspi_pause_streams; with it dspi_resume_streams, dspi_streams_paused, DSPI_RESUME_AS_IS; additions only);
                              * 8 + stream moves: detect by symbol (dspi_move_streams; with it dspi_plan_compaction, dspi_stream_move, DSPI_MOVE_AS_IS, DSPI_COMPACT_ONE_WAY; additions only);
                              * 8 + stream boots: detect by symbol (dspi_boot_streams; with it DSPI_BOOT_STREAMS_AS_IS; additions only);
                              * 8 + per-stream S/PDIF positions: detect by symbol (dspi_spdif_per_stream; with it dspi_spdif_stream_pos, dspi_spdif_encode_v; additions only);
                              * 8 + resizing: detect by symbol (dspi_resize_streams; with it dspi_reserve_streams, dspi_stream_capacity, DSPI_RESIZE_PAUSED; additions only);
                              * 8 + grouping: detect by symbol (dspi_plan_grouping; with it DSPI_GROUP_ONE_WAY; additions only);
                              * 8 + PDM words from the call: detect by symbol (dspi_process_pdm; with it dspi_pdm_running; additions only);
                              * 8 + mixed input formats: detect by symbol (dspi_process_mixed; with it dspi_mixed_pcm_bytes; additions only);
                              * 8 + wire words per device: detect by symbol (dspi_process_wire; with it dspi_wire_encode; additions only);
                              * 8 + a stream's own flash: detect by symbol (dspi_device_flash; with it dspi_flash_read, dspi_flash_write, DSPI_BOOT_STREAMS_OWN_FLASH; additions only);
                              * 8 + wire words on tiled and mixed-depth contexts: detect by symbol (dspi_process_devices; with it dspi_wire_encode_tiled; additions only);
                              * 8 + S/PDIF input: detect by symbol (dspi_process_sources; with it dspi_spdif_decode, dspi_sources_bytes, dspi_spdif_rx, DSPI_SRC_*, DSPI_OUT_WIRE; additions only);
                              * 8 + chained devices: detect by symbol (dspi_process_linked; with it dspi_wire_decode, dspi_wire_view_of, dspi_link_kinds, dspi_wire_view, dspi_link, DSPI_LINK_*; additions only);
                              * 8 + the patch bay: detect by symbol (dspi_process_patched; with it dspi_patched_bytes, dspi_patch, DSPI_SRC_LINK, DSPI_MAX_VIEWS; additions only);
                              * 8 + the meter bridge: detect by symbol (dspi_meters_update; with it dspi_meters_alarms, dspi_status_all, dspi_clear_clips_list; additions only);
                              * 8 + input from a packet table: detect by symbol (dspi_process_packets; with it dspi_packets_check; additions only)
                              * 8 + resident packet tables: detect by symbol (dspi_process_packets_resident; with it the three other _resident
                              *   calls; additions only) */

/* flavours: values equal the firmware's platform ids (config.h:269-270) */
#define DSPI_FLAVOR_RP2040_Q28 0   /* 7 channels, 5 outputs, int32 Q28, 2048-sample delay lines */
#define DSPI_FLAVOR_RP2350_F32 1   /* 11 channels, 9 outputs, float, 4096-sample delay lines   */
/* OR into the flavour of dspi_create: the float flavour AS THE FIRMWARE IS BUILT.  firmware/DSPi/CMakeLists.txt:6-11 sets only
 * -O2/-O3, so GNU C's default -ffp-contract=fast applies and, the Cortex-M33 having vfma, GCC fuses a*b + c into one
 * rounding wherever its contraction pass pairs them: biquad / SVF recurrences (dsp_pipeline.c:298-362), loudness shelves
 * (usb_audio.c:697-712), matrix mix (:766), leveller envelope and smoother (leveller.c:165-166, :200), crossfeed
 * (crossfeed.c:137-148) and the coefficient design functions.  Without the flag every multiply and add rounds on its own
 * (the source read literally, -ffp-contract=off).  Both contracts are pinned bit-for-bit to the reference compiled the
 * corresponding way (oracle/Makefile, tests/test_oracle_vs_fw.py); the fused one needs a third fewer vector instructions.
 * PRECISELY what this contract is: "GCC 11, x86-64, -ffp-contract=fast -mfma with the vectorisers off: the GIMPLE-level contraction of
 * the same source" — not "the Cortex-M33 binary".  That arm-none-eabi-gcc fuses the same pairs is read off GCC's target-independent
 * tree pass (the .FMA / .FMS / .FNMA calls of -fdump-tree-optimized, listed in DESIGN.md section 5), not executed: the image has no ARM
 * toolchain.  What north_star asks of the two contracts — within 1 ULP per stage of each other — is measured (profiles/r02_ulp_per_stage.md). */
#define DSPI_FLOAT_CONTRACT_FMA 0x100
#define DSPI_FLAVOR_RP2350_F32_FMA (DSPI_FLAVOR_RP2350_F32 | DSPI_FLOAT_CONTRACT_FMA)
/* OR into the flavour of dspi_create: what the power-on models.  By default every stream is a device that boots for the FIRST time on an
 * erased flash: preset_boot_load writes the fresh preset directory (flash_storage.c:1097-1100), and every flash sector write arms the
 * preset mute for flash_mute_hold_samples() = max(10 ms, 512) samples (:272-276, :347-348) — so a new context starts with 512 muted
 * samples and the fade-in (5 to 12 ms of silence / ramp at the start of the first packets).  With DSPI_BOOT_POPULATED_FLASH the streams
 * are devices whose flash already holds a directory: nothing is written at boot, audio starts unmuted; load the preset such a device
 * would have booted with dspi_load_flash_dump BEFORE the first dspi_process: on such a context that call IS the boot — the power-on
 * sequence runs again over the dump (preset_boot_load -> apply_slot_to_live, flash_storage.c:1047-1082: the selected slot goes into
 * the live parameters, no mute is armed, no line is zeroed; a boot that itself writes the flash — no directory, a legacy sector to
 * migrate, a v1 directory to convert — arms the 512-sample mute like a first boot; slots saved as I2S arm the type-switch mute,
 * main.c:651-684), and the sample rate, UAC1 volume and mute set since dspi_create are set again after it.  Exact against the firmware
 * build booted from the same flash FROM FRAME 0 (tests/test_gpu_parity.py::test_flash_dump_boots_device_context,
 * tests/test_oracle_vs_fw.py::test_boot_from_flash_dumps).  Once a context has processed audio — and on every context without the
 * flag — dspi_load_flash_dump is a running device switching to the preset the dump selects (preset_load, flash_storage.c:794-849:
 * max(10 ms, 512)-sample mute, delay lines zeroed), exactly like dspi_load_preset_slot. */
#define DSPI_BOOT_POPULATED_FLASH 0x200

#define DSPI_ALL_STREAMS (-1)
#define DSPI_DEVICE_NONE (-1)      /* host-only context: parameter surface works, dspi_process fails */
#define DSPI_MAX_BLOCK_LEN 192     /* usb_audio.c:273-276, :588 */

/* error codes */
#define DSPI_OK 0
#define DSPI_E_INVAL (-10)         /* bad argument */
#define DSPI_E_NODEVICE (-11)      /* HIP runtime / GPU unavailable or host-only context */
#define DSPI_E_NOMEM (-12)
#define DSPI_E_HIP (-13)           /* a HIP call failed; see dspi_last_error() */
#define DSPI_E_UNSUPPORTED (-14)   /* vendor request outside the DSP subset (USB stall in the firmware) */
#define DSPI_E_SHORT (-15)         /* output buffer too small */
/* dspi_load_bulk returns the firmware's own codes: -1 version, -2 platform, -3 channel counts, -4 length */
/* dspi_load_preset_slot returns PRESET_OK (0) or PRESET_ERR_CRC (3)  (config.h:262-266) */

/* dspi_process flags.  Bits not defined here are refused (DSPI_E_INVAL), never ignored: a later ABI may give a bit a meaning that
 * reads further members of dspi_out (as DSPI_OUT_CLIP_FLAGS did in ABI 7). */
#define DSPI_MEM_DEVICE 0x1u       /* pcm_in and every pointer in dspi_out are device pointers (zero-copy) */
#define DSPI_OUT_TILED 0x2u        /* pairs / sub use the device-native tiled layout described at dspi_out */
#define DSPI_OUT_I2S_SLOTS 0x8u    /* pairs whose slot is an I2S slot in the stream's own parameters (output_types[], REQ_SET_OUTPUT_TYPE 0xC0) are written as
                                    * the words the I2S driver shifts out — the S/PDIF producer word left-justified, word << 8
                                    * (pico_audio_i2s_multi/audio_i2s_multi.c:217-226) — instead of going through dspi_i2s_encode afterwards: the same
                                    * words, without the second pass over 64 bytes per frame.  S/PDIF-typed pairs are unaffected. */
#define DSPI_OUT_SPDIF 0x10u       /* `pairs` takes what the S/PDIF driver shifts out instead of the producer words: per frame and pair the two IEC 60958
                                    * subframes of spdif_update_subframe (pico_audio_spdif_multi, sample_encoding.h:27-47; dspi_spdif_encode below) —
                                    *   pairs  uint32 [stream][pair][F][4]   {left lo, left hi, right lo, right hi}: TWICE the bytes of the word layout —
                                    * the words dspi_process + dspi_spdif_encode give, without the second pass (8 bytes in, 16 out per frame and pair).
                                    * The position in the 192-frame channel-status block runs on from call to call (dspi_spdif_block_pos); the
                                    * sample-rate byte of the channel status is each stream's own rate (audio_spdif.c:250-256).  On EVERY context:
                                    * where the float chain's latency layout serves the launch (small contexts) its output waves encode the
                                    * subframes themselves; on every other launch the library runs the chain into a scratch buffer of pair words,
                                    * row chunk by row chunk, and the subframe encoder from there (on the packed kernel the fused encoder would
                                    * cost the chain 60 % more instructions).  Not with DSPI_OUT_TILED or DSPI_OUT_I2S_SLOTS. */
#define DSPI_OUT_ENABLED_ONLY 0x4u /* the caller does not read the sample words of SILENT outputs — an S/PDIF pair whose two outputs are
                                    * disabled (the firmware zero-fills it, usb_audio.c:930-933), the sub while it is disabled or Core 1
                                    * runs the EQ worker — so the library may leave those parts of pairs / sub unwritten instead of storing
                                    * zeros (36 of the 40 bytes per frame for a preset with one live pair).  Peaks, status and every live
                                    * output are unaffected.  Honoured by the float chain's latency layout; the other kernels write the zeros
                                    * (host buffers: the silent parts come back as zeros either way).  With DSPI_OUT_SPDIF: where the library
                                    * serves the call in two passes (any lane off the latency layout) the silent pairs carry the subframes of
                                    * SILENCE, exactly as without this flag; where the latency layout's output waves encode the subframes
                                    * themselves the silent pairs are left unwritten (host buffers: zero words, which are not valid subframes —
                                    * do not shift them out). */
#define DSPI_OUT_CLIP_FLAGS 0x20u  /* the dspi_out passed has the ABI-7 member clip_flags (below) and the library may write through it */

typedef struct dspi_ctx dspi_ctx;

/* Output buffers, all optional (NULL = not produced).  Layouts, F = n_blocks*block_len frames:
 *   pairs      int32 [stream][pair][F][2]   pair p = outputs 2p,2p+1; 24-bit sample per word
 *   sub        int32 [stream][F]            PDM sub channel, Q28 (zeros when the firmware would push nothing)
 *   peaks      uint16 [stream][block][C]    per-packet peak meters (global_status.peaks, config.h:455-460)
 *   clip_flags uint16 [stream]              sticky clip bits (with DSPI_OUT_CLIP_FLAGS only, see the member)
 * where C = 11 / 7 channels and pair count = 4 / 2.
 *
 * With DSPI_OUT_TILED the sample words are stream-minor instead ("tiles" of R = dspi_tile_streams() consecutive
 * streams, 128 float / 64 Q28; tile = stream / R, column = stream % R):
 *   pairs      int32 [tile][output][F][R]   output o = 0 .. 2*pairs-1 (pair o/2, side o%2), same 24-bit words
 *   sub        int32 [tile][F][R]
 * Buffers cover whole tiles (ceil(n_streams / R) of them); columns past n_streams are never written.
 * This is how the kernel produces the samples (one 512-byte row per frame per output, like its delay lines): the
 * layout for a GPU-resident consumer.  The stream-major layout above is the per-device view (one S/PDIF pair buffer
 * per stream) and costs scattered 4-byte writes. */
typedef struct dspi_out {
    int32_t *pairs;
    int32_t *sub;
    uint16_t *peaks;
    uint16_t *clip_flags;  /* ABI 7, read ONLY when flags carry DSPI_OUT_CLIP_FLAGS: uint16 [stream], every stream's sticky clip bits after the
                            * call's last packet — global_status.clip_flags as REQ_GET_STATUS reports them (usb_audio.c:2427-2443: bit c =
                            * channel c's peak exceeded full scale since the last REQ_CLEAR_CLIPS) — one pass instead of a dspi_get_status
                            * per stream.  Not cleared by reading. */
} dspi_out;

/* ---- lifecycle ---------------------------------------------------------------------- */
int dspi_create(dspi_ctx **out, int flavor, uint32_t n_streams, int hip_device);
void dspi_destroy(dspi_ctx *ctx);
const char *dspi_last_error(const dspi_ctx *ctx);
int dspi_abi_version(void);
int dspi_num_channels(const dspi_ctx *ctx);   /* 11 / 7 */
int dspi_num_outputs(const dspi_ctx *ctx);    /* 9 / 5  */
int dspi_num_pairs(const dspi_ctx *ctx);      /* 4 / 2  */
uint32_t dspi_num_streams(const dspi_ctx *ctx);
uint32_t dspi_tile_streams(const dspi_ctx *ctx);   /* R of the tiled layouts: 128 / 64 */

/* ---- whole-state blobs ---------------------------------------------------------------- */
/* REQ_FACTORY_RESET / loading an empty preset slot: flash_storage.c:1144-1238, :811-833 */
int dspi_factory_defaults(dspi_ctx *ctx, int32_t stream);
/* REQ_SET_ALL_PARAMS: main.c:1126-1162 + bulk_params.c:178-377 */
int dspi_load_bulk(dspi_ctx *ctx, int32_t stream, const void *blob, size_t len);
/* REQ_GET_ALL_PARAMS: bulk_params.c:62-172.  Returns 2896. */
int dspi_collect_bulk(dspi_ctx *ctx, int32_t stream, void *blob, size_t cap);
/* REQ_PRESET_LOAD of an occupied slot: main.c:926-976, flash_storage.c:750-849.
 * `expect_slot` = slot number the image must carry (validate_slot), or -1 to accept any. */
int dspi_load_preset_slot(dspi_ctx *ctx, int32_t stream, const void *image, size_t len, int expect_slot);
/* collect_live_state: flash_storage.c:464-552.  Returns the image size (2864 / 1840). */
int dspi_save_preset_slot(dspi_ctx *ctx, int32_t stream, void *image, size_t cap, int slot_index);

/* ---- flash dump --------------------------------------------------------------- */
/* A raw image of the firmware's 48 KB preset area (flash_storage.c:4-26): sector 0 = preset directory (v1 or v2),
 * sectors 1-10 = preset slots 0-9, sector 11 = the legacy single-preset sector. */
#define DSPI_FLASH_DUMP_BYTES (12 * 4096)
typedef struct dspi_flash_dir {
    int32_t valid;                 /* 0: no directory, bad CRC or unknown version */
    int32_t version;               /* 1 or 2 as stored; v1 fields are mapped to v2 as the firmware's migration does (:391-411) */
    uint8_t startup_mode;          /* 0 PRESET_STARTUP_SPECIFIED, 1 _LAST_ACTIVE (config.h:258-259) */
    uint8_t default_slot, last_active_slot, include_pins;
    uint16_t slot_occupied;        /* bit n: slot n holds a preset */
    uint8_t master_volume_mode, pad_;
    float master_volume_db;
    char slot_names[10][32];
} dspi_flash_dir;
/* dir_load_cache: flash_storage.c:370-417 (no context needed) */
int dspi_flash_read_directory(const void *dump, size_t len, dspi_flash_dir *out);
/* Picks the startup preset the way preset_boot_load does (flash_storage.c:1047-1105: startup mode, occupancy, slot
 * validation, legacy-sector migration :997-1045).  On a DSPI_BOOT_POPULATED_FLASH context that has not processed audio yet
 * the call is the device's BOOT from that flash (see the flag: no mute, no line zeroing, exact from frame 0); on every
 * other context the preset is applied the way REQ_PRESET_LOAD does on a running device.  Returns 0..9 = that slot was loaded; 16+n = slot n was selected but is empty or corrupt, factory defaults
 * applied; 32 = no directory, legacy sector migrated and loaded; 48 = nothing usable, factory defaults; negative DSPI_E_*. */
int dspi_load_flash_dump(dspi_ctx *ctx, int32_t stream, const void *dump, size_t len);

/* ---- incremental parameters ------------------------------------------------------------ */
/* vendor_cmd_packet (usb_audio.c:1632-2021): payloads shorter than the request needs are ignored, as upstream */
int dspi_vendor_set(dspi_ctx *ctx, int32_t stream, uint8_t bRequest, uint16_t wValue, const void *payload, uint16_t len);
/* vendor_setup_request_handler IN direction (usb_audio.c:2271-2688).  Returns the byte count. */
int dspi_vendor_get(dspi_ctx *ctx, int32_t stream, uint8_t bRequest, uint16_t wValue, void *buf, uint16_t cap);
int dspi_set_host_volume(dspi_ctx *ctx, int32_t stream, int16_t volume_1_256_db);   /* audio_set_volume */
int dspi_set_mute(dspi_ctx *ctx, int32_t stream, int mute);
int dspi_set_sample_rate(dspi_ctx *ctx, int32_t stream, uint32_t hz);               /* 44100 / 48000 / 96000 */

/* ---- audio ------------------------------------------------------------------------------ */
/* Runs n_blocks packets of block_len frames for every stream.
 * pcm_in: [stream][n_blocks*block_len] frames of interleaved LE stereo; bit_depth 16 (4 B/frame)
 * or 24 (6 B/frame, packed).  With DSPI_MEM_DEVICE the call is asynchronous on the context's
 * HIP stream (use dspi_sync); without it buffers are host memory and the call returns when
 * the outputs are in place. */
int dspi_process(dspi_ctx *ctx, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len,
                 const dspi_out *out, uint32_t flags);
int dspi_sync(dspi_ctx *ctx);

/* ---- stream snapshots: a stream's complete state, out of one context and into another ------------------------------------ */
/* Everything a stream is — its parameters with whatever state operations are still pending on them, every state slot (filters,
 * loudness, crossfeed, leveller, ring position, delay write index, mute envelope, last peaks, clip slots), every delay line at full
 * length, both leveller rings, the PDM modulator's words (power-on values when the source never ran dspi_pdm_modulate) — exported
 * after packet k and imported anywhere else continues from packet k + 1 with exactly the words an uninterrupted run produces: on
 * another context, another GPU, another process, at another stream index (a float stream may change its row and its side of a packed
 * lane).  Write positions (delay write index, leveller ring position) travel as they are unless the import is asked to realign them
 * (DSPI_SNAP_REALIGN below); rows whose streams carry different positions are served by the kernels' per-stream addressing, which
 * is correct and slower than a row that shares one position.
 *   head    host memory, always: a 64-byte header (magic, format version, flavour, float contract, record size, count, number of
 *           parameter objects, fingerprint of the internal layout, CRC-32 of the head), one parameter object per DISTINCT parameter
 *           set in the range, one uint32 index per stream
 *   state   one fixed-size record per stream, stream-major, in range order: state_bytes / count bytes each (a multiple of 16);
 *           host memory, or with DSPI_MEM_DEVICE device memory aligned to 16 bytes.  Records are independent of each other, so a
 *           long range can be moved in chunks: export / import sub-ranges, each with its own head.
 * A snapshot is a HAND-OVER format, not an archive: only a library of the same build (same fingerprint) takes it.
 * What does NOT travel (per context, not per stream): the S/PDIF block position (dspi_spdif_block_pos), the direct path's polling
 * statistics.  A stream's OWN S/PDIF block position (dspi_spdif_per_stream below) does not travel either — the record and head formats and
 * the fingerprint know nothing of it, and an import leaves the slot's position as it is —: a caller that migrates a device carries it with
 * dspi_spdif_stream_pos, get on the source context, set on the destination.  "Has processed audio" does: after an import of running devices the context no longer treats dspi_load_flash_dump as a boot.
 * With DSPI_MEM_DEVICE the calls are asynchronous on the context's stream like dspi_process: between two contexts, dspi_sync the
 * source after the export and before the import reads `state` (the import's own stream does not wait for the source's).  Without
 * the flag the calls stage through device memory in chunks and return when the bytes are in place.  Flags other than
 * DSPI_MEM_DEVICE (both calls) and DSPI_SNAP_REALIGN (import only) are refused (DSPI_E_INVAL).  Host-only contexts:
 * dspi_snapshot_sizes works, the other two return DSPI_E_NODEVICE after validating their arguments. */
#define DSPI_SNAP_REALIGN 0x100u   /* dspi_import_streams: every imported stream takes the write positions of its destination row */
typedef struct dspi_snapshot {
    void *head;   size_t head_bytes;     /* host memory, always */
    void *state;  size_t state_bytes;    /* per-stream records; device memory with DSPI_MEM_DEVICE */
} dspi_snapshot;
/* Bytes an export of streams [first, first + count) needs (either pointer may be NULL).  Returns 0 or a negative DSPI_E_*. */
int dspi_snapshot_sizes(const dspi_ctx *ctx, uint32_t first, uint32_t count, size_t *head_bytes, size_t *state_bytes);
/* Writes streams [first, first + count) into snap (its *_bytes: the capacities).  The context is not changed: it goes on processing
 * bit-exactly.  Returns count, DSPI_E_SHORT when a buffer is too small, or another negative DSPI_E_*. */
int dspi_export_streams(dspi_ctx *ctx, uint32_t first, uint32_t count, const dspi_snapshot *snap, uint32_t flags);
/* Overwrites streams [first, first + n) with the snapshot's n streams (n from the head), in order; `first` and the context's size
 * need not be the source's.  Streams outside the range keep their state and parameters.  The imported parameter objects become images
 * of this context; equal ones (among themselves or to images already present) fold into one at the next commit, so streams on a
 * preset the context already holds return to the shared-parameter kernels.  EVERYTHING is validated before ANYTHING is written:
 * a wrong magic, version, flavour, contract or fingerprint, a CRC mismatch, sizes that do not add up, an image index out of range, a
 * short state buffer (DSPI_E_SHORT) or a range past dspi_num_streams return an error and leave the context exactly as it was.
 * Returns n or a negative DSPI_E_*. */
int dspi_import_streams(dspi_ctx *ctx, uint32_t first, const dspi_snapshot *snap, uint32_t flags);
/* ---- realignment: a row's streams back onto one write position ------------------------------------------------------------- */
/* A delay line and a leveller ring are circular and addressed only relative to the stream's position slot, so a stream whose nine (five)
 * lines are rotated by d and whose delay write index is advanced by d — likewise the two rings and the ring position — is the same
 * stream: its output does not change by a bit.  The chain kernels serve a row (128 float / 64 Q28 streams) whose streams share their
 * positions with one row access per wave; streams that arrived from a context of another age do not share them.
 * With DSPI_SNAP_REALIGN, dspi_import_streams writes stream k rotated: with L the line length (4096 / 2048), N = 1024 the ring length,
 * (w_s, r_s) the positions in k's record (masked to L, N) and (w_t, r_t) the target of k's destination row,
 *   line[o][(p + w_t - w_s) mod L] = record.line[o][p]    ring[ch][(p + r_t - r_s) mod N] = record.ring[ch][p]    widx := w_t   ring_pos := r_t
 * and everything else (other state slots, PDM words, parameters, images, pending operations) exactly as without the flag.
 * The target of a row is the (widx, ring_pos) of its lowest-numbered stream that is below dspi_num_streams and OUTSIDE the range being
 * written — a resident neighbour, read on the device behind whatever the context's stream still has to do —; a row without one takes the
 * pair of the first stream of the range that lands in it.  So a range of whole rows moves its rows' first streams by 0, and into a fresh
 * context it is word for word the plain import.  DSPI_MEM_DEVICE imports stay asynchronous.  dspi_export_streams refuses the flag.
 *
 * dspi_realign_streams does the same in place for streams [first, first + count) of a context (rows mixed by earlier plain imports, or
 * streams that drifted apart with no snapshot at all: different histories of delays active / leveller on): run-time state only, through
 * the context's own device scratch, asynchronous on the context's stream like dspi_process with device buffers.  No parameter object,
 * image or pending operation is touched; a second call on an aligned range changes nothing.  Arguments are validated before anything is
 * written; host-only contexts return DSPI_E_NODEVICE after that.  Returns count or a negative DSPI_E_*. */
int dspi_realign_streams(dspi_ctx *ctx, uint32_t first, uint32_t count);

/* ---- paused streams: devices that receive no packet in a call ---------------------------------------------------------------- */
/* The firmware's chain runs only when a USB packet arrives (usb_audio_drain_ring, usb_audio.c:1326-1332); between packets nothing moves
 * ("clamp during USB gaps", :1304-1305): filters, leveller envelope, delay lines, mute countdown and peak words stay where the last packet
 * left them, and the next packet continues from there.  Vendor requests still land while no audio flows, and their side effects on audio
 * state (path resets, line zeroing on a preset load) happen in the main loop, not in the packet.  A paused stream is such a device: it sits
 * out whole dspi_process calls (feeding it zeros would be wrong: the filters ring down, the leveller adapts, the lines fill with silence,
 * the mute envelope runs).  A stream takes part in a whole call or in none of it; packet lengths stay one per call.
 *   effect and timing   pause and resume take effect at the next dspi_process, like every parameter call.  Pausing a paused stream or
 *                       resuming an active one is a no-op for that stream.  Both calls return count.  A range past dspi_num_streams, a
 *                       count of 0 or (resume) an undefined flag bit is DSPI_E_INVAL and changes nothing.  Both calls and the query work
 *                       on host-only contexts, where they are bookkeeping.
 *   in dspi_process     a paused stream takes no part: none of its state slots, delay lines, rings, peak slots, clip slots or mute
 *                       countdown is read for audio or written, and its part of pcm_in is never read (the buffer still spans all streams).
 *   what the caller finds   with DSPI_MEM_DEVICE no byte of its region of pairs, sub or peaks is written (with DSPI_OUT_TILED the region is
 *                       its column); with host buffers those regions come back as zeros.  With DSPI_OUT_SPDIF on host buffers the regions
 *                       hold zero words, which are not valid subframes — do not shift them out (a later build may deliver the subframes of
 *                       silence there instead, as the two-pass path does for DSPI_OUT_ENABLED_ONLY's silent pairs: rely on neither).
 *                       clip_flags[stream] is still written and dspi_get_status still answers: both report the frozen state.
 *   parameter calls     addressed to a paused stream, single or broadcast, work as before, and their state operations (filter path
 *                       resets, the preset mute, zeroed lines) are applied at the next dspi_process commit whether the stream is paused or
 *                       not: the firmware's main loop does not wait for audio.
 *   every stream paused dspi_process launches no chain kernel and returns DSPI_OK; the S/PDIF block position (per context) still
 *                       advances; such a call does not make a DSPI_BOOT_POPULATED_FLASH context "running" (dspi_load_flash_dump stays a boot).
 *   dspi_pdm_modulate   skips paused streams: their modulator state stays frozen, their `words` are unwritten in device buffers and zero
 *                       in host buffers.  dspi_spdif_encode and dspi_i2s_encode are stateless per stream and know no pauses.
 *   snapshots           activity is a property of the SLOT, not of the stream: it does not travel.  Exporting a paused stream works and
 *                       gives the frozen state; importing into a paused slot leaves the slot paused.
 *   resume              while a stream stands still its row's write positions go on.  By default a resumed stream takes the delay write
 *                       index and ring position of its row, its lines and rings rotated as DSPI_SNAP_REALIGN does (above): the same stream,
 *                       bit for bit, back on the kernels' one-access-per-row path.  The target of a row is the (widx, ring_pos) of the
 *                       row's lowest-numbered stream that is below dspi_num_streams and was ACTIVE before the call; a row without one takes
 *                       the pair of the first stream of the range that this call actually resumes and that lies in the row.  Streams of the
 *                       range that were already active are residents and are not moved.  DSPI_RESUME_AS_IS skips the rotation: the stream
 *                       keeps its stale positions, which is correct and runs on the kernels' per-stream addressing (slower).  The call is
 *                       asynchronous on the context's stream like dspi_realign_streams; it synchronises once when pauses or resumes were
 *                       made since the last dspi_process (the rule reads the activity as it stood before the call, on the device). */
#define DSPI_RESUME_AS_IS 0x1u   /* dspi_resume_streams: keep the streams' own write positions (no realignment) */
int dspi_pause_streams (dspi_ctx *ctx, uint32_t first, uint32_t count);
int dspi_resume_streams(dspi_ctx *ctx, uint32_t first, uint32_t count, uint32_t flags);
/* paused[i] = 1 if stream first + i is paused (paused may be NULL); returns how many of the range are paused */
int dspi_streams_paused(const dspi_ctx *ctx, uint32_t first, uint32_t count, uint8_t *paused);

/* ---- stream moves: a stream changes its slot inside its context ------------------------------------------------------------------ */
/* A context whose devices come and go ends up with its active streams scattered: lanes whose mate is paused leave the packed kernel, and
 * half the streams can cost more than all of them (profiles/pause.md).  dspi_move_streams moves streams between slots by list, so that the
 * active ones can be put back into whole rows; dspi_plan_compaction writes the list that does exactly that.
 *   what the call does  after it, slot `dst` holds the stream that slot `src` held before it, for every entry AT ONCE: all sources are
 *                       read as they stood before the call, so swaps, cycles and chains are legal.  Entries with src == dst are dropped;
 *                       those streams count as residents (below).  Returns the number of entries applied (identities excluded).
 *   what travels        everything a snapshot carries — every state slot (last peaks, clip slots, mute envelope, ring position, delay write
 *                       index among them), every delay line at full length, both leveller rings, the PDM modulator words — and the
 *                       stream's parameter object BY REFERENCE: the slot's image reference moves, no parameter object is copied and no
 *                       image is added; pending state operations stay on the object and reach the stream at its new slot at the next
 *                       commit.  Whether the stream is paused travels too: here, unlike in snapshots, activity belongs to the stream.  So
 *                       dspi_get_status, dspi_collect_bulk, dspi_vendor_get and dspi_clear_clips answer at dst as they answered at src.
 *   open ends           a slot that is a source and not a destination keeps its bytes and its parameter reference as a frozen copy and
 *                       becomes PAUSED.  A slot that is a destination and not a source loses its former occupant; it must be paused
 *                       before the call: a move never overwrites an active stream that the same call does not move away.
 *   realignment         by default every moved stream takes the (widx, ring_pos) of its destination row, its lines and rings rotated
 *                       exactly as DSPI_SNAP_REALIGN rotates them (above).  A resident is a stream below dspi_num_streams that was active
 *                       before the call and is neither a source nor a destination of it.  A row's target is the position pair of its
 *                       lowest-numbered resident, read on the device behind the context's earlier work; a row without a resident takes the
 *                       pair of the stream that arrives at the row's lowest-numbered destination, as it stands at its source.  All
 *                       rotations are fixed once for the whole call before anything is written.  Moved paused streams are rotated too
 *                       (harmless: a later resume realigns them again).  DSPI_MOVE_AS_IS skips the rotation.
 *   validation          everything is validated before anything is written.  n == 0, a null list, an index at or past dspi_num_streams,
 *                       a slot that is the source of two entries, a slot that is the destination of two entries, an active destination
 *                       that is not a source, an undefined flag bit: DSPI_E_INVAL, and the context is bit for bit as it was.  Host-only
 *                       contexts validate and then return DSPI_E_NODEVICE, as the import does.
 *   timing              asynchronous on the context's stream like dspi_realign_streams (who the residents are is decided on the host, whose
 *                       record of the pauses is the truth: the call never waits for the device's copy of it); takes effect at the next
 *                       dspi_process.  A list of any length goes through the context's record scratch in batches (DSPI_MOVE_BATCH, read at
 *                       dspi_create: records per batch, at least 2; default: the snapshot chunk).
 *   not touched         the S/PDIF block position, the direct path's statistics, "has processed audio".
 *
 * dspi_plan_compaction is bookkeeping and works on host-only contexts: it writes the shortest list after which slots [0, A) are active and
 * [A, dspi_num_streams) paused, A = the number of active streams.  H = the paused slots below A, T = the active slots at or above A, both
 * ascending (always equally many); pair i is the swap {T[i] -> H[i]}, {H[i] -> T[i]} — no paused device is lost — or, with
 * DSPI_COMPACT_ONE_WAY (the caller treats paused slots as free), {T[i] -> H[i]} alone.  Returns the number of entries; moves == NULL only
 * counts; a cap below that number is DSPI_E_SHORT and writes nothing.  The caller relocates its own per-stream buffers by the same list.
 * Not in scope here: choosing the pairing by parameter image, so that the two streams of a lane share a preset — that list is
 * dspi_plan_grouping's (below). */
typedef struct dspi_stream_move { uint32_t src, dst; } dspi_stream_move;
#define DSPI_MOVE_AS_IS      0x1u   /* dspi_move_streams: keep the streams' own write positions (no realignment) */
#define DSPI_COMPACT_ONE_WAY 0x1u   /* dspi_plan_compaction: paused slots are free, do not preserve them */
int dspi_move_streams(dspi_ctx *ctx, const dspi_stream_move *moves, uint32_t n, uint32_t flags);
int dspi_plan_compaction(const dspi_ctx *ctx, dspi_stream_move *moves, uint32_t cap, uint32_t flags);

/* ---- migration: streams change their context ---------------------------------------------------------------------------------------- */
/* A node runs one context per GPU, and a device lives where dspi_create put it.  dspi_migrate_streams is dspi_move_streams between two
 * contexts of one process — on one GPU or on two —, addressed by the same kind of list: in every entry `src` is a slot of the SOURCE
 * context and `dst` a slot of the DESTINATION context.  dspi_plan_migration writes the list that shifts `want` streams from a fuller
 * context to an emptier one.  Detected by the symbol dspi_migrate_streams.
 *   what the call does  after it, slot moves[i].dst of `dst` holds the stream that slot moves[i].src of `src` held before it, for every
 *                       entry at once.  Returns n.
 *   what travels        everything a snapshot record carries — every state slot, every delay line at full length, both leveller rings,
 *                       the PDM modulator words (the power-on words if the source never ran the modulator) —; the stream's parameters BY
 *                       VALUE: each distinct parameter object among the listed streams is copied once, with its pending state operations,
 *                       and the copies become objects of `dst` exactly as an import adds them (equal ones fold at dst's next commit); the
 *                       stream's activity, unless DSPI_MIGRATE_PAUSED is set; "has processed audio", as on an import; and the stream's
 *                       S/PDIF block position: both contexts in per-stream mode (dspi_spdif_per_stream): the stream's own position; `dst`
 *                       in the mode and `src` not: src's context position; `dst` not in the mode: nothing per stream exists, so nothing
 *                       travels.
 *   source slots        every listed source slot keeps its bytes and its parameter reference as a frozen copy and becomes PAUSED (the open
 *                       end of dspi_move_streams).  Nothing else in `src` changes.
 *   destination slots   every listed destination must be PAUSED in `dst` before the call: a migration never overwrites an active stream.
 *                       The former occupant is gone and its parameter reference is released; the object is dropped at the next commit if
 *                       that was its last reference.
 *   realignment         by default every arriving stream takes the (widx, ring_pos) of its destination row, its lines and rings rotated
 *                       exactly as DSPI_SNAP_REALIGN rotates them.  A resident is a stream below dspi_num_streams(dst) that is active in
 *                       `dst` before the call (destinations are paused, so none is a resident).  A row's target is the pair of its
 *                       lowest-numbered resident, read on the device behind dst's earlier work; a row without a resident takes the pair of
 *                       the stream that arrives at the row's lowest-numbered destination, as it stands at its source: that pair is read on
 *                       the device behind src's earlier work.  All rotations are fixed once for the whole call before anything is written.
 *                       DSPI_MIGRATE_AS_IS skips the rotation.
 *   validation          everything is validated in BOTH contexts before anything is written in either.  A null context, src == dst (use
 *                       dspi_move_streams), different flavours or float contracts, n == 0 or a null list, a source index at or past
 *                       dspi_num_streams(src), a destination index at or past dspi_num_streams(dst), a slot named twice as a source, a
 *                       slot named twice as a destination, an active destination, an undefined flag bit: DSPI_E_INVAL, and both contexts
 *                       are bit for bit as they were.  A host-only context on either side validates and then returns DSPI_E_NODEVICE, as
 *                       moves do.  The refusal text is set on both contexts (dspi_last_error).
 *   timing and threads  takes effect at each context's next dspi_process.  No thread may use either context during the call.  With the
 *                       device transports the call only enqueues, on both contexts' streams, tied by events: asynchronous like
 *                       dspi_move_streams; the source's stream ends up waiting for the destination's last scatter, so dspi_sync(src) or
 *                       dspi_destroy(src) covers dst's use of src's record scratch.  With the host transport it returns when the bytes are
 *                       in place.  A list of any length goes through the record scratch in batches of the smaller of the two contexts'
 *                       capacities (DSPI_MOVE_BATCH).
 *   transports          DSPI_MIGRATE_VIA, read at dspi_create; the destination context's value decides.  Unset: contexts on one device
 *                       scatter straight out of the source's scratch, contexts on two devices copy device to device into the
 *                       destination's scratch on the destination's stream.  "copy": always copy into the destination's scratch (on one
 *                       GPU the two-device code with equal device numbers).  "host": through a pinned host area, synchronising per batch.
 *   not touched         both contexts' own S/PDIF block positions, the direct path's statistics, the capacities.
 *
 * dspi_plan_migration is bookkeeping and works on host-only contexts.  k = min(want, active streams of src, paused slots of dst).  The
 * sources are the k highest-numbered active slots of `src`, so a compact source stays compact and its top becomes cuttable
 * (dspi_resize_streams: the vacated top slots are paused, which is what a cut range must be); the destinations are the k lowest-numbered
 * paused slots of `dst`; entry i pairs the i-th lowest chosen source with the i-th lowest chosen destination, so order is kept and the
 * runs that grouping made stay runs.  Returns k; moves == NULL only counts; a cap below k is DSPI_E_SHORT and writes nothing; flags != 0,
 * a null context, or different flavours or float contracts: DSPI_E_INVAL.  It treats EVERY paused slot of `dst` as free, as
 * DSPI_COMPACT_ONE_WAY does: a caller who parks real devices in paused slots writes their own list.  dspi_migrate_streams accepts every
 * list it writes.  A rebalance: grow `dst` with DSPI_RESIZE_PAUSED where it is short, plan, migrate, shrink `src`.
 * Not in scope: a policy that decides when to rebalance or how many streams; dspi_host -g N driving it; migration between processes (that
 * remains the snapshot's job); a list-addressed dspi_export_streams; padding arrivals to whole rows; choosing sources by preset; any
 * change to the snapshot format or its fingerprint. */
#define DSPI_MIGRATE_AS_IS  0x1u   /* keep the streams' own write positions (no realignment) */
#define DSPI_MIGRATE_PAUSED 0x2u   /* every migrated stream arrives paused, whatever it was at its source */
int dspi_migrate_streams(dspi_ctx *src, dspi_ctx *dst, const dspi_stream_move *moves, uint32_t n, uint32_t flags);
int dspi_plan_migration(const dspi_ctx *src, const dspi_ctx *dst, uint32_t want, dspi_stream_move *moves, uint32_t cap, uint32_t flags);

/* ---- grouping: streams of one preset into shared rows ------------------------------------------------------------------------------- */
/* Compaction keeps a context's active streams in whole rows; it does not look at their parameters.  The launch plan picks the kernel by
 * who sits beside whom: a float lane whose two streams share a parameter object runs the packed kernel, a row whose streams hold several
 * objects of one structure runs the per-lane-value kernels, every other lane falls to the one-stream kernel, and a Q28 row with two
 * objects leaves the workgroup-uniform path whole.  Two structurally different presets assigned alternately put every stream of a context
 * on the one-stream kernel; devices that arrive by dspi_boot_streams, by import or by per-stream requests land wherever a slot was free.
 * dspi_plan_grouping writes the list for dspi_move_streams after which
 *   - slots [0, A) are active and [A, dspi_num_streams) paused, A = the number of active streams, as after compaction,
 *   - the active streams of every parameter object occupy one contiguous run of slots,
 *   - runs of objects with the same structure lie next to each other.
 * The call is bookkeeping: it works on host-only contexts and writes nothing to the device.  The context is not const because the call
 * first folds equal parameter objects into one (the fold-back pass of dspi_debug_image_count, run here whether or not a broadcast call has
 * asked for it): two devices loaded with the same blob through separate calls are one group.  Nothing else about the context changes.
 * Returns the number of entries; moves == NULL only counts; a cap below that number is DSPI_E_SHORT and writes nothing; an undefined flag
 * bit or a null context is DSPI_E_INVAL.  The caller relocates its own per-stream buffers by the same list, as with compaction.
 * The rule (deterministic):
 *   1 groups     a group is the set of active streams of one parameter object, after folding.  Its structure is what the per-lane-value
 *                kernels need to agree (bypassed channels, enabled and muted outputs, sample rate, delays in samples, band kinds, ...),
 *                compared bytewise (float); on Q28 all objects form one class.  first(g) = the lowest active slot that holds g,
 *                first(class) = the minimum over its groups.  Groups are ordered by (first(class), first(g)).
 *   2 runs       in that order, group g gets the next |g| slots of [0, A).
 *   3 residents  an active stream of g that already sits inside g's run stays.
 *   4 movers     the other streams of g, ascending by slot, take the run's remaining slots, ascending.
 *   5 paused     H = the paused slots below A, T = the slots at or above A that hold an active stream, both ascending (always equally
 *                many): entry i is {H[i] -> T[i]} — no paused device is lost.  With DSPI_GROUP_ONE_WAY (the caller treats paused slots
 *                as free, as DSPI_COMPACT_ONE_WAY) these entries are omitted; the vacated slots at and above A then stay behind as paused,
 *                frozen copies (dspi_move_streams, open ends).
 *   6 output     identities are never emitted; entries are written ascending by dst.
 * What follows from it: dspi_move_streams accepts the list in both modes (every active destination is itself a source, no slot is named
 * twice on either side); for this layout no shorter list exists (the count is the active streams outside their run, plus |H| without the
 * flag); planning again on the result returns 0, so a context that is already grouped is never disturbed; a context with one object, or
 * with nothing active, returns 0.  A context with no paused stream and one object per structure class yields a pure permutation of
 * active slots.
 * Not in scope: padding groups to whole rows with paused slots (a boundary row between two runs costs one extra workgroup: at most
 * groups - 1 such rows), choosing the run order to minimise moves globally, choosing the slot an arrival takes. */
#define DSPI_GROUP_ONE_WAY 0x1u   /* dspi_plan_grouping: paused slots are free, do not preserve them (as DSPI_COMPACT_ONE_WAY) */
int dspi_plan_grouping(dspi_ctx *ctx, dspi_stream_move *moves, uint32_t cap, uint32_t flags);

/* ---- stream boots: a slot is power-cycled inside its running context -------------------------------------------------------------- */
/* Devices are unplugged and plugged in again, firmware reboots, and a slot that compaction freed (dspi_plan_compaction with
 * DSPI_COMPACT_ONE_WAY) is where a device that arrives goes.  dspi_create makes power-on state for a whole context, and
 * dspi_load_flash_dump is a boot only before the first audio; dspi_boot_streams makes it for listed slots of a running context, without a
 * second context and without moving a record of zeros.
 *   what the call does  every listed slot becomes a device that has just been powered on; its former occupant is gone.  The list may
 *                       be in any order.  Returns n.
 *   dump == NULL        the device dspi_create makes on this context: by default a first boot on an erased flash (the 512-sample mute is
 *                       armed, then the fade-in), on a DSPI_BOOT_POPULATED_FLASH context the populated flash without a selected preset.
 *                       len is ignored.
 *   dump != NULL        the device boots from that preset area (DSPI_FLASH_DUMP_BYTES, laid out as for dspi_load_flash_dump) exactly as
 *                       a DSPI_BOOT_POPULATED_FLASH context that has processed no audio boots from it — on every context, whether it
 *                       has processed audio or not.  A boot that writes the flash (no directory, a v1 directory) arms the mute.
 *   selection           (may be NULL) receives preset_boot_load's code as dspi_load_flash_dump returns it (0..9, 16 + n, 32, 48); 48 for
 *                       a NULL dump.
 *   host settings       sample rate 44.1 kHz, UAC1 volume 0 dB and unmuted are power-on values too: the caller sets them afterwards, as
 *                       a USB host does after enumeration.
 *   parameters          all listed streams leave their parameter objects and share ONE new object, so a batch of arrivals stays on the
 *                       shared-parameter kernels.  Pending state operations of the objects they left never reach them; the new
 *                       object's own (the mute that a flash-writing boot arms) are applied at the next dspi_process commit over the
 *                       power-on state, the order after dspi_create.  An object that lost its last stream is dropped at that commit.
 *   run-time state      every state slot goes to its power-on word (unity leveller gains, mute envelope 1.0, zero elsewhere — last
 *                       peaks and clip slots among them: dspi_get_status answers zeros), every delay line is zeroed at full length,
 *                       both leveller rings are zeroed, and the PDM modulator words go to their power-on values if the context has run
 *                       the modulator (otherwise they are power-on values already).
 *   write positions     zero lines and rings are zero under every rotation, so nothing is rotated: by default a booted stream TAKES the
 *                       (widx, ring_pos) of its row, and the row stays on the kernels' one-access-per-row path.  A resident is a stream
 *                       below dspi_num_streams that is active and not in the list, as for moves.  A row's target is the pair of its
 *                       lowest-numbered resident, read on the device behind the context's earlier work; a row without a resident gets
 *                       (0, 0).  DSPI_BOOT_STREAMS_AS_IS writes (0, 0) always.
 *   activity            a property of the slot, as in snapshots: a paused slot stays paused — the new device sits frozen in power-on
 *                       state until dspi_resume_streams — and an active slot stays active.
 *   validation          everything is validated before anything is written.  n == 0, a null list, an index at or past
 *                       dspi_num_streams, a slot listed twice, an undefined flag bit: DSPI_E_INVAL; a non-NULL dump with len below
 *                       DSPI_FLASH_DUMP_BYTES: DSPI_E_SHORT; the context is bit for bit as it was.
 *   timing              asynchronous on the context's stream like dspi_move_streams; takes effect at the next dspi_process.
 *   host-only contexts  the call works there (parameter objects, references, selection): that is what a host-only context is for.
 *   not touched         the S/PDIF block position, the direct path's statistics, "has processed audio".
 *                       (With dspi_spdif_per_stream on, the listed slots' own positions go to 0, with and without DSPI_BOOT_STREAMS_AS_IS: a
 *                       device that has just been powered on sends frame 0 of a block, preamble Z, first; see there.)
 * Not in scope: choosing which free slot an arrival takes. */
#define DSPI_BOOT_STREAMS_AS_IS 0x1u   /* keep the power-on write positions (delay write index 0, ring position 0) */
#define DSPI_BOOT_STREAMS_OWN_FLASH 0x2u   /* every listed slot reboots from its own flash (dspi_device_flash, below); the dump must be NULL */
int dspi_boot_streams(dspi_ctx *ctx, const uint32_t *streams, uint32_t n,
                      const void *dump, size_t len, uint32_t flags, int *selection);

/* ---- a stream's own flash: each stream owns its preset area, REQ_PRESET_* served ----------------------------------------------------------- */
/* A DSPi device keeps ten presets, their names and its startup choice in 48 KB of flash, and its control application works through the
 * preset directory requests: REQ_PRESET_SAVE / LOAD / DELETE (0x90-0x92), REQ_PRESET_GET_NAME / SET_NAME / GET_DIR (0x93-0x95),
 * REQ_PRESET_SET_STARTUP / GET_STARTUP (0x96-0x97), REQ_PRESET_SET_INCLUDE_PINS / GET_INCLUDE_PINS (0x98-0x99), REQ_PRESET_GET_ACTIVE (0x9A)
 * and the legacy REQ_SAVE_PARAMS / REQ_LOAD_PARAMS (0x51 / 0x52).  Without this mode a stream has no flash and those requests
 * answer DSPI_E_UNSUPPORTED; with it every stream owns a preset area (DSPI_FLASH_DUMP_BYTES, laid out as for dspi_load_flash_dump), a device
 * that is re-plugged or rebooted comes back with the presets its user saved, and all of it is held to the reference's own flash_storage.c,
 * request handlers and main loop, byte for byte (tests/test_device_flash_cpu.py, tests/test_gpu_device_flash.py).
 * There is NO NEW KERNEL in this mode and NO TIMING FIGURE: the audio side of these requests is mutes, delay-line zeroing and resets, which
 * reach the streams as state operations at the next dspi_process commit like those of every other request.  The mode is consulted in
 * request and maintenance calls only; dspi_process does no extra work per call.
 *   the mode            belongs to the context, off after dspi_create.  dspi_device_flash(ctx, enable): enable < 0 only reads; returns the
 *                       mode (0 / 1).  Off: every call behaves exactly as before, the requests above answer DSPI_E_UNSUPPORTED, and
 *                       dspi_flash_read / dspi_flash_write / DSPI_BOOT_STREAMS_OWN_FLASH are refused (DSPI_E_INVAL).  Turning it on gives
 *                       every stream the flash its boot left: the first-boot preset area (a version 2 directory in sector 0, name
 *                       "Default", everything else erased; on a DSPI_BOOT_POPULATED_FLASH context an erased area), with the master-volume
 *                       mode and the saved master volume of the stream's own parameters in the directory.  On a fresh default context that
 *                       is byte for byte the flash of a firmware that has just been powered on.  The directory's include_pins is the
 *                       first boot's 1, and load_bulk honours it from then on, as the device does.  Turning it off drops the flashes.
 *   cost                48 KB of host memory per DISTINCT flash: streams share one object until one of them writes (clone on write, like
 *                       the parameter objects).  65 536 distinct flashes are 3.2 GB.
 *   requests            served through dspi_vendor_get / dspi_vendor_set in the direction and with the status bytes the firmware uses:
 *                       SAVE / LOAD / DELETE / SAVE_PARAMS / LOAD_PARAMS answer on the IN side — PRESET_ERR_INVALID_SLOT (1) for a slot
 *                       >= 10, else "accepted" (0); LOAD_PARAMS answers its result (0, or 3 for a slot that fails its CRC).  GET_NAME of a
 *                       slot >= 10 stalls (DSPI_E_UNSUPPORTED).  SET_STARTUP with a bad mode or slot, SET_NAME of a slot >= 10 are
 *                       accepted and ignored.  A SET without payload or with more than 64 bytes stalls, as the device's setup stage does.
 *                       REQ_SET_MASTER_VOLUME_MODE and REQ_SAVE_MASTER_VOLUME write the directory sector.
 *   the mute            what stands after each request is what the firmware leaves once its main loop has served it: every sector write
 *                       re-arms max(10 ms, 512) samples at the stream's rate; deleting the active slot leaves 256 (and factory
 *                       defaults); a load or delete that changes an output slot's type the type switch's 256; a setter that is ignored
 *                       leaves the 120 ms pre-mute of the firmware's flash-write bracket.  The bracket's wall-clock waits pass no audio.
 *   the directory       the firmware's cached one: read from sector 0 at boot, equal to it after every write; it differs from the sector
 *                       only in last_active_slot between a boot that selected another slot and the next write, as on the device.
 *   broadcast           a request addressed to DSPI_ALL_STREAMS is applied once per distinct (parameter object, flash object) pair; streams
 *                       that shared both keep sharing both.  The answer is stream 0's.
 *   dspi_flash_read     (ctx, stream, dump, cap): the stream's 48 KB.  Returns DSPI_FLASH_DUMP_BYTES; cap below it: DSPI_E_SHORT.
 *   dspi_flash_write    (ctx, first, count, dump, len): one image for the whole range, as ONE shared object.  It replaces the bytes and boots
 *                       nothing: the live parameters stay, except that their mirrors of the directory (master-volume mode, saved master
 *                       volume, include_pins) are taken from the new directory (from the fresh one a device would see where the dump
 *                       holds none).  Ranges and lengths are validated before anything is written.  This is how a flash is carried
 *                       beside a snapshot, as dspi_spdif_stream_pos carries positions.
 *   boots               dspi_load_flash_dump and dspi_boot_streams(dump) make the dump the streams' flash (one shared object) with the
 *                       boot's own writes applied: a created directory, a version 1 directory persisted as version 2, a legacy sector
 *                       migrated into slot 0.  dspi_boot_streams(NULL) gives the first-boot flash (DSPI_BOOT_POPULATED_FLASH: an erased one).
 *                       DSPI_BOOT_STREAMS_OWN_FLASH (dump must be NULL): every listed slot reboots from its own flash — the device that
 *                       was re-plugged; the listed streams share one new parameter object per distinct flash object among them, and
 *                       `selection` receives the first listed stream's code.  Everything else is dspi_boot_streams as documented.
 *   travel              dspi_move_streams: by reference, all entries at once; an open-end source keeps its flash.  dspi_migrate_streams:
 *                       by value into the destination's book; the destination must have the mode if the source has (else DSPI_E_INVAL
 *                       before either context is written); arrivals from a context without the mode get first-boot flashes.
 *                       dspi_resize_streams: new slots share one first-boot flash, a shrink releases.  Pause, resume, realign, grouping
 *                       and compaction plans do not touch it.  Snapshots do not carry it: an import leaves the slot's flash alone (the
 *                       imported parameters' directory mirrors follow it); dspi_flash_read / dspi_flash_write carry it.
 *   not touched         dspi_load_preset_slot, dspi_save_preset_slot, dspi_factory_defaults and dspi_load_bulk neither read nor write the
 *                       flash (the firmware's factory reset leaves the directory alone too).
 *   host-only contexts  everything here works on them. */
int dspi_device_flash(dspi_ctx *ctx, int enable);
int dspi_flash_read(dspi_ctx *ctx, uint32_t stream, void *dump, size_t cap);
int dspi_flash_write(dspi_ctx *ctx, uint32_t first, uint32_t count, const void *dump, size_t len);

/* ---- resizing: a context gains and gives back slots ----------------------------------------------------------------------------------- */
/* n_streams is no constant of dspi_create.  A context that has drained (dspi_plan_compaction with DSPI_COMPACT_ONE_WAY, dspi_move_streams:
 * the survivors sit in [0, A)) gives the rest back, a full one takes more devices, and contexts of different device classes on one GPU
 * trade capacity as their population shifts — without a second context and an export and import of everything.
 * The persistent per-stream arrays (state slots, delay lines, leveller rings, the PDM words once allocated) are rows of R =
 * dspi_tile_streams streams, row-outermost.  A context has a CAPACITY of rows, at least the rows in use; dspi_stream_capacity returns it
 * in streams (rows x R).  After dspi_create it is the rows in use.  Capacity is an allocation fact: no kernel launches over rows past
 * the rows in use.
 *   what the call does  dspi_resize_streams sets dspi_num_streams to n_streams and returns it.  Above the current count the context GROWS:
 *                       slots [old, new) appear.  Inside the capacity no allocation is made.  Past it, new arrays of exactly the rows
 *                       needed are allocated — ALL of them must succeed before anything is written; a failed allocation returns
 *                       DSPI_E_NOMEM and the context, its capacity included, is bit for bit as it was —, the rows in use are copied device
 *                       to device on the context's stream behind its earlier work, the stream is synchronised ONCE and the old arrays
 *                       are freed: during the call both copies exist.  Below the current count the context SHRINKS: the occupants of
 *                       [new, old) are gone; nothing is allocated, freed or waited for, and the capacity stays.  At the current count the
 *                       call returns it and does nothing.
 *                       dspi_reserve_streams sets the capacity to rows(n_streams) x R and returns it, both ways: ahead of a burst of
 *                       arrivals, or — dspi_reserve_streams(ctx, dspi_num_streams(ctx)) — to return the memory after a shrink.  Where the
 *                       capacity has that value already nothing happens; otherwise it reallocates, copies and frees as above, with the
 *                       same atomicity and the same single synchronisation.  dspi_num_streams does not change.
 *   new slots           the devices dspi_create makes on this context, exactly what dspi_boot_streams makes with a NULL dump: by default
 *                       a first boot on an erased flash (the 512-sample mute is armed as a pending operation of the new object), on a
 *                       DSPI_BOOT_POPULATED_FLASH context the populated flash without a selected preset; host settings 44.1 kHz, 0 dB,
 *                       unmuted.  All new slots share ONE new parameter object.  Every state slot, line word, ring word and — if the
 *                       context has run the modulator — PDM word of a new slot is written to its power-on word, whatever the column held:
 *                       a column past dspi_num_streams may be dirty from an earlier shrink, and no padding column is trusted.
 *   write positions     the boot's rule; the residents are the ACTIVE streams below the old count.  A new slot in a row that has a
 *                       resident takes the (widx, ring_pos) of the row's lowest-numbered resident, read on the device behind the
 *                       context's earlier work; a row without a resident — every whole new row — gets (0, 0).  A grown row stays on the
 *                       kernels' one-access-per-row path.
 *   activity            new slots are active; with DSPI_RESIZE_PAUSED they are paused, frozen in power-on state until
 *                       dspi_resume_streams.  The flag has no meaning on a shrink and is accepted there.  With dspi_spdif_per_stream on, the
 *                       new slots' positions are 0 and the old slots keep theirs; with it off nothing per stream exists.
 *   open ends           a shrink releases the cut slots' parameter references; an object that lost its last stream is dropped at the
 *                       next commit, as after a boot; pending operations of objects that are still referenced stay.  Every slot of the
 *                       cut range must be PAUSED: a resize never destroys an active stream, which is the moves' rule.
 *   validation          everything is validated before anything is written.  n_streams == 0, an undefined flag bit, an active slot in
 *                       the cut range, a row count whose byte sizes would overflow size_t (or whose streams an int32_t index cannot
 *                       name); for dspi_reserve_streams n_streams == 0 or below dspi_num_streams: DSPI_E_INVAL, and the context is bit
 *                       for bit as it was.
 *   timing              inside the capacity a grow is asynchronous on the context's stream like dspi_boot_streams, and a shrink is
 *                       bookkeeping.  A call that reallocates waits for the stream once: it is rare and may wait.  All take effect at
 *                       the next dspi_process: pcm_in and every dspi_out buffer then span the new dspi_num_streams (tiled buffers the new
 *                       whole tiles), per-stream calls accept the new range, and the launch plan is rebuilt — a small float context that
 *                       grows past the latency layout's size rule leaves that layout, one that shrinks below it returns to it; no output
 *                       word changes either way.
 *   host-only contexts  both calls work there, as dspi_boot_streams does: objects, references, activity, S/PDIF positions and the
 *                       capacity number.
 *   not touched         the context's S/PDIF block position, "has processed audio", the direct path's statistics, the snapshot
 *                       fingerprint: records are per stream, so a snapshot taken before a resize is importable after it.
 * Not in scope: growing in place through virtual-memory mapping, chunked arrays, a growth policy (geometric reserve is the caller's
 * choice), changing a context's flavour. */
#define DSPI_RESIZE_PAUSED 0x1u   /* dspi_resize_streams, growing: the new slots arrive paused */
int dspi_resize_streams(dspi_ctx *ctx, uint32_t n_streams, uint32_t flags);   /* returns the new dspi_num_streams */
int dspi_reserve_streams(dspi_ctx *ctx, uint32_t n_streams);                  /* returns the new capacity */
uint32_t dspi_stream_capacity(const dspi_ctx *ctx);

/* ---- PDM sub output ---------------------------------------------------- */
/* The consumer of dspi_out.sub: the firmware's 256x oversampled 2nd-order sigma-delta modulator with noise-shaped
 * dither (pdm_generator.c:62-108, :351-397; the loop Core 1 runs in CORE1_MODE_PDM).  One stream = one modulator;
 * its state (integrators, noise shaper, dither RNG, 1024-sample fade-in) lives in the context and carries across calls.
 *   sub    int32 [stream][n_frames]        Q28, exactly what dspi_process wrote to dspi_out.sub
 *   words  uint32 [stream][n_frames][8]    8 x 32 PDM bits per sample, MSB = first bit on the wire (the words the
 *                                          firmware queues for its PIO/DMA)
 * With DSPI_OUT_TILED: sub = [tile][n_frames][R], words = [tile][n_frames][8][R].  DSPI_MEM_DEVICE as in dspi_process.
 * Not modelled: DMA ring pacing, under-run recovery and the fade-out on disable (transport, not sample arithmetic). */
int dspi_pdm_modulate(dspi_ctx *ctx, const int32_t *sub, uint32_t n_frames, uint32_t *words, uint32_t flags);
/* the re-enable path (pdm_generator.c:241-252): integrators, noise shaper and fade-in restart, the dither RNG runs on */
int dspi_pdm_restart(dspi_ctx *ctx, int32_t stream);
/* ---- the PDM words straight out of the call, per-stream on/off ------------------------------------------------------------------- */
/* dspi_process_pdm is dspi_process plus pdm_words: the same arguments, the same flags with the same meanings and refusals (no new flag
 * bit), the same three memory paths and the same outputs in `out`, all optional, out->sub included.  pdm_words has the layout of
 * dspi_pdm_modulate's words — uint32 [stream][F][8], with DSPI_OUT_TILED [tile][F][8][R] — in host or device memory as the other
 * pointers.  NULL pdm_words: DSPI_E_INVAL; a host-only context: DSPI_E_NODEVICE.  The chain's Q28 sub words go to out->sub when the caller
 * passed one and to a scratch of the library's otherwise; the modulator reads them where they are, and the words do not depend on which.
 *
 * In the firmware the modulator runs only while the device's last output is enabled (derive_core1_mode, usb_audio.c:1620-1629:
 * GET_CORE1_MODE == 1); a device whose sub is off has its PDM hardware stopped.  The context keeps one byte per stream, RUNNING, 0 after
 * dspi_create, and at every successful dspi_process_pdm each ACTIVE stream is handled by it:
 *   sub on, not running   modulated AFTER THE RE-ENABLE RESET (pdm_generator.c:239-252): every modulator word at its power-on value except
 *                         the dither RNG, which runs on; the fade-in restarts.  The byte becomes 1.  On a stream that never ran, this is
 *                         the power-on state.
 *   sub on, running       modulated, its state carried over.
 *   sub off               not modulated: its state and RNG stay frozen, its `sub` is not read, its words are NOT WRITTEN in a device buffer
 *                         and are zeros in a host buffer.  The byte becomes 0.
 * A paused stream is not modulated either, its words are handled as a stopped stream's, and its byte is left alone: a device that
 * receives no packets is frozen, like everything else about it.  A failed or refused call changes nothing.  Only the streams that are
 * modulated cost anything: the modulator runs over a list of them, one lane each, in one launch behind the chain's.
 * dspi_process and dspi_pdm_modulate neither read nor write the byte; dspi_pdm_restart resets the device words as always and leaves it alone.
 *
 * NOT MODELLED: the fade-out on disable (pdm_generator.c:223-228, :323-348).  It needs a word of per-stream device state (fade_base_pcm)
 * that the snapshot record's nine PDM words have no room for, so a disable is an IMMEDIATE STOP.  Its consequence: after a disable the
 * firmware's dither RNG has advanced through the fade-out's 1,023 samples and ours has not — exactly as with dspi_pdm_restart — so the
 * words after the next re-enable are those of a device whose RNG stood where the disable found it.  That is the DEFAULT.
 *
 * THE FADE-OUT, OPT-IN: dspi_pdm_fade(ctx, enable)   enable 0 or 1, -1 queries; returns the mode after the call.  A property of the context
 * (like dspi_spdif_per_stream), off after dspi_create, no flag bit of dspi_process_pdm; detect it by this symbol.  Works on host-only
 * contexts.  With the mode off nothing is different from the paragraphs above.  With it on, fade_base_pcm lives BESIDE the nine words, in
 * an array of the context's own, and every successful dspi_process_pdm handles each active stream by the rule above plus:
 *   sub off, running, not fading   the stream starts a fade: fade_out_pos = 1024.
 *   fading                for each frame of the call while fade_out_pos > 1: fade_out_pos--, target = ((fade_base_pcm * fade_out_pos) >> 10)
 *                         + 32768 (pdm_generator.c:326-327), then the 8 chunks of dither, noise shaper and 32 modulator steps and the leaky
 *                         integrators of a normal sample (:366-397) on the stream's carried state; 8 words are written; `sub` is not read;
 *                         the fade-in position is not touched.  A whole fade is 1023 frames (positions 1023..1) and may span calls.
 *                         THE RUNNING BYTE STAYS 1 WHILE THE STREAM FADES.
 *   the end of a fade     once position 1 has been written the fade is over: the byte becomes 0 (a later enable goes through the re-enable
 *                         reset, with the RNG where the fade left it) and the rest of THAT call's frames of the stream are ZERO WORDS, in
 *                         device buffers too.  From the next call on it is a stopped stream as above.  A fade that has written its 1023
 *                         samples is over even if the re-enable arrives before the next call (the firmware would need that request
 *                         to land inside one sample period).
 *   sub on while fading   (:233-237) no reset, state carried: fade-in position := 1024 - fade_out_pos (the fade samples already written),
 *                         the fade ends, and the stream is modulated normally from its first frame of this call.
 * Requests made between two calls count as arriving before the first frame of the next call.  fade_base_pcm is the pcm value of the stream's
 * last normally modulated sample, after the limiter and the fade-in scaling (:352-362); 0 at power-on and when the mode is enabled.  Only
 * dspi_process_pdm with the mode on maintains it: dspi_pdm_modulate and dspi_pdm_restart neither read nor write it (nor the position).
 * A paused stream is frozen, fade position included, and continues on resume.  Enabling the mode gives every stream base 0 and "not
 * fading"; disabling it ends every fade in flight at once: byte 0, no more words.
 * The position and the base travel where the byte does: dspi_move_streams (all entries at once), dspi_migrate_streams (the arrival takes
 * the source's; if either context has the mode off the position arrives as 0, the base is dropped, and a fade in flight has ended as an
 * immediate stop, byte 0), dspi_boot_streams and new slots of a grow (0).  Snapshots are unchanged and carry neither:
 * dspi_pdm_fade_state(ctx, first, count, set, get)   one word per stream: fade_out_pos | (uint32_t)(uint16_t)fade_base_pcm << 16; set and get
 *                       (each may be NULL) as with dspi_pdm_running, host memory always; the context's stream is synchronised.  Validated
 *                       before anything is written: the mode off, a range past dspi_num_streams, a count of 0, a position above 1023 (the
 *                       largest a stream holds between two calls) or |base| > 29500 is DSPI_E_INVAL; a host-only context has no bases:
 *                       DSPI_E_NODEVICE.  Carry a fading stream through a snapshot with this call and dspi_pdm_running.  Returns count.
 *
 * The byte is the stream's own and travels where the per-stream S/PDIF position does:
 *   pause / resume        unchanged.
 *   dspi_move_streams     running[dst] := old running[src], for all entries at once; an open-end source keeps its value.
 *   dspi_migrate_streams  the arrival takes the source's value (the source slot keeps its own, as a frozen copy).
 *   dspi_boot_streams     the listed slots go to 0.
 *   dspi_resize_streams   growing: the new slots are 0.
 *   snapshots             the byte does not travel and an import leaves the slot's byte alone: carry it with dspi_pdm_running, get on the
 *                         source context, set on the destination.  An imported running stream whose byte stays 0 comes up through the reset.
 * dspi_pdm_running(ctx, first, count, set, get)   set (may be NULL): count values, each 0 or 1, for streams [first, first + count); get (may
 *                       be NULL): the bytes after the set.  Host memory always.  Everything is validated before anything is written: a range
 *                       past dspi_num_streams, a count of 0 or a value above 1 is DSPI_E_INVAL and leaves the context as it was.  Returns
 *                       count.  Works on host-only contexts. */
int dspi_process_pdm(dspi_ctx *ctx, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len,
                     const dspi_out *out, uint32_t *pdm_words, uint32_t flags);
int dspi_pdm_running(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint8_t *set, uint8_t *get);
int dspi_pdm_fade(dspi_ctx *ctx, int enable);
int dspi_pdm_fade_state(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get);

/* ---- 16- and 24-bit devices in one call ------------------------------------------------------------------------------------------ */
/* A device's USB host chooses its input format (the alternate setting sets usb_input_bit_depth, usb_audio.c:1575-1585; process_audio_packet
 * reads it per packet, :528-530).  dspi_process_mixed is dspi_process (pdm_words NULL) or dspi_process_pdm (else) with the format per
 * STREAM instead of per call:
 *   bit_depths   uint8 [dspi_num_streams], HOST memory always (like the lists of dspi_move_streams), every entry 16 or 24 — a paused stream's
 *                too: its entry sizes its slot.  An argument of the call, as the PCM is: no context state, nothing travels with a stream.
 *   pcm_in       the [stream][F] frames of dspi_process, F = n_blocks * block_len, each stream at its own frame size, tight:
 *                offset[0] = 0, offset[s + 1] = offset[s] + F * (bit_depths[s] == 24 ? 6 : 4).  A stream's run is only 2-byte aligned (so is
 *                pcm_in itself).  A paused stream's bytes are present and never read.  Host or device memory as `flags` says.
 * dspi_mixed_pcm_bytes gives the buffer's size (*total_bytes, may be NULL) and the n_streams + 1 offsets (may be NULL) for a depth vector;
 * it works on host-only contexts.  Outputs, flags, the three memory paths, asynchrony, the S/PDIF and PDM bookkeeping and "a failed call
 * changes nothing" are exactly those of dspi_process / dspi_process_pdm.
 *
 * WHY THIS IS EXACT.  A 16-bit sample s and the 24-bit sample s << 8 go through the firmware's arithmetic identically, so the library
 * widens the 16-bit runs (s becomes the bytes 00 lo hi) in front of the unchanged 24-bit chain:
 *   float (usb_audio.c:601-603 against :680-681)   the gains are 2^-23 p and 2^-15 p (p: the channel's preamp); (float)(s << 8) =
 *         256 (float)s exactly; both products are therefore roundings of the same real number — while both gains are exact, which they
 *         are while 2^-23 p is a normal binary32: p >= 2^-103.
 *   Q28 (usb_audio.c:1001-1002 against :1010-1011)   the 24-bit route is (s24 << 8) >> 2; (s16 << 8) through it equals s16 << 14, the
 *         16-bit route.
 * The one case where the identity fails is refused: update_preamp (usb_audio.c:244-250) does not clamp, and a preamp below 2^-103 (about
 * -620 dB) makes the 24-bit gain subnormal.
 *
 * REFUSALS, each before anything is written or advanced, in this order:
 *   DSPI_E_INVAL        a NULL pointer (ctx, pcm_in, bit_depths, out); a depth that is neither 16 nor 24; n_blocks, block_len or a flag bit
 *                       that dspi_process refuses.
 *   DSPI_E_UNSUPPORTED  on a float context, an ACTIVE 16-bit stream whose parameter object has a preamp p with 0 < p < 2^-103 on either input
 *                       channel; dspi_last_error names the stream.  24-bit streams, paused streams and Q28 contexts are never refused for this.
 *   DSPI_E_NODEVICE     a host-only context.
 * UNIFORM DEPTHS: when every entry is equal the call IS dspi_process / dspi_process_pdm at that depth — no widening pass, no scratch, no
 * preamp refusal.  Otherwise: device buffers go through one more launch (dspi_intake.hip) into a scratch of n_streams * 6F bytes that the
 * context owns (DSPI_E_NOMEM all-or-nothing); small host calls widen on the CPU while copying into the pinned area, no extra launch; large
 * host calls upload each chunk's bytes as they are and widen on the device.
 * The ABI stays 8: detect by symbol (dspi_process_mixed; with it dspi_mixed_pcm_bytes; additions only). */
int dspi_mixed_pcm_bytes(const dspi_ctx *ctx, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,
                         uint64_t *total_bytes, uint64_t *offsets /* [n_streams + 1] or NULL */);
int dspi_process_mixed(dspi_ctx *ctx, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,
                       const dspi_out *out, uint32_t *pdm_words /* NULL: as dspi_process; else as dspi_process_pdm */, uint32_t flags);

/* ---- S/PDIF subframes ---------------------------------------------------- */
/* What the firmware's S/PDIF outputs do to the words of dspi_out.pairs before the PIO shifts them out
 * (pico_audio_spdif_multi: spdif_update_subframe, sample_encoding.h:27-47; preambles Z/X/Y, consumer channel status with
 * the sample-rate byte of stream 0's current rate, 192-frame block position: audio_spdif.c:76-116, :250-256, :385-405).
 *   pairs      int32 [stream][pair][n_frames][2]       exactly what dspi_process wrote
 *   subframes  uint32 [stream][pair][n_frames][4]      {l, h} of the left subframe, {l, h} of the right one: the 16 bytes
 *                                                      the firmware's DMA buffer holds per stereo frame
 * With DSPI_OUT_TILED: pairs = [tile][output][n_frames][R], subframes = [tile][pair][n_frames][4][R].
 * block_pos = position of the first frame in the 192-frame channel-status block (0..191).  Returns the position that
 * follows the last frame (>= 0; feed it to the next call) or a negative DSPI_E_*. */
int dspi_spdif_encode(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, uint32_t block_pos, uint32_t *subframes, uint32_t flags);
/* DSPI_OUT_SPDIF: the position in the 192-frame block of the next dspi_process call's first frame (0 after dspi_create, then advanced by
 * every call made with the flag).  set in 0..191 sets it first; set < 0 only reads.  Returns the position or a negative DSPI_E_*. */
int dspi_spdif_block_pos(dspi_ctx *ctx, int32_t set);
/* ---- per-stream S/PDIF block positions: for contexts whose devices come and go ------------------------------------------------------ */
/* One position per context is right while every stream takes part in every call from dspi_create on.  A paused device shifts nothing out
 * and must continue its block where its last frame left it; a device made by dspi_boot_streams starts a block; a stream moved or migrated
 * from elsewhere has a history of its own.  The Z preamble and the 40 channel-status bits are addressed by position, so a receiver of a
 * stream stamped with its neighbours' position sees blocks of the wrong length and a torn channel status.
 * Per-stream positions are a MODE OF THE CONTEXT, off after dspi_create.  Off, every call behaves and performs as it always did.
 *
 * dspi_spdif_per_stream(ctx, enable)   enable < 0 only reads.  enable = 1 while off: every stream's position becomes the context's current
 *                       one (dspi_spdif_block_pos), so turning the mode on in mid-run changes no word; while on: nothing changes.
 *                       enable = 0: the per-stream positions are dropped.  Returns the mode after the call (0 / 1) or a negative DSPI_E_*.
 *                       Works on host-only contexts.  In BOTH modes the context's own value goes on advancing with every DSPI_OUT_SPDIF
 *                       call exactly as before (all-paused calls included), and dspi_spdif_block_pos reads and sets that value; while the
 *                       mode is on it is not used for encoding.
 * dspi_spdif_stream_pos(ctx, first, count, set, get)   mode on only (off: DSPI_E_INVAL).  set (may be NULL): count values, each 0..191,
 *                       for streams [first, first + count); get (may be NULL): the positions after the set — for each stream the position
 *                       of the first frame of its next DSPI_OUT_SPDIF call.  Host memory always.  Everything is validated before anything
 *                       is written: a range past dspi_num_streams, a count of 0 or a value >= 192 is DSPI_E_INVAL and leaves the context
 *                       as it was.  Returns count.  Works on host-only contexts.
 * With the mode on:
 *   dspi_process        with DSPI_OUT_SPDIF, frame f of stream s is encoded at (pos_s + f) mod 192, and after a successful call pos_s has
 *                       advanced by the call's frames for every stream that was ACTIVE in it.  Paused streams keep theirs, a failed call
 *                       moves nobody, calls without the flag move nobody.  Such calls always run in two passes — the chain's pair words
 *                       into a scratch, then the subframe encoder —, the launches of the latency layout too, whose fused encoder knows one
 *                       position per launch (a fused per-stream encoder is left out; profiles/spdif_pos.md has the price).  So with
 *                       DSPI_OUT_ENABLED_ONLY the silent pairs carry the subframes of silence at the stream's own position.
 *   pause / resume      the position freezes and continues from the frozen value.  It is never realigned: it is the device's own
 *                       counter, not a property of the row.
 *   dspi_move_streams   the position travels with the stream, for all entries at once: pos[dst] := old pos[src].  An open-end source
 *                       keeps its value as a frozen copy.
 *   dspi_boot_streams   the listed slots go to 0, with and without DSPI_BOOT_STREAMS_AS_IS; the first frame after the boot carries preamble Z.
 *   snapshots           the position does not travel and an import leaves the slot's position alone (see the snapshot section).
 *   untouched           dspi_realign_streams, dspi_pdm_modulate, dspi_i2s_encode, dspi_spdif_encode.
 *
 * dspi_spdif_encode_v is dspi_spdif_encode with one starting position per stream: block_pos = uint32 [dspi_num_streams] (with
 * DSPI_OUT_TILED too: the position of tile t, column c is block_pos[t * R + c]; columns past dspi_num_streams have none and are not
 * encoded), host memory without DSPI_MEM_DEVICE and device memory with it, like the other two pointers.  Host values are validated
 * (each < 192, else DSPI_E_INVAL) before anything is launched; device values are taken modulo 192.  Stateless, independent of the mode and
 * unaware of pauses, like dspi_spdif_encode; the sample-rate byte is per stream as there.  Flags other than DSPI_MEM_DEVICE and
 * DSPI_OUT_TILED are refused.  Returns DSPI_OK or a negative DSPI_E_*; the next positions, (block_pos[s] + n_frames) mod 192, are the
 * caller's arithmetic. */
int dspi_spdif_per_stream(dspi_ctx *ctx, int enable);
int dspi_spdif_stream_pos(dspi_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *set, uint32_t *get);
int dspi_spdif_encode_v(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos, uint32_t *subframes, uint32_t flags);
/* ---- I2S slots ----------------------------------------------------------- */
/* An output slot switched to I2S (REQ_SET_OUTPUT_TYPE 0xC0 / output_types[] of a preset, config.h:286-287) takes the same
 * words as an S/PDIF slot and left-justifies them into 32-bit I2S slots, L then R, MSB first on the wire
 * (pico_audio_i2s_multi/audio_i2s_multi.c:217-226: dst = src << 8).
 *   pairs  int32  [stream][pair][n_frames][2]   exactly what dspi_process wrote        (DSPI_OUT_TILED: [tile][output][n_frames][R])
 *   words  uint32 [stream][pair][n_frames][2]   same shape; only the pairs in pair_mask (bit p = pair p) are written
 * pair_mask = DSPI_I2S_PAIRS_BY_TYPE (0): the pairs whose current output type is I2S in stream 0's parameters (the type of a
 * slot is a property of the device, like the sample rate).  Returns the mask that was encoded (>= 0) or a negative DSPI_E_*. */
#define DSPI_I2S_PAIRS_BY_TYPE 0u
/* ---- S/PDIF and I2S slots in one call, per device ------------------------------------------------------------------------------------ */
/* The driver a pair's words are for is a property of the DEVICE, per slot: output_types[slot], set by REQ_SET_OUTPUT_TYPE 0xC0 and carried
 * by presets (config.h:286-287, main.c:230-424).  DSPI_OUT_SPDIF, DSPI_OUT_I2S_SLOTS and dspi_i2s_encode's DSPI_I2S_PAIRS_BY_TYPE take it
 * from the call or from stream 0; the two calls below take it from every stream's OWN parameters, so a context whose devices differ in
 * their types (slots 0-1 on S/PDIF and 2-3 on I2S here, all I2S there) gets what its drivers shift out from one call.
 *
 * THE WIRE LAYOUT has the size and the regions of DSPI_OUT_SPDIF: pair p of stream s owns the 16 F bytes at word offset
 * ((s * P + p) * F) * 4, F = the call's frames, P = dspi_num_pairs.
 *   S/PDIF slot   uint32 [F][4], exactly DSPI_OUT_SPDIF's subframes: the block position is the context's, or the stream's own while
 *                 dspi_spdif_per_stream is on; the sample-rate byte is the stream's own.
 *   I2S slot      (output_types[p] == 1)  uint32 [F][2], word << 8, L then R, in the FIRST 8 F bytes of the region: the words of dspi_i2s_encode
 *                 / DSPI_OUT_I2S_SLOTS, contiguous as a DMA buffer wants them.  The LAST 8 F bytes of the region are never written in a
 *                 caller's device buffer (DSPI_MEM_DEVICE) and come back as zeros in host buffers.
 *   paused stream the existing rule: its regions are untouched in device buffers and zero in host buffers.
 * A tiled wire layout is left out: both calls refuse DSPI_OUT_TILED.  (Of THESE two calls that stays true; the tiled wire layout and the
 * calls that take it, dspi_process_devices and dspi_wire_encode_tiled, have the section below.)
 *
 * dspi_process_wire is dspi_process (pdm_words NULL) or dspi_process_pdm (else, out->sub optional as there) with out->pairs in the wire
 * layout.  Flags: DSPI_MEM_DEVICE, DSPI_OUT_ENABLED_ONLY, DSPI_OUT_CLIP_FLAGS.  Refused with DSPI_E_INVAL before anything else is looked
 * at: DSPI_OUT_SPDIF (it is implied), DSPI_OUT_I2S_SLOTS, DSPI_OUT_TILED and every undefined bit; then the refusals of dspi_process in
 * their order (DSPI_E_INVAL for its arguments, DSPI_E_NODEVICE on a host-only context).  A refused or failed call writes and advances
 * nothing.  The block positions move exactly as for a DSPI_OUT_SPDIF call: the context's value by F, with dspi_spdif_per_stream on every
 * ACTIVE stream's by F — a device whose slots are all I2S counts on too: the position is the device's frame counter.
 * WHEN NO ACTIVE STREAM'S PARAMETER OBJECT HAS AN I2S SLOT the call IS dspi_process / dspi_process_pdm with DSPI_OUT_SPDIF: the same route
 * (the latency layout's fused encoder included), the same bytes.  Otherwise it runs in two passes, as per-stream positions make a
 * DSPI_OUT_SPDIF call run: the chain's pair words into a scratch, then the wire encoder; with DSPI_OUT_ENABLED_ONLY the silent pairs then
 * carry silence in their own format, the subframes of silence at the stream's position or zero slot words.
 * Not combined with dspi_process_mixed.
 *
 * dspi_wire_encode is the stateless twin (as dspi_spdif_encode_v is DSPI_OUT_SPDIF's): pairs = int32 [stream][pair][n_frames][2] exactly
 * as dspi_process wrote them, block_pos = uint32 [dspi_num_streams], required, wire = the layout above; all three in host memory, or in
 * device memory with DSPI_MEM_DEVICE, the only flag.  Host positions are validated (each < 192, else DSPI_E_INVAL) before anything is
 * launched; device positions are taken modulo 192.  Every stream's types and rate are its own parameters' at the time of the call.
 * Independent of the per-stream mode, unaware of pauses.  Returns DSPI_OK or a negative DSPI_E_*.
 * The ABI stays 8: detect by symbol (dspi_process_wire; with it dspi_wire_encode; additions only). */
int dspi_process_wire(dspi_ctx *ctx, const void *pcm_in, int bit_depth, uint32_t n_blocks, uint32_t block_len,
                      const dspi_out *out, uint32_t *pdm_words /* may be NULL */, uint32_t flags);
int dspi_wire_encode(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos,
                     uint32_t *wire, uint32_t flags);
/* ---- wire words on tiled and mixed-depth contexts -------------------------------------------------------------------------------------- */
/* What a device's HOST decides — its sample rate, its preset, its input format (usb_input_bit_depth) and the driver behind each output slot
 * (output_types[]) — in ONE call, in either layout: dspi_process_devices has dspi_process_mixed's arguments (pcm_in, bit_depths: see there and
 * dspi_mixed_pcm_bytes) and dspi_process_wire's out->pairs.
 *
 * Flags: DSPI_MEM_DEVICE, DSPI_OUT_TILED, DSPI_OUT_ENABLED_ONLY, DSPI_OUT_CLIP_FLAGS.  Without DSPI_OUT_TILED out->pairs is THE WIRE LAYOUT
 * above.  With it out->pairs is THE TILED WIRE LAYOUT, and out->sub and pdm_words are tiled as in dspi_process_pdm.
 *
 * THE TILED WIRE LAYOUT has the size and the regions of dspi_spdif_encode_v's tiled subframes.  R = dspi_tile_streams, P = dspi_num_pairs,
 * F = the call's frames; stream s stands in tile t = s / R at column c = s % R.  Pair p of tile t owns 16 F R bytes, 4 F rows of R words, at
 * word offset ((t * P + p) * F) * 4 * R.  Column c of every row belongs to stream s, whose own type decides what stands there:
 *   S/PDIF slot   uint32 [F][4][R] at column c, exactly the tiled subframes of dspi_spdif_encode_v: word (f * 4 + j) * R + c.  The block
 *                 position is the context's, or the stream's own while dspi_spdif_per_stream is on; the sample-rate byte is the stream's own.
 *   I2S slot      (output_types[p] == 1)  uint32 [2][F][R] (side, frame) at column c in the FIRST HALF of the region: word
 *                 (side * F + f) * R + c, value word << 8 — for that column what dspi_i2s_encode with DSPI_OUT_TILED writes for outputs 2p
 *                 and 2p + 1, the two planes back to back.  The column's words in the second half, rows 2 F .. 4 F - 1, are the tail.
 *   no word reaches   an I2S column's tail, a paused stream's column and the columns past dspi_num_streams in the last tile: never written
 *                 in a caller's device buffer (DSPI_MEM_DEVICE), zeros in host buffers.
 * A consumer finds the words of stream s, pair p: region = ((s / R * P + p) * F) * 4 * R, column s % R, rows as above by the stream's type.
 *
 * A NULL ctx is refused first; then, before anything else is looked at, DSPI_OUT_SPDIF (it is implied), DSPI_OUT_I2S_SLOTS and every undefined
 * bit give DSPI_E_INVAL; then the refusals of dspi_process_mixed in their order, the preamp refusal for 16-bit streams (DSPI_E_UNSUPPORTED)
 * included.  A refused or failed call writes and advances nothing.  Block positions, per-stream positions, pauses, the PDM running byte and
 * fade, and the clip flags behave as in dspi_process_wire and dspi_process_pdm.
 *   stream-major, every depth equal                       the call IS dspi_process_wire at that depth: the same route, the same bytes.
 *   stream-major, no active stream holds an I2S slot      the call IS dspi_process_mixed with DSPI_OUT_SPDIF.
 *   tiled         every region holds, re-laid, the words of the stream-major call.  A tiled call ALWAYS runs in two passes, I2S slot or
 *                 not — the chain's tiled pair words into a scratch, then the tiled wire encoder; there is no fused tiled encoder —, so with
 *                 DSPI_OUT_ENABLED_ONLY its silent pairs carry silence in their own format, as on dspi_process_wire's two-pass route.
 *                 At most 2 097 120 frames per tiled call (DSPI_E_UNSUPPORTED above).
 *
 * dspi_wire_encode_tiled is the stateless twin: dspi_wire_encode on tiled pair words, pairs = int32 [tile][output][n_frames][R] exactly as
 * dspi_process wrote them with DSPI_OUT_TILED, wire = the tiled wire layout, block_pos = uint32 [dspi_num_streams], required, indexed by
 * stream (block_pos[t * R + c]) as in dspi_spdif_encode_v; all three in host memory, or in device memory with DSPI_MEM_DEVICE, the only
 * flag.  Host positions are validated (each < 192, else DSPI_E_INVAL) before anything is launched; device positions are taken modulo 192.
 * Independent of the per-stream mode, unaware of pauses.  At most 2 097 120 frames per call (DSPI_E_INVAL above).  Returns DSPI_OK or a
 * negative DSPI_E_*.
 * The ABI stays 8: detect by symbol (dspi_process_devices; with it dspi_wire_encode_tiled; additions only). */
int dspi_process_devices(dspi_ctx *ctx, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,
                         const dspi_out *out, uint32_t *pdm_words /* may be NULL */, uint32_t flags);
int dspi_wire_encode_tiled(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, const uint32_t *block_pos,
                           uint32_t *wire, uint32_t flags);

/* ---- S/PDIF input ------------------------------------------------------------------------------------------------------------------------ */
/* A device takes its audio from an S/PDIF receiver instead of USB, through the identical pipeline (the reference's
 * Documentation/Features/SPDIF_input_spec.md: 24-bit words, hold concealment on the validity bit, a 20-byte receiver status).  The firmware
 * tree has no receiver code, so what is fixed here is: the subframe exactly as the firmware's own encoder writes it (what dspi_spdif_encode
 * emits), the sample path (a decoded sample enters the chain as the 24-bit USB sample of the same value: "replaces USB audio at the entry
 * point"), and the receiver rules below.
 *
 * THE SUBFRAME (pico_audio_spdif_multi: sample_encoding.h:27-47, audio_spdif.c:77-94, :101-113, :141-153).  A frame is four words {l, h} left,
 * {l, h} right.  With cells = h:l (64 bits) time slot k owns bit 2k (the clock cell, 1 for k >= 4) and bit 2k + 1 (the data cell).
 *   preamble     l & 0xff: Z 0x39, X 0xC9 (left), Y 0x69 (right)
 *   sample       the data cells of slots 4..27, slot 4 = LSB, sign-extended from bit 23
 *   status bits  V = slot 28 (h bit 25), U = slot 29 (bit 27), C = slot 30 (bit 29), P = slot 31 (bit 31)
 *   parity       holds when the XOR of the data cells of slots 4..31 is 0
 * A subframe is WELL-FORMED when its preamble byte is Z or X (left) or Y (right), and (l & 0x55555500) == 0x55555500 and
 * (h & 0x55555555) == 0x55555555.
 *
 * THE RECEIVER: one record per stream, caller-owned, read and updated by every call.  A record of all zero bytes is a receiver just started.
 * Its first 20 bytes are the answer to REQ_GET_SPDIF_IN_STATUS (the spec's "Response (20 bytes)").  For each frame, in order:
 *   1. sync      left well-formed with Z: if sync != 1 this is a lock or re-lock and parity_err_count := 0; either way sync := 1.
 *                Left well-formed with X while sync == 1 (Z expected): sync := 0, sample_rate := 0.  Left not well-formed: the same loss.
 *                Then, right not well-formed: the same loss.
 *   2. each side, left then right.  Not well-formed: coding_errors++, the output is hold[side], held++.  Well-formed: a parity failure does
 *                parity_err_count++ and the sample still passes (the spec only counts).  Well-formed with V set: the output is hold[side],
 *                held++.  Otherwise the output is the sample and hold[side] := the sample.
 *   3. if sync != 0, with p = sync - 1: p < 40: bit p % 8 of c_bits[p / 8] := the left subframe's C; p == 31: sample_rate := 44100 / 48000 /
 *                88200 / 96000 / 176400 / 192000 for byte 3 = 0x00 / 02 / 08 / 0A / 0C / 0E, else 0; then sync := 1 + (p + 1) % 192.
 * At the end of the call state = 2 if sync != 0, else 1 if the call held any well-formed subframe, else 0.  Counters wrap.  A host-memory
 * record with sync > 192 is DSPI_E_INVAL; a device-memory one is read as 0.
 * Out of scope: lock timing and watchdogs, the mute during a source switch, TX clock tracking, running the chain at 88.2 / 176.4 / 192 kHz
 * (reported, not settable), applying the detected rate (the caller calls dspi_set_sample_rate), receiver state
 * held by the context, serving 0x80-0x82 inside dspi_vendor_* (INTEGRATION.md says how a caller answers them). */
typedef struct dspi_spdif_rx {      /* 40 bytes; the first 20 are REQ_GET_SPDIF_IN_STATUS's answer */
    uint32_t state;                 /* 0 NO_SIGNAL, 1 ACQUIRING, 2 LOCKED: written at the end of every call */
    uint32_t sample_rate;           /* Hz from channel status byte 3, or 0 */
    uint32_t parity_err_count;      /* since the last lock */
    uint8_t  c_bits[5], pad_[3];
    int32_t  hold[2];               /* last good sample, left / right */
    uint32_t sync;                  /* 0: not locked; 1 + p: the next frame is expected at block position p (0..191) */
    uint32_t held;                  /* subframes concealed */
    uint32_t coding_errors;         /* subframes that were not well-formed */
} dspi_spdif_rx;
#define DSPI_SPDIF_RX_NO_SIGNAL 0u
#define DSPI_SPDIF_RX_ACQUIRING 1u
#define DSPI_SPDIF_RX_LOCKED 2u

/* dspi_spdif_decode: the inverse of dspi_spdif_encode, stateless per context (the state is the caller's records).
 *   subframes  uint32 [line][n_frames][4]      a whole stream-major S/PDIF output buffer is dspi_num_streams * dspi_num_pairs lines
 *   rx         dspi_spdif_rx [n_lines]         required, in/out
 *   pairs      int32 [line][n_frames][2]       the words dspi_out.pairs holds
 * All three in host memory, or in device memory with DSPI_MEM_DEVICE, the only flag (asynchronous on the context's stream then).
 * DSPI_E_INVAL: a NULL pointer, a zero count, sizes that overflow, another flag, a device pointer that is not 16-byte aligned, a host record
 * with sync > 192; then DSPI_E_NODEVICE on a host-only context.  A refused call writes nothing.  Returns DSPI_OK or a negative DSPI_E_*. */
int dspi_spdif_decode(dspi_ctx *ctx, const uint32_t *subframes, uint32_t n_lines, uint32_t n_frames, dspi_spdif_rx *rx, int32_t *pairs, uint32_t flags);

/* dspi_process_sources: dspi_process_mixed with one SOURCE per stream instead of one depth.
 *   sources   uint8 [dspi_num_streams], HOST memory always: DSPI_SRC_PCM16, DSPI_SRC_PCM24 or DSPI_SRC_SPDIF (a paused stream's too: its
 *             entry sizes its slot)
 *   in        every stream's run of F = n_blocks * block_len frames at 4, 6 or 16 bytes per frame, back to back as in dspi_process_mixed,
 *             except that an S/PDIF run starts at the next multiple of 16: offset[s] = offset[s - 1] + F * size[s - 1], rounded up to 16 when
 *             sources[s] is DSPI_SRC_SPDIF.  An S/PDIF run holds the subframes uint32 [F][4] of ONE line (e.g. one pair of another context's
 *             DSPI_OUT_SPDIF output).  A paused stream's bytes are never read.  dspi_sources_bytes gives the size (*total_bytes, may be
 *             NULL) and the n_streams + 1 offsets (may be NULL); it works on host-only contexts.
 *   rx        dspi_spdif_rx [dspi_num_streams], in host or device memory like the other pointers; required when any source is S/PDIF (else
 *             it may be NULL).  Only the entries of ACTIVE S/PDIF streams are read or written.
 * A decoded sample enters the chain as the 24-bit USB sample of the same value.  There is no preamp refusal for S/PDIF streams; 16-bit
 * streams keep dspi_process_mixed's.
 * Flags: dspi_process_mixed's, and DSPI_OUT_WIRE, defined for this call only: out->pairs is THE WIRE LAYOUT (with DSPI_OUT_TILED the tiled
 * one) with the meaning and the flag refusals of dspi_process_devices.  Outputs, pauses, block positions, PDM bookkeeping and clip flags
 * behave as in those calls.
 * REFUSALS in dspi_process_mixed's order (with DSPI_OUT_WIRE: dspi_process_devices' flag rule first): DSPI_E_INVAL for a NULL pointer (ctx,
 * in, sources, out), a source value that is none of the three, n_blocks / block_len / flag bits that dspi_process refuses, and — with an
 * S/PDIF source present — a NULL rx, a host record of an active S/PDIF stream with sync > 192, a device `in` that is not 16-byte aligned, a
 * device rx that is not 4-byte aligned, a size that overflows; then the preamp's DSPI_E_UNSUPPORTED; then DSPI_E_NODEVICE.  A refused or
 * failed call writes nothing, and no host record changes.
 * EQUIVALENCES: with no S/PDIF source the call IS dspi_process_mixed, with DSPI_OUT_WIRE dspi_process_devices (route, bytes and layout are
 * the same); with uniform PCM sources it IS dspi_process.  Otherwise: device buffers take one more launch (dspi_spdifrx.hip) into the
 * scratch the mixed path owns; small host calls decode on the CPU while copying into the pinned area; large host calls upload each
 * chunk's bytes as they are and decode on the device.
 * The ABI stays 8: detect by symbol (dspi_process_sources; with it dspi_spdif_decode, dspi_sources_bytes; additions only). */
#define DSPI_SRC_SPDIF 1
#define DSPI_SRC_PCM16 16
#define DSPI_SRC_PCM24 24
#define DSPI_OUT_WIRE 0x40u        /* dspi_process_sources only: out->pairs in the wire layout, as dspi_process_devices writes it */
int dspi_sources_bytes(const dspi_ctx *ctx, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len,
                       uint64_t *total_bytes, uint64_t *offsets /* [n_streams + 1] or NULL */);
int dspi_process_sources(dspi_ctx *ctx, const void *in, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len,
                         const dspi_out *out, uint32_t *pdm_words /* may be NULL */, dspi_spdif_rx *rx, uint32_t flags);
/* ---- chained devices: input from another context's wire words ------------------------------------------------------------------------------ */
/* A context's input may be another call's OUTPUT, read where it lies: a VIEW names a buffer some call wrote through out->pairs in THE WIRE LAYOUT
 * (tile_streams == 0) or THE TILED WIRE LAYOUT (above), and a LINK names one line of it, pair p of producer stream s, and says which of the two
 * word formats its region holds.  No copy, no gather in front of the call: dspi_process_devices(A, ...); dspi_process_linked(B, ...);
 *
 * THE WORDS OF A LINK.  L = the link's line, s = L / P, p = L % P, P = view->n_pairs, F = view->n_frames, R = view->tile_streams.
 *   stream-major   the region starts at word (L * F) * 4.
 *                  S/PDIF: frame f, word j (of {l, h} left, {l, h} right) is at + f * 4 + j.     I2S: frame f, side k is at + f * 2 + k.
 *   tiled          the region starts at word ((s / R * P + p) * F) * 4 * R, the column is c = s % R.
 *                  S/PDIF: word (f * 4 + j) * R + c.                                            I2S: word (k * F + f) * R + c.
 * These are the two layouts above, read backwards.  An I2S word decodes to (int32_t)word >> 8, an arithmetic shift; the low byte is ignored;
 * no record is read or written.  An S/PDIF line goes through THE RECEIVER (S/PDIF input, above), unchanged, with the caller's record for that
 * link.  A decoded sample enters the chain as the 24-bit USB sample of the same value.
 *
 * dspi_wire_view_of fills *view from a producer context: n_streams, n_pairs, tile_streams (0, or dspi_tile_streams with flags = DSPI_OUT_TILED; any
 * other flag is DSPI_E_INVAL), n_frames and wire as given, producer = the context itself.  dspi_link_kinds sets links[i].kind for i < n from the
 * producer's CURRENT output_types[] of the line links[i].line: DSPI_LINK_I2S where the slot's type is 1, else DSPI_LINK_SPDIF (a line that is
 * not the producer's: DSPI_E_INVAL, nothing written).  Both are bookkeeping only and work on host-only contexts.
 *
 * dspi_wire_decode is the stateless inverse of dspi_wire_encode / dspi_wire_encode_tiled.
 *   links     dspi_link [n_links], HOST memory always.  An entry of kind DSPI_LINK_NONE is skipped: its pair words and its record are untouched.
 *             Several links may name one line (a splitter); each has its own record.
 *   rx        dspi_spdif_rx [n_links], in/out; required only if a link is S/PDIF.  Only S/PDIF links' entries are read or written.
 *   pairs     int32 [n_links][F][2]
 * view->wire, rx and pairs in host memory, or in device memory with DSPI_MEM_DEVICE, the only flag (asynchronous on the context's stream then;
 * view->producer is not looked at: the caller orders the work).  DSPI_E_INVAL, in this order: a NULL ctx, view, links or pairs or n_links == 0;
 * another flag; the view (as in dspi_process_linked, n_frames != 0 in place of its F); a link whose kind is none of the three or, unless its
 * kind is NONE, whose line >= n_streams * n_pairs; a NULL rx where a link is S/PDIF; with DSPI_MEM_DEVICE an rx or pairs that is not 16-byte
 * aligned; a host record of an S/PDIF link with sync > 192; then DSPI_E_NODEVICE on a host-only context.  A refused call writes nothing.
 *
 * dspi_process_linked is dspi_process_sources in which stream s' of ctx takes its F = n_blocks * block_len frames from links[s'] in *view
 * instead of from a run in `in`.
 *   flags     DSPI_MEM_DEVICE is REQUIRED: the view, rx and everything in *out are device memory (a chained context's input is another
 *             context's output buffer).  Beyond that exactly the flags of dspi_process_sources, DSPI_OUT_WIRE and DSPI_OUT_TILED included, so
 *             ctx can be someone else's producer.
 *   links     dspi_link [dspi_num_streams], HOST memory always.  Every ACTIVE stream needs a link of kind S/PDIF or I2S; a paused stream's entry
 *             is ignored: nothing of a paused stream is read or written, and its record is untouched.
 *   rx        dspi_spdif_rx [dspi_num_streams], required if an active stream's link is S/PDIF; only those entries are read or written (a
 *             record with sync > 192 is read as 0).
 *   view      view->n_frames == F; view->wire must not overlap out->pairs of the same call.
 * Outputs, pauses, block positions, PDM bookkeeping and clip flags behave as in dspi_process_sources.  No preamp refusal: no stream is 16-bit.
 * No state is added to the context: records and links are the caller's; snapshots, moves, migrations and resizes know nothing of them.
 * REFUSALS, in this order (a refused call writes nothing):
 *   1. DSPI_E_INVAL   a NULL ctx, view, links or out
 *   2. DSPI_E_INVAL   DSPI_MEM_DEVICE missing; then dspi_process_sources' own flag rule
 *   3. DSPI_E_INVAL   n_blocks / block_len as dspi_process refuses them
 *   4. DSPI_E_INVAL   the view: a NULL wire or one that is not 16-byte aligned, n_pairs not 2 or 4, tile_streams not 0 / 64 / 128,
 *                     n_streams == 0, n_frames != F, a size that overflows 64 bits
 *   5. DSPI_E_INVAL   a link of an active stream whose kind is neither S/PDIF nor I2S, or whose line >= n_streams * n_pairs
 *   6. DSPI_E_INVAL   rx NULL, or not 4-byte aligned, where an active stream's link is S/PDIF
 *   7. DSPI_E_INVAL   view->producer on another HIP device than ctx (a host-only producer has none)
 *   8. DSPI_E_NODEVICE on a host-only context
 * ORDERING.  With view->producer set and != ctx the call records an event on the producer's HIP stream and makes its own stream wait for it
 * before the first kernel that reads view->wire: a chain needs no dspi_sync between the producer's call and this one.  The event is created
 * once per context and destroyed with it.  With producer == ctx, or NULL, nothing is recorded: the stream is the same, or the caller orders
 * the work itself.
 * The ABI stays 8: detect by symbol (dspi_process_linked; with it dspi_wire_decode, dspi_wire_view_of, dspi_link_kinds; additions only). */
#define DSPI_LINK_NONE  0u
#define DSPI_LINK_SPDIF 1u      /* == DSPI_SRC_SPDIF: the region holds subframes */
#define DSPI_LINK_I2S   2u      /* the region holds I2S slot words, word << 8, in its first half */
typedef struct dspi_wire_view {     /* a buffer some call wrote through out->pairs in a wire layout */
    const uint32_t *wire;           /* THE WIRE LAYOUT (tile_streams == 0) or THE TILED WIRE LAYOUT; 16-byte aligned when in device memory */
    uint32_t n_streams;             /* the producer's dspi_num_streams at that call */
    uint32_t n_pairs;               /* its dspi_num_pairs: 4 / 2 */
    uint32_t tile_streams;          /* 0, or its dspi_tile_streams: 128 / 64 */
    uint32_t n_frames;              /* F of that call */
    dspi_ctx *producer;             /* NULL, or the context on whose HIP stream `wire` is being written: ORDERING above */
} dspi_wire_view;
typedef struct dspi_link { uint32_t line; uint32_t kind; } dspi_link;   /* line = producer stream * n_pairs + pair */
int dspi_wire_view_of(const dspi_ctx *producer, const uint32_t *wire, uint32_t n_frames, uint32_t flags /* 0 or DSPI_OUT_TILED */, dspi_wire_view *view);
int dspi_link_kinds(const dspi_ctx *producer, dspi_link *links, uint32_t n);
int dspi_wire_decode(dspi_ctx *ctx, const dspi_wire_view *view, const dspi_link *links, uint32_t n_links,
                     dspi_spdif_rx *rx, int32_t *pairs, uint32_t flags);
int dspi_process_linked(dspi_ctx *ctx, const dspi_wire_view *view, const dspi_link *links /* [dspi_num_streams], HOST memory always */,
                        uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words /* may be NULL */,
                        dspi_spdif_rx *rx, uint32_t flags);
/* ---- the patch bay: USB, S/PDIF and linked inputs in one call --------------------------------------------------------------------------------- */
/* dspi_process_patched is the union of dspi_process_sources and dspi_process_linked: every stream takes its F = n_blocks * block_len frames from
 * wherever it is plugged in — a run of `in`, or one line of one of up to DSPI_MAX_VIEWS views — in one call.
 *   sources   uint8 [dspi_num_streams], HOST memory always: DSPI_SRC_PCM16, DSPI_SRC_PCM24, DSPI_SRC_SPDIF or DSPI_SRC_LINK.  The first three
 *             mean exactly what they mean in dspi_process_sources.  DSPI_SRC_LINK: the stream's words are in somebody's wire buffer.
 *             dspi_sources_bytes and dspi_process_sources keep refusing the value 2.
 *   in        the runs of dspi_process_sources, except that a LINK stream occupies ZERO bytes of `in`: offset[s] = offset[s - 1] + F * size[s - 1]
 *             with size 4, 6, 16 or 0, rounded up to 16 when sources[s] is DSPI_SRC_SPDIF.  dspi_patched_bytes is dspi_sources_bytes with that
 *             one extra rule (*total_bytes and the n_streams + 1 offsets, either may be NULL); it works on host-only contexts.  A paused
 *             stream's entry still sizes its slot; its bytes are never read.  `in` may be NULL when no active stream has a run.
 *   views     dspi_wire_view [n_views], HOST memory always, 1 <= n_views <= DSPI_MAX_VIEWS, each as in dspi_process_linked, of either layout
 *             and any tile size, mixed freely.  A view that no active LINK stream names is not looked at beyond its validation.
 *   patches   dspi_patch [dspi_num_streams], HOST memory always.  patches[s] is read only for an ACTIVE stream whose source is DSPI_SRC_LINK:
 *             views[patches[s].view] is its view, line and kind are dspi_link's, and the words of the link lie where THE WORDS OF A LINK puts
 *             them.  An S/PDIF link goes through THE RECEIVER with rx[s]; an I2S link is word >> 8 with no record.  Any map and any fan-out is
 *             allowed, across views too.  views and patches may be NULL when no active stream is a LINK stream.
 *   rx        dspi_spdif_rx [dspi_num_streams], device memory; required when any active stream is an S/PDIF run or an S/PDIF link.  Only those
 *             streams' entries are read or written (a record with sync > 192 is read as 0).
 *   flags     DSPI_MEM_DEVICE is REQUIRED, as on dspi_process_linked: in, the views, rx and everything in *out are device memory.  Beyond that
 *             exactly the flags of dspi_process_sources, DSPI_OUT_WIRE and DSPI_OUT_TILED included.
 * Outputs, pauses, block positions, PDM bookkeeping and clip flags behave as in dspi_process_sources.  The preamp refusal applies to PCM16
 * streams.  No state is added to the context: records, views and patches are the caller's.
 * ORDERING.  For every DISTINCT views[v].producer that is non-NULL, is not ctx, and is named by an active LINK stream, the call records an event
 * on that producer's HIP stream and makes its own stream wait for it before the first kernel that reads that view.  With producer == ctx or
 * NULL nothing is recorded: with producer == ctx stream s may eat what another stream of ctx put on its wire in the PREVIOUS call (two wire
 * buffers, used alternately).  No view's wire may overlap out->pairs of the same call.
 * REFUSALS, in this order (a refused call writes nothing, and no record changes):
 *   1. DSPI_E_INVAL   a NULL ctx, sources or out
 *   2. DSPI_E_INVAL   DSPI_MEM_DEVICE missing; then dspi_process_sources' own flag rule
 *   3. DSPI_E_INVAL   n_blocks / block_len as dspi_process refuses them
 *   4. DSPI_E_INVAL   a source value that is none of the four
 *   5. DSPI_E_INVAL   when an active stream is a LINK stream: views or patches NULL, n_views == 0 or n_views > DSPI_MAX_VIEWS; then EVERY view
 *                     among the n_views by dspi_process_linked's rule 4, lowest index first; then each such stream, lowest first: view >=
 *                     n_views, a kind that is neither S/PDIF nor I2S, line >= n_streams * n_pairs of its view
 *   6. DSPI_E_INVAL   in NULL, or not 16-byte aligned, where an active stream has a run
 *   7. DSPI_E_INVAL   rx NULL, or not 4-byte aligned, where it is required
 *   8. DSPI_E_INVAL   a size that overflows 64 bits
 *   9. DSPI_E_UNSUPPORTED   the preamp's refusal (dspi_process_mixed)
 *  10. DSPI_E_INVAL   the producer of a view that an active LINK stream names is on another HIP device than ctx
 *  11. DSPI_E_NODEVICE on a host-only context
 * EQUIVALENCES, for outputs and records alike, byte for byte: with no active LINK stream the call IS dspi_process_sources on device buffers;
 * with every active stream a LINK stream and one view it IS dspi_process_linked.  Otherwise a call costs at most one intake launch, one receiver
 * launch over `in`, two launches per stream-major view and ONE launch for all tiled views (dspi_patchrx.hip) in front of the 24-bit chain.
 * The ABI stays 8: detect by symbol (dspi_process_patched; with it dspi_patched_bytes; additions only). */
#define DSPI_SRC_LINK 2            /* dspi_process_patched / dspi_patched_bytes only */
#define DSPI_MAX_VIEWS 8
typedef struct dspi_patch { uint32_t view; uint32_t line; uint32_t kind; } dspi_patch;   /* 12 bytes; line and kind as in dspi_link, view < n_views */
int dspi_patched_bytes(const dspi_ctx *ctx, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len,
                       uint64_t *total_bytes, uint64_t *offsets /* [n_streams + 1] or NULL */);
int dspi_process_patched(dspi_ctx *ctx, const void *in, const uint8_t *sources,
                         const dspi_wire_view *views, uint32_t n_views, const dspi_patch *patches /* [dspi_num_streams], HOST memory always */,
                         uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words /* may be NULL */,
                         dspi_spdif_rx *rx, uint32_t flags);
/* ---- input from a packet table, in arrival order ------------------------------------------------------------------------------------------- */
/* dspi_process_packets is dspi_process_mixed with each stream's frames taken packet by packet from where a table points: the packets stay
 * in the arena they were received into, and the library gathers them as it widens them.
 *   arena     DEVICE memory, arena_bytes long, 2-byte aligned: the received packets, anywhere, in any order, with anything in between.
 *   table     uint64 [dspi_num_streams][n_blocks], HOST memory always (like bit_depths and links).  table[s * n_blocks + k] is the byte offset in
 *             arena of packet k of stream s: block_len frames of 4 bytes (bit_depths[s] == 16) or 6 (24), interleaved LE stereo.  The table goes
 *             up with the call, through the context's pinned area: the caller may reuse its table when the call returns.
 *   flags     DSPI_MEM_DEVICE is REQUIRED: arena and everything in *out are device memory; table and bit_depths are host memory.  The call is
 *             asynchronous on the context's stream like every device call.  Beyond that exactly the flags of dspi_process_sources: with
 *             DSPI_OUT_WIRE, under dspi_process_devices' flag rule, out->pairs is the wire layout, with DSPI_OUT_TILED the tiled one.
 * AN ENTRY IS LEGAL when it is even and offset + block_len * frame bytes <= arena_bytes.  Entries may be equal and may overlap in any way:
 * one programme to many devices (every stream's entries name the same packets), a packet repeated to conceal a lost one, a sliding window.
 * Entries of PAUSED streams are neither read nor checked: they may hold anything.  Nothing outside [offset, offset + length) of an active
 * stream's entries is read from the arena: neighbouring bytes may lie outside the caller's allocation.
 * Outputs, pdm_words, the clip flags, pauses, block positions and the state all behave as in dspi_process_mixed: the call IS
 * dspi_process_mixed on the input that the table describes, byte for byte (uniform depths included).  No state is added to the context:
 * snapshots, moves, migrations and resizes are unaffected.
 * REFUSALS, in this order (a refused call writes nothing and changes nothing):
 *   1. DSPI_E_INVAL   a NULL ctx; DSPI_MEM_DEVICE missing; then dspi_process_sources' own flag rule
 *   2. DSPI_E_INVAL   a NULL arena, table, bit_depths or out; n_blocks == 0 or block_len == 0; block_len > DSPI_MAX_BLOCK_LEN, as
 *                     dspi_process_mixed refuses it
 *   3. DSPI_E_INVAL   a depth that is neither 16 nor 24 (any stream, paused or not, lowest first)
 *   4. DSPI_E_INVAL   a table of more than 2^31 - 1 entries: dspi_num_streams * n_blocks
 *   5. DSPI_E_INVAL   the first illegal entry of an active stream, in table order; the message names its index s * n_blocks + k
 *   6. DSPI_E_UNSUPPORTED   the preamp's refusal for active 16-bit streams, exactly as in dspi_process_mixed
 *   7. DSPI_E_NODEVICE on a host-only context
 * dspi_packets_check applies refusals 2 to 5 (no arena, no out) and works on host-only contexts; at refusal 5 *bad_entry, when not NULL, takes
 * s * n_blocks + k of the entry refused, and is not written otherwise.
 * LEFT OUT: arenas in host memory; tables in device memory; S/PDIF and linked sources in the same call (the patch bay keeps those); a
 * packet-table OUTPUT (a packetiser); per-packet lengths (block_len is one number per call); an option of dspi_host.
 * (Tables in device memory are left out of THIS call only: dspi_process_packets_resident, "resident packet tables" below, takes them.)
 * The ABI stays 8: detect by symbol (dspi_process_packets; with it dspi_packets_check; additions only). */
int dspi_packets_check(const dspi_ctx *ctx, const uint8_t *bit_depths, const uint64_t *table, uint32_t n_blocks, uint32_t block_len,
                       uint64_t arena_bytes, uint64_t *bad_entry /* may be NULL: s * n_blocks + k of the first entry refused */);
int dspi_process_packets(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table,
                         uint32_t n_blocks, uint32_t block_len, const dspi_out *out, uint32_t *pdm_words /* may be NULL */, uint32_t flags);
int dspi_i2s_encode(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_frames, uint32_t pair_mask, uint32_t *words, uint32_t flags);
/* the HIP stream (hipStream_t) the context launches on, for event timing by the caller */
void *dspi_hip_stream(dspi_ctx *ctx);

/* ---- status ------------------------------------------------------------------------------ */
/* REQ_GET_STATUS wValue 9: peaks[C] LE u16, cpu0, cpu1 (always 0 here), clip_flags LE u16 = 26 / 18 bytes */
int dspi_get_status(dspi_ctx *ctx, int32_t stream, void *buf, size_t cap);
/* REQ_CLEAR_CLIPS: returns the flags that were set (DSPI_ALL_STREAMS: clears every stream, returns stream 0's flags) */
int dspi_clear_clips(dspi_ctx *ctx, int32_t stream);

/* ---- the meter bridge: meter ballistics, alarms and status for every stream of a context ----------------------------------------------- */
/* The peaks a process-family call writes through out->peaks are instantaneous block peaks, one per packet and channel: no decay, no hold —
 * ballistics are the host application's (the firmware's metering spec), and the two calls above serve one device at a time.  These four
 * calls are that host's side for a whole context: they consume the words the chain leaves (out->peaks, the sticky clip bits, the status
 * block) and touch no sample arithmetic.  C = dspi_num_channels, n = dspi_num_streams.
 * METER STATE IS THE CALLER'S, like the S/PDIF receiver records: uint32 [n][C], one word = level | count << 16 (level: a block peak's scale,
 * 0..65535; count: the packets its hold has left); an all-zero word is a meter at rest.  The calls keep nothing in the context, so moves,
 * migrations, boots, resizes and snapshots need no new book — the caller relocates its meter words by the same lists as its other
 * per-stream buffers.  Meters that the context owns and that travel with a stream are not part of this interface.
 *
 * dspi_meters_update(ctx, peaks, n_blocks, hold_packets, decay_q15, meters, flags)
 *     peaks = uint16 [n][n_blocks][C], exactly what a process-family call wrote through out->peaks; meters in and out.  For every stream that
 *     is ACTIVE in the context at the time of this call, every channel, and packets k = 0 .. n_blocks - 1 in order, p = peaks[s][k][c]:
 *         if (p >= level)      { level = p; count = hold_packets; }
 *         else if (count > 0)  { count--; }
 *         else                 { level = max(p, (level * decay_q15) >> 15); }      (32-bit unsigned product)
 *     hold_packets 0..65535; decay_q15 0..32768: 32768 never decays (level is the running maximum), 0 drops to p once the hold has run out.
 *     A packet is the unit of time (1 ms of audio at the firmware's packetisation).  Integer arithmetic: the result is defined bit for bit,
 *     and one call over K packets equals calls over any split of them.
 *     PAUSED STREAMS: a paused stream's words are neither read nor written — the meter freezes, as the firmware's peak words do between
 *     packets — and its region of peaks is never read.  The activity used is the context's AT THE TIME OF THIS CALL, not at the time of the
 *     process call that wrote the peaks: update before changing pauses.
 *     flags 0: both buffers in host memory; the call runs on the CPU and works on host-only contexts.  DSPI_MEM_DEVICE: both are device
 *     pointers and the call is asynchronous on the context's stream, behind the process call that wrote peaks: no dspi_sync between them.
 *     REFUSALS, in this order, nothing written: DSPI_E_INVAL for a NULL pointer, n_blocks == 0, hold_packets or decay_q15 out of range,
 *     another flag bit, a size that overflows, a device pointer that is not 4-byte aligned; then DSPI_E_NODEVICE for DSPI_MEM_DEVICE on a
 *     host-only context.  Returns DSPI_OK.
 *
 * dspi_meters_alarms(ctx, meters, level_q15, streams, info, cap, total, flags)
 *     Stream s in [0, n) is IN ALARM when the context's sticky clip bits for s are non-zero (the word DSPI_OUT_CLIP_FLAGS and dspi_get_status
 *     report, read from the context itself), or when meters (may be NULL: clip-only alarms) is given and some channel's level >= level_q15
 *     (0..65535; 0 lists every stream).  Paused streams count, with their frozen state.  streams [cap] receives the alarmed streams in
 *     ASCENDING order, the lowest min(*total, cap) of them; info [cap] (may be NULL), beside each, mask of the channels at or above the level
 *     | clip bits << 16; *total = the number found, which may exceed cap.  The order is deterministic (counts per workgroup, a scan, ordered
 *     writes; no atomic cursor).
 *     flags 0: host memory; returns the number written; on a host-only context the clip bits are 0.  DSPI_MEM_DEVICE: all four pointers are
 *     device pointers, the call is asynchronous on the context's stream, returns DSPI_OK, and *total lands on the device.
 *     REFUSALS: DSPI_E_INVAL for NULL streams or total, cap == 0, level_q15 > 65535, another flag bit, a device pointer that is not 4-byte
 *     aligned; then DSPI_E_NODEVICE as above.
 *
 * dspi_status_all(ctx, first, count, buf, cap, flags)
 *     The REQ_GET_STATUS wValue-9 block of every stream of [first, first + count), packed back to back: 2 C + 4 bytes each (26 / 18), both
 *     CPU-load bytes 0; each block byte for byte what dspi_get_status(ctx, s, ..) answers, paused streams included.  One launch and at most
 *     one copy.  Host memory, or device memory (any alignment) with DSPI_MEM_DEVICE, asynchronous then.  Host-only context: blocks of zero
 *     peaks and flags.  Returns count.  DSPI_E_INVAL for a NULL buf, count == 0, a range past n, another flag bit; DSPI_E_SHORT when
 *     cap < count * (2 C + 4); then DSPI_E_NODEVICE as above.
 *
 * dspi_clear_clips_list(ctx, streams, n)
 *     REQ_CLEAR_CLIPS for a list in HOST memory, any order, duplicates allowed: the clip bits of every listed stream are cleared in one launch
 *     on the context's stream — ordered behind earlier process calls without dspi_clear_clips' per-stream synchronisation —, no other
 *     stream's are touched.  An entry >= n is DSPI_E_INVAL and clears nothing.  Host-only: nothing to clear.  Returns n.  After it
 *     dspi_get_status, DSPI_OUT_CLIP_FLAGS and the next launch see the bits cleared, exactly as after dspi_clear_clips on each entry.
 * The ABI stays 8: detect by symbol (dspi_meters_update; with it dspi_meters_alarms, dspi_status_all, dspi_clear_clips_list; additions only). */
int dspi_meters_update(dspi_ctx *ctx, const uint16_t *peaks, uint32_t n_blocks, uint32_t hold_packets, uint32_t decay_q15,
                       uint32_t *meters, uint32_t flags);
int dspi_meters_alarms(dspi_ctx *ctx, const uint32_t *meters /* may be NULL */, uint32_t level_q15,
                       uint32_t *streams, uint32_t *info /* may be NULL */, uint32_t cap, uint32_t *total, uint32_t flags);
int dspi_status_all(dspi_ctx *ctx, uint32_t first, uint32_t count, void *buf, size_t cap, uint32_t flags);
int dspi_clear_clips_list(dspi_ctx *ctx, const uint32_t *streams, uint32_t n);

/* ---- introspection for tests (host-side derived parameter image of a stream) ------------ */
/* Copies the packed device parameter image; returns its size.  Layout is internal (csrc/dspi_image.h). */
int dspi_debug_image(dspi_ctx *ctx, int32_t stream, void *buf, size_t cap);
/* Which kernel the context's rows currently go to (after the last dspi_process): work items per launch list, counts[5] =
 * {Q28 shared image, packed float shared image, one-stream kernel with per-lane parameter images, packed float with per-lane values
 * incl. band coefficients, packed float with per-lane values and shared band coefficients}.  Tests use it to prove that a scenario
 * ran on the path it was written for.  With n_counts >= 6, counts[5] = items of the float chain's latency layout (any of its three
 * shapes: launches small enough to leave the chip underfilled); with n_counts >= 7, counts[6] = those of them that serve several
 * presets of one structure at once (a workgroup's stream slots each read their own image); with n_counts >= 8, counts[7] = 1 if the
 * context was made with DSPI_NO_EMIT_LINES in the environment (the packed float kernel's emitter wave then never takes its whole-line
 * path), else 0.  Returns the number of counts written (5 to 8) or a negative DSPI_E_*. */
int dspi_debug_launch_plan(dspi_ctx *ctx, uint32_t *counts, size_t n_counts);
/* The delay write index and the leveller ring position of streams [first, first + count), masked to the line / ring length, into host
 * buffers of count words each.  Synchronises the context's stream.  Tests use it to prove that a scenario really was misaligned before
 * a realignment and is uniform per row after it.  Returns count or a negative DSPI_E_*. */
int dspi_debug_stream_positions(dspi_ctx *ctx, uint32_t first, uint32_t count, uint32_t *widx, uint32_t *ring_pos);
/* include/dspi_detmath.h evaluated on the DEVICE, host buffers, n <= 2^24: which = 0: out[i] = log10f(a[i]) and 1: powf(a[i], b[i]) in the two-step
 * forms; 2: log10f, 3: 10^a[i], 4: a[i]^b[i] in the forms the chain kernels use (step 1 + exception tables).  Tests compare all of them bit for
 * bit with the host build of the same header and with binary128. */
int dspi_debug_detmath(dspi_ctx *ctx, int which, const float *a, const float *b, uint32_t n, float *out);
/* Small calls on host buffers (one packet per call, usb_audio.c:1326-1332) do not sleep on their stream: the stream writes the call's sequence
 * number into a word of pinned host memory behind the launches (hipStreamWriteValue32) and the host polls that word — a load per poll, no call
 * into the runtime while waiting, 3-4 us less per call than polling hipStreamQuery — for the audio time the call carries (frames at 44.1 kHz; at
 * least 300 us, at most 50 ms; DSPI_DIRECT_SPIN_US, read at dspi_create, overrides), then the blocking wait.  DSPI_DIRECT_POLL=query polls the
 * stream instead (also the fallback where the write is not available).  What neither way of waiting removes: about one call in 10^5 during
 * which the calling thread itself does not run for 0.5 - 10 ms (the wait phase is long, yet the loop's own clock check never fired): the
 * host's scheduler, for a caller to address with a real-time priority or an isolated core.
 * out[5] = {such calls so far, calls that reached the blocking wait, longest enqueue phase in ns (entry -> launches issued),
 * longest wait phase in ns (these three over the calls after the context's first eight), the last call's polling budget in ns}.  tools/bench_realtime.py reports them next to the latency percentiles.
 * Returns 5 or a negative DSPI_E_*. */
int dspi_debug_direct_stats(dspi_ctx *ctx, uint64_t *out, size_t n);
/* Number of distinct parameter objects the context holds (streams share one until a per-stream call separates them; streams that
 * received the same whole state again through broadcast calls are folded back, here or at the next dspi_process).  Works on
 * host-only contexts.  Returns the count or a negative DSPI_E_*. */
int dspi_debug_image_count(dspi_ctx *ctx);

/* Per-band taps of one EQ channel (float flavour; the parity procedure of SURVEY.md section 8d).  x[n] is run through the ten bands
 * of `channel` (0-1 master, 2.. outputs) of `stream`'s current parameters from zero state, band-major like the firmware's block loop
 * (dsp_pipeline.c:281-365), with the production sample loop in the context's float contract:
 *   taps   float [11][n]   taps[0] = x, taps[b+1] = output of band b
 *   other  float [10][n]   for every sample of band b, what the OTHER contract (canonical <-> DSPI_FLOAT_CONTRACT_FMA) computes from the
 *                          same input and the same filter state: the per-stage rounding difference between the two
 * Host buffers; n <= 2^20.  The chain's own state is not touched. */
int dspi_debug_eq_taps(dspi_ctx *ctx, int32_t stream, int channel, const float *x, uint32_t n, float *taps, float *other);

/* The widening pass of a dspi_process_mixed call on device buffers, alone: pcm_in (DEVICE memory) and bit_depths (host memory) as in that
 * call, one launch on the context's stream into the context's scratch, asynchronous.  No chain runs, nothing is advanced, no preamp is looked
 * at; uniform depths are widened like any others.  For timing the pass (tools/bench_mixed.py); comes with dspi_process_mixed.
 * DSPI_E_INVAL as for that call's pointers, depths and lengths; DSPI_E_NODEVICE on a host-only context. */
int dspi_debug_intake(dspi_ctx *ctx, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len);
/* ... of a dspi_process_sources call on device buffers: the intake for its PCM streams and the receiver for its S/PDIF streams (rx: DEVICE
 * memory, updated), the same way.  For timing (tools/bench_spdif_in.py); comes with dspi_process_sources. */
int dspi_debug_sources_intake(dspi_ctx *ctx, const void *in, const uint8_t *sources, uint32_t n_blocks, uint32_t block_len, dspi_spdif_rx *rx);
/* ... of a dspi_process_patched call: everything in front of the chain (the intake, the receiver over `in`, the link receivers and the one
 * launch for all tiled views), with the call's refusals 3 to 11.  For timing (tools/bench_patched.py); comes with dspi_process_patched. */
int dspi_debug_patched_intake(dspi_ctx *ctx, const void *in, const uint8_t *sources, const dspi_wire_view *views, uint32_t n_views,
                              const dspi_patch *patches, uint32_t n_blocks, uint32_t block_len, dspi_spdif_rx *rx);
/* ... of a dspi_process_packets call: the table's upload and the one launch of dspi_packetrx.hip, with the call's refusals 2 to 5 and then
 * DSPI_E_NODEVICE.  For timing (tools/bench_packets.py); comes with dspi_process_packets. */
int dspi_debug_packets_intake(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths, const uint64_t *table,
                              uint32_t n_blocks, uint32_t block_len);

/* ---- outputs to a packet table, in departure order ------------------------------------------------------------------------------------------ */
/* dspi_packets_emit is the packetiser that the packet-table section above leaves out: it takes the plain pair words that a process call wrote
 * for this context and writes one packet per stream, pair and block into an arena, each where a table points, in the wire format of a USB
 * audio packet or as the words stand.  It is stateless and runs behind any process call; no chain kernel is involved.
 *   pairs     the SOURCE, only read: plain pair words as a process call wrote them for this context without DSPI_OUT_SPDIF, DSPI_OUT_I2S_SLOTS or
 *             DSPI_OUT_WIRE.  With F = n_blocks * block_len: int32 [stream][pair][F][2], or with DSPI_OUT_TILED in flags
 *             int32 [tile][output][F][R], R = dspi_tile_streams(), left = output 2p, right = output 2p + 1.
 *   formats   uint8 [dspi_num_streams], HOST memory always, one value per stream.  32: a packet is block_len frames of the two int32 LE words as
 *             they stand, 8 bytes per frame.  24: a packet is the low three bytes of each word, LE, L then R, 6 bytes per frame: byte for byte
 *             a 24-bit USB packet, the very bytes dspi_process_packets reads at depth 24.
 *   table     uint64 [dspi_num_streams][dspi_num_pairs][n_blocks], HOST memory always.  table[(s * n_pairs + p) * n_blocks + k] is the byte
 *             offset in arena where packet k of pair p of stream s goes, or DSPI_PACKET_SKIP: that packet is not emitted.  The table goes up
 *             with the call, through the context's pinned area: the caller may reuse its emit table when the call returns.
 *   flags     DSPI_MEM_DEVICE: pairs and arena are device memory (pairs 16-byte aligned, as every allocation is; arena 2-byte) and the call is
 *             asynchronous on the context's stream, behind the call that wrote pairs: no dspi_sync between them.  Without it both are host
 *             memory, the call runs on the CPU, synchronously, and works on host-only contexts.  DSPI_OUT_TILED: the source layout, as above.
 *             Every other bit is refused.
 * AN EMIT ENTRY IS LEGAL when it is DSPI_PACKET_SKIP, or when it is even and offset + block_len * frame bytes <= arena_bytes.
 * Entries of one call must not overlap each other or the source; the call does not check this.  Where two entries overlap, every byte of the
 * overlap holds that byte of one of them, unspecified which.  In every case nothing outside the union of the entries is written:
 * neighbouring bytes of the arena are never touched, not even by a read-modify-write, and may belong to someone else.
 * Rows of PAUSED streams are neither read nor checked, their source columns are not read, and nothing is written for them.
 * AN EMIT TABLE CAN BE THE NEXT CONTEXT'S INPUT TABLE: with format 24, the rows of context A's emit table for one pair, handed unchanged to
 * dspi_process_packets on context B with every depth 24 and the same arena, feed B what A wrote; when A and B launch on one HIP stream no
 * synchronisation is needed between the two calls, otherwise B's stream waits for A's (an event, or dspi_sync on A).
 * REFUSALS of dspi_packets_emit, in this order (a refused call writes nothing):
 *   1. DSPI_E_INVAL   a NULL ctx; a flag bit other than DSPI_MEM_DEVICE and DSPI_OUT_TILED
 *   2. DSPI_E_INVAL   a NULL pairs, formats, table or arena; n_blocks == 0 or block_len == 0; block_len > DSPI_MAX_BLOCK_LEN
 *   3. DSPI_E_INVAL   a format that is neither 24 nor 32 (any stream, paused or not, lowest first)
 *   4. DSPI_E_INVAL   an emit table of more than 2^31 - 1 entries: dspi_num_streams * dspi_num_pairs * n_blocks
 *   5. DSPI_E_INVAL   the first illegal emit entry of an active stream, in table order; the message names its index
 *   6. DSPI_E_NODEVICE   DSPI_MEM_DEVICE on a host-only context (then DSPI_E_INVAL for a misaligned device pointer)
 * dspi_packets_emit_check applies refusals 2 to 5 (no pairs, no arena) and works on host-only contexts.  With DSPI_EMIT_CHECK_OVERLAP in
 * check_flags (any other bit: DSPI_E_INVAL) it then refuses the first entry, in table order, that shares a byte with another entry of an
 * active stream; it finds it by sorting, on the CPU, and is the caller's choice.  At refusal 5 and at an overlap *bad_entry, when not NULL,
 * takes the index of the entry refused, and is not written otherwise.
 * LEFT OUT of the packetiser: the sub channel; wire-layout and S/PDIF sources; 16-bit packets; per-packet lengths; tables in device memory; a
 * fused process-and-emit call; an option of dspi_host.
 * (Tables in device memory are left out of THIS call only: dspi_packets_emit_resident, "resident packet tables" below, takes them.)
 * The ABI stays 8: detect by symbol (dspi_packets_emit; with it dspi_packets_emit_check; additions only). */
#define DSPI_PACKET_SKIP UINT64_MAX        /* a table entry that emits nothing */
#define DSPI_EMIT_CHECK_OVERLAP 0x1u       /* dspi_packets_emit_check only */
int dspi_packets_emit_check(const dspi_ctx *ctx, const uint8_t *formats, const uint64_t *table, uint32_t n_blocks, uint32_t block_len,
                            uint64_t arena_bytes, uint32_t check_flags, uint64_t *bad_entry /* may be NULL */);
int dspi_packets_emit(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats,
                      const uint64_t *table, void *arena, uint64_t arena_bytes, uint32_t flags);
/* The one launch of a dspi_packets_emit call on device buffers, alone: formats and table are DEVICE memory here, already uploaded, and are not
 * checked — the table must be one that dspi_packets_emit_check accepts for this context.  flags as for the call, DSPI_MEM_DEVICE required.
 * Asynchronous on the context's stream.  For timing (tools/bench_packets_out.py); comes with dspi_packets_emit. */
int dspi_debug_packets_emit_launch(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats,
                                   const uint64_t *table, void *arena, uint32_t flags);

/* ---- resident packet tables: both packet calls on a table that lies in device memory ---------------------------------------------------------- */
/* A fleet host whose arena is a ring repeats its table from call to call, and often builds it on the GPU.  The four calls below are
 * dspi_packets_check, dspi_packets_emit_check, dspi_process_packets and dspi_packets_emit with ONE difference: `table` is DEVICE memory, 16-byte
 * aligned (every hipMalloc is), and is read where it lies: it does not travel.  The table's layout, the entry rule, the meaning of every other
 * argument and every output are those of the host-table calls.  bit_depths and formats stay HOST memory, uint8 [dspi_num_streams]: their
 * n bytes go up with the call as before, and refusal 3 and the preamp rule are applied on the host as before.  DSPI_MEM_DEVICE is required in
 * flags of both audio calls (dspi_packets_emit_resident has no CPU path).
 * THE ENTRY CHECK RUNS ON THE GPU (refusal 5: the first illegal entry of an active stream in table order).
 *   table_flags == 0, the default route: the call launches the checker on the context's stream, WAITS for its 8-byte answer, and refuses or
 *             proceeds.  The code, the message (entry index, stream, pair, packet) and *bad_entry are exactly what the host-table call gives for
 *             the same table.  The call therefore waits for everything the context queued earlier; what it launches afterwards is asynchronous as
 *             ever.  The table must be complete ON THE CONTEXT'S STREAM when the call is made — written there (dspi_hip_stream), or synchronised
 *             by the caller — and must not be written before the call's work has finished.
 *   DSPI_TABLE_CHECKED: no check, no wait, and no upload beyond the n depth / format bytes: the call is fully asynchronous.  THE CALLER WARRANTS
 *             that dspi_packets_check_resident (dspi_packets_emit_check_resident) accepted THIS table with THESE depths (formats), lengths and
 *             arena_bytes, and that no stream has been resumed, booted active or added since: a paused stream's row was never looked at.  A
 *             violated warrant is out-of-bounds access on the device, reads (input) or WRITES (emit) — nothing looks at the entries again, exactly
 *             as with dspi_debug_packets_emit_launch.  The ring-arena host: check once, then DSPI_TABLE_CHECKED every call until a stream is resumed.
 * REFUSALS, in this order (a refused call writes nothing and advances nothing):
 *   1. to 4.  as in the host-table call; with the flag rule of 1: DSPI_MEM_DEVICE missing, and a bit of table_flags other than DSPI_TABLE_CHECKED
 *   then DSPI_E_NODEVICE on a host-only context
 *   then DSPI_E_INVAL   a table that is not 16-byte aligned; in dspi_packets_emit_resident the host-table call's pointer alignments and its
 *                       limit of 2^31 - 1 workgroups
 *   5.        as in the host-table call, on the default route only
 *   then, in dspi_process_packets_resident, DSPI_E_UNSUPPORTED: the preamp's refusal, and whatever dspi_process_mixed refuses after it
 * The two check calls apply the same refusals up to and including 5 (no arena, no pairs, no out) and wait like the default route; *bad_entry is
 * written at refusal 5 only.  check_flags must be 0: DSPI_EMIT_CHECK_OVERLAP is DSPI_E_INVAL, overlap detection sorts on the CPU and stays with
 * host tables.  Neither works on a host-only context.
 * LEFT OUT: overlap detection on device tables; depth and format vectors in device memory; a check fused into the packet kernels; arenas in
 * host memory; an option of dspi_host.
 * The ABI stays 8: detect by symbol (dspi_process_packets_resident; with it the other three and dspi_debug_table_check_launch; additions only). */
#define DSPI_TABLE_CHECKED 0x1u            /* table_flags: the caller warrants the table; no entry check, no wait */
int dspi_packets_check_resident(dspi_ctx *ctx, const uint8_t *bit_depths, const uint64_t *table /* DEVICE */, uint32_t n_blocks,
                                uint32_t block_len, uint64_t arena_bytes, uint64_t *bad_entry /* may be NULL */);
int dspi_packets_emit_check_resident(dspi_ctx *ctx, const uint8_t *formats, const uint64_t *table /* DEVICE */, uint32_t n_blocks,
                                     uint32_t block_len, uint64_t arena_bytes, uint32_t check_flags /* must be 0 */,
                                     uint64_t *bad_entry /* may be NULL */);
int dspi_process_packets_resident(dspi_ctx *ctx, const void *arena, uint64_t arena_bytes, const uint8_t *bit_depths,
                                  const uint64_t *table /* DEVICE */, uint32_t n_blocks, uint32_t block_len, const dspi_out *out,
                                  uint32_t *pdm_words /* may be NULL */, uint32_t flags, uint32_t table_flags);
int dspi_packets_emit_resident(dspi_ctx *ctx, const int32_t *pairs, uint32_t n_blocks, uint32_t block_len, const uint8_t *formats,
                               const uint64_t *table /* DEVICE */, void *arena, uint64_t arena_bytes, uint32_t flags, uint32_t table_flags);
/* The checker's one launch alone (dspi_tablecheck.hip), asynchronous on the context's stream; the answer stays in the context's own word and is
 * not read.  kind 0: an input table [dspi_num_streams][n_blocks], kinds = the depths; kind 1: an emit table, kinds = the formats.  kinds and
 * table are DEVICE memory, the kinds valid (they are not checked).  For timing (tools/bench_packets_resident.py); comes with
 * dspi_process_packets_resident. */
int dspi_debug_table_check_launch(dspi_ctx *ctx, uint32_t kind, const uint8_t *kinds, const uint64_t *table, uint32_t n_blocks,
                                  uint32_t block_len, uint64_t arena_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DSPI_H */
