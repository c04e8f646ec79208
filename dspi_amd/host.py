"""ctypes binding of the C-ABI (include/dspi.h) — the Python mirror of the reference's data interface.

There is no fallback: if ``libdspi_mi355x.so`` is missing this module raises, and a context without a
GPU (``device=None``) can only exercise the parameter surface — ``process`` fails with DSPI_E_NODEVICE.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import os

LIB_PATH = Path(os.environ.get("DSPI_LIB") or (Path(__file__).resolve().parent / "csrc" / "libdspi_mi355x.so"))

ALL = -1
MEM_DEVICE = 0x1
SNAP_REALIGN = 0x100
RESUME_AS_IS = 0x1
MOVE_AS_IS = 0x1
COMPACT_ONE_WAY = 0x1
MIGRATE_AS_IS = 0x1
MIGRATE_PAUSED = 0x2
GROUP_ONE_WAY = 0x1
BOOT_STREAMS_AS_IS = 0x1
BOOT_STREAMS_OWN_FLASH = 0x2
FLASH_DUMP_BYTES = 12 * 4096
RESIZE_PAUSED = 0x1
OUT_TILED = 0x2
OUT_ENABLED_ONLY = 0x4
OUT_I2S_SLOTS = 0x8
OUT_SPDIF = 0x10
OUT_CLIP_FLAGS = 0x20
OUT_WIRE = 0x40      # dspi_process_sources only
PACKET_SKIP = 2 ** 64 - 1      # dspi_packets_emit: a table entry that emits nothing
EMIT_CHECK_OVERLAP = 0x1       # dspi_packets_emit_check only
TABLE_CHECKED = 0x1            # table_flags of the _resident calls: the caller warrants the table; no entry check, no wait
SRC_SPDIF, SRC_PCM16, SRC_PCM24 = 1, 16, 24
SRC_LINK = 2         # dspi_process_patched / dspi_patched_bytes only
MAX_VIEWS = 8
# dspi_spdif_rx (include/dspi.h): 40 bytes, the first 20 the answer to REQ_GET_SPDIF_IN_STATUS
SPDIF_RX = np.dtype([("state", "<u4"), ("sample_rate", "<u4"), ("parity_err_count", "<u4"), ("c_bits", "u1", (5,)), ("pad_", "u1", (3,)), ("hold", "<i4", (2,)),
                     ("sync", "<u4"), ("held", "<u4"), ("coding_errors", "<u4")])
# dspi_link / dspi_wire_view (include/dspi.h, chained devices): a line of a producer's wire buffer and the buffer itself
LINK_NONE, LINK_SPDIF, LINK_I2S = 0, 1, 2
LINK = np.dtype([("line", "<u4"), ("kind", "<u4")])
PATCH = np.dtype([("view", "<u4"), ("line", "<u4"), ("kind", "<u4")])
WIRE_VIEW = np.dtype([("wire", "<u8"), ("n_streams", "<u4"), ("n_pairs", "<u4"), ("tile_streams", "<u4"), ("n_frames", "<u4"), ("producer", "<u8")])
E_INVAL = -10
E_NODEVICE = -11
E_UNSUPPORTED = -14
E_SHORT = -15


class DspiError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"dspi error {code}: {msg}")
        self.code = code


class _Snapshot(C.Structure):
    _fields_ = [("head", C.c_void_p), ("head_bytes", C.c_size_t), ("state", C.c_void_p), ("state_bytes", C.c_size_t)]      # dspi_snapshot


class _Out(C.Structure):
    _fields_ = [("pairs", C.c_void_p), ("sub", C.c_void_p), ("peaks", C.c_void_p), ("clip_flags", C.c_void_p)]      # clip_flags: ABI 7, read with OUT_CLIP_FLAGS only


_lib = None


def source_fingerprint(pkg_root: Path | None = None) -> str:
    """sha256 (first 16 hex digits) over the library's sources (dspi_amd/csrc/*.hip *.inc *.h *.cpp, include/*.h), in name order.
    tools/prof_summary.py stores it with every counter profile and bench.py compares it with the tree it runs from, so that a
    roofline.traffic figure taken from an older build says so (traffic_stale)."""
    import hashlib
    root = Path(pkg_root) if pkg_root else Path(__file__).resolve().parent
    files = sorted([p for pat in ("*.hip", "*.inc", "*.h", "*.cpp") for p in (root / "csrc").glob(pat)] + list((root.parent / "include").glob("*.h")))
    h = hashlib.sha256()
    for f in files:
        h.update(f.name.encode()); h.update(b"\0"); h.update(f.read_bytes())
    return h.hexdigest()[:16]


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)")
    L = C.CDLL(str(LIB_PATH))
    vp, i32, u32, u16, u8 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint16, C.c_uint8
    L.dspi_create.argtypes = [C.POINTER(vp), C.c_int, u32, C.c_int]
    L.dspi_destroy.argtypes = [vp]
    L.dspi_last_error.argtypes = [vp]
    L.dspi_last_error.restype = C.c_char_p
    for name in ("dspi_num_channels", "dspi_num_outputs", "dspi_num_pairs"):
        getattr(L, name).argtypes = [vp]
    L.dspi_num_streams.argtypes = [vp]
    L.dspi_num_streams.restype = u32
    L.dspi_tile_streams.argtypes = [vp]
    L.dspi_tile_streams.restype = u32
    L.dspi_factory_defaults.argtypes = [vp, i32]
    L.dspi_load_bulk.argtypes = [vp, i32, vp, C.c_size_t]
    L.dspi_collect_bulk.argtypes = [vp, i32, vp, C.c_size_t]
    L.dspi_load_preset_slot.argtypes = [vp, i32, vp, C.c_size_t, C.c_int]
    L.dspi_load_flash_dump.argtypes = [vp, i32, vp, C.c_size_t]
    L.dspi_flash_read_directory.argtypes = [vp, C.c_size_t, vp]
    L.dspi_save_preset_slot.argtypes = [vp, i32, vp, C.c_size_t, C.c_int]
    L.dspi_vendor_set.argtypes = [vp, i32, u8, u16, vp, u16]
    L.dspi_vendor_get.argtypes = [vp, i32, u8, u16, vp, u16]
    L.dspi_set_host_volume.argtypes = [vp, i32, C.c_int16]
    L.dspi_set_mute.argtypes = [vp, i32, C.c_int]
    L.dspi_set_sample_rate.argtypes = [vp, i32, u32]
    L.dspi_process.argtypes = [vp, vp, C.c_int, u32, u32, C.POINTER(_Out), u32]
    L.dspi_pdm_modulate.argtypes = [vp, vp, u32, vp, u32]
    L.dspi_pdm_restart.argtypes = [vp, C.c_int32]
    L.dspi_spdif_encode.argtypes = [vp, vp, u32, u32, vp, u32]
    L.dspi_i2s_encode.argtypes = [vp, vp, u32, u32, vp, u32]
    L.dspi_sync.argtypes = [vp]
    L.dspi_hip_stream.argtypes = [vp]
    L.dspi_hip_stream.restype = vp
    L.dspi_get_status.argtypes = [vp, i32, vp, C.c_size_t]
    L.dspi_clear_clips.argtypes = [vp, i32]
    L.dspi_debug_image.argtypes = [vp, i32, vp, C.c_size_t]
    L.dspi_debug_launch_plan.argtypes = [vp, vp, C.c_size_t]
    if hasattr(L, "dspi_debug_direct_stats"): L.dspi_debug_direct_stats.argtypes = [vp, vp, C.c_size_t]      # (ABI 8; bench.py's same-box A/B loads the previous round's library through this module)
    if hasattr(L, "dspi_snapshot_sizes"):      # (ABI 8 + snapshots: detected by symbol, as above)
        L.dspi_snapshot_sizes.argtypes = [vp, u32, u32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.dspi_export_streams.argtypes = [vp, u32, u32, C.POINTER(_Snapshot), u32]
        L.dspi_import_streams.argtypes = [vp, u32, C.POINTER(_Snapshot), u32]
    if hasattr(L, "dspi_realign_streams"):      # (ABI 8 + realignment: detected by symbol; with it DSPI_SNAP_REALIGN)
        L.dspi_realign_streams.argtypes = [vp, u32, u32]
        L.dspi_debug_stream_positions.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "dspi_pause_streams"):      # (ABI 8 + paused streams: detected by symbol; with it DSPI_RESUME_AS_IS)
        L.dspi_pause_streams.argtypes = [vp, u32, u32]
        L.dspi_resume_streams.argtypes = [vp, u32, u32, u32]
        L.dspi_streams_paused.argtypes = [vp, u32, u32, vp]
    if hasattr(L, "dspi_move_streams"):      # (ABI 8 + stream moves: detected by symbol; with it DSPI_MOVE_AS_IS, DSPI_COMPACT_ONE_WAY)
        L.dspi_move_streams.argtypes = [vp, vp, u32, u32]
        L.dspi_plan_compaction.argtypes = [vp, vp, u32, u32]
    if hasattr(L, "dspi_migrate_streams"):      # (ABI 8 + migration: detected by symbol; with it dspi_plan_migration, DSPI_MIGRATE_AS_IS, DSPI_MIGRATE_PAUSED)
        L.dspi_migrate_streams.argtypes = [vp, vp, vp, u32, u32]
        L.dspi_plan_migration.argtypes = [vp, vp, u32, vp, u32, u32]
    if hasattr(L, "dspi_plan_grouping"):      # (ABI 8 + grouping: detected by symbol; with it DSPI_GROUP_ONE_WAY)
        L.dspi_plan_grouping.argtypes = [vp, vp, u32, u32]
    if hasattr(L, "dspi_boot_streams"):      # (ABI 8 + stream boots: detected by symbol; with it DSPI_BOOT_STREAMS_AS_IS)
        L.dspi_boot_streams.argtypes = [vp, vp, u32, vp, C.c_size_t, u32, C.POINTER(C.c_int)]
    if hasattr(L, "dspi_spdif_per_stream"):      # (ABI 8 + per-stream S/PDIF positions: detected by symbol; with it dspi_spdif_stream_pos, dspi_spdif_encode_v)
        L.dspi_spdif_per_stream.argtypes = [vp, C.c_int]
        L.dspi_spdif_stream_pos.argtypes = [vp, u32, u32, vp, vp]
        L.dspi_spdif_encode_v.argtypes = [vp, vp, u32, vp, vp, u32]
    if hasattr(L, "dspi_resize_streams"):      # (ABI 8 + resizing: detected by symbol; with it dspi_reserve_streams, dspi_stream_capacity, DSPI_RESIZE_PAUSED)
        L.dspi_resize_streams.argtypes = [vp, u32, u32]
        L.dspi_reserve_streams.argtypes = [vp, u32]
        L.dspi_stream_capacity.argtypes = [vp]
        L.dspi_stream_capacity.restype = u32
    if hasattr(L, "dspi_process_pdm"):
        L.dspi_process_pdm.argtypes = [vp, vp, C.c_int, u32, u32, C.POINTER(_Out), vp, u32]
        L.dspi_pdm_running.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "dspi_pdm_fade"):      # (ABI 8 + the PDM fade-out on disable: detected by symbol; with it dspi_pdm_fade_state)
        L.dspi_pdm_fade.argtypes = [vp, C.c_int]
        L.dspi_pdm_fade_state.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "dspi_process_mixed"):      # (ABI 8 + mixed input formats: detected by symbol; with it dspi_mixed_pcm_bytes)
        L.dspi_mixed_pcm_bytes.argtypes = [vp, vp, u32, u32, C.POINTER(C.c_uint64), vp]
        L.dspi_process_mixed.argtypes = [vp, vp, vp, u32, u32, C.POINTER(_Out), vp, u32]
        L.dspi_debug_intake.argtypes = [vp, vp, vp, u32, u32]
    if hasattr(L, "dspi_process_wire"):      # (ABI 8 + wire words per device: detected by symbol; with it dspi_wire_encode)
        L.dspi_process_wire.argtypes = [vp, vp, C.c_int, u32, u32, C.POINTER(_Out), vp, u32]
        L.dspi_wire_encode.argtypes = [vp, vp, u32, vp, vp, u32]
    if hasattr(L, "dspi_process_devices"):      # (ABI 8 + wire words on tiled and mixed-depth contexts: detected by symbol; with it dspi_wire_encode_tiled)
        L.dspi_process_devices.argtypes = [vp, vp, vp, u32, u32, C.POINTER(_Out), vp, u32]
        L.dspi_wire_encode_tiled.argtypes = [vp, vp, u32, vp, vp, u32]
    if hasattr(L, "dspi_device_flash"):      # (ABI 8 + a stream's own flash: detected by symbol; with it dspi_flash_read, dspi_flash_write, DSPI_BOOT_STREAMS_OWN_FLASH)
        L.dspi_device_flash.argtypes = [vp, C.c_int]
        L.dspi_flash_read.argtypes = [vp, u32, vp, C.c_size_t]
        L.dspi_flash_write.argtypes = [vp, u32, u32, vp, C.c_size_t]
    if hasattr(L, "dspi_process_sources"):      # (ABI 8 + S/PDIF input: detected by symbol; with it dspi_spdif_decode, dspi_sources_bytes)
        L.dspi_sources_bytes.argtypes = [vp, vp, u32, u32, C.POINTER(C.c_uint64), vp]
        L.dspi_process_sources.argtypes = [vp, vp, vp, u32, u32, C.POINTER(_Out), vp, vp, u32]
        L.dspi_spdif_decode.argtypes = [vp, vp, u32, u32, vp, vp, u32]
        L.dspi_debug_sources_intake.argtypes = [vp, vp, vp, u32, u32, vp]
    if hasattr(L, "dspi_process_linked"):      # (ABI 8 + chained devices: detected by symbol; with it dspi_wire_decode, dspi_wire_view_of, dspi_link_kinds)
        L.dspi_wire_view_of.argtypes = [vp, vp, u32, u32, vp]
        L.dspi_link_kinds.argtypes = [vp, vp, u32]
        L.dspi_wire_decode.argtypes = [vp, vp, vp, u32, vp, vp, u32]
        L.dspi_process_linked.argtypes = [vp, vp, vp, u32, u32, C.POINTER(_Out), vp, vp, u32]
    if hasattr(L, "dspi_process_patched"):      # (ABI 8 + the patch bay: detected by symbol; with it dspi_patched_bytes)
        L.dspi_patched_bytes.argtypes = [vp, vp, u32, u32, C.POINTER(C.c_uint64), vp]
        L.dspi_process_patched.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, C.POINTER(_Out), vp, vp, u32]
        L.dspi_debug_patched_intake.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, vp]
    if hasattr(L, "dspi_meters_update"):      # (ABI 8 + the meter bridge: detected by symbol; with it dspi_meters_alarms, dspi_status_all, dspi_clear_clips_list)
        L.dspi_meters_update.argtypes = [vp, vp, u32, u32, u32, vp, u32]
        L.dspi_meters_alarms.argtypes = [vp, vp, u32, vp, vp, u32, vp, u32]
        L.dspi_status_all.argtypes = [vp, u32, u32, vp, C.c_size_t, u32]
        L.dspi_clear_clips_list.argtypes = [vp, vp, u32]
    if hasattr(L, "dspi_process_packets"):      # (ABI 8 + input from a packet table: detected by symbol; with it dspi_packets_check)
        L.dspi_packets_check.argtypes = [vp, vp, vp, u32, u32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.dspi_process_packets.argtypes = [vp, vp, C.c_uint64, vp, vp, u32, u32, C.POINTER(_Out), vp, u32]
        L.dspi_debug_packets_intake.argtypes = [vp, vp, C.c_uint64, vp, vp, u32, u32]
    if hasattr(L, "dspi_packets_emit"):      # (ABI 8 + outputs to a packet table: detected by symbol; with it dspi_packets_emit_check)
        L.dspi_packets_emit_check.argtypes = [vp, vp, vp, u32, u32, C.c_uint64, u32, C.POINTER(C.c_uint64)]
        L.dspi_packets_emit.argtypes = [vp, vp, u32, u32, vp, vp, vp, C.c_uint64, u32]
        L.dspi_debug_packets_emit_launch.argtypes = [vp, vp, u32, u32, vp, vp, vp, u32]
    if hasattr(L, "dspi_process_packets_resident"):      # (ABI 8 + resident packet tables: detected by symbol; with it the three other _resident calls)
        L.dspi_packets_check_resident.argtypes = [vp, vp, vp, u32, u32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.dspi_packets_emit_check_resident.argtypes = [vp, vp, vp, u32, u32, C.c_uint64, u32, C.POINTER(C.c_uint64)]
        L.dspi_process_packets_resident.argtypes = [vp, vp, C.c_uint64, vp, vp, u32, u32, C.POINTER(_Out), vp, u32, u32]
        L.dspi_packets_emit_resident.argtypes = [vp, vp, u32, u32, vp, vp, vp, C.c_uint64, u32, u32]
        L.dspi_debug_table_check_launch.argtypes = [vp, u32, vp, vp, u32, u32, C.c_uint64]
        L.dspi_tablecheck_launch_raw.argtypes = [u32, vp, vp, vp, C.c_uint64, u32, u32, C.c_uint64, u32, vp, C.POINTER(C.c_uint64)]      # (no interface: the tests' raw launcher)
    _lib = L
    return L


class Dspi:
    """`n_streams` DSPi devices on one GPU (device=None: host-only, parameter surface only)."""

    def __init__(self, flavor: int, n_streams: int, device: int | None = 0, fma: bool = False, populated_flash: bool = False):
        """fma: the float flavour with the firmware build's FMA contraction (DSPI_FLOAT_CONTRACT_FMA, include/dspi.h).
        populated_flash: DSPI_BOOT_POPULATED_FLASH — devices that do not boot for the first time (no first-boot preset mute)."""
        self.L = lib()
        self.h = C.c_void_p()
        fma = bool(fma or getattr(flavor, "fma", False))      # tests pass wire.F32_FMA: the int 1 carrying the contract
        flavor = int(flavor)
        self.fma = fma
        rc = self.L.dspi_create(C.byref(self.h), flavor | (0x100 if fma else 0) | (0x200 if populated_flash else 0), n_streams, -1 if device is None else device)
        if rc != 0:
            raise DspiError(rc, "dspi_create")
        self.flavor, self.n_streams = flavor, n_streams
        self.C = self.L.dspi_num_channels(self.h)
        self.N = self.L.dspi_num_outputs(self.h)
        self.P = self.L.dspi_num_pairs(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.dspi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int, what: str) -> int:
        if rc < 0:
            raise DspiError(rc, f"{what}: {self.L.dspi_last_error(self.h).decode()}")
        return rc

    # ---- parameters ----
    def factory_defaults(self, stream: int = ALL):
        return self._ck(self.L.dspi_factory_defaults(self.h, stream), "factory_defaults")

    def load_bulk(self, blob, stream: int = ALL) -> int:
        raw = blob.tobytes() if hasattr(blob, "tobytes") else bytes(blob)
        return self.L.dspi_load_bulk(self.h, stream, raw, len(raw))      # firmware codes 0,-1..-4 are returned as-is

    def collect_bulk(self, stream: int = 0) -> bytes:
        buf = C.create_string_buffer(2896)
        self._ck(self.L.dspi_collect_bulk(self.h, stream, buf, 2896), "collect_bulk")
        return buf.raw

    def load_slot(self, image: bytes, expect_slot: int = -1, stream: int = ALL) -> int:
        return self.L.dspi_load_preset_slot(self.h, stream, image, len(image), expect_slot)

    def load_flash_dump(self, dump: bytes, stream: int = ALL) -> int:
        """dspi_load_flash_dump: 0..9 slot loaded | 16+n selected slot empty/corrupt | 32 legacy migrated | 48 factory."""
        return self.L.dspi_load_flash_dump(self.h, stream, dump, len(dump))

    def save_slot(self, slot_index: int = 0, stream: int = 0) -> bytes:
        buf = C.create_string_buffer(4096)
        n = self._ck(self.L.dspi_save_preset_slot(self.h, stream, buf, 4096, slot_index), "save_slot")
        return buf.raw[:n]

    def vendor_set(self, req: int, wvalue: int, payload: bytes, stream: int = ALL) -> int:
        return self.L.dspi_vendor_set(self.h, stream, req, wvalue, payload, len(payload))

    def vendor_get(self, req: int, wvalue: int, cap: int = 64, stream: int = 0):
        buf = C.create_string_buffer(max(cap, 1))
        n = self.L.dspi_vendor_get(self.h, stream, req, wvalue, buf, cap)
        return None if n < 0 else buf.raw[:n]

    def set_volume(self, v: int, stream: int = ALL):
        return self._ck(self.L.dspi_set_host_volume(self.h, stream, v), "set_host_volume")

    def set_mute(self, m: bool, stream: int = ALL):
        return self._ck(self.L.dspi_set_mute(self.h, stream, int(m)), "set_mute")

    def set_rate(self, hz: int, stream: int = ALL) -> int:
        return self.L.dspi_set_sample_rate(self.h, stream, hz)

    def status(self, stream: int = 0) -> bytes:
        n = self.C * 2 + 4
        buf = C.create_string_buffer(n)
        self._ck(self.L.dspi_get_status(self.h, stream, buf, n), "get_status")
        return buf.raw

    def clear_clips(self, stream: int = ALL) -> int:
        return self._ck(self.L.dspi_clear_clips(self.h, stream), "clear_clips")

    def debug_image(self, stream: int = 0) -> bytes:
        buf = C.create_string_buffer(8192)
        n = self._ck(self.L.dspi_debug_image(self.h, stream, buf, 8192), "debug_image")
        return buf.raw[:n]

    def spdif_block_pos(self, set: int = -1) -> int:
        """dspi_spdif_block_pos: position in the 192-frame channel-status block of the next DSPI_OUT_SPDIF call's first frame."""
        return self._ck(self.L.dspi_spdif_block_pos(self.h, set), "spdif_block_pos")

    def spdif_per_stream(self, enable: int = -1) -> bool:
        """dspi_spdif_per_stream: per-stream S/PDIF block positions on (1) / off (0), or only read (default).  Returns the mode after the call."""
        return bool(self._ck(self.L.dspi_spdif_per_stream(self.h, enable), "spdif_per_stream"))

    def spdif_stream_pos(self, first: int = 0, count: int | None = None, set=None) -> np.ndarray:
        """dspi_spdif_stream_pos: sets (set: `count` values 0..191, optional) and returns the block positions of streams [first, first + count),
        uint32 [count] — for each stream the position of the first frame of its next DSPI_OUT_SPDIF call.  Mode on only."""
        count = self.n_streams - first if count is None else count
        get = np.zeros(count, dtype=np.uint32)
        v = None
        if set is not None:
            v = np.ascontiguousarray(np.asarray(set, dtype=np.uint32).reshape(-1))
            assert len(v) == count, (len(v), count)
        self._ck(self.L.dspi_spdif_stream_pos(self.h, first, count, v.ctypes.data if v is not None else None, get.ctypes.data), "spdif_stream_pos")
        return get

    def launch_plan(self) -> dict:
        """dspi_debug_launch_plan: work items per kernel path after the last process call."""
        c = (C.c_uint32 * 8)()
        self._ck(min(self.L.dspi_debug_launch_plan(self.h, c, 8), 0), "debug_launch_plan")
        # (emit_lines_off: not a count of items — 1 while DSPI_NO_EMIT_LINES keeps the packed kernel's emitter wave off its whole-line path)
        return dict(zip(("q28_shared", "packed_shared", "one_stream_per_lane_images", "packed_per_lane_values_and_bands", "packed_per_lane_values", "latency_layout",
                         "latency_layout_paired", "emit_lines_off"), list(c)))

    def direct_stats(self) -> dict:
        """dspi_debug_direct_stats: the one-packet-per-call path's polling record (include/dspi.h)."""
        c = (C.c_uint64 * 5)()
        self._ck(min(self.L.dspi_debug_direct_stats(self.h, c, 5), 0), "debug_direct_stats")
        return dict(calls=int(c[0]), blocking_waits=int(c[1]), max_enqueue_us=c[2] / 1e3, max_wait_us=c[3] / 1e3, spin_budget_us=c[4] / 1e3)

    def image_count(self) -> int:
        """dspi_debug_image_count: distinct parameter objects held (equal ones are folded after broadcast calls)."""
        return self._ck(self.L.dspi_debug_image_count(self.h), "debug_image_count")

    def eq_taps(self, x: np.ndarray, channel: int, stream: int = 0):
        """dspi_debug_eq_taps: (taps [11][n], other [10][n]) of one EQ channel on the GPU, see include/dspi.h."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        taps = np.zeros((11, x.size), dtype=np.float32); other = np.zeros((10, x.size), dtype=np.float32)
        self.L.dspi_debug_eq_taps.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self._ck(self.L.dspi_debug_eq_taps(self.h, stream, channel, x.ctypes.data, x.size, taps.ctypes.data, other.ctypes.data), "debug_eq_taps")
        return taps, other

    # ---- audio ----
    def tile_streams(self) -> int:
        """R of the tiled layouts (dspi.h DSPI_OUT_TILED): 128 float / 64 Q28."""
        return int(self.L.dspi_tile_streams(self.h))

    def process_host(self, pcm: np.ndarray, n_blocks: int, block_len: int, bit_depth: int = 16,
                     want_pairs=True, want_sub=True, want_peaks=True, tiled=False, out=None, enabled_only=False, i2s_slots=False, spdif=False, clip=False):
        """Host-memory convenience path (tests): pcm = int16 [streams][frames][2] or uint8 [streams][frames*6].
        Returns (pairs [S][P][F][2], sub [S][F], peaks [S][blocks][C]); with tiled=True the sample words come back in
        the DSPI_OUT_TILED layout: pairs [tiles][outputs][F][R], sub [tiles][F][R] (see untile()); with spdif=True (DSPI_OUT_SPDIF)
        pairs are the IEC 60958 subframes, uint32 [S][P][F][4].  clip=True (DSPI_OUT_CLIP_FLAGS): every stream's sticky clip flags after the
        call are left in self.last_clip, uint16 [S]."""
        S, F = self.n_streams, n_blocks * block_len
        pcm = np.ascontiguousarray(pcm)
        assert pcm.nbytes == S * F * (6 if bit_depth == 24 else 4), (pcm.shape, S, F)
        if out is not None:      # the arrays of an earlier call, written in place (a host that reuses its buffers: no fresh pages to fault in)
            pairs, sub, peaks = out
            want_pairs, want_sub, want_peaks = pairs is not None, sub is not None, peaks is not None
        elif tiled:
            R = self.tile_streams(); nt = (S + R - 1) // R
            pairs = np.zeros((nt, self.P * 2, F, R), dtype=np.int32) if want_pairs else None
            sub = np.zeros((nt, F, R), dtype=np.int32) if want_sub else None
        else:
            pairs = (np.zeros((S, self.P, F, 4), dtype=np.uint32) if spdif else np.zeros((S, self.P, F, 2), dtype=np.int32)) if want_pairs else None
            sub = np.zeros((S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        self.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        out = _Out(pairs.ctypes.data if want_pairs else None, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, self.last_clip.ctypes.data if clip else None)
        self._ck(self.L.dspi_process(self.h, pcm.ctypes.data, bit_depth, n_blocks, block_len, C.byref(out), (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_I2S_SLOTS if i2s_slots else 0) | (OUT_SPDIF if spdif else 0) | (OUT_CLIP_FLAGS if clip else 0)), "process")
        return pairs, sub, peaks

    def untile(self, pairs_t: np.ndarray, sub_t: np.ndarray):
        """Tiled -> stream-major view of process_host(tiled=True) results (test helper)."""
        S = self.n_streams
        pairs = sub = None
        if pairs_t is not None:
            nt, O, F, R = pairs_t.shape
            pairs = pairs_t.transpose(0, 3, 1, 2).reshape(nt * R, O // 2, 2, F).transpose(0, 1, 3, 2)[:S].copy()
        if sub_t is not None:
            nt, F, R = sub_t.shape
            sub = sub_t.transpose(0, 2, 1).reshape(nt * R, F)[:S].copy()
        return pairs, sub

    def untile_wire(self, wire_t: np.ndarray, types) -> np.ndarray:
        """The tiled wire layout (include/dspi.h: dspi_process_devices) -> the stream-major wire layout, uint32 [S][P][F][4] (test helper).
        wire_t: uint32 [tiles][P][F][4][R], i.e. per (tile, pair) a region of 4 F rows of R words; types: bool [S][P], slot p of stream s is
        an I2S slot.  Stream s is column s % R of tile s // R.  An S/PDIF slot's subframe word j of frame f stands in row f * 4 + j; an I2S
        slot's word of (side, frame f) in row side * F + f and goes to word 2 f + side of the stream-major region's first half; the rows
        2 F .. 4 F - 1 of an I2S column (its tail) go to the second half as they are."""
        nt, P, F, four, R = wire_t.shape
        assert four == 4
        S = self.n_streams
        types = np.asarray(types, dtype=bool)
        assert types.shape == (S, P) and nt * R >= S, (types.shape, wire_t.shape)
        rows = wire_t.reshape(nt, P, 4 * F, R)
        out = np.zeros((S, P, F, 4), dtype=np.uint32)
        for s in range(S):
            t, c = divmod(s, R)
            for p in range(P):
                col = rows[t, p, :, c]
                if types[s, p]:
                    flat = out[s, p].reshape(-1)
                    flat[0:2 * F:2] = col[:F]              # side 0 (L) of frames 0 .. F - 1
                    flat[1:2 * F:2] = col[F:2 * F]         # side 1 (R)
                    flat[2 * F:] = col[2 * F:]             # the tail
                else:
                    out[s, p] = col.reshape(F, 4)
        return out

    def process_device(self, pcm_ptr: int, n_blocks: int, block_len: int, bit_depth: int = 16,
                       pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, i2s_slots: bool = False, spdif: bool = False,
                       clip_ptr: int = 0):
        """Zero-copy path: raw device pointers (e.g. torch.Tensor.data_ptr()); asynchronous, see sync().  clip_ptr: uint16 [S] (DSPI_OUT_CLIP_FLAGS)."""
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process(self.h, pcm_ptr, bit_depth, n_blocks, block_len, C.byref(out), MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_I2S_SLOTS if i2s_slots else 0) | (OUT_SPDIF if spdif else 0) | (OUT_CLIP_FLAGS if clip_ptr else 0)), "process")

    def process_pdm_host(self, pcm: np.ndarray, n_blocks: int, block_len: int, bit_depth: int = 16, want_pairs=True, want_sub=True, want_peaks=True,
                         tiled=False, enabled_only=False, words=None):
        """dspi_process_pdm on host arrays: process_host's (pairs, sub, peaks) and the PDM words, uint32 [S][F][8] (tiled: [tiles][F][8][R]).
        words: an array of that shape to write into (what a stream that is not modulated leaves there is the library's to decide)."""
        S, F = self.n_streams, n_blocks * block_len
        pcm = np.ascontiguousarray(pcm)
        assert pcm.nbytes == S * F * (6 if bit_depth == 24 else 4), (pcm.shape, S, F)
        R = self.tile_streams(); nt = (S + R - 1) // R
        if tiled:
            pairs = np.zeros((nt, self.P * 2, F, R), dtype=np.int32) if want_pairs else None
            sub = np.zeros((nt, F, R), dtype=np.int32) if want_sub else None
        else:
            pairs = np.zeros((S, self.P, F, 2), dtype=np.int32) if want_pairs else None
            sub = np.zeros((S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        if words is None: words = np.zeros((nt, F, 8, R) if tiled else (S, F, 8), dtype=np.uint32)
        assert words.dtype == np.uint32 and words.flags.c_contiguous and words.size == (nt * R if tiled else S) * F * 8
        out = _Out(pairs.ctypes.data if want_pairs else None, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, None)
        self._ck(self.L.dspi_process_pdm(self.h, pcm.ctypes.data, bit_depth, n_blocks, block_len, C.byref(out), words.ctypes.data,
                                         (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0)), "process_pdm")
        return pairs, sub, peaks, words

    def process_pdm_device(self, pcm_ptr: int, n_blocks: int, block_len: int, words_ptr: int, bit_depth: int = 16, pairs_ptr: int = 0, sub_ptr: int = 0,
                           peaks_ptr: int = 0, tiled: bool = False, enabled_only: bool = False):
        """dspi_process_pdm on raw device pointers; asynchronous, see sync()."""
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, None)
        self._ck(self.L.dspi_process_pdm(self.h, pcm_ptr, bit_depth, n_blocks, block_len, C.byref(out), words_ptr,
                                         MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0)), "process_pdm")

    # ---- 16- and 24-bit devices in one call (include/dspi.h: dspi_process_mixed) ----
    def _depths(self, bit_depths) -> np.ndarray:
        d = np.ascontiguousarray(np.asarray(bit_depths, dtype=np.uint8).reshape(-1))
        assert d.size == self.n_streams, (d.size, self.n_streams)
        return d

    def mixed_pcm_bytes(self, bit_depths, n_blocks: int, block_len: int):
        """dspi_mixed_pcm_bytes: (total bytes, offsets uint64 [n_streams + 1]) of the PCM buffer of a dspi_process_mixed call with these depths
        (uint8 [n_streams], each 16 or 24).  Works on host-only contexts."""
        d = self._depths(bit_depths)
        total, off = C.c_uint64(0), np.zeros(self.n_streams + 1, dtype=np.uint64)
        self._ck(self.L.dspi_mixed_pcm_bytes(self.h, d.ctypes.data, n_blocks, block_len, C.byref(total), off.ctypes.data), "mixed_pcm_bytes")
        return total.value, off

    def process_mixed_host(self, pcm: np.ndarray, bit_depths, n_blocks: int, block_len: int, want_pairs=True, want_sub=True, want_peaks=True,
                           tiled=False, enabled_only=False, spdif=False, clip=False, pdm=False, words=None):
        """dspi_process_mixed on host arrays: pcm = one flat uint8 array, every stream's run of frames at its own depth back to back
        (mixed_pcm_bytes); bit_depths uint8 [n_streams].  Returns process_host's (pairs, sub, peaks); with pdm=True (or `words` given)
        process_pdm_host's (pairs, sub, peaks, words).  clip=True: self.last_clip as after process_host."""
        S, F = self.n_streams, n_blocks * block_len
        d = self._depths(bit_depths)
        pcm = np.ascontiguousarray(pcm, dtype=np.uint8).reshape(-1)
        if np.isin(d, (16, 24)).all(): assert pcm.nbytes == F * int(np.where(d == 24, 6, 4).sum()), (pcm.nbytes, S, F)      # (bad depths are the library's to refuse)
        R = self.tile_streams(); nt = (S + R - 1) // R
        if tiled:
            pairs = np.zeros((nt, self.P * 2, F, R), dtype=np.int32) if want_pairs else None
            sub = np.zeros((nt, F, R), dtype=np.int32) if want_sub else None
        else:
            pairs = (np.zeros((S, self.P, F, 4), dtype=np.uint32) if spdif else np.zeros((S, self.P, F, 2), dtype=np.int32)) if want_pairs else None
            sub = np.zeros((S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        if (pdm or words is not None) and words is None: words = np.zeros((nt, F, 8, R) if tiled else (S, F, 8), dtype=np.uint32)
        if words is not None: assert words.dtype == np.uint32 and words.flags.c_contiguous and words.size == (nt * R if tiled else S) * F * 8
        self.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        out = _Out(pairs.ctypes.data if want_pairs else None, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, self.last_clip.ctypes.data if clip else None)
        self._ck(self.L.dspi_process_mixed(self.h, pcm.ctypes.data, d.ctypes.data, n_blocks, block_len, C.byref(out), words.ctypes.data if words is not None else None,
                                           (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_CLIP_FLAGS if clip else 0)), "process_mixed")
        return (pairs, sub, peaks) if words is None else (pairs, sub, peaks, words)

    def process_mixed_device(self, pcm_ptr: int, bit_depths, n_blocks: int, block_len: int, pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0,
                             words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, clip_ptr: int = 0):
        """dspi_process_mixed on raw device pointers (the depths stay a host array); asynchronous, see sync().  words_ptr: as process_pdm_device."""
        d = self._depths(bit_depths)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_mixed(self.h, pcm_ptr, d.ctypes.data, n_blocks, block_len, C.byref(out), words_ptr or None,
                                           MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_mixed")

    def debug_intake(self, pcm_ptr: int, bit_depths, n_blocks: int, block_len: int):
        """dspi_debug_intake: the widening pass of process_mixed_device alone, into the context's scratch; asynchronous, see sync()."""
        d = self._depths(bit_depths)
        self._ck(self.L.dspi_debug_intake(self.h, pcm_ptr, d.ctypes.data, n_blocks, block_len), "debug_intake")

    def pdm_running(self, first: int = 0, count: int | None = None, set=None) -> np.ndarray:
        """dspi_pdm_running: the running bytes of streams [first, first + count) (default: to the end), after writing `set` (0 / 1 each) if given."""
        if count is None: count = self.n_streams - first
        get = np.zeros(count, dtype=np.uint8)
        if set is not None:
            set = np.ascontiguousarray(set, dtype=np.uint8)
            assert set.size == count
        self._ck(self.L.dspi_pdm_running(self.h, first, count, set.ctypes.data if set is not None else None, get.ctypes.data), "pdm_running")
        return get

    def pdm_fade(self, enable: int = -1) -> bool:
        """dspi_pdm_fade: the PDM fade-out on disable on (1) / off (0), or only read (default).  Returns the mode after the call."""
        return bool(self._ck(self.L.dspi_pdm_fade(self.h, enable), "pdm_fade"))

    def pdm_fade_state(self, first: int = 0, count: int | None = None, set=None) -> np.ndarray:
        """dspi_pdm_fade_state: the fade words (fade_out_pos | (uint16)base << 16) of streams [first, first + count) (default: to the end), after
        writing `set` if given."""
        if count is None: count = self.n_streams - first
        get = np.zeros(count, dtype=np.uint32)
        if set is not None:
            set = np.ascontiguousarray(set, dtype=np.uint32)
            assert set.size == count
        self._ck(self.L.dspi_pdm_fade_state(self.h, first, count, set.ctypes.data if set is not None else None, get.ctypes.data), "pdm_fade_state")
        return get

    def pdm_host(self, sub: np.ndarray, tiled: bool = False) -> np.ndarray:
        """PDM sub output (dspi_pdm_modulate) on host arrays: sub int32 [streams][frames] -> uint32 [streams][frames][8];
        tiled: [tiles][frames][R] -> [tiles][frames][8][R]."""
        sub = np.ascontiguousarray(sub, dtype=np.int32)
        words = np.zeros(sub.shape[:2] + (8,) + sub.shape[2:], dtype=np.uint32)
        n_frames = sub.shape[1]
        self._ck(self.L.dspi_pdm_modulate(self.h, sub.ctypes.data, n_frames, words.ctypes.data, OUT_TILED if tiled else 0), "pdm_modulate")
        return words

    def pdm_device(self, sub_ptr: int, n_frames: int, words_ptr: int, tiled: bool = False):
        self._ck(self.L.dspi_pdm_modulate(self.h, sub_ptr, n_frames, words_ptr, MEM_DEVICE | (OUT_TILED if tiled else 0)), "pdm_modulate")

    def spdif_host(self, pairs: np.ndarray, block_pos: int = 0, tiled: bool = False):
        """S/PDIF subframes (dspi_spdif_encode) on host arrays: pairs int32 [streams][P][frames][2] -> uint32
        [streams][P][frames][4]; tiled: [tiles][2P][frames][R] -> [tiles][P][frames][4][R].  Returns (subframes, next_pos)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        if tiled:
            nt, O, F, R = pairs.shape
            out = np.zeros((nt, O // 2, F, 4, R), dtype=np.uint32)
        else:
            S, P, F, _ = pairs.shape
            out = np.zeros((S, P, F, 4), dtype=np.uint32)
        nxt = self.L.dspi_spdif_encode(self.h, pairs.ctypes.data, F, block_pos, out.ctypes.data, OUT_TILED if tiled else 0)
        self._ck(min(nxt, 0), "spdif_encode")
        return out, nxt

    def i2s_host(self, pairs: np.ndarray, pair_mask: int = 0, out: np.ndarray | None = None, tiled: bool = False):
        """I2S slot words (dspi_i2s_encode) on host arrays shaped like the pair words; pair_mask 0 = the slots whose type is I2S.
        Returns (words, mask encoded); pairs outside the mask keep what `out` held (zeros when not given)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        F = pairs.shape[2]
        words = np.zeros(pairs.shape, dtype=np.uint32) if out is None else np.ascontiguousarray(out, dtype=np.uint32)
        m = self.L.dspi_i2s_encode(self.h, pairs.ctypes.data, F, pair_mask, words.ctypes.data, OUT_TILED if tiled else 0)
        self._ck(min(m, 0), "i2s_encode")
        return words, m

    def i2s_device(self, pairs_ptr: int, n_frames: int, pair_mask: int, out_ptr: int, tiled: bool = False) -> int:
        m = self.L.dspi_i2s_encode(self.h, pairs_ptr, n_frames, pair_mask, out_ptr, MEM_DEVICE | (OUT_TILED if tiled else 0))
        self._ck(min(m, 0), "i2s_encode")
        return m

    def spdif_device(self, pairs_ptr: int, n_frames: int, block_pos: int, out_ptr: int, tiled: bool = False) -> int:
        nxt = self.L.dspi_spdif_encode(self.h, pairs_ptr, n_frames, block_pos, out_ptr, MEM_DEVICE | (OUT_TILED if tiled else 0))
        self._ck(min(nxt, 0), "spdif_encode")
        return nxt

    def spdif_encode_v_host(self, pairs: np.ndarray, block_pos, tiled: bool = False) -> np.ndarray:
        """dspi_spdif_encode_v on host arrays: spdif_host with one starting position per stream, block_pos uint32 [n_streams] (each 0..191).
        Returns the subframes; the next positions are (block_pos + frames) % 192."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        pos = np.ascontiguousarray(np.asarray(block_pos, dtype=np.uint32).reshape(-1))
        assert len(pos) == self.n_streams, (len(pos), self.n_streams)
        if tiled:
            nt, O, F, R = pairs.shape
            out = np.zeros((nt, O // 2, F, 4, R), dtype=np.uint32)
        else:
            S, P, F, _ = pairs.shape
            out = np.zeros((S, P, F, 4), dtype=np.uint32)
        self._ck(self.L.dspi_spdif_encode_v(self.h, pairs.ctypes.data, F, pos.ctypes.data, out.ctypes.data, OUT_TILED if tiled else 0), "spdif_encode_v")
        return out

    def spdif_encode_v_device(self, pairs_ptr: int, n_frames: int, block_pos_ptr: int, out_ptr: int, tiled: bool = False):
        """dspi_spdif_encode_v on device pointers (block_pos: uint32 [n_streams] in device memory, taken modulo 192); asynchronous, see sync()."""
        self._ck(self.L.dspi_spdif_encode_v(self.h, pairs_ptr, n_frames, block_pos_ptr, out_ptr, MEM_DEVICE | (OUT_TILED if tiled else 0)), "spdif_encode_v")

    # ---- S/PDIF and I2S slots in one call, per device (include/dspi.h: dspi_process_wire / dspi_wire_encode) ----
    def process_wire_host(self, pcm: np.ndarray, n_blocks: int, block_len: int, bit_depth: int = 16, want_sub=True, want_peaks=True, enabled_only=False,
                          clip=False, pdm=False):
        """dspi_process_wire on host arrays: (wire, sub, peaks) — wire uint32 [S][P][F][4] in the wire layout: an S/PDIF slot's region holds its
        F x 4 subframe words, an I2S slot's region F x 2 slot words in its first half (wire[s, p].reshape(-1)[:2 * F]) and zeros behind.
        pdm=True: (wire, sub, peaks, words) with the PDM words uint32 [S][F][8].  clip=True: self.last_clip as after process_host."""
        S, F = self.n_streams, n_blocks * block_len
        pcm = np.ascontiguousarray(pcm)
        assert pcm.nbytes == S * F * (6 if bit_depth == 24 else 4), (pcm.shape, S, F)
        wire = np.zeros((S, self.P, F, 4), dtype=np.uint32)
        sub = np.zeros((S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        words = np.zeros((S, F, 8), dtype=np.uint32) if pdm else None
        self.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        out = _Out(wire.ctypes.data, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, self.last_clip.ctypes.data if clip else None)
        self._ck(self.L.dspi_process_wire(self.h, pcm.ctypes.data, bit_depth, n_blocks, block_len, C.byref(out), words.ctypes.data if pdm else None,
                                          (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_CLIP_FLAGS if clip else 0)), "process_wire")
        return (wire, sub, peaks, words) if pdm else (wire, sub, peaks)

    def process_wire_device(self, pcm_ptr: int, n_blocks: int, block_len: int, wire_ptr: int, bit_depth: int = 16, sub_ptr: int = 0, peaks_ptr: int = 0,
                            words_ptr: int = 0, enabled_only: bool = False, clip_ptr: int = 0):
        """dspi_process_wire on raw device pointers (wire: uint32 [S][P][F][4]; the second half of an I2S slot's region is not written);
        asynchronous, see sync()."""
        out = _Out(wire_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_wire(self.h, pcm_ptr, bit_depth, n_blocks, block_len, C.byref(out), words_ptr or None,
                                          MEM_DEVICE | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_wire")

    def wire_encode_host(self, pairs: np.ndarray, block_pos) -> np.ndarray:
        """dspi_wire_encode on host arrays: pairs int32 [S][P][F][2], block_pos uint32 [S] (each 0..191) -> uint32 [S][P][F][4] in the wire layout
        (process_wire_host), every stream's types and rate its own."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        pos = np.ascontiguousarray(np.asarray(block_pos, dtype=np.uint32).reshape(-1))
        assert len(pos) == self.n_streams, (len(pos), self.n_streams)
        S, P, F, _ = pairs.shape
        out = np.zeros((S, P, F, 4), dtype=np.uint32)
        self._ck(self.L.dspi_wire_encode(self.h, pairs.ctypes.data, F, pos.ctypes.data, out.ctypes.data, 0), "wire_encode")
        return out

    def wire_encode_device(self, pairs_ptr: int, n_frames: int, block_pos_ptr: int, out_ptr: int):
        """dspi_wire_encode on device pointers (block_pos: uint32 [S] in device memory, taken modulo 192); asynchronous, see sync()."""
        self._ck(self.L.dspi_wire_encode(self.h, pairs_ptr, n_frames, block_pos_ptr, out_ptr, MEM_DEVICE), "wire_encode")

    # ---- wire words on tiled and mixed-depth contexts (include/dspi.h: dspi_process_devices / dspi_wire_encode_tiled) ----
    def process_devices_host(self, pcm: np.ndarray, bit_depths, n_blocks: int, block_len: int, want_sub=True, want_peaks=True, tiled=False, enabled_only=False,
                             clip=False, pdm=False):
        """dspi_process_devices on host arrays: pcm and bit_depths as for process_mixed_host; returns (wire, sub, peaks), with pdm=True
        (wire, sub, peaks, words).  Stream-major: process_wire_host's arrays.  tiled=True: wire uint32 [tiles][P][F][4][R] in the tiled wire
        layout (untile_wire), sub [tiles][F][R], words [tiles][F][8][R].  clip=True: self.last_clip as after process_host."""
        S, F = self.n_streams, n_blocks * block_len
        d = self._depths(bit_depths)
        pcm = np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)
        if np.isin(d, (16, 24)).all(): assert pcm.nbytes == F * int(np.where(d == 24, 6, 4).sum()), (pcm.nbytes, S, F)      # (bad depths are the library's to refuse)
        R = self.tile_streams(); nt = (S + R - 1) // R
        wire = np.zeros((nt, self.P, F, 4, R) if tiled else (S, self.P, F, 4), dtype=np.uint32)
        sub = np.zeros((nt, F, R) if tiled else (S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        words = np.zeros((nt, F, 8, R) if tiled else (S, F, 8), dtype=np.uint32) if pdm else None
        self.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        out = _Out(wire.ctypes.data, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, self.last_clip.ctypes.data if clip else None)
        self._ck(self.L.dspi_process_devices(self.h, pcm.ctypes.data, d.ctypes.data, n_blocks, block_len, C.byref(out), words.ctypes.data if pdm else None,
                                             (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_CLIP_FLAGS if clip else 0)), "process_devices")
        return (wire, sub, peaks, words) if pdm else (wire, sub, peaks)

    def process_devices_device(self, pcm_ptr: int, bit_depths, n_blocks: int, block_len: int, wire_ptr: int, sub_ptr: int = 0, peaks_ptr: int = 0, words_ptr: int = 0,
                               tiled: bool = False, enabled_only: bool = False, clip_ptr: int = 0):
        """dspi_process_devices on raw device pointers (the depths stay a host array); what no word reaches is not written; asynchronous, see sync()."""
        d = self._depths(bit_depths)
        out = _Out(wire_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_devices(self.h, pcm_ptr, d.ctypes.data, n_blocks, block_len, C.byref(out), words_ptr or None,
                                             MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_devices")

    def wire_encode_tiled_host(self, pairs_t: np.ndarray, block_pos) -> np.ndarray:
        """dspi_wire_encode_tiled on host arrays: pairs_t int32 [tiles][2P][F][R] (process_host(tiled=True)), block_pos uint32 [S] (each 0..191)
        -> uint32 [tiles][P][F][4][R] in the tiled wire layout (untile_wire), every stream's types and rate its own."""
        pairs_t = np.ascontiguousarray(pairs_t, dtype=np.int32)
        pos = np.ascontiguousarray(np.asarray(block_pos, dtype=np.uint32).reshape(-1))
        assert len(pos) == self.n_streams, (len(pos), self.n_streams)
        nt, O, F, R = pairs_t.shape
        assert O == 2 * self.P and R == self.tile_streams() and nt == (self.n_streams + R - 1) // R, pairs_t.shape
        out = np.zeros((nt, self.P, F, 4, R), dtype=np.uint32)
        self._ck(self.L.dspi_wire_encode_tiled(self.h, pairs_t.ctypes.data, F, pos.ctypes.data, out.ctypes.data, 0), "wire_encode_tiled")
        return out

    def wire_encode_tiled_device(self, pairs_ptr: int, n_frames: int, block_pos_ptr: int, out_ptr: int):
        """dspi_wire_encode_tiled on device pointers (block_pos: uint32 [S] in device memory, taken modulo 192); asynchronous, see sync()."""
        self._ck(self.L.dspi_wire_encode_tiled(self.h, pairs_ptr, n_frames, block_pos_ptr, out_ptr, MEM_DEVICE), "wire_encode_tiled")

    # ---- S/PDIF input (include/dspi.h: dspi_spdif_decode / dspi_process_sources) ----
    def spdif_decode_host(self, subframes: np.ndarray, rx: np.ndarray) -> np.ndarray:
        """dspi_spdif_decode on host arrays: subframes uint32 [lines][F][4], rx SPDIF_RX [lines] (updated in place) -> pairs int32 [lines][F][2]."""
        sub = np.ascontiguousarray(subframes, dtype=np.uint32)
        lines, F, _ = sub.shape
        assert rx.dtype == SPDIF_RX and rx.flags.c_contiguous and rx.size == lines, (rx.dtype, rx.shape)
        pairs = np.zeros((lines, F, 2), dtype=np.int32)
        self._ck(self.L.dspi_spdif_decode(self.h, sub.ctypes.data, lines, F, rx.ctypes.data, pairs.ctypes.data, 0), "spdif_decode")
        return pairs

    def spdif_decode_device(self, sub_ptr: int, n_lines: int, n_frames: int, rx_ptr: int, pairs_ptr: int):
        """dspi_spdif_decode on device pointers (16-byte aligned); asynchronous, see sync()."""
        self._ck(self.L.dspi_spdif_decode(self.h, sub_ptr, n_lines, n_frames, rx_ptr, pairs_ptr, MEM_DEVICE), "spdif_decode")

    def sources_bytes(self, sources, n_blocks: int, block_len: int):
        """dspi_sources_bytes: (total bytes, offsets uint64 [n_streams + 1]) of the input of a dspi_process_sources call (sources uint8
        [n_streams], each SRC_PCM16, SRC_PCM24 or SRC_SPDIF; an S/PDIF run starts at a multiple of 16).  Works on host-only contexts."""
        d = self._depths(sources)
        total, off = C.c_uint64(0), np.zeros(self.n_streams + 1, dtype=np.uint64)
        self._ck(self.L.dspi_sources_bytes(self.h, d.ctypes.data, n_blocks, block_len, C.byref(total), off.ctypes.data), "sources_bytes")
        return total.value, off

    def process_sources_host(self, data: np.ndarray, sources, n_blocks: int, block_len: int, rx: np.ndarray | None = None, want_pairs=True, want_sub=True, want_peaks=True,
                             tiled=False, enabled_only=False, spdif=False, wire=False, clip=False, pdm=False):
        """dspi_process_sources on host arrays: data = one flat uint8 array laid out as sources_bytes says, rx = SPDIF_RX [n_streams] (updated in
        place; may be None without an S/PDIF source).  Returns process_mixed_host's arrays; with wire=True (DSPI_OUT_WIRE) `pairs` is
        process_devices_host's wire array."""
        S, F = self.n_streams, n_blocks * block_len
        d = self._depths(sources)
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if rx is not None: assert rx.dtype == SPDIF_RX and rx.flags.c_contiguous and rx.size == S, (rx.dtype, rx.shape)
        R = self.tile_streams(); nt = (S + R - 1) // R
        if wire: pairs = np.zeros((nt, self.P, F, 4, R) if tiled else (S, self.P, F, 4), dtype=np.uint32)
        elif tiled: pairs = np.zeros((nt, self.P * 2, F, R), dtype=np.int32) if want_pairs else None
        else: pairs = (np.zeros((S, self.P, F, 4), dtype=np.uint32) if spdif else np.zeros((S, self.P, F, 2), dtype=np.int32)) if want_pairs else None
        sub = np.zeros((nt, F, R) if tiled else (S, F), dtype=np.int32) if want_sub else None
        peaks = np.zeros((S, n_blocks, self.C), dtype=np.uint16) if want_peaks else None
        words = np.zeros((nt, F, 8, R) if tiled else (S, F, 8), dtype=np.uint32) if pdm else None
        self.last_clip = np.zeros(S, dtype=np.uint16) if clip else None
        out = _Out(pairs.ctypes.data if pairs is not None else None, sub.ctypes.data if want_sub else None, peaks.ctypes.data if want_peaks else None, self.last_clip.ctypes.data if clip else None)
        self._ck(self.L.dspi_process_sources(self.h, data.ctypes.data, d.ctypes.data, n_blocks, block_len, C.byref(out), words.ctypes.data if pdm else None,
                                             rx.ctypes.data if rx is not None else None,
                                             (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_WIRE if wire else 0) |
                                             (OUT_CLIP_FLAGS if clip else 0)), "process_sources")
        return (pairs, sub, peaks, words) if pdm else (pairs, sub, peaks)

    def process_sources_device(self, in_ptr: int, sources, n_blocks: int, block_len: int, rx_ptr: int = 0, pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0,
                               words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, wire: bool = False, clip_ptr: int = 0):
        """dspi_process_sources on raw device pointers (the sources stay a host array; rx: SPDIF_RX [n_streams] in device memory); asynchronous, see sync()."""
        d = self._depths(sources)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_sources(self.h, in_ptr, d.ctypes.data, n_blocks, block_len, C.byref(out), words_ptr or None, rx_ptr or None,
                                             MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_WIRE if wire else 0) |
                                             (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_sources")

    def debug_sources_intake(self, in_ptr: int, sources, n_blocks: int, block_len: int, rx_ptr: int = 0):
        """dspi_debug_sources_intake: the intake and the receiver of process_sources_device alone, into the context's scratch; asynchronous, see sync()."""
        d = self._depths(sources)
        self._ck(self.L.dspi_debug_sources_intake(self.h, in_ptr, d.ctypes.data, n_blocks, block_len, rx_ptr or None), "debug_sources_intake")

    # ---- chained devices (include/dspi.h: dspi_wire_decode / dspi_process_linked) ----
    def wire_view_of(self, wire_ptr: int, n_frames: int, tiled: bool = False) -> np.ndarray:
        """dspi_wire_view_of: a WIRE_VIEW record (0-d array) of a buffer THIS context wrote, or will write, in the wire layout (tiled: the tiled
        one); producer = this context.  Bookkeeping only: works on host-only contexts, wire_ptr may be a host or a device address."""
        v = np.zeros((), dtype=WIRE_VIEW)
        self._ck(self.L.dspi_wire_view_of(self.h, wire_ptr or None, n_frames, OUT_TILED if tiled else 0, v.ctypes.data), "wire_view_of")
        return v

    def link_kinds(self, lines) -> np.ndarray:
        """dspi_link_kinds: LINK [n] naming `lines` (stream * pairs + pair of THIS context), each kind from its stream's current output type."""
        links = np.zeros(len(lines), dtype=LINK)
        links["line"] = lines
        self._ck(self.L.dspi_link_kinds(self.h, links.ctypes.data, len(links)), "link_kinds")
        return links

    @staticmethod
    def _links(links) -> np.ndarray:
        links = np.ascontiguousarray(links)
        assert links.dtype == LINK and links.ndim == 1, (links.dtype, links.shape)
        return links

    def wire_decode_host(self, view: np.ndarray, wire: np.ndarray, links, rx: np.ndarray | None, pairs: np.ndarray | None = None) -> np.ndarray:
        """dspi_wire_decode on host arrays: `wire` = the buffer `view` describes (its address is put into a copy of the view), links LINK [n],
        rx SPDIF_RX [n] (updated in place; may be None without an S/PDIF link) -> pairs int32 [n][F][2] (given: only the links' entries are written)."""
        links = self._links(links)
        wire = np.ascontiguousarray(wire, dtype=np.uint32)
        v = view.copy(); v["wire"] = wire.ctypes.data
        F = int(v["n_frames"])
        if rx is not None: assert rx.dtype == SPDIF_RX and rx.flags.c_contiguous and rx.size == len(links), (rx.dtype, rx.shape)
        if pairs is None: pairs = np.zeros((len(links), F, 2), dtype=np.int32)
        assert pairs.dtype == np.int32 and pairs.flags.c_contiguous and pairs.shape == (len(links), F, 2), pairs.shape
        self._ck(self.L.dspi_wire_decode(self.h, v.ctypes.data, links.ctypes.data, len(links), rx.ctypes.data if rx is not None else None, pairs.ctypes.data, 0), "wire_decode")
        return pairs

    def wire_decode_device(self, view: np.ndarray, links, rx_ptr: int, pairs_ptr: int):
        """dspi_wire_decode on device pointers (view["wire"], rx and pairs 16-byte aligned; the links stay a host array); asynchronous, see sync()."""
        links = self._links(links)
        self._ck(self.L.dspi_wire_decode(self.h, view.ctypes.data, links.ctypes.data, len(links), rx_ptr or None, pairs_ptr, MEM_DEVICE), "wire_decode")

    def process_linked_device(self, view: np.ndarray, links, n_blocks: int, block_len: int, rx_ptr: int = 0, pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0,
                              words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, wire: bool = False, clip_ptr: int = 0):
        """dspi_process_linked on raw device pointers: stream s of this context takes its frames from links[s] (LINK [n_streams], a host array) of
        the device buffer `view` describes; rx: SPDIF_RX [n_streams] in device memory.  With view["producer"] set the call waits for the
        producer's stream itself.  Asynchronous, see sync()."""
        links = self._links(links)
        assert len(links) == self.n_streams, (len(links), self.n_streams)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_linked(self.h, view.ctypes.data, links.ctypes.data, n_blocks, block_len, C.byref(out), words_ptr or None, rx_ptr or None,
                                            MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_WIRE if wire else 0) |
                                            (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_linked")

    # ---- the patch bay (include/dspi.h: dspi_process_patched) ----
    def patched_bytes(self, sources, n_blocks: int, block_len: int):
        """dspi_patched_bytes: (total bytes, offsets uint64 [n_streams + 1]) of `in` of a dspi_process_patched call: sources_bytes in which a
        SRC_LINK stream occupies no bytes.  Works on host-only contexts."""
        d = self._depths(sources)
        total, off = C.c_uint64(0), np.zeros(self.n_streams + 1, dtype=np.uint64)
        self._ck(self.L.dspi_patched_bytes(self.h, d.ctypes.data, n_blocks, block_len, C.byref(total), off.ctypes.data), "patched_bytes")
        return total.value, off

    def _patch_args(self, sources, views, patches):
        d = self._depths(sources)
        views = np.ascontiguousarray(views).reshape(-1) if views is not None else None
        patches = np.ascontiguousarray(patches) if patches is not None else None
        if views is not None: assert views.dtype == WIRE_VIEW, views.dtype
        if patches is not None: assert patches.dtype == PATCH and patches.shape == (self.n_streams,), (patches.dtype, patches.shape)
        return d, views, patches

    def process_patched_device(self, in_ptr: int, sources, views, patches, n_blocks: int, block_len: int, rx_ptr: int = 0, pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0,
                               words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, wire: bool = False, clip_ptr: int = 0):
        """dspi_process_patched on raw device pointers: stream s takes its frames from its run of `in` (sources[s] = SRC_PCM16 / SRC_PCM24 /
        SRC_SPDIF, laid out as patched_bytes says) or, sources[s] = SRC_LINK, from line patches[s]["line"] of views[patches[s]["view"]] (WIRE_VIEW
        [n_views] and PATCH [n_streams], host arrays; both may be None without a LINK stream); rx: SPDIF_RX [n_streams] in device memory.  The
        call waits for the views' producers itself.  Asynchronous, see sync()."""
        d, views, patches = self._patch_args(sources, views, patches)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_patched(self.h, in_ptr or None, d.ctypes.data, views.ctypes.data if views is not None else None, len(views) if views is not None else 0,
                                             patches.ctypes.data if patches is not None else None, n_blocks, block_len, C.byref(out), words_ptr or None, rx_ptr or None,
                                             MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_WIRE if wire else 0) |
                                             (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_patched")

    def debug_patched_intake(self, in_ptr: int, sources, views, patches, n_blocks: int, block_len: int, rx_ptr: int = 0):
        """dspi_debug_patched_intake: everything process_patched_device runs in front of the chain, into the context's scratch; asynchronous, see sync()."""
        d, views, patches = self._patch_args(sources, views, patches)
        self._ck(self.L.dspi_debug_patched_intake(self.h, in_ptr or None, d.ctypes.data, views.ctypes.data if views is not None else None, len(views) if views is not None else 0,
                                                  patches.ctypes.data if patches is not None else None, n_blocks, block_len, rx_ptr or None), "debug_patched_intake")

    # ---- input from a packet table (include/dspi.h: dspi_process_packets) ----
    def _packet_table(self, table, n_blocks: int) -> np.ndarray:
        t = np.ascontiguousarray(table, dtype=np.uint64)
        assert t.size == self.n_streams * n_blocks, (t.shape, self.n_streams, n_blocks)
        return t

    def packets_check(self, bit_depths, table, n_blocks: int, block_len: int, arena_bytes: int):
        """dspi_packets_check: None when a dspi_process_packets call would accept this table (uint64 [n_streams][n_blocks], byte offsets in an arena
        of arena_bytes) and these depths; raises DspiError otherwise, after setting self.bad_entry to s * n_blocks + k of the entry refused (None
        when the refusal is not about an entry).  Works on host-only contexts."""
        d, t = self._depths(bit_depths), self._packet_table(table, n_blocks)
        bad = C.c_uint64(2 ** 64 - 1)
        rc = self.L.dspi_packets_check(self.h, d.ctypes.data, t.ctypes.data, n_blocks, block_len, arena_bytes, C.byref(bad))
        self.bad_entry = None if rc == 0 or bad.value == 2 ** 64 - 1 else bad.value
        self._ck(rc, "packets_check")

    def process_packets_device(self, arena_ptr: int, arena_bytes: int, bit_depths, table, n_blocks: int, block_len: int, pairs_ptr: int = 0, sub_ptr: int = 0, peaks_ptr: int = 0,
                               words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, wire: bool = False, clip_ptr: int = 0):
        """dspi_process_packets on raw device pointers: packet k of stream s is block_len frames at bit_depths[s] at arena_ptr + table[s][k] (the
        depths and the table stay host arrays; the table may be reused when this returns).  Otherwise process_mixed_device; wire=True
        (DSPI_OUT_WIRE): pairs in the wire layout, with tiled=True the tiled one.  Asynchronous, see sync()."""
        d, t = self._depths(bit_depths), self._packet_table(table, n_blocks)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_packets(self.h, arena_ptr, arena_bytes, d.ctypes.data, t.ctypes.data, n_blocks, block_len, C.byref(out), words_ptr or None,
                                             MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) | (OUT_WIRE if wire else 0) |
                                             (OUT_CLIP_FLAGS if clip_ptr else 0)), "process_packets")

    def debug_packets_intake(self, arena_ptr: int, arena_bytes: int, bit_depths, table, n_blocks: int, block_len: int):
        """dspi_debug_packets_intake: what process_packets_device runs in front of the chain, into the context's scratch; asynchronous, see sync()."""
        d, t = self._depths(bit_depths), self._packet_table(table, n_blocks)
        self._ck(self.L.dspi_debug_packets_intake(self.h, arena_ptr, arena_bytes, d.ctypes.data, t.ctypes.data, n_blocks, block_len), "debug_packets_intake")

    # ---- outputs to a packet table (include/dspi.h: dspi_packets_emit) ----
    def _formats(self, formats) -> np.ndarray:
        f = np.ascontiguousarray(np.asarray(formats, dtype=np.uint8).reshape(-1))
        assert f.size == self.n_streams, (f.size, self.n_streams)
        return f

    def _emit_table(self, table, n_blocks: int) -> np.ndarray:
        t = np.ascontiguousarray(table, dtype=np.uint64)
        assert t.size == self.n_streams * self.P * n_blocks, (t.shape, self.n_streams, self.P, n_blocks)
        return t

    def packets_emit_check(self, formats, table, n_blocks: int, block_len: int, arena_bytes: int, overlap: bool = False):
        """dspi_packets_emit_check: None when a dspi_packets_emit call would accept this table (uint64 [n_streams][n_pairs][n_blocks], byte offsets
        in an arena of arena_bytes, or PACKET_SKIP) and these formats (24 or 32 per stream), and, overlap=True, no two entries share a byte; raises
        DspiError otherwise, after setting self.bad_entry to the index of the entry refused (None when the refusal is not about an entry).
        Works on host-only contexts."""
        f, t = self._formats(formats), self._emit_table(table, n_blocks)
        bad = C.c_uint64(2 ** 64 - 1)
        rc = self.L.dspi_packets_emit_check(self.h, f.ctypes.data, t.ctypes.data, n_blocks, block_len, arena_bytes, EMIT_CHECK_OVERLAP if overlap else 0, C.byref(bad))
        self.bad_entry = None if rc == 0 or bad.value == 2 ** 64 - 1 else bad.value
        self._ck(rc, "packets_emit_check")

    def packets_emit_host(self, pairs: np.ndarray, n_blocks: int, block_len: int, formats, table, arena: np.ndarray, tiled: bool = False) -> np.ndarray:
        """dspi_packets_emit on host arrays (the CPU path; works on host-only contexts): pairs int32 as a process call returned them
        ([S][P][F][2], tiled=True: [tiles][2 P][F][R]); arena uint8, written in place where the table's entries point, and returned."""
        f, t = self._formats(formats), self._emit_table(table, n_blocks)
        F, R = n_blocks * block_len, self.tile_streams()
        shape = ((self.n_streams + R - 1) // R, 2 * self.P, F, R) if tiled else (self.n_streams, self.P, F, 2)
        assert pairs.dtype == np.int32 and pairs.flags.c_contiguous and pairs.shape == shape, (pairs.shape, shape)
        assert arena.dtype == np.uint8 and arena.flags.c_contiguous and arena.ndim == 1
        self._ck(self.L.dspi_packets_emit(self.h, pairs.ctypes.data, n_blocks, block_len, f.ctypes.data, t.ctypes.data, arena.ctypes.data, arena.size, OUT_TILED if tiled else 0), "packets_emit")
        return arena

    def packets_emit_device(self, pairs_ptr: int, n_blocks: int, block_len: int, formats, table, arena_ptr: int, arena_bytes: int, tiled: bool = False):
        """dspi_packets_emit on raw device pointers (the formats and the table stay host arrays; the table may be reused when this returns).
        Asynchronous on the context's stream, behind the process call that wrote the pairs; see sync()."""
        f, t = self._formats(formats), self._emit_table(table, n_blocks)
        self._ck(self.L.dspi_packets_emit(self.h, pairs_ptr, n_blocks, block_len, f.ctypes.data, t.ctypes.data, arena_ptr, arena_bytes, MEM_DEVICE | (OUT_TILED if tiled else 0)), "packets_emit")

    def debug_packets_emit_launch(self, pairs_ptr: int, n_blocks: int, block_len: int, formats_ptr: int, table_ptr: int, arena_ptr: int, tiled: bool = False):
        """dspi_debug_packets_emit_launch: the one launch of packets_emit_device, formats and table already in DEVICE memory and unchecked; asynchronous"""
        self._ck(self.L.dspi_debug_packets_emit_launch(self.h, pairs_ptr, n_blocks, block_len, formats_ptr, table_ptr, arena_ptr, MEM_DEVICE | (OUT_TILED if tiled else 0)), "debug_packets_emit_launch")

    # ---- resident packet tables (include/dspi.h: dspi_process_packets_resident): the twins above with the table in DEVICE memory ----
    def packets_check_resident(self, bit_depths, table_ptr: int, n_blocks: int, block_len: int, arena_bytes: int):
        """dspi_packets_check_resident: packets_check on a table in device memory (table_ptr, 16-byte aligned), checked on the GPU and waited for;
        self.bad_entry as there.  Needs a device."""
        d = self._depths(bit_depths)
        bad = C.c_uint64(2 ** 64 - 1)
        rc = self.L.dspi_packets_check_resident(self.h, d.ctypes.data, table_ptr, n_blocks, block_len, arena_bytes, C.byref(bad))
        self.bad_entry = None if rc == 0 or bad.value == 2 ** 64 - 1 else bad.value
        self._ck(rc, "packets_check_resident")

    def packets_emit_check_resident(self, formats, table_ptr: int, n_blocks: int, block_len: int, arena_bytes: int):
        """dspi_packets_emit_check_resident: packets_emit_check (without the overlap rule) on a table in device memory; self.bad_entry as there"""
        f = self._formats(formats)
        bad = C.c_uint64(2 ** 64 - 1)
        rc = self.L.dspi_packets_emit_check_resident(self.h, f.ctypes.data, table_ptr, n_blocks, block_len, arena_bytes, 0, C.byref(bad))
        self.bad_entry = None if rc == 0 or bad.value == 2 ** 64 - 1 else bad.value
        self._ck(rc, "packets_emit_check_resident")

    def process_packets_resident_device(self, arena_ptr: int, arena_bytes: int, bit_depths, table_ptr: int, n_blocks: int, block_len: int, pairs_ptr: int = 0, sub_ptr: int = 0,
                                        peaks_ptr: int = 0, words_ptr: int = 0, tiled: bool = False, enabled_only: bool = False, spdif: bool = False, wire: bool = False,
                                        clip_ptr: int = 0, checked: bool = False):
        """dspi_process_packets_resident: process_packets_device with the table in device memory (the depths stay a host array).  checked=False:
        the entries are checked on the GPU first and the call waits for that answer; checked=True (DSPI_TABLE_CHECKED): the caller warrants that
        packets_check_resident accepted this table with these arguments and that no stream was resumed since; fully asynchronous, see sync()."""
        d = self._depths(bit_depths)
        out = _Out(pairs_ptr or None, sub_ptr or None, peaks_ptr or None, clip_ptr or None)
        self._ck(self.L.dspi_process_packets_resident(self.h, arena_ptr, arena_bytes, d.ctypes.data, table_ptr, n_blocks, block_len, C.byref(out), words_ptr or None,
                                                      MEM_DEVICE | (OUT_TILED if tiled else 0) | (OUT_ENABLED_ONLY if enabled_only else 0) | (OUT_SPDIF if spdif else 0) |
                                                      (OUT_WIRE if wire else 0) | (OUT_CLIP_FLAGS if clip_ptr else 0), TABLE_CHECKED if checked else 0), "process_packets_resident")

    def packets_emit_resident_device(self, pairs_ptr: int, n_blocks: int, block_len: int, formats, table_ptr: int, arena_ptr: int, arena_bytes: int, tiled: bool = False,
                                     checked: bool = False):
        """dspi_packets_emit_resident: packets_emit_device with the table in device memory (the formats stay a host array); checked as in
        process_packets_resident_device, the warrant being packets_emit_check_resident's"""
        f = self._formats(formats)
        self._ck(self.L.dspi_packets_emit_resident(self.h, pairs_ptr, n_blocks, block_len, f.ctypes.data, table_ptr, arena_ptr, arena_bytes, MEM_DEVICE | (OUT_TILED if tiled else 0),
                                                   TABLE_CHECKED if checked else 0), "packets_emit_resident")

    def debug_table_check_launch(self, kind: int, kinds_ptr: int, table_ptr: int, n_blocks: int, block_len: int, arena_bytes: int):
        """dspi_debug_table_check_launch: the checker's one launch alone (kind 0: input table and depths, 1: emit table and formats; both in
        DEVICE memory); the answer is not read; asynchronous"""
        self._ck(self.L.dspi_debug_table_check_launch(self.h, kind, kinds_ptr, table_ptr, n_blocks, block_len, arena_bytes), "debug_table_check_launch")

    def pdm_restart(self, stream: int = ALL):
        self._ck(self.L.dspi_pdm_restart(self.h, stream), "pdm_restart")

    # ---- stream snapshots (include/dspi.h: dspi_export_streams / dspi_import_streams) ----
    def snapshot_sizes(self, first: int, count: int):
        """(head_bytes, state_bytes) an export of streams [first, first + count) needs.  Works on host-only contexts."""
        hb, sb = C.c_size_t(0), C.c_size_t(0)
        self._ck(self.L.dspi_snapshot_sizes(self.h, first, count, C.byref(hb), C.byref(sb)), "snapshot_sizes")
        return hb.value, sb.value

    def export_streams(self, first: int, count: int):
        """The complete state of streams [first, first + count): (head: bytes, state: uint32 [count][record words]).  The context is unchanged."""
        hb, sb = self.snapshot_sizes(first, count)
        head = C.create_string_buffer(hb)
        state = np.zeros((count, sb // (4 * count)), dtype=np.uint32)
        snap = _Snapshot(C.addressof(head), hb, state.ctypes.data, sb)
        self._ck(self.L.dspi_export_streams(self.h, first, count, C.byref(snap), 0), "export_streams")
        return head.raw, state

    def import_streams(self, first: int, head: bytes, state: np.ndarray, realign: bool = False) -> int:
        """Overwrites streams [first, first + n) with a snapshot's n streams (n from the head); returns n.  A refused snapshot
        (DspiError) leaves the context as it was.  realign: DSPI_SNAP_REALIGN, every stream takes its destination row's write positions."""
        state = np.ascontiguousarray(state, dtype=np.uint32)
        hbuf = C.create_string_buffer(bytes(head), len(head))
        snap = _Snapshot(C.addressof(hbuf), len(head), state.ctypes.data, state.nbytes)
        return self._ck(self.L.dspi_import_streams(self.h, first, C.byref(snap), SNAP_REALIGN if realign else 0), "import_streams")

    def export_streams_device(self, first: int, count: int, state_ptr: int, state_bytes: int) -> bytes:
        """export_streams with the records in device memory (16-byte aligned, e.g. torch.Tensor.data_ptr()); asynchronous on the
        context's stream: sync() before another context imports them.  Returns the head."""
        hb, _ = self.snapshot_sizes(first, count)
        head = C.create_string_buffer(hb)
        snap = _Snapshot(C.addressof(head), hb, state_ptr, state_bytes)
        self._ck(self.L.dspi_export_streams(self.h, first, count, C.byref(snap), MEM_DEVICE), "export_streams")
        return head.raw

    def import_streams_device(self, first: int, head: bytes, state_ptr: int, state_bytes: int, realign: bool = False) -> int:
        """import_streams from records in device memory; asynchronous on the context's stream (also with realign)."""
        hbuf = C.create_string_buffer(bytes(head), len(head))
        snap = _Snapshot(C.addressof(hbuf), len(head), state_ptr, state_bytes)
        return self._ck(self.L.dspi_import_streams(self.h, first, C.byref(snap), MEM_DEVICE | (SNAP_REALIGN if realign else 0)), "import_streams")

    def realign_streams(self, first: int, count: int) -> int:
        """dspi_realign_streams: streams [first, first + count) take their rows' write positions, in place; asynchronous on the context's stream."""
        return self._ck(self.L.dspi_realign_streams(self.h, first, count), "realign_streams")

    def stream_positions(self, first: int, count: int):
        """dspi_debug_stream_positions: (delay write index, leveller ring position) of streams [first, first + count), uint32 [count] each, masked."""
        w, r = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
        self._ck(self.L.dspi_debug_stream_positions(self.h, first, count, w.ctypes.data, r.ctypes.data), "debug_stream_positions")
        return w, r

    # ---- paused streams (include/dspi.h: devices that receive no packet in a call) ----
    def pause_streams(self, first: int, count: int) -> int:
        """dspi_pause_streams: streams [first, first + count) sit out every dspi_process from the next one on, their state frozen."""
        return self._ck(self.L.dspi_pause_streams(self.h, first, count), "pause_streams")

    def resume_streams(self, first: int, count: int, as_is: bool = False) -> int:
        """dspi_resume_streams: the paused streams of the range take part again, realigned to their rows' write positions (as_is:
        DSPI_RESUME_AS_IS, they keep their own)."""
        return self._ck(self.L.dspi_resume_streams(self.h, first, count, RESUME_AS_IS if as_is else 0), "resume_streams")

    def streams_paused(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """dspi_streams_paused: uint8 [count], 1 = paused (default: the whole context)."""
        count = self.n_streams - first if count is None else count
        p = np.zeros(count, dtype=np.uint8)
        self._ck(self.L.dspi_streams_paused(self.h, first, count, p.ctypes.data), "streams_paused")
        return p

    # ---- stream moves (include/dspi.h: a stream changes its slot inside its context) ----
    def move_streams(self, moves, as_is: bool = False) -> int:
        """dspi_move_streams: moves = [(src, dst), ...] (or an (n, 2) array); slot dst takes the stream slot src held, all entries at once,
        realigned to its destination row (as_is: DSPI_MOVE_AS_IS, it keeps its own write positions).  Returns the entries applied."""
        m = np.ascontiguousarray(np.asarray(moves, dtype=np.uint32).reshape(-1, 2))
        return self._ck(self.L.dspi_move_streams(self.h, m.ctypes.data if len(m) else None, len(m), MOVE_AS_IS if as_is else 0), "move_streams")

    def plan_compaction(self, one_way: bool = False) -> np.ndarray:
        """dspi_plan_compaction: the (src, dst) list, uint32 [n][2], after which the active streams fill the lowest slots (one_way:
        DSPI_COMPACT_ONE_WAY, paused slots are free and not preserved).  Works on host-only contexts."""
        flags = COMPACT_ONE_WAY if one_way else 0
        n = self._ck(self.L.dspi_plan_compaction(self.h, None, 0, flags), "plan_compaction")
        m = np.zeros((n, 2), dtype=np.uint32)
        if n: self._ck(self.L.dspi_plan_compaction(self.h, m.ctypes.data, n, flags), "plan_compaction")
        return m

    # ---- migration (include/dspi.h: streams change their context; self is the SOURCE context) ----
    def migrate_streams(self, dst: "Dspi", moves, as_is: bool = False, paused: bool = False) -> int:
        """dspi_migrate_streams: moves = [(src, dst), ...] (or an (n, 2) array); slot dst of the context `dst` takes the stream slot src of this
        context held, all entries at once, realigned to its destination row (as_is: DSPI_MIGRATE_AS_IS) and as active as it was (paused:
        DSPI_MIGRATE_PAUSED, it arrives paused).  The source slots stay behind paused.  Returns the entries applied."""
        m = np.ascontiguousarray(np.asarray(moves, dtype=np.uint32).reshape(-1, 2))
        return self._ck(self.L.dspi_migrate_streams(self.h, dst.h, m.ctypes.data if len(m) else None, len(m),
                                                    (MIGRATE_AS_IS if as_is else 0) | (MIGRATE_PAUSED if paused else 0)), "migrate_streams")

    def plan_migration(self, dst: "Dspi", want: int) -> np.ndarray:
        """dspi_plan_migration: the (src, dst) list, uint32 [k][2], that shifts k = min(want, active streams here, paused slots of `dst`)
        streams from the top of this context into the lowest paused slots of `dst`.  Works on host-only contexts."""
        n = self._ck(self.L.dspi_plan_migration(self.h, dst.h, want, None, 0, 0), "plan_migration")
        m = np.zeros((n, 2), dtype=np.uint32)
        if n: self._ck(self.L.dspi_plan_migration(self.h, dst.h, want, m.ctypes.data, n, 0), "plan_migration")
        return m

    def plan_grouping(self, one_way: bool = False) -> np.ndarray:
        """dspi_plan_grouping: the (src, dst) list, uint32 [n][2], after which the active streams fill the lowest slots, those of one parameter
        object in one run and runs of one structure side by side (one_way: DSPI_GROUP_ONE_WAY, paused slots are free and not preserved).
        Equal parameter objects are folded first.  Works on host-only contexts."""
        flags = GROUP_ONE_WAY if one_way else 0
        n = self._ck(self.L.dspi_plan_grouping(self.h, None, 0, flags), "plan_grouping")
        m = np.zeros((n, 2), dtype=np.uint32)
        if n: self._ck(self.L.dspi_plan_grouping(self.h, m.ctypes.data, n, flags), "plan_grouping")
        return m

    # ---- stream boots (include/dspi.h: a slot is power-cycled inside its running context) ----
    def device_flash(self, enable: int = -1) -> int:
        """dspi_device_flash: every stream owns a 48 KB preset area and the preset directory requests are served from it (enable < 0: only
        read the mode).  Host memory only: no kernel, nothing per dspi_process call."""
        return self._ck(self.L.dspi_device_flash(self.h, enable), "device_flash")

    def flash_read(self, stream: int) -> bytes:
        """dspi_flash_read: the stream's own flash (mode on only)"""
        buf = C.create_string_buffer(FLASH_DUMP_BYTES)
        self._ck(self.L.dspi_flash_read(self.h, stream, buf, FLASH_DUMP_BYTES), "flash_read")
        return buf.raw

    def flash_write(self, first: int, count: int, dump: bytes) -> int:
        """dspi_flash_write: one image for [first, first + count) as one shared object; boots nothing"""
        return self._ck(self.L.dspi_flash_write(self.h, first, count, dump, len(dump)), "flash_write")

    def boot_streams(self, streams, dump: bytes | None = None, as_is: bool = False, own_flash: bool = False) -> int:
        """dspi_boot_streams: every listed slot becomes a device that has just been powered on — dspi_create's own (dump None) or one that
        boots from the 48 KB preset area `dump` — on its row's write positions (as_is: DSPI_BOOT_STREAMS_AS_IS, on the power-on positions).
        own_flash: DSPI_BOOT_STREAMS_OWN_FLASH, every listed slot reboots from its own flash (dspi_device_flash).
        Returns preset_boot_load's selection (dspi_load_flash_dump's codes; 48 without a dump).  Works on host-only contexts."""
        s = np.ascontiguousarray(np.asarray(streams, dtype=np.uint32).reshape(-1))
        sel = C.c_int(-1)
        n = self._ck(self.L.dspi_boot_streams(self.h, s.ctypes.data if len(s) else None, len(s), dump, len(dump) if dump is not None else 0,
                                              (BOOT_STREAMS_AS_IS if as_is else 0) | (BOOT_STREAMS_OWN_FLASH if own_flash else 0), C.byref(sel)), "boot_streams")
        assert n == len(s)
        return sel.value

    # ---- resizing (include/dspi.h: a context gains and gives back slots) ----
    def resize_streams(self, n: int, paused: bool = False) -> int:
        """dspi_resize_streams: the context holds n streams from now on.  Growing: slots [old, n) are devices that have just been powered on
        (paused: DSPI_RESIZE_PAUSED, they arrive paused); shrinking: every slot of [n, old) must be paused.  self.n_streams follows.
        Works on host-only contexts."""
        self.n_streams = self._ck(self.L.dspi_resize_streams(self.h, n, RESIZE_PAUSED if paused else 0), "resize_streams")
        return self.n_streams

    def reserve_streams(self, n: int) -> int:
        """dspi_reserve_streams: room for n streams (whole rows), more than now or less; returns the new capacity in streams."""
        return self._ck(self.L.dspi_reserve_streams(self.h, n), "reserve_streams")

    def stream_capacity(self) -> int:
        """dspi_stream_capacity: the streams the context's arrays have room for (rows x tile_streams())."""
        return int(self.L.dspi_stream_capacity(self.h))

    # ---- the meter bridge (include/dspi.h: meter ballistics, alarms and status for every stream of a context) ----
    def meters_update_host(self, peaks: np.ndarray, meters: np.ndarray, hold_packets: int, decay_q15: int) -> np.ndarray:
        """dspi_meters_update on host arrays (the CPU path): peaks uint16 [S][blocks][C] as a process call returned them, meters uint32 [S][C]
        (level | count << 16), updated in place and returned."""
        S = self.n_streams
        assert peaks.dtype == np.uint16 and peaks.flags.c_contiguous and peaks.ndim == 3 and peaks.shape[0] == S and peaks.shape[2] == self.C, peaks.shape
        assert meters.dtype == np.uint32 and meters.flags.c_contiguous and meters.shape == (S, self.C), meters.shape
        self._ck(self.L.dspi_meters_update(self.h, peaks.ctypes.data, peaks.shape[1], hold_packets, decay_q15, meters.ctypes.data, 0), "meters_update")
        return meters

    def meters_update_device(self, peaks_ptr: int, n_blocks: int, meters_ptr: int, hold_packets: int, decay_q15: int):
        """dspi_meters_update on device pointers: asynchronous on the context's stream, behind the process call that wrote the peaks"""
        self._ck(self.L.dspi_meters_update(self.h, peaks_ptr, n_blocks, hold_packets, decay_q15, meters_ptr, MEM_DEVICE), "meters_update")

    def meters_alarms_host(self, meters: np.ndarray | None, level_q15: int, cap: int | None = None, want_info: bool = True):
        """dspi_meters_alarms on host arrays: (streams uint32 [written], info uint32 [written] or None, total).  meters None: clip-only alarms;
        cap: the list's room (default: every stream)."""
        cap = self.n_streams if cap is None else cap
        streams, info, total = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32) if want_info else None, C.c_uint32(0)
        if meters is not None: assert meters.dtype == np.uint32 and meters.flags.c_contiguous and meters.shape == (self.n_streams, self.C), meters.shape
        n = self._ck(self.L.dspi_meters_alarms(self.h, meters.ctypes.data if meters is not None else None, level_q15, streams.ctypes.data,
                                               info.ctypes.data if want_info else None, cap, C.byref(total), 0), "meters_alarms")
        return streams[:n], info[:n] if want_info else None, total.value

    def meters_alarms_device(self, meters_ptr: int, level_q15: int, streams_ptr: int, info_ptr: int, cap: int, total_ptr: int):
        """dspi_meters_alarms on device pointers (meters_ptr / info_ptr 0: not given): asynchronous; *total lands on the device"""
        self._ck(self.L.dspi_meters_alarms(self.h, meters_ptr or None, level_q15, streams_ptr, info_ptr or None, cap, total_ptr, MEM_DEVICE), "meters_alarms")

    def status_all(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """dspi_status_all into host memory: uint8 [count][2 C + 4], row i what status(first + i) answers"""
        count = self.n_streams - first if count is None else count
        buf = np.zeros((count, self.C * 2 + 4), dtype=np.uint8)
        self._ck(self.L.dspi_status_all(self.h, first, count, buf.ctypes.data, buf.nbytes, 0), "status_all")
        return buf

    def status_all_device(self, buf_ptr: int, cap: int, first: int = 0, count: int | None = None) -> int:
        """dspi_status_all into device memory (cap bytes at buf_ptr): asynchronous"""
        count = self.n_streams - first if count is None else count
        return self._ck(self.L.dspi_status_all(self.h, first, count, buf_ptr, cap, MEM_DEVICE), "status_all")

    def clear_clips_list(self, streams) -> int:
        """dspi_clear_clips_list: REQ_CLEAR_CLIPS for the listed streams (any order, duplicates allowed), one launch on the context's stream"""
        s = np.ascontiguousarray(np.asarray(streams, dtype=np.uint32).reshape(-1))
        return self._ck(self.L.dspi_clear_clips_list(self.h, s.ctypes.data if len(s) else None, len(s)), "clear_clips_list")

    def sync(self):
        self._ck(self.L.dspi_sync(self.h), "sync")

    def hip_stream(self) -> int:
        return self.L.dspi_hip_stream(self.h) or 0
