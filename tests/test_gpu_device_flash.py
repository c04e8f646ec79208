"""A stream's own flash on the GPU (dspi_device_flash, include/dspi.h): streams of a running device context issue the preset directory
requests between calls while their neighbours play on, and every requesting stream and its two neighbours are held to THEIR OWN firmware
build (oracle/_ref/libref_fw_*: the reference's request handlers, main loop and flash_storage.c compiled in place, one private library
per device) — pairs, sub, peaks, clip flags and status bytes from the first frame after each request, which is where the mute a request
leaves shows: max(10 ms, 512) samples after a sector write (960 at 96 kHz), 256 after the delete of the active slot, the 120 ms pre-mute
after a setter the firmware ignores, none after a load that fails its CRC.  Then a reboot from the stream's own flash (exact from frame
0), a swap inside the context, a migration into a second context and a grown context.  No compared stream is left out: the Q28 preset
has no leveller (an x86 build of the reference cannot hold the limiter's cast, profiles/ref_leg.md) and the input is -6 dBFS noise.

    figures: none (no new kernel, no timing claim).  One row plus two streams (130 float, 66 Q28), 48-frame packets, 30 packets after
    each request, seven calls per case."""
import struct

import numpy as np
import pytest

import orclib
from conftest import has_gpu
from orclib import Oracle
from dspi_amd import wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

B, P, VOL = 48, 30, -12 * 256
R_ = W.REQ
SAVE_PARAMS, LOAD_PARAMS = 0x51, 0x52
CASES = [(W.F32_FMA, 48000), (1, 48000), (0, 48000), (W.F32_FMA, 96000)]
_pcm = {}


def case_id(c):
    flavor, fs = c
    return ("q28" if int(flavor) == 0 else "f32_fma" if getattr(flavor, "fma", False) else "f32") + f"_{fs // 1000}k"


def pcm_for(S, fs, packets):
    """-6 dBFS noise, one row per slot; computed once per shape and left unchanged"""
    key = (S, fs, packets)
    if key not in _pcm: _pcm[key] = WL.synth_pcm16(S, packets * B, fs, mix=False)
    return _pcm[key]


def preset(flavor):
    blob = WL.full_chain_blob(int(flavor))
    if int(flavor) == 0: blob["leveller"]["enabled"] = 0
    return blob


def firmware(flavor, fs, flash=None, blob=None):
    fw = Oracle(int(flavor), ref="fw", fma=bool(getattr(flavor, "fma", False)), flash=flash)
    assert fw.set_rate(fs) == 0
    fw.set_volume(VOL)
    if blob is not None: assert fw.load_bulk(blob) == 0
    return fw


class Rig:
    """a device context and one firmware build per compared slot; run() plays P packets on all of them and compares"""

    def __init__(self, flavor, fs, S, compared, rows, blob=None):
        self.flavor, self.fs = flavor, fs
        self.d = Dspi(flavor, S, device=0)
        assert self.d.device_flash(1) == 1
        assert self.d.set_rate(fs) == 0
        self.d.set_volume(VOL)
        if blob is not None: assert self.d.load_bulk(blob) == 0
        self.fw = {s: firmware(flavor, fs, blob=blob) for s in compared}
        self.pcm, self.pos = rows, 0

    def both(self, s, kind, req, wvalue=0, payload=b""):
        """one request to slot s and to its firmware: the same answer"""
        if kind == "get":
            a, b = self.fw[s].vendor_get(req, wvalue), self.d.vendor_get(req, wvalue, stream=s)
        else:
            a, b = self.fw[s].vendor_set(req, wvalue, payload) == 0, self.d.vendor_set(req, wvalue, payload, stream=s) == 0
        assert a == b, (s, kind, hex(req), wvalue, a, b)
        return a

    def run(self, what):
        d, n = self.d, self.d.n_streams
        x = np.ascontiguousarray(self.pcm[:n, self.pos * B:(self.pos + P) * B])
        pairs, sub, peaks = d.process_host(x, P, B, clip=True)
        for s, fw in self.fw.items():
            rp, rs, rk, rc = fw.process(x[s], P, B)
            for name, got, ref in (("pairs", pairs[s], rp), ("sub", sub[s], rs), ("peaks", peaks[s], rk)):
                assert np.array_equal(got, ref), f"{what}: stream {s} {name} differ from its firmware build, first at {np.argwhere(got != ref)[:3].tolist()}"
            assert int(d.last_clip[s]) == rc, f"{what}: stream {s} clip flags {int(d.last_clip[s]):#x} / {rc:#x}"
            assert d.status(s) == fw.status(), f"{what}: stream {s} status bytes"
            assert d.flash_read(s) == fw.read_flash(), f"{what}: stream {s} flash"
        self.pos += P

    def close(self):
        for fw in self.fw.values(): fw.close()
        self.d.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_requests_reboot_and_travel(case):
    flavor, fs = case
    fma = bool(getattr(flavor, "fma", False))
    if not orclib.ref_available(int(flavor), "fw", fma): pytest.skip("needs the firmware build under oracle/_ref")
    R = 128 if int(flavor) else 64
    S = R + 2
    q0, q1, q2, q3 = 3, R // 2, R - 1, R + 1                      # the requesting streams: three in the full row (its last slot among them), one in the second
    compared = sorted({s + k for s in (q0, q1, q2, q3) for k in (-1, 0, 1) if 0 <= s + k < S})
    blob = preset(flavor)
    x = Rig(flavor, fs, S, compared, pcm_for(S + 1, fs, 7 * P), blob)
    d = x.d
    assert d.tile_streams() == R
    ssz = len(d.save_slot(0))
    x.run("power-on")                                             # the first boot's directory write and the bulk load: both mutes
    hold = max((fs * 10 + 999) // 1000, 512)
    assert hold == (960 if fs == 96000 else 512)

    # ---- saves: a slot, a name, the legacy save, a slot on the second row ----
    x.both(q0, "set", R_["SET_PREAMP"], 0, struct.pack("<f", -9.0))
    assert x.both(q0, "get", R_["PRESET_SAVE"], 2) == b"\x00"
    x.both(q1, "set", R_["PRESET_SET_NAME"], 5, b"Night")
    assert x.both(q2, "get", SAVE_PARAMS) == b"\x00"
    assert x.both(q3, "get", R_["PRESET_SAVE"], 4) == b"\x00"
    assert d.vendor_get(R_["PRESET_GET_DIR"], 0, stream=q0) == bytes([4, 0, 0, 0, 2, 1, 0]) and d.vendor_get(R_["PRESET_GET_DIR"], 0, stream=q0 + 1) == bytes([0, 0, 0, 0, 0, 1, 0])
    x.run("after the saves")

    # ---- loads: occupied, empty, corrupt, the legacy load ----
    x.both(q0, "set", R_["SET_PREAMP"], 0, struct.pack("<f", 0.0))
    assert x.both(q0, "get", R_["PRESET_LOAD"], 2) == b"\x00"
    assert d.vendor_get(R_["GET_PREAMP"], 0, stream=q0) == struct.pack("<f", -9.0)
    assert x.both(q1, "get", R_["PRESET_LOAD"], 7) == b"\x00"       # empty: factory defaults
    dump = bytearray(d.flash_read(q2)); bad = bytearray(dump[4096:4096 + ssz]); bad[100] ^= 0x40; dump[4096 + 100] ^= 0x40
    assert x.fw[q2].load_slot(bytes(bad), 0) == 3                 # (the firmware build: the image into sector 1, then REQ_PRESET_LOAD 0 -> PRESET_ERR_CRC)
    assert d.flash_write(q2, 1, bytes(dump)) == 1 and d.vendor_get(R_["PRESET_LOAD"], 0, stream=q2) == b"\x00"
    assert d.collect_bulk(q2) == x.fw[q2].collect_bulk(), "a load that fails its CRC changes nothing"
    x.both(q3, "set", R_["SET_PREAMP"], 0, struct.pack("<f", -4.0))
    assert x.both(q3, "get", LOAD_PARAMS) == b"\x00"              # slot 4, the last active one
    assert d.vendor_get(R_["GET_PREAMP"], 0, stream=q3) == struct.pack("<f", -3.0)
    x.run("after the loads")

    # ---- delete of the active slot, an ignored setter, a startup choice ----
    assert x.both(q0, "get", R_["PRESET_DELETE"], 2) == b"\x00"     # active: factory defaults under 256 samples
    x.both(q1, "set", R_["PRESET_SET_STARTUP"], 0, bytes([2, 3]))   # bad mode: ignored, the 120 ms pre-mute stands
    assert x.both(q2, "get", R_["PRESET_DELETE"], 9) == b"\x00"     # neither active nor occupied: the two sector operations' hold
    x.both(q3, "set", R_["PRESET_SET_STARTUP"], 0, bytes([1, 0]))   # boot with the last active slot (4)
    x.run("after the deletes")

    # ---- the device that was re-plugged: q0 and q3 reboot from their own flash ----
    flashes = {s: d.flash_read(s) for s in (q0, q3)}
    assert d.boot_streams([q3, q0], own_flash=True) == 4          # the first listed stream's selection
    for s in (q0, q3):
        x.fw[s].close()
        x.fw[s] = firmware(flavor, fs, flash=flashes[s])
        assert d.set_rate(fs, stream=s) == 0
        d.set_volume(VOL, stream=s)
        assert d.collect_bulk(s) == x.fw[s].collect_bulk(), s
    assert d.vendor_get(R_["GET_PREAMP"], 0, stream=q3) == struct.pack("<f", -3.0) and d.vendor_get(R_["PRESET_GET_ACTIVE"], 0, stream=q3) == b"\x04"
    x.run("rebooted from the own flash, from frame 0")

    # ---- travel: a swap inside the context, a migration into a second context, a slot grown beside the last stream ----
    f0, f2 = d.flash_read(q0), d.flash_read(q2)
    assert f0 != f2 and d.move_streams([(q0, q2), (q2, q0)]) == 2
    assert d.flash_read(q2) == f0 and d.flash_read(q0) == f2
    x.fw[q0], x.fw[q2] = x.fw[q2], x.fw[q0]
    e = Rig(flavor, fs, 3, [], pcm_for(3, fs, 2 * P))
    off = Dspi(flavor, 2, device=0)                               # a destination without the mode is refused before either context is written
    off.pause_streams(1, 1)
    with pytest.raises(DspiError): d.migrate_streams(off, [(q0, 1)])
    off.close()
    e.d.pause_streams(1, 1)
    assert d.migrate_streams(e.d, [(q0, 1)]) == 1
    assert e.d.flash_read(1) == f2 and d.flash_read(q0) == f2     # by value: the source slot stays behind, frozen, with its own
    e.fw[1] = x.fw.pop(q0)
    fq3 = d.flash_read(q3)
    assert d.resize_streams(S + 1) == S + 1
    assert d.set_rate(fs, stream=S) == 0
    d.set_volume(VOL, stream=S)
    x.fw[S] = firmware(flavor, fs)
    assert d.flash_read(q3) == fq3 and d.flash_read(S) == x.fw[S].read_flash()
    x.run("after the swap, the migration and the grow")
    e.run("the migrated stream in its new context")
    e.close(); x.close()
