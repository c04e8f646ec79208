"""A stream's own flash: request scripts that run alike on a firmware build (oracle/_ref/libref_fw_*, orclib.Oracle(ref="fw")) and on one
stream of a library context with dspi_device_flash on.  TEST INFRASTRUCTURE ONLY: tests/test_device_flash_cpu.py runs them on both and
compares after every step; tools/gen_flash_fixture.py records the scripted sequence from the firmware build into tests/golden/ for
machines without it.

A step is a list: ["get", req, wValue] | ["set", req, wValue, payload hex] | ["rate", hz] | ["volume", v] | ["bulk", blob hex] |
["bad", slot] (an occupied slot's sector gets one flipped byte behind the directory's back, then REQ_PRESET_LOAD of it: a load that fails its
CRC; nothing happens where the slot is not occupied)."""
import struct

import numpy as np

from dspi_amd import wire as W

R = W.REQ
SAVE_PARAMS, LOAD_PARAMS, FACTORY_RESET = 0x51, 0x52, 0x53
# IN requests that change the device: never sent as a probe
MUTATING = (0x50, SAVE_PARAMS, LOAD_PARAMS, FACTORY_RESET, 0x83, R["PRESET_SAVE"], R["PRESET_LOAD"], R["PRESET_DELETE"], 0xC0, R["SAVE_MASTER_VOLUME"])
# outside the library's DSP subset with and without the mode (pins, serial number, buffer statistics, I2S clock pins)
NOT_SERVED = (0x7C, 0x7D, 0x7E, 0xA0, 0xB0, 0xB1, 0xB2, 0xB3, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9)
PROBES = [(req, wv) for req in range(0x40, 0xE0) if req not in MUTATING and req not in NOT_SERVED for wv in (0, 2, 10)]


def occupied(dev, slot):
    """(a corrupted sector is a case only where the directory says the slot holds a preset)"""
    d = dev.get(R["PRESET_GET_DIR"], 0)
    return bool((d[0] | d[1] << 8) >> slot & 1)


class FwDev:
    """the firmware build as a script target"""

    def __init__(self, fw): self.o = fw
    def get(self, req, wv): return self.o.vendor_get(req, wv, 64)
    def set(self, req, wv, payload): return self.o.vendor_set(req, wv, payload) == 0
    def rate(self, hz): return self.o.set_rate(hz)
    def volume(self, v): self.o.set_volume(v)
    def bulk(self, blob): return self.o.load_bulk(blob)
    def flash(self): return self.o.read_flash()
    def collect(self): return self.o.collect_bulk()
    def slot(self, k): return self.o.save_slot(k)

    def bad(self, slot):
        if not occupied(self, slot): return
        n = len(self.o.save_slot(0))
        img = bytearray(self.o.read_flash()[4096 * (1 + slot):4096 * (1 + slot) + n]); img[100] ^= 0x40
        self.o.load_slot(bytes(img), slot)      # the image into the sector, the occupied bit into the cached directory, REQ_PRESET_LOAD


class LibDev:
    """one stream of a library context (dspi_device_flash on)"""

    def __init__(self, d, stream): self.d, self.s = d, stream
    def get(self, req, wv): return self.d.vendor_get(req, wv, 64, stream=self.s)
    def set(self, req, wv, payload): return self.d.vendor_set(req, wv, payload, stream=self.s) == 0
    def rate(self, hz): return self.d.set_rate(hz, stream=self.s)
    def volume(self, v): self.d.set_volume(v, stream=self.s)
    def bulk(self, blob): return self.d.load_bulk(blob, stream=self.s)
    def flash(self): return self.d.flash_read(self.s)
    def collect(self): return self.d.collect_bulk(self.s)
    def slot(self, k): return self.d.save_slot(k, self.s)

    def bad(self, slot):
        if not occupied(self, slot): return
        dump = bytearray(self.d.flash_read(self.s)); dump[4096 * (1 + slot) + 100] ^= 0x40
        self.d.flash_write(self.s, 1, bytes(dump))
        self.d.vendor_get(R["PRESET_LOAD"], slot, 64, stream=self.s)


def apply(dev, step):
    """the step's answer: bytes / None (a stall) for get, True / False for set, the return code for rate and bulk"""
    kind = step[0]
    if kind == "get": return dev.get(step[1], step[2])
    if kind == "set": return dev.set(step[1], step[2], bytes.fromhex(step[3]))
    if kind == "rate": return dev.rate(step[1])
    if kind == "volume": return dev.volume(step[1])
    if kind == "bulk": return dev.bulk(bytes.fromhex(step[1]))
    if kind == "bad": return dev.bad(step[1])
    raise ValueError(kind)


def observe(dev):
    """everything a host can read back: every GET request the library serves, the parameter blob, a collected slot image, the flash"""
    return dict(gets=[dev.get(req, wv) for req, wv in PROBES], bulk=dev.collect(), slot=dev.slot(5), flash=dev.flash())


def f32(v): return struct.pack("<f", v).hex()


def scripted(flavor):
    """every directory request, out-of-range slots and short payloads included, with parameter changes in between so that slots differ"""
    from test_gpu_fuzz import random_blob
    blob = random_blob(np.random.default_rng(77 + flavor), flavor, 48000).tobytes().hex()
    get, st = (lambda req, wv=0: ["get", req, wv]), (lambda req, wv, payload: ["set", req, wv, payload.hex() if isinstance(payload, bytes) else payload])
    return [
        get(R["PRESET_GET_DIR"]), get(R["PRESET_SAVE"], 10), get(R["PRESET_SAVE"], 255), get(R["PRESET_SAVE"], 3), get(R["PRESET_GET_DIR"]),
        ["rate", 48000], ["volume", -9 * 256], st(R["SET_PREAMP"], 0, f32(-6.0)), ["bulk", blob], get(R["PRESET_SAVE"], 0), get(R["PRESET_SAVE"], 9),
        st(R["PRESET_SET_NAME"], 3, b"Evening"), st(R["PRESET_SET_NAME"], 9, b"A" * 40), st(R["PRESET_SET_NAME"], 0, b"ab\x00cd"), st(R["PRESET_SET_NAME"], 10, b"x"),
        st(R["PRESET_SET_NAME"], 4, b""), st(R["PRESET_SET_NAME"], 0x0103, b"wValue high byte"), get(R["PRESET_GET_NAME"], 3), get(R["PRESET_GET_NAME"], 10),
        st(R["PRESET_SET_STARTUP"], 0, bytes([1, 3])), st(R["PRESET_SET_STARTUP"], 0, bytes([2, 3])), st(R["PRESET_SET_STARTUP"], 0, bytes([0, 10])),
        st(R["PRESET_SET_STARTUP"], 0, bytes([1])), st(R["PRESET_SET_STARTUP"], 0, bytes([0, 9, 7])), get(R["PRESET_GET_STARTUP"]),
        st(R["PRESET_SET_INCLUDE_PINS"], 0, b"\x00"), ["bulk", blob], st(R["PRESET_SET_INCLUDE_PINS"], 0, b"\x07"), get(R["PRESET_GET_INCLUDE_PINS"]),
        st(R["SET_MASTER_VOLUME_MODE"], 0, b"\x01"), st(R["SET_MASTER_VOLUME"], 0, f32(-31.5)), get(R["SAVE_MASTER_VOLUME"]), get(R["PRESET_SAVE"], 1),
        st(R["SET_MASTER_VOLUME_MODE"], 0, b"\x05"), st(R["SET_MASTER_VOLUME"], 0, f32(-3.0)), get(R["PRESET_LOAD"], 1), get(R["PRESET_LOAD"], 10),
        st(R["SET_MASTER_VOLUME_MODE"], 0, b"\x01"), get(R["PRESET_LOAD"], 1), get(R["PRESET_LOAD"], 3), get(R["PRESET_LOAD"], 6), get(R["PRESET_GET_ACTIVE"]),
        ["get", 0xC0, 0x0100], get(SAVE_PARAMS), ["rate", 96000], get(FACTORY_RESET), get(LOAD_PARAMS), ["get", 0xC0, 0x0001], get(R["PRESET_LOAD"], 9),
        ["bad", 9], get(LOAD_PARAMS), get(R["PRESET_DELETE"], 3), get(R["PRESET_DELETE"], 9), get(R["PRESET_DELETE"], 12), get(R["PRESET_DELETE"], 5), ["rate", 44100],
        get(R["PRESET_SAVE"], 2), get(R["PRESET_DELETE"], 2), get(SAVE_PARAMS), get(R["PRESET_GET_DIR"]),
    ]


def random_script(rng, flavor, steps=30):
    """directory requests, parameter requests, bulk loads and rate changes interleaved"""
    from test_gpu_fuzz import random_blob
    N = 9 if flavor else 5
    fs, out = 48000, []
    slot = lambda: int(rng.choice([0, 1, 2, 3, 9, 10, 200], p=[0.25, 0.2, 0.15, 0.15, 0.15, 0.05, 0.05]))
    for _ in range(steps):
        k = rng.integers(0, 20)
        if k < 3: out.append(["get", R["PRESET_SAVE"], slot()])
        elif k < 6: out.append(["get", R["PRESET_LOAD"], slot()])
        elif k == 6: out.append(["get", R["PRESET_DELETE"], slot()])
        elif k == 7: out.append(["set", R["PRESET_SET_NAME"], slot(), bytes(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8)).hex()])
        elif k == 8: out.append(["set", R["PRESET_SET_STARTUP"], 0, bytes([int(rng.integers(0, 3)), slot()][:int(rng.integers(1, 3))]).hex()])
        elif k == 9: out.append(["set", R["PRESET_SET_INCLUDE_PINS"], 0, bytes([int(rng.integers(0, 3))]).hex()])
        elif k == 10: out.append(["set", R["SET_MASTER_VOLUME_MODE"], 0, bytes([int(rng.integers(0, 3))]).hex()])
        elif k == 11: out.append(["get", R["SAVE_MASTER_VOLUME"], 0])
        elif k == 12: out.append(["get", int(rng.choice([SAVE_PARAMS, LOAD_PARAMS, FACTORY_RESET])), 0])
        elif k == 13: out.append(["bad", int(rng.integers(0, 4))])
        elif k == 14:
            fs = int(rng.choice([44100, 48000, 96000])); out.append(["rate", fs])
        elif k == 15: out.append(["bulk", random_blob(rng, flavor, fs).tobytes().hex()])
        elif k == 16: out.append(["get", 0xC0, (int(rng.integers(0, 2)) << 8) | int(rng.integers(0, 3))])      # REQ_SET_OUTPUT_TYPE: loads and deletes then switch types
        elif k == 17: out.append(["set", R["SET_OUTPUT_ENABLE"], int(rng.integers(0, N)), bytes([int(rng.integers(0, 2))]).hex()])
        elif k == 18: out.append(["set", R["SET_MASTER_VOLUME"], 0, f32(float(rng.uniform(-60, 0)))])
        else: out.append(["set", R["SET_PREAMP"], 0, f32(float(rng.uniform(-12, 6)))])
    return out
