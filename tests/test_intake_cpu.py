"""16- and 24-bit devices in one call, without a GPU: the input layout of dspi_process_mixed (dspi_amd/csrc/dspi_intake.{h,cpp}) through a g++
driver (tests/intake_driver.cpp) against naive Python, the two identities that make widening exact — stated in numpy float32 / int32, for
every 16-bit sample —, and the two calls of include/dspi.h on host-only contexts: the sizes, and every refusal in its order."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from dspi_amd import host, wire as W
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
FRAMES = (1, 45, 135, 960)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver has its own main: it is built with AddressSanitizer and UBSan where this g++ has their runtimes — asked of an empty program,
    so that a sanitized build of the driver that fails for any other reason fails here —, else plain; which build ran is printed (pytest -s, or
    with the failure's captured output)"""
    tmp = tmp_path_factory.mktemp("intake")
    exe = tmp / "intake_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "intake_driver.cpp"),
           os.path.join(CSRC, "dspi_intake.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("intake_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def feature():
    """everything here, the identities included, is about a library that has the call"""
    assert hasattr(host.lib(), "dspi_process_mixed"), "libdspi_mi355x has no dspi_process_mixed"


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def depth_vectors():
    r = random.Random(7)
    vecs = [[16], [24], [16, 24], [24, 16] * 150]
    for _ in range(40):
        n = r.randrange(1, 301)
        vecs.append([r.choice((16, 24)) for _ in range(n)])
    return vecs


def naive_offsets(depths, F):
    off = [0]
    for d in depths: off.append(off[-1] + F * (6 if d == 24 else 4))
    return off


# ---- the symbols and the header's words -------------------------------------------------------------------------------------------------------
def test_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_process_mixed") and hasattr(L, "dspi_mixed_pcm_bytes") and hasattr(L, "dspi_debug_intake")
    assert L.dspi_abi_version() == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + mixed input formats: detect by symbol (dspi_process_mixed; with it dspi_mixed_pcm_bytes; additions only)",
                 "int dspi_mixed_pcm_bytes(const dspi_ctx *ctx, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,\n"
                 "                         uint64_t *total_bytes, uint64_t *offsets /* [n_streams + 1] or NULL */);",
                 "int dspi_process_mixed(dspi_ctx *ctx, const void *pcm_in, const uint8_t *bit_depths, uint32_t n_blocks, uint32_t block_len,\n"
                 "                       const dspi_out *out, uint32_t *pdm_words /* NULL: as dspi_process; else as dspi_process_pdm */, uint32_t flags);",
                 "usb_audio.c:601-603 against :680-681", "usb_audio.c:1001-1002 against :1010-1011", "usb_audio.c:244-250", "p >= 2^-103",
                 "offset[s + 1] = offset[s] + F * (bit_depths[s] == 24 ? 6 : 4)"):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()      # the module and the kernel are the library's
    assert "dspi_intake" in mk.split("HOST =")[1].split("\n")[0] and "dspi_intake" in mk.split("KERNELS =")[1].split("\n")[0]


# ---- the layout -------------------------------------------------------------------------------------------------------------------------------
def test_depth_validation(driver):
    cases = [([16, 24, 16], 3, 0), ([16] * 9, 9, 16), ([24] * 4, 4, 24), ([16, 24, 8], 2, 0), ([0], 0, 0), ([24, 32, 16, 17], 1, 0), ([16, 16, 255], 2, 0), ([], 0, 0)]
    got = run(driver, ["check " + " ".join(map(str, d)) for d, _, _ in cases])
    for (d, bad, uni), line in zip(cases, got):
        first, u = map(int, line.split())
        assert first == bad, (d, line)
        if bad == len(d): assert u == uni, (d, line)


def test_offsets_and_total(driver):
    cases = [(d, F) for d in depth_vectors() for F in FRAMES]
    got = run(driver, [f"off {F} " + " ".join(map(str, d)) for d, F in cases])
    for (d, F), line in zip(cases, got):
        v = list(map(int, line.split()))
        want = naive_offsets(d, F)
        assert v[0] == want[-1] and v[1:] == want, (len(d), F)


def test_offsets_overflow(driver):
    """frames as large as the interface allows (2^32 - 1 blocks of 192) still fit; a frame count that cannot be multiplied out is refused"""
    F = (2 ** 32 - 1) * 192
    got = run(driver, [f"off {F} 16 24 24", f"off {2 ** 62} 16 24 24"])
    assert list(map(int, got[0].split())) == [16 * F, 0, 4 * F, 10 * F, 16 * F] and got[1] == "overflow"


@pytest.mark.parametrize("row", [64, 128])
def test_chunk_byte_ranges(driver, row):
    cases = [(d, F, k) for d in depth_vectors()[3::4] for F in FRAMES for k in range(1, 9)]
    got = run(driver, [f"rows {F} {row} {k} " + " ".join(map(str, d)) for d, F, k in cases])
    for (d, F, k), line in zip(cases, got):
        off = naive_offsets(d, F)
        ranges = [tuple(map(int, x.split("-"))) for x in line.split()]
        rows = -(-len(d) // row); per = -(-rows // k)
        assert len(ranges) == -(-rows // per) <= k
        assert ranges[0][0] == 0 and ranges[-1][1] == off[-1], "the chunks cover the whole buffer"
        for i, (b, e) in enumerate(ranges):
            assert b < e and (i == 0 or b == ranges[i - 1][1]), "contiguous and disjoint"
            assert b == off[min(len(d), i * per * row)] and e == off[min(len(d), (i + 1) * per * row)], "a chunk is its rows' streams"


# ---- the widening copy ------------------------------------------------------------------------------------------------------------------------
def widen_model(src, depth):
    """numpy: int16 samples -> the bytes of (s << 8) as 24-bit little endian; a 24-bit run as it is"""
    if depth == 24: return src.copy()
    s = src.view("<i2").astype(np.int32) << 8
    return np.stack([s & 0xff, (s >> 8) & 0xff, (s >> 16) & 0xff], axis=-1).astype(np.uint8).reshape(-1)


def test_widen_cpu(driver):
    r = np.random.default_rng(3)
    cases = []
    for F in (1, 2, 45, 135, 960):
        for depth in (16, 24):
            cases.append((depth, F, r.integers(0, 256, F * (6 if depth == 24 else 4), dtype=np.uint8)))
    extremes = np.array([-32768, 32767, -1, 0, 1, -2, 255, 256, -256, 0x1234], dtype="<i2")
    cases.append((16, 5, extremes.view(np.uint8).copy()))
    got = run(driver, [f"widen {depth} {F} {src.tobytes().hex()}" for depth, F, src in cases])
    for (depth, F, src), line in zip(cases, got):
        assert bytes.fromhex(line) == widen_model(src, depth).tobytes(), (depth, F)
    assert got[-1].startswith("000080" "00ff7f" "00ffff" "000000"), "the extremes: 00 lo hi"
    assert run(driver, ["widen 16 1 0102" "0304"]) == ["000102" "000304"], "00 Llo Lhi 00 Rlo Rhi"


# ---- the preamp predicate -----------------------------------------------------------------------------------------------------------------------
def f32_word(x): return struct.unpack("<I", struct.pack("<f", x))[0]


def test_preamp_predicate(driver):
    limit = np.float32(2.0 ** -103)
    below = np.nextafter(limit, np.float32(0))
    cases = [(0.0, 0), (float(np.float32(2.0 ** -149)), 1), (2.0 ** -104, 1), (float(below), 1), (float(limit), 0), (1.0, 0), (float("inf"), 0)]
    assert f32_word(2.0 ** -149) == 1 and f32_word(float(below)) == f32_word(float(limit)) - 1
    got = run(driver, [f"preamp {f32_word(x)}" for x, _ in cases])
    assert got == [str(w) for _, w in cases], list(zip(cases, got))
    # the requests of tests/test_gpu_mixed_input.py: -640 dB is refused, -600 dB is not
    assert run(driver, [f"preamp {f32_word(float(np.float32(10.0) ** np.float32(db / 20)))}" for db in (-640.0, -600.0)]) == ["1", "0"]


# ---- the two identities (usb_audio.c:601-603 against :680-681, :1001-1002 against :1010-1011) -------------------------------------------------
S16 = np.arange(-32768, 32768, dtype=np.int32)


def float_routes(p):
    """(the 24-bit route on s << 8, the 16-bit route on s) for every 16-bit sample, binary32 throughout, as words"""
    p = np.float32(p)
    g24, g16 = np.float32(2.0 ** -23) * p, np.float32(2.0 ** -15) * p
    a = (S16 << 8).astype(np.float32) * g24
    b = S16.astype(np.float32) * g16
    assert a.dtype == b.dtype == np.float32
    return a.view(np.uint32), b.view(np.uint32)


@pytest.mark.parametrize("p", [2.0 ** -103, float(np.nextafter(np.float32(2.0 ** -103), np.float32(1))), 0.9e-30, 1e-30, 1.1e-30, 3e-20, 0.1, 1.0 / 3, 1.0,
                               1.0000001, 15.848932, 1e30, 3e30], ids=lambda p: f"{p:.8g}")
def test_float_identity_holds_from_2_pow_minus_103(p):
    a, b = float_routes(p)
    assert np.array_equal(a, b), np.argwhere(a != b)[:3]


def test_float_identity_fails_below(p=1e-32):
    """... and not below: the refusal stands where it is needed"""
    a, b = float_routes(p)
    assert np.count_nonzero(a != b) >= 1


def test_q28_identity():
    s16 = S16.astype(np.int32)
    assert np.array_equal(((s16 << 8) << 8) >> 2, s16 << 14) and np.array_equal((s16 << 16) >> 2, s16 << 14)
    assert ((s16 << 16) >> 2).dtype == np.int32


# ---- host-only contexts -----------------------------------------------------------------------------------------------------------------------
def _call(d, pcm, depths, n_blocks, block_len, out, flags=0, words=None):
    return d.L.dspi_process_mixed(d.h, pcm, depths, n_blocks, block_len, out, words, flags)


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_mixed_pcm_bytes_on_a_host_only_context(flavor):
    S = 37
    d = Dspi(flavor, S, device=None)
    r = random.Random(flavor)
    for n_blocks, block_len in ((1, 1), (3, 45), (10, 96), (5, 192)):
        depths = [r.choice((16, 24)) for _ in range(S)]
        total, off = d.mixed_pcm_bytes(depths, n_blocks, block_len)
        want = naive_offsets(depths, n_blocks * block_len)
        assert total == want[-1] and off.tolist() == want
        # either output alone
        dp = np.array(depths, dtype=np.uint8)
        t = C.c_uint64(0)
        assert d.L.dspi_mixed_pcm_bytes(d.h, dp.ctypes.data, n_blocks, block_len, C.byref(t), None) == 0 and t.value == total
        assert d.L.dspi_mixed_pcm_bytes(d.h, dp.ctypes.data, n_blocks, block_len, None, None) == 0
    dp = np.full(S, 16, dtype=np.uint8)
    assert d.L.dspi_mixed_pcm_bytes(None, dp.ctypes.data, 1, 48, None, None) == host.E_INVAL
    assert d.L.dspi_mixed_pcm_bytes(d.h, None, 1, 48, None, None) == host.E_INVAL
    for nb, bl in ((0, 48), (1, 0), (1, 193)): assert d.L.dspi_mixed_pcm_bytes(d.h, dp.ctypes.data, nb, bl, None, None) == host.E_INVAL
    dp[S - 1] = 20
    assert d.L.dspi_mixed_pcm_bytes(d.h, dp.ctypes.data, 1, 48, None, None) == host.E_INVAL and f"stream {S - 1}" in d.L.dspi_last_error(d.h).decode()
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_refusals_in_their_order(flavor):
    """INVAL (pointers, depths, lengths, flag bits), then UNSUPPORTED (float: an active 16-bit stream with a preamp below 2^-103), then NODEVICE"""
    S, F = 12, 48
    d = Dspi(flavor, S, device=None)
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=7) >= 0
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 1, struct.pack("<f", -600.0), stream=3) >= 0      # (small, and above the limit)
    mixed = np.array([16, 24] * (S // 2), dtype=np.uint8)      # stream 7: 24 bit
    bad = mixed.copy(); bad[7] = 16                             # stream 7: 16 bit
    pcm = np.zeros(S * F * 6, dtype=np.uint8)
    out = host._Out(None, None, None, None)
    po, pp = C.byref(out), pcm.ctypes.data
    refused = host.E_UNSUPPORTED if flavor else host.E_NODEVICE
    # the pointers
    assert d.L.dspi_process_mixed(None, pp, bad.ctypes.data, 1, F, po, None, 0) == host.E_INVAL
    assert _call(d, None, bad.ctypes.data, 1, F, po) == host.E_INVAL
    assert _call(d, pp, None, 1, F, po) == host.E_INVAL
    assert _call(d, pp, bad.ctypes.data, 1, F, None) == host.E_INVAL
    # a depth: before the lengths' refusal says anything else, and before the preamp's
    worse = bad.copy(); worse[9] = 8
    assert _call(d, pp, worse.ctypes.data, 1, F, po) == host.E_INVAL and "stream 9" in d.L.dspi_last_error(d.h).decode()
    # lengths and flag bits: before the preamp's refusal
    for nb, bl, flags in ((0, F, 0), (1, 0, 0), (1, 193, 0), (1, F, 0x40), (1, F, 0x80000000), (1, F, host.OUT_SPDIF | host.OUT_TILED)):
        assert _call(d, pp, bad.ctypes.data, nb, bl, po, flags) == host.E_INVAL, (nb, bl, flags)
    # uniform depths with a bad flag bit: dspi_process's own refusal
    u16 = np.full(S, 16, dtype=np.uint8)
    assert _call(d, pp, u16.ctypes.data, 1, F, po, 0x40) == host.E_INVAL
    # the preamp: float contexts, active 16-bit streams only, and the message names the stream
    assert _call(d, pp, bad.ctypes.data, 1, F, po) == refused
    if flavor: assert "stream 7" in d.L.dspi_last_error(d.h).decode()
    assert _call(d, pp, bad.ctypes.data, 1, F, po, host.MEM_DEVICE) == refused
    # ... never for a 24-bit stream, a paused stream, or uniform depths (that call is dspi_process): the host-only context's refusal is what is left
    assert _call(d, pp, mixed.ctypes.data, 1, F, po) == host.E_NODEVICE
    assert _call(d, pp, u16.ctypes.data, 1, F, po) == host.E_NODEVICE
    assert _call(d, pp, np.full(S, 24, dtype=np.uint8).ctypes.data, 1, F, po) == host.E_NODEVICE
    d.pause_streams(7, 1)
    assert _call(d, pp, bad.ctypes.data, 1, F, po) == host.E_NODEVICE
    d.resume_streams(7, 1)
    assert _call(d, pp, bad.ctypes.data, 1, F, po) == refused
    # channel 1 counts as channel 0 does
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", 0.0), stream=7) >= 0
    assert _call(d, pp, bad.ctypes.data, 1, F, po) == host.E_NODEVICE
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 1, struct.pack("<f", -640.0), stream=7) >= 0
    assert _call(d, pp, bad.ctypes.data, 1, F, po) == refused
    # with pdm_words the same
    words = np.zeros(8, dtype=np.uint32)
    assert _call(d, pp, bad.ctypes.data, 1, F, po, 0, words.ctypes.data) == refused
    assert _call(d, pp, mixed.ctypes.data, 1, F, po, 0, words.ctypes.data) == host.E_NODEVICE
    with pytest.raises(DspiError) as e: d.process_mixed_host(pcm[:int(np.where(mixed == 24, 6, 4).sum()) * F], mixed, 1, F)
    assert e.value.code == host.E_NODEVICE
    # the widening pass alone (dspi_debug_intake): the same argument checks, no preamp rule, no host-only context
    assert d.L.dspi_debug_intake(d.h, None, bad.ctypes.data, 1, F) == host.E_INVAL and d.L.dspi_debug_intake(d.h, pp, None, 1, F) == host.E_INVAL
    assert d.L.dspi_debug_intake(d.h, pp, worse.ctypes.data, 1, F) == host.E_INVAL and d.L.dspi_debug_intake(d.h, pp, bad.ctypes.data, 1, 193) == host.E_INVAL
    assert d.L.dspi_debug_intake(d.h, pp, bad.ctypes.data, 1, F) == host.E_NODEVICE
    d.close()
