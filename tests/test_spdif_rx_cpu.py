"""S/PDIF input without a GPU: the CPU receiver and the layout of dspi_process_sources (dspi_amd/csrc/dspi_spdifrx.{h,cpp}) through a g++ driver
(tests/spdifrx_driver.cpp) against the sequential model (tests/spdifrx_model.py) — in one call and split at every frame, and once more
through the kernel's own chunk arithmetic (rx_walk) on the host —, the model against the encoder it reads back, and the calls of
include/dspi.h on host-only contexts: sizes, and every refusal in its order."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import spdifrx_model as M
from dspi_amd import host, wire as W
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
N = 400


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """own main: built with AddressSanitizer and UBSan where this g++ has their runtimes (asked of an empty program), else plain; which build
    ran is printed"""
    tmp = tmp_path_factory.mktemp("spdifrx")
    exe = tmp / "spdifrx_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "spdifrx_driver.cpp"),
           os.path.join(CSRC, "dspi_spdifrx.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("spdifrx_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_process_sources"), "libdspi_mi355x has no dspi_process_sources"


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def corrupted_line(seed=11):
    """400 frames from block position 100 at 48 kHz with every kind of trouble: V (with and without its parity), flipped data cells, cleared
    clock cells, bad preambles on either side, a misplaced Z, an X where Z belongs, zero frames"""
    rng = np.random.default_rng(seed)
    w = M.encode(M.random_pairs(rng, N), 100, 48000)
    M.set_v(w, 0, 0); M.set_v(w, 5, 1, keep_parity=False)
    for f in range(62, 67): M.set_v(w, f, 0)
    for f in range(126, 131): M.set_v(w, f, 1)
    M.flip_data_cell(w, 20, 0, 9); M.flip_data_cell(w, 21, 1, 27); M.flip_data_cell(w, 150, 0, 30)      # (the last: a C bit, and a parity error)
    M.clear_clock_cell(w, 40, 0, 12); M.clear_clock_cell(w, 200, 1, 31)
    M.set_preamble(w, 110, 0, M.Z)                 # a misplaced Z: re-lock
    M.set_preamble(w, 284, 0, M.X)                 # X at position 0 (92 + 192): loss
    M.set_preamble(w, 300, 1, M.X); M.set_preamble(w, 301, 0, M.Y); M.set_preamble(w, 302, 0, 0x00)
    w[320:323] = 0
    M.set_preamble(w, 350, 0, M.Z); M.set_preamble(w, 351, 0, M.Z)      # Z twice: lock, then the second is a re-lock too
    return w


def parse(line, n):
    rec, pairs, packed = line.split()
    return np.frombuffer(bytes.fromhex(rec), dtype=M.RX)[0], np.frombuffer(bytes.fromhex(pairs), dtype="<i4").reshape(n, 2), np.frombuffer(bytes.fromhex(packed), dtype=np.uint8)


def test_symbols_and_header():
    L = host.lib()
    for name in ("dspi_process_sources", "dspi_spdif_decode", "dspi_sources_bytes", "dspi_debug_sources_intake"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    assert host.SPDIF_RX == M.RX and host.SPDIF_RX.itemsize == 40
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + S/PDIF input: detect by symbol (dspi_process_sources;", "#define DSPI_OUT_WIRE 0x40u", "#define DSPI_SRC_SPDIF 1", "#define DSPI_SRC_PCM16 16",
                 "#define DSPI_SRC_PCM24 24", "} dspi_spdif_rx;", "(l & 0x55555500) == 0x55555500"):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()
    assert "dspi_spdifrx" in mk.split("HOST =")[1].split("\n")[0] and "dspi_spdifrx" in mk.split("KERNELS =")[1].split("\n")[0]


# ---- the model against the encoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,byte3", [(44100, 0x00), (48000, 0x02), (96000, 0x0A)])
def test_model_reads_back_the_encoder(fs, byte3):
    """what the issue states of the reference's encoder: samples round-trip, clocks, parity, preambles, channel status 04 00 00 xx 0B"""
    rng = np.random.default_rng(fs)
    pairs = M.random_pairs(rng, 500)
    w = M.encode(pairs, 100, fs)
    rx = M.new_rx()
    got = M.receive(rx, w)
    assert np.array_equal(got[92:], pairs[92:]) and np.array_equal(got[:92], pairs[:92]), "samples pass whether locked or not"
    assert rx["state"] == 2 and rx["sync"] == 1 + (100 + 500) % 192 and rx["sample_rate"] == fs
    assert rx["c_bits"] == [0x04, 0x00, 0x00, byte3, 0x0B] and rx["parity_err_count"] == rx["held"] == rx["coding_errors"] == 0
    for f in range(500):
        assert int(w[f, 0]) & 0xff == (M.Z if (100 + f) % 192 == 0 else M.X) and int(w[f, 2]) & 0xff == M.Y


# ---- the CPU receiver against the model ------------------------------------------------------------------------------------------------------
def model_run(w, split, rx0=None):
    rx = dict(rx0 or M.new_rx(), c_bits=list((rx0 or M.new_rx())["c_bits"]), hold=list((rx0 or M.new_rx())["hold"]))
    split = min(split, len(w)) if split else len(w)
    out = np.concatenate([M.receive(rx, w[:split]), M.receive(rx, w[split:])]) if split < len(w) else M.receive(rx, w)
    return rx, out


@pytest.mark.parametrize("cmd", ["line", "walk"])
def test_receiver_equals_the_model_in_one_call_and_split_at_every_frame(driver, cmd):
    w = corrupted_line()
    zero = M.to_record(M.new_rx()).tobytes().hex()
    got = run(driver, [f"{cmd} {k} {zero} {w.tobytes().hex()}" for k in range(N)])      # k = 0: one call
    for k, line in enumerate(got):
        rx, want = model_run(w, k)
        rec, pairs, packed = parse(line, N)
        assert np.array_equal(pairs, want), (cmd, k, np.argwhere(pairs != want)[:3])
        assert rec.tobytes() == M.to_record(rx).tobytes(), (cmd, k, rec, M.to_record(rx))
        assert np.array_equal(packed, M.pack24(want)), (cmd, k)
    # the line does what it was built for (one call)
    rx, want = model_run(w, 0)
    # (11 malformed subframes: 40 L, 200 R, 300 R, 301 L, 302 L, 320..322 both; 12 V subframes more are held; the Z at 351 re-locks 67 positions
    #  off the block, so byte 3 is read from the block's zero bits 91..98: "44100"; no parity error behind that lock)
    assert rx["coding_errors"] == 11 and rx["held"] == 23 and rx["state"] == 2 and rx["sample_rate"] == 44100 and rx["parity_err_count"] == 0 and rx["sync"] == 1 + 49


@pytest.mark.parametrize("cmd", ["line", "walk"])
def test_receiver_on_random_trouble_and_any_record(driver, cmd):
    """random corruptions at a rate that makes events common, from records in every state (sync 0..192, counters near their wrap)"""
    r = random.Random(5)
    script, cases = [], []
    for i in range(60):
        rng = np.random.default_rng(i)
        n = r.choice((1, 63, 64, 65, 135, 240, 333))
        w = M.encode(M.random_pairs(rng, n), r.randrange(192), r.choice((44100, 48000, 96000)))
        for _ in range(r.randrange(0, 12)):
            f, side, kind = r.randrange(n), r.randrange(2), r.randrange(6)
            if kind == 0: M.set_v(w, f, side, keep_parity=r.random() < 0.7)
            elif kind == 1: M.flip_data_cell(w, f, side, r.randrange(4, 32))
            elif kind == 2: M.clear_clock_cell(w, f, side, r.randrange(4, 32))
            elif kind == 3: M.set_preamble(w, f, side, r.choice((M.Z, M.X, M.Y, 0)))
            elif kind == 4: w[f] = 0
            else: M.set_preamble(w, f, 0, M.Z)
        rx0 = M.new_rx()
        if i % 3:
            rx0.update(sync=r.randrange(193), sample_rate=r.choice((0, 48000, 12345)), parity_err_count=r.choice((0, 7, 0xffffffff)), held=r.choice((0, 0xfffffffe)),
                       coding_errors=r.choice((3, 0xffffffff)), hold=[r.randrange(-(1 << 23), 1 << 23), r.randrange(-(1 << 23), 1 << 23)], c_bits=[r.randrange(256) for _ in range(5)])
        split = r.randrange(n + 1)
        cases.append((w, split, rx0, n))
        script.append(f"{cmd} {split} {M.to_record(rx0).tobytes().hex()} {w.tobytes().hex()}")
    for (w, split, rx0, n), line in zip(cases, run(driver, script)):
        rx, want = model_run(w, split, rx0)
        rec, pairs, packed = parse(line, n)
        assert np.array_equal(pairs, want) and rec.tobytes() == M.to_record(rx).tobytes() and np.array_equal(packed, M.pack24(want)), (cmd, n, split, rec, M.to_record(rx))


def test_padding_bytes_of_the_record_are_kept(driver):
    w = M.encode(M.random_pairs(np.random.default_rng(1), 70), 0, 48000)
    rec = M.to_record(M.new_rx()); rec["pad_"] = (0xAA, 0xBB, 0xCC)
    for cmd in ("line", "walk"):
        got, _, _ = parse(run(driver, [f"{cmd} 0 {rec.tobytes().hex()} {w.tobytes().hex()}"])[0], 70)
        assert got["pad_"].tolist() == [0xAA, 0xBB, 0xCC] and got["c_bits"].tolist() == [0x04, 0, 0, 0x02, 0x0B]


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------------
def naive_offsets(src, F):
    off, at = [], 0
    for s in src:
        if s == 1: at = -(-at // 16) * 16
        off.append(at)
        at += F * {16: 4, 24: 6, 1: 16}[s]
    return off + [at]


def source_vectors():
    r = random.Random(9)
    vecs = [[1], [16], [24], [16, 1], [24, 1, 1], [16, 24, 1] * 50, [1] * 7]
    for _ in range(30): vecs.append([r.choice((16, 24, 1)) for _ in range(r.randrange(1, 200))])
    return vecs


def test_offsets_and_the_16_byte_rule(driver):
    cases = [(d, F) for d in source_vectors() for F in (1, 45, 135, 240)]
    got = run(driver, [f"off {F} " + " ".join(map(str, d)) for d, F in cases])
    padded = 0
    for (d, F), line in zip(cases, got):
        v = list(map(int, line.split()))
        want = naive_offsets(d, F)
        assert v[0] == want[-1] and v[1:] == want, (d[:8], F)
        for s, src in enumerate(d):
            if src == 1: assert v[1 + s] % 16 == 0
        padded += want[-1] != F * sum({16: 4, 24: 6, 1: 16}[s] for s in d)
    assert padded > 20, "the cases do pad"
    # without an S/PDIF entry: dspi_mixed_pcm_bytes' values
    d = Dspi(0, 9, device=None)
    src = [16, 24, 24, 16, 16, 24, 16, 24, 24]
    assert d.sources_bytes(src, 3, 45)[0] == d.mixed_pcm_bytes(src, 3, 45)[0] and np.array_equal(d.sources_bytes(src, 3, 45)[1], d.mixed_pcm_bytes(src, 3, 45)[1])
    d.close()
    F = (2 ** 32 - 1) * 192
    got = run(driver, [f"off {F} 16 1 24", f"off {2 ** 60} 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1", "check 16 24 1", "check 16 2 1", "check 16 24", "check"])
    assert list(map(int, got[0].split())) == [26 * F, 0, 4 * F, 20 * F, 26 * F] and got[1] == "overflow"      # (4 F is a multiple of 16: F is one of 192)
    assert got[2:] == ["3 1", "1 1", "2 0", "0 0"]


# ---- host-only contexts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_sources_bytes_on_a_host_only_context(flavor):
    S = 37
    d = Dspi(flavor, S, device=None)
    r = random.Random(flavor)
    for n_blocks, block_len in ((1, 1), (3, 45), (5, 48), (5, 192)):
        src = [r.choice((16, 24, 1)) for _ in range(S)]
        total, off = d.sources_bytes(src, n_blocks, block_len)
        want = naive_offsets(src, n_blocks * block_len)
        assert total == want[-1] and off.tolist() == want
        sp = np.array(src, dtype=np.uint8)
        t = C.c_uint64(0)
        assert d.L.dspi_sources_bytes(d.h, sp.ctypes.data, n_blocks, block_len, C.byref(t), None) == 0 and t.value == total
        assert d.L.dspi_sources_bytes(d.h, sp.ctypes.data, n_blocks, block_len, None, None) == 0
    sp = np.full(S, 1, dtype=np.uint8)
    assert d.L.dspi_sources_bytes(None, sp.ctypes.data, 1, 48, None, None) == host.E_INVAL
    assert d.L.dspi_sources_bytes(d.h, None, 1, 48, None, None) == host.E_INVAL
    for nb, bl in ((0, 48), (1, 0), (1, 193)): assert d.L.dspi_sources_bytes(d.h, sp.ctypes.data, nb, bl, None, None) == host.E_INVAL
    sp[S - 1] = 20
    assert d.L.dspi_sources_bytes(d.h, sp.ctypes.data, 1, 48, None, None) == host.E_INVAL and f"stream {S - 1}" in d.L.dspi_last_error(d.h).decode()
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_process_sources_refusals_in_their_order(flavor):
    """INVAL (pointers, sources, lengths, flag bits, then what an S/PDIF source asks: rx, its records, alignment), then UNSUPPORTED (float: an
    active 16-bit stream with a preamp below 2^-103 — never an S/PDIF stream), then NODEVICE; no record changes"""
    S, F = 12, 48
    d = Dspi(flavor, S, device=None)
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=7) >= 0
    src = np.array([16, 24, 1] * (S // 3), dtype=np.uint8)      # stream 7: 24 bit
    bad = src.copy(); bad[7] = 16                                # stream 7: 16 bit
    spd = src.copy(); spd[7] = 1                                 # stream 7: S/PDIF
    data = np.zeros(S * F * 16 + 64, dtype=np.uint8)
    rx = np.zeros(S, dtype=host.SPDIF_RX); rx["held"] = 77
    before = rx.tobytes()
    out = host._Out(None, None, None, None)
    po, pd, pr = C.byref(out), data.ctypes.data, rx.ctypes.data
    call = lambda dp, sp, nb, bl, o, r, flags=0, words=None: d.L.dspi_process_sources(d.h, dp, sp, nb, bl, o, words, r, flags)
    refused = host.E_UNSUPPORTED if flavor else host.E_NODEVICE
    # the pointers
    assert d.L.dspi_process_sources(None, pd, src.ctypes.data, 1, F, po, None, pr, 0) == host.E_INVAL
    assert call(None, src.ctypes.data, 1, F, po, pr) == host.E_INVAL
    assert call(pd, None, 1, F, po, pr) == host.E_INVAL
    assert call(pd, src.ctypes.data, 1, F, None, pr) == host.E_INVAL
    # with DSPI_OUT_WIRE dspi_process_devices' flag rule comes first: before a bad source is looked at
    worse = bad.copy(); worse[9] = 8
    for flags in (host.OUT_WIRE | host.OUT_SPDIF, host.OUT_WIRE | host.OUT_I2S_SLOTS, host.OUT_WIRE | 0x80):
        assert call(pd, worse.ctypes.data, 1, F, po, pr, flags) == host.E_INVAL and "DSPI_OUT_WIRE" in d.L.dspi_last_error(d.h).decode()
    # a source value: before the lengths, the flag bits, rx and the preamp
    assert call(pd, worse.ctypes.data, 0, F, po, None, 0x80) == host.E_INVAL and "stream 9" in d.L.dspi_last_error(d.h).decode()
    # lengths and flag bits: before rx and the preamp
    for nb, bl, flags in ((0, F, 0), (1, 0, 0), (1, 193, 0), (1, F, 0x80), (1, F, 0x80000000), (1, F, host.OUT_SPDIF | host.OUT_TILED)):
        assert call(pd, bad.ctypes.data, nb, bl, po, None, flags) == host.E_INVAL and "rx" not in d.L.dspi_last_error(d.h).decode(), (nb, bl, flags)
    # what an S/PDIF source asks: before the preamp
    assert call(pd, bad.ctypes.data, 1, F, po, None) == host.E_INVAL and "(rx)" in d.L.dspi_last_error(d.h).decode()
    rx["sync"][5] = 193
    assert call(pd, bad.ctypes.data, 1, F, po, pr) == host.E_INVAL and "stream 5" in d.L.dspi_last_error(d.h).decode()
    rx["sync"][5] = 192; rx["sync"][0] = 500      # (stream 0 is no S/PDIF stream: its entry is not read)
    assert call(pd, bad.ctypes.data, 1, F, po, pr) == refused
    d.pause_streams(5, 1); rx["sync"][5] = 193   # (nor is a paused stream's)
    assert call(pd, bad.ctypes.data, 1, F, po, pr) == refused
    d.resume_streams(5, 1); rx["sync"][5] = 0
    assert call(pd + 8, bad.ctypes.data, 1, F, po, pr, host.MEM_DEVICE) == host.E_INVAL and "16-byte" in d.L.dspi_last_error(d.h).decode()
    assert call(pd, bad.ctypes.data, 1, F, po, pr + 2, host.MEM_DEVICE) == host.E_INVAL and "4-byte" in d.L.dspi_last_error(d.h).decode()
    assert call(pd + 8, bad.ctypes.data, 1, F, po, pr) == refused, "host memory needs no alignment"
    # the preamp: 16-bit streams only — never an S/PDIF stream, whatever its preamp
    assert call(pd, bad.ctypes.data, 1, F, po, pr) == refused
    if flavor: assert "stream 7" in d.L.dspi_last_error(d.h).decode()
    assert call(pd, spd.ctypes.data, 1, F, po, pr) == host.E_NODEVICE
    assert call(pd, src.ctypes.data, 1, F, po, pr) == host.E_NODEVICE
    assert call(pd, src.ctypes.data, 1, F, po, pr, host.OUT_WIRE) == host.E_NODEVICE
    assert call(pd, src.ctypes.data, 1, F, po, pr, host.OUT_WIRE | host.OUT_TILED) == host.E_NODEVICE
    # no S/PDIF source: dspi_process_mixed's refusals (rx may be NULL), uniform: dspi_process's
    pcm_only = np.array([16, 24] * (S // 2), dtype=np.uint8)
    assert call(pd, pcm_only.ctypes.data, 1, F, po, None) == host.E_NODEVICE
    all24, all_spdif = np.full(S, 24, dtype=np.uint8), np.full(S, 1, dtype=np.uint8)
    assert call(pd, all24.ctypes.data, 1, F, po, None) == host.E_NODEVICE
    assert call(pd, all24.ctypes.data, 1, F, po, None, 0x80) == host.E_INVAL
    assert call(pd, all_spdif.ctypes.data, 1, F, po, pr) == host.E_INVAL and "stream 0" in d.L.dspi_last_error(d.h).decode(), "stream 0's record is read now"
    rx["sync"][0] = 0
    assert call(pd, all_spdif.ctypes.data, 1, F, po, pr) == host.E_NODEVICE, "all S/PDIF is no uniform depth"
    assert rx.tobytes() == before, "no record changes"
    with pytest.raises(DspiError) as e: d.process_sources_host(data[:d.sources_bytes(src, 1, F)[0]], src, 1, F, rx)
    assert e.value.code == host.E_NODEVICE
    # DSPI_OUT_WIRE is this call's alone
    for other in (lambda: d.L.dspi_process_mixed(d.h, pd, pcm_only.ctypes.data, 1, F, po, None, host.OUT_WIRE),
                  lambda: d.L.dspi_process_devices(d.h, pd, pcm_only.ctypes.data, 1, F, po, None, host.OUT_WIRE),
                  lambda: d.L.dspi_process(d.h, pd, 24, 1, F, po, host.OUT_WIRE)):
        assert other() == host.E_INVAL
    d.close()


def test_spdif_decode_refusals_in_their_order():
    d = Dspi(1, 4, device=None)
    sub = np.zeros((3, 8, 4), dtype=np.uint32); rx = np.zeros(3, dtype=host.SPDIF_RX); pairs = np.full((3, 8, 2), 5, dtype=np.int32)
    ps, pr, pp = sub.ctypes.data, rx.ctypes.data, pairs.ctypes.data
    dec = d.L.dspi_spdif_decode
    assert dec(None, ps, 3, 8, pr, pp, 0) == host.E_INVAL
    for args in ((None, 3, 8, pr, pp, 0), (ps, 3, 8, None, pp, 0), (ps, 3, 8, pr, None, 0), (ps, 0, 8, pr, pp, 0), (ps, 3, 0, pr, pp, 0)):
        assert dec(d.h, *args) == host.E_INVAL, args
    assert dec(d.h, ps, 0xffffffff, 0xffffffff, pr, pp, host.MEM_DEVICE) == host.E_INVAL and "overflow" in d.L.dspi_last_error(d.h).decode()
    for flags in (host.OUT_TILED, 0x40, host.MEM_DEVICE | 0x80000000): assert dec(d.h, ps, 3, 8, pr, pp, flags) == host.E_INVAL
    for k in range(3):
        args = [ps, 3, 8, pr, pp, host.MEM_DEVICE]; args[(0, 3, 4)[k]] += 8
        assert dec(d.h, *args) == host.E_INVAL and "16-byte" in d.L.dspi_last_error(d.h).decode()
    rx["sync"][2] = 193
    assert dec(d.h, ps, 3, 8, pr, pp, 0) == host.E_INVAL and "line 2" in d.L.dspi_last_error(d.h).decode()
    rx["sync"][2] = 192
    assert dec(d.h, ps, 3, 8, pr, pp, 0) == host.E_NODEVICE and dec(d.h, ps, 3, 8, pr, pp, host.MEM_DEVICE) == host.E_NODEVICE
    assert (pairs == 5).all() and rx["sync"].tolist() == [0, 0, 192] and not rx["held"].any(), "a refused call writes nothing"
    d.close()
