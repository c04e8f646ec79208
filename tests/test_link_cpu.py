"""Chained devices without a GPU: the CPU reader, the index functions and the refusals of dspi_amd/csrc/dspi_link.{h,cpp} through a g++ driver
(tests/linkrx_driver.cpp) against the model (tests/linkrx_model.py: the four index formulas from the header's prose, tests/spdifrx_model.py's
receiver, `>> 8`) — both layouts, both word formats, in one call and split at every frame —, and the calls of include/dspi.h on host-only
contexts: dspi_wire_view_of / dspi_link_kinds, and every refusal of dspi_process_linked and dspi_wire_decode in its order.  Everything is
compared for equality."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import linkrx_model as LM
import spdifrx_model as M
from dspi_amd import host, wire as W
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
RX = host.SPDIF_RX
POISON = 0xEE
# (tile_streams, streams, pairs): both tiles ragged in their last row
SHAPES = {"q28": (64, 100, 2), "f32": (128, 150, 4)}
FRAMES = (135, 240)      # odd, 6 F = 2 mod 4; across the 192-frame block


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_process_linked"), "libdspi_mi355x has no dspi_process_linked"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """own main: built with AddressSanitizer and UBSan where this g++ has their runtimes (asked of an empty program), else plain; which build
    ran is printed"""
    tmp = tmp_path_factory.mktemp("linkrx")
    exe = tmp / "linkrx_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "linkrx_driver.cpp"),
           os.path.join(CSRC, "dspi_link.cpp"), os.path.join(CSRC, "dspi_spdifrx.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("linkrx_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe), tmp


def run(driver, script):
    out = subprocess.run([driver[0]], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script), out
    return out


def poison_records(n): return np.frombuffer(bytes([POISON]) * (40 * n), dtype=RX).copy()


def records_for(links):
    """a receiver just started for every S/PDIF link, poison for every other entry (no call may touch those)"""
    rx = poison_records(len(links))
    rx[links["kind"] == LM.SPDIF] = np.zeros((), dtype=RX)
    return rx


class Job:
    """one `dec` command: its files, and what comes back"""
    def __init__(self, tmp, tag, wire, S, P, R, F, links, rx):
        self.n, self.F = len(links), F
        self.paths = [str(tmp / f"{tag}.{k}") for k in ("wire", "links", "rx", "out")]
        for path, a in zip(self.paths, (wire, links, rx)): np.ascontiguousarray(a).tofile(path)
        self.cmd = f"dec {self.paths[0]} {S} {P} {R} {F} {self.paths[1]} {self.paths[2]} {self.paths[3]}"

    def result(self):
        raw = np.fromfile(self.paths[3], dtype=np.uint8)
        n, F = self.n, self.F
        assert raw.size == n * (40 + 8 * F + 6 * F)
        for p in self.paths: os.remove(p)
        return raw[:40 * n].view(RX).copy(), raw[40 * n:40 * n + 8 * F * n].view("<i4").reshape(n, F, 2).copy(), raw[40 * n + 8 * F * n:].reshape(n, 6 * F).copy()


@functools.lru_cache(maxsize=None)
def built(shape, F):
    R, S, P = SHAPES[shape]
    lines, kinds = LM.build(S, P, F, seed=F + S)
    return lines, kinds, {0: LM.lay(lines, S, P, 0, F), R: LM.lay(lines, S, P, R, F)}


@functools.lru_cache(maxsize=None)
def model_line(shape, F, tiled, line):
    """one line of `built` from a record of zeros -> (pairs, record or None): the same for every link that names it"""
    R, S, P = SHAPES[shape]
    lines, kinds, wires = built(shape, F)
    rx = M.new_rx() if kinds[line] == LM.SPDIF else None
    pairs = LM.decode(wires[R if tiled else 0], P, R if tiled else 0, F, line, int(kinds[line]), rx)
    return pairs, (M.to_record(rx) if rx is not None else None)


def test_symbols_and_header():
    L = host.lib()
    for name in ("dspi_process_linked", "dspi_wire_decode", "dspi_wire_view_of", "dspi_link_kinds"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    assert host.LINK == LM.LINK and host.LINK.itemsize == 8 and host.WIRE_VIEW.itemsize == 32 and (host.LINK_NONE, host.LINK_SPDIF, host.LINK_I2S) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + chained devices: detect by symbol (dspi_process_linked;", "#define DSPI_LINK_NONE  0u", "#define DSPI_LINK_SPDIF 1u", "#define DSPI_LINK_I2S   2u",
                 "} dspi_wire_view;", "typedef struct dspi_link { uint32_t line; uint32_t kind; } dspi_link;", "((s / R * P + p) * F) * 4 * R", "(int32_t)word >> 8"):
        assert word in text, word
    assert "I2S input, a tiled input" not in text, "both are in scope now"
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()
    assert "dspi_link" in mk.split("HOST =")[1].split("\n")[0].split() and "dspi_linkrx" in mk.split("KERNELS =")[1].split("\n")[0].split()


# ---- the CPU reader against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reader_equals_the_model_in_every_link_order(driver, shape, tiled, F):
    R, S, P = SHAPES[shape]
    lines, kinds, wires = built(shape, F)
    Rv = R if tiled else 0
    orders = LM.link_orders(kinds)
    jobs = [Job(driver[1], name, wires[Rv], S, P, Rv, F, links, records_for(links)) for name, links in orders.items()]
    assert run(driver, [j.cmd for j in jobs]) == ["ok"] * len(jobs)
    seen = set()
    for (name, links), job in zip(orders.items(), jobs):
        rx, pairs, packed = job.result()
        for i, (line, kind) in enumerate(links.tolist()):
            what = (shape, tiled, F, name, i, line, kind)
            if kind == LM.NONE:
                assert (pairs[i] == 0x5A5A5A5A).all() and (packed[i] == 0x5A).all() and rx[i].tobytes() == bytes([POISON]) * 40, what
                continue
            want, rec = model_line(shape, F, tiled, line)
            assert np.array_equal(pairs[i], want) and np.array_equal(packed[i], M.pack24(want)), what
            assert rx[i].tobytes() == (rec.tobytes() if kind == LM.SPDIF else bytes([POISON]) * 40), what + (rx[i], rec)
            if kind == LM.SPDIF: seen.add((int(rec["state"]), bool(rec["held"]), bool(rec["coding_errors"]), bool(rec["parity_err_count"])))
    assert {s for s, *_ in seen} == {0, 1, 2} and any(h for _, h, _, _ in seen) and any(c for _, _, c, _ in seen) and any(p for *_, p in seen), "the lines do what they were built for"
    # the I2S rule itself: the sample is the word's upper 24 bits, whatever the low byte
    line = next(l for l in range(S * P) if kinds[l] == LM.I2S)
    assert np.array_equal(model_line(shape, F, tiled, line)[0], lines[line].view(np.int32) >> 8) and (lines[line] & 0xff).any()


@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
@pytest.mark.parametrize("shape,F", [("q28", 135), ("f32", 240)])
def test_reader_split_at_every_frame(driver, shape, tiled, F):
    """two views of k and F - k frames of the same lines (another F: another layout), the records carried: S/PDIF lines of every kind of trouble,
    two I2S lines and a hole, the first and the last streams of the ragged tile among them"""
    R, S, P = SHAPES[shape]
    Rv = R if tiled else 0
    lines, kinds, _ = built(shape, F)
    spdif = [l for l in range(S * P) if kinds[l] == LM.SPDIF]
    pick = spdif[:12:2] + spdif[-2:] + [l for l in range(S * P) if kinds[l] == LM.I2S][:1] + [S * P - 1 if kinds[S * P - 1] == LM.I2S else S * P - 2]
    links = np.zeros(len(pick) + 1, dtype=LM.LINK)
    links["line"][:-1] = pick; links["kind"][:-1] = kinds[pick]      # (the last entry: a hole)
    n = len(links)
    rx0 = records_for(links)
    script, jobs = [], []
    for k in range(1, F):
        a = Job(driver[1], f"a{k}", LM.lay({l: lines[l][:k] for l in pick}, S, P, Rv, k), S, P, Rv, k, links, rx0)
        script.append(a.cmd); jobs.append(a)
    assert run(driver, script) == ["ok"] * len(script)
    mids = [j.result() for j in jobs]
    script, jobs = [], []
    for k in range(1, F):
        b = Job(driver[1], f"b{k}", LM.lay({l: lines[l][k:] for l in pick}, S, P, Rv, F - k), S, P, Rv, F - k, links, mids[k - 1][0])
        script.append(b.cmd); jobs.append(b)
    assert run(driver, script) == ["ok"] * len(script)
    for k, job in zip(range(1, F), jobs):
        rx_mid, pa, ka = mids[k - 1]
        rx_end, pb, kb = job.result()
        for i, (line, kind) in enumerate(links.tolist()):
            if kind == LM.NONE:
                assert (pa[i] == 0x5A5A5A5A).all() and (pb[i] == 0x5A5A5A5A).all() and rx_end[i].tobytes() == bytes([POISON]) * 40
                continue
            w = lines[line]
            if kind == LM.I2S:
                want = w.view(np.int32) >> 8
                assert rx_mid[i].tobytes() == rx_end[i].tobytes() == bytes([POISON]) * 40
            else:
                rx = M.new_rx()
                first = M.receive(rx, w[:k]); mid = M.to_record(rx)
                want = np.concatenate([first, M.receive(rx, w[k:])])
                assert rx_mid[i].tobytes() == mid.tobytes() and rx_end[i].tobytes() == M.to_record(rx).tobytes(), (shape, tiled, k, line, rx_end[i], M.to_record(rx))
            got = np.concatenate([pa[i], pb[i]])
            assert np.array_equal(got, want) and np.array_equal(np.concatenate([ka[i], kb[i]]), M.pack24(want)), (shape, tiled, k, line)


def test_view_and_link_rules(driver):
    """link_view_why, one refusal per line of the contract, in its order; link_view_words; links_check / links_any"""
    got = run(driver, ["view 0 0 3 32 0 48 1", "view 8 0 3 32 0 48 1", "view 8 0 3 32 0 48 0", "view 16 0 2 32 0 48 1", "view 16 0 2 0 0 48 1", "view 16 5 4 128 47 48 1",
                       "view 16 5 4 128 48 48 1", "view 16 5 2 64 0 0 0", "view 16 5 2 64 7 0 0", "view 16 4294967295 4 128 4294967295 4294967295 1", "view 16 1048576 4 0 4294967295 4294967295 1",
                       "words 100 2 64 135", "words 100 2 0 135", "words 150 4 128 240", "words 4294967295 4 128 4294967295", "words 1048576 4 0 4294967295"])
    assert "NULL" in got[0] and "aligned" in got[1] and "n_pairs" in got[2] and "tile_streams" in got[3] and "no streams" in got[4] and "n_frames" in got[5] and got[6] == "ok"
    assert "no frames" in got[7] and got[8] == "ok" and "overflows" in got[9] and got[10] == "ok"
    assert got[11:] == [str(2 * 2 * 135 * 4 * 64), str(100 * 2 * 135 * 4), str(2 * 4 * 240 * 4 * 128), "overflow", str(1048576 * 4 * (2 ** 32 - 1) * 4)]
    got = run(driver, ["check 8 0 0:1:1 7:2:1", "check 8 0 0:1:1 8:2:1", "check 8 0 0:1:1 8:2:0 3:0:1", "check 8 1 0:1:1 8:2:0 3:0:1 9:0:1 2:3:1", "check 8 0 1:2:1 5:2:1", "check 8 0 1:1:0 5:2:0"])
    assert got == ["2 1 1", "1 1 1", "2 1 0", "4 1 0", "2 0 1", "2 0 0"]


# ---- host-only contexts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_view_of_and_link_kinds(flavor):
    S = 9
    d = Dspi(flavor, S, device=None)
    P, R = d.P, d.tile_streams()
    assert (P, R) == ((4, 128) if flavor else (2, 64))
    v = d.wire_view_of(0x1000, 240)
    assert (int(v["wire"]), int(v["n_streams"]), int(v["n_pairs"]), int(v["tile_streams"]), int(v["n_frames"]), int(v["producer"])) == (0x1000, S, P, 0, 240, d.h.value)
    assert int(d.wire_view_of(0, 135, tiled=True)["tile_streams"]) == R
    raw = np.zeros((), dtype=host.WIRE_VIEW)
    for flags in (host.MEM_DEVICE, host.OUT_SPDIF, 0x80000000): assert d.L.dspi_wire_view_of(d.h, None, 1, flags, raw.ctypes.data) == host.E_INVAL
    assert d.L.dspi_wire_view_of(None, None, 1, 0, raw.ctypes.data) == host.E_INVAL and d.L.dspi_wire_view_of(d.h, None, 1, 0, None) == host.E_INVAL
    assert not raw.tobytes().strip(b"\0"), "a refused call writes nothing"
    # the kinds follow REQ_SET_OUTPUT_TYPE, per stream
    assert (d.link_kinds(np.arange(S * P))["kind"] == host.LINK_SPDIF).all()
    assert d.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 1 | (1 << 8), 1, 3) == b"\x00"      # stream 3, slot 1: I2S
    assert d.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 0 | (1 << 8), 1, 7) == b"\x00"      # stream 7, slot 0
    want = np.full(S * P, host.LINK_SPDIF); want[3 * P + 1] = want[7 * P] = host.LINK_I2S
    assert np.array_equal(d.link_kinds(np.arange(S * P))["kind"], want)
    back = np.arange(S * P)[::-1]
    assert np.array_equal(d.link_kinds(np.repeat(back, 2))["kind"], np.repeat(want[::-1], 2)), "any order, any line twice"
    assert d.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 1 | (0 << 8), 1, 3) == b"\x00"      # ... and back: the CURRENT type
    want[3 * P + 1] = host.LINK_SPDIF
    assert np.array_equal(d.link_kinds(np.arange(S * P))["kind"], want)
    links = np.zeros(3, dtype=host.LINK); links["line"] = (0, S * P, 1); links["kind"] = 77
    assert d.L.dspi_link_kinds(d.h, links.ctypes.data, 3) == host.E_INVAL and "link 1" in d.L.dspi_last_error(d.h).decode() and (links["kind"] == 77).all()
    assert d.L.dspi_link_kinds(None, links.ctypes.data, 3) == host.E_INVAL and d.L.dspi_link_kinds(d.h, None, 3) == host.E_INVAL and d.L.dspi_link_kinds(d.h, None, 0) == 0
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_process_linked_refusals_in_their_order(flavor):
    """each refusal with every later one provoked as well: pointers, DSPI_MEM_DEVICE then the flag rule, the lengths, the view (its own order),
    the links of ACTIVE streams, rx, then NODEVICE (the producer's device needs two GPUs: not tested)"""
    S, F = 12, 48
    d = Dspi(flavor, S, device=None)
    a = Dspi(1, 5, device=None)      # the producer: 4 pairs, 20 lines
    buf = np.zeros(64, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    rx = np.zeros(S, dtype=RX)
    out = host._Out(None, None, None, None)
    po, pr = C.byref(out), rx.ctypes.data
    good_v = a.wire_view_of(base, F)
    good_l = np.zeros(S, dtype=host.LINK); good_l["line"] = np.arange(S) % 20; good_l["kind"] = host.LINK_SPDIF
    bad_v = good_v.copy(); bad_v["wire"] = 0; bad_v["n_pairs"] = 3; bad_v["tile_streams"] = 32; bad_v["n_streams"] = 0; bad_v["n_frames"] = F + 1
    bad_l = good_l.copy(); bad_l["kind"][4] = 3; bad_l["line"][6] = 20
    DEV = host.MEM_DEVICE
    err = lambda: d.L.dspi_last_error(d.h).decode()
    call = lambda v, l, nb, bl, o, r, flags: d.L.dspi_process_linked(d.h, v.ctypes.data if v is not None else None, l.ctypes.data if l is not None else None, nb, bl, o, None, r, flags)
    # 1. the pointers (everything else wrong as well)
    assert d.L.dspi_process_linked(None, bad_v.ctypes.data, bad_l.ctypes.data, 0, F, po, None, None, 0x80) == host.E_INVAL
    for args in ((None, bad_l, 0, F, po, None, 0x80), (bad_v, None, 0, F, po, None, 0x80), (bad_v, bad_l, 0, F, None, None, 0x80)): assert call(*args) == host.E_INVAL
    # 2. DSPI_MEM_DEVICE, then dspi_process_sources' flag rule
    assert call(bad_v, bad_l, 0, F, po, None, 0x80) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    assert call(bad_v, bad_l, 0, F, po, None, host.OUT_WIRE | host.OUT_TILED) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    for flags in (DEV | host.OUT_WIRE | host.OUT_SPDIF, DEV | host.OUT_WIRE | host.OUT_I2S_SLOTS, DEV | host.OUT_WIRE | 0x80):
        assert call(bad_v, bad_l, 0, F, po, None, flags) == host.E_INVAL and "DSPI_OUT_WIRE" in err()
    for flags in (DEV | 0x80, DEV | 0x80000000): assert call(bad_v, bad_l, 0, F, po, None, flags) == host.E_INVAL and "undefined flag bits" in err()
    assert call(bad_v, bad_l, 0, F, po, None, DEV | host.OUT_SPDIF | host.OUT_TILED) == host.E_INVAL and "DSPI_OUT_SPDIF goes with neither" in err()
    # 3. the lengths
    for nb, bl in ((0, F), (1, 0), (1, 193)): assert call(bad_v, bad_l, nb, bl, po, None, DEV) == host.E_INVAL and "block_len" in err()
    # 4. the view, member by member
    v = bad_v.copy()
    for member, value, word in (("wire", base + 8, "NULL"), ("wire", base, "aligned"), ("n_pairs", 4, "n_pairs"), ("tile_streams", 128, "tile_streams"), ("n_streams", 5, "no streams"),
                                ("n_frames", F, "n_frames")):
        assert call(v, bad_l, 1, F, po, None, DEV) == host.E_INVAL and word in err(), (member, err())
        v[member] = value
    big = good_v.copy(); big["n_streams"] = 0xffffffff; big["tile_streams"] = 128; big["n_frames"] = 0xffffffff
    assert d.L.dspi_process_linked(d.h, big.ctypes.data, bad_l.ctypes.data, 0xffffffff // 3, 3, po, None, None, DEV) == host.E_INVAL and "overflows" in err()
    # 5. the links of the active streams
    assert call(v, bad_l, 1, F, po, None, DEV) == host.E_INVAL and "stream 4" in err()
    bad_l["kind"][4] = host.LINK_NONE
    assert call(v, bad_l, 1, F, po, None, DEV) == host.E_INVAL and "stream 4" in err(), "an active stream needs a link"
    d.pause_streams(4, 1)
    assert call(v, bad_l, 1, F, po, None, DEV) == host.E_INVAL and "stream 6" in err(), "a paused stream's entry is ignored"
    bad_l["line"][6] = 19
    # 6. the records
    assert call(v, bad_l, 1, F, po, None, DEV) == host.E_INVAL and "(rx)" in err()
    assert call(v, bad_l, 1, F, po, pr + 2, DEV) == host.E_INVAL and "4-byte" in err()
    # 8. the host-only context: everything before it holds
    assert call(v, bad_l, 1, F, po, pr, DEV) == host.E_NODEVICE
    i2s = bad_l.copy(); i2s["kind"] = host.LINK_I2S
    assert call(v, i2s, 1, F, po, None, DEV) == host.E_NODEVICE, "no S/PDIF link: no records"
    sp = i2s.copy(); sp["kind"][4] = host.LINK_SPDIF
    assert call(v, sp, 1, F, po, None, DEV) == host.E_NODEVICE, "the only S/PDIF link is a paused stream's"
    tv = a.wire_view_of(base, 3 * 45, tiled=True)
    for flags in (DEV, DEV | host.OUT_WIRE, DEV | host.OUT_WIRE | host.OUT_TILED, DEV | host.OUT_TILED | host.OUT_CLIP_FLAGS): assert call(tv, good_l, 3, 45, po, pr, flags) == host.E_NODEVICE
    assert not rx.tobytes().strip(b"\0"), "no record changes"
    d.close(); a.close()


def test_wire_decode_refusals_in_their_order():
    d = Dspi(1, 4, device=None)
    F, n = 8, 3
    wire = np.zeros(4 * 4 * F * 4 + 8, dtype=np.uint32)
    base = wire.ctypes.data + (-wire.ctypes.data) % 16
    rx = np.zeros(n, dtype=RX); pairs = np.full((n, F, 2) , 5, dtype=np.int32)
    pr, pp = rx.ctypes.data, pairs.ctypes.data
    assert pr % 16 == 0 and pp % 16 == 0
    v = d.wire_view_of(base, F)
    links = np.zeros(n, dtype=host.LINK); links["line"] = (0, 15, 3); links["kind"] = (host.LINK_SPDIF, host.LINK_I2S, host.LINK_SPDIF)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    dec = lambda v_, l_, n_, r_, p_, flags: d.L.dspi_wire_decode(d.h, v_.ctypes.data if v_ is not None else None, l_.ctypes.data if l_ is not None else None, n_, r_, p_, flags)
    bad_v = v.copy(); bad_v["n_pairs"] = 3
    bad_l = links.copy(); bad_l["kind"][1] = 3
    assert d.L.dspi_wire_decode(None, v.ctypes.data, links.ctypes.data, n, pr, pp, 0) == host.E_INVAL
    for args in ((None, bad_l, n, None, pp, 0x40), (bad_v, None, n, None, pp, 0x40), (bad_v, bad_l, n, None, None, 0x40), (bad_v, bad_l, 0, None, pp, 0x40)):
        assert dec(*args) == host.E_INVAL and "NULL pointer or no link" in err()
    for flags in (host.OUT_TILED, 0x40, host.MEM_DEVICE | 0x80000000): assert dec(bad_v, bad_l, n, None, pp, flags) == host.E_INVAL and "only flag" in err()
    assert dec(bad_v, bad_l, n, None, pp, 0) == host.E_INVAL and "n_pairs" in err()
    zero = v.copy(); zero["n_frames"] = 0
    assert dec(zero, bad_l, n, None, pp, 0) == host.E_INVAL and "no frames" in err()
    off = v.copy(); off["wire"] = base + 4
    assert dec(off, bad_l, n, None, pp, host.MEM_DEVICE) == host.E_INVAL and "aligned" in err()
    assert dec(off, bad_l, n, None, pp, 0) == host.E_INVAL and "link 1" in err(), "host memory needs no alignment"
    bad_l["kind"][1] = host.LINK_I2S; bad_l["line"][1] = 16
    assert dec(v, bad_l, n, None, pp, 0) == host.E_INVAL and "link 1" in err()
    bad_l["kind"][1] = host.LINK_NONE
    assert dec(v, bad_l, n, None, pp, 0) == host.E_INVAL and "(rx)" in err(), "a hole's line means nothing"
    assert dec(v, links, n, pr + 8, pp, host.MEM_DEVICE) == host.E_INVAL and "16-byte" in err()
    assert dec(v, links, n, pr, pp + 8, host.MEM_DEVICE) == host.E_INVAL and "16-byte" in err()
    rx["sync"][2] = 193
    assert dec(v, links, n, pr, pp, 0) == host.E_INVAL and "link 2" in err()
    rx["sync"][2] = 192; rx["sync"][1] = 500      # (link 1 is an I2S link: its record is not read)
    assert dec(v, links, n, pr, pp, 0) == host.E_NODEVICE and dec(v, links, n, pr, pp, host.MEM_DEVICE) == host.E_NODEVICE
    i2s = links.copy(); i2s["kind"] = host.LINK_I2S
    assert dec(v, i2s, n, None, pp, 0) == host.E_NODEVICE, "no S/PDIF link: no records"
    assert (pairs == 5).all() and rx["sync"].tolist() == [0, 500, 192] and not rx["held"].any(), "a refused call writes nothing"
    d.close()
