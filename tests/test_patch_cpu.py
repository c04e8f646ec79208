"""The patch bay without a GPU: the layout and the plan of dspi_amd/csrc/dspi_patch.{h,cpp} through a g++ driver with its own main
(tests/patch_driver.cpp) against the model (tests/patch_model.py, written from the header's prose), and the calls of include/dspi.h on
host-only contexts: dspi_patched_bytes, and every refusal of dspi_process_patched in its order.  Everything is compared for equality."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import patch_model as PM
from dspi_amd import host, wire as W
from dspi_amd.host import Dspi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
RX = host.SPDIF_RX


def test_symbols_header_and_makefile():
    L = host.lib()
    for name in ("dspi_process_patched", "dspi_patched_bytes", "dspi_debug_patched_intake"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    assert host.PATCH == PM.PATCH and host.PATCH.itemsize == 12 and host.SRC_LINK == PM.LINK == 2 and host.MAX_VIEWS == PM.MAX_VIEWS == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + the patch bay: detect by symbol (dspi_process_patched;", "#define DSPI_SRC_LINK 2", "#define DSPI_MAX_VIEWS 8",
                 "typedef struct dspi_patch { uint32_t view; uint32_t line; uint32_t kind; } dspi_patch;", "a LINK stream occupies ZERO bytes of `in`",
                 "with no active LINK stream the call IS dspi_process_sources on device buffers", "a LINK stream and one view it IS dspi_process_linked",
                 "For every DISTINCT views[v].producer that is non-NULL, is not ctx, and is named by an active LINK stream",
                 "No view's wire may overlap out->pairs of the same call", "dspi_sources_bytes and dspi_process_sources keep refusing the value 2",
                 "ONE launch for all tiled views", "11. DSPI_E_NODEVICE on a host-only context"):
        assert word in text, word
    assert "I2S input, a tiled input" not in text
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()
    assert "dspi_patch" in mk.split("HOST =")[1].split("\n")[0].split() and "dspi_patchrx" in mk.split("KERNELS =")[1].split("\n")[0].split()
    for name in ("dspi_patch.h", "dspi_patch.cpp", "dspi_patchrx.hip"): assert os.path.exists(os.path.join(CSRC, name)), name


# ---- dspi_patched_bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_patched_bytes_equals_the_model(flavor):
    S = 23
    d = Dspi(flavor, S, device=None)
    rng = np.random.default_rng(flavor)
    d.pause_streams(4, 1)      # (a paused stream's entry still sizes its slot)
    for nb, bl in ((1, 1), (3, 45), (5, 48), (1, 192)):
        F = nb * bl
        for _ in range(20):
            src = rng.choice(np.array([16, 24, 1, 2], dtype=np.uint8), S)
            total, off = d.patched_bytes(src, nb, bl)
            want = PM.offsets(src, F)
            assert off.tolist() == want and total == want[-1], (src.tolist(), F)
            if not (src == 2).any(): assert d.sources_bytes(src, nb, bl)[0] == total and d.sources_bytes(src, nb, bl)[1].tolist() == want
    links = np.full(S, host.SRC_LINK, dtype=np.uint8)
    total, off = d.patched_bytes(links, 5, 48)
    assert total == 0 and not off.any(), "a context of LINK streams has no input buffer"
    one = links.copy(); one[7] = 16; one[9] = 1
    assert d.patched_bytes(one, 3, 45)[1].tolist() == [0] * 8 + [4 * 135, 544] + [544 + 16 * 135] * 14, "the rounding in front of an S/PDIF run is unchanged"
    # NULL outputs, and the refusals
    assert d.L.dspi_patched_bytes(d.h, links.ctypes.data, 1, 48, None, None) == 0
    err = lambda: d.L.dspi_last_error(d.h).decode()
    bad = links.copy(); bad[11] = 3
    total, off = C.c_uint64(77), np.full(S + 1, 77, dtype=np.uint64)
    assert d.L.dspi_patched_bytes(None, links.ctypes.data, 1, 48, C.byref(total), off.ctypes.data) == host.E_INVAL
    assert d.L.dspi_patched_bytes(d.h, None, 1, 48, C.byref(total), off.ctypes.data) == host.E_INVAL
    assert d.L.dspi_patched_bytes(d.h, bad.ctypes.data, 1, 48, C.byref(total), off.ctypes.data) == host.E_INVAL and "stream 11" in err()
    for nb, bl in ((0, 48), (1, 0), (1, 193)): assert d.L.dspi_patched_bytes(d.h, links.ctypes.data, nb, bl, C.byref(total), off.ctypes.data) == host.E_INVAL and "block_len" in err()
    assert total.value == 77 and (off == 77).all(), "a refused call writes nothing"
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_the_sources_calls_still_refuse_a_link(flavor):
    S, F = 6, 48
    d = Dspi(flavor, S, device=None)
    src = np.array([16, 24, 1, 2, 16, 24], dtype=np.uint8)
    buf = np.zeros(S * F * 16 + 16, dtype=np.uint8)
    rx = np.zeros(S, dtype=RX)
    out = host._Out(None, None, None, None)
    total, off = C.c_uint64(77), np.full(S + 1, 77, dtype=np.uint64)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    assert d.L.dspi_sources_bytes(d.h, src.ctypes.data, 1, F, C.byref(total), off.ctypes.data) == host.E_INVAL and "stream 3" in err()
    assert total.value == 77 and (off == 77).all()
    for flags in (0, host.MEM_DEVICE):
        assert d.L.dspi_process_sources(d.h, buf.ctypes.data + (-buf.ctypes.data) % 16, src.ctypes.data, 1, F, C.byref(out), None, rx.ctypes.data, flags) == host.E_INVAL and "stream 3" in err()
    d.pause_streams(3, 1)
    assert d.L.dspi_sources_bytes(d.h, src.ctypes.data, 1, F, C.byref(total), off.ctypes.data) == host.E_INVAL and "stream 3" in err(), "a paused stream's entry sizes its slot there"
    d.close()


# ---- the refusals of dspi_process_patched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_process_patched_refusals_in_their_order(flavor):
    """each refusal with every later one provoked as well: pointers, DSPI_MEM_DEVICE then the flag rule, the lengths, the sources, the views and
    the patches of ACTIVE LINK streams (their own order), in, rx, the preamp, then NODEVICE (a size that overflows needs over a million
    streams, the producer's device two GPUs: not tested)"""
    S, F = 12, 48
    d = Dspi(flavor, S, device=None)
    a = Dspi(1, 5, device=None)      # a producer: 4 pairs, 20 lines
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=8) >= 0      # (stream 8 is PCM16 below)
    buf = np.zeros(64, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    rx = np.zeros(S, dtype=RX)
    out = host._Out(None, None, None, None)
    po, pr = C.byref(out), rx.ctypes.data
    src = np.array([16, 24, 1, 2, 2, 2, 2, 2, 16, 24, 1, 2], dtype=np.uint8)
    bad_src = src.copy(); bad_src[9] = 3
    good_v = np.stack([a.wire_view_of(base, F), a.wire_view_of(base + 16, F, tiled=True)])
    bad_v = good_v.copy()
    for m, x in (("wire", 0), ("n_pairs", 3), ("tile_streams", 32), ("n_streams", 0), ("n_frames", F + 1)): bad_v[m][1] = x
    good_p = np.zeros(S, dtype=host.PATCH); good_p["view"] = np.arange(S) % 2; good_p["line"] = np.arange(S) % 20; good_p["kind"] = host.LINK_SPDIF
    bad_p = good_p.copy(); bad_p["view"][4] = 2; bad_p["kind"][5] = 3; bad_p["line"][6] = 20
    DEV = host.MEM_DEVICE
    err = lambda: d.L.dspi_last_error(d.h).decode()
    ptr = lambda x: x.ctypes.data if x is not None else None
    call = lambda i, s, v, nv, p, nb, bl, o, r, flags: d.L.dspi_process_patched(d.h, i, ptr(s), ptr(v), nv, ptr(p), nb, bl, o, None, r, flags)
    worst = (None, bad_src, bad_v, 9, bad_p)
    # 1. the pointers (everything else wrong as well)
    assert d.L.dspi_process_patched(None, None, ptr(bad_src), ptr(bad_v), 9, ptr(bad_p), 0, F, po, None, None, 0x80) == host.E_INVAL
    assert call(None, None, bad_v, 9, bad_p, 0, F, po, None, 0x80) == host.E_INVAL and call(*worst, 0, F, None, None, 0x80) == host.E_INVAL
    # 2. DSPI_MEM_DEVICE, then dspi_process_sources' flag rule
    for flags in (0x80, host.OUT_WIRE | host.OUT_TILED): assert call(*worst, 0, F, po, None, flags) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    for flags in (DEV | host.OUT_WIRE | host.OUT_SPDIF, DEV | host.OUT_WIRE | host.OUT_I2S_SLOTS, DEV | host.OUT_WIRE | 0x80):
        assert call(*worst, 0, F, po, None, flags) == host.E_INVAL and "DSPI_OUT_WIRE" in err()
    for flags in (DEV | 0x80, DEV | 0x80000000): assert call(*worst, 0, F, po, None, flags) == host.E_INVAL and "undefined flag bits" in err()
    assert call(*worst, 0, F, po, None, DEV | host.OUT_SPDIF | host.OUT_TILED) == host.E_INVAL and "DSPI_OUT_SPDIF goes with neither" in err()
    # 3. the lengths
    for nb, bl in ((0, F), (1, 0), (1, 193)): assert call(*worst, nb, bl, po, None, DEV) == host.E_INVAL and "block_len" in err()
    # 4. the sources
    assert call(*worst, 1, F, po, None, DEV) == host.E_INVAL and "stream 9" in err() and "DSPI_SRC_LINK" in err()
    # 5. with an active LINK stream: views and patches, n_views, every view (the second is the bad one), then the patches of such streams
    assert call(None, src, None, 9, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "needs views and patches" in err()
    assert call(None, src, bad_v, 9, None, 1, F, po, None, DEV) == host.E_INVAL and "needs views and patches" in err()
    for nv in (0, 9): assert call(None, src, bad_v, nv, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "n_views" in err()
    v = bad_v.copy()
    for member, value, word in (("wire", base + 8, "NULL"), ("wire", base + 16, "aligned"), ("n_pairs", 4, "n_pairs"), ("tile_streams", 128, "tile_streams"), ("n_streams", 5, "no streams"),
                                ("n_frames", F, "n_frames")):
        assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and word in err() and "view or stream 1" in err(), (member, err())
        v[member][1] = value
    only0 = bad_p.copy(); only0["view"] = 0      # (no active stream names the bad view: it is validated all the same)
    assert call(None, src, bad_v, 2, only0, 1, F, po, None, DEV) == host.E_INVAL and "NULL" in err()
    assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "names no view" in err() and "stream 4" in err()
    assert call(None, src, v, 1, good_p, 1, F, po, None, DEV) == host.E_INVAL and "names no view" in err() and "stream 3" in err(), "view < n_views"
    d.pause_streams(4, 1)
    assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "kind" in err() and "stream 5" in err(), "a paused stream's patch is ignored"
    bad_p["kind"][5] = host.LINK_NONE
    assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "kind" in err() and "stream 5" in err(), "an active LINK stream needs a link"
    bad_p["kind"][5] = host.LINK_I2S
    assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "no line" in err() and "stream 6" in err()
    bad_p["line"][6] = 19
    # 6. in
    assert call(None, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "needs `in`" in err()
    assert call(base + 8, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "16-byte" in err()
    # 7. the records
    assert call(base, src, v, 2, bad_p, 1, F, po, None, DEV) == host.E_INVAL and "(rx)" in err()
    assert call(base, src, v, 2, bad_p, 1, F, po, pr + 2, DEV) == host.E_INVAL and "4-byte" in err()
    # 9. the preamp: float contexts, active PCM16 streams only; then 11. the host-only context
    refused = host.E_UNSUPPORTED if flavor else host.E_NODEVICE
    assert call(base, src, v, 2, bad_p, 1, F, po, pr, DEV) == refused
    if flavor: assert "stream 8" in err()
    d.pause_streams(8, 1)
    assert call(base, src, v, 2, bad_p, 1, F, po, pr, DEV) == host.E_NODEVICE
    # what is not required is not asked for
    links = np.full(S, host.SRC_LINK, dtype=np.uint8)
    i2s = bad_p.copy(); i2s["kind"] = host.LINK_I2S
    assert call(None, links, v, 2, i2s, 1, F, po, None, DEV) == host.E_NODEVICE, "every stream an I2S link: neither `in` nor records"
    sp = i2s.copy(); sp["kind"][4] = host.LINK_SPDIF
    assert call(None, links, v, 2, sp, 1, F, po, None, DEV) == host.E_NODEVICE, "the only S/PDIF link is a paused stream's"
    pcm = np.where(np.arange(S) == 4, host.SRC_LINK, 24).astype(np.uint8)
    assert call(base, pcm, None, 0, None, 1, F, po, None, DEV) == host.E_NODEVICE, "the only LINK stream is paused: no views, no patches, no records"
    for flags in (DEV | host.OUT_WIRE, DEV | host.OUT_WIRE | host.OUT_TILED, DEV | host.OUT_TILED | host.OUT_CLIP_FLAGS): assert call(base, src, v, 2, bad_p, 1, F, po, pr, flags) == host.E_NODEVICE
    # the front end alone shares refusals 3 to 11
    dbg = lambda i, s, v_, nv, p, nb, bl, r: d.L.dspi_debug_patched_intake(d.h, i, ptr(s), ptr(v_), nv, ptr(p), nb, bl, r)
    assert dbg(base, None, v, 2, bad_p, 1, F, pr) == host.E_INVAL and dbg(base, src, v, 2, bad_p, 1, 193, pr) == host.E_INVAL and "block_len" in err()
    assert dbg(base, bad_src, v, 2, bad_p, 1, F, pr) == host.E_INVAL and "stream 9" in err()
    assert dbg(base, src, v, 9, bad_p, 1, F, pr) == host.E_INVAL and "n_views" in err() and dbg(base, src, v, 2, bad_p, 1, F, None) == host.E_INVAL and "(rx)" in err()
    assert dbg(base, src, v, 2, bad_p, 1, F, pr) == host.E_NODEVICE
    assert not rx.tobytes().strip(b"\0"), "no record changes"
    d.close(); a.close()


# ---- the plan against the model -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """own main: built with AddressSanitizer and UBSan where this g++ has their runtimes (asked of an empty program), else plain; which build
    ran is printed"""
    tmp = tmp_path_factory.mktemp("patch")
    exe = tmp / "patch_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "patch_driver.cpp"),
           os.path.join(CSRC, "dspi_patch.cpp"), os.path.join(CSRC, "dspi_link.cpp"), os.path.join(CSRC, "dspi_spdifrx.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("patch_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


def case_text(sources, active, views, patches, F):
    lines = [f"case {len(sources)} {len(views)} {F}"]
    lines += [f'{int(v["wire"])} {int(v["n_streams"])} {int(v["n_pairs"])} {int(v["tile_streams"])} {int(v["n_frames"])}' for v in views]
    lines += [f'{int(sources[s])} {int(active[s])} {int(patches[s]["view"])} {int(patches[s]["line"])} {int(patches[s]["kind"])}' for s in range(len(sources))]
    return "\n".join(lines) + "\n"


def run(driver, text):
    out = subprocess.run([driver], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    cases, cur = [], []
    for line in out:
        if line == "end": cases.append(cur); cur = []
        else: cur.append(line)
    assert not cur
    return cases


def want_text(sources, active, views, patches, F):
    """what the driver prints for a valid case, from the model"""
    p = PM.plan(sources, active, views, patches, F)
    j = lambda name, xs: " ".join([name] + [str(x) for x in xs])
    out = ["sources 0 ok", "views 0 ok", f'bytes ok {p["in_offsets"][-1]}',
           f"needs {int(any(active[s] and sources[s] != PM.LINK for s in range(len(sources))))} {int(PM.needs_rx(sources, active, patches))}",
           j("flags", p["flags"]), j("in_offsets", p["in_offsets"]), j("in_kinds", p["in_kinds"]), j("pcm_mask", p["pcm_mask"])]
    for v, d in enumerate(p["views"]):
        out.append(f'view {v} {d["used"]} {d["any_spdif"]} {d["any_i2s"]}')
        if "offsets" in d: out += [j("offsets", d["offsets"]), j("links", d["links"]), j("kinds", d["kinds"])]
    if "cols" in p: out.append(j("cols 1", p["cols"]))
    return out


def random_case(rng, n, n_views, F, weights):
    views = np.zeros(n_views, dtype=host.WIRE_VIEW)
    for v in range(n_views):
        R = (0, 64, 128)[(v + int(rng.integers(3))) % 3]
        views[v] = ((1 << 20) * (v + 1) * 16, int(rng.integers(1, 300)), (2, 4)[int(rng.integers(2))] if R == 0 else (2 if R == 64 else 4), R, F, 0)
    sources = rng.choice(np.array([16, 24, 1, 2], dtype=np.uint8), n, p=weights)
    active = (rng.random(n) > 0.15).astype(np.uint8)
    patches = np.zeros(n, dtype=host.PATCH)
    used = rng.integers(0, n_views, n)
    if n_views > 2: used[used == 1] = 0      # a hole: nobody names view 1, and fan-out into view 0
    patches["view"] = used
    patches["line"] = [int(rng.integers(0, int(views[v]["n_streams"]) * int(views[v]["n_pairs"]))) for v in used]
    patches["kind"] = rng.integers(1, 3, n)
    paused = np.flatnonzero(active == 0)
    patches["view"][paused] = 0xffffffff; patches["kind"][paused] = 77; patches["line"][paused] = 0xffffffff      # (a paused stream's patch is ignored)
    return sources, active, views, patches


def test_plan_equals_the_model(driver):
    rng = np.random.default_rng(2026)
    cases = []
    for n_views in range(1, 9):
        for k, n in enumerate((1, 31, 64, 150)):
            weights = [(0.15, 0.15, 0.2, 0.5), (0, 0, 0, 1), (0.3, 0.3, 0.4, 0), (0.1, 0.1, 0.1, 0.7)][k]
            F = (135, 240, 5, 1)[k]
            cases.append(random_case(rng, n, n_views, F, weights) + (F,))
    # every layout in one call, by hand: views of layout 0, 64 and 128 all used
    n = 12
    views = np.zeros(3, dtype=host.WIRE_VIEW)
    views[0] = (4096, 100, 2, 0, 48, 0); views[1] = (8192, 100, 2, 64, 48, 0); views[2] = (1 << 33, 150, 4, 128, 48, 0)
    patches = np.zeros(n, dtype=host.PATCH); patches["view"] = np.arange(n) % 3; patches["line"] = [199, 199, 599, 0, 64 * 2 + 1, 128 * 4 + 3, 5, 5, 5, 7, 63 * 2, 149 * 4]; patches["kind"] = 1 + np.arange(n) // 3 % 2
    cases.append((np.full(n, 2, dtype=np.uint8), np.ones(n, dtype=np.uint8), views, patches, 48))
    got = run(driver, "".join(case_text(*c) for c in cases))
    assert len(got) == len(cases)
    seen = set()
    for c, g in zip(cases, got):
        want = want_text(*c)
        assert g == want, (c, [x for x in zip(g, want) if x[0] != x[1]][:2])
        seen |= {(int(v["tile_streams"]), d["used"]) for v, d in zip(c[2], PM.plan(*c)["views"])}
    assert seen >= {(0, 1), (64, 1), (128, 1), (0, 0)}, "every layout used, and a view nobody names"
    # the resolved column by hand: view 2 above, line 128 * 4 + 3 is stream 128, pair 3: tile 1, column 0
    assert PM.column(views[2], 128 * 4 + 3) == (1 << 33) + 4 * ((1 * 4 + 3) * 48 * 4 * 128 + 0) and PM.column(views[1], 64 * 2 + 1) == 8192 + 4 * ((1 * 2 + 1) * 48 * 4 * 64)


def test_plan_refusals_through_the_driver(driver):
    """the module's own refusal functions: a bad source, an active stream's bad patch, a size that overflows"""
    views = np.zeros(2, dtype=host.WIRE_VIEW)
    views[0] = (4096, 10, 2, 0, 48, 0); views[1] = (8192, 10, 2, 64, 48, 0)
    src = np.array([2, 16, 2, 1], dtype=np.uint8)
    act = np.ones(4, dtype=np.uint8)
    p = np.zeros(4, dtype=host.PATCH); p["kind"] = 1
    def first(sources=src, active=act, v=views, patches=p, F=48): return run(driver, case_text(sources, active, v, patches, F))[0]
    assert first(sources=np.array([2, 16, 5, 1], dtype=np.uint8))[0].startswith("sources 2 a source is none of")
    q = p.copy(); q["view"][2] = 2
    assert first(patches=q)[1].startswith("views 2 a patch names no view")
    assert first(patches=q, active=np.array([1, 1, 0, 1], dtype=np.uint8))[1] == "views 0 ok"
    q = p.copy(); q["line"][0] = 20
    assert first(patches=q)[1].startswith("views 0 a patch names no line")
    q = p.copy(); q["kind"][2] = 0
    assert first(patches=q)[1].startswith("views 2 a patch's kind")
    w = views.copy(); w["tile_streams"][1] = 32
    assert first(v=w)[1].startswith("views 1 the view's tile_streams")
    assert first(v=views[:0])[1].startswith("views 0 an active DSPI_SRC_LINK stream needs views") or first(v=views[:0])[1].startswith("views 0 n_views")
    assert first(F=47)[1].startswith("views 0 the view's n_frames")
    big = np.full(4, 1, dtype=np.uint8)
    assert first(sources=big, F=(1 << 64) // 60)[2].startswith("bytes overflow")
