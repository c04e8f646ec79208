"""The owner of the context's device memory without a GPU (dspi_amd/csrc/dspi_devmem.{h,cpp}): grow-only buffers, the growth that keeps its
contents, pinned areas, the registry's single release path, the table of the persistent per-stream arrays and their all-or-nothing
reallocation, through a g++ driver (tests/devmem_driver.cpp) whose allocator really allocates and records every call — built twice, plainly
and as a stand-alone program under AddressSanitizer + UBSan, and every driver case runs on both.  And what the source of the C-ABI must keep:
one place that allocates and frees, no capacity number beside a pointer."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("devmem_" + request.param) / "devmem_driver"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (SAN if request.param == "sanitized" else ["-O2"]) +
                   ["-o", str(exe), os.path.join(ROOT, "tests", "devmem_driver.cpp")] + [os.path.join(CSRC, f"dspi_{m}.cpp") for m in ("devmem", "resize", "boot")], check=True)
    return str(exe)


def run(driver, mode, arg, cases):
    """one line of input per case, one line of output per case; a sanitizer report ends the program with a failure"""
    text = "".join(c + "\n" for c in cases)
    p = subprocess.run([driver, mode] + ([str(arg)] if arg is not None else []), input=text, capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    for o in out: assert "LEAK" not in o and "?" not in o, o
    return out


# ---- one buffer --------------------------------------------------------------------------------------------------------------------------
def test_grow(driver):
    got, = run(driver, "grow", None, ["100 50 100 0 300 !400 0 20 21"])
    assert got.strip() == " ".join([
        "ok[A100=1]p100",                        # the first request allocates exactly its bytes
        "ok[]p100", "ok[]p100", "ok[]p100",      # a request that fits makes no allocator call
        "ok[F1 A300=2]p300",                     # growing: one free, then one allocation of exactly the bytes
        "refused[F2 X400]-0",                    # a refused allocation leaves {nullptr, 0} (the allocator left garbage in the pointer) ...
        "ok[]-0",                                # (nothing is still nothing)
        "ok[A20=3]p20",                          # ... and a later request succeeds, with no free before it
        "ok[F3 A21=4]p21"])


def test_grow_keep(driver):
    got, = run(driver, "keep", None, ["100 50 300 !400 350"])
    assert got.strip() == " ".join([
        "ok[A100=1]p100kept", "ok[]p100kept",
        "ok[A300=2 C2,1,100 F1]p300kept",        # allocate, copy old_cap bytes, free the old buffer — in this order
        "refused[X400]p300kept",                 # refused: the old buffer stays, with its contents
        "ok[A350=3 C3,2,300 F2]p350kept"])


def test_pinned(driver):
    got, = run(driver, "pinned", None, ["100:200:0 150:150:0 200:999:1 201:402:1 !500:500:1 8:8:1 8:64:1"])
    assert got.strip() == " ".join([
        "ok[HA200=1]p200-",                      # grow > bytes: the capacity is `grow`
        "ok[]p200-", "ok[]p200-",                # fits, whatever `grow` says (and an area that stays is asked nothing)
        "ok[HF1 HA402=2 HD2]p402d",              # replaced: one free, one allocation of `grow`, the device's address
        "refused[HF2 HX500]-0-",
        "ok[HA8=3 HD3]p8d", "ok[]p8d"])


# ---- the registry --------------------------------------------------------------------------------------------------------------------------
def test_release(driver):
    got = run(driver, "release", None, ["100 0 p50 20 p0 7", "0 0 p0", "5", ""])
    assert got[0] == "order ok [F1 HF2 F3 F4] [] 0", "every live buffer once, in construction order, no empty one; a second release does nothing"
    assert got[1] == "order ok [] [] 0" and got[2] == "order ok [F1] [] 0" and got[3] == "order ok [] [] 0"


# ---- the persistent per-stream arrays ------------------------------------------------------------------------------------------------------
# StateMap of both flavours (dspi_image.h make_state_map), and the five per-row byte counts as the code had them before the table existed
MAPS = {1: dict(n_ch=11, n_out=9, max_delay=4096, row=128), 0: dict(n_ch=7, n_out=5, max_delay=2048, row=64)}
K_RING_LEN, K_PDM_STATE_WORDS, K_BANDS = 1024, 9, 10


def n_slots(n_ch):
    return n_ch * K_BANDS * 2 + 8 + 4 + 5 + 1 + 1 + 3 + n_ch + 4      # eq, loudness, crossfeed, leveller, ring position, write index, mute, peaks, clip


def row_bytes(m):
    row = m["row"]
    return [("state", n_slots(m["n_ch"]) * row * 4, 1),                  # dspi_create: n_wg * n_slots * row * 4
            ("delay lines", m["n_out"] * m["max_delay"] * row * 4, 1),   # dspi_create: n_wg * n_out * max_delay * row * 4
            ("leveller ring", K_RING_LEN * 2 * row * 4, 1),              # dspi_create: n_wg * kRingLen * 2 * row * 4
            ("PDM state", K_PDM_STATE_WORDS * row * 4, 0),               # pdm_state: cap_wg * kPdmStateWords * row * 4
            ("PDM fade bases", row * 4, 0)]                              # dspi_pdm_fade: cap_wg * row * 4


@pytest.mark.parametrize("flavor", [0, 1])
def test_table(driver, flavor):
    got, = run(driver, "table", flavor, [""])
    assert got == "".join(f"{name}={b}/{at_create};" for name, b, at_create in row_bytes(MAPS[flavor]))
    assert n_slots(11) == 257 and n_slots(7) == 173


def test_overflow(driver):
    """the probe values of tests/test_resize_cpu.py's overflow cases, as row counts and (through synthetic StateMaps) as per-row byte counts"""
    top = (1 << 64) - 1
    real = MAPS[1]
    cases = [(3, n_slots(11), 9, 4096, 128), (0, n_slots(11), 9, 4096, 128), ((1 << 32) - 1, n_slots(11), 9, 4096, 128),
             (1 << 26, 1 << 20, 1, 1, 1 << 18),                  # 2^26 rows of 2^40 bytes of state: only the state array overflows
             (1 << 26, 1, 1 << 15, 1 << 23, 4),                  # ... only the delay lines do
             ((1 << 32) - 1, (1 << 30) + 1, 1, 1, 1),            # (2^32 - 1) * (2^32 + 4): the state array overflows
             ((1 << 32) - 1, 1 << 30, 1, 1, 1)]                  # (2^32 - 1) * 2^32 fits
    got = run(driver, "fit", None, [" ".join(map(str, c)) for c in cases])
    for (rows, slots, n_out, max_delay, row), g in zip(cases, got):
        per_row = [slots * row * 4, n_out * max_delay * row * 4, K_RING_LEN * 2 * row * 4, K_PDM_STATE_WORDS * row * 4, row * 4]
        want = [str(rows * b) if rows * b <= top else "overflow" for b in per_row]
        assert g.split() == want + ["refused" if "overflow" in want else "fit"], (rows, slots, n_out, max_delay, row)
    assert [g.split()[-1] for g in got] == ["fit", "fit", "fit", "refused", "refused", "refused", "fit"] and real["row"] == 128
    assert got[3].split()[:2] == ["overflow", str(1 << 46)] and got[4].split()[:2] == [str(1 << 30), "overflow"], "every entry of the table is checked"


@pytest.mark.parametrize("flavor", [0, 1])
def test_reallocate(driver, flavor):
    b = [x for _, x, _ in row_bytes(MAPS[flavor])]
    got = run(driver, "realloc", flavor, ["1 2 0 0 0 1", "1 2 3 1 1 1", "1 2 1 1 1 1", "1 2 5 1 1 1", "2 3 0 1 0 0", "3 1 0 1 1 1", "2 2 0 0 1 1"])
    # grow, the lazy arrays absent: every allocation, then the copy and its one wait, then the frees; the absent arrays stay absent
    assert got[0] == f"ok[A{2 * b[0]}=4 A{2 * b[1]}=5 A{2 * b[2]}=6 copied F1 F2 F3] moved{2 * b[0]} moved{2 * b[1]} moved{2 * b[2]} absent0 absent0 2 rows_kept"
    # the third allocation is refused: the first two are freed, all five pointers and the capacity stay, nothing was copied
    assert got[1] == f"refused[A{2 * b[0]}=6 A{2 * b[1]}=7 X{2 * b[2]} F6 F7] " + " ".join(f"same{x}" for x in b) + " 1 rows_kept"
    assert got[2] == f"refused[X{2 * b[0]}] " + " ".join(f"same{x}" for x in b) + " 1 rows_kept"
    assert got[3] == "refused[" + " ".join(f"A{2 * x}={6 + k}" for k, x in enumerate(b[:4])) + f" X{2 * b[4]} F6 F7 F8 F9] " + " ".join(f"same{x}" for x in b) + " 1 rows_kept"
    # the copy fails: the new arrays go, the old ones stay
    assert got[4] == "copy-failed[" + " ".join(f"A{3 * x}={5 + k}" for k, x in enumerate(b[:4])) + " copied F5 F6 F7 F8] " + " ".join(f"same{2 * x}" for x in b[:4]) + " absent0 2 rows_kept"
    # shrinking the capacity (dspi_reserve_streams): the rows in use come over
    assert got[5] == "ok[" + " ".join(f"A{x}={6 + k}" for k, x in enumerate(b)) + " copied F1 F2 F3 F4 F5] " + " ".join(f"moved{x}" for x in b) + " 1 rows_kept"
    # the fade bases without the modulator's words
    assert got[6] == f"ok[A{2 * b[0]}=5 A{2 * b[1]}=6 A{2 * b[2]}=7 A{2 * b[4]}=8 copied F1 F2 F3 F4] moved{2 * b[0]} moved{2 * b[1]} moved{2 * b[2]} absent0 moved{2 * b[4]} 2 rows_kept"


# ---- the source ----------------------------------------------------------------------------------------------------------------------------
def code_of(path):
    """the file without its comments and string literals"""
    with open(path) as f: text = f.read()
    text = re.sub(r'"(\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_one_place_allocates():
    names = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b")
    files = sorted(glob.glob(os.path.join(CSRC, "*.cpp")))
    assert os.path.join(CSRC, "dspi_capi.cpp") in files and os.path.join(CSRC, "dspi_devmem.cpp") in files
    for path in files:
        code = code_of(path)
        if os.path.basename(path) == "dspi_capi.cpp":      # only inside the HIP allocator policy
            m = re.search(r"struct HipAlloc \{.*?\n\};\n", code, flags=re.S)
            assert m and sorted(set(names.findall(m.group(0)))) == ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"]
            code = code.replace(m.group(0), "")
        assert not names.search(code), (path, names.search(code).group(0))
    for word in ("hipFreeAsync", "hipMallocAsync", "hipMemPool", "hipMallocFromPoolAsync"):      # frees must wait for the device
        for path in files: assert word not in code_of(path), (path, word)


def test_no_capacity_beside_a_pointer():
    code = code_of(os.path.join(CSRC, "dspi_capi.cpp"))
    ctx = re.search(r"struct dspi_ctx \{.*?\n\};\n", code, flags=re.S).group(0)
    assert "DevMem mem;" in ctx and ctx.index("DevMem mem;") < ctx.index("DevBuf<"), "the registry is constructed before every buffer that joins it"
    assert "d_state{mem}" in ctx and "cap_wg" in ctx      # (this is the context)
    assert not re.findall(r"\b\w+_cap\b", ctx), "a member ending in _cap"
    assert not re.findall(r"\b\w+_cap\b", code), "no `_cap` name anywhere in the C-ABI's code"
