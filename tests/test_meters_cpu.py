"""The meter bridge without a GPU: the CPU paths of dspi_meters_update / dspi_meters_alarms / dspi_status_all / dspi_clear_clips_list through the
C-ABI on host-only contexts and through a sanitized g++ driver (tests/meters_driver.cpp) against the model written from the header
(tests/meters_model.py); the update kernel's staging arithmetic walked on the CPU with every index checked; every refusal in its order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meters_model as M
from dspi_amd import host
from dspi_amd.host import Dspi, DspiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
STAGE = 64      # packets the update kernel stages in LDS at once (dspi_meters.h kMeterStagePackets)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """own main: built with AddressSanitizer and UBSan where this g++ has their runtimes (asked of an empty program), else plain; which build
    ran is printed"""
    tmp = tmp_path_factory.mktemp("meters")
    exe = tmp / "meters_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "meters_driver.cpp"), os.path.join(CSRC, "dspi_meters.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", "-o", str(tmp / "probe"), str(probe)] + san, capture_output=True).returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0
    subprocess.run(cmd + (san if have else []), check=True)
    print("meters_driver:", "AddressSanitizer + UBSan" if have else "UNSANITIZED (this g++ has no sanitizer runtimes)")
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_meters_update"), "libdspi_mi355x has no dspi_meters_update"


def run(driver, script):
    out = subprocess.run([driver], input="".join(l + "\n" for l in script), check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(script)
    return out


def hx(a):
    return np.ascontiguousarray(a).tobytes().hex() if a is not None and np.size(a) else "-"


def random_peaks(rng, S, K, Cn):
    """levels that rise, hold and fall: a slow envelope per (stream, channel) times noise, with exact zeros and full scale sprinkled in"""
    env = np.abs(np.sin(np.arange(K)[None, :, None] * rng.uniform(0.02, 0.6, (S, 1, Cn)) + rng.uniform(0, 6, (S, 1, Cn))))
    p = (env * rng.uniform(0.2, 1.0, (S, K, Cn)) * 65535).astype(np.uint16)
    p[rng.random((S, K, Cn)) < 0.05] = 0
    p[rng.random((S, K, Cn)) < 0.02] = 65535
    return p


def random_meters(rng, S, Cn):
    return (rng.integers(0, 65536, (S, Cn)).astype(np.uint32) | rng.integers(0, 40, (S, Cn)).astype(np.uint32) << 16).astype(np.uint32)


def test_symbols_header_and_makefile():
    L = host.lib()
    for name in ("dspi_meters_update", "dspi_meters_alarms", "dspi_status_all", "dspi_clear_clips_list"): assert hasattr(L, name), name
    assert L.dspi_abi_version() == 8
    with open(os.path.join(ROOT, "include", "dspi.h")) as f: text = f.read()
    for word in ("8 + the meter bridge: detect by symbol (dspi_meters_update;", "int dspi_meters_update(", "int dspi_meters_alarms(", "int dspi_status_all(", "int dspi_clear_clips_list(",
                 "update before changing pauses", "travel with a stream are not part of this interface"):
        assert word in text, word
    with open(os.path.join(CSRC, "Makefile")) as f: mk = f.read()
    assert "dspi_meters" in mk.split("HOST =")[1].split("\n")[0].split() and "dspi_meterbridge" in mk.split("KERNELS =")[1].split("\n")[0].split()
    with open(os.path.join(CSRC, "dspi_meters.h")) as f: assert f"kMeterStagePackets = {STAGE};" in f.read()


def test_the_vectorised_model_is_the_rule_written_out():
    rng = np.random.default_rng(3)
    for hold, decay in ((0, 0), (3, 30000), (65535, 1), (2, 32768), (1, 32767)):
        p = random_peaks(rng, 5, 40, 3)
        m0 = random_meters(rng, 5, 3)
        got = M.update(m0, p, hold, decay)
        for s in range(5):
            for c in range(3): assert int(got[s, c]) == M.update_scalar(int(m0[s, c]), p[s, :, c], hold, decay), (hold, decay, s, c)


# ---- the update -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_update_equals_the_model_with_state_carried_over_calls(flavor, driver):
    rng = np.random.default_rng(10 + flavor)
    S = 37
    d = Dspi(flavor, S, device=None)
    assert d.C == (11 if flavor else 7)
    meters, want = np.zeros((S, d.C), dtype=np.uint32), np.zeros((S, d.C), dtype=np.uint32)
    script, wants = [], []
    for K, hold, decay in ((7, 3, 31000), (1, 3, 31000), (50, 10, 32000), (13, 0, 16384), (9, 2, 32768)):
        p = random_peaks(rng, S, K, d.C)
        script.append(f"update {d.C} {S} {K} {hold} {decay} - {hx(meters)} {hx(p)}")
        d.meters_update_host(p, meters, hold, decay)
        want = M.update(want, p, hold, decay)
        wants.append(want)
        assert np.array_equal(meters, want), (K, hold, decay, np.argwhere(meters != want)[:3])
    assert (want >> 16).any() and (want & 0xffff).any()
    for line, w in zip(run(driver, script), wants): assert line == hx(w)
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_split_invariance(flavor):
    """one call over K packets equals calls over every split j | K - j, word for word"""
    rng = np.random.default_rng(20 + flavor)
    S, K = 5, 24
    d = Dspi(flavor, S, device=None)
    for hold, decay in ((4, 30000), (0, 0), (30, 32768)):
        p = random_peaks(rng, S, K, d.C)
        m0 = random_meters(rng, S, d.C)
        whole = d.meters_update_host(p, m0.copy(), hold, decay)
        assert np.array_equal(whole, M.update(m0, p, hold, decay))
        for j in range(1, K):
            m = m0.copy()
            d.meters_update_host(np.ascontiguousarray(p[:, :j]), m, hold, decay)
            d.meters_update_host(np.ascontiguousarray(p[:, j:]), m, hold, decay)
            assert np.array_equal(m, whole), (hold, decay, j)
    d.close()


@pytest.mark.parametrize("hold", (0, 65535))
@pytest.mark.parametrize("decay", (0, 1, 32767, 32768))
def test_corner_parameters(hold, decay):
    S, K = 3, 12
    d = Dspi(1, S, device=None)
    p = np.zeros((S, K, d.C), dtype=np.uint16)
    p[0, 0] = 65535                                  # full scale once, then silence
    p[1, :, :] = np.arange(K)[:, None] % 2 * 65535    # full scale and 0 in turn
    p[2, 3] = 40000; p[2, 4:] = 100                   # a burst over a floor
    m = d.meters_update_host(p, np.zeros((S, d.C), dtype=np.uint32), hold, decay)
    assert np.array_equal(m, M.update(np.zeros((S, d.C), dtype=np.uint32), p, hold, decay))
    level, count = m & 0xffff, m >> 16
    if hold == 65535:
        assert (level[0] == 65535).all() and (count[0] == 65535 - (K - 1)).all() and (level[2] == 40000).all() and (count[2] == 65535 - 8).all()
    else:
        assert (count == 0).all()
        # (K - 1 packets of silence behind the burst; a decay of 0 or 1 is down at once)
        assert (level[0] == {0: 0, 1: 0, 32767: M.update_scalar(0, [65535] + [0] * (K - 1), 0, 32767) & 0xffff, 32768: 65535}[decay]).all()
        assert (level[2] == {0: 100, 1: 100, 32767: max(100, M.update_scalar(0, [40000] + [100] * 8, 0, 32767) & 0xffff), 32768: 40000}[decay]).all()
    assert (level[1] == 65535).all(), "the last packet is at full scale"
    # a meter at rest under silence stays at rest; full scale everywhere pins it
    z = d.meters_update_host(np.zeros((S, K, d.C), dtype=np.uint16), np.zeros((S, d.C), dtype=np.uint32), hold, decay)
    assert np.array_equal(z & 0xffff, np.zeros((S, d.C))) and np.array_equal(z >> 16, np.full((S, d.C), hold))      # (0 >= 0: the hold is re-armed)
    f = d.meters_update_host(np.full((S, K, d.C), 65535, dtype=np.uint16), np.zeros((S, d.C), dtype=np.uint32), hold, decay)
    assert (f == (65535 | hold << 16)).all()
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_paused_streams_keep_their_words_and_alarms_still_list_them(flavor, driver):
    rng = np.random.default_rng(30 + flavor)
    S, K = 20, 9
    d = Dspi(flavor, S, device=None)
    d.pause_streams(1, 1); d.pause_streams(6, 5); d.pause_streams(S - 1, 1)
    active = d.streams_paused() == 0
    assert (~active).sum() == 7
    p = random_peaks(rng, S, K, d.C)
    m0 = random_meters(rng, S, d.C)
    m0[7] = 65535 | 9 << 16      # a paused stream above any level
    m = d.meters_update_host(p, m0.copy(), 3, 30000)
    want = M.update(m0, p, 3, 30000, active)
    assert np.array_equal(m, want) and np.array_equal(m[~active], m0[~active]) and not np.array_equal(m[active], m0[active])
    assert run(driver, [f"update {d.C} {S} {K} 3 30000 {hx(active.astype(np.uint8))} {hx(m0)} {hx(p)}"])[0] == hx(want)
    streams, info, total = d.meters_alarms_host(m, 65535)
    ws, wi, wt = M.alarms(m, np.zeros(S, dtype=np.uint16), 65535, S)
    assert streams.tolist() == ws.tolist() and info.tolist() == wi.tolist() and total == wt and 7 in streams.tolist()
    # the activity is the context's at the time of the call
    d.resume_streams(0, S)
    assert np.array_equal(d.meters_update_host(p, m0.copy(), 3, 30000), M.update(m0, p, 3, 30000))
    d.close()


# ---- the update kernel's staging arithmetic, on the CPU ---------------------------------------------------------------------------------------
def test_the_kernels_staging_walk_on_the_cpu(driver):
    """every global byte the kernel would load lies inside peaks and belongs to an active stream, every LDS index lies inside the array, every
    lane reads what was staged — at every alignment of `peaks`, with one piece (K <= 64) and with chunks (K > 64), ragged last workgroups,
    paused streams at the pieces' seams — and the words equal the model's"""
    rng = np.random.default_rng(40)
    script, wants = [], []
    for Cn, S, K in ((11, 1, 1), (11, 23, 50), (11, 24, 7), (11, 47, 64), (11, 30, 65), (11, 5, 130), (7, 1, 1), (7, 36, 50), (7, 37, 1), (7, 75, 64), (7, 40, 65), (7, 3, 200), (7, 73, 3)):
        p = random_peaks(rng, S, K, Cn)
        m0 = random_meters(rng, S, Cn)
        for lead in (0, 2, 8, 14) if K * S < 2000 else (0, 6):
            for paused in (None, "some"):
                active = None
                if paused:
                    active = rng.random(S) < 0.6
                    active[[0, S - 1]] = rng.random(2) < 0.5
                script.append(f"stage {Cn} {S} {K} 5 31000 {hx(active.astype(np.uint8)) if active is not None else '-'} {hx(m0)} {hx(p)} {lead}")
                wants.append(hx(M.update(m0, p, 5, 31000, active)))
    got = run(driver, script)
    for line, cmd, w in zip(got, script, wants): assert line == w, (cmd[:40], line[:80])


# ---- alarms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_alarm_lists(flavor, driver):
    rng = np.random.default_rng(50 + flavor)
    S = 150
    d = Dspi(flavor, S, device=None)
    m = random_meters(rng, S, d.C)
    m[::3] &= 0xffff0fff      # a third of the streams well below the level
    level = 0xf000
    zero = np.zeros(S, dtype=np.uint16)
    ws, wi, wt = M.alarms(m, zero, level, S)
    assert 10 < wt < S - 10
    for cap in (1, wt - 1, wt, wt + 1, S):
        streams, info, total = d.meters_alarms_host(m, level, cap)
        k = min(cap, wt)
        assert total == wt and streams.tolist() == ws[:k].tolist() and info.tolist() == wi[:k].tolist(), cap
        assert (np.diff(streams.astype(np.int64)) > 0).all() and (info >> 16 == 0).all() and (info != 0).all()
        s2, i2, t2 = d.meters_alarms_host(m, level, cap, want_info=False)
        assert i2 is None and t2 == wt and s2.tolist() == ws[:k].tolist()
    # info masks: exactly the channels at or above the level
    streams, info, _ = d.meters_alarms_host(m, level)
    for s, w in zip(streams, info): assert int(w) == sum(1 << c for c in range(d.C) if (int(m[s, c]) & 0xffff) >= level)
    # meters == NULL: clip-only alarms — none on a host-only context
    streams, info, total = d.meters_alarms_host(None, 0)
    assert total == 0 and len(streams) == 0
    # level 0 lists every stream
    streams, info, total = d.meters_alarms_host(m, 0)
    assert total == S and streams.tolist() == list(range(S)) and (info == (1 << d.C) - 1).all()
    streams, info, total = d.meters_alarms_host(m, 0, 7)
    assert total == S and streams.tolist() == list(range(7))
    # the scan with clip words (the words a device context brings down), through the driver
    clip = np.where(rng.random(S) < 0.1, rng.integers(1, 1 << 9, S), 0).astype(np.uint16)
    script, wants = [], []
    for mm, lv, cap, wi_ in ((m, level, S, 1), (m, level, 5, 1), (None, 0, S, 1), (None, 123, 3, 0), (m, 65535, S, 1), (m, 0, S + 5, 0)):
        script.append(f"alarms {d.C} {S} {lv} {cap} {wi_} {hx(mm)} {hx(clip)}")
        ws, wi, wt = M.alarms(mm, clip, lv, cap)
        wants.append(f"{len(ws)} {wt} {ws.tobytes().hex()}- {wi.tobytes().hex() if wi_ else ''}-")
    assert run(driver, script) == wants
    assert M.alarms(None, clip, 0, S)[2] == (clip != 0).sum() > 0
    d.close()


# ---- status blocks and the clear list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_status_all_on_a_host_only_context_equals_get_status(flavor, driver):
    S = 9
    d = Dspi(flavor, S, device=None)
    d.pause_streams(2, 3)
    n = 2 * d.C + 4
    assert n == (26 if flavor else 18)
    blocks = d.status_all()
    assert blocks.shape == (S, n)
    for s in range(S): assert blocks[s].tobytes() == d.status(s) == M.status_block([0] * d.C, 0)
    part = d.status_all(3, 4)
    assert part.shape == (4, n) and not part.any()
    # exactly count * n bytes are written
    buf = np.full(5 * n + 3, 0xEE, dtype=np.uint8)
    assert d.L.dspi_status_all(d.h, 1, 5, buf.ctypes.data, 5 * n, 0) == 5 and not buf[:5 * n].any() and (buf[5 * n:] == 0xEE).all()
    # the packing itself, on words that are not zero
    rng = np.random.default_rng(flavor)
    script, wants = [], []
    for _ in range(5):
        pk, clip = rng.integers(0, 65536, d.C).astype(np.uint16), int(rng.integers(0, 65536))
        script.append(f"pack {d.C} {clip} {hx(pk)}")
        wants.append(M.status_block(pk, clip).hex())
    assert run(driver, script) == wants
    d.close()


def test_clear_clips_list_on_a_host_only_context(driver):
    d = Dspi(1, 10, device=None)
    assert d.clear_clips_list([3, 3, 9, 0]) == 4 and d.clear_clips_list([]) == 0
    bad = np.array([1, 10, 2], dtype=np.uint32)
    assert d.L.dspi_clear_clips_list(d.h, bad.ctypes.data, 3) == host.E_INVAL and "entry 1" in d.L.dspi_last_error(d.h).decode()
    assert d.L.dspi_clear_clips_list(d.h, None, 3) == host.E_INVAL and d.L.dspi_clear_clips_list(None, bad.ctypes.data, 1) == host.E_INVAL
    with pytest.raises(DspiError): d.clear_clips_list([0xffffffff])
    assert run(driver, ["list 10 1 10 2", "list 10 9 0 9", "list 10", "list 1 0 0 1"]) == ["1", "3", "0", "2"]
    d.close()


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_update_refusals_in_their_order(flavor, driver):
    S, K = 6, 4
    d = Dspi(flavor, S, device=None)
    p = np.full((S, K, d.C), 999, dtype=np.uint16)
    m = np.full((S, d.C), 0x00030007, dtype=np.uint32)
    before = m.tobytes()
    pp, pm = p.ctypes.data, m.ctypes.data
    up = d.L.dspi_meters_update
    err = lambda: d.L.dspi_last_error(d.h).decode()
    assert up(None, pp, K, 1, 1, pm, 0) == host.E_INVAL
    # a NULL pointer comes first, then n_blocks, the ranges, the flag bits, the size, the alignment; NODEVICE last
    assert up(d.h, None, 0, 70000, 40000, pm, 0x80) == host.E_INVAL and "NULL" in err()
    assert up(d.h, pp, 0, 70000, 40000, None, 0x80) == host.E_INVAL and "NULL" in err()
    assert up(d.h, pp, 0, 70000, 40000, pm, 0x80) == host.E_INVAL and "n_blocks" in err()
    assert up(d.h, pp, K, 65536, 40000, pm, 0x80) == host.E_INVAL and "hold_packets" in err()
    assert up(d.h, pp, K, 65535, 32769, pm, 0x80) == host.E_INVAL and "decay_q15" in err()
    for flags in (0x80, 0x2, host.MEM_DEVICE | 0x20, 0x80000000):
        assert up(d.h, pp, 0xffffffff, 65535, 32768, pm + 2, flags) == host.E_INVAL and "flag" in err()
    # (a size that overflows takes a context of 2 * 10^8 streams: the rule itself, through the driver — before the alignment, behind the flags)
    got = run(driver, [f"why_update {0xffffffff} {d.C} {0xffffffff} 65535 32768 1 4098 4098", f"why_update {0xffffffff} {d.C} {0xffffffff} 65535 32768 3 4098 4098",
                       f"why_update {0xffffffff} {d.C} {2 ** 27} 65535 32768 1 4096 4096", f"why_update {0xffffffff} {d.C} {2 ** 27} 65535 32768 1 4096 4098",
                       f"why_update {0xffffffff} {d.C} {2 ** 27} 65535 32768 0 4097 4099"])
    assert "overflow" in got[0] and "flag" in got[1] and got[2] == "ok" and "4-byte" in got[3] and got[4] == "ok"
    assert up(d.h, pp + 2, K, 0, 0, pm, host.MEM_DEVICE) == host.E_INVAL and "4-byte" in err()
    assert up(d.h, pp, K, 0, 0, pm + 2, host.MEM_DEVICE) == host.E_INVAL and "4-byte" in err()
    assert up(d.h, pp, K, 0, 0, pm, host.MEM_DEVICE) == host.E_NODEVICE
    assert m.tobytes() == before, "a refused call writes nothing"
    # host memory needs no alignment, and the largest parameters are accepted
    assert up(d.h, pp, K, 65535, 32768, pm, 0) == 0 and (m == (999 | 65535 << 16)).all()
    with pytest.raises(DspiError) as e: d.meters_update_device(pp, K, pm, 1, 1)
    assert e.value.code == host.E_NODEVICE
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_alarms_refusals_in_their_order(flavor):
    S = 6
    d = Dspi(flavor, S, device=None)
    m = np.full((S, d.C), 50000, dtype=np.uint32)
    streams, info = np.full(S, 77, dtype=np.uint32), np.full(S, 77, dtype=np.uint32)
    total = np.full(1, 77, dtype=np.uint32)
    pm, ps, pi, pt = m.ctypes.data, streams.ctypes.data, info.ctypes.data, total.ctypes.data
    al = d.L.dspi_meters_alarms
    err = lambda: d.L.dspi_last_error(d.h).decode()
    assert al(None, pm, 1, ps, pi, S, pt, 0) == host.E_INVAL
    assert al(d.h, pm, 70000, None, pi, 0, pt, 0x80) == host.E_INVAL and "NULL" in err()
    assert al(d.h, pm, 70000, ps, pi, 0, None, 0x80) == host.E_INVAL and "NULL" in err()
    assert al(d.h, pm, 70000, ps, pi, 0, pt, 0x80) == host.E_INVAL and "cap" in err()
    assert al(d.h, pm, 65536, ps, pi, S, pt, 0x80) == host.E_INVAL and "level_q15" in err()
    for flags in (0x80, 0x2, host.MEM_DEVICE | 0x40): assert al(d.h, pm + 2, 65535, ps, pi, S, pt, flags) == host.E_INVAL and "flag" in err()
    for k in range(4):
        args = [pm, 1, ps, pi, S, pt, host.MEM_DEVICE]; args[(0, 2, 3, 5)[k]] += 2
        assert al(d.h, *args) == host.E_INVAL and "4-byte" in err(), k
    assert al(d.h, pm, 1, ps, pi, S, pt, host.MEM_DEVICE) == host.E_NODEVICE and al(d.h, None, 1, ps, None, S, pt, host.MEM_DEVICE) == host.E_NODEVICE
    assert (streams == 77).all() and (info == 77).all() and total[0] == 77, "a refused call writes nothing"
    assert al(d.h, pm, 65535, ps, None, S, pt, 0) == 0 and total[0] == 0
    assert al(d.h, pm, 50000, ps, pi, 4, pt, 0) == 4 and total[0] == S and streams.tolist() == [0, 1, 2, 3, 77, 77] and info.tolist() == [(1 << d.C) - 1] * 4 + [77, 77]
    d.close()


@pytest.mark.parametrize("flavor", (0, 1), ids=("q28", "f32"))
def test_status_all_refusals(flavor):
    S = 6
    d = Dspi(flavor, S, device=None)
    n = 2 * d.C + 4
    buf = np.full(S * n, 0xEE, dtype=np.uint8)
    pb = buf.ctypes.data
    st = d.L.dspi_status_all
    assert st(None, 0, S, pb, S * n, 0) == host.E_INVAL
    for args in ((0, S, None, S * n, 0), (0, 0, pb, S * n, 0), (0, S + 1, pb, (S + 1) * n, 0), (S, 1, pb, S * n, 0), (3, 4, pb, S * n, 0), (0xffffffff, 2, pb, S * n, 0),
                 (0, S, pb, S * n, 0x80), (0, S, pb, S * n, host.MEM_DEVICE | 0x2)):
        assert st(d.h, *args) == host.E_INVAL, args
    assert st(d.h, 0, S, pb, S * n - 1, 0) == host.E_SHORT and st(d.h, 2, 3, pb, 3 * n - 1, host.MEM_DEVICE) == host.E_SHORT
    assert st(d.h, 0, S, pb, S * n - 1, 0x80) == host.E_INVAL, "the flag bits come before the size"
    assert st(d.h, 0, S, pb, S * n, host.MEM_DEVICE) == host.E_NODEVICE
    assert (buf == 0xEE).all(), "a refused call writes nothing"
    assert st(d.h, 0, S, pb, S * n, 0) == S and not buf.any()
    d.close()
