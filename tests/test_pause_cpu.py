"""Paused streams without a GPU (dspi_pause_streams / dspi_resume_streams / dspi_streams_paused, include/dspi.h): the launch plan built
from an activity vector (dspi_amd/csrc/dspi_plan.cpp, PlanInput::active) held to the WgItem contract over the seeded scenarios of
test_launch_plan_cpu.py, each under several activity patterns; the plan with nothing paused against the plan without the field, textually;
the activity-aware target rule of the resume (dspi_amd/csrc/dspi_snapshot.h snap_row_target_active) against a model written from the
header's words; and the three calls on host-only contexts.  Driver: tests/pause_plan_driver.cpp, built with g++."""
import os
import random
import subprocess

import numpy as np
import pytest

from dspi_amd import host
from dspi_amd.host import Dspi, DspiError
from test_launch_plan_cpu import N_SCENARIOS, PART_SHIFT, PATHS, parse, render, scenario, skew_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
PATTERNS = ("nothing", "everything", "whole-rows", "even-streams", "odd-streams", "whole-lanes", "last-stream", "random", "few-active")


def build(tmp, name, *sources):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), *sources], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pause"), "pause_plan_driver", os.path.join(ROOT, "tests", "pause_plan_driver.cpp"), os.path.join(CSRC, "dspi_plan.cpp"))


@pytest.fixture(scope="module")
def plain_driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pause_plain"), "launch_plan_driver", os.path.join(ROOT, "tests", "launch_plan_driver.cpp"), os.path.join(CSRC, "dspi_plan.cpp"))


def test_the_library_exports_the_new_symbols():
    L = host.lib()
    assert hasattr(L, "dspi_pause_streams") and hasattr(L, "dspi_resume_streams") and hasattr(L, "dspi_streams_paused")
    assert host.RESUME_AS_IS == 0x1


def activity(sc, kind, r):
    """1 = active, per stream"""
    n, row = sc["n"], 128 if sc["flavor"] else 64
    a = [1] * n
    if kind == "everything": a = [0] * n
    elif kind == "whole-rows":
        for wg in range(-(-n // row)):
            if r.random() < 0.5: a[wg * row:(wg + 1) * row] = [0] * len(a[wg * row:(wg + 1) * row])
    elif kind == "even-streams": a = [s & 1 for s in range(n)]
    elif kind == "odd-streams": a = [1 - (s & 1) for s in range(n)]
    elif kind == "whole-lanes":      # both streams of some float lanes (Q28: pairs of neighbouring lanes)
        for l in range(-(-n // 2)):
            if r.random() < 0.4: a[2 * l:2 * l + 2] = [0] * len(a[2 * l:2 * l + 2])
    elif kind == "last-stream": a[n - 1] = 0
    elif kind == "random":
        p = r.choice((0.05, 0.5, 0.95))
        a = [0 if r.random() < p else 1 for _ in range(n)]
    elif kind == "few-active":
        a = [0] * n
        for s in r.sample(range(n), min(n, 16)): a[s] = 1
    return a


def render_with(sc, act):
    return render(sc) + ("0\n" if act is None else f"{sc['n']} " + " ".join(map(str, act)) + "\n")


def check(sc, plan, act):
    """The WgItem contract (dspi_image.h) for the ACTIVE streams: each served exactly once, on its own image or (per-lane values, paired presets)
    an image of its ImageSig; no paused stream's bit in any mask; rows without an active stream in no list; lists sorted; latency items
    inside their part."""
    flavor, n, si, images = sc["flavor"], sc["n"], sc["si"], sc["images"]
    sig = lambda i: images[i][:5]
    row = 128 if flavor else 64
    served = [0] * n
    live_rows = {s // row for s in range(n) if act[s]}

    def stream_of(wg, lane, comp): return wg * row + (2 * lane + comp if flavor else lane)

    def serve(wg, lane, comp, on=None):
        s = stream_of(wg, lane, comp)
        assert s < n, f"stream {s} past the end"
        served[s] += 1
        if on is not None: assert on(si[s]), f"stream {s} on image {si[s]}"

    def no_paused_bits(wg, m, comp):      # every bit of a mask, read by the kernel or not (the size rule's items carry their whole row's)
        for l in bits(m):
            s = stream_of(wg, l, comp)
            assert s < n and act[s], f"mask bit of {'paused' if s < n else 'missing'} stream {s}"

    bits = lambda m, lo=0, hi=64: [l for l in range(lo, hi) if (m >> l) & 1]
    for name, items in plan["items"].items():
        shape, paired = next((sh, pp) for nm, sh, pp in PATHS if nm == name)
        assert name.startswith("F32" if flavor else "Q28"), name
        assert [it[0] for it in items] == sorted(it[0] for it in items), f"{name} not sorted by row"
        for wg, image, m0, m1 in items:
            assert wg in live_rows, f"{name}: row {wg} holds no active stream"
            assert m0 | m1, f"{name}: an item without lanes in row {wg}"
            if name.startswith("F32Packed"):
                assert m1 == m0 and bool(skew_class(images[image]) == 3) == name.endswith("Lev")
                no_paused_bits(wg, m0, 0); no_paused_bits(wg, m0, 1)
                for l in bits(m0): serve(wg, l, 0, lambda i: i == image); serve(wg, l, 1, lambda i: i == image)
            elif name.startswith("F32Pv"):
                assert m1 == 0 and plan["row_pv"][wg] == (1 if "Bands" in name else 2)
                no_paused_bits(wg, m0, 0); no_paused_bits(wg, m0, 1)
                for l in bits(m0):
                    serve(wg, l, 0, lambda i: sig(i) == sig(image)); serve(wg, l, 1, lambda i: sig(i) == sig(image))
            elif name == "F32OneStream":
                assert image in (0, 1) and m1 == 0
                no_paused_bits(wg, m0, image)
                for l in bits(m0): serve(wg, l, image)
            elif shape:
                part, img = image >> PART_SHIFT, image & ((1 << PART_SHIFT) - 1)
                ppw = 8 if shape == 1 else 2
                assert part < 64 // ppw and (m0 | m1) >> (part * ppw) & ((1 << ppw) - 1), f"{name}: part {part} without lanes"
                assert skew_class(images[img]) == shape
                no_paused_bits(wg, m0, 0); no_paused_bits(wg, m1, 1)
                same = (lambda i: sig(i) == sig(img)) if paired else (lambda i: i == img)
                for l in bits(m0, part * ppw, part * ppw + ppw): serve(wg, l, 0, same)
                for l in bits(m1, part * ppw, part * ppw + ppw): serve(wg, l, 1, same)
            elif name == "Q28Uniform":
                assert m1 == 0
                no_paused_bits(wg, m0, 0)
                for l in bits(m0): serve(wg, l, 0, lambda i: i == image)
            else:
                assert name == "Q28PerLane" and image == 0 and m1 == 0
                no_paused_bits(wg, m0, 0)
                for l in bits(m0): serve(wg, l, 0)
    bad = [s for s in range(n) if served[s] != (1 if act[s] else 0)]
    assert not bad, f"streams served other than once (active) / never (paused): {[(s, act[s], served[s]) for s in bad[:8]]}"
    latency = [nm for nm, sh, _ in PATHS if sh and plan["items"].get(nm)]
    if sc["layout"] == 2: assert not latency
    if sc["layout"] == 1 and flavor: assert set(plan["items"]) == set(latency)
    if not any(act): assert not plan["items"], "everything paused: no list holds an item"


def test_plan_contract_with_paused_streams(driver):
    """the 320 seeded scenarios, each under three activity patterns (the kinds rotate with the seed, so every kind meets every kind of scenario)"""
    cases = []
    for seed in range(N_SCENARIOS):
        sc = scenario(seed)
        r = random.Random(9000 + seed)
        for k in range(3):
            kind = PATTERNS[(seed + 3 * k + seed // len(PATTERNS)) % len(PATTERNS)]
            cases.append((seed, kind, sc, activity(sc, kind, r)))
    out = subprocess.run([driver], input="".join(render_with(sc, act) for _, _, sc, act in cases), capture_output=True, text=True, check=True, timeout=600).stdout
    plans = parse(out)
    assert len(plans) == len(cases)
    seen, kinds, shapes = set(), set(), set()
    for (seed, kind, sc, act), plan in zip(cases, plans):
        try:
            check(sc, plan, act)
        except AssertionError as e:
            raise AssertionError(f"scenario seed {seed}, pattern {kind} (flavour {sc['flavor']}, {sc['n']} streams): {e}") from None
        seen |= {nm for nm, items in plan["items"].items() if items}
        kinds.add(kind)
        n, row = sc["n"], 128 if sc["flavor"] else 64
        if any(not any(act[w * row:(w + 1) * row]) for w in range(-(-n // row))) and any(act): shapes.add("a whole row paused beside active rows")
        if sc["flavor"] and any(act[2 * l] != act[2 * l + 1] for l in range(n // 2)): shapes.add("one stream of a lane")
        if sc["flavor"] and any(not act[2 * l] and not act[2 * l + 1] for l in range(n // 2)) and any(act): shapes.add("both streams of a lane")
        if sc["flavor"] and n & 1 and not act[n - 1] and any(act): shapes.add("the odd last stream")
    assert kinds == set(PATTERNS)
    assert shapes == {"a whole row paused beside active rows", "one stream of a lane", "both streams of a lane", "the odd last stream"}, shapes
    assert seen == {nm for nm, _, _ in PATHS}, sorted({nm for nm, _, _ in PATHS} - seen)      # every path is still reached with streams paused


def test_a_half_paused_lane_goes_to_the_one_stream_kernel(driver):
    """256 float streams on one image, packed layout: stream 5 paused -> lane 2 of row 0 leaves the packed item and its first stream (4) is a
    one-stream item of component 0; row 1 paused whole -> it is in no list."""
    sc = dict(flavor=1, n=256, si=[0] * 256, images=[(0, 0x1ff, 0, 0, 0, 0, 0)], cus=256, layout=2, paired=1)
    act = [1] * 256
    act[5] = 0
    act[128:] = [0] * 128
    plan = parse(subprocess.run([driver], input=render_with(sc, act), capture_output=True, text=True, check=True).stdout)[0]
    full = (1 << 64) - 1
    assert plan["items"] == {"F32Packed": [(0, 0, full & ~(1 << 2), full & ~(1 << 2))], "F32OneStream": [(0, 0, 1 << 2, 0)]}, plan["items"]


def test_few_active_streams_take_the_latency_layout(driver):
    """2 048 float streams on one preset, a device of 64 compute units (the latency layout's limit for this preset class: 4 stream pairs per
    unit): the packed kernel; paused down to 16 active streams the size rule sees 16 streams and moves them to the latency layout"""
    sc = dict(flavor=1, n=2048, si=[0] * 2048, images=[(0, 0x1ff, 0, 0, 0, 0, 0)], cus=64, layout=0, paired=1)
    act = [0] * 2048
    for s in range(0, 2048, 128): act[s] = 1
    both = parse(subprocess.run([driver], input=render_with(sc, None) + render_with(sc, act), capture_output=True, text=True, check=True).stdout)
    assert set(both[0]["items"]) == {"F32Packed"} and len(both[0]["items"]["F32Packed"]) == 16
    assert set(both[1]["items"]) == {"F32Skew2"} and len(both[1]["items"]["F32Skew2"]) == 16, both[1]["items"]
    check(sc, both[1], act)


def test_nothing_paused_is_the_plan_without_the_field(driver, plain_driver):
    """field left empty, and an all-active vector: both print what tests/launch_plan_driver.cpp (which does not know the field) prints"""
    scs = [scenario(seed) for seed in range(N_SCENARIOS)]
    plain = subprocess.run([plain_driver], input="".join(map(render, scs)), capture_output=True, text=True, check=True, timeout=300).stdout
    empty = subprocess.run([driver], input="".join(render_with(sc, None) for sc in scs), capture_output=True, text=True, check=True, timeout=300).stdout
    ones = subprocess.run([driver], input="".join(render_with(sc, [1] * sc["n"]) for sc in scs), capture_output=True, text=True, check=True, timeout=300).stdout
    assert plain.count("E\n") == N_SCENARIOS
    assert empty == plain
    assert ones == plain


# ---- the resume's target rule ----
def model_target(R, n, first, count, act, row):
    """include/dspi.h, "resume": the row's lowest-numbered stream below n that was active before the call; else the first stream of the range
    that the call actually resumes (it was paused) and that lies in the row"""
    r0, r1 = row * R, min(row * R + R, n)
    for s in range(r0, r1):
        if act[s]: return s, True
    for s in range(max(r0, first), min(r1, first + count)):
        if not act[s]: return s, False
    return None


def run_target(driver, R, n, first, count, act):
    out = {}
    for ln in subprocess.run([driver, "target", str(R), str(n), str(first), str(count), "".join(map(str, act))], check=True, capture_output=True, text=True).stdout.splitlines():
        w = ln.split()
        out[int(w[1])] = ((int(w[3]), bool(int(w[5]))), (int(w[7]), bool(int(w[8]))))
    return out


@pytest.mark.parametrize("R", [64, 128])
def test_target_rule_against_the_model(driver, R):
    r = random.Random(77 + R)
    rows_with_target = fallbacks = paused_first = 0
    for _ in range(600):
        n = r.choice((1, 2, R - 1, R, R + 1, 3 * R + 17, 5 * R))
        first = r.randrange(n)
        count = r.randrange(1, n - first + 1)
        kind = r.choice(("random", "rows", "sparse", "dense"))
        if kind == "random": act = [r.randrange(2) for _ in range(n)]
        elif kind == "rows": act = [(s // R) & 1 for s in range(n)]
        elif kind == "sparse": act = [1 if r.random() < 0.02 else 0 for _ in range(n)]
        else: act = [0 if r.random() < 0.02 else 1 for _ in range(n)]
        got = run_target(driver, R, n, first, count, act)
        assert set(got) == set(range(first // R, (first + count - 1) // R + 1))
        for row, (t, _) in got.items():
            resumed = [s for s in range(max(row * R, first), min(row * R + R, n, first + count)) if not act[s]]
            if not resumed: continue      # (the call moves nobody in this row: its target is never read)
            want = model_target(R, n, first, count, act, row)
            assert t == want, (R, n, first, count, row, t, want)
            rows_with_target += 1
            fallbacks += 0 if t[1] else 1
            paused_first += 1 if not act[row * R] and t[1] else 0
    assert rows_with_target > 300 and fallbacks > 20 and paused_first > 20      # (the row's first stream itself still paused: the next active one)


@pytest.mark.parametrize("R", [64, 128])
def test_target_rule_agrees_with_the_plain_rule_for_a_fully_resumed_range(driver, R):
    """every stream outside the range active, every stream inside paused (the call resumes its whole range): snap_row_target's answer"""
    r = random.Random(5 + R)
    for _ in range(200):
        n = r.choice((1, R, R + 1, 4 * R + 9))
        first = r.randrange(n)
        count = r.randrange(1, n - first + 1)
        act = [0 if first <= s < first + count else 1 for s in range(n)]
        for row, (t, plain) in run_target(driver, R, n, first, count, act).items():
            assert t == plain, (R, n, first, count, row, t, plain)


# ---- the calls on a host-only context ----
@pytest.mark.parametrize("flavor", [0, 1])
def test_host_only_context(flavor):
    d = Dspi(flavor, 300, device=None)
    L = d.L
    assert not d.streams_paused().any() and L.dspi_streams_paused(d.h, 0, 300, None) == 0
    assert d.pause_streams(10, 5) == 5
    assert d.pause_streams(12, 10) == 10                 # (pausing a paused stream: a no-op for that stream)
    want = np.zeros(300, dtype=np.uint8); want[10:22] = 1
    assert np.array_equal(d.streams_paused(), want) and L.dspi_streams_paused(d.h, 0, 300, None) == 12
    assert np.array_equal(d.streams_paused(8, 6), want[8:14]) and L.dspi_streams_paused(d.h, 20, 280, None) == 2
    assert d.resume_streams(0, 12) == 12                 # (resuming active streams likewise)
    want[10:12] = 0
    assert np.array_equal(d.streams_paused(), want)
    assert d.resume_streams(15, 3, as_is=True) == 3
    want[15:18] = 0
    assert np.array_equal(d.streams_paused(), want)
    # refusals change nothing
    for first, count in ((0, 0), (300, 1), (299, 2), (0, 301), (0xFFFFFFFF, 2)):
        assert L.dspi_pause_streams(d.h, first, count) == host.E_INVAL and b"range" in L.dspi_last_error(d.h), (first, count)
        assert L.dspi_resume_streams(d.h, first, count, 0) == host.E_INVAL and b"range" in L.dspi_last_error(d.h), (first, count)
        assert L.dspi_streams_paused(d.h, first, count, None) == host.E_INVAL
    for bad in (0x2, 0x3, 0x100, 0x80000000):
        assert L.dspi_resume_streams(d.h, 0, 300, bad) == host.E_INVAL and b"flag bits" in L.dspi_last_error(d.h), hex(bad)
    with pytest.raises(DspiError) as e: d.pause_streams(299, 2)
    assert e.value.code == host.E_INVAL
    assert np.array_equal(d.streams_paused(), want)
    # parameter calls reach paused streams, and activity is not a parameter: no image is made for it
    assert d.image_count() == 1
    d.set_volume(-3 * 256, stream=13)
    assert d.image_count() == 2
    assert d.resume_streams(0, 300) == 300 and not d.streams_paused().any()
    assert d.pause_streams(0, 300) == 300 and d.streams_paused().all()
    d.close()
