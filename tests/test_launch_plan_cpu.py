"""The launch plan (dspi_amd/csrc/dspi_plan.cpp) on the CPU: seeded scenarios of both flavours go through plan_launches (driver:
tests/launch_plan_driver.cpp, built with g++), and every plan is held to the WgItem contract (dspi_amd/csrc/dspi_image.h):
every stream served exactly once, on its own image (or, per-lane values and paired presets, on images of one ImageSig); every list
sorted by row; latency items inside their part; the DSPI_F32_LAYOUT overrides respected.  The same driver runs plan_call on seeded
dspi_process calls, whose buffer sizes are held to the arrays dspi_amd/host.py process_host allocates (test_call_layout)."""
import math
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")

# dspi_plan.h Path, in its order: (name, latency shape or 0, paired)
PATHS = [("F32Packed", 0, False), ("F32Skew1", 1, False), ("F32Skew2", 2, False), ("F32Skew1PP", 1, True), ("F32Skew2PP", 2, True),
         ("F32PvBands", 0, False), ("F32PvShared", 0, False), ("F32OneStream", 0, False), ("F32PackedLev", 0, False), ("F32Skew3", 3, False),
         ("F32Skew3PP", 3, True), ("F32PvBandsLev", 0, False), ("F32PvSharedLev", 0, False), ("Q28Uniform", 0, False), ("Q28PerLane", 0, False)]
PART_SHIFT = 26          # kSkPartShift
LEVELLER_ON, SUB_ACTIVE = 1 << 1, 1 << 4
N_SCENARIOS = 320


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "launch_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "launch_plan_driver.cpp"),
                    os.path.join(CSRC, "dspi_plan.cpp")], check=True)
    return str(exe)


def scenario(seed):
    """One context: flavour, stream count, stream -> image map, per-image structure / filters, CU count, the two switches."""
    r = random.Random(seed)
    flavor = r.choice((0, 1, 1))
    n = r.choice((1, 2, 3, r.randrange(1, 300), r.randrange(1, 300), r.randrange(300, 3000)))
    kind = r.choice(("shared", "own", "blocks", "random", "sprinkle"))
    if kind == "shared": si = [0] * n
    elif kind == "own": si = list(range(n))
    elif kind == "blocks":
        b, wrap = r.randrange(1, 200), r.choice((None, 2, 3, 7))
        si = [(s // b) % wrap if wrap else s // b for s in range(n)]
    elif kind == "random":
        k = r.randrange(1, 9)
        si = [r.randrange(k) for _ in range(n)]
    else:
        si = [r.randrange(1, 5) if r.random() < 0.05 else 0 for _ in range(n)]
    n_images = max(si) + 1 + (1 if r.random() < 0.1 else 0)      # (sometimes an image no stream uses)
    # a few structures per context, so that rows and workgroups share an ImageSig; filters mostly follow the band hash, sometimes not
    lev_p = r.choice((0.0, 0.0, 0.3, 1.0))
    structures = []
    for _ in range(r.randrange(1, 4)):
        flags = (LEVELLER_ON if r.random() < lev_p else 0) | (SUB_ACTIVE if r.random() < 0.5 else 0)
        out_enabled = r.choice((0, 0, 1, 0x1ff))
        structures.append((flags, out_enabled, r.choice((0, 0, 1)), r.choice((0, 0, 4)), r.randrange(2)))
    images, n_bands = [], r.choice((1, 1, 3))
    for _ in range(n_images):
        band = r.randrange(n_bands)
        images.append(r.choice(structures) + (band, band if r.random() < 0.8 else band + 10))
    return dict(flavor=flavor, n=n, si=si, images=images, cus=r.choice((1, 2, 4, 8, 32, 256)), layout=r.choice((0, 0, 0, 1, 2)),
                paired=r.choice((0, 1, 1)))


def render(sc):
    out = [f"{sc['flavor']} {sc['n']} {len(sc['images'])} {sc['cus']} {sc['layout']} {sc['paired']}", " ".join(map(str, sc["si"]))]
    out += [" ".join(map(str, im)) for im in sc["images"]]
    return "\n".join(out) + "\n"


def parse(text):
    plans, cur, lines = [], None, iter(text.splitlines())
    for line in lines:
        f = line.split()
        if f[0] == "R": cur = dict(row_pv=[int(x) for x in f[1:]], items={})
        elif f[0] == "P":
            cur["items"][PATHS[int(f[1])][0]] = [tuple(int(x) for x in next(lines).split()) for _ in range(int(f[2]))]
        elif f[0] == "E": plans.append(cur)
    return plans


def skew_class(im):
    flags, out_enabled, out_mute, ch_bypassed = im[0], im[1], im[2], im[3]
    if flags & LEVELLER_ON: return 3
    for o in range(9):
        processed = o != 8 or bool(flags & SUB_ACTIVE)
        if processed and (out_enabled >> o) & 1 and not (out_mute >> o) & 1 and not (ch_bypassed >> (2 + o)) & 1: return 2
    return 1


def check(sc, plan):
    """The WgItem contract (dspi_image.h), path by path."""
    flavor, n, si, images = sc["flavor"], sc["n"], sc["si"], sc["images"]
    sig = lambda i: images[i][:5]      # ImageSig of the driver: flags, out_enabled, out_mute, ch_bypassed, variant
    row = 128 if flavor else 64
    served = [0] * n

    def serve(wg, lane, comp, on=None):
        s = wg * row + (2 * lane + comp if flavor else lane)
        assert s < n, f"stream {s} past the end"
        served[s] += 1
        if on is not None: assert on(si[s]), f"stream {s} on image {si[s]}"

    bits = lambda m, lo=0, hi=64: [l for l in range(lo, hi) if (m >> l) & 1]
    for name, items in plan["items"].items():
        shape, paired = next((sh, pp) for nm, sh, pp in PATHS if nm == name)
        assert name.startswith("F32" if flavor else "Q28"), name
        assert [it[0] for it in items] == sorted(it[0] for it in items), f"{name} not sorted by row"      # (b)
        for wg, image, m0, m1 in items:
            if name.startswith("F32Packed"):
                assert m1 == m0 and bool(skew_class(images[image]) == 3) == name.endswith("Lev")
                for l in bits(m0): serve(wg, l, 0, lambda i: i == image); serve(wg, l, 1, lambda i: i == image)
            elif name.startswith("F32Pv"):
                assert m1 == 0 and plan["row_pv"][wg] == (1 if "Bands" in name else 2)
                for l in bits(m0):
                    serve(wg, l, 0, lambda i: sig(i) == sig(image)); serve(wg, l, 1, lambda i: sig(i) == sig(image))
            elif name == "F32OneStream":
                assert image in (0, 1) and m1 == 0
                for l in bits(m0): serve(wg, l, image)
            elif shape:
                part, img = image >> PART_SHIFT, image & ((1 << PART_SHIFT) - 1)
                ppw = 8 if shape == 1 else 2
                assert part < 64 // ppw and (m0 | m1) >> (part * ppw) & ((1 << ppw) - 1), f"{name}: part {part} without lanes"      # (c)
                assert skew_class(images[img]) == shape
                same = (lambda i: sig(i) == sig(img)) if paired else (lambda i: i == img)                                         # (d)
                for l in bits(m0, part * ppw, part * ppw + ppw): serve(wg, l, 0, same)
                for l in bits(m1, part * ppw, part * ppw + ppw): serve(wg, l, 1, same)
            elif name == "Q28Uniform":
                assert m1 == 0
                for l in bits(m0): serve(wg, l, 0, lambda i: i == image)
            else:
                assert name == "Q28PerLane" and image == 0 and m1 == 0
                for l in bits(m0): serve(wg, l, 0)
    bad = [s for s in range(n) if served[s] != 1]
    assert not bad, f"streams served other than once: {[(s, served[s]) for s in bad[:8]]}"                                        # (a)
    latency = [nm for nm, sh, _ in PATHS if sh and plan["items"].get(nm)]
    if sc["layout"] == 2: assert not latency                                                                                          # (e)
    if sc["layout"] == 1 and flavor: assert set(plan["items"]) == set(latency)


def test_launch_plan_contract(driver):
    scs = [scenario(seed) for seed in range(N_SCENARIOS)]
    out = subprocess.run([driver], input="".join(map(render, scs)), capture_output=True, text=True, check=True, timeout=300).stdout
    plans = parse(out)
    assert len(plans) == len(scs)
    seen = set()
    for seed, (sc, plan) in enumerate(zip(scs, plans)):
        try:
            check(sc, plan)
        except AssertionError as e:
            raise AssertionError(f"scenario seed {seed} (flavour {sc['flavor']}, {sc['n']} streams): {e}") from None
        seen |= {nm for nm, items in plan["items"].items() if items}
    # the scenarios reach every path
    assert seen == {nm for nm, _, _ in PATHS}, sorted({nm for nm, _, _ in PATHS} - seen)


# ---- the layout of one dspi_process call (plan_call), held to the buffers host.py process_host allocates for the same call ----
STATE_MAP = {0: dict(C=7, P=2, R=64), 1: dict(C=11, P=4, R=128)}      # channels, output pairs, streams per row (dspi_image.h make_state_map)
MEM_DEVICE, OUT_TILED, OUT_ENABLED_ONLY, OUT_I2S_SLOTS, OUT_SPDIF, OUT_CLIP_FLAGS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20      # include/dspi.h
ACCEPTED_FLAGS = [f for f in range(64) if not (f & OUT_SPDIF and f & (OUT_TILED | OUT_I2S_SLOTS))]
DEVICE, DIRECT, STAGED = 0, 1, 2
MIB, GIB = 1 << 20, 1 << 30
N_CALLS = 800
BUFFERS = ("pcm", "pairs", "sub", "peaks", "clip")


def call(seed):
    r = random.Random(seed)
    flavor = r.choice((0, 1))
    n = r.choice((1, 2, r.randrange(1, 300), r.randrange(300, 3000), r.randrange(3000, 70000), r.choice((65536, 65537, 65600))))
    n_blocks = r.choice((1, 1, 2, r.randrange(1, 20), r.randrange(1, 2001)))
    block_len = r.choice((1, 48, 96, 192, r.randrange(1, 193)))
    flags = ACCEPTED_FLAGS[seed % len(ACCEPTED_FLAGS)]          # every combination dspi_process accepts, N_CALLS / 40 times each
    passed = dict(pcm=True, pairs=r.random() < 0.7, sub=r.random() < 0.6, peaks=r.random() < 0.6,
                  clip=bool(flags & OUT_CLIP_FLAGS) and r.random() < 0.8)
    return dict(flavor=flavor, n=n, n_blocks=n_blocks, block_len=block_len, bit_depth=r.choice((16, 24)), flags=flags, passed=passed,
                no_direct=r.random() < 0.3, all_latency=flavor == 1 and r.random() < 0.4)


def render_call(c):
    sm, O = STATE_MAP[c["flavor"]], 9 if c["flavor"] else 5
    n_wg = -(-c["n"] // sm["R"])
    p = c["passed"]
    f = (c["n"], n_wg, sm["R"], sm["C"], O, sm["P"], c["n_blocks"], c["block_len"], c["bit_depth"], c["flags"],
         p["pairs"], p["sub"], p["peaks"], p["clip"], c["no_direct"], c["all_latency"])
    return "C " + " ".join(str(int(x)) for x in f) + "\n"


def parse_call(line):
    f = line.split()
    assert f[0] == "L", line
    v = [int(x) for x in f[1:]]
    lay = dict(zip(("frames", "mem", "two_pass", "two_pass_rows", "two_pass_bytes", "direct_bytes", "n_chunks", "rows_per_chunk"), v[:8]))
    for k, name in enumerate(BUFFERS):
        lay[name] = dict(zip(("bytes", "per", "tile_cols", "off"), v[8 + 4 * k:12 + 4 * k]))
    return lay


def host_buffers(c):
    """(shape, item size, tile columns?) of each buffer, as process_host (dspi_amd/host.py) allocates them for this call."""
    sm = STATE_MAP[c["flavor"]]
    S, F, R, P, C = c["n"], c["n_blocks"] * c["block_len"], sm["R"], sm["P"], sm["C"]
    nt, tiled = -(-S // R), bool(c["flags"] & OUT_TILED)
    if tiled: pairs, sub = ((nt, 2 * P, F, R), 4, True), ((nt, F, R), 4, True)
    else: pairs, sub = ((S, P, F, 4) if c["flags"] & OUT_SPDIF else (S, P, F, 2), 4, False), ((S, F), 4, False)
    return dict(pcm=((S, F, 6 if c["bit_depth"] == 24 else 4), 1, False), pairs=pairs, sub=sub, peaks=((S, c["n_blocks"], C), 2, False),
                clip=((S,), 2, False))


def check_call(c, lay):
    sm = STATE_MAP[c["flavor"]]
    S, R, F, flags = c["n"], sm["R"], c["n_blocks"] * c["block_len"], c["flags"]
    n_wg = -(-S // R)
    assert lay["frames"] == F
    want = {}
    for name, (shape, item, tile_cols) in host_buffers(c).items():
        b, full = lay[name], math.prod(shape) * item
        want[name] = full if c["passed"][name] else 0
        assert b["bytes"] == want[name], f"{name}: {b['bytes']} bytes, process_host allocates {want[name]}"
        assert bool(b["tile_cols"]) == tile_cols and b["per"] * (n_wg * R if tile_cols else S) == full, f"{name}: {b}"
    # the memory path
    if flags & MEM_DEVICE: assert lay["mem"] == DEVICE
    else: assert lay["mem"] == (DIRECT if not c["no_direct"] and lay["direct_bytes"] <= 2 * MIB else STAGED)
    # the direct area: 256-byte aligned regions in buffer order, each holding its buffer, nothing but alignment between them
    offs = [lay[nm]["off"] for nm in BUFFERS]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs + [lay["direct_bytes"]])
    for k, nm in enumerate(BUFFERS):
        end = offs[k + 1] if k + 1 < len(BUFFERS) else lay["direct_bytes"]
        assert offs[k] + want[nm] <= end < offs[k] + want[nm] + 256, f"direct area: {nm} at {offs[k]}, {want[nm]} bytes, next at {end}"
    # the staged chunks: they partition the rows, and each output's pieces of consecutive chunks are consecutive and cover it
    moved = sum(want[nm] for nm in ("pcm", "pairs", "sub", "peaks"))
    k, rp = lay["n_chunks"], lay["rows_per_chunk"]
    assert 1 <= k <= 8 and (k > 1) == (moved >= 32 * MIB and n_wg >= 2), (k, moved, n_wg)
    chunks = [(i * rp, min(n_wg, (i + 1) * rp)) for i in range(k)]
    assert chunks[0][0] == 0 and chunks[-1][1] == n_wg and all(r0 < r1 for r0, r1 in chunks)
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    for nm in ("pcm", "pairs", "sub", "peaks"):
        b, at = lay[nm], 0
        for r0, r1 in chunks:
            u0, u1 = r0 * R, r1 * R if b["tile_cols"] else min(r1 * R, S)
            assert u0 * b["per"] == at
            at = u1 * b["per"]
        assert at == host_buffers(c)[nm][1] * math.prod(host_buffers(c)[nm][0])
    # two-pass S/PDIF: only with S/PDIF, pairs and a plan that is not all on the latency layout; its scratch holds whole rows of pair words
    assert bool(lay["two_pass"]) == (bool(flags & OUT_SPDIF) and c["passed"]["pairs"] and not c["all_latency"])
    if lay["two_pass"]:
        row_b = R * sm["P"] * F * 2 * 4          # the int32 pair words (R, P, F, 2) of one row
        assert 1 <= lay["two_pass_rows"] <= n_wg and lay["two_pass_bytes"] == lay["two_pass_rows"] * row_b
        assert lay["two_pass_bytes"] <= max(2 * GIB, row_b)
    else:
        assert lay["two_pass_rows"] == 0 and lay["two_pass_bytes"] == 0


def test_call_layout(driver):
    calls = [call(seed) for seed in range(N_CALLS)]
    out = subprocess.run([driver], input="".join(map(render_call, calls)), capture_output=True, text=True, check=True, timeout=300).stdout
    lays = [parse_call(line) for line in out.splitlines()]
    assert len(lays) == len(calls)
    reached = set()
    for seed, (c, lay) in enumerate(zip(calls, lays)):
        try:
            check_call(c, lay)
        except AssertionError as e:
            raise AssertionError(f"call seed {seed} ({c}): {e}") from None
        n_wg = -(-c["n"] // STATE_MAP[c["flavor"]]["R"])
        reached |= {("mem", lay["mem"]), ("chunks", min(lay["n_chunks"], 3)), ("flavour", c["flavor"])}
        if lay["two_pass"]: reached.add(("two_pass_rows", "some" if lay["two_pass_rows"] < n_wg else "all"))
        if lay["mem"] == DIRECT and c["n"] % STATE_MAP[c["flavor"]]["R"]: reached.add("direct, partial last row")
    # the calls reach every memory path, one / two / more chunks, both kinds of two-pass row counts
    assert reached >= {("mem", DEVICE), ("mem", DIRECT), ("mem", STAGED), ("chunks", 1), ("chunks", 2), ("chunks", 3), ("flavour", 0), ("flavour", 1),
                       ("two_pass_rows", "some"), ("two_pass_rows", "all"), "direct, partial last row"}, reached
