"""The lifecycle fuzz without a GPU (tests/lifecycle_model.py): what the default seeds of tests/test_gpu_lifecycle_fuzz.py::test_fuzz contain,
counted from the op lists alone by a reader of its own (crossings() below follows the streams through moves, boots and imports with tags,
independently of how the generator strings its ops together), and the same generator on host-only contexts, where the parameter books,
the activity record, the S/PDIF positions and the compaction plan are the whole library."""
import collections
import os
import subprocess

import numpy as np
import pytest

from orclib import Oracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_boot_cpu import flash_cases
from test_gpu_snapshot import oracle
import lifecycle_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspi_amd", "csrc")
DEFAULT_SEEDS = range(32)      # tests/test_gpu_lifecycle_fuzz.py::_fuzz_seeds without its environment variables

SPDIF_AFTER = ("pause", "resume", "move", "boot", "import")
PDM_AROUND = ("move", "import", "boot")
CROSSINGS = (["boot, move of the booted stream, run", "export, change at the source, import of that stash", "import into a paused slot, resume",
              "one-way move, request to the moved stream, run", "boot, run, enumerate"]
             + [f"spdif run directly after {k}" for k in SPDIF_AFTER] + [f"pdm on both sides of {k}" for k in PDM_AROUND])


def crossings(cfg, ops):
    """how often each crossing of two features occurs in one op list"""
    sizes = (cfg["S"], cfg["side"])
    paused = [np.zeros(n, dtype=bool) for n in sizes]
    tags = [[set() for _ in range(n)] for n in sizes]      # what has happened to the STREAM in a slot: travels with moves and snapshots
    stashes = {}
    out = collections.Counter()
    kind = lambda op: "move" if op["op"] == "compact" else op["op"]
    for i, op in enumerate(ops):
        c, k = op["ctx"], kind(op)
        touched = set()                                    # slots of context c whose stream this op changes or replaces
        if k == "run":
            hit = set()
            for s in np.flatnonzero(~paused[c]):
                hit |= tags[c][s]
                tags[c][s] -= {"booted, moved", "moved one-way, requested"}
                if "not enumerated" in tags[c][s]: tags[c][s] = (tags[c][s] - {"not enumerated"}) | {"played before its enumeration"}
            if "booted, moved" in hit: out["boot, move of the booted stream, run"] += 1
            if "moved one-way, requested" in hit: out["one-way move, request to the moved stream, run"] += 1
            prev = ops[i - 2] if ops[i - 1]["op"] == "spdif_carry" else ops[i - 1]      # (an import with its position carried over is an import)
            if op["spdif"] and prev["ctx"] == c and kind(prev) in SPDIF_AFTER: out[f"spdif run directly after {kind(prev)}"] += 1
        elif k == "pause": paused[c][op["first"]:op["first"] + op["count"]] = True
        elif k == "resume":
            r = range(op["first"], op["first"] + op["count"])
            if any(paused[c][s] and "imported while paused" in tags[c][s] for s in r): out["import into a paused slot, resume"] += 1
            for s in r: tags[c][s].discard("imported while paused")
            paused[c][op["first"]:op["first"] + op["count"]] = False
        elif k == "request":
            touched = set(range(sizes[c])) if op["stream"] is None else {op["stream"]}
            if op["stream"] is not None and "moved one-way" in tags[c][op["stream"]]: tags[c][op["stream"]].add("moved one-way, requested")
        elif k == "move":
            old = [set(t) for t in tags[c]]
            dsts = {d for _, d in op["moves"]}
            for s, d in op["moves"]:
                tags[c][d] = set(old[s]) - {"moved one-way"}
                if "booted" in old[s]: tags[c][d].add("booted, moved")
                if s not in dsts: tags[c][d].add("moved one-way")      # (its source stays behind as a frozen copy on the same parameter object)
                touched |= {s, d}
            paused[c] = M.moved_activity(paused[c], op["moves"])
        elif k == "boot":
            for s in op["streams"]: tags[c][s] = {"booted", "not enumerated"}
            touched = set(op["streams"])
        elif k == "enumerate":
            for s in op["streams"]:
                if "played before its enumeration" in tags[c][s]: out["boot, run, enumerate"] += 1; break
            for s in op["streams"]: tags[c][s] -= {"not enumerated", "played before its enumeration"}
        elif k == "export":
            stashes[op["stash"]] = dict(ctx=c, slots=set(range(op["first"], op["first"] + op["count"])), stale=False,
                                        tags=[set(tags[c][s]) for s in range(op["first"], op["first"] + op["count"])])
        elif k == "import":
            st = stashes[op["stash"]]
            if st["stale"]: out["export, change at the source, import of that stash"] += 1
            for j, t in enumerate(st["tags"]):
                tags[c][op["to"] + j] = set(t) | ({"imported while paused"} if paused[c][op["to"] + j] else set())
        for st in stashes.values():
            if st["ctx"] == c and st["slots"] & touched: st["stale"] = True
    for c in (0, 1):      # PDM on both sides: among the context's ops other than runs and enumerations, the neighbours of the call are PDM calls
        mine = [kind(op) for op in ops if op["ctx"] == c and op["op"] not in ("run", "enumerate", "spdif_carry", "spdif_mode")]
        for j in range(1, len(mine) - 1):
            if mine[j] in PDM_AROUND and mine[j - 1] == mine[j + 1] == "pdm": out[f"pdm on both sides of {mine[j]}"] += 1
    return out


def test_schedule_is_a_pure_function_of_the_seed():
    for seed in (0, 7):
        (c1, o1), (c2, o2) = M.schedule(seed), M.schedule(seed)
        assert o1 == o2 and {k: v for k, v in c1.items() if "blob" not in k} == {k: v for k, v in c2.items() if "blob" not in k}
        assert c1["blob"].tobytes() == c2["blob"].tobytes() and c1["blob2"].tobytes() == c2["blob2"].tobytes()
    assert M.schedule(0)[1] != M.schedule(1)[1]


def test_every_op_is_legal():
    """the generator's own rules, checked from the outside: move lists (no duplicate sources or destinations, a destination that is no source
    is paused), ranges inside the context, imports of earlier stashes only, S/PDIF runs only in the mode and never tiled or with I2S words,
    compactions that are the documented pairing"""
    for seed in range(200):
        cfg, ops = M.schedule(seed)
        sizes = (cfg["S"], cfg["side"])
        paused = [np.zeros(n, dtype=bool) for n in sizes]
        stashes, mode = {}, False
        after = [op for op in ops if not op.get("warm")]
        assert 8 <= len(after) <= 15, (seed, len(after))      # (8 to 14 ops, and the early switch to the S/PDIF mode where a seed has one)
        assert ops[0].get("warm") and ops[1].get("warm") and [(op["op"], op["ctx"]) for op in ops[-2:]] == [("run", 1), ("run", 0)]
        for op in ops:
            c, k = op["ctx"], op["op"]
            S = sizes[c]
            assert k in M.KINDS
            if "first" in op: assert 0 <= op["first"] and op["count"] >= 1 and op["first"] + op["count"] <= S, (seed, op)
            if k == "run": assert (not op["spdif"] or (mode and not op["tiled"] and not op["i2s"])) and (op.get("warm") or 1 <= op["n"] <= 3), (seed, op)
            elif k == "pause": paused[c][op["first"]:op["first"] + op["count"]] = True
            elif k == "resume": paused[c][op["first"]:op["first"] + op["count"]] = False
            elif k in ("move", "compact"):
                srcs, dsts = [s for s, _ in op["moves"]], [d for _, d in op["moves"]]
                assert op["moves"] and len(set(srcs)) == len(srcs) and len(set(dsts)) == len(dsts) and all(0 <= v < S for v in srcs + dsts) and all(s != d for s, d in op["moves"]), (seed, op)
                assert all(paused[c][d] for d in dsts if d not in srcs), (seed, op)
                if k == "compact": assert op["moves"] == M.compaction(paused[c], op["one_way"])
                paused[c] = M.moved_activity(paused[c], op["moves"])
            elif k in ("boot", "enumerate"): assert op["streams"] and len(set(op["streams"])) == len(op["streams"]) and all(0 <= s < S for s in op["streams"]), (seed, op)
            elif k == "request": assert op["stream"] is None or 0 <= op["stream"] < S
            elif k == "export": stashes[op["stash"]] = (op["count"], mode)
            elif k == "import": assert op["stash"] in stashes and stashes[op["stash"]][0] == op["count"] and op["to"] + op["count"] <= S, (seed, op)
            elif k == "spdif_mode": assert not mode; mode = True
            elif k == "spdif_carry": assert mode and stashes[op["stash"]][1], (seed, op)


def test_default_seeds_contain_the_crossings():
    """A condition, not a measurement: together the default seeds hold every op kind at least five times, every flavour, float layout and
    size, and every crossing at least twice."""
    kinds, total = collections.Counter(), collections.Counter()
    flavors, layouts, size_classes, requests = set(), set(), set(), collections.Counter()
    for seed in DEFAULT_SEEDS:
        cfg, ops = M.schedule(seed)
        kinds.update(op["op"] for op in ops)
        requests.update(op["kind"] for op in ops if op["op"] == "request")
        total.update(crossings(cfg, ops))
        flavors.add(cfg["flavor"]); layouts.add(cfg["layout"]); size_classes.add(M.sizes(cfg["flavor"]).index(cfg["S"]))
    print(dict(kinds), dict(total), dict(requests))
    assert all(kinds[k] >= 5 for k in M.KINDS), {k: kinds[k] for k in M.KINDS}
    assert flavors == set(M.FLAVORS) and layouts == set(M.LAYOUTS) and size_classes == set(range(6)), (flavors, layouts, size_classes)
    assert set(requests) == set(M.REQUESTS), requests
    assert all(total[k] >= 2 for k in CROSSINGS), {k: total[k] for k in CROSSINGS}


# ---- host-only books ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("life") / "snapshot_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", str(exe), os.path.join(ROOT, "tests", "snapshot_driver.cpp"), os.path.join(CSRC, "dspi_snapshot.cpp")], check=True)
    return str(exe)


FS, VOL = 48000, -20 * 256


@pytest.mark.parametrize("seed", range(30))
def test_host_only_books(seed, snap_driver, tmp_path):
    """40 random ops on a host-only context; after every one, for every stream: dspi_collect_bulk is the stream's oracle's (requests applied
    as issued, a boot replaces the oracle by a fresh one), the activity and the S/PDIF positions are the model's, dspi_plan_compaction is
    the documented pairing; the image count is within its bounds wherever the schedule asks for it (dspi_debug_image_count runs the fold-back
    pass, so asking after every op would fix when that pass happens: the schedule draws the moments instead); dspi_move_streams, dspi_import_streams, dspi_export_streams and
    dspi_realign_streams, given valid arguments, answer DSPI_E_NODEVICE and change none of it."""
    fl = ("fma", "q28")[seed % 2]
    S = (3, 131, 300)[seed // 2 % 3]
    flavor = M.FLAVORS[fl]
    ops = M.host_schedule(seed, fl, S, 40)
    blob, blob2 = WL.full_chain_blob(flavor), WL.full_chain_blob(flavor, max_delay_ms=7.0)
    names = {"blob2": blob2, "image": M.preset_image(flavor, FS)}
    dump, code = flash_cases(flavor)[0]
    d = Dspi(flavor, S, device=None)
    assert d.set_rate(FS) == 0
    d.set_volume(VOL)
    assert d.load_bulk(blob) == 0
    o = [oracle(flavor, FS, blob, VOL) for _ in range(S)]
    paused, sp, mode = np.zeros(S, dtype=bool), np.zeros(S, dtype=np.int64), False
    bulk = [x.collect_bulk() for x in o]      # the oracles' parameters, read again only where an op has addressed the stream

    def books():
        return [d.collect_bulk(s) for s in range(S)], d.streams_paused().tolist(), d.spdif_stream_pos().tolist() if mode else None

    def call(x, name, args):
        return x.vendor_get(W.REQ["CLEAR_CLIPS"], 0) if name == "clear_clips" else getattr(x, name)(*args)

    for i, op in enumerate(ops):
        k, what = op["op"], f"seed {seed}, op {i} ({op['op']})"
        if k == "request":
            args = tuple(names.get(a, a) if isinstance(a, str) else a for a in op["args"])
            t = range(S) if op["stream"] is None else (op["stream"],)
            if op["name"] == "clear_clips": d.clear_clips(stream=host.ALL if op["stream"] is None else op["stream"])
            else: assert getattr(d, op["name"])(*args, stream=host.ALL if op["stream"] is None else op["stream"]) == 0, what
            for s in t:
                call(o[s], op["name"], args); bulk[s] = o[s].collect_bulk()
        elif k == "pause":
            assert d.pause_streams(op["first"], op["count"]) == op["count"]; paused[op["first"]:op["first"] + op["count"]] = True
        elif k == "resume":
            assert d.resume_streams(op["first"], op["count"], as_is=op["as_is"]) == op["count"]; paused[op["first"]:op["first"] + op["count"]] = False
        elif k == "boot":
            assert d.boot_streams(op["streams"], dump if op["dump"] else None, as_is=op["as_is"]) == (code if op["dump"] else 48), what
            for s in op["streams"]:
                o[s].close(); o[s] = Oracle(flavor, detmath=True, flash=dump if op["dump"] else None); bulk[s] = o[s].collect_bulk()
                sp[s] = 0
        elif k == "enumerate":
            for s in op["streams"]:
                assert d.set_rate(FS, stream=s) == 0 and o[s].set_rate(FS) == 0
                d.set_volume(VOL, stream=s); o[s].set_volume(VOL)
                if s in op["blob_on"]: assert d.load_bulk(blob, stream=s) == 0 and o[s].load_bulk(blob) == 0
                bulk[s] = o[s].collect_bulk()
        elif k == "spdif_mode":
            assert d.spdif_per_stream(1) is True
            mode = True
            assert not d.spdif_stream_pos().any()      # (the context's own position, which nothing has advanced)
            sp[:] = (np.arange(S) * op["mul"] + op["add"]) % 192
            assert np.array_equal(d.spdif_stream_pos(set=sp), sp)
        elif k == "spdif_pos":
            n = len(op["values"])
            assert np.array_equal(d.spdif_stream_pos(op["first"], n, set=op["values"]), op["values"])
            sp[op["first"]:op["first"] + n] = op["values"]
        elif k == "plan":
            assert [tuple(m) for m in d.plan_compaction(op["one_way"]).tolist()] == M.compaction(paused, op["one_way"]), what
        elif k == "image_count":
            n, distinct = d.image_count(), len(set(d.collect_bulk(s) for s in range(S)))
            assert distinct <= n <= S, f"{what}: {n} parameter objects for {distinct} distinct parameter sets on {S} streams"
        elif k == "refused":
            before, images = books(), d.image_count()
            first, count = op["first"], op["count"]
            hb, sb = d.snapshot_sizes(first, count)
            state = np.zeros(sb // 4, dtype=np.uint32)
            with pytest.raises(DspiError) as e:
                if op["what"] == "move": d.move_streams(op["moves"])
                elif op["what"] == "export": d.export_streams(first, count)
                elif op["what"] == "realign": d.realign_streams(first, count)
                else:
                    path = tmp_path / "head.bin"
                    subprocess.run([snap_driver, "write", str(int(flavor)), "1" if fl == "fma" else "0", str(count), "1", str(path)], check=True)
                    d.import_streams(first, path.read_bytes(), state.reshape(count, -1), realign=bool(i & 1))
            assert e.value.code == host.E_NODEVICE, f"{what}: {op['what']} with valid arguments on a host-only context: {e.value}"
            assert books() == before and d.image_count() == images, f"{what}: a refused {op['what']} changed the books"
        else: raise AssertionError(k)
        got = books()
        for s in range(S): assert got[0][s] == bulk[s], f"{what}: dspi_collect_bulk of stream {s} is not its oracle's"
        assert got[1] == paused.astype(int).tolist(), f"{what}: dspi_streams_paused"
        if mode: assert got[2] == sp.tolist(), f"{what}: dspi_spdif_stream_pos"
        for one_way in (False, True):
            assert [tuple(m) for m in d.plan_compaction(one_way).tolist()] == M.compaction(paused, one_way), f"{what}: dspi_plan_compaction is not the documented pairing"
    for x in o: x.close()
    d.close()


def test_stand_alone_books_driver(tmp_path):
    """tools/lifecycle_books.cpp — a program of its own that drives the books of host-only contexts, the vehicle for AddressSanitizer and UBSan
    (dspi_amd/csrc/Makefile: lifecycle_books_asan; its own sequences, no oracle) — built here against the plain library: 30 contexts x 40
    ops, the program's own checks"""
    exe = tmp_path / "lifecycle_books"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tools", "lifecycle_books.cpp"),
                    "-L", CSRC, "-ldspi_mi355x", f"-Wl,-rpath,{CSRC}", f"-Wl,-rpath,{os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib')}"], check=True)
    r = subprocess.run([str(exe), "30", "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "books consistent" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
