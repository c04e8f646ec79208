"""The wide lifecycle fuzz without a GPU (tests/lifecycle_wide.py): a pin on the old generator, the legality of every op of the wide one checked
by a reader of its own, what the default seeds of tests/test_gpu_lifecycle_wide.py::test_fuzz_wide contain (crossings() below follows the
streams through moves, migrations, boots, resizes and imports independently of how the generator strings its ops together), and the wide
generator on host-only contexts, where sizes, capacities, activity, parameter books, plans and the running bytes are the whole library."""
import collections
import hashlib
import json

import numpy as np
import pytest

from orclib import Oracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_boot_cpu import flash_cases
from test_gpu_snapshot import oracle
import lifecycle_model as M
import lifecycle_wide as X

DEFAULT_SEEDS = range(32)      # tests/test_gpu_lifecycle_wide.py::_fuzz_seeds without its environment variables


# ---- 1. the old generator is what it was ----------------------------------------------------------------------------------------------------
OLD_SCHEDULES = "2a14795a1df6a6a1fc1012f157ae3ac157c4750da0075f1535b6838f9d4cff55"      # computed with tests/lifecycle_model.py as it stood before this file existed


def test_the_old_schedules_are_pinned():
    """sha256 over schedule(seed) for seeds 0..31: the configuration without the blobs as sorted JSON, the two blobs' bytes, the op list as
    sorted JSON (bytes as hex).  Widening the fuzz must not change what the old 32 seeds exercise."""
    def as_json(b):
        if isinstance(b, (bytes, bytearray)): return {"hex": bytes(b).hex()}
        raise TypeError(type(b))
    h = hashlib.sha256()
    for seed in range(32):
        cfg, ops = M.schedule(seed)
        h.update(json.dumps({k: v for k, v in cfg.items() if k not in ("blob", "blob2")}, sort_keys=True).encode())
        h.update(cfg["blob"].tobytes()); h.update(cfg["blob2"].tobytes())
        h.update(json.dumps(ops, sort_keys=True, default=as_json).encode())
    assert h.hexdigest() == OLD_SCHEDULES


def test_schedule_wide_is_a_pure_function_of_the_seed():
    for seed in (0, 5):
        (c1, o1), (c2, o2) = X.schedule_wide(seed), X.schedule_wide(seed)
        assert o1 == o2 and {k: v for k, v in c1.items() if "blob" not in k} == {k: v for k, v in c2.items() if "blob" not in k}
        assert c1["blob"].tobytes() == c2["blob"].tobytes() and c1["blob2"].tobytes() == c2["blob2"].tobytes()
    assert X.schedule_wide(0)[1] != X.schedule_wide(1)[1]


# ---- 2. legality ----------------------------------------------------------------------------------------------------------------------------
def test_every_wide_op_is_legal():
    """An independent reader re-derives sizes, activity and stashes from the op lists and checks every precondition include/dspi.h names."""
    for seed in range(200):
        cfg, ops = X.schedule_wide(seed)
        R, top = cfg["R"], 3 * cfg["R"] + 1
        size = [cfg["S"], cfg["side"]]
        start = list(size)
        paused = [np.zeros(n, dtype=bool) for n in size]
        stashes, mode, fmode, ran = {}, False, [False, False], [False, False]
        assert ops[0].get("warm") and ops[1].get("warm") and 20 <= len(ops) <= 70, (seed, len(ops))
        for i, op in enumerate(ops):
            c, k, at = op["ctx"], op["op"], (seed, i, op)
            S = size[c]
            assert k in X.KINDS and c in (0, 1), at
            if "first" in op: assert 0 <= op["first"] and op["count"] >= 1 and op["first"] + op["count"] <= S, at
            if k == "run":
                ran[c] = True
                assert op["form"] in X.FORMS and (op.get("warm") or 1 <= op["n"] <= 3), at
                assert not op["spdif"] or (mode and not op["tiled"] and not op["i2s"]), at
                if op["form"] in ("mixed", "mixed_pdm"): assert len(op["depths"]) == S and set(op["depths"]) <= {16, 24}, at
                else: assert op["depths"] is None, at
            elif k == "pdm": assert ran[c], at
            elif k == "pause": paused[c][op["first"]:op["first"] + op["count"]] = True
            elif k == "resume": paused[c][op["first"]:op["first"] + op["count"]] = False
            elif k in ("move", "compact"):
                srcs, dsts = [s for s, _ in op["moves"]], [d for _, d in op["moves"]]
                assert op["moves"] and len(set(srcs)) == len(srcs) and len(set(dsts)) == len(dsts) and all(0 <= v < S for v in srcs + dsts) and all(s != d for s, d in op["moves"]), at
                assert all(paused[c][d] for d in dsts if d not in srcs), at
                if k == "compact": assert op["moves"] == M.compaction(paused[c], op["one_way"]), at
                paused[c] = M.moved_activity(paused[c], op["moves"])
            elif k in ("boot", "enumerate"): assert op["streams"] and len(set(op["streams"])) == len(op["streams"]) and all(0 <= s < S for s in op["streams"]), at
            elif k == "request": assert (op["stream"] is None or 0 <= op["stream"] < S) and op["kind"] in X.REQUESTS, at
            elif k == "export": stashes[op["stash"]] = (op["count"], mode)
            elif k == "import": assert op["stash"] in stashes and stashes[op["stash"]][0] == op["count"] and 0 <= op["to"] and op["to"] + op["count"] <= S, at
            elif k == "spdif_mode": assert not mode; mode = True
            elif k == "spdif_carry": assert mode and stashes[op["stash"]][1], at
            elif k == "pdm_carry":
                prev = ops[i - 2] if ops[i - 1]["op"] == "spdif_carry" else ops[i - 1]
                assert prev["op"] == "import" and (prev["ctx"], prev["stash"], prev["to"], prev["count"]) == (c, op["stash"], op["to"], op["count"]), at
            elif k == "grow":
                assert op["old"] == S < op["n"] <= top, at
                paused[c] = np.concatenate([paused[c], np.full(op["n"] - S, op["paused"])]); size[c] = op["n"]
            elif k == "shrink":
                assert op["old"] == S and 1 <= op["n"] < S and paused[c][op["n"]:].all(), at      # "Every slot of the cut range must be PAUSED"
                paused[c] = paused[c][:op["n"]].copy(); size[c] = op["n"]
            elif k == "reserve": assert op["n"] >= S >= 1, at                                    # "for dspi_reserve_streams n_streams == 0 or below dspi_num_streams: DSPI_E_INVAL"
            elif k in ("migrate", "plan_migrate"):
                t = op["dst"]
                assert t == 1 - c and op["moves"], at
                srcs, dsts = [s for s, _ in op["moves"]], [d for _, d in op["moves"]]
                assert len(set(srcs)) == len(srcs) and all(0 <= s < S for s in srcs), at
                assert len(set(dsts)) == len(dsts) and all(0 <= d < size[t] and paused[t][d] for d in dsts), at      # "every listed destination must be PAUSED in `dst`"
                if k == "plan_migrate": assert [tuple(m) for m in op["moves"]] == X.migration_pairing(paused[c], paused[t], op["want"]) and not op["paused"], at
                for s, d in op["moves"]: paused[t][d] = op["paused"] or paused[c][s]
                for s in srcs: paused[c][s] = True
            elif k == "group":
                A = int((~paused[c]).sum())
                paused[c][:A] = False; paused[c][A:] = True
            elif k == "pdm_fade": assert op["on"] != fmode[c]; fmode[c] = op["on"]
            assert all(size[j] <= max(start[j], top) for j in (0, 1)), at


# ---- 3. what the default seeds contain ------------------------------------------------------------------------------------------------------
PDM_AROUND = ("move", "migrate", "import with carry", "import without carry", "boot", "grow")
FADE_THROUGH = ("pause and resume", "move", "migrate with the mode on at both ends", "migrate into a mode-off context", "boot", "shrink", "mode off")
MIXED_AFTER = ("move", "group", "migrate", "grow", "boot", "import", "resume")
SPDIF_AFTER = ("grow", "migrate")
CROSSINGS = (["reallocating grow, run", "grow over dirty columns with the PDM words allocated, PDM call", "grown stream moved into an older slot, run",
              "export, reallocating or cut-and-regrow resize, import of that stash", "not-yet-enumerated stream migrated, enumerated at its destination",
              "migration, request to the arrival alone, source copy resumed", "plan-grow-migrate-shrink rebalance", "group over three parameter objects or more, run",
              "a stream fed at both depths", "uniform-vector mixed call"]
             + [f"PDM call on both sides of {k}" for k in PDM_AROUND] + [f"fade in flight through {k}" for k in FADE_THROUGH]
             + [f"mixed-depth call directly after {k}" for k in MIXED_AFTER] + [f"spdif run directly after {k}" for k in SPDIF_AFTER])


class St:
    """what the reader knows of one stream: tags, whether its sub is on (None: not known), its running byte and fade position as far as the op
    list fixes them, its parameter-object tag, the depths it was fed at"""
    def __init__(self, obj):
        self.tags, self.sub, self.running, self.fade, self.obj, self.depths = set(), None, False, 0, obj, set()

    def copy(self):
        n = St(self.obj)
        n.tags, n.sub, n.running, n.fade, n.depths = set(self.tags), self.sub, self.running, self.fade, set(self.depths)
        return n


def crossings(cfg, ops):
    """how often each crossing occurs in one op list"""
    R, B = cfg["R"], cfg["B"]
    rows = lambda n: -(-n // R)
    size = [cfg["S"], cfg["side"]]
    paused = [np.zeros(n, dtype=bool) for n in size]
    st = [[St(f"base{c}") for _ in range(size[c])] for c in (0, 1)]
    cap = [rows(n) for n in size]
    dirty, words, fmode, pending, stashes = [0, 0], [False, False], [False, False], [set(), set()], {}
    requested, ids = set(), iter(range(1 << 30))
    out = collections.Counter()
    kind = lambda op: "move" if op["op"] == "compact" else op["op"]
    is_pdm = lambda op: op["op"] == "run" and op["form"] in ("pdm", "mixed_pdm")
    runs = [[i for i, op in enumerate(ops) if op["op"] == "run" and op["ctx"] == c] for c in (0, 1)]

    def around(i, before, after):
        """the context's nearest run before op i and the other context's (or its own) nearest run after it are both PDM calls"""
        b, a = [j for j in runs[before] if j < i], [j for j in runs[after] if j > i]
        return bool(b and a and is_pdm(ops[b[-1]]) and is_pdm(ops[a[0]]))

    def reallocated(c):
        for s in stashes.values():
            if s["ctx"] == c: s["resized"] = True

    for i, op in enumerate(ops):
        c, k = op["ctx"], kind(op)
        prev = next((o for o in reversed(ops[:i]) if o["op"] not in ("spdif_carry", "pdm_carry")), None)
        if k == "run":
            F, pdm_call = op["n"] * B, is_pdm(op)
            hit = set()
            for s in np.flatnonzero(~paused[c]):
                x = st[c][s]
                hit |= x.tags
                x.tags -= {"grown, moved"}
                x.depths.add(op["depths"][s] if op["depths"] else cfg["depth"])
                if pdm_call:
                    if x.sub: x.running, x.fade = True, 0
                    elif x.sub is False and x.running and fmode[c]:
                        if not x.fade: x.fade = 1024
                        x.fade -= min(F, x.fade - 1)
                        if x.fade == 1: x.fade, x.running = 0, False
                    else: x.running, x.fade = False, 0
            if "grown, moved" in hit: out["grown stream moved into an older slot, run"] += 1
            for key in sorted(pending[c]):
                if key.startswith("fade") or key.startswith("grow over dirty"):
                    if pdm_call: out[key] += 1; pending[c].discard(key)
                else: out[key] += 1; pending[c].discard(key)
            if pdm_call: words[c] = True
            where = prev["dst"] if prev and prev["op"] in ("migrate", "plan_migrate") else prev["ctx"] if prev else None
            if prev and where == c:
                pk = "migrate" if prev["op"] == "plan_migrate" else kind(prev)
                if op["depths"] and len(set(op["depths"])) == 2 and pk in MIXED_AFTER: out[f"mixed-depth call directly after {pk}"] += 1
                if op["spdif"] and pk in SPDIF_AFTER: out[f"spdif run directly after {pk}"] += 1
            if op["depths"] and len(set(op["depths"])) == 1: out["uniform-vector mixed call"] += 1
        elif k == "pause": paused[c][op["first"]:op["first"] + op["count"]] = True
        elif k == "resume":
            for s in range(op["first"], op["first"] + op["count"]):
                x = st[c][s]
                if paused[c][s] and x.fade: pending[c].add("fade in flight through pause and resume")
                if paused[c][s] and x.tags & {f"copy{j}" for j in requested}:
                    out["migration, request to the arrival alone, source copy resumed"] += 1
                    x.tags = {t for t in x.tags if not t.startswith("copy")}
            paused[c][op["first"]:op["first"] + op["count"]] = False
        elif k == "request":
            for s in (range(size[c]) if op["stream"] is None else (op["stream"],)):
                x = st[c][s]
                if op["kind"] == "sub_on": x.sub = True
                elif op["kind"] == "sub_off": x.sub = False
                elif op["kind"] in ("load_bulk", "load_slot"): x.sub, x.obj = None, "blob2" if op["kind"] == "load_bulk" else "image"
                elif op["kind"] in ("band", "preamp", "delay") and op["stream"] is not None: x.obj = f"own{next(ids)}"
                if op["stream"] is not None: requested.update(int(t[7:]) for t in x.tags if t.startswith("arrival"))
        elif k == "move":
            old = [x.copy() for x in st[c]]
            for s, d in op["moves"]:
                x = old[s].copy()
                if "grown" in x.tags and d < next(int(t[5:]) for t in x.tags if t.startswith("from:")): x.tags.add("grown, moved")
                if x.fade: pending[c].add("fade in flight through move")
                st[c][d] = x
            if any(old[s].sub for s, _ in op["moves"]) and around(i, c, c): out["PDM call on both sides of move"] += 1
            paused[c] = M.moved_activity(paused[c], op["moves"])
        elif k == "boot":
            if around(i, c, c): out["PDM call on both sides of boot"] += 1
            tag = f"boot{next(ids)}"
            for s in op["streams"]:
                if st[c][s].fade: pending[c].add("fade in flight through boot")
                st[c][s] = St(tag); st[c][s].tags = {"not enumerated"}
        elif k == "enumerate":
            for s in op["streams"]:
                x = st[c][s]
                if "migrated before its enumeration" in x.tags: out["not-yet-enumerated stream migrated, enumerated at its destination"] += 1; break
            for s in op["streams"]:
                st[c][s].tags -= {"not enumerated", "migrated before its enumeration"}
                if s in op["blob_on"]: st[c][s].sub, st[c][s].obj = None, f"enum{c}"
        elif k == "export":
            r = range(op["first"], op["first"] + op["count"])
            stashes[op["stash"]] = dict(ctx=c, first=op["first"], count=op["count"], resized=False, cut=False, st=[st[c][s].copy() for s in r])
        elif k == "import":
            s_ = stashes[op["stash"]]
            if s_["resized"] and s_["ctx"] == c: out["export, reallocating or cut-and-regrow resize, import of that stash"] += 1
            carried = i + 1 < len(ops) and any(o["op"] == "pdm_carry" for o in ops[i + 1:i + 3] if o["op"] in ("spdif_carry", "pdm_carry"))
            if any(x.sub for x in s_["st"]) and around(i, c, c): out[f"PDM call on both sides of import {'with' if carried else 'without'} carry"] += 1
            for j, x in enumerate(s_["st"]):
                was = st[c][op["to"] + j]
                n = x.copy()
                n.tags -= {"grown", "grown, moved"}
                n.running, n.fade = (x.running, x.fade if fmode[c] else 0) if carried else (was.running, was.fade)
                st[c][op["to"] + j] = n
        elif k == "grow":
            n, S = op["n"], size[c]
            if rows(n) > cap[c]:
                cap[c] = rows(n); pending[c].add("reallocating grow, run"); reallocated(c); dirty[c] = 0
            elif S < dirty[c] and words[c]: pending[c].add("grow over dirty columns with the PDM words allocated, PDM call")
            if around(i, c, c): out["PDM call on both sides of grow"] += 1
            tag = f"grow{next(ids)}"
            for s in range(S, n):
                x = St(tag); x.tags = {"not enumerated", "grown", f"from:{S}"}
                st[c].append(x)
            paused[c] = np.concatenate([paused[c], np.full(n - S, op["paused"])]); size[c] = n
            for s_ in stashes.values():
                if s_["ctx"] == c and s_["cut"] and n >= s_["first"] + s_["count"]: s_["resized"] = True
        elif k == "shrink":
            n, S = op["n"], size[c]
            if any(x.fade for x in st[c][n:]): pending[c].add("fade in flight through shrink")
            dirty[c] = max(dirty[c], S)
            del st[c][n:]
            paused[c] = paused[c][:n].copy(); size[c] = n
            for s_ in stashes.values():
                if s_["ctx"] == c and n < s_["first"] + s_["count"]: s_["cut"] = True
            plan = ops[i - 1]      # the rebalance: the destination grown paused, the plan migrated, the source cut
            if plan["op"] == "plan_migrate" and plan["ctx"] == c and i >= 2 and ops[i - 2]["op"] == "grow" and ops[i - 2]["ctx"] == plan["dst"] and ops[i - 2]["paused"]:
                out["plan-grow-migrate-shrink rebalance"] += 1
        elif k == "reserve":
            if rows(op["n"]) != cap[c]: cap[c] = rows(op["n"]); reallocated(c); dirty[c] = 0
        elif k in ("migrate", "plan_migrate"):
            t = op["dst"]
            both = fmode[c] and fmode[t]
            if any(st[c][s].sub for s, _ in op["moves"]) and around(i, c, t): out["PDM call on both sides of migrate"] += 1
            for s, d in op["moves"]:
                x, j = st[c][s].copy(), next(ids)
                x.tags -= {"grown", "grown, moved"}
                if "not enumerated" in x.tags: x.tags.add("migrated before its enumeration")
                if x.fade: pending[t].add("fade in flight through migrate with the mode on at both ends" if both else "fade in flight through migrate into a mode-off context" if fmode[c] else "")
                if not both: x.running, x.fade = x.running and not x.fade, 0
                x.tags.add(f"arrival{j}"); st[c][s].tags.add(f"copy{j}")
                st[t][d] = x
                paused[t][d] = op["paused"] or paused[c][s]
            for s, _ in op["moves"]: paused[c][s] = True
            pending[t].discard("")
        elif k == "group":
            active = [x for x, p in zip(st[c], paused[c]) if not p]
            if len({x.obj for x in active}) >= 3: pending[c].add("group over three parameter objects or more, run")
            A = len(active)
            st[c] = [St("unknown") for _ in range(size[c])]      # (the list is the library's: the reader cannot follow the streams through it)
            paused[c][:A] = False; paused[c][A:] = True
        elif k == "pdm_fade":
            if not op["on"] and any(x.fade for x in st[c]): pending[c].add("fade in flight through mode off")
            fmode[c] = op["on"]
            for x in st[c]:
                if x.fade: x.running = False
                x.fade = 0
    if any(len(x.depths) == 2 for c in (0, 1) for x in st[c]): out["a stream fed at both depths"] += 1
    return out


def test_default_wide_seeds_contain_the_crossings():
    """A condition, not a measurement: together the default seeds hold every new op kind and both new request kinds at least five times, every
    flavour, float layout and starting size, and every crossing at least twice."""
    kinds, total, requests = collections.Counter(), collections.Counter(), collections.Counter()
    flavors, layouts, size_classes = set(), set(), set()
    for seed in DEFAULT_SEEDS:
        cfg, ops = X.schedule_wide(seed)
        kinds.update(op["op"] for op in ops)
        requests.update(op["kind"] for op in ops if op["op"] == "request")
        total.update(crossings(cfg, ops))
        flavors.add(cfg["flavor"]); layouts.add(cfg["layout"]); size_classes.add((cfg["flavor"] == "q28", M.sizes(cfg["flavor"]).index(cfg["S"])))
    print(dict(kinds), dict(requests))
    for k in CROSSINGS: print(f"{total[k]:4d}  {k}")
    assert all(kinds[k] >= 5 for k in X.NEW_KINDS) and all(kinds[k] >= 2 for k in M.KINDS), {k: kinds[k] for k in X.KINDS}      # (the old kinds' own counts are test_lifecycle_cpu.py's)
    assert all(requests[k] >= 5 for k in X.NEW_REQUESTS) and set(requests) <= set(X.REQUESTS), requests
    assert flavors == set(M.FLAVORS) and layouts == set(M.LAYOUTS) and size_classes == {(q, i) for q in (False, True) for i in range(6)}, (flavors, layouts, size_classes)
    assert all(total[k] >= 2 for k in CROSSINGS), {k: total[k] for k in CROSSINGS if total[k] < 2}


# ---- 4. host-only books ---------------------------------------------------------------------------------------------------------------------
FS, VOL = 48000, -20 * 256


def mixed_offsets(depths, F):
    """the header's formula: offset[0] = 0, offset[s + 1] = offset[s] + F * (bit_depths[s] == 24 ? 6 : 4)"""
    return np.concatenate([[0], np.cumsum([F * (6 if d == 24 else 4) for d in depths])]).astype(np.uint64)


@pytest.mark.parametrize("seed", range(24))
def test_host_only_wide_books(seed):
    """50 random ops on two host-only contexts; after every one, for both: dspi_num_streams, dspi_stream_capacity (where the header fixes it),
    dspi_streams_paused, the S/PDIF positions, dspi_pdm_running, the fade mode and every stream's dspi_collect_bulk are the model's.
    dspi_plan_grouping's list leaves slots [0, A) active when applied to the activity record, dspi_plan_migration is the documented pairing,
    dspi_mixed_pcm_bytes is the header's offset formula; dspi_migrate_streams, dspi_process_mixed, dspi_process_pdm and dspi_pdm_fade_state,
    given valid arguments, answer DSPI_E_NODEVICE and change none of it."""
    fl = ("fma", "q28")[seed % 2]
    S0 = (3, 131, M.sizes(fl)[-1])[seed // 2 % 3]
    flavor, R = M.FLAVORS[fl], M.row(fl)
    rows = lambda n: -(-n // R)
    ops = X.host_schedule_wide(seed, fl, S0, 50)
    blob, blob2 = WL.full_chain_blob(flavor), WL.full_chain_blob(flavor, max_delay_ms=7.0)
    names = {"blob2": blob2, "image": M.preset_image(flavor, FS)}
    dump, code = flash_cases(flavor)[0]
    N = W.dims(int(flavor))[1]
    ds, model = [], []
    for S in (S0, M.SIDE):
        d = Dspi(flavor, S, device=None)
        assert d.set_rate(FS) == 0
        d.set_volume(VOL)
        assert d.load_bulk(blob) == 0
        ds.append(d)
        model.append(dict(o=[oracle(flavor, FS, blob, VOL) for _ in range(S)], paused=np.zeros(S, dtype=bool), sp=np.zeros(S, dtype=np.int64),
                          running=np.zeros(S, dtype=np.uint8), fmode=False, cap=rows(S)))
        model[-1]["bulk"] = [x.collect_bulk() for x in model[-1]["o"]]
    mode = False

    def books(c):
        d = ds[c]
        return ([d.collect_bulk(s) for s in range(d.n_streams)], d.n_streams, d.stream_capacity(), d.streams_paused().tolist(), d.spdif_stream_pos().tolist() if mode else None,
                d.pdm_running().tolist(), d.pdm_fade())

    def call(x, name, args):
        if name == "clear_clips": return x.vendor_get(W.REQ["CLEAR_CLIPS"], 0)
        if name == "sub_on":
            for o in range(2, N - 1): x.vendor_set(W.REQ["SET_OUTPUT_ENABLE"], o, b"\x00")
            return x.vendor_set(W.REQ["SET_OUTPUT_ENABLE"], N - 1, b"\x01")
        if name == "sub_off": return x.vendor_set(W.REQ["SET_OUTPUT_ENABLE"], N - 1, b"\x00")
        return getattr(x, name)(*args)

    def fresh(m, s, flash=None):
        m["o"][s].close(); m["o"][s] = Oracle(flavor, detmath=True, flash=flash); m["bulk"][s] = m["o"][s].collect_bulk()
        m["sp"][s] = 0; m["running"][s] = 0

    for i, op in enumerate(ops):
        c, k, what = op["ctx"], op["op"], f"seed {seed}, op {i} ({op['op']})"
        d, m = ds[c], model[c]
        S = d.n_streams
        if k == "request":
            args = tuple(names.get(a, a) if isinstance(a, str) else a for a in op["args"])
            st = host.ALL if op["stream"] is None else op["stream"]
            if op["name"] == "clear_clips": d.clear_clips(stream=st)
            elif op["name"] in X.NEW_REQUESTS:
                class to_d:      # (the same request sequence, addressed to the context)
                    vendor_set = staticmethod(lambda req, w, p: d.vendor_set(req, w, p, stream=st))
                call(to_d, op["name"], ())
            else: assert getattr(d, op["name"])(*args, stream=st) == 0, what
            for s in (range(S) if op["stream"] is None else (op["stream"],)):
                call(m["o"][s], op["name"], args); m["bulk"][s] = m["o"][s].collect_bulk()
        elif k == "pause":
            assert d.pause_streams(op["first"], op["count"]) == op["count"]; m["paused"][op["first"]:op["first"] + op["count"]] = True
        elif k == "resume":
            assert d.resume_streams(op["first"], op["count"], as_is=op["as_is"]) == op["count"]; m["paused"][op["first"]:op["first"] + op["count"]] = False
        elif k == "boot":
            assert d.boot_streams(op["streams"], dump if op["dump"] else None, as_is=op["as_is"]) == (code if op["dump"] else 48), what
            for s in op["streams"]: fresh(m, s, dump if op["dump"] else None)
        elif k == "enumerate":
            for s in op["streams"]:
                o = m["o"][s]
                assert d.set_rate(FS, stream=s) == 0 and o.set_rate(FS) == 0
                d.set_volume(VOL, stream=s); o.set_volume(VOL)
                if s in op["blob_on"]: assert d.load_bulk(blob, stream=s) == 0 and o.load_bulk(blob) == 0
                m["bulk"][s] = o.collect_bulk()
        elif k == "spdif_mode":
            mode = True
            for y, my in zip(ds, model):
                assert y.spdif_per_stream(1) is True
                my["sp"][:] = (np.arange(y.n_streams) * op["mul"] + op["add"]) % 192
                assert np.array_equal(y.spdif_stream_pos(set=my["sp"]), my["sp"])
        elif k == "grow":
            n = op["n"]
            assert d.resize_streams(n, paused=op["paused"]) == n == d.n_streams == int(d.L.dspi_num_streams(d.h)), what
            if rows(n) > m["cap"]: m["cap"] = rows(n)
            m["o"] += [Oracle(flavor, detmath=True) for _ in range(n - S)]; m["bulk"] += [x.collect_bulk() for x in m["o"][S:]]
            m["paused"] = np.concatenate([m["paused"], np.full(n - S, op["paused"])])
            m["sp"] = np.concatenate([m["sp"], np.zeros(n - S, dtype=np.int64)]); m["running"] = np.concatenate([m["running"], np.zeros(n - S, dtype=np.uint8)])
        elif k == "shrink":
            n = op["n"]
            assert d.resize_streams(n) == n == d.n_streams, what
            for x in m["o"][n:]: x.close()
            del m["o"][n:], m["bulk"][n:]
            m["paused"], m["sp"], m["running"] = m["paused"][:n].copy(), m["sp"][:n].copy(), m["running"][:n].copy()
        elif k == "reserve":
            assert d.reserve_streams(op["n"]) == rows(op["n"]) * R == op["rows"] * R, what
            m["cap"] = rows(op["n"])
        elif k == "plan_group":
            moves = [tuple(int(v) for v in mv) for mv in np.asarray(d.plan_grouping(op["one_way"])).reshape(-1, 2).tolist()]
            srcs, dsts = [s for s, _ in moves], [t for _, t in moves]
            assert len(set(srcs)) == len(srcs) and len(set(dsts)) == len(dsts) and all(s != t for s, t in moves) and dsts == sorted(dsts), f"{what}: {moves[:6]}"
            assert all(m["paused"][t] for t in dsts if t not in srcs), f"{what}: an active destination that is no source"
            A = int((~m["paused"]).sum())
            after = M.moved_activity(m["paused"], moves) if moves else m["paused"]
            assert not after[:A].any() and after[A:].all(), f"{what}: the list does not leave slots [0, {A}) active"
        elif k == "plan":
            t = op["dst"]
            plan = [tuple(mv) for mv in np.asarray(d.plan_migration(ds[t], op["want"])).reshape(-1, 2).tolist()]
            assert plan == X.migration_pairing(m["paused"], model[t]["paused"], op["want"]), f"{what}: dspi_plan_migration is not the documented pairing"
        elif k == "pdm_fade":
            assert d.pdm_fade(1 if op["on"] else 0) is op["on"]; m["fmode"] = op["on"]
        elif k == "pdm_running":
            n = len(op["values"])
            assert d.pdm_running(op["first"], n, set=op["values"]).tolist() == op["values"]
            m["running"][op["first"]:op["first"] + n] = op["values"]
        elif k == "mixed_bytes":
            total, off = d.mixed_pcm_bytes(op["depths"], op["n"], op["B"])
            want = mixed_offsets(op["depths"], op["n"] * op["B"])
            assert total == int(want[-1]) and np.array_equal(off, want), what
        elif k == "image_count":
            n, distinct = d.image_count(), len(set(d.collect_bulk(s) for s in range(S)))
            assert distinct <= n <= S, f"{what}: {n} parameter objects for {distinct} distinct parameter sets on {S} streams"
        elif k == "refused":
            before, images = (books(0), books(1)), (ds[0].image_count(), ds[1].image_count())
            depths, F = op["depths"], 48
            pcm = np.zeros(int(mixed_offsets(depths, F)[-1]), dtype=np.uint8)
            with pytest.raises(DspiError) as e:
                if op["what"] == "migrate": d.migrate_streams(ds[1 - c], op["moves"])
                elif op["what"] == "mixed": d.process_mixed_host(pcm, depths, 1, F)
                elif op["what"] == "pdm": d.process_pdm_host(np.zeros((S, F, 2), dtype=np.int16), 1, F)
                else: d.pdm_fade_state(op["first"], op["count"])
            assert e.value.code == host.E_NODEVICE, f"{what}: {op['what']} with valid arguments on a host-only context: {e.value}"
            assert (books(0), books(1)) == before and (ds[0].image_count(), ds[1].image_count()) == images, f"{what}: a refused {op['what']} changed the books"
        else: raise AssertionError(k)
        for j in (0, 1):
            got, mj = books(j), model[j]
            assert got[1] == len(mj["o"]) == int(ds[j].L.dspi_num_streams(ds[j].h)), f"{what}: dspi_num_streams of context {j}"
            for s in range(got[1]): assert got[0][s] == mj["bulk"][s], f"{what}: context {j}: dspi_collect_bulk of stream {s} is not its oracle's"
            assert got[2] == mj["cap"] * R, f"{what}: context {j}: dspi_stream_capacity is {got[2]}, the header says {mj['cap'] * R}"
            assert got[3] == mj["paused"].astype(int).tolist(), f"{what}: context {j}: dspi_streams_paused"
            if mode: assert got[4] == mj["sp"].tolist(), f"{what}: context {j}: dspi_spdif_stream_pos"
            assert got[5] == mj["running"].tolist(), f"{what}: context {j}: dspi_pdm_running"
            assert got[6] is mj["fmode"], f"{what}: context {j}: dspi_pdm_fade"
    for mj in model:
        for x in mj["o"]: x.close()
    for d in ds: d.close()
