"""What migrating streams between two contexts (dspi_migrate_streams, include/dspi.h) costs (profiles/migrate.md).  One GPU, two contexts in one
child process; method of profiles/pause.md: every figure comes from child processes that alternate, ROUNDS times, and is the median over the
children's medians.

(a)  N = 8 192 streams (float, FMA contract: `f32`; Q28: `q28`), scattered: every second stream of the source's first 2 N slots, into the N paused
     slots behind the destination's one row of residents.  Per child REPS timed calls after one untimed; between calls only books are put back
     (the sources resumed as they are, the destinations paused again), so every call moves the same bytes.  Wall time from before the call until
     both contexts' streams are idle (the two routes enqueue on different streams, so one stream's events cannot time both); `src_stream_ms`
     beside it is the new call by HIP events on the source's stream, which ends up waiting for the destination's last scatter.
         migrate        this build: dspi_migrate_streams, default and DSPI_MIGRATE_AS_IS, per transport (DSPI_MIGRATE_VIA unset, copy, host)
         todays_route   the PARENT commit's library (PARENT_LIB; skipped without it): dspi_move_streams of the same streams into one range of free
                        slots of the source (which the source must have: N more slots), dspi_export_streams with DSPI_MEM_DEVICE, dspi_sync,
                        dspi_import_streams with DSPI_SNAP_REALIGN
         device_copy    a device-to-device copy of the same bytes (read once, written once)
(b)  nothing that dspi_move_streams and dspi_process run has changed: tools/bench_move.py's children `whole_rows` and `full` (config 3 and 5) on
     this build against the parent's.

    PARENT_LIB=<parent's libdspi_mi355x.so> python tools/bench_migrate.py [a] [b]        ROUNDS=3 REPS=5 N=8192 CONFIGS="3 5" MODES="whole_rows full"
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, REPS, N = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("REPS", 5), ("N", 8192)))
med = lambda v: round(statistics.median(v), 4)


def child(kind, mode, as_is):
    """two contexts on device 0: a JSON line"""
    import numpy as np
    import torch
    from bench import HipEvents
    from dspi_amd import wire as W, workloads as WL
    from dspi_amd.host import Dspi
    flavor = W.F32_FMA if kind == "f32" else 0
    fs, B = 48000, 48

    def context(S):
        d = Dspi(flavor, S, device=0)
        d.set_rate(fs); d.set_volume(-20 * 256)
        assert d.load_bulk(WL.full_chain_blob(int(flavor))) == 0
        pcm = torch.randint(-16384, 16385, (S, 2 * B, 2), dtype=torch.int16, device="cuda")
        out = (torch.empty((S, d.P, 2 * B, 2), dtype=torch.int32, device="cuda"), torch.empty((S, 2 * B), dtype=torch.int32, device="cuda"),
               torch.empty((S, 2, d.C), dtype=torch.int16, device="cuda"))
        d.process_device(pcm.data_ptr(), 2, B, 16, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()); d.sync()
        return d
    src = context(3 * N)
    R = src.tile_streams()
    dst = context(R + N)
    src.pause_streams(2 * N, N); dst.pause_streams(R, N)
    sources = np.arange(1, 2 * N, 2, dtype=np.uint32)
    rec_bytes = src.snapshot_sizes(0, 1)[1]
    res = {"kind": kind, "mode": mode, "as_is": as_is, "streams": N, "gb": round(N * rec_bytes / 1e9, 4)}
    both_idle = lambda: (src.sync(), dst.sync())

    def put_back():
        for s in sources.tolist(): src.resume_streams(s, 1, as_is=True)      # (books only: nothing is enqueued)
        dst.pause_streams(R, N)
    wall, dev = [], []
    if mode == "migrate":
        moves = np.stack([sources, R + np.arange(N, dtype=np.uint32)], axis=1)
        ev = HipEvents(src.hip_stream())
        for i in range(1 + REPS):
            both_idle()
            e0, e1 = ev.new(), ev.new()
            t = time.perf_counter(); ev.record(e0)
            assert src.migrate_streams(dst, moves, as_is=as_is) == N
            ev.record(e1); host = time.perf_counter() - t
            both_idle()
            if i: wall.append((time.perf_counter() - t) * 1e3); dev.append(ev.elapsed_ms(e0, e1)); res["host_ms"] = round(host * 1e3, 3)
            put_back()
        res.update(ms=med(wall), min=round(min(wall), 4), src_stream_ms=med(dev), via=os.environ.get("DSPI_MIGRATE_VIA", "unset"))
    elif mode == "todays_route":
        together = np.stack([sources, 2 * N + np.arange(N, dtype=np.uint32)], axis=1)
        hb, sb = src.snapshot_sizes(0, N)
        state = torch.empty(sb // 4, dtype=torch.int32, device="cuda")
        for i in range(1 + REPS):
            both_idle()
            t = time.perf_counter()
            assert src.move_streams(together, as_is=as_is) == N
            head = src.export_streams_device(2 * N, N, state.data_ptr(), sb)
            src.sync()
            dst.import_streams_device(R, head, state.data_ptr(), sb, realign=not as_is)
            both_idle()
            if i: wall.append((time.perf_counter() - t) * 1e3)
            # (books back: the gathered range paused again, the sources resumed, the destination's slots paused — its caller would ALSO have
            #  to pause the range [2 N, 3 N) and carry activity and S/PDIF positions by hand, which is not timed)
            src.pause_streams(2 * N, N); put_back()
        res.update(ms=med(wall), min=round(min(wall), 4))
    elif mode == "device_copy":
        n = N * rec_bytes // 4
        a, b = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        for i in range(1 + REPS):
            torch.cuda.synchronize()
            t = time.perf_counter(); b.copy_(a); torch.cuda.synchronize()
            if i: wall.append((time.perf_counter() - t) * 1e3)
        res.update(ms=med(wall), min=round(min(wall), 4))
    else:
        raise SystemExit(f"unknown mode {mode}")
    print(json.dumps(res), flush=True)
    src.close(); dst.close()


def run_child(args, lib, via=None, script=None):
    env = dict(os.environ)
    env.pop("DSPI_LIB", None); env.pop("DSPI_MIGRATE_VIA", None)
    if lib: env["DSPI_LIB"] = lib
    if via: env["DSPI_MIGRATE_VIA"] = via
    out = subprocess.run([sys.executable, script or os.path.abspath(__file__), "--child"] + args, env=env, capture_output=True, text=True, timeout=500)
    if out.returncode != 0: raise RuntimeError(f"child {args} ({lib or 'this build'}): {out.stderr[-800:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def alternate(children):
    """children: {name: thunk}; ROUNDS rounds in this order; {name: {"ms": [child medians], "last": the last child's line}}"""
    got = {k: [] for k in children}
    for _ in range(ROUNDS):
        for k, f in children.items(): got[k].append(f())
    return {k: {"ms": [x["ms"] for x in v], "median": med([x["ms"] for x in v]), "last": v[-1]} for k, v in got.items()}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3], sys.argv[4] == "1")
    parts = [a for a in sys.argv[1:] if a in ("a", "b")] or ["a", "b"]
    parent = os.environ.get("PARENT_LIB")
    parent = os.path.abspath(parent) if parent else None
    if "a" in parts:
        for kind in ("f32", "q28"):
            for as_is in (False, True):
                ch = {f"migrate_{via or 'unset'}": (lambda via=via: run_child([kind, "migrate", str(int(as_is))], None, via)) for via in (None, "copy", "host")}
                ch["device_copy"] = lambda: run_child([kind, "device_copy", "0"], None)
                if parent: ch["todays_route_parent"] = lambda: run_child([kind, "todays_route", str(int(as_is))], parent)
                r = alternate(ch)
                line = {"part": "a", "kind": kind, "as_is": as_is, "streams": N, "rounds": ROUNDS, "reps": REPS, **r}
                if parent: line["migrate_unset_over_todays_route"] = round(r["migrate_unset"]["median"] / r["todays_route_parent"]["median"], 4)
                else: line["todays_route_parent"] = "skipped: PARENT_LIB not set"
                line["migrate_unset_over_device_copy"] = round(r["migrate_unset"]["median"] / r["device_copy"]["median"], 4)
                print(json.dumps(line), flush=True)
    if "b" in parts:
        mv = os.path.join(ROOT, "tools", "bench_move.py")
        for config in os.environ.get("CONFIGS", "3 5").split():
            for mode in os.environ.get("MODES", "whole_rows full").split():
                ch = {"this_build": lambda: run_child([config, mode], None, script=mv)}
                if parent: ch["parent"] = lambda: run_child([config, mode], parent, script=mv)
                r = alternate(ch)
                line = {"part": "b", "config": config, "what": "dspi_move_streams, whole rows" if mode == "whole_rows" else "dspi_process, the headline launch", "rounds": ROUNDS,
                        **{k: {"ms": v["ms"], "median": v["median"]} for k, v in r.items()}}
                if parent: line["ratio"] = round(r["this_build"]["median"] / r["parent"]["median"], 4)
                else: line["parent"] = "skipped: PARENT_LIB not set"
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
