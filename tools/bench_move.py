"""What moving streams (dspi_move_streams / dspi_plan_compaction, include/dspi.h) costs and saves (profiles/move.md).  bench.py's config 3
(65 536 float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major words) and config 5 (16 384 Q28 streams), device
buffers, times by HIP events on the contexts' streams after a warm-up, medians, shader clock and socket power per child.

Everything is a child process with one context; the three criteria alternate this build with the PARENT commit's library
(PARENT_LIB=<path of its libdspi_mi355x.so>; without it they are skipped and the line says so), ROUNDS times, median over the children's medians:
    a  compacted    this build: every second stream paused, dspi_plan_compaction applied      against   the parent, a context of half the streams
    b  whole_rows   this build: ROWS whole rows moved onto whole (paused) rows, one call       against   the parent, dspi_export_streams + realigning
                                                                                                       dspi_import_streams of the same streams (device buffers)
    c  untouched    this build, nothing paused or moved                                       against   the parent, the same context
Recorded beside them, this build alone (no criterion): the launch before compaction; the compacting call itself (scattered: one stream of
every second lane) per gigabyte moved, beside a device-to-device copy of the same bytes; one-way against swap; DSPI_MOVE_AS_IS; the host
time of the call and of the next launch's replan.

    python tools/bench_move.py [3 5]        ROUNDS=3 LAUNCHES=10 WARMUP=3 ROWS=16 PARENT_LIB=...
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pause import new_context, setup      # noqa: E402  (the same workloads, buffers and contexts)

ROUNDS, LAUNCHES, WARMUP, ROWS = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("LAUNCHES", 10), ("WARMUP", 3), ("ROWS", 16)))
med = lambda v: round(statistics.median(v), 4)


def timed(ev, fn):
    e0, e1 = ev.new(), ev.new()
    t = time.perf_counter(); ev.record(e0); fn(); ev.record(e1)
    host = (time.perf_counter() - t) * 1e3
    return ev.elapsed_ms(e0, e1), host


def child(config, mode):
    """one context: a JSON line"""
    import torch
    from bench import HipEvents, PowerSampler, chain_workload
    full = chain_workload(config)["streams"]
    w, S, pcm, (pairs, sub, peaks) = setup(config, full // 2 if mode == "small" else full)
    d = new_context(w, S)
    R = d.tile_streams()
    launch = lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    launch(); d.sync()
    ev = HipEvents(d.hip_stream())
    rec_bytes = d.snapshot_sizes(0, 1)[1]
    res = {"streams": S}

    def launches():
        ms = []
        for i in range(WARMUP + LAUNCHES):
            v, _ = timed(ev, launch)
            if i >= WARMUP: ms.append(v)
        return ms

    def wall(fn):
        t = time.perf_counter(); fn(); d.sync()
        return (time.perf_counter() - t) * 1e3

    smi = PowerSampler(0); smi.start()
    t0 = time.perf_counter()
    if mode in ("full", "small"):
        ms = launches()
        res.update(ms=med(ms), min=round(min(ms), 4))
    elif mode == "compacted":
        for s in range(1, S, 2): d.pause_streams(s, 1)
        before = launches()
        res["scattered_ms"] = med(before); res["scattered_plan"] = {k: v for k, v in d.launch_plan().items() if v}
        steady = med([wall(launch) for _ in range(3)])
        t = time.perf_counter(); moves = d.plan_compaction(); res["plan_compaction_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        dev_ms, host_ms = timed(ev, lambda: d.move_streams(moves))
        gb = len(moves) * rec_bytes / 1e9
        res.update(entries=len(moves), moved_gb=round(gb, 3), move_device_ms=round(dev_ms, 3), move_host_ms=round(host_ms, 3), move_ms_per_gb=round(dev_ms / gb, 3))
        res["next_launch_beyond_steady_ms"] = round(wall(launch) - steady, 3)
        ms = launches()
        res.update(ms=med(ms), min=round(min(ms), 4))
        # the same bytes as one device-to-device copy (read once, written once; the move reads and writes them twice)
        n = int(min(gb * 1e9, 4e9)) // 4
        a, b = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        t_ms = []
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
            t_ms.append(e0.elapsed_time(e1))
        res["device_copy_ms_per_gb"] = round(med(t_ms[1:]) / (n * 4 / 1e9), 3)
        del a, b
    elif mode == "whole_rows":
        count, half = ROWS * R, S // 2
        d.pause_streams(half, half)
        launch(); d.sync()
        down = [(s, half + s) for s in range(count)]; up = [(t, s) for s, t in down]
        dev, hst = [], []
        for i in range(2 + 2 * (LAUNCHES // 2)):      # [0, count) -> the paused rows, and back: every call is one-way into paused slots
            v, h = timed(ev, lambda: d.move_streams(up if i & 1 else down))
            if i >= 2: dev.append(v); hst.append(h)
            launch(); d.sync()
        res.update(count=count, ms=med(dev), min=round(min(dev), 4), host_ms=med(hst), gb=round(count * rec_bytes / 1e9, 3))
        steady = med([wall(launch) for _ in range(3)])
        d.move_streams(down); res["next_launch_beyond_steady_ms"] = round(wall(launch) - steady, 3); d.move_streams(up); launch(); d.sync()
        as_is = []
        for i in range(4):
            v, _ = timed(ev, lambda: d.move_streams(up if i & 1 else down, as_is=True)); as_is.append(v); launch(); d.sync()
        res["as_is_ms"] = med(as_is)
        swap = down + up
        sw = []
        for i in range(4):
            v, _ = timed(ev, lambda: d.move_streams(swap)); sw.append(v); launch(); d.sync()
        res["swap_ms"] = med(sw); res["swap_entries"] = len(swap)
    elif mode == "export_import":      # (the parent's way, also available in this build)
        count, half = ROWS * R, S // 2
        hb, sb = d.snapshot_sizes(0, count)
        state = torch.empty(sb // 4, dtype=torch.int32, device="cuda")
        dev = []
        for i in range(2 + LAUNCHES):
            def both():
                head = d.export_streams_device(0, count, state.data_ptr(), sb)
                d.import_streams_device(half, head, state.data_ptr(), sb, realign=True)
            v, _ = timed(ev, both)
            if i >= 2: dev.append(v)
            launch(); d.sync()
        res.update(count=count, ms=med(dev), min=round(min(dev), 4))
    else:
        raise SystemExit(f"unknown mode {mode}")
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    smi.stop()
    res.update(plan={k: v for k, v in d.launch_plan().items() if v}, power_w=pw and round(pw["power_w"], 1), sclk_mhz=pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]))
    print(json.dumps(res), flush=True)
    d.close()


def run_child(config, mode, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, mode], env=env, capture_output=True, text=True, timeout=400)
    if out.returncode != 0: raise RuntimeError(f"child {config} {mode} ({lib or 'this build'}): {out.stderr[-600:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3])
    parent = os.environ.get("PARENT_LIB")
    parent = os.path.abspath(parent) if parent else None
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "rows": ROWS}
        for name, mine, theirs in (("a_compacted_over_parent_half_context", "compacted", "small"), ("b_whole_rows_over_parent_export_import", "whole_rows", "export_import"),
                                   ("c_untouched_over_parent", "full", "full")):
            a, b = [], []
            for _ in range(ROUNDS):
                a.append(run_child(config, mine, None))
                if parent: b.append(run_child(config, theirs, parent))
            rec = {"this_build_ms": [x["ms"] for x in a], "this_build": a[-1]}
            if parent: rec.update(parent_ms=[x["ms"] for x in b], parent=b[-1], ratio=round(med([x["ms"] for x in a]) / med([x["ms"] for x in b]), 4))
            else: rec["parent"] = "skipped: PARENT_LIB not set"
            line[name] = rec
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
