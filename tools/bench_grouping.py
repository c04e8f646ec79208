"""What grouping (dspi_plan_grouping through dspi_move_streams, include/dspi.h) gives back (profiles/grouping.md).  bench.py's config 3
(65 536 float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major words) and config 5 (16 384 Q28 streams) at their
own sizes, with TWO presets of different structure: the config's own, and the same chain with delays capped at 1 ms and one master band
bypassed.  Device buffers, times by HIP events on the contexts' streams after a warm-up, medians, shader clock and socket power per child.

Every figure comes from a child process with one context; the criterion alternates this build with the PARENT commit's library
(PARENT_LIB=<path of its libdspi_mi355x.so>; without it the parent's side is skipped and the line says so), ROUNDS times, median over the
children's medians:
    a  scattered   this build: the presets assigned by s % 2, launch time                                    recorded only
    b  grouped     the same context after dspi_plan_grouping + dspi_move_streams, launch time     against   the parent, a context whose presets
                                                                                                            were loaded in grouped order from the
                                                                                                            start (first half, second half)
    c  host cost   host time of the planning call (two objects: the per-stream calls' equal objects were folded by the first launch; on the
                   grouped context `plan_again_host_ms`), host and device time of the move, what the first launch after the move takes
                   beyond a steady one (the replan)                                                          recorded only

    python tools/bench_grouping.py [3 5]        ROUNDS=3 LAUNCHES=10 WARMUP=3 PARENT_LIB=...
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

from bench_move import timed      # noqa: E402
from bench_pause import new_context, setup      # noqa: E402  (the same workloads, buffers and contexts)

ROUNDS, LAUNCHES, WARMUP = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("LAUNCHES", 10), ("WARMUP", 3)))
med = lambda v: round(statistics.median(v), 4)


def second_preset(flavor):
    from dspi_amd import wire as W, workloads as WL
    y = WL.full_chain_blob(flavor, max_delay_ms=1.0)
    W.set_band(y, 1, 4, W.FILTER_FLAT, WL.PEQ_FREQS[4], 1.41, 0.0)
    return y


def child(config, mode):
    """one context: a JSON line"""
    from bench import HipEvents, PowerSampler
    w, S, pcm, (pairs, sub, peaks) = setup(config)
    d = new_context(w, S)
    y = second_preset(w["flavor"])
    t = time.perf_counter()
    for s in (range(1, S, 2) if mode == "scattered" else range(S // 2, S)): assert d.load_bulk(y, stream=s) == 0
    d.set_volume(w["vol"])      # (a broadcast call: the per-stream calls' equal objects fold into one at the next launch — the parent's library has no other way)
    load_ms = (time.perf_counter() - t) * 1e3
    launch = lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    launch(); d.sync()
    assert d.image_count() == 2
    ev = HipEvents(d.hip_stream())
    res = {"streams": S, "load_host_ms": round(load_ms, 1)}

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
    if mode == "grouped":
        ms = launches()
    elif mode == "scattered":
        before = launches()
        res.update(scattered_ms=med(before), scattered_min=round(min(before), 4), scattered_plan={k: v for k, v in d.launch_plan().items() if v})
        t = time.perf_counter(); moves = d.plan_grouping(); res["plan_grouping_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        dev_ms, host_ms = timed(ev, lambda: d.move_streams(moves))
        d.sync()
        gb = len(moves) * d.snapshot_sizes(0, 1)[1] / 1e9
        res.update(entries=len(moves), moved_gb=round(gb, 3), move_device_ms=round(dev_ms, 3), move_host_ms=round(host_ms, 3))
        first = wall(launch)      # (the launch that commits the move: new assignment, new launch lists)
        t = time.perf_counter(); again = d.plan_grouping(); res["plan_again_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        assert len(again) == 0 and d.image_count() == 2
        ms = launches()
        res["next_launch_beyond_steady_ms"] = round(first - med([wall(launch) for _ in range(3)]), 3)
    else:
        raise SystemExit(f"unknown mode {mode}")
    res.update(ms=med(ms), min=round(min(ms), 4))
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
        line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES}
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(run_child(config, "scattered", None))
            if parent: b.append(run_child(config, "grouped", parent))
        rec = {"a_scattered_ms": [x["scattered_ms"] for x in a], "b_grouped_ms": [x["ms"] for x in a], "this_build": a[-1]}
        if parent: rec.update(parent_grouped_from_start_ms=[x["ms"] for x in b], parent=b[-1], b_ratio=round(med([x["ms"] for x in a]) / med([x["ms"] for x in b]), 4))
        else: rec["parent"] = "skipped: PARENT_LIB not set"
        line.update(rec)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
