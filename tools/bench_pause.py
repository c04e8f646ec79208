"""What paused streams (dspi_pause_streams / dspi_resume_streams, include/dspi.h) cost and save (profiles/pause.md).  bench.py's config 3
(65 536 float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major words) and config 5 (16 384 Q28 streams), device
buffers, per-launch times by HIP events on the contexts' streams after a warm-up, medians, shader clock and socket power per phase.

Against the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it these two parts are skipped and the line says so)
— alternating child processes, one context each, ROUNDS times: this build, then the parent, and the median over the children's medians:
    half     this build, the upper half of the rows paused          against     the parent, a context of half the streams
    full     this build, nothing paused                             against     the parent, the same context
In one process, this build alone, contexts alternating launch by launch (the method of tools/bench_snapshot.py --realign=cost), every ratio
against the undisturbed context `a` of its own phase:
    r        one stream per row paused for three launches, then resumed (default: realigned)
    r_as_is  the same with DSPI_RESUME_AS_IS
    e        every second stream paused: every float lane on the one-stream kernel
and the host time of dspi_pause_streams / dspi_resume_streams and of the next call's replan for 1, 128 and all streams, and a default resume
of the whole context (HIP events) beside dspi_realign_streams.

    python tools/bench_pause.py [3 5]        ROUNDS=3 LAUNCHES=15 WARMUP=3 PARENT_LIB=...
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("LAUNCHES", 15)), int(os.environ.get("WARMUP", 3))
med = lambda v: round(statistics.median(v), 4)


def setup(config, streams=None):
    import torch
    from bench import chain_workload, synth_device
    from dspi_amd import wire as W
    w = chain_workload(config)
    S = streams or w["streams"]
    frames = w["blocks"] * w["B"]
    dev = torch.device("cuda", 0)
    _, N, P, _, _ = W.dims(w["flavor"])
    pcm = synth_device(torch, dev, S, frames, w["fs"], 1234, True, 0)
    out = (torch.empty((S, P, frames, 2), dtype=torch.int32, device=dev), torch.empty((S, frames), dtype=torch.int32, device=dev),
           torch.empty((S, w["blocks"], 2 + N), dtype=torch.int16, device=dev))
    return w, S, pcm, out


def new_context(w, S):
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    d = Dspi(W.F32_FMA if w["flavor"] else 0, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    return d


def child(config, mode):
    """one context, LAUNCHES timed launches: a JSON line {ms: median per launch}"""
    from bench import HipEvents, PowerSampler, chain_workload
    full = chain_workload(config)["streams"]
    w, S, pcm, (pairs, sub, peaks) = setup(config, full // 2 if mode == "small" else full)
    d = new_context(w, S)
    launch = lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    launch(); d.sync()
    if mode == "half": d.pause_streams(S // 2, S // 2)
    ev = HipEvents(d.hip_stream())
    smi = PowerSampler(0); smi.start()
    ms = []
    for i in range(WARMUP + LAUNCHES):
        if i == WARMUP: t0 = time.perf_counter()
        e0, e1 = ev.new(), ev.new()
        ev.record(e0); launch(); ev.record(e1)
        t = ev.elapsed_ms(e0, e1)
        if i >= WARMUP: ms.append(t)
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    smi.stop()
    print(json.dumps({"ms": med(ms), "min": round(min(ms), 4), "plan": {k: v for k, v in d.launch_plan().items() if v}, "streams": S,
                      "power_w": pw and round(pw["power_w"], 1), "sclk_mhz": pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])}), flush=True)
    d.close()


def run_child(config, mode, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, mode], env=env, capture_output=True, text=True, timeout=300)
    if out.returncode != 0: raise RuntimeError(f"child {config} {mode} ({lib or 'this build'}): {out.stderr[-400:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def against_parent(config, parent):
    res = {}
    for name, mine, theirs in (("half_paused_over_parent_half_context", "half", "small"), ("nothing_paused_over_parent", "full", "full")):
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(run_child(config, mine, None)); b.append(run_child(config, theirs, parent))
        res[name] = {"this_build_ms": [x["ms"] for x in a], "parent_ms": [x["ms"] for x in b], "ratio": round(med([x["ms"] for x in a]) / med([x["ms"] for x in b]), 4),
                     "this_build_plan": a[-1]["plan"], "parent_plan": b[-1]["plan"], "sclk_mhz": [a[-1]["sclk_mhz"], b[-1]["sclk_mhz"]], "power_w": [a[-1]["power_w"], b[-1]["power_w"]]}
    return res


def in_process(config):
    from bench import HipEvents, PowerSampler
    w, S, pcm, (pairs, sub, peaks) = setup(config)
    launch = lambda d: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    names = ["a", "r", "r_as_is", "e"]
    ctx = {k: new_context(w, S) for k in names}
    R = ctx["a"].tile_streams()
    for d in ctx.values():
        for _ in range(2): launch(d)
        d.sync()
    for k in ("r", "r_as_is"):
        for row in range(S // R): ctx[k].pause_streams(row * R + 5, 1)
    for k in names:
        for _ in range(3): launch(ctx[k])
        ctx[k].sync()
    out = {"config": config, "streams": S, "rows": S // R, "launches": LAUNCHES, "warmup": WARMUP}
    t = time.perf_counter()
    ctx["r"].resume_streams(0, S); ctx["r"].sync()
    out["resume_one_per_row_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    ctx["r_as_is"].resume_streams(0, S, as_is=True)
    for s in range(0, S, 2): ctx["e"].pause_streams(s, 1)
    distinct = lambda d: len(set(zip(*[v[:R].tolist() for v in d.stream_positions(0, R)])))
    out["distinct_positions_row0"] = {k: distinct(ctx[k]) for k in ("a", "r", "r_as_is")}
    evs = {k: HipEvents(d.hip_stream()) for k, d in ctx.items()}
    smi = PowerSampler(0); smi.start()
    out["process_ms"], out["over_a"], out["power_w"], out["sclk_mhz"] = {}, {}, {}, {}
    for phase, order in (("resumed", ["a", "r", "r_as_is"]), ("every_second_paused", ["a", "e"])):
        ms = {k: [] for k in order}
        for i in range(WARMUP + LAUNCHES):
            if i == WARMUP: t0 = time.perf_counter()
            for k in order:
                ev = evs[k]
                e0, e1 = ev.new(), ev.new()
                ev.record(e0); launch(ctx[k]); ev.record(e1)
                v = ev.elapsed_ms(e0, e1)
                if i >= WARMUP: ms[k].append(v)
        pw = smi.window(t0, time.perf_counter()) if smi.ok else None
        out["power_w"][phase], out["sclk_mhz"][phase] = pw and round(pw["power_w"], 1), pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])
        out["process_ms"][phase] = {k: {"median": med(v), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}
        out["over_a"].update({k: round(med(ms[k]) / med(ms["a"]), 4) for k in order if k != "a"})
    smi.stop()
    out["plans"] = {k: {p: n for p, n in d.launch_plan().items() if n} for k, d in ctx.items()}
    # the calls themselves on context a: host time of the call, and of the next dspi_process (replan, uploads) beyond a steady one
    d, ev = ctx["a"], evs["a"]
    def wall(fn):
        t = time.perf_counter(); fn(); d.sync()
        return (time.perf_counter() - t) * 1e3
    steady = med([wall(lambda: launch(d)) for _ in range(5)])
    out["calls_ms"] = {"steady_launch_wall": round(steady, 3)}
    for n in (1, 128, S):
        rec = {}
        rec["pause"] = round(wall(lambda: d.pause_streams(0, n)), 3)
        rec["next_launch_beyond_steady"] = round(wall(lambda: launch(d)) - (steady if n < S else 0.0), 3)
        launch(d); d.sync()
        e0, e1 = ev.new(), ev.new()
        t = time.perf_counter(); ev.record(e0); d.resume_streams(0, n); ev.record(e1)
        rec["resume_call_host"] = round((time.perf_counter() - t) * 1e3, 3)
        rec["resume_device"] = round(ev.elapsed_ms(e0, e1), 3)
        rec["next_launch_beyond_steady_after_resume"] = round(wall(lambda: launch(d)) - steady, 3)
        out["calls_ms"][str(n)] = rec
    e0, e1 = ev.new(), ev.new()
    ev.record(e0); d.realign_streams(0, S); ev.record(e1)
    out["calls_ms"]["realign_streams_whole_context_device"] = round(ev.elapsed_ms(e0, e1), 3)
    for d in ctx.values(): d.close()
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3])
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        line = {"config": config, "rounds": ROUNDS}
        line["against_parent"] = against_parent(config, os.path.abspath(parent)) if parent else "skipped: PARENT_LIB not set"
        if "--no-in-process" not in sys.argv: line.update(in_process(config))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
