"""What per-stream S/PDIF block positions (dspi_spdif_per_stream, include/dspi.h) cost (profiles/spdif_pos.md).  Every figure is a child
process with one context; children alternate, ROUNDS times; a ratio is the ratio of the medians of the children's medians, and the yardstick
is the PARENT commit's library on the same box (PARENT_LIB=<its libdspi_mi355x.so>), as in profiles/pause.md.

    process 3 / process 5   DSPI_OUT_SPDIF on bench.py's config 3 (65 536 float streams, 50 x 96 frames) and config 5 (16 384 Q28 streams),
                            device buffers, HIP events on the context's stream: this build with the mode off, this build with the mode on
                            (distinct positions), the parent
    encode                  the encoder alone, 65 536 streams x 4 pairs x 2 400 frames, stream-major, device buffers: dspi_spdif_encode on this
                            build and on the parent, dspi_spdif_encode_v on this build
    latency                 one float stream, one 48-frame packet per call on host buffers with DSPI_OUT_SPDIF (the latency layout): the
                            parent's fused encoder, this build with the mode off (the same fused encoder) and with the mode on (the forced
                            second pass): p50 / p99 of CALLS calls, host clock around the call (it returns when the words are in place)
Criterion: mode off over parent within 1.02 on process 3, process 5 and encode.  Everything else is recorded.

    python tools/bench_spdif_pos.py        ROUNDS=3 LAUNCHES=15 WARMUP=3 CALLS=5000 PARENT_LIB=...
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

ROUNDS, LAUNCHES, WARMUP, CALLS = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("LAUNCHES", 15), ("WARMUP", 3), ("CALLS", 5000)))
med = lambda v: round(statistics.median(v), 4)


def mode_on(d):
    import numpy as np
    d.spdif_per_stream(1)
    d.spdif_stream_pos(set=(np.arange(d.n_streams) * 7 + 5) % 192)


def event_times(d, step):
    from bench import HipEvents, PowerSampler
    ev = HipEvents(d.hip_stream())
    smi = PowerSampler(0); smi.start()
    ms = []
    for i in range(WARMUP + LAUNCHES):
        if i == WARMUP: t0 = time.perf_counter()
        e0, e1 = ev.new(), ev.new()
        ev.record(e0); step(); ev.record(e1)
        t = ev.elapsed_ms(e0, e1)
        if i >= WARMUP: ms.append(t)
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    smi.stop()
    return {"ms": med(ms), "min": round(min(ms), 4), "power_w": pw and round(pw["power_w"], 1), "sclk_mhz": pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])}


def child(what, arg, variant):
    """one context: a JSON line.  variant: off / on (this build's mode) / v (dspi_spdif_encode_v)"""
    import numpy as np
    import torch
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    dev = torch.device("cuda", 0)
    if what == "process":
        from bench_pause import new_context, setup
        w, S, pcm, (_, sub, peaks) = setup(arg)
        frames = w["blocks"] * w["B"]
        d = new_context(w, S)
        words = torch.empty((S, d.P, frames, 4), dtype=torch.int32, device=dev)
        if variant == "on": mode_on(d)
        res = event_times(d, lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, words.data_ptr(), sub.data_ptr(), peaks.data_ptr(), spdif=True))
        res.update(streams=S, plan={k: v for k, v in d.launch_plan().items() if v})
    elif what == "encode":
        S, F = 65536, 2400
        d = Dspi(W.F32_FMA, S, device=0); d.set_rate(96000)
        pairs = torch.randint(-(1 << 23), 1 << 23, (S, d.P, F, 2), dtype=torch.int32, device=dev)
        out = torch.empty((S, d.P, F, 4), dtype=torch.int32, device=dev)
        pos = torch.from_numpy(((np.arange(S) * 7 + 5) % 192).astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        if variant == "v": step = lambda: d.spdif_encode_v_device(pairs.data_ptr(), F, pos.data_ptr(), out.data_ptr())
        else: step = lambda: d.spdif_device(pairs.data_ptr(), F, 5, out.data_ptr())
        res = event_times(d, step)
        res.update(streams=S, frames=F, tb_per_s=round(S * F * 96 / res["ms"] / 1e9, 3))
    elif what == "latency":
        from dspi_amd import workloads as WL
        S, B, fs = 1, 48, 48000
        d = Dspi(W.F32_FMA, S, device=0); d.set_rate(fs); d.set_volume(-20 * 256)
        assert d.load_bulk(WL.full_chain_blob(W.F32_FMA)) == 0
        if variant == "on": mode_on(d)
        pcm = WL.synth_pcm16(S, B, fs)
        out = (np.zeros((S, d.P, B, 4), dtype=np.uint32), np.zeros((S, B), dtype=np.int32), np.zeros((S, 1, d.C), dtype=np.uint16))
        us = []
        for i in range(200 + CALLS):
            t = time.perf_counter()
            d.process_host(pcm, 1, B, 16, out=out, spdif=True)
            if i >= 200: us.append((time.perf_counter() - t) * 1e6)
        us.sort()
        res = {"p50_us": round(us[len(us) // 2], 1), "p99_us": round(us[len(us) * 99 // 100], 1), "calls": CALLS, "plan": {k: v for k, v in d.launch_plan().items() if v},
               "direct_calls": d.direct_stats()["calls"]}
    else:
        raise SystemExit(f"unknown measurement {what}")
    print(json.dumps(res), flush=True)
    d.close()


def run_child(what, arg, variant, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, arg, variant], env=env, capture_output=True, text=True, timeout=400)
    if out.returncode != 0: raise RuntimeError(f"child {what} {arg} {variant} ({lib or 'this build'}): {out.stderr[-600:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(*sys.argv[2:5])
    parent = os.environ.get("PARENT_LIB")
    parent = os.path.abspath(parent) if parent else None
    wanted = [a for a in sys.argv[1:] if not a.startswith("--")] or ["process:3", "process:5", "encode", "latency"]
    for item in wanted:
        what, _, arg = item.partition(":")
        arg = arg or "-"
        variants = [("mode_off", "off", None), ("mode_on", "v" if what == "encode" else "on", None)] + ([("parent", "off", parent)] if parent else [])
        runs = {name: [] for name, _, _ in variants}
        for _ in range(ROUNDS):
            for name, variant, lib in variants: runs[name].append(run_child(what, arg, variant, lib))
        key = "p50_us" if what == "latency" else "ms"
        line = {"what": item, "rounds": ROUNDS, "launches": LAUNCHES}
        for name in runs:
            line[name] = {key: [x[key] for x in runs[name]], "last": runs[name][-1]}
            if what == "latency": line[name]["p99_us"] = [x["p99_us"] for x in runs[name]]
        if parent:
            for name in ("mode_off", "mode_on"): line[name + "_over_parent"] = round(med([x[key] for x in runs[name]]) / med([x[key] for x in runs["parent"]]), 4)
        else: line["parent"] = "skipped: PARENT_LIB not set"
        line["mode_on_over_mode_off"] = round(med([x[key] for x in runs["mode_on"]]) / med([x[key] for x in runs["mode_off"]]), 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
