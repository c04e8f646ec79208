"""What dspi_process_pdm (include/dspi.h) costs and saves against the two calls it replaces (profiles/pdm_out.md).  bench.py's config 3
(65 536 float streams, 96-frame packets, FMA contract) and config 5 (16 384 Q28 streams, 48-frame packets), 50 packets per call, device
buffers, stream-major words, per-call times by HIP events on the context's stream after a warm-up, medians.

Against the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it only this build is timed and the line says so):
alternating child processes, one context each, ROUNDS times, and the median over the children's medians.  A child times three calls
interleaved, call by call, on one context and one set of buffers — the same device work in the same order in every child, so that clocks
and temperature treat all of them alike (the modulator is the heaviest integer kernel here: what runs before a call moves its time by
several percent):
    old child (this build and the parent):   process, modulate, two_calls
    new child (this build):                  process, modulate, pdm_out          and then, in a loop of its own, pdm_out_ns
    process     dspi_process alone                                         criterion (c): this / parent within 1.02, old children
    modulate    dspi_pdm_modulate alone, on the sub words of `process`     criterion (c): this / parent within 1.02, old children
    two_calls   dspi_process, then dspi_pdm_modulate, as one timed span
    pdm_out     dspi_process_pdm with out->sub
    pdm_out_ns  dspi_process_pdm without out->sub: the library's scratch
in two settings:
    all         every stream's sub on                                      criterion (a): pdm_out / the parent's two_calls <= 1.02
    eighth      the sub on for s % 8 == 3 only (per-stream requests)       criterion (b): the parent's two_calls / pdm_out > 1.02
and the modulator's own share, pdm_out - process of the new child, in both settings.

    python tools/bench_pdm_out.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=50 STREAMS=... PARENT_LIB=...
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("LAUNCHES", 8)), int(os.environ.get("WARMUP", 2))
PACKETS, STREAMS = int(os.environ.get("PACKETS", 50)), int(os.environ.get("STREAMS", 0))
med = lambda v: round(statistics.median(v), 4)


def child(config, setting, kind):
    """one context, the calls of an `old` or a `new` child interleaved LAUNCHES times: a JSON line {call: median ms}"""
    import torch
    from bench import HipEvents, chain_workload, synth_device
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    w = chain_workload(config)
    S, n, B = STREAMS or w["streams"], PACKETS, w["B"]
    F = n * B
    dev = torch.device("cuda", 0)
    C_, N = W.dims(w["flavor"])[:2]
    d = Dspi(W.F32_FMA if w["flavor"] else 0, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    R = W.REQ
    for o in range(2, N - 1): d.vendor_set(R["SET_OUTPUT_ENABLE"], o, b"\x00")      # the interlock refuses the sub while outputs 2..N-2 are on
    d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01")
    assert d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=S - 1) == b"\x01"
    if setting == "eighth":
        for s in range(S):
            if s % 8 != 3: d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x00", stream=s)
        assert d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=3) == b"\x01" and d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=4) != b"\x01"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    pairs = torch.empty((S, d.P, F, 2), dtype=torch.int32, device=dev)
    sub = torch.zeros((S, F), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    words = torch.empty((S, F, 8), dtype=torch.int32, device=dev)
    process = lambda: d.process_device(pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    modulate = lambda: d.pdm_device(sub.data_ptr(), F, words.data_ptr())
    loops = [{"process": process, "modulate": modulate, "two_calls": lambda: (process(), modulate())}]
    if kind == "new":
        loops[0]["pdm_out"] = lambda: d.process_pdm_device(pcm.data_ptr(), n, B, words.data_ptr(), 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
        del loops[0]["two_calls"]
        loops.append({"pdm_out_ns": lambda: d.process_pdm_device(pcm.data_ptr(), n, B, words.data_ptr(), 16, pairs.data_ptr(), 0, peaks.data_ptr())})
    ev = HipEvents(d.hip_stream())
    ms = {}
    for calls in loops:
        for f in calls.values(): f()
        d.sync()
        for i in range(WARMUP + LAUNCHES):
            for k, f in calls.items():
                e0, e1 = ev.new(), ev.new()
                ev.record(e0); f(); ev.record(e1)
                t = ev.elapsed_ms(e0, e1)
                if i >= WARMUP: ms.setdefault(k, []).append(t)
    out = {k: med(v) for k, v in ms.items()}
    out.update(streams=S, frames=F, plan={k: v for k, v in d.launch_plan().items() if v}, images=d.image_count())
    if hasattr(d.L, "dspi_pdm_running"): out["running"] = int(d.pdm_running().sum())
    print(json.dumps(out), flush=True)
    d.close()


def run_child(config, setting, kind, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, setting, kind], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {setting} ({lib or 'this build'}): {out.stderr[-600:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP, "packets": PACKETS}
    for setting in ("all", "eighth"):
        new, old, theirs = [], [], []
        for _ in range(ROUNDS):
            new.append(run_child(config, setting, "new", None)); old.append(run_child(config, setting, "old", None))
            if parent: theirs.append(run_child(config, setting, "old", parent))
        m = {k: med([x[k] for x in new]) for k in ("process", "modulate", "pdm_out", "pdm_out_ns")}
        o = {k: med([x[k] for x in old]) for k in ("process", "modulate", "two_calls")}
        rec = {"this_build_new_child_ms": m, "this_build_old_child_ms": o, "children_ms": {"new": [x["pdm_out"] for x in new], "old": [x["two_calls"] for x in old]},
               "streams": new[-1]["streams"], "frames": new[-1]["frames"], "plan": new[-1]["plan"], "images": new[-1]["images"],
               "running": new[-1]["running"], "modulator_share_ms": round(m["pdm_out"] - m["process"], 4), "pdm_out_over_own_two_calls": round(m["pdm_out"] / o["two_calls"], 4)}
        if parent:
            p = {k: med([x[k] for x in theirs]) for k in ("process", "modulate", "two_calls")}
            rec["parent_ms"] = p
            rec["children_ms"]["parent"] = [x["two_calls"] for x in theirs]
            rec["pdm_out_over_parent_two_calls"] = round(m["pdm_out"] / p["two_calls"], 4)
            rec["parent_two_calls_over_pdm_out"] = round(p["two_calls"] / m["pdm_out"], 4)
            rec["process_over_parent"] = round(o["process"] / p["process"], 4)
            rec["modulate_over_parent"] = round(o["modulate"] / p["modulate"], 4)
        else: rec["parent_ms"] = "skipped: PARENT_LIB not set"
        line[setting] = rec
    line["modulator_share_eighth_over_all"] = round(line["eighth"]["modulator_share_ms"] / line["all"]["modulator_share_ms"], 4)
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3], sys.argv[4])
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
