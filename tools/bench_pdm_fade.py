"""What dspi_pdm_fade (include/dspi.h) costs (profiles/pdm_fade.md).  bench.py's config 3 (65 536 float streams, 96-frame packets, FMA
contract: the float headline size) and config 5 (16 384 Q28 streams, 48-frame packets), 10 packets per call, device buffers, stream-major
words, dspi_process_pdm with out->sub, per-call times by HIP events on the context's stream after a warm-up, medians.

A B A B on one box against the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it only this build is timed and
the line says so): alternating child processes, one context each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the parent's dspi_process_pdm, every stream's sub on
    off         this build, the mode off, every stream's sub on            criterion: off / parent <= 1.02 (the same kernels are launched)
    idle        this build, the mode on, nobody fading                     recorded: one 4-byte store per lane and call more
    stopped     this build, the mode off, one stream in eight's sub off    the yardstick of `fading`: the same per-stream requests (every row then
                                                                           runs the chain kernel with per-lane parameter images), 7/8 of the lanes
    fading      this build, the mode on, one stream in eight fading        recorded: before every call the streams s % 8 == 3 (sub off, byte 1)
                                                                           are put back to fade position 1023 with dspi_pdm_fade_state, outside
                                                                           the timed span; the span holds the rebuilt list's and the aux words'
                                                                           upload, as every call does while somebody fades

    python tools/bench_pdm_fade.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=10 STREAMS=... PARENT_LIB=...
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("LAUNCHES", 8)), int(os.environ.get("WARMUP", 2))
PACKETS, STREAMS = int(os.environ.get("PACKETS", 10)), int(os.environ.get("STREAMS", 0))
med = lambda v: round(statistics.median(v), 4)


def child(config, leg):
    """one context, LAUNCHES timed calls of one leg: a JSON line {ms: median}"""
    import numpy as np
    import torch
    import time
    from bench import HipEvents, PowerSampler, chain_workload, synth_device
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    w = chain_workload(config)
    S, n, B = STREAMS or w["streams"], PACKETS, w["B"]
    F = n * B
    dev = torch.device("cuda", 0)
    N = W.dims(w["flavor"])[1]
    d = Dspi(W.F32_FMA if w["flavor"] else 0, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    R = W.REQ
    for o in range(2, N - 1): d.vendor_set(R["SET_OUTPUT_ENABLE"], o, b"\x00")      # the interlock refuses the sub while outputs 2..N-2 are on
    d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x01")
    assert d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=S - 1) == b"\x01"
    if leg in ("idle", "fading"): assert d.pdm_fade(1) is True
    elif leg in ("off", "stopped"): assert d.pdm_fade() is False
    else: assert not hasattr(d.L, "dspi_pdm_fade"), "PARENT_LIB has the feature: it is not the parent"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    pairs = torch.empty((S, d.P, F, 2), dtype=torch.int32, device=dev)
    sub = torch.zeros((S, F), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    words = torch.empty((S, F, 8), dtype=torch.int32, device=dev)
    call = lambda: d.process_pdm_device(pcm.data_ptr(), n, B, words.data_ptr(), 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    call(); d.sync()
    fade_words = None
    if leg in ("fading", "stopped"):
        for s in range(3, S, 8): d.vendor_set(R["SET_OUTPUT_ENABLE"], N - 1, b"\x00", stream=s)
        assert d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=3) != b"\x01" and d.vendor_get(R["GET_CORE1_MODE"], 0, 1, stream=4) == b"\x01"
        if leg == "stopped": call(); d.sync()
    if leg == "fading":
        fade_words = d.pdm_fade_state()
        fade_words[3::8] = (fade_words[3::8] & 0xFFFF0000) | 1023
    ev = HipEvents(d.hip_stream())
    ms = []
    smi = PowerSampler(0); smi.start()
    t0 = time.perf_counter()
    for i in range(WARMUP + LAUNCHES):
        if fade_words is not None:
            d.pdm_fade_state(set=fade_words); d.pdm_running(set=np.ones(S, dtype=np.uint8))
        e0, e1 = ev.new(), ev.new()
        ev.record(e0); call(); ev.record(e1)
        t = ev.elapsed_ms(e0, e1)
        if i >= WARMUP: ms.append(t)
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    smi.stop()
    out = {"ms": med(ms), "power_w": pw and round(pw["power_w"], 1), "sclk_mhz": pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]), "streams": S, "frames": F, "running": int(d.pdm_running().sum())}
    if fade_words is not None: out["fading_after"] = int((d.pdm_fade_state() & 0xFFFF != 0).sum())
    print(json.dumps(out), flush=True)
    d.close()


def run_child(config, leg, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, leg], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {leg} ({lib or 'this build'}): {out.stderr[-600:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP, "packets": PACKETS}
    legs = (["parent"] if parent else []) + ["off", "idle", "stopped", "fading"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    line.update(streams=got["off"][-1]["streams"], frames=got["off"][-1]["frames"], fading_after=got["fading"][-1]["fading_after"])
    line["ms"] = {k: med([x["ms"] for x in v]) for k, v in got.items()}
    line["children_ms"] = {k: [x["ms"] for x in v] for k, v in got.items()}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    line["idle_over_off"] = round(line["ms"]["idle"] / line["ms"]["off"], 4)
    line["fading_over_off"] = round(line["ms"]["fading"] / line["ms"]["off"], 4)
    line["fading_over_stopped"] = round(line["ms"]["fading"] / line["ms"]["stopped"], 4)
    if parent:
        for k in ("off", "idle", "stopped", "fading"): line[f"{k}_over_parent"] = round(line["ms"][k] / line["ms"]["parent"], 4)
        line["criterion_off_over_parent_le_1.02"] = line["off_over_parent"] <= 1.02
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3])
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
