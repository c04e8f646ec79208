"""What dspi_process_mixed (include/dspi.h) costs (profiles/mixed_input.md).  bench.py's config 3 (65 536 float streams, 96-frame packets,
FMA contract) and config 5 (16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device buffers, stream-major
words, per-call times by HIP events on the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one context each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says
                so): dspi_process on the bench's 16-bit input
    process     this build, the same call: the same-box spread of row 1
    uniform     this build, dspi_process_mixed with every depth 16            row 1, criterion: uniform / parent <= 1.02 (the fast path is
                                                                              supposed to be the same call)
    half        this build, one context, four calls interleaved, call by call:
                  mixed     dspi_process_mixed, depths 16 / 24 by s % 2
                  intake    the widening pass of that call alone (dspi_debug_intake: the one launch of dspi_intake.hip, timed by itself)
                  widened   dspi_process at 24 bit on the same input widened beforehand (what a caller without the call would feed)
                  copy      a hipMemcpyDtoDAsync of (bytes the intake reads + bytes it writes) / 2 on the same stream: the yardstick of
                            profiles/snapshot.md
                row 2, recorded: intake / copy; beside it (mixed - widened) / copy, the call's time minus the chain's, launch gap included
                row 3, recorded: mixed / widened — the price of the prepass, the number that says whether a fused per-row switch is worth proposing

    python tools/bench_mixed.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=... STREAMS=... PARENT_LIB=...
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("LAUNCHES", 8)), int(os.environ.get("WARMUP", 2))
PACKETS, STREAMS = int(os.environ.get("PACKETS", 0)), int(os.environ.get("STREAMS", 0))
med = lambda v: round(statistics.median(v), 4)


def widen_device(torch, pcm16):
    """int16 [S][F][2] -> uint8 [S][F * 6]: the bytes of s << 8"""
    S = pcm16.shape[0]
    b = pcm16.contiguous().view(torch.uint8).reshape(S, -1, 2)
    w = torch.zeros((S, b.shape[1], 3), dtype=torch.uint8, device=pcm16.device)
    w[:, :, 1:] = b
    return w.reshape(S, -1)


def child(config, leg):
    """one context, LAUNCHES timed rounds of the leg's calls: a JSON line {call: median ms}"""
    import numpy as np
    import time
    import torch
    from bench import HipEvents, PowerSampler, chain_workload, synth_device
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    w = chain_workload(config)
    S, n, B = STREAMS or w["streams"], PACKETS or w["blocks"], w["B"]
    F = n * B
    assert S % 2 == 0
    dev = torch.device("cuda", 0)
    d = Dspi(W.F32_FMA if w["flavor"] else 0, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    if leg == "parent": assert not hasattr(d.L, "dspi_process_mixed"), "PARENT_LIB has the feature: it is not the parent"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    pairs = torch.empty((S, d.P, F, 2), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    outs = (pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    ev = HipEvents(d.hip_stream())
    out = {"streams": S, "frames": F}
    if leg in ("parent", "process"): calls = {"ms": lambda: d.process_device(pcm.data_ptr(), n, B, 16, *outs)}
    elif leg == "uniform":
        depths = np.full(S, 16, dtype=np.uint8)
        calls = {"ms": lambda: d.process_mixed_device(pcm.data_ptr(), depths, n, B, *outs)}
    else:
        depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
        wide = widen_device(torch, pcm)                                   # [S][6F]
        mixed = torch.cat([pcm[0::2].contiguous().view(torch.uint8).reshape(S // 2, -1), wide[1::2]], dim=1).contiguous()      # per pair of streams: 4F + 6F bytes
        total, _ = d.mixed_pcm_bytes(depths, n, B)
        assert total == mixed.numel() == S * F * 5
        moved = (total + S * F * 6) // 2
        src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
        hip = ev.hip
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

        def copy(): assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), moved, ev.stream) == 0
        calls = {"mixed": lambda: d.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs),
                 "intake": lambda: d.debug_intake(mixed.data_ptr(), depths, n, B),
                 "widened": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs), "copy": copy}
        out.update(intake_bytes_read=int(total), intake_bytes_written=S * F * 6, copy_bytes=int(moved))
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    ms = {}
    smi = PowerSampler(0); smi.start()
    t0 = time.perf_counter()
    for i in range(WARMUP + LAUNCHES):
        for k, f in calls.items():
            e0, e1 = ev.new(), ev.new()
            ev.record(e0); f(); ev.record(e1)
            t = ev.elapsed_ms(e0, e1)
            if i >= WARMUP: ms.setdefault(k, []).append(t)
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    smi.stop()
    out.update({k: med(v) for k, v in ms.items()})
    out.update(power_w=pw and round(pw["power_w"], 1), sclk_mhz=pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]), plan={k: v for k, v in d.launch_plan().items() if v})
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
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["process", "uniform", "half"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    half = got["half"]
    line.update(streams=half[-1]["streams"], frames=half[-1]["frames"], plan=half[-1]["plan"],
                intake_bytes_read=half[-1]["intake_bytes_read"], intake_bytes_written=half[-1]["intake_bytes_written"], copy_bytes=half[-1]["copy_bytes"])
    line["ms"] = {k: med([x["ms"] for x in got[k]]) for k in legs if k != "half"}
    for k in ("mixed", "intake", "widened", "copy"): line["ms"][k] = med([x[k] for x in half])
    line["children_ms"] = {k: [x["ms"] for x in got[k]] for k in legs if k != "half"}
    line["children_ms"].update({k: [x[k] for x in half] for k in ("mixed", "intake", "widened", "copy")})
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m = line["ms"]
    line["uniform_over_process"] = round(m["uniform"] / m["process"], 4)
    line["row2_intake_over_copy"] = round(m["intake"] / m["copy"], 4)
    line["intake_tb_per_s"] = round((line["intake_bytes_read"] + line["intake_bytes_written"]) / m["intake"] / 1e9, 3)
    line["call_minus_chain_ms"] = round(m["mixed"] - m["widened"], 4)
    line["call_minus_chain_over_copy"] = round((m["mixed"] - m["widened"]) / m["copy"], 4)
    line["row3_mixed_over_widened"] = round(m["mixed"] / m["widened"], 4)
    if parent:
        line["row1_uniform_over_parent"] = round(m["uniform"] / m["parent"], 4)
        line["process_over_parent"] = round(m["process"] / m["parent"], 4)
        line["criterion_row1_le_1.02"] = line["row1_uniform_over_parent"] <= 1.02
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3])
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
