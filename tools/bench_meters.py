"""What the meter bridge (include/dspi.h: dspi_meters_update, dspi_meters_alarms, dspi_status_all, dspi_clear_clips_list) costs, and that the
call it stands behind costs what it did (profiles/meters.md).  tools/bench_link.py's method and helpers: bench.py's config 3 (65 536 float
streams, 96-frame packets, FMA contract) and config 5 (16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device
buffers, per-call times by HIP events on the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so):
                p16 = dspi_process at 16 bit with out->peaks given; then, by the wall clock, once: dspi_get_status for every stream, one call
                each (poll_status), and dspi_clear_clips for every stream, one call each (poll_clear) — what a context's poll costs there
    same        this build, p16                                           GATED: same / parent within 1.02
    meters      this build, behind one p16 call, interleaved:
                  update     dspi_meters_update on the call's device peaks (hold 300, decay 32000)
                  copy       a hipMemcpyDtoDAsync of the same peaks bytes
                  alarms     dspi_meters_alarms on device buffers, the level at the median of the streams' loudest meter, cap = every stream
                  status     dspi_status_all of every stream into device memory
                  clear      dspi_clear_clips_list of every stream (the list goes up from host memory inside the call)
                RECORDED: update / copy; the launch times; by the wall clock (call until the host has the result) status_host, alarms_host
                and clear + dspi_sync; and whether the device words agree with the CPU paths at this size (update: every word; alarms: list,
                info and total)

    python tools/bench_meters.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=...
"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_link import LAUNCHES, ROUNDS, WARMUP, make, med, outputs, timed, workload      # noqa: E402


def child_gated(config, leg):
    import torch
    from bench import HipEvents, synth_device
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    if leg == "parent": assert not hasattr(d.L, "dspi_meters_update"), "PARENT_LIB has the feature: it is not the parent"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    keep, outs = outputs(torch, dev, d, S, n, F)
    calls = {"p16": lambda: d.process_device(pcm.data_ptr(), n, B, 16, *outs)}
    out = {"streams": S, "frames": F}
    torch.cuda.synchronize()
    calls["p16"]()
    d.sync()
    timed(HipEvents(d.hip_stream()), calls, d, out)
    if leg == "parent":      # the poll of a context as it is made without the bridge: one call per stream
        buf = ctypes.create_string_buffer(d.C * 2 + 4)
        t0 = time.perf_counter()
        for s in range(S): d.L.dspi_get_status(d.h, s, buf, len(buf))
        t1 = time.perf_counter()
        for s in range(S): d.L.dspi_clear_clips(d.h, s)
        out.update(poll_status=round((t1 - t0) * 1e3, 2), poll_clear=round((time.perf_counter() - t1) * 1e3, 2))
    print(json.dumps(out), flush=True)
    d.close()


def child_meters(config):
    import numpy as np
    import torch
    from bench import HipEvents, synth_device
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    keep, outs = outputs(torch, dev, d, S, n, F)
    peaks = keep[2]
    hold, decay = 300, 32000
    meters = torch.zeros((S, d.C), dtype=torch.int32, device=dev)
    t_streams, t_info, t_total = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    t_status = torch.zeros(S * (2 * d.C + 4), dtype=torch.uint8, device=dev)
    peaks_copy = torch.empty_like(peaks)
    every = np.arange(S, dtype=np.uint32)
    torch.cuda.synchronize()
    d.process_device(pcm.data_ptr(), n, B, 16, *outs)
    # the device words against the CPU paths, at this size
    d.meters_update_device(peaks.data_ptr(), n, meters.data_ptr(), hold, decay)
    d.sync()
    h_peaks = peaks.cpu().numpy().view(np.uint16)
    h_meters = d.meters_update_host(h_peaks, np.zeros((S, d.C), dtype=np.uint32), hold, decay)
    agree_update = bool(np.array_equal(meters.cpu().numpy().view(np.uint32), h_meters))
    level = int(np.median((h_meters & 0xffff).max(axis=1)))
    hs, hi, ht = d.meters_alarms_host(h_meters, level)
    d.meters_alarms_device(meters.data_ptr(), level, t_streams.data_ptr(), t_info.data_ptr(), S, t_total.data_ptr())
    d.sync()
    total = int(t_total.cpu().numpy().view(np.uint32)[0])
    agree_alarms = bool(total == ht and np.array_equal(t_streams.cpu().numpy().view(np.uint32)[:total], hs) and np.array_equal(t_info.cpu().numpy().view(np.uint32)[:total], hi))
    d.status_all_device(t_status.data_ptr(), t_status.numel())
    d.sync()
    agree_status = bool(np.array_equal(t_status.cpu().numpy().reshape(S, -1), d.status_all()))
    ev = HipEvents(d.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    peak_bytes = peaks.numel() * 2
    calls = {"update": lambda: d.meters_update_device(peaks.data_ptr(), n, meters.data_ptr(), hold, decay),
             "copy": lambda: hip.hipMemcpyDtoDAsync(peaks_copy.data_ptr(), peaks.data_ptr(), peak_bytes, ev.stream),
             "alarms": lambda: d.meters_alarms_device(meters.data_ptr(), level, t_streams.data_ptr(), t_info.data_ptr(), S, t_total.data_ptr()),
             "status": lambda: d.status_all_device(t_status.data_ptr(), t_status.numel()),
             "clear": lambda: d.clear_clips_list(every)}
    out = {"streams": S, "frames": F, "packets": n, "peak_bytes": peak_bytes, "alarmed": total, "agree_update": agree_update, "agree_alarms": agree_alarms, "agree_status": agree_status}
    timed(ev, calls, d, out)
    wall = {"status_host_wall": [], "alarms_host_wall": [], "clear_sync_wall": []}
    for i in range(WARMUP + LAUNCHES):
        for name, f in (("status_host_wall", lambda: d.status_all()), ("alarms_host_wall", lambda: d.meters_alarms_host(h_meters, level)),
                        ("clear_sync_wall", lambda: (d.clear_clips_list(every), d.sync()))):
            t0 = time.perf_counter(); f()
            if i >= WARMUP: wall[name].append((time.perf_counter() - t0) * 1e3)
    out.update({k: med(v) for k, v in wall.items()})
    print(json.dumps(out), flush=True)
    d.close()


def run_child(config, leg, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, leg], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {leg} ({lib or 'this build'}): {out.stderr[-800:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["same", "meters"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs:
            got[k].append(run_child(config, k, parent if k == "parent" else None))
            print(f"config {config}: leg {k} done", file=sys.stderr, flush=True)
    skip = ("streams", "frames", "packets", "peak_bytes", "alarmed", "agree_update", "agree_alarms", "agree_status", "power_w", "sclk_mhz")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m, mt = line["ms"], got["meters"][-1]
    line["meters"] = {"streams": mt["streams"], "packets": mt["packets"], "peak_bytes": mt["peak_bytes"], "alarmed": mt["alarmed"],
                      "device_words_agree_with_cpu_paths": all(x["agree_update"] and x["agree_alarms"] and x["agree_status"] for x in got["meters"]),
                      "update_over_copy_of_same_bytes": round(m["meters.update"] / m["meters.copy"], 3),
                      "update_read_tb_per_s": round(mt["peak_bytes"] / m["meters.update"] / 1e9, 3), "copy_tb_per_s_read_plus_written": round(2 * mt["peak_bytes"] / m["meters.copy"] / 1e9, 3)}
    if parent:
        line["gate_p16_over_parent"] = round(m["same.p16"] / m["parent.p16"], 4)
        line["criterion_gate_within_1.02"] = 1 / 1.02 <= line["gate_p16_over_parent"] <= 1.02
        line["parent_poll_over_bridge"] = {"status": round(m["parent.poll_status"] / m["meters.status_host_wall"], 1), "clear": round(m["parent.poll_clear"] / m["meters.clear_sync_wall"], 1)}
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        return child_meters(config) if leg == "meters" else child_gated(config, leg)
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
