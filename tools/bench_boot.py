"""What booting streams inside a running context (dspi_boot_streams, include/dspi.h) costs (profiles/boot.md).  bench.py's config 3 (65 536
float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major words) and config 5 (16 384 Q28 streams), device buffers,
times by HIP events on the contexts' own streams after a warm-up, medians, shader clock and socket power per child.

Everything is a child process with one context; alternating children, ROUNDS times, the ratio of the medians of the children's medians:
    boot     boot_all    this build: dspi_boot_streams over every stream (NULL dump)    against   import_all, the PARENT commit's library
                                                                                                  (PARENT_LIB=<its libdspi_mi355x.so>) importing a
                                                                                                  device-resident snapshot of power-on streams
    after    booted_all  this build: whole-context boot, the usual setup, then launches  against   full, this build, an undisturbed context
             booted_rows this build: one stream per row booted (default flags) and set up like its neighbours, then launches   against   full
Recorded beside them by boot_all (no criterion): a hipMemsetAsync of the same bytes on the same stream, the boot of one stream per row, the
host time of the calls.

    python tools/bench_boot.py [3 5]        ROUNDS=3 LAUNCHES=10 WARMUP=3 REPS=6 PARENT_LIB=...
"""
import ctypes
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

ROUNDS, LAUNCHES, WARMUP, REPS = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("LAUNCHES", 10), ("WARMUP", 3), ("REPS", 6)))
med = lambda v: round(statistics.median(v), 4)


def timed(ev, fn):
    e0, e1 = ev.new(), ev.new()
    t = time.perf_counter(); ev.record(e0); fn(); ev.record(e1)
    host = (time.perf_counter() - t) * 1e3
    return ev.elapsed_ms(e0, e1), host


def boot_bytes(flavor, S, R):
    """what a whole-context boot stores: per row of R streams the state slots, the delay lines, both rings and the PDM words (dspi_image.h)"""
    n_ch, n_out, line = (11, 9, 4096) if flavor else (7, 5, 2048)
    words = (21 * n_ch + 26) + n_out * line + 2 * 1024 + 9
    return -(-S // R) * R * words * 4


def child(config, mode):
    """one context: a JSON line"""
    import numpy as np
    import torch
    from bench import HipEvents, PowerSampler, hip_runtime
    w, S, pcm, (pairs, sub, peaks) = setup(config)
    d = new_context(w, S)
    R = d.tile_streams()
    launch = lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    usual = lambda stream=-1: (d.set_rate(w["fs"], stream), d.set_volume(w["vol"], stream), d.load_bulk(w["blob"], stream))
    ev = HipEvents(d.hip_stream())
    res = {"streams": S}

    def launches():
        ms = []
        for i in range(WARMUP + LAUNCHES):
            v, _ = timed(ev, launch)
            if i >= WARMUP: ms.append(v)
        return ms

    def repeated(fn, between=None):
        dev, hst = [], []
        for i in range(2 + REPS):
            v, h = timed(ev, fn)
            if i >= 2: dev.append(v); hst.append(h)
            if between: between()
        return dev, hst

    smi = PowerSampler(0); smi.start()
    t0 = time.perf_counter()
    if mode == "import_all":      # (today's only route to power-on state; runs on the parent's library)
        hb, sb = d.snapshot_sizes(0, S)
        state = torch.empty(sb // 4, dtype=torch.int32, device="cuda")
        head = d.export_streams_device(0, S, state.data_ptr(), sb); d.sync()      # (nothing has run yet: power-on state)
        launch(); d.sync()
        dev, hst = repeated(lambda: d.import_streams_device(0, head, state.data_ptr(), sb))
        res.update(ms=med(dev), min=round(min(dev), 4), host_ms=med(hst), gb=round(sb / 1e9, 3))
    elif mode == "boot_all":
        launch(); d.sync()
        everybody = np.arange(S, dtype=np.uint32)
        dev, hst = repeated(lambda: d.boot_streams(everybody))
        nbytes = boot_bytes(w["flavor"], S, R)
        res.update(ms=med(dev), min=round(min(dev), 4), host_ms=med(hst), gb=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / 1e9 / med(dev), 3))
        hip = hip_runtime()
        hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
        buf = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms, _ = repeated(lambda: hip.hipMemsetAsync(buf.data_ptr(), 0, nbytes, d.hip_stream()))
        res.update(memset_ms=med(ms), boot_over_memset=round(med(dev) / med(ms), 4))
        del buf
        usual(); launch(); d.sync()
        rows = np.arange(0, S, R, dtype=np.uint32) + 5
        dev, hst = repeated(lambda: d.boot_streams(rows), between=lambda: (launch(), d.sync()))
        res.update(one_per_row_ms=med(dev), one_per_row_host_ms=med(hst), one_per_row_streams=len(rows))
    elif mode in ("full", "booted_all", "booted_rows"):
        launch(); d.sync()
        if mode == "booted_all":
            d.boot_streams(np.arange(S, dtype=np.uint32)); usual()
        elif mode == "booted_rows":
            rows = np.arange(0, S, R, dtype=np.uint32) + 5
            d.boot_streams(rows)
            for s in rows: usual(int(s))
            launch(); d.sync()
            d.set_volume(w["vol"])      # a broadcast call: the arrivals' object, now equal to their neighbours', folds into it at the next commit
        launch(); d.sync()
        res["images"] = d.image_count()
        ms = launches()
        res.update(ms=med(ms), min=round(min(ms), 4))
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
        line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "reps": REPS}
        boots, imports, runs = [], [], {"full": [], "booted_all": [], "booted_rows": []}
        for _ in range(ROUNDS):
            boots.append(run_child(config, "boot_all", None))
            if parent: imports.append(run_child(config, "import_all", parent))
            for mode in runs: runs[mode].append(run_child(config, mode, None))
        rec = {"this_build_ms": [x["ms"] for x in boots], "this_build": boots[-1]}
        if parent: rec.update(parent_ms=[x["ms"] for x in imports], parent=imports[-1], ratio=round(med([x["ms"] for x in boots]) / med([x["ms"] for x in imports]), 4))
        else: rec["parent"] = "skipped: PARENT_LIB not set"
        line["boot_all_over_parent_import"] = rec
        full = med([x["ms"] for x in runs["full"]])
        line["undisturbed"] = {"ms": [x["ms"] for x in runs["full"]], "last": runs["full"][-1]}
        for mode in ("booted_all", "booted_rows"):
            line[mode + "_over_undisturbed"] = {"ms": [x["ms"] for x in runs[mode]], "last": runs[mode][-1], "ratio": round(med([x["ms"] for x in runs[mode]]) / full, 4)}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
