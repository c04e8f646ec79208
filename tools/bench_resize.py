"""What resizing a context (dspi_resize_streams / dspi_reserve_streams, include/dspi.h) costs (profiles/resize.md).  bench.py's config 3
(65 536 float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major words) and config 5 (16 384 Q28 streams), device
buffers, launch times by HIP events on the contexts' own streams after a warm-up, medians, shader clock and socket power per child.

Everything is a child process with one context; alternating children, ROUNDS times, the ratio of the medians of the children's medians:
    1  realloc    config 3 at half its streams: the reallocating grow to all of them and dspi_reserve_streams trimming back, host wall time
                  (both calls wait for the stream once), beside a hipMemcpyDtoDAsync of the surviving bytes and the runtime's own
                  hipMalloc + hipFree of the new arrays' sizes                                                    recorded, not gated
    2  grown      config 3 created at half its streams and grown to all, the usual setup, launches   against   created, a context
                  created at the full size                                                                        within 1.02
    3  created    configs 3 and 5, this build                        against   the PARENT commit's library (PARENT_LIB=<its libdspi_mi355x.so>)   within 1.02
    4  within     config 3, capacity reserved for 128 more: the grow by 128 slots (asynchronous)   beside   dspi_boot_streams of the same slots   recorded

    python tools/bench_resize.py [3 5]        ROUNDS=3 LAUNCHES=10 WARMUP=3 REPS=4 PARENT_LIB=...
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
from bench_boot import boot_bytes, timed        # noqa: E402

ROUNDS, LAUNCHES, WARMUP, REPS = (int(os.environ.get(k, v)) for k, v in (("ROUNDS", 3), ("LAUNCHES", 10), ("WARMUP", 3), ("REPS", 4)))
med = lambda v: round(statistics.median(v), 4)


def wall(fn):
    t = time.perf_counter(); fn()
    return (time.perf_counter() - t) * 1e3


def child(config, mode):
    """one context: a JSON line"""
    import numpy as np
    import torch
    from bench import HipEvents, PowerSampler, hip_runtime
    w, S, pcm, (pairs, sub, peaks) = setup(config)
    half = S // 2
    d = new_context(w, half if mode in ("realloc", "grown") else S)
    R = d.tile_streams()
    launch = lambda: d.process_device(pcm.data_ptr(), w["blocks"], w["B"], 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    usual = lambda: (d.set_rate(w["fs"]), d.set_volume(w["vol"]), d.load_bulk(w["blob"]))
    ev = HipEvents(d.hip_stream())
    res = {"streams": S}
    smi = PowerSampler(0); smi.start()
    t0 = time.perf_counter()
    if mode == "realloc":
        launch(); d.sync()
        grow, trim = [], []
        for i in range(1 + REPS):
            g = wall(lambda: d.resize_streams(S))
            assert d.stream_capacity() == S
            d.pause_streams(half, half); d.resize_streams(half)
            t = wall(lambda: d.reserve_streams(half))
            assert d.stream_capacity() == half
            if i: grow.append(g); trim.append(t)
        kept, made = boot_bytes(w["flavor"], half, R), boot_bytes(w["flavor"], S, R)      # (the PDM words are part of it only once the modulator has run: 9 words in 39 178)
        res.update(grow_ms=med(grow), trim_ms=med(trim), kept_gb=round(kept / 1e9, 3), new_arrays_gb=round(made / 1e9, 3))
        hip = hip_runtime()
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]; hip.hipFree.argtypes = [ctypes.c_void_p]
        src, dst = torch.empty(kept // 4, dtype=torch.int32, device="cuda"), torch.empty(kept // 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        copies = []
        for i in range(2 + REPS):
            v, _ = timed(ev, lambda: hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), kept, d.hip_stream()))
            d.sync()
            if i >= 2: copies.append(v)
        del src, dst
        mallocs, frees = [], []
        for i in range(1 + REPS):      # the runtime's own share of a reallocation: the new arrays' bytes, allocated and freed
            p = ctypes.c_void_p()
            m = wall(lambda: hip.hipMalloc(ctypes.byref(p), made)); f = wall(lambda: hip.hipFree(p))
            if i: mallocs.append(m); frees.append(f)
        res.update(copy_ms=med(copies), copy_tb_per_s=round(2 * kept / 1e9 / med(copies), 3), malloc_ms=med(mallocs), free_ms=med(frees),
                   grow_over_copy=round(med(grow) / med(copies), 3), trim_over_copy=round(med(trim) / med(copies), 3))
    elif mode in ("created", "grown"):
        if mode == "grown":
            launch(); d.sync()
            d.resize_streams(S); usual()
        launch(); d.sync()
        res["images"] = d.image_count()
        ms = []
        for i in range(WARMUP + LAUNCHES):
            v, _ = timed(ev, launch)
            if i >= WARMUP: ms.append(v)
        res.update(ms=med(ms), min=round(min(ms), 4))
    elif mode == "within":
        assert d.reserve_streams(S + 128) >= S + 128
        launch(); d.sync()
        new = np.arange(S, S + 128, dtype=np.uint32)
        grow, grow_host, boot, boot_host = [], [], [], []
        for i in range(2 + REPS):
            g, gh = timed(ev, lambda: d.resize_streams(S + 128)); d.sync()
            b, bh = timed(ev, lambda: d.boot_streams(new)); d.sync()
            d.pause_streams(S, 128); d.resize_streams(S)
            if i >= 2: grow.append(g); grow_host.append(gh); boot.append(b); boot_host.append(bh)
        res.update(grow_ms=med(grow), grow_host_ms=med(grow_host), boot_ms=med(boot), boot_host_ms=med(boot_host))
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
        runs = {"created": [], "parent": []}
        if config == "3": runs.update(grown=[], realloc=[], within=[])
        for _ in range(ROUNDS):
            for mode in runs:
                if mode == "parent":
                    if parent: runs[mode].append(run_child(config, "created", parent))
                else: runs[mode].append(run_child(config, mode, None))
        created = med([x["ms"] for x in runs["created"]])
        line["created"] = {"ms": [x["ms"] for x in runs["created"]], "last": runs["created"][-1]}
        if parent: line["created_over_parent"] = {"parent_ms": [x["ms"] for x in runs["parent"]], "ratio": round(created / med([x["ms"] for x in runs["parent"]]), 4)}
        else: line["created_over_parent"] = "skipped: PARENT_LIB not set"
        if config == "3":
            line["grown_over_created"] = {"ms": [x["ms"] for x in runs["grown"]], "last": runs["grown"][-1], "ratio": round(med([x["ms"] for x in runs["grown"]]) / created, 4)}
            line["realloc"] = runs["realloc"]
            line["within"] = runs["within"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
