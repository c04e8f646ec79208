"""What outputs to a packet table (include/dspi.h: dspi_packets_emit) cost, and that the calls they stand beside cost what they did
(profiles/packets_out.md).  tools/bench_packets.py's method and helpers: bench.py's config 3 (65 536 float streams, FMA contract) and config 5
(16 384 Q28 streams), both at 50 packets of 96 frames per call, device buffers, per-call times by HIP events on the context's stream after a
warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so),
                one context, two calls interleaved: p16 = dspi_process at 16 bit, stream-major; ppackets = dspi_process_packets, 24 bit, by the
                table of its own contiguous layout
    same        this build, the same two calls                          GATED: same / parent within 1.02 for each
    emit        this build.  The pair words of one dspi_process call, stream-major and then tiled in the same buffer, and per layout:
                  kernel_{major,tiled}_{32,24}_{identity,shuffled}    dspi_debug_packets_emit_launch: the ONE launch, formats and table already on
                                      the device.  identity: entry (s, p, k) at packet bytes x ((s P + p) NB + k), the packets back to back in
                                      table order; shuffled: the same places, permuted
                  copy_32, copy_24    a hipMemcpyDtoDAsync of the bytes an emit of that format writes: the yardstick
                  call_{major,tiled}_32_identity                      the whole dspi_packets_emit call: the table through the pinned area, its
                                      upload, the launch (the host's copy of the table into the pinned area is the caller's thread's)
                  process_major, process_tiled                        dspi_process into the pair words alone (no sub, no peaks), either layout
                RECORDED: every kernel's time over its copy's; process_tiled + kernel_tiled_32_identity over process_major — whether tiled
                output plus the packetiser beats the stream-major layout outright — and the same with the whole call.  (That the two layouts
                emit the same bytes is the test suite's to show, not the benchmark's.)

    python tools/bench_packets_out.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=...
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_link import LAUNCHES, ROUNDS, WARMUP, make, med, outputs, timed, workload      # noqa: E402

BLOCK_LEN = 96


def sized(config):
    w, flavor, dev = workload(config)
    return dict(w, B=BLOCK_LEN), flavor, dev


def child_gated(config, leg):
    import numpy as np
    import torch
    from bench import HipEvents, synth_device
    from bench_mixed import widen_device
    w, flavor, dev = sized(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    if leg == "parent": assert not hasattr(d.L, "dspi_packets_emit"), "PARENT_LIB has the feature: it is not the parent"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    wide = widen_device(torch, pcm)
    depths = np.full(S, 24, dtype=np.uint8)
    table = (np.arange(S * n, dtype=np.uint64) * np.uint64(6 * B)).reshape(S, n)
    keep, outs = outputs(torch, dev, d, S, n, F)
    calls = {"p16": lambda: d.process_device(pcm.data_ptr(), n, B, 16, *outs),
             "ppackets": lambda: d.process_packets_device(wide.data_ptr(), S * F * 6, depths, table, n, B, *outs)}
    out = {"streams": S, "frames": F}
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    timed(HipEvents(d.hip_stream()), calls, d, out)
    print(json.dumps(out), flush=True)
    d.close()


def child_emit(config):
    import numpy as np
    import torch
    from bench import HipEvents, synth_device
    w, flavor, dev = sized(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    P, R = d.P, d.tile_streams()
    assert S % R == 0
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    pairs = torch.zeros(S * P * F * 2, dtype=torch.int32, device=dev)      # either layout: S is a whole number of tiles
    arena = torch.zeros(S * P * F * 8, dtype=torch.uint8, device=dev)
    ev = HipEvents(d.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    entries = S * P * n
    rng = np.random.default_rng(5)
    order = {"identity": np.arange(entries, dtype=np.uint64), "shuffled": rng.permutation(entries).astype(np.uint64)}
    tables = {(fmt, k): np.ascontiguousarray(v * np.uint64(B * fb)) for fmt, fb in ((32, 8), (24, 6)) for k, v in order.items()}
    formats = {fmt: np.full(S, fmt, dtype=np.uint8) for fmt in (32, 24)}
    for (fmt, k), t in tables.items(): assert d.packets_emit_check(formats[fmt], t, n, B, entries * B * (8 if fmt == 32 else 6), overlap=(k == "shuffled")) is None
    t_tables = {key: torch.from_numpy(t.view(np.int64)).to(dev) for key, t in tables.items()}
    t_formats = {fmt: torch.from_numpy(f).to(dev) for fmt, f in formats.items()}
    torch.cuda.synchronize()
    out = {"streams": S, "frames": F, "bytes_32": entries * B * 8, "bytes_24": entries * B * 6, "table_bytes": entries * 8 + S}
    ms = {}
    for tiled, name in ((False, "major"), (True, "tiled")):
        process = lambda tiled=tiled: d.process_device(pcm.data_ptr(), n, B, 16, pairs_ptr=pairs.data_ptr(), tiled=tiled)
        calls = {f"process_{name}": process}
        for (fmt, k), tt in t_tables.items():
            calls[f"kernel_{name}_{fmt}_{k}"] = lambda fmt=fmt, tt=tt, tiled=tiled: d.debug_packets_emit_launch(pairs.data_ptr(), n, B, t_formats[fmt].data_ptr(), tt.data_ptr(), arena.data_ptr(), tiled=tiled)
        calls[f"call_{name}_32_identity"] = lambda tiled=tiled: d.packets_emit_device(pairs.data_ptr(), n, B, formats[32], tables[(32, "identity")], arena.data_ptr(), arena.numel(), tiled=tiled)
        if not tiled:
            scratch = torch.empty(S * P * F * 8, dtype=torch.uint8, device=dev)
            for fmt in (32, 24): calls[f"copy_{fmt}"] = lambda fmt=fmt: hip.hipMemcpyDtoDAsync(scratch.data_ptr(), arena.data_ptr(), out[f"bytes_{fmt}"], ev.stream)
        o = {}
        timed(ev, calls, d, o)
        ms.update({k: v for k, v in o.items() if k not in ("power_w", "sclk_mhz")})
        out.setdefault("power_w", o["power_w"]); out.setdefault("sclk_mhz", o["sclk_mhz"])
        if not tiled: del scratch
    out.update(ms)
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
    line = {"config": config, "block_len": BLOCK_LEN, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["same", "emit"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    skip = ("streams", "frames", "bytes_32", "bytes_24", "table_bytes", "power_w", "sclk_mhz")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m, em = line["ms"], got["emit"][-1]
    rep = {"streams": em["streams"], "frames": em["frames"], "bytes_32": em["bytes_32"], "bytes_24": em["bytes_24"], "table_bytes_uploaded_per_call": em["table_bytes"]}
    for name in ("major", "tiled"):
        for fmt in (32, 24):
            for k in ("identity", "shuffled"):
                t = m[f"emit.kernel_{name}_{fmt}_{k}"]
                rep[f"kernel_{name}_{fmt}_{k}_over_copy"] = round(t / m[f"emit.copy_{fmt}"], 3)
                rep[f"kernel_{name}_{fmt}_{k}_written_tb_per_s"] = round(em[f"bytes_{fmt}"] / t / 1e9, 3)
    rep["tiled_plus_kernel_over_major"] = round((m["emit.process_tiled"] + m["emit.kernel_tiled_32_identity"]) / m["emit.process_major"], 3)
    rep["tiled_plus_call_over_major"] = round((m["emit.process_tiled"] + m["emit.call_tiled_32_identity"]) / m["emit.process_major"], 3)
    line["emit"] = rep
    if parent:
        gates = {f"gate_{c}_over_parent": round(m[f"same.{c}"] / m[f"parent.{c}"], 4) for c in ("p16", "ppackets")}
        line.update(gates)
        line["criterion_gate_within_1.02"] = all(g <= 1.02 for g in gates.values())
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        return child_gated(config, leg) if leg in ("parent", "same") else child_emit(config)
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
