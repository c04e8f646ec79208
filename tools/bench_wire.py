"""What dspi_process_wire / dspi_wire_encode (include/dspi.h) cost, and that the existing DSPI_OUT_SPDIF path costs what it did
(profiles/wire.md).  One MI355X, device buffers, per-call times by HIP events on the context's own stream (dspi_hip_stream) after a warm-up,
medians; every leg is a child process with one context, children alternate ROUNDS times, a figure is the median over the children's
medians; socket power and shader clock are sampled per child as bench.py samples them.

    path      bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract) and config 5 (16 384 Q28 streams, 48-frame packets),
              PACKETS packets per call: dspi_process with DSPI_OUT_SPDIF on this build against the PARENT commit's library
              (PARENT_LIB=<path of its libdspi_mi355x.so>; without it only this build is timed and the line says so).
              criterion: this / parent <= 1.02 (nothing on that path changes)
    encoder   dspi_wire_encode at the largest even frame count whose buffers fit beside the context (FRAMES overrides; at most 4 800), random
              words, against dspi_spdif_encode_v of the same library on the same words and a device-to-device copy that moves the same bytes
              (read + written), for three type layouts: no I2S slot; every other stream all I2S; alternating slots in every stream.
              Each with every stream at one rate (dspi_spdif_encode_v then reads no image at all: one status word for everybody) and with the
              last stream at 44.1 kHz (it reads each stream's rate from its image, as the wire encoder always reads type and rate).
              criterion: with no I2S slot, wire / spdif_encode_v <= 1.02 (one more word from a cache line the lane already touches)
    call      dspi_process_wire with slots 0 and 2 of every stream I2S against what gives those words without it: dspi_process into pair
              words, dspi_spdif_encode and dspi_i2s_encode (types of stream 0: every stream has them here) from there, and a masked copy of
              the slot words into the subframe buffer, all on the context's stream.  Recorded, not gated.

    python tools/bench_wire.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=10 STREAMS=... FRAMES=... PARENT_LIB=...
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("LAUNCHES", 8)), int(os.environ.get("WARMUP", 2))
PACKETS, STREAMS, FRAMES = int(os.environ.get("PACKETS", 10)), int(os.environ.get("STREAMS", 0)), int(os.environ.get("FRAMES", 0))
med = lambda v: round(statistics.median(v), 4)
TYPE_LAYOUTS = ("none", "half_streams", "alternating_slots")


def make_context(config):
    from bench import chain_workload
    from dspi_amd import wire as W
    from dspi_amd.host import Dspi
    w = chain_workload(config)
    d = Dspi(W.F32_FMA if w["flavor"] else 0, STREAMS or w["streams"], device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    return w, d


def set_layout(d, w, layout):
    """the output types of a type layout, with broadcast requests wherever that gives it; returns bool [S][P]"""
    import numpy as np
    from dspi_amd import wire as W
    req = W.REQ["SET_OUTPUT_TYPE"]
    types = np.zeros((d.n_streams, d.P), dtype=bool)
    if layout == "alternating_slots":
        for p in range(0, d.P, 2): assert d.vendor_get(req, p | (1 << 8), 1, -1) == b"\x00"
        types[:, 0::2] = True
    elif layout == "half_streams":      # every stream all I2S, then the even streams back: two parameter objects after the fold-back pass
        for p in range(d.P): assert d.vendor_get(req, p | (1 << 8), 1, -1) == b"\x00"
        for s in range(0, d.n_streams, 2):
            for p in range(d.P): assert d.vendor_get(req, p, 1, s) == b"\x00"
        d.set_volume(w["vol"])          # (a broadcast call asks for the fold-back pass)
        types[1::2] = True
    return types


def timed(ev, smi, fn, sync):
    """LAUNCHES timed calls of fn after WARMUP: (median ms, power and clock of the window)"""
    import time
    ms = []
    t0 = time.perf_counter()
    for i in range(WARMUP + LAUNCHES):
        e0, e1 = ev.new(), ev.new()
        ev.record(e0); fn(); ev.record(e1)
        t = ev.elapsed_ms(e0, e1)
        if i >= WARMUP: ms.append(t)
    sync()
    pw = smi.window(t0, time.perf_counter()) if smi.ok else None
    return med(ms), (pw and round(pw["power_w"], 1)), (pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]))


def child_path(config):
    """dspi_process with DSPI_OUT_SPDIF, whichever library DSPI_LIB names"""
    import torch
    from bench import HipEvents, PowerSampler, synth_device
    w, d = make_context(config)
    S, n, B = d.n_streams, PACKETS, w["B"]
    F = n * B
    dev = torch.device("cuda", 0)
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    pairs = torch.empty((S, d.P, F, 4), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev); peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    call = lambda: d.process_device(pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr(), spdif=True)
    call(); d.sync()
    smi = PowerSampler(0); smi.start()
    ms, pw, ck = timed(HipEvents(d.hip_stream()), smi, call, d.sync)
    smi.stop()
    print(json.dumps({"ms": ms, "power_w": pw, "sclk_mhz": ck, "streams": S, "frames": F, "has_wire": hasattr(d.L, "dspi_process_wire"), "plan": d.launch_plan()}), flush=True)
    d.close()


def child_encoder(config, layout, rates):
    """dspi_wire_encode, dspi_spdif_encode_v and a copy of the same bytes, one type layout; rates: one_rate / two_rates"""
    import torch
    from bench import HipEvents, PowerSampler
    w, d = make_context(config)
    types = set_layout(d, w, layout)
    if rates == "two_rates": assert d.set_rate(44100, stream=d.n_streams - 1) == 0
    S, P = d.n_streams, d.P
    dev = torch.device("cuda", 0)
    free = torch.cuda.mem_get_info(0)[0]
    F = FRAMES or min(4800, int(free * 0.5 / (S * P * 24)) // 2 * 2)      # 8 bytes in and 16 out per frame and pair
    assert F >= 2 and F % 2 == 0
    g = torch.Generator(device=dev); g.manual_seed(77)
    words = torch.randint(-(1 << 23), 1 << 23, (S, P, F, 2), dtype=torch.int32, device=dev, generator=g)
    out = torch.empty((S, P, F, 4), dtype=torch.int32, device=dev)
    pos = torch.randint(0, 192, (S,), dtype=torch.int32, device=dev, generator=g)
    n_i2s = int(types.sum())
    moved = (S * P * 24 - n_i2s * 8) * F                                   # an I2S region takes 8 F bytes in and 8 F bytes out
    half = moved // 2 // 16 * 16                                          # a copy reads and writes each byte it moves
    flat_out = out.view(-1).view(torch.uint8)
    assert half <= flat_out.numel()
    scratch = torch.empty((half,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.ExternalStream(d.hip_stream())
    def copy():
        with torch.cuda.stream(stream): scratch.copy_(flat_out[:half])
    legs = {"wire": lambda: d.wire_encode_device(words.data_ptr(), F, pos.data_ptr(), out.data_ptr()),
            "spdif_v": lambda: d.spdif_encode_v_device(words.data_ptr(), F, pos.data_ptr(), out.data_ptr()), "copy": copy}
    torch.cuda.synchronize()
    for f in legs.values(): f()
    d.sync()
    smi = PowerSampler(0); smi.start()
    ev = HipEvents(d.hip_stream())
    res = {"layout": layout, "rates": rates, "streams": S, "frames": F, "i2s_regions": n_i2s, "regions": S * P, "moved_bytes": moved, "copy_bytes_moved": 2 * half, "images": d.image_count()}
    for k in ("wire", "spdif_v", "copy", "wire", "spdif_v", "copy"):      # A B C A B C in one process: the later pass is kept
        ms, pw, ck = timed(ev, smi, legs[k], d.sync)
        res[k] = {"ms": ms, "power_w": pw, "sclk_mhz": ck}
    smi.stop()
    res["wire"]["gb_per_s"] = round(moved / res["wire"]["ms"] / 1e6, 1)
    res["spdif_v"]["gb_per_s"] = round(S * P * 24 * F / res["spdif_v"]["ms"] / 1e6, 1)
    res["copy"]["gb_per_s"] = round(2 * half / res["copy"]["ms"] / 1e6, 1)
    print(json.dumps(res), flush=True)
    d.close()


def child_call(config, leg):
    """leg wire: dspi_process_wire; leg today: dspi_process + dspi_spdif_encode + dspi_i2s_encode + the masked copy"""
    import torch
    from bench import HipEvents, PowerSampler, synth_device
    w, d = make_context(config)
    types = set_layout(d, w, "alternating_slots")
    S, n, B, P = d.n_streams, PACKETS, w["B"], d.P
    F = n * B
    dev = torch.device("cuda", 0)
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    wire = torch.empty((S, P, F, 4), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev); peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    if leg == "wire":
        call = lambda: d.process_wire_device(pcm.data_ptr(), n, B, wire.data_ptr(), 16, sub.data_ptr(), peaks.data_ptr())
    else:
        pairs = torch.empty((S, P, F, 2), dtype=torch.int32, device=dev); slots = torch.empty((S, P, F, 2), dtype=torch.int32, device=dev)
        stream = torch.cuda.ExternalStream(d.hip_stream())
        i2s = [p for p in range(P) if types[0, p]]
        state = {"pos": 0}
        def call():
            d.process_device(pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
            state["pos"] = d.spdif_device(pairs.data_ptr(), F, state["pos"], wire.data_ptr())
            d.i2s_device(pairs.data_ptr(), F, 0, slots.data_ptr())
            with torch.cuda.stream(stream):
                for p in i2s: wire.view(S, P, F * 4)[:, p, :2 * F].copy_(slots.view(S, P, F * 2)[:, p])
    call(); d.sync()
    smi = PowerSampler(0); smi.start()
    ms, pw, ck = timed(HipEvents(d.hip_stream()), smi, call, d.sync)
    smi.stop()
    print(json.dumps({"ms": ms, "power_w": pw, "sclk_mhz": ck, "streams": S, "frames": F, "plan": d.launch_plan()}), flush=True)
    d.close()


def run_child(args, lib=None):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + list(args), env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {args} ({lib or 'this build'}): {out.stderr[-800:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent, parts):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP, "packets": PACKETS}
    if "path" in parts:
        legs = (["parent"] if parent else []) + ["this"]
        got = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k in legs: got[k].append(run_child(["path", config], parent if k == "parent" else None))
        if parent: assert not got["parent"][0]["has_wire"], "PARENT_LIB has the feature: it is not the parent"
        p = {"ms": {k: med([x["ms"] for x in v]) for k, v in got.items()}, "children": got}
        if parent:
            p["this_over_parent"] = round(p["ms"]["this"] / p["ms"]["parent"], 4)
            p["criterion_le_1.02"] = p["this_over_parent"] <= 1.02
        else: p["parent"] = "skipped: PARENT_LIB not set"
        line["path"] = p
    if "encoder" in parts:
        enc = {}
        for layout in TYPE_LAYOUTS:
            for rates in ("one_rate", "two_rates"):
                runs = [run_child(["encoder", config, layout, rates]) for _ in range(ROUNDS)]
                e = {"children": runs, "ms": {k: med([r[k]["ms"] for r in runs]) for k in ("wire", "spdif_v", "copy")},
                     "gb_per_s": {k: med([r[k]["gb_per_s"] for r in runs]) for k in ("wire", "spdif_v", "copy")}}
                e["wire_over_spdif_v"] = round(e["ms"]["wire"] / e["ms"]["spdif_v"], 4)
                e["wire_over_copy"] = round(e["ms"]["wire"] / e["ms"]["copy"], 4)
                if layout == "none": e["criterion_le_1.02"] = e["wire_over_spdif_v"] <= 1.02
                enc[f"{layout}/{rates}"] = e
        line["encoder"] = enc
    if "call" in parts:
        got = {"wire": [], "today": []}
        for _ in range(ROUNDS):
            for k in got: got[k].append(run_child(["call", config, k]))
        c = {"ms": {k: med([x["ms"] for x in v]) for k, v in got.items()}, "children": got}
        c["wire_over_today"] = round(c["ms"]["wire"] / c["ms"]["today"], 4)
        line["call"] = c
    return line


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child":
        return {"path": child_path, "encoder": child_encoder, "call": child_call}[a[1]](*a[2:])
    parent = os.environ.get("PARENT_LIB")
    parts = [p for p in os.environ.get("PARTS", "path,encoder,call").split(",") if p]
    for config in [x for x in a if not x.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None, parts)), flush=True)


if __name__ == "__main__":
    main()
