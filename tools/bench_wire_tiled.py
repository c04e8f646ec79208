"""What dspi_process_devices / dspi_wire_encode_tiled (include/dspi.h) cost, and that the existing calls cost what they did
(profiles/wire_tiled.md).  Method of tools/bench_wire.py, whose helpers this file uses: one MI355X, device buffers, per-call times by HIP
events on the context's own stream (dspi_hip_stream) after a warm-up, medians; every leg is a child process with one context, children
alternate ROUNDS times, a figure is the median over the children's medians; socket power and shader clock are sampled per child.
bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract) and config 5 (16 384 Q28 streams, 48-frame packets), PACKETS
packets per call.

    path      this build against the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it only this build is timed
              and the line says so), three existing calls: dspi_process with DSPI_OUT_SPDIF; dspi_process_wire with slots 0 and 2 of every
              stream I2S; dspi_process_mixed with depths 16 / 24 by s % 2.     criterion: this / parent <= 1.02 each
    encoder   dspi_wire_encode_tiled at the largest even frame count whose buffers fit beside the context (FRAMES overrides; at most 4 800),
              random words, against dspi_spdif_encode_v with DSPI_OUT_TILED of the same library on the same words, the stream-major
              dspi_wire_encode on as many words, and a device-to-device copy that moves the same bytes; type layouts and rates of
              tools/bench_wire.py (two_rates: the last stream at 44.1 kHz, so dspi_spdif_encode_v reads every stream's rate from its image
              as the wire encoders always read type and rate).     criterion: no I2S slot, two_rates: wire_tiled / spdif_v_tiled <= 1.02
    call      recorded: dspi_process_devices with DSPI_OUT_TILED, slots 0 and 2 of every stream I2S, against today's route for a tiled
              context — dspi_process(TILED), dspi_spdif_encode_v(TILED), dspi_i2s_encode(TILED) and the merge copy, all on the context's
              stream — and against the stream-major dspi_process_wire; and stream-major dspi_process_devices with depths 16 / 24 by s % 2
              against dspi_process_wire at 24 bit on input widened beforehand

    python tools/bench_wire_tiled.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=10 STREAMS=... FRAMES=... PARENT_LIB=... PARTS=path,encoder,call
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_wire import FRAMES, LAUNCHES, PACKETS, ROUNDS, TYPE_LAYOUTS, WARMUP, make_context, med, set_layout, timed      # noqa: E402


def report(d, S, F, legs, extra=None):
    """the legs of one child, A B C A B C: the later pass is kept; prints the child's JSON line"""
    from bench import HipEvents, PowerSampler
    for f in legs.values(): f()
    d.sync()
    smi = PowerSampler(0); smi.start()
    ev = HipEvents(d.hip_stream())
    res = dict(extra or {}, streams=S, frames=F, has_devices=hasattr(d.L, "dspi_process_devices"), plan={k: v for k, v in d.launch_plan().items() if v})
    for k in list(legs) * 2:
        ms, pw, ck = timed(ev, smi, legs[k], d.sync)
        res[k] = {"ms": ms, "power_w": pw, "sclk_mhz": ck}
    smi.stop()
    print(json.dumps(res), flush=True)
    d.close()


def mixed_input(torch, d, pcm, n, B):
    """depths 16 / 24 by s % 2: (depths, the call's buffer, the same input as packed 24-bit rows)"""
    import numpy as np
    from bench_mixed import widen_device
    S, F = d.n_streams, n * B
    depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
    wide = widen_device(torch, pcm)
    mixed = torch.cat([pcm[0::2].contiguous().view(torch.uint8).reshape(S // 2, -1), wide[1::2]], dim=1).contiguous()
    assert d.mixed_pcm_bytes(depths, n, B)[0] == mixed.numel() == S * F * 5
    return depths, mixed, wide


def child_path(config, leg):
    """one existing call, whichever library DSPI_LIB names"""
    import torch
    from bench import synth_device
    w, d = make_context(config)
    if leg == "wire_half": set_layout(d, w, "alternating_slots")
    S, n, B = d.n_streams, PACKETS, w["B"]
    F = n * B
    dev = torch.device("cuda", 0)
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    words = 2 if leg == "mixed_half" else 4
    pairs = torch.empty((S, d.P, F, words), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev); peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    outs = (pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    if leg == "spdif": call = lambda: d.process_device(pcm.data_ptr(), n, B, 16, *outs, spdif=True)
    elif leg == "wire_half": call = lambda: d.process_wire_device(pcm.data_ptr(), n, B, outs[0], 16, outs[1], outs[2])
    else:
        depths, mixed, _ = mixed_input(torch, d, pcm, n, B)
        call = lambda: d.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs)
    report(d, S, F, {"ms": call})


def child_encoder(config, layout, rates):
    """the tiled wire encoder, the tiled subframe encoder, the stream-major wire encoder and a copy of the same bytes, one type layout"""
    import torch
    w, d = make_context(config)
    types = set_layout(d, w, layout)
    if rates == "two_rates": assert d.set_rate(44100, stream=d.n_streams - 1) == 0
    S, P, R = d.n_streams, d.P, d.tile_streams()
    assert S % R == 0
    dev = torch.device("cuda", 0)
    free = torch.cuda.mem_get_info(0)[0]
    F = FRAMES or min(4800, int(free * 0.5 / (S * P * 24)) // 2 * 2)      # 8 bytes in and 16 out per frame and pair
    assert F >= 2 and F % 2 == 0
    g = torch.Generator(device=dev); g.manual_seed(77)
    words = torch.randint(-(1 << 23), 1 << 23, (S * P * F * 2,), dtype=torch.int32, device=dev, generator=g)      # either layout: random words
    out = torch.empty((S * P * F * 4,), dtype=torch.int32, device=dev)
    pos = torch.randint(0, 192, (S,), dtype=torch.int32, device=dev, generator=g)
    n_i2s = int(types.sum())
    moved = (S * P * 24 - n_i2s * 8) * F
    half = moved // 2 // 16 * 16
    flat_out = out.view(torch.uint8)
    scratch = torch.empty((half,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.ExternalStream(d.hip_stream())
    def copy():
        with torch.cuda.stream(stream): scratch.copy_(flat_out[:half])
    legs = {"wire_tiled": lambda: d.wire_encode_tiled_device(words.data_ptr(), F, pos.data_ptr(), out.data_ptr()),
            "spdif_v_tiled": lambda: d.spdif_encode_v_device(words.data_ptr(), F, pos.data_ptr(), out.data_ptr(), tiled=True),
            "wire": lambda: d.wire_encode_device(words.data_ptr(), F, pos.data_ptr(), out.data_ptr()), "copy": copy}
    torch.cuda.synchronize()
    report(d, S, F, legs, {"layout": layout, "rates": rates, "i2s_regions": n_i2s, "regions": S * P, "moved_bytes": moved, "spdif_v_bytes": S * P * 24 * F,
                           "copy_bytes_moved": 2 * half, "images": d.image_count()})


def child_call(config, leg):
    import torch
    from bench import synth_device
    w, d = make_context(config)
    types = set_layout(d, w, "alternating_slots")
    S, n, B, P, R = d.n_streams, PACKETS, w["B"], d.P, d.tile_streams()
    F, nt = n * B, d.n_streams // d.tile_streams()
    assert S % R == 0
    dev = torch.device("cuda", 0)
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    wire = torch.empty((S * P * F * 4,), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev); peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    import numpy as np
    u16 = np.full(S, 16, dtype=np.uint8)
    if leg == "devices_tiled": call = lambda: d.process_devices_device(pcm.data_ptr(), u16, n, B, wire.data_ptr(), sub.data_ptr(), peaks.data_ptr(), tiled=True)
    elif leg == "wire": call = lambda: d.process_wire_device(pcm.data_ptr(), n, B, wire.data_ptr(), 16, sub.data_ptr(), peaks.data_ptr())
    elif leg == "today_tiled":
        pairs = torch.empty((nt, 2 * P, F, R), dtype=torch.int32, device=dev); slots = torch.empty((nt, 2 * P, F, R), dtype=torch.int32, device=dev)
        pos = torch.zeros((S,), dtype=torch.int32, device=dev)
        stream = torch.cuda.ExternalStream(d.hip_stream())
        i2s = [p for p in range(P) if types[0, p]]
        wire_v, slots_v = wire.view(nt, P, 4 * F, R), slots.view(nt, P, 2 * F, R)
        def call():
            d.process_device(pcm.data_ptr(), n, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr(), tiled=True)
            d.spdif_encode_v_device(pairs.data_ptr(), F, pos.data_ptr(), wire.data_ptr(), tiled=True)
            d.i2s_device(pairs.data_ptr(), F, 0, slots.data_ptr(), tiled=True)
            with torch.cuda.stream(stream):
                for p in i2s: wire_v[:, p, :2 * F].copy_(slots_v[:, p])
    else:
        depths, mixed, wide = mixed_input(torch, d, pcm, n, B)
        if leg == "devices_mixed": call = lambda: d.process_devices_device(mixed.data_ptr(), depths, n, B, wire.data_ptr(), sub.data_ptr(), peaks.data_ptr())
        else: call = lambda: d.process_wire_device(wide.data_ptr(), n, B, wire.data_ptr(), 24, sub.data_ptr(), peaks.data_ptr())      # wire_widened
    report(d, S, F, {"ms": call})


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
        line["path"] = {}
        for leg in ("spdif", "wire_half", "mixed_half"):
            who = (["parent"] if parent else []) + ["this"]
            got = {k: [] for k in who}
            for _ in range(ROUNDS):
                for k in who: got[k].append(run_child(["path", config, leg], parent if k == "parent" else None))
            if parent: assert not got["parent"][0]["has_devices"], "PARENT_LIB has the feature: it is not the parent"
            p = {"ms": {k: med([x["ms"]["ms"] for x in v]) for k, v in got.items()}, "children": got}
            if parent:
                p["this_over_parent"] = round(p["ms"]["this"] / p["ms"]["parent"], 4)
                p["criterion_le_1.02"] = p["this_over_parent"] <= 1.02
            else: p["parent"] = "skipped: PARENT_LIB not set"
            line["path"][leg] = p
    if "encoder" in parts:
        enc = {}
        names = ("wire_tiled", "spdif_v_tiled", "wire", "copy")
        for layout in TYPE_LAYOUTS:
            for rates in ("one_rate", "two_rates"):
                runs = [run_child(["encoder", config, layout, rates]) for _ in range(ROUNDS)]
                e = {"children": runs, "ms": {k: med([r[k]["ms"] for r in runs]) for k in names}}
                e["gb_per_s"] = {"wire_tiled": round(runs[0]["moved_bytes"] / e["ms"]["wire_tiled"] / 1e6, 1), "wire": round(runs[0]["moved_bytes"] / e["ms"]["wire"] / 1e6, 1),
                                 "spdif_v_tiled": round(runs[0]["spdif_v_bytes"] / e["ms"]["spdif_v_tiled"] / 1e6, 1), "copy": round(runs[0]["copy_bytes_moved"] / e["ms"]["copy"] / 1e6, 1)}
                for k in ("spdif_v_tiled", "wire", "copy"): e[f"wire_tiled_over_{k}"] = round(e["ms"]["wire_tiled"] / e["ms"][k], 4)
                if layout == "none" and rates == "two_rates": e["criterion_le_1.02"] = e["wire_tiled_over_spdif_v_tiled"] <= 1.02
                enc[f"{layout}/{rates}"] = e
        line["encoder"] = enc
    if "call" in parts:
        legs = ("devices_tiled", "today_tiled", "wire", "devices_mixed", "wire_widened")
        got = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k in legs: got[k].append(run_child(["call", config, k]))
        c = {"ms": {k: med([x["ms"]["ms"] for x in v]) for k, v in got.items()}, "children": got}
        c["devices_tiled_over_today_tiled"] = round(c["ms"]["devices_tiled"] / c["ms"]["today_tiled"], 4)
        c["devices_tiled_over_wire"] = round(c["ms"]["devices_tiled"] / c["ms"]["wire"], 4)
        c["devices_mixed_over_wire_widened"] = round(c["ms"]["devices_mixed"] / c["ms"]["wire_widened"], 4)
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
