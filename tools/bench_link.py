"""What chained devices (include/dspi.h: dspi_wire_decode, dspi_process_linked) cost, and that the calls they stand beside cost what they did
(profiles/link.md).  tools/bench_spdif_in.py's method: bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract) and config 5
(16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device buffers, per-call times by HIP events on the context's
stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so),
                one context, two calls interleaved: p24 = dspi_process at 24 bit, psources = dspi_process_sources, every source S/PDIF
    same        this build, the same two calls                       GATED: same / parent <= 1.02 for both calls
    decode      this build, the link receiver alone: dspi_wire_decode on device buffers, DECODE_FRAMES (4 800) frames, every line of a
                producer of DECODE_STREAMS (16 384) streams x 2 pairs linked once, identity order; six calls and a copy interleaved:
                  {tiled, sm} x {spdif, i2s, alt}   the view's layout x what the lines hold (alt: by producer stream, s % 2)
                  copy                              a hipMemcpyDtoDAsync of (bytes read + bytes written) / 2 of the all-S/PDIF case
                RECORDED: TB/s (read + written) and the ratio to the copy of the same bytes, per case
    chain<S>    this build, S streams (CHAIN_STREAMS, default 4096 and 65536), producer A and consumer B of the config's flavour, pair 0 of
                stream s linked to B's stream s, A's slots all S/PDIF:
                  a_tiled / a_sm      A's dspi_process_devices, tiled / stream-major wire words
                  linked              B's dspi_process_linked on A's TILED buffer
                  gather              S hipMemcpyDtoDAsync of one line each out of A's STREAM-MAJOR buffer into B's input buffer
                  sources             B's dspi_process_sources on the gathered buffer
                RECORDED: (a_tiled + linked) against today's only route (a_sm + gather + sources)

    python tools/bench_link.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=... DECODE_STREAMS=... DECODE_FRAMES=... CHAIN_STREAMS=4096,65536
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUNDS, LAUNCHES, WARMUP = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("LAUNCHES", 8)), int(os.environ.get("WARMUP", 2))
DECODE_STREAMS, DECODE_FRAMES = int(os.environ.get("DECODE_STREAMS", 16384)), int(os.environ.get("DECODE_FRAMES", 4800))
CHAIN_STREAMS = [int(x) for x in os.environ.get("CHAIN_STREAMS", "4096,65536").split(",") if x]
med = lambda v: round(statistics.median(v), 4)


def timed(ev, calls, d, out):
    """WARMUP + LAUNCHES rounds of the calls, interleaved; medians in ms, clock and power of the window into `out`"""
    import time
    from bench import PowerSampler
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
    out.update(power_w=pw and round(pw["power_w"], 1), sclk_mhz=pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]))
    d.sync()


def workload(config):
    import torch
    from bench import chain_workload
    from dspi_amd import wire as W
    w = chain_workload(config)
    return w, (W.F32_FMA if w["flavor"] else 0), torch.device("cuda", 0)


def make(flavor, S, w):
    from dspi_amd.host import Dspi
    d = Dspi(flavor, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    return d


def outputs(torch, dev, d, S, n, F):
    pairs = torch.empty((S, d.P, F, 2), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    return (pairs, sub, peaks), (pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())


def child_gated(config, leg):
    import numpy as np
    import torch
    from bench import HipEvents, synth_device
    from bench_mixed import widen_device
    from bench_spdif_in import spdif_lines
    from dspi_amd import host
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    if leg == "parent": assert not hasattr(d.L, "dspi_process_linked"), "PARENT_LIB has the feature: it is not the parent"
    wide = widen_device(torch, synth_device(torch, dev, S, F, w["fs"], 1234, True, 0))
    keep, outs = outputs(torch, dev, d, S, n, F)
    src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
    lines = spdif_lines(torch, flavor, wide, S, F, w["fs"])
    rx = torch.zeros(S * 40, dtype=torch.uint8, device=dev)
    calls = {"p24": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs),
             "psources": lambda: d.process_sources_device(lines.data_ptr(), src, n, B, rx.data_ptr(), *outs)}
    out = {"streams": S, "frames": F}
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    timed(HipEvents(d.hip_stream()), calls, d, out)
    out["plan"] = {k: v for k, v in d.launch_plan().items() if v}
    print(json.dumps(out), flush=True)
    d.close()


def child_decode(config):
    """the receiver alone; the lines are the library's own encoders' (dspi_wire_encode / dspi_wire_encode_tiled on random pair words)"""
    import numpy as np
    import torch
    from bench import HipEvents
    from dspi_amd import host, wire as W
    from dspi_amd.host import Dspi
    dev = torch.device("cuda", 0)
    S, F, P = DECODE_STREAMS, DECODE_FRAMES, 2
    p = Dspi(0, S, device=0)      # the producer: two pairs per stream, tile 64
    assert p.P == P
    R = p.tile_streams(); nt = (S + R - 1) // R
    n = S * P
    pairs_sm = torch.randint(-(1 << 23), 1 << 23, (S, P, F, 2), dtype=torch.int32, device=dev)
    pairs_t = pairs_sm.permute(0, 1, 3, 2).reshape(nt, R, 2 * P, F).permute(0, 2, 3, 1).contiguous()
    pos = torch.zeros(S, dtype=torch.int32, device=dev)
    wires = {}
    for kinds in ("spdif", "i2s", "alt"):
        # all streams at once, then the even streams back for `alt`
        for slot in range(P): p.vendor_get(W.REQ["SET_OUTPUT_TYPE"], slot | ((0 if kinds == "spdif" else 1) << 8), 1, -1)
        if kinds == "alt":
            for s in range(0, S, 2):
                for slot in range(P): p.vendor_get(W.REQ["SET_OUTPUT_TYPE"], slot | (0 << 8), 1, s)
        sm = torch.empty((S, P, F, 4), dtype=torch.int32, device=dev); tl = torch.empty((nt, P, F, 4, R), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p.wire_encode_device(pairs_sm.data_ptr(), F, pos.data_ptr(), sm.data_ptr())
        p.wire_encode_tiled_device(pairs_t.data_ptr(), F, pos.data_ptr(), tl.data_ptr())
        p.sync()
        wires[kinds] = (sm, tl, p.link_kinds(np.arange(n)))
    d = Dspi(0, 4, device=0)
    out_pairs = torch.empty((n, F, 2), dtype=torch.int32, device=dev)
    rx = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    ev = HipEvents(d.hip_stream())
    calls, nbytes = {}, {}
    for kinds, (sm, tl, links) in wires.items():
        n_sp = int((links["kind"] == host.LINK_SPDIF).sum())
        nbytes[kinds] = (n_sp * 16 + (n - n_sp) * 8) * F + n * F * 8
        for layout, buf in (("tiled", tl), ("sm", sm)):
            view = p.wire_view_of(buf.data_ptr(), F, tiled=layout == "tiled")
            calls[f"{layout}_{kinds}"] = lambda view=view, links=links: d.wire_decode_device(view, links, rx.data_ptr(), out_pairs.data_ptr())
    moved = nbytes["spdif"] // 2
    a, b = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    calls["copy"] = lambda: hip.hipMemcpyDtoDAsync(b.data_ptr(), a.data_ptr(), moved, ev.stream)
    torch.cuda.synchronize()
    calls["tiled_spdif"](); d.sync()
    assert torch.equal(out_pairs.reshape(S, P, F, 2), pairs_sm), "the bench's lines do not decode to the words that went in"
    r = rx.cpu().numpy().view(host.SPDIF_RX)
    assert (r["state"] == 2).all() and not r["held"].any() and not r["coding_errors"].any()
    out = {"links": n, "frames": F, "bytes": nbytes, "copy_bytes": moved}
    timed(ev, calls, d, out)
    print(json.dumps(out), flush=True)
    d.close(); p.close()


def child_chain(config, S):
    import numpy as np
    import torch
    from bench import HipEvents, synth_device
    from dspi_amd import host
    w, flavor, dev = workload(config)
    n, B = w["blocks"], w["B"]
    F = n * B
    A, Bc = make(flavor, S, w), make(flavor, S, w)
    P, R = A.P, A.tile_streams(); nt = (S + R - 1) // R
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    depths = np.full(S, 16, dtype=np.uint8)
    wire_t = torch.empty((nt, P, F, 4, R), dtype=torch.int32, device=dev)
    wire_sm = torch.empty((S, P, F, 4), dtype=torch.int32, device=dev)
    gathered = torch.empty((S, F, 4), dtype=torch.int32, device=dev)
    keep, outs = outputs(torch, dev, Bc, S, n, F)
    rx = [torch.zeros(S * 40, dtype=torch.uint8, device=dev) for _ in range(2)]
    links = A.link_kinds(np.arange(S) * P)
    assert (links["kind"] == host.LINK_SPDIF).all()
    view = A.wire_view_of(wire_t.data_ptr(), F, tiled=True)
    src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
    ev = HipEvents(Bc.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    line_b = F * 16
    g0, w0 = gathered.data_ptr(), wire_sm.data_ptr()

    def gather():
        for s in range(S): hip.hipMemcpyDtoDAsync(g0 + s * line_b, w0 + s * P * line_b, line_b, ev.stream)
    # (A's calls are timed on B's stream's clock by waiting for A first: the events bracket the launch on A only when A's stream is B's; so A
    #  is timed by its own events)
    ev_a = HipEvents(A.hip_stream())
    calls_a = {"a_tiled": lambda: A.process_devices_device(pcm.data_ptr(), depths, n, B, wire_t.data_ptr(), tiled=True),
               "a_sm": lambda: A.process_devices_device(pcm.data_ptr(), depths, n, B, wire_sm.data_ptr())}
    calls_b = {"linked": lambda: Bc.process_linked_device(view, links, n, B, rx[0].data_ptr(), *outs),
               "gather": gather,
               "sources": lambda: Bc.process_sources_device(gathered.data_ptr(), src, n, B, rx[1].data_ptr(), *outs)}
    torch.cuda.synchronize()
    for f in calls_a.values(): f()
    A.sync()
    for f in calls_b.values(): f()
    Bc.sync()
    out = {"streams": S, "frames": F}
    oa = {}
    timed(ev_a, calls_a, A, oa)
    timed(ev, calls_b, Bc, out)
    out.update({k: oa[k] for k in calls_a})
    out["power_w_a"], out["sclk_mhz_a"] = oa["power_w"], oa["sclk_mhz"]
    print(json.dumps(out), flush=True)
    A.close(); Bc.close()


def run_child(config, leg, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, leg], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {leg} ({lib or 'this build'}): {out.stderr[-800:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["same", "decode"] + [f"chain{S}" for S in CHAIN_STREAMS]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    skip = ("streams", "frames", "links", "bytes", "copy_bytes", "plan", "power_w", "sclk_mhz", "power_w_a", "sclk_mhz_a")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m = line["ms"]
    dec = got["decode"][-1]
    line["decode"] = {"links": dec["links"], "frames": dec["frames"], "bytes": dec["bytes"], "copy_bytes": dec["copy_bytes"]}
    copy_rate = dec["copy_bytes"] * 2 / m["decode.copy"]
    for layout in ("tiled", "sm"):
        for kinds in ("spdif", "i2s", "alt"):
            t = m[f"decode.{layout}_{kinds}"]
            line["decode"][f"{layout}_{kinds}"] = {"tb_per_s": round(dec["bytes"][kinds] / t / 1e9, 3), "over_copy_of_same_bytes": round(t / (dec["bytes"][kinds] / copy_rate), 3)}
    line["decode"]["copy_tb_per_s"] = round(copy_rate / 1e9, 3)
    for S in CHAIN_STREAMS:
        k = f"chain{S}"
        new, old = m[f"{k}.a_tiled"] + m[f"{k}.linked"], m[f"{k}.a_sm"] + m[f"{k}.gather"] + m[f"{k}.sources"]
        line[k] = {"linked_route_ms": round(new, 4), "gather_route_ms": round(old, 4), "gather_over_linked": round(old / new, 3), "linked_over_sources": round(m[f"{k}.linked"] / m[f"{k}.sources"], 4)}
    if parent:
        line["gate_p24_over_parent"] = round(m["same.p24"] / m["parent.p24"], 4)
        line["gate_psources_over_parent"] = round(m["same.psources"] / m["parent.psources"], 4)
        line["criterion_gate_within_1.02"] = max(line["gate_p24_over_parent"], line["gate_psources_over_parent"], 1 / line["gate_p24_over_parent"], 1 / line["gate_psources_over_parent"]) <= 1.02
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        if leg in ("parent", "same"): return child_gated(config, leg)
        if leg == "decode": return child_decode(config)
        return child_chain(config, int(leg[len("chain"):]))
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
