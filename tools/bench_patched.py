"""What the patch bay (include/dspi.h: dspi_process_patched) costs, and that the calls it stands beside cost what they did
(profiles/patched.md).  tools/bench_link.py's method and helpers: bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract)
and config 5 (16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device buffers, per-call times by HIP events on
the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so),
                one context, three calls interleaved: p24 = dspi_process at 24 bit, psources = dspi_process_sources, every source S/PDIF,
                plinked = dspi_process_linked on a TILED view whose neighbouring columns go to neighbouring streams
    same        this build, the same three calls                        GATED: same / parent within 1.02 for each
    pdecode     the parent's library, tools/bench_link.py's decode leg (dspi_wire_decode, 4 800 frames x 32 768 links)
    decode      this build, the same                                     GATED: the three tiled cases, same / parent within 1.02
    patched     this build: a consumer whose streams are, a contiguous fifth each, PCM16, PCM24, S/PDIF runs, links into A's TILED wire
                buffer and links into B's STREAM-MAJOR wire buffer (A, B: a fifth of the consumer's streams each, the config's flavour,
                pair 0 of producer stream i to the i-th stream of the fifth):
                  patched    ONE dspi_process_patched
                  route      what is available without it, on a twin: pause the two LINK fifths, dspi_process_sources, resume; pause all but
                             A's fifth, dspi_process_linked, resume; the same for B's fifth — nine calls
                  front      dspi_debug_patched_intake: everything in front of the chain
                  copy       a hipMemcpyDtoDAsync of (bytes the front end reads + writes) / 2
                RECORDED: route / patched by HIP events and by the wall clock (the toggles have host work), front / copy, and whether the
                first patched call and the first route left the same pair words, sub words and records

    python tools/bench_patched.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=...
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

from bench_link import LAUNCHES, ROUNDS, WARMUP, child_decode, make, med, outputs, timed, workload      # noqa: E402


def producer_wire(torch, dev, flavor, S, w, tiled):
    """a producer of S streams, its wire buffer written once by dspi_process_devices -> (context, buffer, view)"""
    import numpy as np
    from bench import synth_device
    n, B = w["blocks"], w["B"]
    F = n * B
    A = make(flavor, S, w)
    R = A.tile_streams(); nt = (S + R - 1) // R
    wire = torch.zeros((nt, A.P, F, 4, R) if tiled else (S, A.P, F, 4), dtype=torch.int32, device=dev)
    pcm = synth_device(torch, dev, S, F, w["fs"], 99, True, 0)
    torch.cuda.synchronize()
    A.process_devices_device(pcm.data_ptr(), np.full(S, 16, dtype=np.uint8), n, B, wire.data_ptr(), tiled=tiled)
    A.sync()
    view = A.wire_view_of(wire.data_ptr(), F, tiled=tiled)
    view["producer"] = 0      # (written once, long ago: nothing to wait for)
    return A, wire, view


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
    if leg == "parent": assert not hasattr(d.L, "dspi_process_patched"), "PARENT_LIB has the feature: it is not the parent"
    wide = widen_device(torch, synth_device(torch, dev, S, F, w["fs"], 1234, True, 0))
    keep, outs = outputs(torch, dev, d, S, n, F)
    src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
    lines = spdif_lines(torch, flavor, wide, S, F, w["fs"])
    rx = [torch.zeros(S * 40, dtype=torch.uint8, device=dev) for _ in range(2)]
    SA = S // d.P      # S lines: every consumer stream its own, stream s column s % SA of pair s // SA
    A, wire, view = producer_wire(torch, dev, flavor, SA, w, True)
    links = A.link_kinds((np.arange(S) % SA) * A.P + np.arange(S) // SA)
    calls = {"p24": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs),
             "psources": lambda: d.process_sources_device(lines.data_ptr(), src, n, B, rx[0].data_ptr(), *outs),
             "plinked": lambda: d.process_linked_device(view, links, n, B, rx[1].data_ptr(), *outs)}
    out = {"streams": S, "frames": F}
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    timed(HipEvents(d.hip_stream()), calls, d, out)
    print(json.dumps(out), flush=True)
    d.close(); A.close()


def child_patched(config):
    import numpy as np
    import torch
    from bench import HipEvents, PowerSampler, synth_device
    from bench_mixed import widen_device
    from bench_spdif_in import spdif_lines
    from dspi_amd import host
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    q = S // 5
    lo = [0, q, 2 * q, 3 * q, 4 * q, S]      # the five runs of streams
    c, twin = make(flavor, S, w), make(flavor, S, w)
    P = c.P
    A, wire_a, view_a = producer_wire(torch, dev, flavor, lo[4] - lo[3], w, True)
    Bp, wire_b, view_b = producer_wire(torch, dev, flavor, lo[5] - lo[4], w, False)
    src = np.zeros(S, dtype=np.uint8)
    for k, x in enumerate((16, 24, host.SRC_SPDIF, host.SRC_LINK, host.SRC_LINK)): src[lo[k]:lo[k + 1]] = x
    patches = np.zeros(S, dtype=host.PATCH)
    patches["view"][lo[4]:] = 1
    patches["line"][lo[3]:lo[4]] = np.arange(lo[4] - lo[3]) * P; patches["line"][lo[4]:] = np.arange(lo[5] - lo[4]) * P
    patches["kind"] = host.LINK_SPDIF
    views = np.stack([view_a, view_b])
    # `in`: the three runs where dspi_patched_bytes puts them; the twin's buffer is dspi_sources_bytes' with the LINK streams as PCM16 slots
    pcm16 = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    wide = widen_device(torch, pcm16)
    lines = spdif_lines(torch, flavor, wide, S, F, w["fs"])
    b16, b24, bsp = pcm16.view(torch.uint8).reshape(S, -1), wide.view(torch.uint8).reshape(S, -1), lines.view(torch.uint8).reshape(S, -1)

    def laid(total, off, sources):
        buf = torch.zeros(int(total) + 16, dtype=torch.uint8, device=dev)
        for k, rows in ((0, b16), (1, b24), (2, bsp)):
            a, b = int(off[lo[k]]), int(off[lo[k + 1] - 1]) + rows.shape[1]
            assert b - a == (lo[k + 1] - lo[k]) * rows.shape[1], "the runs of one kind lie back to back"
            buf[a:b] = rows[lo[k]:lo[k + 1]].reshape(-1)
        return buf
    total, off = c.patched_bytes(src, n, B)
    t_in = laid(total, off, src)
    src2 = np.where(src == host.SRC_LINK, 16, src).astype(np.uint8)
    total2, off2 = twin.sources_bytes(src2, n, B)
    t_in2 = laid(total2, off2, src2)
    links_a = np.zeros(S, dtype=host.LINK); links_a["line"] = patches["line"]; links_a["kind"] = host.LINK_SPDIF
    keep, outs = outputs(torch, dev, c, S, n, F)
    keep2, outs2 = outputs(torch, dev, twin, S, n, F)
    rx, rx2 = torch.zeros(S * 40, dtype=torch.uint8, device=dev), torch.zeros(S * 40, dtype=torch.uint8, device=dev)

    def route():
        twin.pause_streams(lo[3], S - lo[3]); twin.process_sources_device(t_in2.data_ptr(), src2, n, B, rx2.data_ptr(), *outs2); twin.resume_streams(lo[3], S - lo[3])
        twin.pause_streams(0, lo[3]); twin.pause_streams(lo[4], S - lo[4]); twin.process_linked_device(view_a, links_a, n, B, rx2.data_ptr(), *outs2)
        twin.resume_streams(0, lo[3]); twin.resume_streams(lo[4], S - lo[4])
        twin.pause_streams(0, lo[4]); twin.process_linked_device(view_b, links_a, n, B, rx2.data_ptr(), *outs2); twin.resume_streams(0, lo[4])
    moved = (int(total) + (S - lo[3]) * F * 16 + S * F * 6) // 2      # `in`, a 16-byte frame per LINK stream, 6 bytes written per stream
    ca, cb = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    ev, ev2 = HipEvents(c.hip_stream()), HipEvents(twin.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    calls = {"patched": lambda: c.process_patched_device(t_in.data_ptr(), src, views, patches, n, B, rx.data_ptr(), *outs),
             "front": lambda: c.debug_patched_intake(t_in.data_ptr(), src, views, patches, n, B, rx.data_ptr()),
             "copy": lambda: hip.hipMemcpyDtoDAsync(cb.data_ptr(), ca.data_ptr(), moved, ev.stream)}
    torch.cuda.synchronize()
    calls["patched"](); route()
    c.sync(); twin.sync()
    # the two routes compute the same words (the S/PDIF and LINK streams' records differ in nothing either)
    agree = bool(torch.equal(keep[0], keep2[0]) and torch.equal(keep[1], keep2[1]) and torch.equal(rx, rx2))
    out = {"streams": S, "frames": F, "front_bytes": moved * 2, "agree": agree}
    timed(ev, calls, c, out)
    o2 = {}
    timed(ev2, {"route": route}, twin, o2)
    out["route"] = o2["route"]
    # the wall clock of one call and the wait for it: the toggles have host work that events on the stream do not see
    wall = {"patched_wall": [], "route_wall": []}
    smi = PowerSampler(0); smi.start()
    for i in range(WARMUP + LAUNCHES):
        for name, f, d in (("patched_wall", calls["patched"], c), ("route_wall", route, twin)):
            t0 = time.perf_counter(); f(); d.sync()
            if i >= WARMUP: wall[name].append((time.perf_counter() - t0) * 1e3)
    smi.stop()
    out.update({k: med(v) for k, v in wall.items()})
    print(json.dumps(out), flush=True)
    for x in (c, twin, A, Bp): x.close()


def run_child(config, leg, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, leg], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {leg} ({lib or 'this build'}): {out.stderr[-800:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["same"] + (["pdecode"] if parent else []) + ["decode", "patched"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k in ("parent", "pdecode") else None))
    skip = ("streams", "frames", "links", "bytes", "copy_bytes", "front_bytes", "agree", "plan", "power_w", "sclk_mhz")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m = line["ms"]
    pt = got["patched"][-1]
    line["patched"] = {"streams": pt["streams"], "frames": pt["frames"], "outputs_and_records_agree_with_route": all(x["agree"] for x in got["patched"]), "route_over_patched_events": round(m["patched.route"] / m["patched.patched"], 3),
                       "route_over_patched_wall": round(m["patched.route_wall"] / m["patched.patched_wall"], 3),
                       "front_tb_per_s": round(pt["front_bytes"] / m["patched.front"] / 1e9, 3), "front_over_copy_of_same_bytes": round(m["patched.front"] / m["patched.copy"], 3)}
    if parent:
        gates = {f"gate_{c}_over_parent": round(m[f"same.{c}"] / m[f"parent.{c}"], 4) for c in ("p24", "psources", "plinked")}
        gates.update({f"gate_decode_{c}_over_parent": round(m[f"decode.{c}"] / m[f"pdecode.{c}"], 4) for c in ("tiled_spdif", "tiled_i2s", "tiled_alt")})
        line.update(gates)
        line["criterion_gate_within_1.02"] = all(1 / 1.02 <= g <= 1.02 for g in gates.values())
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        if leg in ("parent", "same"): return child_gated(config, leg)
        if leg in ("pdecode", "decode"): return child_decode(config)
        return child_patched(config)
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
