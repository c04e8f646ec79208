"""What resident packet tables (include/dspi.h: dspi_process_packets_resident, dspi_packets_emit_resident) save, and that the calls they stand
beside cost what they did (profiles/packets_resident.md).  tools/bench_packets.py's method and helpers: bench.py's config 3 (65 536 float
streams, FMA contract) and config 5 (16 384 Q28 streams), both at 50 packets of 96 frames per call, device buffers, per-call times by HIP events
on the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so),
                one context, three calls interleaved: p24 = dspi_process at 24 bit; ppackets = dspi_process_packets, 24 bit, by the HOST table of
                its own contiguous layout; pemit = dspi_packets_emit of the pair words, format 32, by the HOST identity table
    same        this build, the same three calls                        GATED: same / parent within 1.02 for each
    resident    this build, RECORDED.  Each call is waited for (the events around ONE call), and queued: LAUNCHES calls between two events with
                nothing waiting in between, per call (q_*):
                  check_input, check_emit       dspi_debug_table_check_launch: the checker's ONE launch, depths / formats and table on the device
                  copy_input, copy_emit         a hipMemcpyDtoDAsync of the table's bytes: the yardstick.  The checker only READS those bytes, the
                                                copy reads and writes them: "/ copy" flatters the checker by up to a factor of two
                  packets_host / _default / _checked      dspi_process_packets; dspi_process_packets_resident by the default route (check, wait,
                                                launches) and with DSPI_TABLE_CHECKED; mixed24 = dspi_process_mixed on the same bytes: the launch
                                                alone that a packets call is measured against (profiles/packets.md)
                  emit_host / _default / _checked / _launch   dspi_packets_emit; dspi_packets_emit_resident either route;
                                                dspi_debug_packets_emit_launch: the launch alone

    python tools/bench_packets_resident.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=...
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
GATED = ("p24", "ppackets", "pemit")


def setup(config):
    """the context, the 24-bit input in dspi_process_mixed's own layout, its table, the outputs, the identity emit table at format 32"""
    import numpy as np
    import torch
    from bench import synth_device
    from bench_mixed import widen_device
    w, flavor, dev = workload(config)
    w = dict(w, B=BLOCK_LEN)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d = make(flavor, S, w)
    wide = widen_device(torch, synth_device(torch, dev, S, F, w["fs"], 1234, True, 0))
    keep, outs = outputs(torch, dev, d, S, n, F)
    x = dict(d=d, dev=dev, S=S, n=n, B=B, F=F, wide=wide, keep=keep, outs=outs, pairs=keep[0])
    x["depths"] = np.full(S, 24, dtype=np.uint8)
    x["table"] = (np.arange(S * n, dtype=np.uint64) * np.uint64(6 * B)).reshape(S, n)
    x["formats"] = np.full(S, 32, dtype=np.uint8)
    x["etable"] = np.arange(S * d.P * n, dtype=np.uint64) * np.uint64(8 * B)
    x["arena"] = torch.zeros(S * d.P * F * 8, dtype=torch.uint8, device=dev)
    return x


def child_gated(config, leg):
    import torch
    from bench import HipEvents
    x = setup(config)
    d, S, n, B, F = x["d"], x["S"], x["n"], x["B"], x["F"]
    if leg == "parent": assert not hasattr(d.L, "dspi_process_packets_resident"), "PARENT_LIB has the feature: it is not the parent"
    calls = {"p24": lambda: d.process_device(x["wide"].data_ptr(), n, B, 24, *x["outs"]),
             "ppackets": lambda: d.process_packets_device(x["wide"].data_ptr(), S * F * 6, x["depths"], x["table"], n, B, *x["outs"]),
             "pemit": lambda: d.packets_emit_device(x["pairs"].data_ptr(), n, B, x["formats"], x["etable"], x["arena"].data_ptr(), x["arena"].numel())}
    out = {"streams": S, "frames": F}
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    timed(HipEvents(d.hip_stream()), calls, d, out)
    print(json.dumps(out), flush=True)
    d.close()


def queued(ev, calls, d, out):
    """LAUNCHES calls of each kind between two events, nothing waiting in between: ms per call"""
    for k, f in calls.items():
        for _ in range(WARMUP): f()
        d.sync()
        e0, e1 = ev.new(), ev.new()
        ev.record(e0)
        for _ in range(LAUNCHES): f()
        ev.record(e1)
        out["q_" + k] = round(ev.elapsed_ms(e0, e1) / LAUNCHES, 4)
        d.sync()


def child_resident(config):
    import numpy as np
    import torch
    from bench import HipEvents
    x = setup(config)
    d, dev, S, n, B, F = x["d"], x["dev"], x["S"], x["n"], x["B"], x["F"]
    wide, outs, pairs, arena = x["wide"], x["outs"], x["pairs"], x["arena"]
    ab_in, ab_out = S * F * 6, arena.numel()
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    t_table, t_etable, t_depths, t_formats = up(x["table"]), up(x["etable"]), up(x["depths"]), up(x["formats"])
    scratch = torch.empty(max(t_table.numel(), t_etable.numel()), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    # the warrant of every DSPI_TABLE_CHECKED call below, and of the launches alone
    assert d.packets_check_resident(x["depths"], t_table.data_ptr(), n, B, ab_in) is None
    assert d.packets_emit_check_resident(x["formats"], t_etable.data_ptr(), n, B, ab_out) is None
    ev = HipEvents(d.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    out = {"streams": S, "frames": F, "input_table_bytes": t_table.numel() * 8, "emit_table_bytes": t_etable.numel() * 8}
    calls = {
        "check_input": lambda: d.debug_table_check_launch(0, t_depths.data_ptr(), t_table.data_ptr(), n, B, ab_in),
        "check_emit": lambda: d.debug_table_check_launch(1, t_formats.data_ptr(), t_etable.data_ptr(), n, B, ab_out),
        "copy_input": lambda: hip.hipMemcpyDtoDAsync(scratch.data_ptr(), t_table.data_ptr(), out["input_table_bytes"], ev.stream),
        "copy_emit": lambda: hip.hipMemcpyDtoDAsync(scratch.data_ptr(), t_etable.data_ptr(), out["emit_table_bytes"], ev.stream),
        "mixed24": lambda: d.process_mixed_device(wide.data_ptr(), x["depths"], n, B, *outs),
        "packets_host": lambda: d.process_packets_device(wide.data_ptr(), ab_in, x["depths"], x["table"], n, B, *outs),
        "packets_default": lambda: d.process_packets_resident_device(wide.data_ptr(), ab_in, x["depths"], t_table.data_ptr(), n, B, *outs),
        "packets_checked": lambda: d.process_packets_resident_device(wide.data_ptr(), ab_in, x["depths"], t_table.data_ptr(), n, B, *outs, checked=True),
        "emit_launch": lambda: d.debug_packets_emit_launch(pairs.data_ptr(), n, B, t_formats.data_ptr(), t_etable.data_ptr(), arena.data_ptr()),
        "emit_host": lambda: d.packets_emit_device(pairs.data_ptr(), n, B, x["formats"], x["etable"], arena.data_ptr(), ab_out),
        "emit_default": lambda: d.packets_emit_resident_device(pairs.data_ptr(), n, B, x["formats"], t_etable.data_ptr(), arena.data_ptr(), ab_out),
        "emit_checked": lambda: d.packets_emit_resident_device(pairs.data_ptr(), n, B, x["formats"], t_etable.data_ptr(), arena.data_ptr(), ab_out, checked=True),
    }
    for f in calls.values(): f()
    d.sync()
    timed(ev, calls, d, out)
    queued(ev, calls, d, out)
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
    legs = (["parent"] if parent else []) + ["same", "resident"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    skip = ("streams", "frames", "input_table_bytes", "emit_table_bytes", "power_w", "sclk_mhz")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m, r = line["ms"], got["resident"][-1]
    rep = {k: r[k] for k in ("streams", "frames", "input_table_bytes", "emit_table_bytes")}
    for kind in ("input", "emit"):
        rep[f"check_{kind}_over_copy"] = round(m[f"resident.check_{kind}"] / m[f"resident.copy_{kind}"], 3)
        rep[f"check_{kind}_read_tb_per_s"] = round(r[f"{kind}_table_bytes"] / m[f"resident.check_{kind}"] / 1e9, 3)
    for q in ("", "q_"):
        rep[f"{q}packets_default_over_host"] = round(m[f"resident.{q}packets_default"] / m[f"resident.{q}packets_host"], 3)
        rep[f"{q}packets_checked_over_host"] = round(m[f"resident.{q}packets_checked"] / m[f"resident.{q}packets_host"], 3)
        rep[f"{q}packets_checked_over_mixed24"] = round(m[f"resident.{q}packets_checked"] / m[f"resident.{q}mixed24"], 3)
        rep[f"{q}packets_host_over_mixed24"] = round(m[f"resident.{q}packets_host"] / m[f"resident.{q}mixed24"], 3)
        rep[f"{q}emit_default_over_host"] = round(m[f"resident.{q}emit_default"] / m[f"resident.{q}emit_host"], 3)
        rep[f"{q}emit_checked_over_host"] = round(m[f"resident.{q}emit_checked"] / m[f"resident.{q}emit_host"], 3)
        rep[f"{q}emit_checked_over_launch"] = round(m[f"resident.{q}emit_checked"] / m[f"resident.{q}emit_launch"], 3)
    line["resident"] = rep
    if parent:
        gates = {f"gate_{c}_over_parent": round(m[f"same.{c}"] / m[f"parent.{c}"], 4) for c in GATED}
        line.update(gates)
        line["criterion_gate_within_1.02"] = all(g <= 1.02 for g in gates.values())
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        return child_gated(config, leg) if leg in ("parent", "same") else child_resident(config)
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
