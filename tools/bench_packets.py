"""What input from a packet table (include/dspi.h: dspi_process_packets) costs, and that the calls it stands beside cost what they did
(profiles/packets.md).  tools/bench_link.py's method and helpers: bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract)
and config 5 (16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device buffers, per-call times by HIP events on
the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one leg each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says so),
                one context, two calls interleaved: p24 = dspi_process at 24 bit, pmixed = dspi_process_mixed, every other stream 24 bit
    same        this build, the same two calls                          GATED: same / parent within 1.02 for each
    packets     this build, the half-and-half input of pmixed as the arena, and three tables over it:
                  contiguous   the table that describes dspi_process_mixed's own layout
                  shuffled     every entry names a random packet of its stream's depth anywhere in the arena (a permutation: every packet
                               is read once, none where the layout would have it)
                  fanout       every 16-bit stream names stream 0's packets, every 24-bit stream stream 1's: two programmes
                calls:
                  intake              dspi_debug_intake on the arena: the existing kernel, not under test
                  front_contiguous, front_shuffled, front_fanout      dspi_debug_packets_intake: the table's upload and the one launch
                  packets             the whole dspi_process_packets call, shuffled table
                  mixed               dspi_process_mixed on the same input already gathered
                  copy_mixed          a hipMemcpyDtoDAsync of the same bytes, then dspi_process_mixed: the floor of a caller's own gather
                  upload              a hipMemcpyAsync of the table's bytes from pinned host memory, alone
                  kernel_contiguous, kernel_shuffled, kernel_fanout   the kernel by itself, the table already in device memory (its
                                      launcher on the null stream, waited for: a round trip of the host is in the figure)
                  packets_back_to_back, mixed_back_to_back            LAUNCHES calls queued without a wait in between, per call: the host's
                                      copy of the next table runs while the GPU works on the previous call
                RECORDED: TB/s of the three front ends (bytes read + written; fan-out: written) and their ratio to intake; packets / mixed
                and packets / copy_mixed; the table's bytes and upload time; the host's time inside one dspi_process_packets call (the
                copy of the table into the pinned area is the caller's thread's), and whether packets by the contiguous table left the
                words that mixed left

    python tools/bench_packets.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PARENT_LIB=...
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


def half_and_half(torch, dev, d, S, n, B, fs):
    """(the mixed buffer: per pair of streams 4F + 6F bytes, the depths, its size)"""
    import numpy as np
    from bench import synth_device
    from bench_mixed import widen_device
    F = n * B
    pcm = synth_device(torch, dev, S, F, fs, 1234, True, 0)
    wide = widen_device(torch, pcm)
    depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
    mixed = torch.cat([pcm[0::2].contiguous().view(torch.uint8).reshape(S // 2, -1), wide[1::2]], dim=1).contiguous()
    total, off = d.mixed_pcm_bytes(depths, n, B)
    assert total == mixed.numel() == S * F * 5
    return mixed, wide, depths, int(total), off


def child_gated(config, leg):
    import torch
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    d = make(flavor, S, w)
    if leg == "parent": assert not hasattr(d.L, "dspi_process_packets"), "PARENT_LIB has the feature: it is not the parent"
    mixed, wide, depths, total, _ = half_and_half(torch, dev, d, S, n, B, w["fs"])
    keep, outs = outputs(torch, dev, d, S, n, n * B)
    calls = {"p24": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs),
             "pmixed": lambda: d.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs)}
    out = {"streams": S, "frames": n * B}
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    from bench import HipEvents
    timed(HipEvents(d.hip_stream()), calls, d, out)
    print(json.dumps(out), flush=True)
    d.close()


def child_packets(config):
    import numpy as np
    import torch
    from bench import HipEvents
    w, flavor, dev = workload(config)
    S, n, B = w["streams"], w["blocks"], w["B"]
    F = n * B
    d, twin = make(flavor, S, w), make(flavor, S, w)
    mixed, wide, depths, total, off = half_and_half(torch, dev, d, S, n, B, w["fs"])
    size = np.where(depths == 24, 6, 4).astype(np.uint64) * np.uint64(B)
    contiguous = off[:S, None] + np.arange(n, dtype=np.uint64)[None, :] * size[:, None]
    rng = np.random.default_rng(5)
    shuffled = contiguous.copy()
    for dp in (16, 24): shuffled[depths == dp] = rng.permutation(contiguous[depths == dp].reshape(-1)).reshape(-1, n)
    fanout = np.where((depths == 24)[:, None], contiguous[1][None, :], contiguous[0][None, :]).astype(np.uint64)
    tables = {"contiguous": np.ascontiguousarray(contiguous), "shuffled": np.ascontiguousarray(shuffled), "fanout": np.ascontiguousarray(fanout)}
    for t in tables.values(): assert d.packets_check(depths, t, n, B, total) is None
    keep, outs = outputs(torch, dev, d, S, n, F)
    keep2, outs2 = outputs(torch, dev, twin, S, n, F)
    ev = HipEvents(d.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    gathered = torch.empty_like(mixed)
    table_bytes = S * n * 8 + S
    pinned = torch.empty(table_bytes, dtype=torch.uint8).pin_memory()
    t_up = torch.empty(table_bytes, dtype=torch.uint8, device=dev)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def copy_mixed():
        assert hip.hipMemcpyDtoDAsync(gathered.data_ptr(), mixed.data_ptr(), total, ev.stream) == 0
        d.process_mixed_device(gathered.data_ptr(), depths, n, B, *outs)
    # the two calls compute the same words (one call each on fresh contexts: their states are equal)
    torch.cuda.synchronize()
    d.process_packets_device(mixed.data_ptr(), total, depths, tables["contiguous"], n, B, *outs)
    twin.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs2)
    d.sync(); twin.sync()
    agree = bool(all(torch.equal(a, b) for a, b in zip(keep, keep2)))
    twin.close()
    calls = {"intake": lambda: d.debug_intake(mixed.data_ptr(), depths, n, B),
             "front_contiguous": lambda: d.debug_packets_intake(mixed.data_ptr(), total, depths, tables["contiguous"], n, B),
             "front_shuffled": lambda: d.debug_packets_intake(mixed.data_ptr(), total, depths, tables["shuffled"], n, B),
             "front_fanout": lambda: d.debug_packets_intake(mixed.data_ptr(), total, depths, tables["fanout"], n, B),
             "packets": lambda: d.process_packets_device(mixed.data_ptr(), total, depths, tables["shuffled"], n, B, *outs),
             "mixed": lambda: d.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs),
             "copy_mixed": copy_mixed,
             "upload": lambda: hip.hipMemcpyAsync(t_up.data_ptr(), pinned.data_ptr(), table_bytes, 1, ev.stream)}
    for f in calls.values(): f()
    d.sync()
    out = {"streams": S, "frames": F, "arena_bytes": total, "written_bytes": S * F * 6, "table_bytes": table_bytes, "agree": agree}
    timed(ev, calls, d, out)
    # the kernel by itself, the table already in device memory: its launcher on the null stream, which waits for it (so a round trip of the
    # host is in every figure; the front ends above also hold the host's copy of the table, for which the idle stream waits)
    raw = d.L.dspi_packetrx_launch_raw
    raw.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    t_depths = torch.from_numpy(depths).to(dev)
    t_tables = {k: torch.from_numpy(v.view(np.int64)).to(dev) for k, v in tables.items()}
    scratch = torch.empty(S * F * 6, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    kernels = {f"kernel_{k}": (lambda tt=tt: raw(mixed.data_ptr(), tt.data_ptr(), t_depths.data_ptr(), scratch.data_ptr(), S, n, B)) for k, tt in t_tables.items()}
    o2 = {}
    timed(HipEvents(0), kernels, d, o2)
    out.update({k: o2[k] for k in kernels})
    # back to back, as a host that serves a fleet makes its calls: LAUNCHES calls queued without a wait in between, so that the host's copy
    # of call i + 1's table runs while the GPU works on call i; per call
    for name in ("packets", "mixed"):
        per = []
        for i in range(WARMUP + 2):
            e0, e1 = ev.new(), ev.new()
            ev.record(e0)
            for _ in range(LAUNCHES): calls[name]()
            ev.record(e1)
            if i >= WARMUP: per.append(ev.elapsed_ms(e0, e1) / LAUNCHES)
            d.sync()
        out[name + "_back_to_back"] = med(per)
    host_ms = []
    for i in range(WARMUP + LAUNCHES):
        t0 = time.perf_counter(); calls["packets"](); t1 = time.perf_counter(); d.sync()
        if i >= WARMUP: host_ms.append((t1 - t0) * 1e3)
    out["packets_host_ms"] = med(host_ms)
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
    legs = (["parent"] if parent else []) + ["same", "packets"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    skip = ("streams", "frames", "arena_bytes", "written_bytes", "table_bytes", "agree", "power_w", "sclk_mhz")
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in v]) for leg, v in got.items() for c in v[0] if c not in skip}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m, pk = line["ms"], got["packets"][-1]
    moved = pk["arena_bytes"] + pk["written_bytes"]
    line["packets"] = {"streams": pk["streams"], "frames": pk["frames"], "arena_bytes": pk["arena_bytes"], "table_bytes_uploaded_per_call": pk["table_bytes"],
                       "outputs_agree_with_mixed": all(x["agree"] for x in got["packets"]),
                       "intake_tb_per_s": round(moved / m["packets.intake"] / 1e9, 3),
                       "front_contiguous_tb_per_s": round(moved / m["packets.front_contiguous"] / 1e9, 3),
                       "front_shuffled_tb_per_s": round(moved / m["packets.front_shuffled"] / 1e9, 3),
                       "front_fanout_written_tb_per_s": round(pk["written_bytes"] / m["packets.front_fanout"] / 1e9, 3),
                       "front_contiguous_over_intake": round(m["packets.front_contiguous"] / m["packets.intake"], 3),
                       "front_shuffled_over_intake": round(m["packets.front_shuffled"] / m["packets.intake"], 3),
                       "front_fanout_over_intake": round(m["packets.front_fanout"] / m["packets.intake"], 3),
                       "kernel_contiguous_tb_per_s": round(moved / m["packets.kernel_contiguous"] / 1e9, 3),
                       "kernel_shuffled_tb_per_s": round(moved / m["packets.kernel_shuffled"] / 1e9, 3),
                       "kernel_shuffled_over_intake": round(m["packets.kernel_shuffled"] / m["packets.intake"], 3),
                       "kernel_fanout_over_intake": round(m["packets.kernel_fanout"] / m["packets.intake"], 3),
                       "packets_over_mixed_back_to_back": round(m["packets.packets_back_to_back"] / m["packets.mixed_back_to_back"], 3),
                       "packets_over_mixed": round(m["packets.packets"] / m["packets.mixed"], 3),
                       "packets_over_copy_then_mixed": round(m["packets.packets"] / m["packets.copy_mixed"], 3),
                       "front_shuffled_over_copy_plus_intake": round(m["packets.front_shuffled"] / (m["packets.copy_mixed"] - m["packets.mixed"] + m["packets.intake"]), 3)}
    if parent:
        gates = {f"gate_{c}_over_parent": round(m[f"same.{c}"] / m[f"parent.{c}"], 4) for c in ("p24", "pmixed")}
        line.update(gates)
        line["criterion_gate_within_1.02"] = all(g <= 1.02 for g in gates.values())
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        config, leg = sys.argv[2], sys.argv[3]
        return child_gated(config, leg) if leg in ("parent", "same") else child_packets(config)
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
