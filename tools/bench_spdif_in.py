"""What S/PDIF input (include/dspi.h: dspi_process_sources, dspi_spdif_decode) costs, and that the calls it stands beside cost what they did
(profiles/spdif_in.md).  tools/bench_mixed.py's method: bench.py's config 3 (65 536 float streams, 96-frame packets, FMA contract) and config
5 (16 384 Q28 streams, 48-frame packets) at their own sizes (50 packets per call), device buffers, stream-major words, per-call times by HIP
events on the context's stream after a warm-up, medians, shader clock and socket power per child.

Alternating child processes, one context each, ROUNDS times, and the median over the children's medians.  Legs:
    parent      the PARENT commit's library (PARENT_LIB=<path of its libdspi_mi355x.so>; without it the leg is skipped and the line says
                so), one context, two calls interleaved: p24 = dspi_process at 24 bit, pmixed = dspi_process_mixed, depths 16 / 24 by s % 2
    same        this build, the same two calls                               row 1, criterion: same / parent <= 1.02 for both calls
    spdif       this build, one context whose every source is S/PDIF (the lines are the library's own dspi_spdif_encode output of the
                24-bit input, block positions 0), four calls interleaved, call by call:
                  sources   dspi_process_sources
                  decoder   the receiver launch of that call alone (dspi_debug_sources_intake: dspi_spdifrx.hip, timed by itself)
                  decoded   dspi_process at 24 bit on the same input decoded beforehand
                  copy      a hipMemcpyDtoDAsync of 11 bytes per frame (the decoder reads 16 and writes 6: 22 moved either way) on the same stream
                row 2, recorded: decoder / copy (beside the intake's 1.04 x / 1.29 x of profiles/mixed_input.md)
                row 3, recorded: sources / decoded

    python tools/bench_spdif_in.py [3 5]        ROUNDS=2 LAUNCHES=8 WARMUP=2 PACKETS=... STREAMS=... PARENT_LIB=...
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
PACKETS, STREAMS = int(os.environ.get("PACKETS", 0)), int(os.environ.get("STREAMS", 0))
med = lambda v: round(statistics.median(v), 4)


def spdif_lines(torch, flavor, wide, S, F, fs):
    """packed 24-bit input uint8 [S][6 F] -> its S lines of subframes, int32 [S][F][4], through the library's own encoder on a helper context
    (dspi_spdif_encode takes n_streams * pairs lines at once)"""
    from dspi_amd.host import Dspi
    b = wide.reshape(S, 2 * F, 3).to(torch.int32)
    v = b[:, :, 0] | b[:, :, 1] << 8 | b[:, :, 2] << 16
    v = ((v ^ 0x800000) - 0x800000).reshape(S, F, 2)
    e = Dspi(flavor, 1, device=0)
    P = e.P
    e.close()
    n = (S + P - 1) // P
    e = Dspi(flavor, n, device=0)
    e.set_rate(fs)
    pairs = torch.zeros((n * P, F, 2), dtype=torch.int32, device=wide.device)
    pairs[:S] = v
    out = torch.empty((n * P, F, 4), dtype=torch.int32, device=wide.device)
    torch.cuda.synchronize()
    e.spdif_device(pairs.data_ptr(), F, 0, out.data_ptr())
    e.sync()
    e.close()
    return out[:S].contiguous()


def child(config, leg):
    """one context, LAUNCHES timed rounds of the leg's calls: a JSON line {call: median ms}"""
    import numpy as np
    import time
    import torch
    from bench import HipEvents, PowerSampler, chain_workload, synth_device
    from bench_mixed import widen_device
    from dspi_amd import host, wire as W
    from dspi_amd.host import Dspi
    w = chain_workload(config)
    S, n, B = STREAMS or w["streams"], PACKETS or w["blocks"], w["B"]
    F = n * B
    assert S % 2 == 0
    dev = torch.device("cuda", 0)
    flavor = W.F32_FMA if w["flavor"] else 0
    d = Dspi(flavor, S, device=0)
    d.set_rate(w["fs"]); d.set_volume(w["vol"])
    assert d.load_bulk(w["blob"]) == 0
    if leg == "parent": assert not hasattr(d.L, "dspi_process_sources"), "PARENT_LIB has the feature: it is not the parent"
    pcm = synth_device(torch, dev, S, F, w["fs"], 1234, True, 0)
    wide = widen_device(torch, pcm)                                   # [S][6F]
    pairs = torch.empty((S, d.P, F, 2), dtype=torch.int32, device=dev)
    sub = torch.empty((S, F), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, n, d.C), dtype=torch.int16, device=dev)
    outs = (pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())
    ev = HipEvents(d.hip_stream())
    out = {"streams": S, "frames": F}
    if leg in ("parent", "same"):
        depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
        mixed = torch.cat([pcm[0::2].contiguous().view(torch.uint8).reshape(S // 2, -1), wide[1::2]], dim=1).contiguous()
        calls = {"p24": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs),
                 "pmixed": lambda: d.process_mixed_device(mixed.data_ptr(), depths, n, B, *outs)}
    else:
        src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
        lines = spdif_lines(torch, flavor, wide, S, F, w["fs"])
        total, _ = d.sources_bytes(src, n, B)
        assert total == lines.numel() * 4 == S * F * 16
        rx = torch.zeros(S * 40, dtype=torch.uint8, device=dev)
        moved = S * F * 11
        a, b = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
        hip = ev.hip
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

        def copy(): assert hip.hipMemcpyDtoDAsync(b.data_ptr(), a.data_ptr(), moved, ev.stream) == 0
        calls = {"sources": lambda: d.process_sources_device(lines.data_ptr(), src, n, B, rx.data_ptr(), *outs),
                 "decoder": lambda: d.debug_sources_intake(lines.data_ptr(), src, n, B, rx.data_ptr()),
                 "decoded": lambda: d.process_device(wide.data_ptr(), n, B, 24, *outs), "copy": copy}
        out.update(decoder_bytes_read=int(total), decoder_bytes_written=S * F * 6, copy_bytes=int(moved))
    torch.cuda.synchronize()
    for f in calls.values(): f()
    d.sync()
    if leg == "spdif":      # the lines are what the decoder is there for: every receiver locked at the context's rate, nothing concealed
        r = rx.cpu().numpy().view(host.SPDIF_RX)
        assert (r["state"] == 2).all() and (r["sample_rate"] == w["fs"]).all() and not r["held"].any() and not r["coding_errors"].any(), "the bench's lines do not decode cleanly"
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
    out.update(power_w=pw and round(pw["power_w"], 1), sclk_mhz=pw and pw["sclk_mhz"] and round(pw["sclk_mhz"]), plan={k: v for k, v in d.launch_plan().items() if v})
    print(json.dumps(out), flush=True)
    d.close()


def run_child(config, leg, lib):
    env = dict(os.environ)
    if lib: env["DSPI_LIB"] = lib
    else: env.pop("DSPI_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, leg], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError(f"child {config} {leg} ({lib or 'this build'}): {out.stderr[-600:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


CALLS = {"parent": ("p24", "pmixed"), "same": ("p24", "pmixed"), "spdif": ("sources", "decoder", "decoded", "copy")}


def measure(config, parent):
    line = {"config": config, "rounds": ROUNDS, "launches": LAUNCHES, "warmup": WARMUP}
    legs = (["parent"] if parent else []) + ["same", "spdif"]
    got = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs: got[k].append(run_child(config, k, parent if k == "parent" else None))
    last = got["spdif"][-1]
    line.update(streams=last["streams"], frames=last["frames"], plan=last["plan"], decoder_bytes_read=last["decoder_bytes_read"],
                decoder_bytes_written=last["decoder_bytes_written"], copy_bytes=last["copy_bytes"])
    line["ms"] = {f"{leg}.{c}": med([x[c] for x in got[leg]]) for leg in legs for c in CALLS[leg]}
    line["children_ms"] = {f"{leg}.{c}": [x[c] for x in got[leg]] for leg in legs for c in CALLS[leg]}
    line["power_w"] = {k: [x["power_w"] for x in v] for k, v in got.items()}
    line["sclk_mhz"] = {k: [x["sclk_mhz"] for x in v] for k, v in got.items()}
    m = line["ms"]
    line["row2_decoder_over_copy"] = round(m["spdif.decoder"] / m["spdif.copy"], 4)
    line["decoder_tb_per_s"] = round((line["decoder_bytes_read"] + line["decoder_bytes_written"]) / m["spdif.decoder"] / 1e9, 3)
    line["call_minus_chain_ms"] = round(m["spdif.sources"] - m["spdif.decoded"], 4)
    line["row3_sources_over_decoded"] = round(m["spdif.sources"] / m["spdif.decoded"], 4)
    if parent:
        line["row1_p24_over_parent"] = round(m["same.p24"] / m["parent.p24"], 4)
        line["row1_pmixed_over_parent"] = round(m["same.pmixed"] / m["parent.pmixed"], 4)
        line["criterion_row1_le_1.02"] = max(line["row1_p24_over_parent"], line["row1_pmixed_over_parent"]) <= 1.02
    else: line["parent"] = "skipped: PARENT_LIB not set"
    return line


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child": return child(sys.argv[2], sys.argv[3])
    parent = os.environ.get("PARENT_LIB")
    for config in [a for a in sys.argv[1:] if not a.startswith("--")] or ["3", "5"]:
        print(json.dumps(measure(config, os.path.abspath(parent) if parent else None)), flush=True)


if __name__ == "__main__":
    main()
