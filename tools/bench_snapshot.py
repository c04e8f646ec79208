"""Throughput of stream snapshots (dspi_export_streams / dspi_import_streams, include/dspi.h) with device buffers: whole-context export
and import at 4 096 and 65 536 float streams and 16 384 Q28 streams, timed with HIP events on the context's stream after a warm-up,
median of at least REPS = 20 repetitions (more, until a timed region lasts MIN_WINDOW_S = 0.6 s: clock and power settle).  The yardstick is a hipMemcpyDtoDAsync of the same number of bytes on the same stream in the same run: one
read and one write per byte is the least a hand-over can cost, and all the transposition needs.  A context larger than the record
buffer (BUF_GB, default 4) is moved in chunks of whole rows through it, all chunks inside one timed region; the copy is timed the
same way.  Prints one JSON line per case.

    python tools/bench_snapshot.py [f32:4096 f32:65536 q28:16384]      REPS=20 WARMUP=3 BUF_GB=4 MIN_WINDOW_S=0.6

--realign (profiles/realign.md) adds two things:
  * to each of the cases above the REALIGNING import (DSPI_SNAP_REALIGN), in the same run as the copy and the plain import.  An import of a
    context's own export would rotate nothing, so the context is given the full-chain preset and run to a position p1, exported, run on
    to p2 = p1 + 225 frames and the first stream of every row exported again: the records then hold rows whose first stream stands at p2 and
    whose other streams at p1, and the import — whole rows, no residents: each row aligns to its first stream — rotates all but one stream
    of every row by 225 words: odd, not a multiple of four, wrapping.  The plain import is timed on the same records.
  * what misaligned rows cost dspi_process and that realigning removes it (--realign=cost alone; --realign=import for the first part alone):
    bench.py's config 3 (65 536 float streams, 96-frame packets, 50 packets per launch, FMA contract, stream-major) and config 5 (16 384 Q28
    streams), per-launch times by HIP events, contexts alternating launch by launch in one process (three phases, a in each: a b1 b2,
    a c1 c2, a b2r), medians, every ratio against the a of its own phase:
      a    the undisturbed context                               b2r  b2 after dspi_realign_streams over the whole context (whose own
      b1   a + one stream per row imported plainly from a donor       time is reported too)
           of another age                                        c1   b1's imports with DSPI_SNAP_REALIGN
      b2   a + every row imported plainly from eight donors      c2   b2's imports with DSPI_SNAP_REALIGN
           of different ages, round-robin by stream
    COST_ROUNDS=15 COST_WARMUP=3
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import HipEvents, PowerSampler, chain_workload, synth_device  # noqa: E402
from dspi_amd import wire as W  # noqa: E402
from dspi_amd.host import Dspi  # noqa: E402

REPS, WARMUP, BUF_GB = int(os.environ.get("REPS", 20)), int(os.environ.get("WARMUP", 3)), float(os.environ.get("BUF_GB", 4))
MIN_WINDOW_S = float(os.environ.get("MIN_WINDOW_S", 0.6))      # every timed region lasts at least this long (repetitions are added beyond REPS)


COST_ROUNDS, COST_WARMUP = int(os.environ.get("COST_ROUNDS", 15)), int(os.environ.get("COST_WARMUP", 3))


def case(flavor_name: str, S: int, smi, realign=False):
    flavor = {"f32": W.F32_FMA, "q28": 0}[flavor_name]
    d = Dspi(flavor, S, device=0)
    rec = d.snapshot_sizes(0, 1)[1]
    R = d.tile_streams()
    chunk = min(S, max(R, int(BUF_GB * (1 << 30)) // rec // R * R))
    buf = torch.empty(chunk * rec // 4, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(buf)
    ev = HipEvents(d.hip_stream())
    hip = ev.hip
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    ranges = [(f, min(chunk, S - f)) for f in range(0, S, chunk)]
    heads = {}

    def export():
        for f, n in ranges: heads[f] = d.export_streams_device(f, n, buf.data_ptr(), n * rec)

    def imp():
        for f, n in ranges: d.import_streams_device(f, heads[f], buf.data_ptr(), n * rec)

    def copy():
        for f, n in ranges: assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), buf.data_ptr(), n * rec, ev.stream) == 0

    def timed(fn):
        for _ in range(WARMUP): fn()
        d.sync()
        t = time.perf_counter(); fn(); d.sync()
        reps = max(REPS, min(3000, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-5)) + 1))      # a window of a fraction of a second measures the clock ramp
        ms, t0 = [], time.perf_counter()
        for _ in range(reps):
            a, b = ev.new(), ev.new()
            ev.record(a); fn(); ev.record(b)
            ms.append(ev.elapsed_ms(a, b))
        return statistics.median(ms), min(ms), (t0, time.perf_counter()), reps

    def imp_realign():
        for f, n in ranges: d.import_streams_device(f, heads[f], buf.data_ptr(), n * rec, realign=True)

    if realign:      # positions p1 for every stream, p2 = p1 + 225 for the first stream of every row (see the top of the file)
        from dspi_amd import workloads as WL
        fs, B = 44100, 45
        d.set_rate(fs); d.set_volume(-20 * 256)
        assert d.load_bulk(WL.full_chain_blob(flavor)) == 0
        pcm = torch.zeros((S, 5 * B, 2), dtype=torch.int16, device="cuda")
        peaks = torch.empty((S, 5, 11), dtype=torch.int16, device="cuda")
        run5 = lambda: d.process_device(pcm.data_ptr(), 5, B, 16, 0, 0, peaks.data_ptr())
        run5(); run5(); run5(); d.sync()
        p1 = [int(x[0]) for x in d.stream_positions(0, 1)]
    export(); d.sync()      # (heads for the import; an import of a context's own export leaves it as it is)
    out = {"flavor": flavor_name, "streams": S, "record_bytes": rec, "bytes": S * rec, "chunks": len(ranges), "warmup": WARMUP}

    def mix_rows():      # after the timed exports (they rewrite `buf`): on to p2, and the first stream of every row exported again
        run5(); d.sync()
        p2 = [int(x[0]) for x in d.stream_positions(0, 1)]
        one = torch.empty(rec // 4, dtype=torch.int32, device="cuda")
        view = buf.view(chunk, rec // 4)      # (every chunk is imported from this one buffer: all of its rows are mixed)
        for k in range(0, chunk, R):
            d.export_streams_device(k, 1, one.data_ptr(), rec); d.sync()
            view[k].copy_(one)
        torch.cuda.synchronize()
        out["realign"] = {"positions_rows_mates": p1, "positions_rows_first_stream": p2, "rotation_words": p2[0] - p1[0]}
    for name, fn in (("copy", copy), ("export", export), ("import", imp)) + ((("import_realign", imp_realign),) if realign else ()):
        if realign and name == "import": mix_rows()
        med, best, win, reps = timed(fn)
        pw = smi.window(*win) if smi and smi.ok else None
        out[name] = {"ms": round(med, 4), "ms_min": round(best, 4), "reps": reps, "gb_per_s_read_plus_write": round(2 * S * rec / med / 1e6, 1),
                     "power_w": pw and round(pw["power_w"], 1), "sclk_mhz": pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])}
    out["export_over_copy"] = round(out["export"]["ms"] / out["copy"]["ms"], 3)
    out["import_over_copy"] = round(out["import"]["ms"] / out["copy"]["ms"], 3)
    if realign:
        out["import_realign_over_copy"] = round(out["import_realign"]["ms"] / out["copy"]["ms"], 3)
        out["import_realign_over_import"] = round(out["import_realign"]["ms"] / out["import"]["ms"], 3)
        w, r = d.stream_positions(0, min(S, 4 * R))
        out["realign"]["uniform_after"] = bool((w == w[0]).all() and (r == r[0]).all()) if len(ranges) == 1 else None      # (chunked: `buf` held the last chunk only)
    d.close()
    print(json.dumps(out), flush=True)


def cost_case(config: str, smi):
    """What misaligned rows cost dspi_process (see the top of the file).  One JSON line."""
    w = chain_workload(config)
    flavor = W.F32_FMA if w["flavor"] else 0
    S, fs, B, NB = w["streams"], w["fs"], w["B"], w["blocks"]
    frames = NB * B
    dev = torch.device("cuda", 0)
    _, N, P, _, _ = W.dims(w["flavor"])
    pcm = synth_device(torch, dev, S, frames, fs, 1234, True, 0)
    pairs = torch.empty((S, P, frames, 2), dtype=torch.int32, device=dev)
    sub = torch.empty((S, frames), dtype=torch.int32, device=dev)
    peaks = torch.empty((S, NB, 2 + N), dtype=torch.int16, device=dev)

    def context(n):
        d = Dspi(flavor, n, device=0)
        d.set_rate(fs); d.set_volume(w["vol"])
        assert d.load_bulk(w["blob"]) == 0
        return d

    def launch(d):
        d.process_device(pcm.data_ptr(), NB, B, 16, pairs.data_ptr(), sub.data_ptr(), peaks.data_ptr())

    names = ["a", "b1", "b2", "c1", "c2"]
    ctx = {k: context(S) for k in names}
    R = ctx["a"].tile_streams()
    rows = S // R
    rec = ctx["a"].snapshot_sizes(0, 1)[1]
    for d in ctx.values():
        for _ in range(3): launch(d)
        d.sync()
    # eight donors of one row each, of ages other than the contexts' three launches
    ages = (1, 2, 4, 5, 6, 7, 8, 9)
    rowbuf = torch.empty((R, rec // 4), dtype=torch.int32, device=dev)
    tmp = torch.empty_like(rowbuf)
    donor_pos = []
    for i, age in enumerate(ages):
        dn = context(R)
        for _ in range(age): launch(dn)
        head_row = dn.export_streams_device(0, R, tmp.data_ptr(), R * rec); dn.sync()
        rowbuf[i::8].copy_(tmp[i::8])
        if i == 0:
            one = tmp[5].clone()
            head_one = dn.export_streams_device(5, 1, tmp.data_ptr(), rec); dn.sync()      # (the head of a one-stream snapshot; the record is `one`)
        donor_pos.append([int(x[0]) for x in dn.stream_positions(0, 1)])
        dn.close()
    torch.cuda.synchronize()
    for k, realign in (("b1", False), ("c1", True)):
        for row in range(rows): ctx[k].import_streams_device(row * R + 5, head_one, one.data_ptr(), rec, realign=realign)
    for k, realign in (("b2", False), ("c2", True)):
        for row in range(rows): ctx[k].import_streams_device(row * R, head_row, rowbuf.data_ptr(), R * rec, realign=realign)
    for d in ctx.values(): d.sync()

    def distinct(d):      # distinct (write index, ring position) pairs in the context's first row / in the whole context
        wv, rv = d.stream_positions(0, S)
        return len(set(zip(wv[:R].tolist(), rv[:R].tolist()))), len(set(zip(wv.tolist(), rv.tolist())))
    out = {"config": config, "flavor": "f32" if w["flavor"] else "q28", "streams": S, "rows": rows, "block_len": B, "blocks_per_launch": NB, "rounds": COST_ROUNDS, "warmup_rounds": COST_WARMUP,
           "context_positions": [int(x[0]) for x in ctx["a"].stream_positions(0, 1)], "donor_positions": donor_pos,
           "distinct_positions_row0_and_context": {k: distinct(d) for k, d in ctx.items()}}
    evs = {k: HipEvents(d.hip_stream()) for k, d in ctx.items()}

    def alternate(order, rounds, warm):
        ms = {k: [] for k in order}
        t0 = None
        for i in range(warm + rounds):
            if i == warm: t0 = time.perf_counter()
            for k in order:
                ev, d = evs[k], ctx[k]
                e0, e1 = ev.new(), ev.new()
                ev.record(e0); launch(d); ev.record(e1)
                t = ev.elapsed_ms(e0, e1)      # (waits for the launch: the contexts never overlap)
                if i >= warm: ms[k].append(t)
        return ms, (t0, time.perf_counter())

    # three phases, each alternating with a: the misaligned contexts (a b1 b2), the realigned ones (a c1 c2) and, further down, b2 after
    # dspi_realign_streams (a b2r).  (One rotation over all five lets whatever follows b2 — a launch several times as long, at the board's
    # power limit — run at a lower clock than a does: profiles/realign.md, section 2.)
    med = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["process_ms"], out["over_a"], out["power_w"], out["sclk_mhz"] = {}, {}, {}, {}
    for phase, order in (("misaligned", ["a", "b1", "b2"]), ("realigned", ["a", "c1", "c2"])):
        ms, win = alternate(order, COST_ROUNDS, COST_WARMUP)
        pw = smi.window(*win) if smi and smi.ok else None
        out["power_w"][phase], out["sclk_mhz"][phase] = pw and round(pw["power_w"], 1), pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])
        out["process_ms"][phase] = {k: med(v) for k, v in ms.items()}
        out["over_a"].update({k: round(statistics.median(ms[k]) / statistics.median(ms["a"]), 4) for k in order if k != "a"})
    out["plans"] = {k: {p: n for p, n in d.launch_plan().items() if n} for k, d in ctx.items()}
    # b2, realigned in place: the call's own time (twice: the second call moves nothing and does the same work), then a against b2r
    ev, d = evs["b2"], ctx["b2"]
    t = []
    for _ in range(2):
        e0, e1 = ev.new(), ev.new()
        ev.record(e0); d.realign_streams(0, S); ev.record(e1)
        t.append(round(ev.elapsed_ms(e0, e1), 3))
    out["realign_streams_ms"] = t
    out["distinct_positions_row0_and_context"]["b2r"] = distinct(d)
    ms2, win = alternate(["a", "b2"], COST_ROUNDS, COST_WARMUP)
    pw = smi.window(*win) if smi and smi.ok else None
    out["power_w"]["realigned_in_place"], out["sclk_mhz"]["realigned_in_place"] = pw and round(pw["power_w"], 1), pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])
    out["process_ms"]["realigned_in_place"] = {"a": med(ms2["a"]), "b2r": med(ms2["b2"])}
    out["over_a"]["b2r"] = round(statistics.median(ms2["b2"]) / statistics.median(ms2["a"]), 4)
    for d in ctx.values(): d.close()
    print(json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    mode = next((a for a in argv if a.startswith("--realign")), None)
    cases = [a for a in argv if not a.startswith("--")]
    what = (mode.partition("=")[2] or "both") if mode else None
    assert what in (None, "both", "import", "cost"), "--realign[=import|cost]"
    smi = PowerSampler(0)
    smi.start()
    try:
        if what != "cost":
            for c in [c for c in cases if ":" in c] or ["f32:4096", "f32:65536", "q28:16384"]:
                name, s = c.split(":")
                case(name, int(s), smi, realign=bool(mode))
                torch.cuda.empty_cache()
        if what in ("both", "cost"):
            for c in [c for c in cases if ":" not in c] or ["3", "5"]:      # bench.py's configs: 3 = 65 536 float streams, 5 = 16 384 Q28 streams
                cost_case(c, smi)
                torch.cuda.empty_cache()
    finally:
        smi.stop()


if __name__ == "__main__":
    main()
