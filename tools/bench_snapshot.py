"""Throughput of stream snapshots (dspi_export_streams / dspi_import_streams, include/dspi.h) with device buffers: whole-context export
and import at 4 096 and 65 536 float streams and 16 384 Q28 streams, timed with HIP events on the context's stream after a warm-up,
median of at least REPS = 20 repetitions (more, until a timed region lasts MIN_WINDOW_S = 0.6 s: clock and power settle).  The yardstick is a hipMemcpyDtoDAsync of the same number of bytes on the same stream in the same run: one
read and one write per byte is the least a hand-over can cost, and all the transposition needs.  A context larger than the record
buffer (BUF_GB, default 4) is moved in chunks of whole rows through it, all chunks inside one timed region; the copy is timed the
same way.  Prints one JSON line per case.

    python tools/bench_snapshot.py [f32:4096 f32:65536 q28:16384]      REPS=20 WARMUP=3 BUF_GB=4 MIN_WINDOW_S=0.6
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

from bench import HipEvents, PowerSampler  # noqa: E402
from dspi_amd import wire as W  # noqa: E402
from dspi_amd.host import Dspi  # noqa: E402

REPS, WARMUP, BUF_GB = int(os.environ.get("REPS", 20)), int(os.environ.get("WARMUP", 3)), float(os.environ.get("BUF_GB", 4))
MIN_WINDOW_S = float(os.environ.get("MIN_WINDOW_S", 0.6))      # every timed region lasts at least this long (repetitions are added beyond REPS)


def case(flavor_name: str, S: int, smi):
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

    export(); d.sync()      # (heads for the import; an import of a context's own export leaves it as it is)
    out = {"flavor": flavor_name, "streams": S, "record_bytes": rec, "bytes": S * rec, "chunks": len(ranges), "warmup": WARMUP}
    for name, fn in (("copy", copy), ("export", export), ("import", imp)):
        med, best, win, reps = timed(fn)
        pw = smi.window(*win) if smi and smi.ok else None
        out[name] = {"ms": round(med, 4), "ms_min": round(best, 4), "reps": reps, "gb_per_s_read_plus_write": round(2 * S * rec / med / 1e6, 1),
                     "power_w": pw and round(pw["power_w"], 1), "sclk_mhz": pw and pw["sclk_mhz"] and round(pw["sclk_mhz"])}
    out["export_over_copy"] = round(out["export"]["ms"] / out["copy"]["ms"], 3)
    out["import_over_copy"] = round(out["import"]["ms"] / out["copy"]["ms"], 3)
    d.close()
    print(json.dumps(out), flush=True)


def main():
    cases = sys.argv[1:] or ["f32:4096", "f32:65536", "q28:16384"]
    smi = PowerSampler(0)
    smi.start()
    try:
        for c in cases:
            name, s = c.split(":")
            case(name, int(s), smi)
            torch.cuda.empty_cache()
    finally:
        smi.stop()


if __name__ == "__main__":
    main()
