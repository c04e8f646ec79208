"""bench.py's plain run and --dump-outputs on the GPU: one line with the headline keys, exactly --steps timed steps, and a dump of the last
timed step that is the same on every run with the same arguments and bit-exact against the CPU oracle replaying the context's launches."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", "1024"]


def run_bench(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DSPI_BENCH_FORCE_DIST"): env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    import torch
    import orclib
    spec = importlib.util.spec_from_file_location("dspi_bench_for_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)

    a, b = run_bench(tmp_path / "a"), run_bench(tmp_path / "b")
    for rec in (a, b):
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
        assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["metric"]
        assert rec["parity_checked"] == 0 and "cpu_baseline" not in rec and "also" not in rec and "configs" not in rec      # --full only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["packets.npy", "pairs.npy", "peaks.npy", "streams.npy", "sub.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.array_equal(x, y), n
    # the dump is the timed context's last launch: the oracle replays warm-up + pre-load + timed launches on the same input buffer
    w = bench.chain_workload("3")
    S, NB, B, fs = 1024, w["blocks"], w["B"], w["fs"]
    launches = a["warmup"] + a["config"]["preload_steps"] + a["steps"]
    assert a["config"]["preload_steps"] == b["config"]["preload_steps"] == bench.preload_steps(S * NB * B, 1)
    pcm = bench.synth_device(torch, torch.device("cuda", 0), S, NB * B, fs, 1234, True).cpu().numpy()
    idx = np.load(tmp_path / "a" / "streams.npy").astype(np.int64)
    pairs, sub, peaks = (np.load(tmp_path / "a" / n) for n in ("pairs.npy", "sub.npy", "peaks.npy"))
    for j in (0, len(idx) - 1):
        s = int(idx[j])
        o = orclib.Oracle(1, detmath=True, fma=True)
        o.set_rate(fs); o.set_volume(w["vol"]); assert o.load_bulk(w["blob"]) == 0
        for _ in range(launches):
            rp, rs, rk, _ = o.process(pcm[s], NB, B, 16)
        assert np.array_equal(rp, pairs[j]) and np.array_equal(rs, sub[j]), s
        assert np.array_equal(rk.view(np.int16), peaks[j]), s
