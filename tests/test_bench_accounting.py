"""bench.py's byte accounting and input generator, on CPU: the algorithmic bytes per frame of every chain config (SURVEY.md section 8d:
both the HBM-resident-delay-line figure the roofline fraction uses and the launch-span figure), the profile lookup by kernel variant,
and the stream classes of the synthetic mix."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("dspi_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_algorithmic_bytes():
    w = bench.chain_workload("3")
    a = bench.algorithmic_bytes(w, 50 * 96)
    assert a["resident"] == 104.0                 # 4 in + 8 x 4 S/PDIF words + 4 sub + 8 x 8 delayed outputs (write + read)
    assert 55.0 < a["span"] < 65.0                # delays shorter than the 4 800-frame launch count only dly/T of their 8 bytes
    # the strict figure (roofline.frac): 40 + 4 * (sum of min(dly, T) over the 8 delayed outputs + 8 * min(4096, T)) / T with the lines'
    # whole history kept — 48 + 96 + 192 + 480 + 960 + 1920 + 3840 + 4096 delay samples at 96 kHz
    assert abs(a["exact"] - (40.0 + 4.0 * (11632 + 8 * 4096) / 4800.0)) < 1e-9 and 76.9 < a["exact"] < 77.1
    assert a["span"] < a["exact"] < a["resident"]
    big, one = bench.algorithmic_bytes(w, 10 ** 9), bench.algorithmic_bytes(w, 1)
    assert big["span"] < 41.0 and big["exact"] < 41.0 and one["span"] == one["exact"] == one["resident"] == 104.0
    assert bench.algorithmic_bytes(bench.chain_workload("2"), 2000 * 48) == dict(exact=12.0, resident=12.0, span=12.0)
    q = bench.algorithmic_bytes(bench.chain_workload("5"), 50 * 48)
    assert q["resident"] == 56.0                  # 4 in + 4 x 4 words + 4 sub + 4 x 8 delayed outputs
    assert 24.0 < q["span"] < q["exact"] < 56.0   # 2 048-sample lines, 2 400-frame launches
    for name in ("perstream", "perstream_eq"):
        assert bench.algorithmic_bytes(bench.chain_workload(name), 50 * 96)["resident"] == 104.0


def test_profile_lookup_matches_the_variant():
    found = 0
    for key, contract, layout in (("chain3", "fma", "stream"), ("chain3", "fma", "tiled"), ("chain3", "canonical", "tiled"), ("chain5", "integer", "stream"),
                                  ("perstream", "fma", "stream")):
        p = bench.latest_profile(key, contract, layout)
        if p is None: continue
        found += 1
        t = json.load(open(os.path.join(ROOT, "profiles", p["source"])))
        assert t.get("kernel_key", "chain3") == key and t.get("contract", "canonical") == contract and t.get("out_layout", "stream") == layout
        assert 50.0 < p["hbm_bytes_per_frame"] < 400.0
    assert found >= 3
    assert bench.latest_profile("no-such-kernel", "fma", "stream") is None


def test_synthetic_mix_classes():
    fs, frames, S = 96000, 4800, 40
    pcm = bench.synth_device(torch, torch.device("cpu"), S, frames, fs, 7, True).numpy()
    assert pcm.shape == (S, frames, 2) and pcm.dtype == np.int16
    assert np.abs(pcm[0]).max() <= 16384 and np.abs(pcm[0]).max() > 12000            # white noise at -6 dBFS
    assert not pcm[18].any() and not pcm[38].any()                                    # digital silence
    assert set(np.unique(pcm[19, :, 0]).tolist()) == {-32768, 32767}                  # full-scale square
    assert np.abs(pcm[16, :frames // 2]).max() < 1100 < np.abs(pcm[16, frames // 2:]).max()      # bursts: -30 dBFS then -6 dBFS
    assert 8000 < np.abs(pcm[14]).max() <= 8231                                       # sweep at -12 dBFS
    shifted = bench.synth_device(torch, torch.device("cpu"), 4, frames, fs, 7, True, first_stream=16).numpy()
    assert not shifted[2].any()                                                       # classes follow the GLOBAL stream index (shards)
    noise = bench.synth_device(torch, torch.device("cpu"), S, frames, fs, 7, False).numpy()
    assert noise[18].any()


def test_source_fingerprint_tracks_the_kernel_sources(tmp_path):
    """Counter profiles carry the fingerprint of the sources they were taken from (tools/prof_summary.py); bench.py marks
    roofline.traffic stale when the tree it runs from has another one."""
    from dspi_amd import host
    a = host.source_fingerprint()
    assert len(a) == 16 and a == host.source_fingerprint()
    pkg = tmp_path / "pkg"; (pkg / "csrc").mkdir(parents=True); (tmp_path / "include").mkdir()
    (pkg / "csrc" / "k.hip").write_text("kernel"); (tmp_path / "include" / "api.h").write_text("api")
    f0 = host.source_fingerprint(pkg)
    (pkg / "csrc" / "k.hip").write_text("kernel, edited")
    f1 = host.source_fingerprint(pkg)
    (tmp_path / "include" / "api.h").write_text("api v2")
    assert len({f0, f1, host.source_fingerprint(pkg), a}) == 4
    p = bench.latest_profile("chain3", "fma", "stream")
    if p is not None: assert "src_sha16" in p


def test_dump_outputs_sample_is_layout_independent_and_capped(tmp_path):
    """--dump-outputs: the same seeded streams, stream-major, whichever word layout the timed path wrote; float64; under 64 MB."""
    S, P, R, frames, nb, n_out = 300, 4, 64, 96, 2, 9
    g = torch.Generator().manual_seed(5)
    pairs = torch.randint(-(1 << 23), 1 << 23, (S, P, frames, 2), dtype=torch.int32, generator=g)
    sub = torch.randint(-(1 << 30), 1 << 30, (S, frames), dtype=torch.int32, generator=g)
    peaks = torch.randint(0, 1 << 15, (S, nb, 2 + n_out), dtype=torch.int16, generator=g)
    tiles = (S + R - 1) // R
    tp = torch.zeros((tiles * R, P, frames, 2), dtype=torch.int32); tp[:S] = pairs      # [tile][output][frame][R]
    tp = tp.reshape(tiles, R, P, frames, 2).permute(0, 2, 4, 3, 1).reshape(tiles, 2 * P, frames, R).contiguous()
    ts = torch.zeros((tiles * R, frames), dtype=torch.int32); ts[:S] = sub
    ts = ts.reshape(tiles, R, frames).permute(0, 2, 1).contiguous()                       # [tile][frame][R]
    bench.dump_chain_outputs(str(tmp_path / "s"), torch, pairs, sub, peaks, False, R, S, P, frames, nb, n_out)
    bench.dump_chain_outputs(str(tmp_path / "t"), torch, tp, ts, peaks, True, R, S, P, frames, nb, n_out)
    names = sorted(p.name for p in (tmp_path / "s").iterdir())
    assert names == ["packets.npy", "pairs.npy", "peaks.npy", "streams.npy", "sub.npy"]
    idx = np.load(tmp_path / "s" / "streams.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s" / "packets.npy"), np.arange(nb))
    assert len(idx) == 128 and len(set(idx)) == 128 and idx.max() < S
    for n in names:
        a, b = np.load(tmp_path / "s" / n), np.load(tmp_path / "t" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "s" / "pairs.npy"), pairs.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "s" / "sub.npy"), sub.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "s" / "peaks.npy"), peaks.numpy()[idx])
    # the full-size headline (65 536 streams x 4 800 frames) stays under the cap
    per_stream = 8 * (P * 4800 * 2 + 4800 + 50 * (2 + n_out))
    assert min(128, bench.DUMP_BYTES // per_stream) * per_stream + 1024 < 64e6
    bench.dump_flat_output(str(tmp_path / "f"), torch, torch.arange(10 ** 6, dtype=torch.int32), "words")
    w, i = np.load(tmp_path / "f" / "words.npy"), np.load(tmp_path / "f" / "words_index.npy")
    assert np.array_equal(w, i) and w.dtype == np.float64


def test_preload_is_fixed_by_the_workload():
    """The untimed pre-load is a step count set by the launch's size (~52 launches of the headline before its timed region), never by a
    clock: the chain's state carries over, so only a fixed history makes the last step's words reproducible (--dump-outputs)."""
    assert bench.preload_steps(65536 * 4800, 10) == 76 and bench.preload_steps(65536 * 4800, 5) == 81      # 86 launches of config 3: 0.83 s
    assert bench.preload_steps(4096 * 96000, 2) == 67                                  # configs 2 / 2b: 69 launches, >= 0.6 s at 8.8 ms
    assert bench.preload_steps(65536 * 4800, 100) == 0
    assert bench.preload_steps(2048 * 4800, 1) == 400                                  # capped


def test_dump_outputs_cap_holds_for_any_launch_length(tmp_path):
    """A launch whose words for one stream alone exceed the cap: the dump keeps the launch's last packets that fit, and says which."""
    S, P, R, B, nb, n_out = 4, 4, 64, 96, 9000, 9
    frames = nb * B
    pairs = torch.arange(S * P * frames * 2, dtype=torch.int32).reshape(S, P, frames, 2)
    sub = torch.arange(S * frames, dtype=torch.int32).reshape(S, frames)
    peaks = torch.arange(S * nb * (2 + n_out), dtype=torch.int32).reshape(S, nb, 2 + n_out).to(torch.int16)
    bench.dump_chain_outputs(str(tmp_path), torch, pairs, sub, peaks, False, R, S, P, frames, nb, n_out)
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) < 64e6
    pk = np.load(tmp_path / "packets.npy").astype(np.int64)
    m = len(pk)
    assert 0 < m < nb and np.array_equal(pk, np.arange(nb - m, nb))
    idx = np.load(tmp_path / "streams.npy").astype(np.int64)
    assert len(idx) == 1
    assert np.array_equal(np.load(tmp_path / "pairs.npy"), pairs.numpy()[idx][:, :, (nb - m) * B:])
    assert np.array_equal(np.load(tmp_path / "sub.npy"), sub.numpy()[idx][:, (nb - m) * B:])
    assert np.array_equal(np.load(tmp_path / "peaks.npy"), peaks.numpy()[idx][:, nb - m:])


def test_config_runs_of_a_full_line_never_dump():
    """--full --dump-outputs: the short config 2 / 2b / 5 runs after config 3 must not overwrite the headline's dump."""
    import argparse
    args = argparse.Namespace(config="3", steps=50, warmup=10, dump_outputs="/some/dir", contract="canonical", out_layout="tiled", input="noise",
                              no_variants=False, no_realtime=False, no_cpu_baseline=False, full=True)
    for name in ("2", "2b", "5"):
        a2 = bench.config_args(args, name, 5, 2)
        assert a2.dump_outputs is None and a2.config == name and (a2.steps, a2.warmup) == (5, 2)
        assert (a2.contract, a2.out_layout, a2.input) == ("fma", "stream", "mix")
    assert args.dump_outputs == "/some/dir" and args.config == "3"
