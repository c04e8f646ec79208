"""dspi_host --save-state / --load-state: one process running 2 n packets against two processes of n packets joined by a state file.
The second process's words are the second half of the single run's, and both are the oracle's.  Needs an MI355X."""
import os
import subprocess

import numpy as np
import pytest

from conftest import has_gpu
from orclib import Oracle
from dspi_amd import wire as W, workloads as WL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dspi_amd", "csrc", "dspi_host")


@pytest.mark.parametrize("flavor,streams", [(W.F32_FMA, 70), (1, 700), (0, 600)], ids=("fma-70", "f32-700-chunked", "q28-600-chunked"))
def test_two_processes_joined_by_a_state_file(tmp_path, flavor, streams):
    fs, B, n, vol_db = 48000, 48, 20, -20
    ref = Oracle(flavor); assert ref.load_bulk(WL.full_chain_blob(flavor)) == 0
    image = ref.save_slot(4)
    pcm = WL.synth_pcm16(1, 2 * n * B, fs, first_stream=3)[0]
    (tmp_path / "preset.bin").write_bytes(image)
    for name, part in (("whole", pcm), ("first", pcm[:n * B]), ("second", pcm[n * B:])):
        (tmp_path / f"{name}.raw").write_bytes(np.ascontiguousarray(part).tobytes())
    base = [HOST, "-f", ("f32fma" if getattr(flavor, "fma", False) else "f32") if int(flavor) else "q28", "-s", str(streams), "-r", str(fs), "-b", str(B), "-c", "1", "-v", str(vol_db)]
    preset = ["-P", str(tmp_path / "preset.bin")]

    def host(*args):
        r = subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    host(*preset, "-n", 2 * n, "-i", tmp_path / "whole.raw", "-o", tmp_path / "whole.out")
    out = host(*preset, "-n", n, "-i", tmp_path / "first.raw", "-o", tmp_path / "first.out", "--save-state", tmp_path / "state.bin")
    assert f"state of {streams} streams saved" in out
    # the second process sets nothing up itself: no preset, the default volume — the parameters come with the state
    out = host("-n", n, "-i", tmp_path / "second.raw", "-o", tmp_path / "second.out", "--load-state", tmp_path / "state.bin", "-v", "0")
    assert f"state of {streams} streams loaded" in out
    o = Oracle(flavor, detmath=True)
    assert o.set_rate(fs) == 0
    o.set_volume(vol_db * 256)
    assert o.load_slot(image) == 0
    pairs, _, _, _ = o.process(pcm, 2 * n, B)
    words = lambda name, frames: np.frombuffer((tmp_path / name).read_bytes(), dtype=np.int32).reshape(pairs.shape[0], frames, 2)      # stream 0
    whole, first, second = words("whole.out", 2 * n * B), words("first.out", n * B), words("second.out", n * B)
    assert np.array_equal(whole, pairs), "the single run differs from the oracle"
    assert np.array_equal(first, whole[:, :n * B]), "the first process differs from the single run's first half"
    assert np.array_equal(second, whole[:, n * B:]), "the second process differs from the single run's second half"
    assert np.array_equal(second, pairs[:, n * B:]), "the second process differs from the oracle"
    # a state file of another flavour is refused
    r = subprocess.run([HOST, "-f", "q28" if int(flavor) else "f32", "-s", str(streams), "-n", "1", "-c", "1", "--load-state", str(tmp_path / "state.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "flavour" in r.stderr, r.stdout + r.stderr
