"""S/PDIF input on the GPU (include/dspi.h: dspi_spdif_decode, dspi_process_sources).

What each part is held to, always for equality:
  the subframes   tests/spdifrx_model.encode: the reference's own encoder where oracle/_ref exists, else its restatement; corruptions are
                  applied to those words here
  the receiver    tests/spdifrx_model.receive, the sequential model: pair words and every byte of every record
  the sample path every stream's own Oracle(detmath=True) at its native format; an S/PDIF stream's oracle is fed the MODEL's output as 24-bit
                  PCM.  Pair words, sub words, peaks, clip flags, status bytes.
Shapes: float S = 150 (a full row of 128 and a ragged one with an odd last stream), Q28 S = 100 (row 64); 5 packets of 48 frames (F = 240
crosses the 192-frame block and three 64-lane chunks) and 3 packets of 45 (F = 135 is odd, 6 F = 2 mod 4); the direct host path takes one
packet per call (it is the path of small calls).  References are computed once per shape and shared."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import spdifrx_model as M
from conftest import has_gpu
from orclib import spdif_encode
from dspi_amd import host, wire as W, workloads as WL
from test_gpu_snapshot import context, oracle, packets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS = {"f32": 1, "fma": W.F32_FMA, "q28": 0}
FILL = 0xA5          # a paused stream's input bytes and the padding in front of S/PDIF runs: never read
POISON = 0xEE        # the records the call must not touch (as a record: sync > 192)
PAUSED = 5           # an S/PDIF stream (5 % 3 == 2)
RX = host.SPDIF_RX


def streams_of(flavor): return 150 if int(flavor) else 100
def sources_of(S): return np.array([(16, 24, 1)[s % 3] for s in range(S)], dtype=np.uint8)
def fs_of(Bk): return 44100 if Bk == 45 else 48000
def sign24(v): return ((v & 0xffffff) ^ 0x800000) - 0x800000


def pairs_of_pcm24(row):
    """packed 24-bit bytes [frames * 6] -> the sample values int32 [frames][2]"""
    b = np.ascontiguousarray(row).reshape(-1, 3).astype(np.int32)
    return sign24(b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16).astype(np.int32).reshape(-1, 2)


def trouble(w, kind, F):
    """a stream's line with one kind of trouble in each call (frames f and F + f)"""
    for base in (0, F):
        if kind == 1:
            for f in range(3): M.set_v(w, base + f, 0)                                   # V on the first frames of a call
            for f in range(min(62, F - 8), min(67, F - 3)): M.set_v(w, base + f, f & 1)      # (across the first chunk boundary where the call is that long)
        elif kind == 2: M.clear_clock_cell(w, base + 10, 1, 17); M.set_preamble(w, base + 30, 0, M.Z)
        elif kind == 3: M.flip_data_cell(w, base + 20, 0, 11); M.set_v(w, base + 21, 1, keep_parity=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(fl, n, Bk):
    """two calls of n packets of Bk frames: per stream its input at its native format, the model's pairs and records (S/PDIF), the oracle's
    outputs and status per call"""
    flavor = FLAVORS[fl]
    S, fs, F = streams_of(flavor), fs_of(Bk), n * Bk
    blob = WL.full_chain_blob(int(flavor))
    src = sources_of(S)
    p16 = WL.synth_pcm16(S, 2 * F, fs); p24 = WL.pcm16_to_pcm24_bytes(p16)
    lines, recs, calls, status0 = {}, {}, [[None] * S, [None] * S], [None] * S
    for s in range(S):
        o = oracle(flavor, fs, blob)
        status0[s] = o.status()
        if s == PAUSED: continue
        if src[s] == 1:
            w = trouble(M.encode(pairs_of_pcm24(p24[s]), (7 * s) % 192, (44100, 48000, 96000)[s // 3 % 3]), s // 3 % 4, F)
            rx = M.new_rx()
            fed = [M.pack24(M.receive(rx, w[:F])), None]; recs[s] = [M.to_record(rx)]
            fed[1] = M.pack24(M.receive(rx, w[F:])); recs[s].append(M.to_record(rx))
            lines[s] = w
        for k in range(2):
            if src[s] == 1: x, depth = fed[k], 24
            elif src[s] == 24: x, depth = packets(p24[s], 24, Bk, k * n, (k + 1) * n), 24
            else: x, depth = packets(p16[s], 16, Bk, k * n, (k + 1) * n), 16
            calls[k][s] = o.process(x, n, Bk, depth) + (o.status(),)
    assert any(r[1]["held"] for r in recs.values()) and any(r[1]["coding_errors"] for r in recs.values()) and any(r[1]["parity_err_count"] for r in recs.values())
    return dict(flavor=flavor, S=S, fs=fs, F=F, blob=blob, src=src, p16=p16, p24=p24, lines=lines, recs=recs, calls=calls, status0=status0)


def input_buffer(ref, d, k, n, Bk):
    S, F, src = ref["S"], ref["F"], ref["src"]
    total, off = d.sources_bytes(src, n, Bk)
    buf = np.full(total, FILL, dtype=np.uint8)
    for s in range(S):
        if s == PAUSED: continue
        if src[s] == 1: x = ref["lines"][s][k * F:(k + 1) * F]
        elif src[s] == 24: x = packets(ref["p24"][s], 24, Bk, k * n, (k + 1) * n)
        else: x = packets(ref["p16"][s], 16, Bk, k * n, (k + 1) * n)
        x = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        assert x.nbytes == F * {16: 4, 24: 6, 1: 16}[int(src[s])] and (src[s] != 1 or off[s] % 16 == 0)
        buf[int(off[s]):int(off[s]) + x.nbytes] = x
    return buf


def run_case(fl, n, Bk, mem, monkeypatch=None, wire=False, tiled=False):
    ref = reference(fl, n, Bk)
    flavor, S, fs, F, src = ref["flavor"], ref["S"], ref["fs"], ref["F"], ref["src"]
    if mem == "staged": monkeypatch.setenv("DSPI_NO_DIRECT", "1")      # (read once at dspi_create)
    d = context(flavor, S, fs, ref["blob"])
    if mem == "staged": monkeypatch.delenv("DSPI_NO_DIRECT", raising=False)
    d.pause_streams(PAUSED, 1)
    rx = np.frombuffer(bytes([POISON]) * (40 * S), dtype=RX).copy()
    for s in ref["lines"]: rx[s] = np.zeros((), dtype=RX)
    pos = 0
    for k in range(2):
        buf = input_buffer(ref, d, k, n, Bk)
        before = d.direct_stats()["calls"]
        if mem == "device":
            import torch
            dev = torch.device("cuda", 0)
            t_in = torch.from_numpy(buf).to(dev); t_rx = torch.from_numpy(rx.view(np.uint8).copy()).to(dev)
            t_pairs = torch.zeros((S, d.P, F, 4 if wire else 2), dtype=torch.int32, device=dev)
            t_sub = torch.zeros((S, F), dtype=torch.int32, device=dev); t_peaks = torch.zeros((S, n, d.C), dtype=torch.int16, device=dev)
            t_clip = torch.zeros(S, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            d.process_sources_device(t_in.data_ptr(), src, n, Bk, t_rx.data_ptr(), t_pairs.data_ptr(), t_sub.data_ptr(), t_peaks.data_ptr(), wire=wire, clip_ptr=t_clip.data_ptr())
            d.sync()
            pairs, sub, peaks, clip = t_pairs.cpu().numpy(), t_sub.cpu().numpy(), t_peaks.cpu().numpy().view(np.uint16), t_clip.cpu().numpy().view(np.uint16)
            rx = t_rx.cpu().numpy().view(RX).reshape(S).copy()
        else:
            pairs, sub, peaks = d.process_sources_host(buf, src, n, Bk, rx, wire=wire, tiled=tiled, clip=True)
            clip = d.last_clip.copy()
            assert (d.direct_stats()["calls"] > before) == (mem == "direct"), "the call did not take the memory path this case is about"
            if tiled: pairs, sub = d.untile_wire(pairs, np.zeros((S, d.P), dtype=bool)), d.untile(None, sub)[1]
        pairs = pairs.view(np.uint32) if wire else pairs
        for s in range(S):
            what = f"{fl} {n}x{Bk} {mem} call {k} stream {s} (source {src[s]})"
            if s == PAUSED:
                assert not pairs[s].any() and not sub[s].any() and not peaks[s].any() and d.status(s) == ref["status0"][s], what + ": paused"
                continue
            rp, rs, rk, rclip, status = ref["calls"][k][s]
            if wire: rp = np.stack([spdif_encode(rp[p], pos, fs)[0] for p in range(d.P)])
            assert np.array_equal(rp, pairs[s]), what + ": pair words"
            assert np.array_equal(rs, sub[s]) and np.array_equal(rk, peaks[s]) and int(clip[s]) == rclip, what + ": sub words, peaks or clip flags"
            assert d.status(s) == status, what + ": status bytes"
        for s in range(S):
            if s in ref["lines"]: assert rx[s].tobytes() == ref["recs"][s][k].tobytes(), (fl, mem, k, s, rx[s], ref["recs"][s][k])
            else: assert rx[s].tobytes() == bytes([POISON]) * 40, f"stream {s}'s record was written"
        pos = (pos + F) % 192
    d.close()


# ---- 1. decode round trip --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_lines():
    rng = np.random.default_rng(1)
    pairs = np.stack([M.random_pairs(rng, 250) for _ in range(130)])
    pos = [(37 * l) % 192 for l in range(130)]; pos[0], pos[1], pos[2] = 0, 191, 1
    fs = [(44100, 48000, 96000)[l % 3] for l in range(130)]
    words = np.stack([M.encode(pairs[l], pos[l], fs[l]) for l in range(130)])
    recs = []
    for l in range(130):
        rx = M.new_rx(); got = M.receive(rx, words[l]); recs.append(M.to_record(rx))
        assert np.array_equal(got, pairs[l]) and rx["sample_rate"] == fs[l], "every line passes a Z and position 31 behind it"
    return pairs, words, np.array(recs, dtype=RX)


def decode(d, words, rx, mem):
    """dspi_spdif_decode on host or device buffers -> (pairs, records)"""
    if mem == "host":
        rx = rx.copy()
        return d.spdif_decode_host(words, rx), rx
    import torch
    dev = torch.device("cuda", 0)
    t_w = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev); t_rx = torch.from_numpy(rx.view(np.uint8).copy()).to(dev)
    t_p = torch.zeros(words.shape[:2] + (2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d.spdif_decode_device(t_w.data_ptr(), words.shape[0], words.shape[1], t_rx.data_ptr(), t_p.data_ptr())
    d.sync()
    return t_p.cpu().numpy(), t_rx.cpu().numpy().view(RX).reshape(-1).copy()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_decode_round_trip(mem):
    pairs, words, recs = clean_lines()
    d = host.Dspi(0, 3, device=0)      # (stateless per context: the context's size is not the call's)
    got, rx = decode(d, words, np.zeros(130, dtype=RX), mem)
    assert np.array_equal(got, pairs), np.argwhere(got != pairs)[:3]
    assert rx.tobytes() == recs.tobytes(), [l for l in range(130) if rx[l] != recs[l]][:5]
    assert (rx["state"] == 2).all() and not rx["held"].any()
    d.close()


@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_decode_reads_the_librarys_own_encoder(fl):
    """dspi_spdif_encode_v's output, a whole stream-major buffer of n_streams * pairs lines, decodes to the words that went in"""
    S, F, fs = 23, 250, 96000
    d = host.Dspi(FLAVORS[fl], S, device=0)
    assert d.set_rate(fs) == 0
    pairs = np.stack([M.random_pairs(np.random.default_rng(s), d.P * F).reshape(d.P, F, 2) for s in range(S)])
    pos = [(11 * s) % 192 for s in range(S)]
    sub = d.spdif_encode_v_host(pairs, pos)
    rx = np.zeros(S * d.P, dtype=RX)
    got = d.spdif_decode_host(sub.reshape(S * d.P, F, 4), rx)
    assert np.array_equal(got.reshape(pairs.shape), pairs)
    rx = rx.reshape(S, d.P)
    assert (rx["state"] == 2).all() and (rx["sample_rate"] == fs).all() and not rx["parity_err_count"].any() and not rx["held"].any() and not rx["coding_errors"].any()
    for s in range(S): assert (rx["sync"][s] == 1 + (pos[s] + F) % 192).all() and (rx["c_bits"][s] == [0x04, 0, 0, 0x0A, 0x0B]).all()
    d.close()


# ---- 2. corruptions against the model ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corrupted_lines():
    rng = np.random.default_rng(2)
    F = 250
    def line(pos=0, fs=48000): return M.encode(M.random_pairs(rng, F), pos, fs)
    L = []
    for k in (70, 130):
        w = line(); M.set_v(w, 0, 0); M.set_v(w, k, 0); M.set_v(w, k, 1); L.append(w)                      # V on the first frame of a call
        w = line(5); [M.set_v(w, f, 0) for f in range(62, 67)]; L.append(w)                                  # V across the chunk boundary, left only
        w = line(9); [M.set_v(w, f, 1) for f in range(62, 67)]; L.append(w)                                  # ... right only
        w = line(); M.flip_data_cell(w, 40, 0, 4); M.flip_data_cell(w, k + 3, 1, 27); L.append(w)             # parity is counted, the sample passes
        w = line(); M.clear_clock_cell(w, 50, 0, 20); M.clear_clock_cell(w, k + 1, 1, 4); L.append(w)         # a cleared clock cell
        L.append(line(100))                                                                                  # starts mid-block: no Z for 92 frames
        w = line(); M.flip_data_cell(w, 10, 0, 8); M.set_preamble(w, 77, 0, M.Z); M.flip_data_cell(w, 90, 1, 8); L.append(w)      # a misplaced Z: re-lock, count reset
        w = line(); M.set_preamble(w, 192, 0, M.X); L.append(w)                                              # X at position 0
        w = line(20); M.set_preamble(w, 172, 0, M.X); M.set_preamble(w, 200, 0, M.Z); L.append(w)              # ... and a Z that is none of the block's, later
        L.append(np.zeros((F, 4), dtype=np.uint32))                                                          # all-zero frames
        w = line(); w[k - 2:k + 2] = 0; L.append(w)                                                          # ... a few, across the cut
    return np.stack(L)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("split", [70, 130])
def test_corruptions_in_two_calls(split, mem):
    words = corrupted_lines()
    n = len(words)
    want_pairs, want_mid, want_end = [], [], []
    for l in range(n):
        rx = M.new_rx()
        a = M.receive(rx, words[l, :split]); want_mid.append(M.to_record(rx))
        b = M.receive(rx, words[l, split:]); want_end.append(M.to_record(rx))
        want_pairs.append(np.concatenate([a, b]))
    d = host.Dspi(1, 2, device=0)
    got_a, rx = decode(d, np.ascontiguousarray(words[:, :split]), np.zeros(n, dtype=RX), mem)
    assert rx.tobytes() == np.array(want_mid, dtype=RX).tobytes(), [(l, rx[l], want_mid[l]) for l in range(n) if rx[l] != want_mid[l]][:3]
    got_b, rx = decode(d, np.ascontiguousarray(words[:, split:]), rx, mem)
    got = np.concatenate([got_a, got_b], axis=1)
    for l in range(n): assert np.array_equal(got[l], want_pairs[l]), (l, np.argwhere(got[l] != want_pairs[l])[:3])
    assert rx.tobytes() == np.array(want_end, dtype=RX).tobytes(), [(l, rx[l], want_end[l]) for l in range(n) if rx[l] != want_end[l]][:3]
    # the scenarios do what they are there for
    end = np.array(want_end, dtype=RX)
    mid = np.array(want_mid, dtype=RX)
    assert end["parity_err_count"][3] == 2 and end["coding_errors"][4] == 2 and end["state"][9] == 0 and end["held"][9] == 500
    assert mid["parity_err_count"][6] == 1 and end["parity_err_count"][6] == 0, "one error behind the last lock at either cut; the block's own Z at 192 re-locks once more"
    assert end["state"][7] == 0 + 1 and end["sample_rate"][7] == 0, "X at position 0: the lock is lost and nothing gives it back"
    d.close()


# ---- 3. dspi_process_sources against the oracles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Bk", [(5, 48), (3, 45)], ids=["5x48", "3x45"])
@pytest.mark.parametrize("fl", ["f32", "fma", "q28"])
def test_sources_device(fl, n, Bk):
    run_case(fl, n, Bk, "device")


@pytest.mark.parametrize("Bk", [48, 45])
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_sources_direct_host(fl, Bk):
    run_case(fl, 1, Bk, "direct")


@pytest.mark.parametrize("n,Bk", [(5, 48), (3, 45)], ids=["5x48", "3x45"])
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_sources_staged_host(fl, n, Bk, monkeypatch):
    run_case(fl, n, Bk, "staged", monkeypatch)


@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_sources_wire_stream_major(fl):
    run_case(fl, 5, 48, "device", wire=True)


@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_sources_wire_tiled(fl, monkeypatch):
    run_case(fl, 3, 45, "staged", monkeypatch, wire=True, tiled=True)


# ---- 4. equivalences on twin contexts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_equivalences(fl):
    """no S/PDIF source: the call IS dspi_process_mixed, with DSPI_OUT_WIRE dspi_process_devices; uniform PCM sources: dspi_process — byte for byte"""
    flavor = FLAVORS[fl]
    S, fs, Bk, n = streams_of(flavor), 48000, 48, 2
    blob = WL.full_chain_blob(int(flavor))
    p16 = WL.synth_pcm16(S, n * Bk, fs); p24 = WL.pcm16_to_pcm24_bytes(p16)
    depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
    mixed = np.concatenate([np.ascontiguousarray(p24[s] if depths[s] == 24 else p16[s]).reshape(-1).view(np.uint8) for s in range(S)])
    def same(a, b, what):
        for x, y in zip(a, b): assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    assert a.sources_bytes(depths, n, Bk)[0] == mixed.nbytes
    same(a.process_sources_host(mixed, depths, n, Bk, None, clip=True) + (a.last_clip,), b.process_mixed_host(mixed, depths, n, Bk, clip=True) + (b.last_clip,), "dspi_process_mixed")
    assert a.launch_plan() == b.launch_plan() and a.direct_stats()["calls"] == b.direct_stats()["calls"]
    same(a.process_sources_host(mixed, depths, n, Bk, None, spdif=True), b.process_mixed_host(mixed, depths, n, Bk, spdif=True), "dspi_process_mixed with DSPI_OUT_SPDIF")
    same(a.process_sources_host(mixed, depths, n, Bk, None, wire=True, pdm=True), b.process_devices_host(mixed, depths, n, Bk, pdm=True), "dspi_process_devices")
    same(a.process_sources_host(mixed, depths, n, Bk, None, wire=True, tiled=True), b.process_devices_host(mixed, depths, n, Bk, tiled=True), "dspi_process_devices, tiled")
    same(a.process_sources_host(p24, np.full(S, 24), n, Bk, None), b.process_host(p24, n, Bk, 24), "dspi_process at 24 bit")
    same(a.process_sources_host(p16, np.full(S, 16), n, Bk, None), b.process_host(p16, n, Bk, 16), "dspi_process at 16 bit")
    for s in (0, 1, S - 1): assert a.status(s) == b.status(s)
    assert a.spdif_block_pos() == b.spdif_block_pos() == (3 * n * Bk) % 192
    a.close(); b.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_refusals_write_nothing(fl):
    flavor = FLAVORS[fl]
    S, F = 12, 48
    d = host.Dspi(flavor, S, device=0)
    assert d.vendor_set(W.REQ["SET_PREAMP_CH"], 0, struct.pack("<f", -640.0), stream=7) >= 0
    src = np.array([16, 24, 1] * (S // 3), dtype=np.uint8)
    bad = src.copy(); bad[7] = 16
    worse = bad.copy(); worse[9] = 8
    data = np.zeros(S * F * 16 + 64, dtype=np.uint8)
    rx = np.zeros(S, dtype=RX); rx["held"] = 77
    pairs = np.full((S, d.P, F, 4), 0x5A5A5A5A, dtype=np.uint32); sub = np.full((S, F), 0x5A5A5A5A, dtype=np.uint32); peaks = np.full((S, 1, d.C), 0x5A5A, dtype=np.uint16)
    clip = np.full(S, 0x5A5A, dtype=np.uint16)
    out = host._Out(pairs.ctypes.data, sub.ctypes.data, peaks.ctypes.data, clip.ctypes.data)
    po, pd, pr = C.byref(out), data.ctypes.data, rx.ctypes.data
    call = lambda dp, sp, nb, bl, o, r, flags=host.OUT_CLIP_FLAGS: d.L.dspi_process_sources(d.h, dp, sp.ctypes.data if sp is not None else None, nb, bl, o, None, r, flags)
    status = [d.status(s) for s in range(S)]
    snap = rx.tobytes()
    INV, UNS = host.E_INVAL, host.E_UNSUPPORTED
    order = [(call(None, src, 1, F, po, pr), INV), (call(pd, None, 1, F, po, pr), INV), (call(pd, src, 1, F, None, pr), INV),
             (call(pd, worse, 1, F, po, pr, host.OUT_WIRE | host.OUT_SPDIF), INV), (call(pd, worse, 0, F, po, None, 0x80), INV), (call(pd, bad, 0, F, po, None), INV),
             (call(pd, bad, 1, 193, po, None), INV), (call(pd, bad, 1, F, po, None, 0x80), INV), (call(pd, bad, 1, F, po, None, host.OUT_SPDIF | host.OUT_TILED), INV),
             (call(pd, bad, 1, F, po, None), INV)]
    rx["sync"][5] = 193
    order.append((call(pd, bad, 1, F, po, pr), INV))
    rx["sync"][5] = 0
    order += [(call(pd + 8, bad, 1, F, po, pr, host.MEM_DEVICE), INV), (call(pd, bad, 1, F, po, pr + 2, host.MEM_DEVICE), INV)]
    if int(flavor): order.append((call(pd, bad, 1, F, po, pr), UNS))
    assert [g for g, _ in order] == [w for _, w in order]
    # dspi_spdif_decode on a context with a device
    w = np.zeros((3, 8, 4), dtype=np.uint32); r3 = np.zeros(3, dtype=RX); p3 = np.full((3, 8, 2), 0x5A5A5A5A, dtype=np.uint32)
    r3["sync"][1] = 200
    assert d.L.dspi_spdif_decode(d.h, w.ctypes.data, 3, 8, r3.ctypes.data, p3.ctypes.data, 0) == INV
    assert d.L.dspi_spdif_decode(d.h, w.ctypes.data, 3, 8, r3.ctypes.data, p3.ctypes.data, host.OUT_TILED) == INV
    assert d.L.dspi_spdif_decode(d.h, w.ctypes.data + 4, 3, 8, r3.ctypes.data, p3.ctypes.data, host.MEM_DEVICE) == INV
    assert (p3 == 0x5A5A5A5A).all() and r3["sync"].tolist() == [0, 200, 0] and not r3["held"].any()
    assert (pairs == 0x5A5A5A5A).all() and (sub == 0x5A5A5A5A).all() and (peaks == 0x5A5A).all() and (clip == 0x5A5A).all(), "a refused call wrote output"
    assert rx.tobytes() == snap and [d.status(s) for s in range(S)] == status and d.spdif_block_pos() == 0
    # ... and the context still works
    d.process_sources_host(data[:d.sources_bytes(src, 1, F)[0]], src, 1, F, rx)
    assert (rx["coding_errors"][src == 1] == 2 * F).all() and (rx["state"][src == 1] == 0).all() and (rx["held"][src != 1] == 77).all()
    d.close()


# ---- 6. loopback ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_loopback(fl):
    """context A's DSPI_OUT_SPDIF output, pair 0 of every stream, is context B's all-S/PDIF input: B equals the oracle of B's preset fed the oracle
    of A's pair-0 words, and every record is LOCKED at A's rate"""
    flavor = FLAVORS[fl]
    S, fs, Bk, n = streams_of(flavor), 48000, 48, 5
    F = n * Bk
    blob = WL.full_chain_blob(int(flavor))
    p16 = WL.synth_pcm16(S, F, fs)
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob, vol=-10 * 256)
    sub_a = a.process_host(p16, n, Bk, 16, spdif=True, want_sub=False, want_peaks=False)[0]      # uint32 [S][P][F][4]
    src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
    total, off = b.sources_bytes(src, n, Bk)
    assert total == S * F * 16 and np.array_equal(off, np.arange(S + 1, dtype=np.uint64) * (F * 16))
    rx = np.zeros(S, dtype=RX)
    pairs, sub, peaks = b.process_sources_host(np.ascontiguousarray(sub_a[:, 0]), src, n, Bk, rx, clip=True)
    for s in range(S):
        oa, ob = oracle(flavor, fs, blob), oracle(flavor, fs, blob, vol=-10 * 256)
        word0 = oa.process(p16[s], n, Bk, 16)[0][0]
        rp, rs, rk, rclip = ob.process(M.pack24(word0), n, Bk, 24)
        assert np.array_equal(rp, pairs[s]) and np.array_equal(rs, sub[s]) and np.array_equal(rk, peaks[s]) and int(b.last_clip[s]) == rclip, f"stream {s}"
        assert b.status(s) == ob.status(), f"stream {s}: status bytes"
    assert (rx["state"] == 2).all() and (rx["sample_rate"] == fs).all() and (rx["sync"] == 1 + F % 192).all()
    assert not rx["held"].any() and not rx["parity_err_count"].any() and not rx["coding_errors"].any()
    a.close(); b.close()
