"""The emitter wave's whole-line path (dspi_chain_pk.inc pair_lines_*: the master SIMD's third wave reads the rows of pairs 2 and 3 with
16-byte loads in the lane mapping of its stores and writes whole 128-byte pair-buffer lines) and its fallback (pair_emit_load / _finish).
Every case runs twice, with and without DSPI_NO_EMIT_LINES=1, and both runs are compared with the CPU oracle the way
tests/test_gpu_parity.py::compare does it — every pair word, sub word, peak, status byte and clip flag — never with each other.  The
oracle's results of a case are computed once and shared by its runs, and so are those of its reference leg (tests/refleg.py: the reference's
leaf sources compiled unmodified, held to the GPU's words directly; float only here, so every stream is expected to be held).  Needs an MI355X."""
import numpy as np
import pytest

from conftest import has_gpu
import refleg
from dspi_amd import wire as W, workloads as WL
from dspi_amd.host import Dspi
from test_gpu_pause import new_sched

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS = (1, W.F32_FMA)          # the float flavour under both contracts
ROW = 128                         # streams per row of the packed kernel
LINE = 4096                       # positions of a delay line
flavor_ids = ("canonical", "fma")
switch = pytest.mark.parametrize("off", (False, True), ids=("lines", "fallback"))
both_flavors = pytest.mark.parametrize("flavor", FLAVORS, ids=flavor_ids)


def _env(monkeypatch, off):
    monkeypatch.setenv("DSPI_F32_LAYOUT", "packed")      # small contexts reach the packed kernel
    if off: monkeypatch.setenv("DSPI_NO_EMIT_LINES", "1")
    else: monkeypatch.delenv("DSPI_NO_EMIT_LINES", raising=False)


def bench_mix(S, frames, fs, quiet_from):
    """the bench's mix classes (workloads.synth_pcm16); the class that falls silent does so inside the test's few packets (its filters' tails go on)"""
    pcm = WL.synth_pcm16(S, frames, fs)
    pcm[18::20, quiet_from:] = 0
    return pcm


def samples_ms(n, fs):
    """a delay of n samples, in the preset's unit (a fifth of a sample above n: the same count whether the conversion rounds or truncates)"""
    return (n + 0.2) * 1000.0 / fs


_REF = {}
_LEG = {}      # the same keys: {stream: the oracle's reference leg, its words of every call kept}


def reference(key, flavor, fs, vol, blob, pcm, per, calls, B, setup, between):
    """{stream: ([(pairs, sub, peaks, clip) per call], status after the last call)} of the oracle, computed once per case; the reference
    build runs beside it (refleg.Leg) and keeps its own words of every call for hold_to_reference()"""
    key = key + (bool(getattr(flavor, "fma", False)),)      # (W.F32_FMA compares equal to the int 1)
    if key not in _REF:
        ref, legs = {}, {}
        for s in range(pcm.shape[0]):
            o = refleg.Leg(flavor, f"stream {s}")
            assert o.set_rate(fs) == 0
            o.set_volume(vol)
            assert o.load_bulk(blob) == 0
            if setup: setup(o)
            parts, kept = [], []
            for c in range(calls):
                if between and c in between: between[c](o)
                parts.append(o.process(np.ascontiguousarray(pcm[s, c * per * B:(c + 1) * per * B]), per, B))
                kept.append(o.last)
            ref[s] = (parts, o.status())
            legs[s] = (o, kept)
            o.close()
        _REF[key], _LEG[key] = ref, legs
    return _REF[key]


def left_justified(words, i2s_mask):
    """pair words [P][frames][2] as DSPI_OUT_I2S_SLOTS hands them back: the pairs of i2s_mask shifted up by eight bits"""
    words = words.copy()
    for p in range(words.shape[0]):
        if i2s_mask >> p & 1: words[p] = (words[p].astype(np.uint32) << np.uint32(8)).astype(np.int32)
    return words


def hold_to_reference(key, flavor, s, c, pairs=None, sub=None, peaks=None, clip=None, status=None, i2s_mask=0):
    """stream s, call c of a case: the GPU's words against the reference build's (status: after the last call)"""
    leg, kept = _LEG[key + (bool(getattr(flavor, "fma", False)),)][s]
    if not leg.on: return
    (rp, rs, rk, rclip), rstatus, held = kept[c]
    assert held, f"stream {s}, call {c}: a float->int cast overflowed on the x86 reference build — not expected of the float chain"
    if i2s_mask: rp = left_justified(rp, i2s_mask)
    leg.hold(pairs, sub, peaks, status, clip, what=f"call {c}", last=((rp, rs, rk, rclip), rstatus, held))


def run_case(monkeypatch, off, key, flavor, fs, B, per, calls, S, blob, pcm=None, vol=-20 * 256, setup=None, between=None, i2s_mask=0,
             want_pairs=True, want_peaks=True):
    """One context, `calls` launches of `per` packets; every stream against the oracle.  setup(x) / between[c](x) are applied to the context
    and to every oracle alike.  i2s_mask: pairs whose words must come back left-justified (DSPI_OUT_I2S_SLOTS)."""
    _env(monkeypatch, off)
    if pcm is None: pcm = bench_mix(S, B * per * calls, fs, 2 * B)
    d = Dspi(flavor, S, device=0)
    assert d.set_rate(fs) == 0
    d.set_volume(vol)
    assert d.load_bulk(blob) == 0
    if setup: setup(d)
    outs, clips = [], []
    for c in range(calls):
        if between and c in between: between[c](d)
        outs.append(d.process_host(np.ascontiguousarray(pcm[:, c * per * B:(c + 1) * per * B]), per, B, clip=True, i2s_slots=bool(i2s_mask),
                                   want_pairs=want_pairs, want_peaks=want_peaks))
        clips.append(d.last_clip.copy())
    plan = d.launch_plan()
    assert plan["emit_lines_off"] == int(off) and plan["packed_shared"] == (S + ROW - 1) // ROW and plan["latency_layout"] == 0, plan
    ref = reference(key, flavor, fs, vol, blob, pcm, per, calls, B, setup, between)
    for s in range(S):
        parts, status = ref[s]
        for c, (rp, rs, rk, rclip) in enumerate(parts):
            pairs, sub, peaks = outs[c]
            if want_pairs:
                want = left_justified(rp, i2s_mask) if i2s_mask else rp
                assert np.array_equal(want, pairs[s]), f"pairs differ, stream {s}, call {c}: {np.argwhere(want != pairs[s])[:3].tolist()}"
            assert np.array_equal(rs, sub[s]), f"sub differs, stream {s}, call {c}"
            if want_peaks: assert np.array_equal(rk, peaks[s]), f"peaks differ, stream {s}, call {c}: {np.argwhere(rk != peaks[s])[:3].tolist()}"
            assert int(clips[c][s]) == rclip, f"clip flags differ, stream {s}, call {c}"
            hold_to_reference(key, flavor, s, c, pairs[s] if want_pairs else None, sub[s], peaks[s] if want_peaks else None, int(clips[c][s]),
                              d.status(s) if c == calls - 1 else None, i2s_mask=i2s_mask)
        assert status == d.status(s), f"status differs, stream {s}"
    d.close()
    return ref


def hot_blob():
    """config 3's preset with the outputs of pairs 2 and 3 early and loud: the full-scale square drives them past 1.001 (their clip bits, their
    peaks at 32767) within the test's packets"""
    b = WL.full_chain_blob(1)
    for o in (4, 5, 6, 7):
        b["outputs"][o]["gain_db"] = 14.0
        b["outputs"][o]["delay_ms"] = (0.0, 0.5, 1.0, 2.0)[o - 4]
    return b


# ---- 1. one full row --------------------------------------------------------------------------------------------------------------------
@both_flavors
@switch
@pytest.mark.parametrize("fs,B", [(96000, 96), (48000, 48)], ids=("96k", "48k"))
@pytest.mark.parametrize("preset", ("config3", "hot"))
def test_one_full_row(flavor, off, fs, B, preset, monkeypatch):
    """128 streams, 8 packets per call, three calls in a row: state, write positions and the launch's head are carried.  Config 3's preset,
    and the same with pairs 2 and 3 loud enough to clip (the preset as it is clips on the master and on output 2 only)."""
    blob = WL.full_chain_blob(1) if preset == "config3" else hot_blob()
    vol = -20 * 256 if preset == "config3" else 0
    ref = run_case(monkeypatch, off, ("row", flavor, fs, preset), flavor, fs, B, 8, 3, ROW, blob, vol=vol)
    clip = [ref[s][0][-1][3] for s in range(ROW)]
    peaks = np.stack([ref[s][0][-1][2] for s in range(ROW)])
    if fs == 96000: assert any(c & 0x3 for c in clip), "the square clips the master"      # (at 48 kHz the 24-frame square is an octave lower and stays below 1.001 there)
    if preset == "hot":
        assert any(c & (0xf << 6) for c in clip) and int(peaks[:, :, 6:10].max()) == 32767, "outputs 4-7 are meant to clip here"


# ---- 2. rows that must fall back beside rows that must not ------------------------------------------------------------------------------------
@both_flavors
@switch
def test_partial_row_beside_full_rows(flavor, off, monkeypatch):
    """258 streams: two full rows and a row of two, one launch"""
    run_case(monkeypatch, off, ("258", flavor), flavor, 96000, 96, 4, 2, 2 * ROW + 2, WL.full_chain_blob(1))


@both_flavors
@switch
def test_row_with_drifted_write_positions(flavor, off, monkeypatch):
    """Two full rows; some streams of the second are paused for two packets and resumed as they are, so its streams stand at two line write
    positions (tests/test_gpu_pause.py builds it the same way) while the first row stays uniform."""
    _env(monkeypatch, off)
    fs, B, S = 96000, 96, 2 * ROW
    x = new_sched(flavor, S, fs, B, 16, 12)
    x.run(3)
    x.pause(ROW + 9, 20)
    x.run(2)                                   # (the second row runs with a lane mask here)
    x.resume(ROW + 9, 20, as_is=True)
    w, _ = x.d.stream_positions(0, S)
    assert len(set(w[:ROW].tolist())) == 1 and len(set(w[ROW:].tolist())) == 2, "one uniform row, one with two write positions"
    x.run(4); x.run(3)
    plan = x.d.launch_plan()
    assert plan["packed_shared"] == 2 and plan["emit_lines_off"] == int(off), plan
    x.verify()
    x.d.close()


# ---- 3. positions that are not chunk-aligned, a wrap inside a chunk ------------------------------------------------------------------------------
@both_flavors
@switch
def test_unaligned_delays_and_wraps(flavor, off, monkeypatch):
    """Delays of 37, 1 000 and 4 095 samples on pairs 2 and 3: read positions that are no multiple of the chunk, so chunks wrap inside the
    4 096-position line (the mask per row); 90 packets of 96 frames: the lines wrap twice."""
    fs, B = 96000, 96
    blob = WL.full_chain_blob(1)
    for o, n in zip((4, 5, 6, 7), (37, 1000, 4095, 37)): blob["outputs"][o]["delay_ms"] = samples_ms(n, fs)
    assert 3 * 30 * B >= 2 * LINE
    ref = run_case(monkeypatch, off, ("unaligned", flavor), flavor, fs, B, 30, 3, ROW, blob)
    assert all(np.abs(ref[0][0][-1][0][p]).max() > 0 for p in (2, 3)), "the delayed audio has arrived"


# ---- 4. the edges of the emitter's sources ---------------------------------------------------------------------------------------------------
_EDGES = {      # samples of delay on outputs 4..7: 0 = the mini line; the line's length and beyond it; within three chunks of it (mini line) and just outside
    "a": (0, LINE, LINE - 16, LINE - 48),
    "b": (LINE - 47, LINE + 15, LINE - 32, 1),
    "c": (LINE - 1, LINE - 49, 2 * LINE, 0),
}


@both_flavors
@switch
@pytest.mark.parametrize("fs,B", [(96000, 96), (48000, 48)], ids=("96k", "48k"))
@pytest.mark.parametrize("edges", sorted(_EDGES))
def test_delay_edges(flavor, off, fs, B, edges, monkeypatch):
    """delay 0, a delay equal to the line's length (and past it), delays within three chunks of it — where the emitter reads the three-chunk
    mini line instead of the delay line — and the first delays outside that band; in samples, so at every rate in use"""
    blob = WL.full_chain_blob(1)
    for o, n in zip((4, 5, 6, 7), _EDGES[edges]): blob["outputs"][o]["delay_ms"] = samples_ms(n, fs)
    per = -(-(LINE + 4 * B) // (3 * B))        # three calls that end after the longest delay has come through
    run_case(monkeypatch, off, ("edges", flavor, fs, edges), flavor, fs, B, per, 3, ROW, blob)


@both_flavors
@switch
def test_disabled_outputs_and_zero_fill(flavor, off, monkeypatch):
    """after the first call output 5 is switched off (pair 2: one output left) and outputs 6 and 7 (pair 3: zero-filled at once, whatever its
    lines still hold, usb_audio.c:930-933; the meters still see the tail)"""
    R = W.REQ
    def switch_off(x):
        for o in (5, 6, 7): x.vendor_set(R["SET_OUTPUT_ENABLE"], o, b"\x00")
    ref = run_case(monkeypatch, off, ("disabled", flavor), flavor, 96000, 96, 8, 3, ROW, hot_blob(), between={1: switch_off})
    assert not ref[0][0][-1][0][3].any() and ref[0][0][0][0][3].any() and ref[0][0][-1][0][2].any()


@both_flavors
@switch
def test_i2s_pair(flavor, off, monkeypatch):
    """slot 2 is an I2S slot: DSPI_OUT_I2S_SLOTS leaves the words of pair 2 left-justified (the type switch mutes the pipeline for the first
    packets: 48 packets in all)"""
    def to_i2s(x):
        if isinstance(x, Dspi): x.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 2 | (1 << 8), 1, -1)
        else: x.vendor_get(W.REQ["SET_OUTPUT_TYPE"], 2 | (1 << 8), 1)
    ref = run_case(monkeypatch, off, ("i2s", flavor), flavor, 96000, 96, 16, 3, ROW, hot_blob(), setup=to_i2s, i2s_mask=0b0100)
    assert ref[0][0][-1][0][2].any(), "pair 2 carries audio after the mute"


# ---- 5. buffers ----------------------------------------------------------------------------------------------------------------------------
@both_flavors
@switch
@pytest.mark.parametrize("without", ("peaks", "pairs"))
def test_null_buffers(flavor, off, without, monkeypatch):
    """no peaks buffer; no pair buffer (meters only: peaks, clip flags and status still equal the oracle's)"""
    run_case(monkeypatch, off, ("null", flavor), flavor, 96000, 96, 8, 2, ROW, hot_blob(), vol=0, want_pairs=without != "pairs", want_peaks=without != "peaks")


@both_flavors
@switch
@pytest.mark.parametrize("offset_words", (32, 2), ids=("line-aligned", "8-byte-aligned"))
def test_device_pair_buffer_alignment_and_guards(flavor, off, offset_words, monkeypatch):
    """DSPI_MEM_DEVICE: a pair buffer that starts 128 bytes into an allocation (whole lines) and one that starts 8 bytes into it (no line of
    it is aligned: the fallback, still exact); the words before and behind the buffer keep their sentinel"""
    import torch
    _env(monkeypatch, off)
    fs, B, per, calls, S, vol = 96000, 96, 8, 2, ROW, 0
    blob = hot_blob()
    pcm = bench_mix(S, B * per * calls, fs, 2 * B)
    d = Dspi(flavor, S, device=0)
    assert d.set_rate(fs) == 0
    d.set_volume(vol)
    assert d.load_bulk(blob) == 0
    P, C, F = d.P, d.C, per * B
    n, back, sentinel = S * P * F * 2, 64, 0x5A5A5A5A
    ref = reference(("null", flavor), flavor, fs, vol, blob, pcm, per, calls, B, None, None)      # (test_null_buffers' case: the same preset and input)
    for c in range(calls):
        buf = torch.full((offset_words + n + back,), sentinel, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 128 == 0
        sub = torch.zeros((S, F), dtype=torch.int32, device="cuda")
        peaks = torch.zeros((S, per, C), dtype=torch.int16, device="cuda")
        clip = torch.zeros((S,), dtype=torch.int16, device="cuda")
        x = torch.from_numpy(np.ascontiguousarray(pcm[:, c * F:(c + 1) * F])).cuda()
        d.process_device(x.data_ptr(), per, B, 16, pairs_ptr=buf.data_ptr() + 4 * offset_words, sub_ptr=sub.data_ptr(), peaks_ptr=peaks.data_ptr(), clip_ptr=clip.data_ptr())
        d.sync()
        host = buf.cpu().numpy()
        assert (host[:offset_words] == sentinel).all() and (host[offset_words + n:] == sentinel).all(), "guard words were written"
        pairs = host[offset_words:offset_words + n].reshape(S, P, F, 2)
        sub, peaks, clip = sub.cpu().numpy(), peaks.cpu().numpy().view(np.uint16), clip.cpu().numpy().view(np.uint16)
        for s in range(S):
            rp, rs, rk, rclip = ref[s][0][c]
            assert np.array_equal(rp, pairs[s]), f"pairs differ, stream {s}, call {c}: {np.argwhere(rp != pairs[s])[:3].tolist()}"
            assert np.array_equal(rs, sub[s]) and np.array_equal(rk, peaks[s]) and int(clip[s]) == rclip, f"stream {s}, call {c}"
            hold_to_reference(("null", flavor), flavor, s, c, pairs[s], sub[s], peaks[s], int(clip[s]), d.status(s) if c == calls - 1 else None)
    for s in range(S): assert ref[s][1] == d.status(s), f"status differs, stream {s}"
    d.close()


# ---- 6. packets of the TAIL instantiation ----------------------------------------------------------------------------------------------------
@both_flavors
@switch
@pytest.mark.parametrize("B", (44, 45))
def test_ragged_packets_keep_the_old_path(flavor, off, B, monkeypatch):
    """44 / 45 frames at 44.1 kHz: the last chunk of a packet is ragged, the kernel's TAIL instantiation emits by the row mapping"""
    run_case(monkeypatch, off, ("tail", flavor, B), flavor, 44100, B, 8, 3, ROW, WL.full_chain_blob(1))
