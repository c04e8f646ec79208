"""Chained devices on the GPU (include/dspi.h: dspi_wire_decode, dspi_process_linked).

What each part is held to, always for equality:
  the link reader   tests/linkrx_model.py (the four index formulas from the header's prose) with tests/spdifrx_model.receive for an S/PDIF link
                    and `>> 8` for an I2S link: pair words and every byte of every record; an I2S link's record stays the poison it was
  the wire words    the library's own encoders (dspi_wire_encode / dspi_wire_encode_tiled, held to the oracle by tests/test_gpu_wire*.py) in test
                    1 and 2, orclib.spdif_encode / `<< 8` on the ORACLE's pair words in test 4
  the sample path   every consumer stream's own Oracle(detmath=True), fed the model's decode of its line as 24-bit PCM: pair words, sub words,
                    peaks, clip flags, status bytes
Shapes: float S = 150 (a full tile of 128 and a ragged one), Q28 S = 100 (tile 64); F = 135 (odd, 6 F = 2 mod 4) and 240 (crosses the 192-frame
block); types by (s + p) % 2, so neighbouring lanes of one wave differ.  References are computed once per shape and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import linkrx_model as LM
import spdifrx_model as M
from conftest import has_gpu
from orclib import spdif_encode
from dspi_amd import host, wire as W, workloads as WL
from test_gpu_snapshot import context, oracle, packets
from test_gpu_spdif_in import FLAVORS, POISON, RX, streams_of, trouble

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FILL = 0x5A5A5A5A
WARM = 12          # packets of 48 before anything is compared: the power-on mute is 512 samples and a type switch arms one of 256
R_ = W.REQ


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_process_linked"), "libdspi_mi355x has no dspi_process_linked"


def dev():
    import torch
    return torch, torch.device("cuda", 0)


def up(a):
    torch, d = dev()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(d)


def types_of(S, P): return np.array([[(s + p) % 2 == 1 for p in range(P)] for s in range(S)])
def set_types(x, types, **kw):
    for s, p in np.argwhere(types): assert x.vendor_get(R_["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1, int(s), **kw) == b"\x00"
def poison(n): return np.frombuffer(bytes([POISON]) * (40 * n), dtype=RX).copy()


def records_for(links):
    rx = poison(len(links))
    rx[links["kind"] == LM.SPDIF] = np.zeros((), dtype=RX)
    return rx


def tile_pairs(pairs, R):
    """int32 [S][P][F][2] -> the tiled pair words [tiles][2 P][F][R] (what dspi_process writes with DSPI_OUT_TILED)"""
    S, P, F, _ = pairs.shape
    nt = -(-S // R)
    pt = np.zeros((nt * R, P, 2, F), dtype=np.int32)
    pt[:S] = pairs.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(pt.reshape(nt, R, 2 * P, F).transpose(0, 2, 3, 1))


# ---- 1. round trip of the library's own encoders ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoded(fl, F):
    """random pair words through dspi_wire_encode and dspi_wire_encode_tiled, per-stream types and three rates; per line the model's decode of
    the stream-major words (the tiled buffer holds the same words re-laid: tests/test_gpu_wire_tiled.py)"""
    flavor = FLAVORS[fl]
    S = streams_of(flavor)
    d = host.Dspi(flavor, S, device=0)
    P, R = d.P, d.tile_streams()
    types = types_of(S, P)
    set_types(d, types)
    rates = np.full(S, 48000)
    assert d.set_rate(48000) == 0
    for s, r in ((1, 44100), (2, 96000), (S - 1, 44100), (S - 2, 96000)): rates[s] = r; assert d.set_rate(int(r), stream=int(s)) == 0
    rng = np.random.default_rng(F)
    pairs = rng.integers(-(1 << 23), 1 << 23, (S, P, F, 2), dtype=np.int64).astype(np.int32)
    pos = np.array([100 + (7 * s) % 80 for s in range(S)], dtype=np.uint32)      # a Z and position 31 behind it inside 135 frames: every line locks and reads its rate
    sm = d.wire_encode_host(pairs, pos)
    tiled = d.wire_encode_tiled_host(tile_pairs(pairs, R), pos)
    kinds = d.link_kinds(np.arange(S * P))["kind"]
    assert np.array_equal(kinds == host.LINK_I2S, types.reshape(-1)), "dspi_link_kinds follows REQ_SET_OUTPUT_TYPE"
    recs = {}
    flat = sm.reshape(-1)
    for line in np.flatnonzero(kinds == LM.SPDIF):
        rx = M.new_rx()
        got = LM.decode(flat, P, 0, F, int(line), LM.SPDIF, rx)
        s = line // P
        assert np.array_equal(got, pairs[s, line % P]) and rx["state"] == 2 and rx["sample_rate"] == rates[s] and rx["sync"] == 1 + (int(pos[s]) + F) % 192 and not rx["held"]
        recs[int(line)] = M.to_record(rx)
    d.close()
    return dict(S=S, P=P, R=R, pairs=pairs.reshape(S * P, F, 2), sm=sm, tiled=tiled, kinds=kinds, recs=recs)


def wire_decode(d, view, wire, links, rx, mem):
    """dspi_wire_decode on host or device buffers, the pair words pre-filled -> (pairs, records)"""
    n, F = len(links), int(view["n_frames"])
    if mem == "host":
        rx = rx.copy()
        return d.wire_decode_host(view, wire, links, rx, np.full((n, F, 2), FILL, dtype=np.int32)), rx
    torch, _ = dev()
    t_w, t_rx, t_p = up(wire), up(rx), up(np.full((n, F, 2), FILL, dtype=np.int32))
    v = view.copy(); v["wire"] = t_w.data_ptr()
    torch.cuda.synchronize()
    d.wire_decode_device(v, links, t_rx.data_ptr(), t_p.data_ptr())
    d.sync()
    return t_p.cpu().numpy().view(np.int32).reshape(n, F, 2), t_rx.cpu().numpy().view(RX).reshape(n).copy()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("F", [135, 240])
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_round_trip_of_the_encoders(fl, F, mem):
    e = encoded(fl, F)
    S, P, R = e["S"], e["P"], e["R"]
    d = host.Dspi(0, 3, device=0)      # (stateless per context: the decoding context is not the producer, nor of its flavour)
    for tiled in (False, True):
        view = np.zeros((), dtype=host.WIRE_VIEW)
        view["n_streams"], view["n_pairs"], view["tile_streams"], view["n_frames"] = S, P, R if tiled else 0, F
        for name, links in LM.link_orders(e["kinds"]).items():
            what = f"{fl} F={F} {mem} {'tiled' if tiled else 'stream-major'} {name}"
            got, rx = wire_decode(d, view, e["tiled"] if tiled else e["sm"], links, records_for(links), mem)
            for i, (line, kind) in enumerate(links.tolist()):
                if kind == LM.NONE:
                    assert (got[i] == FILL).all() and rx[i].tobytes() == bytes([POISON]) * 40, f"{what}: link {i} is a hole"
                    continue
                assert np.array_equal(got[i], e["pairs"][line]), f"{what}: link {i} (line {line}, kind {kind}) at {np.argwhere(got[i] != e['pairs'][line])[:3].tolist()}"
                assert rx[i].tobytes() == (e["recs"][line].tobytes() if kind == LM.SPDIF else bytes([POISON]) * 40), f"{what}: the record of link {i}: {rx[i]}"
    d.close()


def test_many_links_of_a_tiled_view(n=70000):
    """a thousand workgroups on one small view: any map, heavy fan-out, every link its own record"""
    F = 135
    e = encoded("q28", F)
    S, P, R = e["S"], e["P"], e["R"]
    lines = np.random.default_rng(n).integers(0, S * P, n)
    links = np.zeros(n, dtype=host.LINK); links["line"] = lines; links["kind"] = e["kinds"][lines]
    want_rx = poison(S * P)
    for line, rec in e["recs"].items(): want_rx[line] = rec
    view = np.zeros((), dtype=host.WIRE_VIEW)
    view["n_streams"], view["n_pairs"], view["tile_streams"], view["n_frames"] = S, P, R, F
    d = host.Dspi(1, 2, device=0)
    got, rx = wire_decode(d, view, e["tiled"], links, records_for(links), "device")
    assert np.array_equal(got, e["pairs"][lines]), np.argwhere((got != e["pairs"][lines]).any(axis=(1, 2)))[:5].tolist()
    assert rx.tobytes() == want_rx[lines].tobytes(), np.flatnonzero(rx != want_rx[lines])[:5].tolist()
    d.close()


# ---- 2. trouble per lane ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl,F", [("f32", 135), ("q28", 240)])
def test_trouble_per_lane_in_two_calls(fl, F):
    """the library's own subframes of 2 F frames, every S/PDIF column with its own kind of trouble (neighbouring columns differ, one column is
    all zeros), laid into two TILED buffers of F frames and decoded in two calls, the records carried on the device"""
    flavor = FLAVORS[fl]
    S = streams_of(flavor)
    p = host.Dspi(flavor, S, device=0)
    P, R = p.P, p.tile_streams()
    types = types_of(S, P)
    set_types(p, types)
    rng = np.random.default_rng(7)
    pairs = rng.integers(-(1 << 23), 1 << 23, (S, P, 2 * F, 2), dtype=np.int64).astype(np.int32)
    words = p.wire_encode_host(pairs, np.array([(11 * s) % 192 for s in range(S)], dtype=np.uint32)).reshape(S * P, 2 * F, 4)
    kinds = p.link_kinds(np.arange(S * P))["kind"]
    lines = {}
    for line in range(S * P):
        if kinds[line] == LM.I2S: lines[line] = words[line].reshape(-1)[:4 * F].reshape(2 * F, 2)      # (the first half of the region: [2 F][2])
        else: lines[line] = trouble(words[line].copy(), line // 2 % 4, F)
    zero = int(np.flatnonzero(kinds == LM.SPDIF)[5]); lines[zero][:] = 0
    links = LM.link_orders(kinds)["identity"]
    rx = records_for(links)
    model = {int(l): M.new_rx() for l in np.flatnonzero(kinds == LM.SPDIF)}
    view = p.wire_view_of(0, F, tiled=True)
    seen = np.zeros(3, dtype=bool)
    for k in range(2):
        half = {l: w[k * F:(k + 1) * F] for l, w in lines.items()}
        got, rx = wire_decode(p, view, LM.lay(half, S, P, R, F), links, rx, "device")
        for line in range(S * P):
            if kinds[line] == LM.I2S:
                assert np.array_equal(got[line], pairs[line // P, line % P, k * F:(k + 1) * F]) and rx[line].tobytes() == bytes([POISON]) * 40, (fl, k, line)
                continue
            want = M.receive(model[line], half[line])
            assert np.array_equal(got[line], want), (fl, k, line, np.argwhere(got[line] != want)[:3].tolist())
            assert rx[line].tobytes() == M.to_record(model[line]).tobytes(), (fl, k, line, rx[line], M.to_record(model[line]))
        seen |= np.array([rx["held"][kinds == LM.SPDIF].any(), rx["coding_errors"][kinds == LM.SPDIF].any(), rx["parity_err_count"][kinds == LM.SPDIF].any()])
    assert seen.all() and rx["state"][zero] == 0 and rx["coding_errors"][zero] == 4 * F, "the columns do what they were corrupted for"
    p.close()


# ---- 3. the linked call IS the sources call --------------------------------------------------------------------------------------------------------
def device_outputs(d, n, F, wire=False):
    torch, dv = dev()
    S = d.n_streams
    t = dict(pairs=torch.full((S, d.P, F, 4 if wire else 2), FILL, dtype=torch.int32, device=dv), sub=torch.full((S, F), FILL, dtype=torch.int32, device=dv),
             peaks=torch.full((S, n, d.C), 0x5A5A, dtype=torch.int16, device=dv), clip=torch.full((S,), 0x5A5A, dtype=torch.int16, device=dv))
    return t


def down(t): return [t[k].cpu().numpy() for k in ("pairs", "sub", "peaks", "clip")]


@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_linked_is_the_sources_call(fl):
    """a stream-major view, every link S/PDIF: dspi_process_linked on one context, dspi_process_sources on its twin fed the same lines gathered
    into its buffer — pair words, sub words, peaks, clip flags, status bytes and records byte for byte, over two calls"""
    torch, dv = dev()
    flavor = FLAVORS[fl]
    S, fs, n, Bk = streams_of(flavor), 48000, 5, 48
    F = n * Bk
    blob = WL.full_chain_blob(int(flavor))
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    warm = WL.synth_pcm16(S, WARM * 48, fs, first_stream=900)
    for x in (a, b): x.process_host(warm, WARM, 48, 16); x.pause_streams(5, 1)
    VS, VP = 25, 4      # the view: 100 lines of 2 F frames, each with its trouble
    rng = np.random.default_rng(3)
    lines = np.stack([trouble(M.encode(M.random_pairs(rng, 2 * F), (7 * l) % 192, (44100, 48000, 96000)[l % 3]), l % 4, F) for l in range(VS * VP)])
    links = np.zeros(S, dtype=host.LINK)
    links["line"] = (3 * np.arange(S)) % (VS * VP); links["kind"] = host.LINK_SPDIF      # (S = 150: fan-out)
    links["line"][5] = 0xffffffff; links["kind"][5] = 77                                    # (the paused stream's entry is ignored)
    rx0 = poison(S); rx0[np.arange(S) != 5] = np.zeros((), dtype=RX)
    t_rx = [up(rx0), up(rx0)]
    src = np.full(S, host.SRC_SPDIF, dtype=np.uint8)
    for k in range(2):
        wire = np.ascontiguousarray(lines[:, k * F:(k + 1) * F])
        t_wire = up(wire)
        gathered = wire[np.where(np.arange(S) == 5, 0, links["line"])]; gathered[5] = 0xA5A5A5A5      # (a paused stream's run is never read)
        t_in = up(gathered)
        view = np.zeros((), dtype=host.WIRE_VIEW)
        view["wire"], view["n_streams"], view["n_pairs"], view["n_frames"] = t_wire.data_ptr(), VS, VP, F
        oa, ob = device_outputs(a, n, F), device_outputs(b, n, F)
        torch.cuda.synchronize()
        a.process_linked_device(view, links, n, Bk, t_rx[0].data_ptr(), oa["pairs"].data_ptr(), oa["sub"].data_ptr(), oa["peaks"].data_ptr(), clip_ptr=oa["clip"].data_ptr())
        b.process_sources_device(t_in.data_ptr(), src, n, Bk, t_rx[1].data_ptr(), ob["pairs"].data_ptr(), ob["sub"].data_ptr(), ob["peaks"].data_ptr(), clip_ptr=ob["clip"].data_ptr())
        a.sync(); b.sync()
        for x, y, what in zip(down(oa), down(ob), ("pair words", "sub words", "peaks", "clip flags")): assert x.tobytes() == y.tobytes(), f"{fl} call {k}: {what}"
        ra, rb = t_rx[0].cpu().numpy(), t_rx[1].cpu().numpy()
        assert ra.tobytes() == rb.tobytes() and ra.view(RX)[5].tobytes() == bytes([POISON]) * 40, f"{fl} call {k}: records"
        assert [a.status(s) for s in range(S)] == [b.status(s) for s in range(S)], f"{fl} call {k}: status bytes"
        pairs = down(oa)[0]
        assert (pairs[5] == FILL).all() and pairs[np.arange(S) != 5].any() and (pairs[np.arange(S) != 5] != FILL).all(), "a paused stream is untouched, the others sound"
    assert ra.view(RX)["held"][np.arange(S) != 5].any() and ra.view(RX)["coding_errors"][np.arange(S) != 5].any() and ra.view(RX)["parity_err_count"].any()
    a.close(); b.close()


# ---- 4. a chain across flavours and layouts, held to the oracle ----------------------------------------------------------------------------------------
PAUSED = 5


def chain_case(fl_a, tiled_a, fl_b, out_b, n, Bk, rounds, line_of):
    """A runs dspi_process_devices on PCM, B = dspi_process_linked on A's buffer with view.producer = A and NO dspi_sync in between.
    out_b: "pairs", or "wire_tiled" (DSPI_OUT_WIRE | DSPI_OUT_TILED: B could be someone's producer in turn)."""
    torch, dv = dev()
    fa, fb = FLAVORS[fl_a], FLAVORS[fl_b]
    SA, SB = streams_of(fa), streams_of(fb)
    fs = 44100 if Bk == 45 else 48000
    F = n * Bk
    blob_a, blob_b = WL.full_chain_blob(int(fa)), WL.full_chain_blob(int(fb))
    A, B = context(fa, SA, fs, blob_a), context(fb, SB, fs, blob_b, vol=-10 * 256)
    PA, PB = A.P, B.P
    types_a = np.array([[(s // 2 + p) % 2 == 1 for p in range(PA)] for s in range(SA)])      # (by (s + p) % 2 the lines linked below would all be S/PDIF)
    types_b = np.zeros((SB, PB), dtype=bool)
    if out_b == "wire_tiled": types_b[::3, 1] = True
    set_types(A, types_a); set_types(B, types_b)
    warm_a, warm_b = WL.synth_pcm16(SA, WARM * 48, fs, first_stream=900), WL.synth_pcm16(SB, WARM * 48, fs, first_stream=1900)
    A.process_host(warm_a, WARM, 48, 16); B.process_host(warm_b, WARM, 48, 16)
    B.pause_streams(PAUSED, 1)
    status_paused = B.status(PAUSED)
    pcm = WL.synth_pcm16(SA, rounds * F, fs)
    lines = np.array([line_of(s) for s in range(SB)])
    links = A.link_kinds(lines)
    assert np.array_equal(links["kind"] == host.LINK_I2S, types_a.reshape(-1)[lines]) and (links["kind"] == host.LINK_I2S).any() and (links["kind"] == host.LINK_SPDIF).any()
    rx0 = records_for(links); rx0[PAUSED] = poison(1)[0]
    t_rx = up(rx0)
    RA = A.tile_streams()
    t_wire = torch.full((-(-SA // RA) * RA * PA * F * 4,), FILL, dtype=torch.int32, device=dv)      # (either layout fits)
    view = A.wire_view_of(t_wire.data_ptr(), F, tiled=tiled_a)
    depths = np.full(SA, 16, dtype=np.uint8)
    RB = B.tile_streams()
    got = []
    for k in range(rounds):
        t_pcm = up(packets(pcm, 16, Bk, k * n, (k + 1) * n))
        wire_b = out_b == "wire_tiled"
        o = device_outputs(B, n, F)
        if wire_b:
            o["pairs"] = torch.full((-(-SB // RB), PB, F, 4, RB), FILL, dtype=torch.int32, device=dv)
            o["sub"] = torch.full((-(-SB // RB), F, RB), FILL, dtype=torch.int32, device=dv)
        torch.cuda.synchronize()
        A.process_devices_device(t_pcm.data_ptr(), depths, n, Bk, t_wire.data_ptr(), tiled=tiled_a)
        B.process_linked_device(view, links, n, Bk, t_rx.data_ptr(), o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), clip_ptr=o["clip"].data_ptr(), wire=wire_b, tiled=wire_b)
        B.sync()
        pairs, sub, peaks, clip = down(o)
        if wire_b:
            raw_sub = sub
            pairs, sub = B.untile_wire(pairs.view(np.uint32), types_b), B.untile(None, sub)[1]
            assert (raw_sub.transpose(0, 2, 1).reshape(-1, F)[PAUSED] == FILL).all()
        got.append((pairs, sub, peaks.view(np.uint16), clip.view(np.uint16), t_rx.cpu().numpy().view(RX).reshape(SB).copy(), [B.status(s) for s in range(SB)]))
    # ---- the oracles: A's streams that are linked, then every B stream fed the model's decode of its line ----
    words_a = {}
    for sa in sorted({int(l) // PA for i, l in enumerate(lines) if i != PAUSED}):
        oa = oracle(fa, fs, blob_a, setup=lambda x, sa=sa: [x.vendor_get(R_["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1) for p in np.flatnonzero(types_a[sa])])
        oa.process(warm_a[sa], WARM, 48, 16)
        words_a[sa] = [oa.process(packets(pcm[sa], 16, Bk, k * n, (k + 1) * n), n, Bk, 16)[0] for k in range(rounds)]
    sounding = 0
    for s in range(SB):
        what = f"{fl_a}->{fl_b} stream {s} (line {lines[s]}, kind {links['kind'][s]})"
        if s == PAUSED:
            for k in range(rounds):
                pairs, sub, peaks, clip, rx, status = got[k]
                if out_b == "pairs": assert (pairs[s] == FILL).all() and (sub[s].view(np.uint32) == FILL).all()
                assert (peaks[s] == 0x5A5A).all() and clip[s] == int.from_bytes(status_paused[-2:], "little") and rx[s].tobytes() == bytes([POISON]) * 40 and status[s] == status_paused, what + ": paused"
            continue
        ob = oracle(fb, fs, blob_b, vol=-10 * 256, setup=lambda x, s=s: [x.vendor_get(R_["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1) for p in np.flatnonzero(types_b[s])])
        ob.process(warm_b[s], WARM, 48, 16)
        sa, pa = divmod(int(lines[s]), PA)
        model, pos_a, pos_b = M.new_rx(), 0, 0
        for k in range(rounds):
            pairs, sub, peaks, clip, rx, status = got[k]
            w = words_a[sa][k][pa]
            if types_a[sa, pa]: fed = (w.astype(np.uint32) << 8).view(np.int32) >> 8
            else: fed = M.receive(model, spdif_encode(w, pos_a, fs)[0])
            sounding += bool(fed.any())
            rp, rs, rk, rclip = ob.process(M.pack24(fed), n, Bk, 24)
            if out_b == "pairs": assert np.array_equal(rp, pairs[s]), what + f" round {k}: pair words"
            else:
                for p in range(PB):
                    region = pairs[s, p].reshape(-1)
                    if types_b[s, p]: assert np.array_equal(region[:2 * F], (rp[p].astype(np.uint32) << 8).reshape(-1)) and (region[2 * F:] == FILL).all(), what + f" round {k}: I2S slot {p}"
                    else: assert np.array_equal(pairs[s, p], spdif_encode(rp[p], pos_b, fs)[0]), what + f" round {k}: subframes of slot {p}"
            assert np.array_equal(rs, sub[s]) and np.array_equal(rk, peaks[s]) and int(clip[s]) == rclip, what + f" round {k}: sub words, peaks or clip flags"
            assert status[s] == ob.status(), what + f" round {k}: status bytes"
            assert rx[s].tobytes() == (bytes([POISON]) * 40 if types_a[sa, pa] else M.to_record(model).tobytes()), what + f" round {k}: record {rx[s]}"
            pos_a = (pos_a + F) % 192; pos_b = (pos_b + F) % 192
    assert 2 * sounding > (SB - 1) * rounds, "the chain carries sound (the preset leaves some pairs silent)"
    A.close(); B.close()


def test_chain_float_tiled_into_q28():
    chain_case("f32", True, "q28", "pairs", 5, 48, 2, lambda s: ((7 * s) % 150) * 4 + s % 4)


def test_chain_q28_stream_major_into_float_wire_tiled():
    chain_case("q28", False, "f32", "wire_tiled", 3, 45, 1, lambda s: ((7 * s) % 100) * 2 + s % 2)      # (150 consumers of 100 streams: fan-out)


# ---- 5. the refusals that need a device --------------------------------------------------------------------------------------------------------------
def test_device_refusals_write_nothing():
    torch, dv = dev()
    S, F = 12, 48
    d = host.Dspi(0, S, device=0)
    a = host.Dspi(1, 5, device=0)
    t_wire = torch.full((5 * 4 * F * 4 + 8,), 0x11, dtype=torch.int32, device=dv)
    o = device_outputs(d, 1, F)
    links = np.zeros(S, dtype=host.LINK); links["line"] = np.arange(S); links["kind"] = host.LINK_SPDIF
    rx0 = np.zeros(S + 1, dtype=RX); rx0["held"] = 77
    t_rx = up(rx0)
    out = host._Out(o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), o["clip"].data_ptr())
    status = [d.status(s) for s in range(S)]
    call = lambda v, r, flags: d.L.dspi_process_linked(d.h, v.ctypes.data, links.ctypes.data, 1, F, C.byref(out), None, r, flags)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    good = a.wire_view_of(t_wire.data_ptr(), F)
    off = a.wire_view_of(t_wire.data_ptr() + 8, F)
    DEV = host.MEM_DEVICE | host.OUT_CLIP_FLAGS
    assert call(good, t_rx.data_ptr(), host.OUT_CLIP_FLAGS) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    assert call(off, t_rx.data_ptr(), DEV) == host.E_INVAL and "aligned" in err()
    assert call(good, t_rx.data_ptr() + 2, DEV) == host.E_INVAL and "4-byte" in err()
    assert call(good, None, DEV) == host.E_INVAL and "(rx)" in err()
    # dspi_wire_decode
    t_p = torch.full((S, F, 2), FILL, dtype=torch.int32, device=dv)
    dec = lambda v, r, p: d.L.dspi_wire_decode(d.h, v.ctypes.data, links.ctypes.data, S, r, p, host.MEM_DEVICE)
    assert dec(off, t_rx.data_ptr(), t_p.data_ptr()) == host.E_INVAL and "aligned" in err()
    assert dec(good, t_rx.data_ptr() + 8, t_p.data_ptr()) == host.E_INVAL and "16-byte" in err()
    assert dec(good, t_rx.data_ptr(), t_p.data_ptr() + 8) == host.E_INVAL and "16-byte" in err()
    d.sync()
    assert (t_p.cpu().numpy() == FILL).all() and t_rx.cpu().numpy().tobytes() == rx0.tobytes(), "a refused call wrote"
    pairs, sub, peaks, clip = down(o)
    assert (pairs == FILL).all() and (sub == FILL).all() and (peaks == 0x5A5A).all() and (clip == 0x5A5A).all(), "a refused call wrote output"
    assert [d.status(s) for s in range(S)] == status and d.spdif_block_pos() == 0
    # ... and the context still works: lines of 0x11 words are no subframes
    assert call(good, t_rx.data_ptr(), DEV) == 0
    d.sync()
    rx = t_rx.cpu().numpy().view(RX)
    assert (rx["coding_errors"][:S] == 2 * F).all() and (rx["state"][:S] == 0).all() and (rx["held"][:S] == 77 + 2 * F).all() and rx[S].tobytes() == rx0[S].tobytes()
    d.close(); a.close()
