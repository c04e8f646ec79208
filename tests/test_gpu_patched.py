"""The patch bay on the GPU (include/dspi.h: dspi_process_patched).

What each part is held to, always for equality:
  the equivalences    dspi_process_sources and dspi_process_linked on a twin context: pair words, sub words, peaks, clip flags, status bytes and
                      every byte of every record (tests 1, 2 and 5)
  the sample path     every consumer stream's own Oracle(detmath=True): PCM streams fed at their native depth, the others the model's decode
                      (tests/patch_model.py, tests/linkrx_model.py, tests/spdifrx_model.py) of their line, the producers' words coming from
                      their own oracles (tests 3 and 4)
Shapes: float S = 150, Q28 S = 100 (three and two workgroups, neither a multiple of 64).  Outputs and records are pre-filled (FILL, POISON), so
a stream that is served twice, not at all, or from the wrong column shows.  References are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import linkrx_model as LM
import patch_model as PM
import spdifrx_model as M
from conftest import has_gpu
from orclib import spdif_encode
from dspi_amd import host, wire as W, workloads as WL
from test_gpu_link import FILL, WARM, dev, device_outputs, down, poison, set_types, up
from test_gpu_snapshot import context, oracle
from test_gpu_spdif_in import FLAVORS, POISON, RX, streams_of, trouble

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

R_ = W.REQ
PAUSED = 5
IN_FILL = 0xA5      # a paused stream's bytes and the padding in front of S/PDIF runs: never read


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_process_patched"), "libdspi_mi355x has no dspi_process_patched"


def input_buffer(d, src, n, Bk, runs):
    """`in` of a patched call: runs {stream: array} at their offsets, everything else IN_FILL"""
    total, off = d.patched_bytes(src, n, Bk)
    assert off.tolist() == PM.offsets(src, n * Bk)
    buf = np.full(max(total, 16), IN_FILL, dtype=np.uint8)
    for s, x in runs.items():
        x = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        assert x.nbytes == n * Bk * PM.SIZE[int(src[s])]
        buf[int(off[s]):int(off[s]) + x.nbytes] = x
    return buf


def same(oa, ob, a, b, t_rxa, t_rxb, what):
    for x, y, name in zip(down(oa), down(ob), ("pair words", "sub words", "peaks", "clip flags")): assert x.tobytes() == y.tobytes(), f"{what}: {name}"
    ra, rb = t_rxa.cpu().numpy(), t_rxb.cpu().numpy()
    assert ra.tobytes() == rb.tobytes(), f"{what}: records"
    assert [a.status(s) for s in range(a.n_streams)] == [b.status(s) for s in range(b.n_streams)], f"{what}: status bytes"
    return ra.view(RX).reshape(-1)


# ---- 1. with no LINK stream the call IS the sources call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_patched_is_the_sources_call(fl):
    torch, dv = dev()
    flavor = FLAVORS[fl]
    S, fs, n, Bk = streams_of(flavor), 48000, 5, 48
    F = n * Bk
    blob = WL.full_chain_blob(int(flavor))
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    warm = WL.synth_pcm16(S, WARM * 48, fs, first_stream=900)
    for x in (a, b): x.process_host(warm, WARM, 48, 16); x.pause_streams(PAUSED, 1)
    src = np.array([(16, 24, 1)[s % 3] for s in range(S)], dtype=np.uint8)
    assert src[PAUSED] == 1
    p16 = WL.synth_pcm16(S, 2 * F, fs); p24 = WL.pcm16_to_pcm24_bytes(p16)
    rng = np.random.default_rng(11)
    lines = {s: trouble(M.encode(M.random_pairs(rng, 2 * F), (7 * s) % 192, (44100, 48000, 96000)[s // 3 % 3]), s // 3 % 4, F) for s in range(S) if src[s] == 1}
    rx0 = poison(S); rx0[[s for s in lines if s != PAUSED]] = np.zeros((), dtype=RX)
    t_rx = [up(rx0), up(rx0)]
    assert a.patched_bytes(src, n, Bk)[1].tolist() == a.sources_bytes(src, n, Bk)[1].tolist()
    # (views and patches that nobody names: not looked at)
    patches = np.zeros(S, dtype=host.PATCH); patches["view"] = 0xffffffff
    for k in range(2):
        runs = {s: lines[s][k * F:(k + 1) * F] if src[s] == 1 else p24[s, 6 * k * F:6 * (k + 1) * F] if src[s] == 24 else p16[s, k * F:(k + 1) * F] for s in range(S) if s != PAUSED}
        t_in = up(input_buffer(a, src, n, Bk, runs))
        oa, ob = device_outputs(a, n, F), device_outputs(b, n, F)
        torch.cuda.synchronize()
        a.process_patched_device(t_in.data_ptr(), src, None, patches if k else None, n, Bk, t_rx[0].data_ptr(), oa["pairs"].data_ptr(), oa["sub"].data_ptr(), oa["peaks"].data_ptr(), clip_ptr=oa["clip"].data_ptr())
        b.process_sources_device(t_in.data_ptr(), src, n, Bk, t_rx[1].data_ptr(), ob["pairs"].data_ptr(), ob["sub"].data_ptr(), ob["peaks"].data_ptr(), clip_ptr=ob["clip"].data_ptr())
        a.sync(); b.sync()
        rx = same(oa, ob, a, b, t_rx[0], t_rx[1], f"{fl} call {k}")
        pairs = down(oa)[0]
        others = np.arange(S) != PAUSED
        assert (pairs[PAUSED] == FILL).all() and (pairs[others] != FILL).all() and all(pairs[src == x][np.flatnonzero(src == x) != PAUSED].any() for x in (16, 24, 1)), "a paused stream is untouched, the others sound"
        assert all(rx[s].tobytes() == bytes([POISON]) * 40 for s in range(S) if src[s] != 1 or s == PAUSED), "only the S/PDIF runs' records are written"
    assert rx["held"][others & (src == 1)].any() and rx["coding_errors"][others & (src == 1)].any() and (rx["state"][others & (src == 1)] == 2).any()
    a.close(); b.close()


# ---- 2. with every stream a LINK stream and one view the call IS the linked call ----------------------------------------------------------------
@pytest.mark.parametrize("fl", ["f32", "q28"])
def test_patched_is_the_linked_call(fl):
    """the inputs of test_gpu_link.py::test_linked_is_the_sources_call: a stream-major view of 100 lines with their trouble, fan-out"""
    torch, dv = dev()
    flavor = FLAVORS[fl]
    S, fs, n, Bk = streams_of(flavor), 48000, 5, 48
    F = n * Bk
    blob = WL.full_chain_blob(int(flavor))
    a, b = context(flavor, S, fs, blob), context(flavor, S, fs, blob)
    warm = WL.synth_pcm16(S, WARM * 48, fs, first_stream=900)
    for x in (a, b): x.process_host(warm, WARM, 48, 16); x.pause_streams(PAUSED, 1)
    VS, VP = 25, 4
    rng = np.random.default_rng(3)
    lines = np.stack([trouble(M.encode(M.random_pairs(rng, 2 * F), (7 * l) % 192, (44100, 48000, 96000)[l % 3]), l % 4, F) for l in range(VS * VP)])
    links = np.zeros(S, dtype=host.LINK)
    links["line"] = (3 * np.arange(S)) % (VS * VP); links["kind"] = host.LINK_SPDIF
    links["line"][PAUSED] = 0xffffffff; links["kind"][PAUSED] = 77
    patches = np.zeros(S, dtype=host.PATCH); patches["line"] = links["line"]; patches["kind"] = links["kind"]; patches["view"][PAUSED] = 9
    src = np.full(S, host.SRC_LINK, dtype=np.uint8)
    rx0 = poison(S); rx0[np.arange(S) != PAUSED] = np.zeros((), dtype=RX)
    t_rx = [up(rx0), up(rx0)]
    for k in range(2):
        t_wire = up(np.ascontiguousarray(lines[:, k * F:(k + 1) * F]))
        view = np.zeros((), dtype=host.WIRE_VIEW)
        view["wire"], view["n_streams"], view["n_pairs"], view["n_frames"] = t_wire.data_ptr(), VS, VP, F
        oa, ob = device_outputs(a, n, F), device_outputs(b, n, F)
        torch.cuda.synchronize()
        a.process_patched_device(0, src, view, patches, n, Bk, t_rx[0].data_ptr(), oa["pairs"].data_ptr(), oa["sub"].data_ptr(), oa["peaks"].data_ptr(), clip_ptr=oa["clip"].data_ptr())
        b.process_linked_device(view, links, n, Bk, t_rx[1].data_ptr(), ob["pairs"].data_ptr(), ob["sub"].data_ptr(), ob["peaks"].data_ptr(), clip_ptr=ob["clip"].data_ptr())
        a.sync(); b.sync()
        rx = same(oa, ob, a, b, t_rx[0], t_rx[1], f"{fl} call {k}")
        pairs = down(oa)[0]
        assert rx[PAUSED].tobytes() == bytes([POISON]) * 40 and (pairs[PAUSED] == FILL).all() and (pairs[np.arange(S) != PAUSED] != FILL).all() and pairs[np.arange(S) != PAUSED].any()
    assert rx["held"][np.arange(S) != PAUSED].any() and rx["coding_errors"][np.arange(S) != PAUSED].any() and rx["parity_err_count"].any()
    a.close(); b.close()


# ---- 3. the patch bay, held to the oracle ----------------------------------------------------------------------------------------------------------
BAY_FS = 44100
BAY_ROUNDS = ((3, 45), (5, 48))      # F = 135 (135 % 8 != 0: the receiver's tail), then 240
BAY_AT = (0, 135, 375)
VOL_C = -10 * 256
def line_a(s): return ((7 * s) % 150) * 4 + s % 4      # test_gpu_link.py::test_chain_float_tiled_into_q28
def line_b(s): return ((7 * s) % 100) * 2 + s % 2      # ... ::test_chain_q28_stream_major_into_float_wire_tiled
def types_prod(S, P): return np.array([[(s // 2 + p) % 2 == 1 for p in range(P)] for s in range(S)])
def bay_sources(S): return np.array([(16, 24, 1, 2, 2)[s % 5] for s in range(S)], dtype=np.uint8)
def i2s_fed(w): return (w.astype(np.uint32) << 8).view(np.int32) >> 8


@functools.lru_cache(maxsize=None)
def bay_producers():
    """A (float, 150 streams) and B (Q28, 100 streams): their PCM, and per linked producer stream the oracle's pair words of both rounds"""
    out = {}
    for name, fl, first, line_of, k5 in (("a", "f32", 0, line_a, 3), ("b", "q28", 400, line_b, 4)):
        flavor = FLAVORS[fl]
        S = streams_of(flavor)
        blob = WL.full_chain_blob(int(flavor))
        P = 4 if int(flavor) else 2
        types = types_prod(S, P)
        warm, pcm = WL.synth_pcm16(S, WARM * 48, BAY_FS, first_stream=900 + first), WL.synth_pcm16(S, BAY_AT[-1], BAY_FS, first_stream=first)
        words = {}
        for sp in sorted({line_of(s) // P for s in range(150) if s % 5 == k5}):
            o = oracle(flavor, BAY_FS, blob, setup=lambda x, sp=sp: [x.vendor_get(R_["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1) for p in np.flatnonzero(types[sp])])
            o.process(warm[sp], WARM, 48, 16)
            words[sp] = [o.process(np.ascontiguousarray(pcm[sp, BAY_AT[k]:BAY_AT[k + 1]]), n, Bk, 16)[0] for k, (n, Bk) in enumerate(BAY_ROUNDS)]
        out[name] = dict(flavor=flavor, S=S, P=P, blob=blob, types=types, warm=warm, pcm=pcm, words=words)
    return out


@functools.lru_cache(maxsize=None)
def bay_reference(fl_c, wire_c):
    """the consumer C on the CPU: per stream and round what it is fed (its run's bytes for `in`, or nothing: a LINK stream), the model's record
    and its own oracle's outputs.  The cap is checked here, with the oracles alone."""
    prod = bay_producers()
    flavor = FLAVORS[fl_c]
    S = streams_of(flavor)
    P = 4 if int(flavor) else 2
    blob = WL.full_chain_blob(int(flavor))
    src = bay_sources(S)
    types = np.zeros((S, P), dtype=bool)
    if wire_c: types[::3, 1] = True
    warm = WL.synth_pcm16(S, WARM * 48, BAY_FS, first_stream=2900)
    p16 = WL.synth_pcm16(S, BAY_AT[-1], BAY_FS, first_stream=3300); p24 = WL.pcm16_to_pcm24_bytes(p16)
    rng = np.random.default_rng(5)
    patches = np.zeros(S, dtype=host.PATCH)
    runs, recs, outs, status = [{} for _ in BAY_ROUNDS], [{} for _ in BAY_ROUNDS], [{} for _ in BAY_ROUNDS], [{} for _ in BAY_ROUNDS]
    sounding = np.zeros((len(BAY_ROUNDS), 5), dtype=int)
    for s in range(S):
        k5 = s % 5
        o = oracle(flavor, BAY_FS, blob, vol=VOL_C, setup=lambda x, s=s: [x.vendor_get(R_["SET_OUTPUT_TYPE"], int(p) | (1 << 8), 1) for p in np.flatnonzero(types[s])])
        o.process(warm[s], WARM, 48, 16)
        if s == PAUSED:
            status[0][s] = o.status()
            patches[s] = (0xffffffff, 0xffffffff, 77)
            continue
        model = M.new_rx()
        spdif = k5 == 2
        if k5 >= 3:
            pr = prod["a" if k5 == 3 else "b"]
            line = (line_a if k5 == 3 else line_b)(s)
            sp, pp = divmod(line, pr["P"])
            spdif = not pr["types"][sp, pp]
            patches[s] = (k5 - 3, line, host.LINK_SPDIF if spdif else host.LINK_I2S)
        pos = 0
        for k, (n, Bk) in enumerate(BAY_ROUNDS):
            F, f0, f1 = n * Bk, BAY_AT[k], BAY_AT[k + 1]
            if k5 == 0: runs[k][s] = p16[s, f0:f1]; x, depth = runs[k][s], 16
            elif k5 == 1: runs[k][s] = p24[s, 6 * f0:6 * f1]; x, depth = runs[k][s], 24
            else:
                if k5 == 2:
                    w = trouble(M.encode(M.random_pairs(rng, 2 * F) >> 3, (7 * s) % 192, (44100, 48000, 96000)[s // 5 % 3]), s // 5 % 4, F)[:F]
                    runs[k][s] = w
                    fed = M.receive(model, w)
                else:
                    w = pr["words"][sp][k][pp]
                    fed = M.receive(model, spdif_encode(w, pos, BAY_FS)[0]) if spdif else i2s_fed(w)
                x, depth = M.pack24(fed), 24
                sounding[k, k5] += bool(fed.any())
            if k5 < 2: sounding[k, k5] += bool(np.asarray(x).any())
            outs[k][s] = o.process(np.ascontiguousarray(x), n, Bk, depth)
            status[k][s] = o.status()
            recs[k][s] = M.to_record(model) if spdif else None
            pos = (pos + F) % 192
    n_link = sum(1 for s in range(S) if s % 5 >= 3 and s != PAUSED)
    assert (2 * (sounding[:, 3] + sounding[:, 4]) > n_link).all() and (sounding > 0).all(), f"the cap: {sounding.tolist()} of {n_link} LINK streams"
    return dict(flavor=flavor, S=S, P=P, blob=blob, src=src, types=types, warm=warm, patches=patches, runs=runs, recs=recs, outs=outs, status=status)


@pytest.mark.parametrize("fl_c,wire_c", [("fma", False), ("q28", True)], ids=["fma-pairs", "q28-wire-tiled"])
def test_patch_bay_held_to_the_oracle(fl_c, wire_c):
    """C takes PCM16, PCM24 and S/PDIF runs from `in`, lines of A's TILED wire words and lines of B's stream-major wire words in ONE call, with
    both views' producers set and no dspi_sync between the three calls of a round"""
    torch, dv = dev()
    prod, ref = bay_producers(), bay_reference(fl_c, wire_c)
    S, P, src, types, patches = ref["S"], ref["P"], ref["src"], ref["types"], ref["patches"]
    ctx = {}
    for name in ("a", "b"):
        p = prod[name]
        ctx[name] = context(p["flavor"], p["S"], BAY_FS, p["blob"])
        set_types(ctx[name], p["types"])
        ctx[name].process_host(p["warm"], WARM, 48, 16)
    c = context(ref["flavor"], S, BAY_FS, ref["blob"], vol=VOL_C)
    set_types(c, types)
    c.process_host(ref["warm"], WARM, 48, 16)
    c.pause_streams(PAUSED, 1)
    status_paused = c.status(PAUSED)
    A, B = ctx["a"], ctx["b"]
    RA, RC = A.tile_streams(), c.tile_streams()
    spdif_streams = [s for s in range(S) if s != PAUSED and ref["recs"][0][s] is not None]
    rx0 = poison(S); rx0[spdif_streams] = np.zeros((), dtype=RX)
    t_rx = up(rx0)
    Fmax = 240
    t_wa = torch.full((-(-A.n_streams // RA) * RA * A.P * Fmax * 4,), FILL, dtype=torch.int32, device=dv)
    t_wb = torch.full((B.n_streams * B.P * Fmax * 4,), FILL, dtype=torch.int32, device=dv)
    d16a, d16b = np.full(A.n_streams, 16, dtype=np.uint8), np.full(B.n_streams, 16, dtype=np.uint8)
    pos_c = 0
    for k, (n, Bk) in enumerate(BAY_ROUNDS):
        F, f0, f1 = n * Bk, BAY_AT[k], BAY_AT[k + 1]
        views = np.stack([A.wire_view_of(t_wa.data_ptr(), F, tiled=True), B.wire_view_of(t_wb.data_ptr(), F)])
        t_pa, t_pb = up(prod["a"]["pcm"][:, f0:f1]), up(prod["b"]["pcm"][:, f0:f1])
        t_in = up(input_buffer(c, src, n, Bk, ref["runs"][k]))
        o = device_outputs(c, n, F)
        if wire_c:
            o["pairs"] = torch.full((-(-S // RC), P, F, 4, RC), FILL, dtype=torch.int32, device=dv)
            o["sub"] = torch.full((-(-S // RC), F, RC), FILL, dtype=torch.int32, device=dv)
        torch.cuda.synchronize()
        A.process_devices_device(t_pa.data_ptr(), d16a, n, Bk, t_wa.data_ptr(), tiled=True)
        B.process_devices_device(t_pb.data_ptr(), d16b, n, Bk, t_wb.data_ptr(), tiled=False)
        c.process_patched_device(t_in.data_ptr(), src, views, patches, n, Bk, t_rx.data_ptr(), o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), clip_ptr=o["clip"].data_ptr(),
                                 wire=wire_c, tiled=wire_c)
        c.sync()
        pairs, sub, peaks, clip = down(o)
        peaks, clip = peaks.view(np.uint16), clip.view(np.uint16)
        if wire_c:
            assert (sub.transpose(0, 2, 1).reshape(-1, F)[PAUSED] == FILL).all()
            pairs, sub = c.untile_wire(pairs.view(np.uint32), types), c.untile(None, sub)[1]
        rx = t_rx.cpu().numpy().view(RX).reshape(S)
        for s in range(S):
            what = f"{fl_c} round {k} stream {s} (source {src[s]}, patch {patches[s]})"
            if s == PAUSED:
                if not wire_c: assert (pairs[s] == FILL).all() and (sub[s].view(np.uint32) == FILL).all(), what + ": paused"
                assert (peaks[s] == 0x5A5A).all() and clip[s] == int.from_bytes(status_paused[-2:], "little") and rx[s].tobytes() == bytes([POISON]) * 40 and c.status(s) == status_paused, what + ": paused"
                continue
            rp, rs, rk, rclip = ref["outs"][k][s]
            if not wire_c: assert np.array_equal(rp, pairs[s]), what + f": pair words at {np.argwhere(rp != pairs[s])[:3].tolist()}"
            else:
                for p in range(P):
                    region = pairs[s, p].reshape(-1)
                    if types[s, p]: assert np.array_equal(region[:2 * F], (rp[p].astype(np.uint32) << 8).reshape(-1)) and (region[2 * F:] == FILL).all(), what + f": I2S slot {p}"
                    else: assert np.array_equal(pairs[s, p], spdif_encode(rp[p], pos_c, BAY_FS)[0]), what + f": subframes of slot {p}"
            assert np.array_equal(rs, sub[s]) and np.array_equal(rk, peaks[s]) and int(clip[s]) == rclip, what + ": sub words, peaks or clip flags"
            assert c.status(s) == ref["status"][k][s], what + ": status bytes"
            want = ref["recs"][k][s]
            assert rx[s].tobytes() == (want.tobytes() if want is not None else bytes([POISON]) * 40), what + f": record {rx[s]}, want {want}"
        pos_c = (pos_c + F) % 192
    for x in (A, B, c): x.close()


# ---- 4. a chain inside one context -------------------------------------------------------------------------------------------------------------------
def test_chain_inside_one_context():
    """odd stream s eats pair 0 of stream s - 1 from the PREVIOUS call's wire buffer (producer == ctx, two buffers used alternately)"""
    torch, dv = dev()
    flavor, S, fs, n, Bk, rounds = FLAVORS["q28"], 100, 48000, 2, 48, 3
    F = n * Bk
    blob = WL.full_chain_blob(0)
    c = context(flavor, S, fs, blob)
    P = c.P
    warm = WL.synth_pcm16(S, WARM * 48, fs, first_stream=900)
    c.process_host(warm, WARM, 48, 16)
    c.spdif_block_pos(96)      # the silence ends where round 0 begins: the receivers find one unbroken signal
    assert c.spdif_block_pos() == 96
    p24 = WL.pcm16_to_pcm24_bytes(WL.synth_pcm16(S, rounds * F, fs))
    silence = c.wire_encode_host(np.zeros((S, P, F, 2), dtype=np.int32), np.zeros(S, dtype=np.uint32))
    assert np.array_equal(silence[0, 0], spdif_encode(np.zeros((F, 2), dtype=np.int32), 0, fs)[0])
    bufs = [torch.full((S * P * F * 4,), FILL, dtype=torch.int32, device=dv), up(silence).view(torch.int32)]
    src = np.where(np.arange(S) % 2 == 0, 24, host.SRC_LINK).astype(np.uint8)
    patches = np.zeros(S, dtype=host.PATCH); patches["line"] = (np.arange(S) - 1) * P; patches["kind"] = host.LINK_SPDIF; patches["line"][::2] = 0xffffffff
    rx0 = poison(S); rx0[1::2] = np.zeros((), dtype=RX)
    t_rx = up(rx0)
    got, sounding = [], 0
    for k in range(rounds):
        view = c.wire_view_of(bufs[(k + 1) % 2].data_ptr(), F)
        assert int(view["producer"]) == c.h.value
        runs = {s: p24[s, 6 * k * F:6 * (k + 1) * F] for s in range(0, S, 2)}
        t_in = up(input_buffer(c, src, n, Bk, runs))
        o = device_outputs(c, n, F, wire=True)
        o["pairs"] = bufs[k % 2].view(S, P, F, 4)
        torch.cuda.synchronize()
        c.process_patched_device(t_in.data_ptr(), src, view, patches, n, Bk, t_rx.data_ptr(), o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), clip_ptr=o["clip"].data_ptr(), wire=True)
        c.sync()
        pairs, sub, peaks, clip = down(o)
        got.append((pairs.view(np.uint32).copy(), sub, peaks.view(np.uint16), clip.view(np.uint16), t_rx.cpu().numpy().view(RX).reshape(S).copy(), [c.status(s) for s in range(S)]))
    for s in range(0, S, 2):
        oe, oo = oracle(flavor, fs, blob), oracle(flavor, fs, blob)
        oe.process(warm[s], WARM, 48, 16); oo.process(warm[s + 1], WARM, 48, 16)
        model = M.new_rx()
        before = spdif_encode(np.zeros((F, 2), dtype=np.int32), 0, fs)[0]
        for k in range(rounds):
            pairs, sub, peaks, clip, rx, status = got[k]
            pos = (96 + k * F) % 192
            fed = M.receive(model, before)
            sounding += bool(fed.any())
            for t, orc, x in ((s, oe, p24[s, 6 * k * F:6 * (k + 1) * F]), (s + 1, oo, M.pack24(fed))):
                what = f"round {k} stream {t}"
                rp, rs, rk, rclip = orc.process(np.ascontiguousarray(x), n, Bk, 24)
                words = np.stack([spdif_encode(rp[p], pos, fs)[0] for p in range(P)])
                assert np.array_equal(words, pairs[t]), what + ": wire words"
                assert np.array_equal(rs, sub[t]) and np.array_equal(rk, peaks[t]) and int(clip[t]) == rclip and status[t] == orc.status(), what + ": sub words, peaks, clip flags or status"
                if t == s: before = words[0]
            assert rx[s].tobytes() == bytes([POISON]) * 40 and rx[s + 1].tobytes() == M.to_record(model).tobytes(), f"round {k}: records of streams {s}, {s + 1}: {rx[s + 1]}"
            assert rx[s + 1]["state"] == 2 and rx[s + 1]["coding_errors"] == 0 and rx[s + 1]["held"] == 0, f"round {k}: stream {s + 1} is LOCKED"
    assert 2 * sounding > (S // 2) * (rounds - 1), "the chain carries sound"
    c.close()


# ---- 5. tiled views of both tile sizes in one launch ----------------------------------------------------------------------------------------------------
TILED_VIEWS = ((128, 4, 128), (100, 2, 64), (150, 4, 128))      # (streams, pairs, tile): a whole tile of 128, tiles of 64, a ragged last tile of 128


def short_lines(S, P, F, seed):
    """LM.build for a call shorter than its corruptions reach: types by (s + p) % 2, V, a bad preamble or a zero frame by line"""
    rng = np.random.default_rng(seed)
    lines, kinds = {}, np.zeros(S * P, dtype=np.uint32)
    for line in range(S * P):
        s, p = divmod(line, P)
        pairs = M.random_pairs(rng, F)
        if (s + p) % 2: kinds[line] = LM.I2S; lines[line] = (pairs.astype(np.uint32) << 8) | np.uint32(line & 0xff)
        else:
            kinds[line] = LM.SPDIF
            w = M.encode(pairs, (190 + line) % 192, 48000)      # (most lines pass a Z inside their five frames)
            if line % 4 == 1: M.set_v(w, 1, 0)
            elif line % 4 == 2: M.set_preamble(w, F - 1, 1, M.X)
            elif line % 4 == 3: w[F // 2] = 0
            lines[line] = w
    return lines, kinds


@pytest.mark.parametrize("F,n,Bk", [(5, 1, 5), (135, 3, 45)])
def test_tiled_views_of_both_tile_sizes_in_one_launch(F, n, Bk):
    """stream s patches view s % 3, kinds alternating per lane; held to dspi_process_linked run once per view on twins with the other streams paused"""
    torch, dv = dev()
    flavor, S, fs = FLAVORS["q28"], 100, 48000
    blob = WL.full_chain_blob(0)
    warm = WL.synth_pcm16(S, WARM * 48, fs, first_stream=900)
    views, wires, kinds = np.zeros(3, dtype=host.WIRE_VIEW), [], []
    for v, (VS, VP, R) in enumerate(TILED_VIEWS):
        lines, kd = LM.build(VS, VP, F, seed=F + v) if F >= 135 else short_lines(VS, VP, F, seed=F + v)
        wires.append(up(LM.lay(lines, VS, VP, R, F))); kinds.append(kd)
        views[v] = (wires[v].data_ptr(), VS, VP, R, F, 0)
    patches = np.zeros(S, dtype=host.PATCH)
    for s in range(S):
        v = s % 3
        want = LM.SPDIF if s % 2 else LM.I2S
        of_kind = np.flatnonzero(kinds[v] == want)
        patches[s] = (v, of_kind[-1 - (7 * s) % len(of_kind)] if s % 4 < 2 else of_kind[(11 * s) % len(of_kind)], want)      # (the ragged tile's last streams among them)
    src = np.full(S, host.SRC_LINK, dtype=np.uint8)
    rx0 = poison(S); rx0[1::2] = np.zeros((), dtype=RX)
    main = context(flavor, S, fs, blob)
    main.process_host(warm, WARM, 48, 16)
    t_rx = up(rx0)
    o = device_outputs(main, n, F)
    torch.cuda.synchronize()
    main.process_patched_device(0, src, views, patches, n, Bk, t_rx.data_ptr(), o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), clip_ptr=o["clip"].data_ptr())
    main.sync()
    got, rx = down(o), t_rx.cpu().numpy().view(RX).reshape(S)
    status = [main.status(s) for s in range(S)]
    assert all(rx[s].tobytes() == bytes([POISON]) * 40 for s in range(0, S, 2)), "an I2S patch has no record"
    for v in range(3):
        twin = context(flavor, S, fs, blob)
        twin.process_host(warm, WARM, 48, 16)
        for s in range(S):
            if s % 3 != v: twin.pause_streams(s, 1)
        links = np.zeros(S, dtype=host.LINK); links["line"] = patches["line"]; links["kind"] = patches["kind"]
        t_rx2 = up(rx0)
        o2 = device_outputs(twin, n, F)
        torch.cuda.synchronize()
        twin.process_linked_device(views[v:v + 1].reshape(()), links, n, Bk, t_rx2.data_ptr(), o2["pairs"].data_ptr(), o2["sub"].data_ptr(), o2["peaks"].data_ptr(), clip_ptr=o2["clip"].data_ptr())
        twin.sync()
        want, rx2 = down(o2), t_rx2.cpu().numpy().view(RX).reshape(S)
        mine = np.arange(S) % 3 == v
        for x, y, name in zip(got, want, ("pair words", "sub words", "peaks", "clip flags")):
            assert x[mine].tobytes() == y[mine].tobytes(), f"F={F} view {v}: {name} of streams {np.flatnonzero(mine)[[x[s].tobytes() != y[s].tobytes() for s in np.flatnonzero(mine)]][:5].tolist()}"
        assert rx[mine].tobytes() == rx2[mine].tobytes(), f"F={F} view {v}: records"
        assert [status[s] for s in np.flatnonzero(mine)] == [twin.status(int(s)) for s in np.flatnonzero(mine)], f"F={F} view {v}: status bytes"
        twin.close()
    if F >= 135: assert rx["held"][1::2].any() and rx["coding_errors"][1::2].any() and (rx["state"][1::2] == 2).any(), "the columns do what they were corrupted for"
    assert (got[0] != FILL).all() and got[0].any()
    main.close()


# ---- 6. the refusals that need a device --------------------------------------------------------------------------------------------------------------
def test_device_refusals_write_nothing():
    torch, dv = dev()
    S, F = 12, 48
    d = host.Dspi(0, S, device=0)
    a = host.Dspi(1, 5, device=0)
    t_wire = torch.full((128 * 4 * F * 4 + 8,), 0x11, dtype=torch.int32, device=dv)
    o = device_outputs(d, 1, F)
    src = np.array([16, 24, 1, 2, 2, 2] * 2, dtype=np.uint8)
    patches = np.zeros(S, dtype=host.PATCH); patches["view"] = np.arange(S) % 2; patches["line"] = np.arange(S); patches["kind"] = host.LINK_SPDIF
    rx0 = np.zeros(S + 1, dtype=RX); rx0["held"] = 77
    t_rx = up(rx0)
    t_in = torch.full((d.patched_bytes(src, 1, F)[0] + 16,), 0x11, dtype=torch.uint8, device=dv)
    out = host._Out(o["pairs"].data_ptr(), o["sub"].data_ptr(), o["peaks"].data_ptr(), o["clip"].data_ptr())
    status = [d.status(s) for s in range(S)]
    call = lambda i, v, nv, p, r, flags: d.L.dspi_process_patched(d.h, i, src.ctypes.data, v.ctypes.data, nv, p.ctypes.data, 1, F, C.byref(out), None, r, flags)
    err = lambda: d.L.dspi_last_error(d.h).decode()
    good = np.stack([a.wire_view_of(t_wire.data_ptr(), F), a.wire_view_of(t_wire.data_ptr(), F, tiled=True)])
    off = good.copy(); off["wire"][1] += 8
    DEV = host.MEM_DEVICE | host.OUT_CLIP_FLAGS
    pi, pr = t_in.data_ptr(), t_rx.data_ptr()
    assert call(pi, good, 2, patches, pr, host.OUT_CLIP_FLAGS) == host.E_INVAL and "DSPI_MEM_DEVICE is required" in err()
    assert call(pi, off, 2, patches, pr, DEV) == host.E_INVAL and "aligned" in err()
    assert call(pi, good, 9, patches, pr, DEV) == host.E_INVAL and "n_views" in err()
    far = patches.copy(); far["line"][11] = 20
    assert call(pi, good, 2, far, pr, DEV) == host.E_INVAL and "no line" in err() and "stream 11" in err()
    assert call(None, good, 2, patches, pr, DEV) == host.E_INVAL and "needs `in`" in err()
    assert call(pi + 8, good, 2, patches, pr, DEV) == host.E_INVAL and "16-byte" in err()
    assert call(pi, good, 2, patches, pr + 2, DEV) == host.E_INVAL and "4-byte" in err()
    assert call(pi, good, 2, patches, None, DEV) == host.E_INVAL and "(rx)" in err()
    d.sync()
    assert t_rx.cpu().numpy().tobytes() == rx0.tobytes(), "a refused call wrote a record"
    pairs, sub, peaks, clip = down(o)
    assert (pairs == FILL).all() and (sub == FILL).all() and (peaks == 0x5A5A).all() and (clip == 0x5A5A).all(), "a refused call wrote output"
    assert [d.status(s) for s in range(S)] == status and d.spdif_block_pos() == 0
    # ... and the context still works: lines of 0x11 words are no subframes, and only the S/PDIF runs' and links' records are written
    assert call(pi, good, 2, patches, pr, DEV) == 0
    d.sync()
    rx = t_rx.cpu().numpy().view(RX)
    served = src != 16; served &= src != 24
    assert (rx["coding_errors"][:S][served] == 2 * F).all() and (rx["state"][:S][served] == 0).all() and (rx["held"][:S][served] == 77 + 2 * F).all()
    assert rx[:S][~served].tobytes() == rx0[:S][~served].tobytes() and rx[S].tobytes() == rx0[S].tobytes()
    d.close(); a.close()
