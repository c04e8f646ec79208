"""The context's device memory on the GPU (dspi_amd/csrc/dspi_devmem.h under dspi_capi.cpp): a scratch buffer that grows while the call before
it may still be running, every lazily allocated buffer once in one context's life and then its release, and the image table that grows with
its images in it.  Every expectation is the oracle's, per stream: its own Oracle(detmath=True) (and PdmOracle) fed the same packets, the
S/PDIF subframes orclib.spdif_encode of its pair words, the I2S words orclib.i2s_frames.  A stream that changes its slot takes its oracle with
it; a stream that is copied (import, migration) gets an oracle that replays the original's history.  Every comparison is for equality.

Shapes: one full row and one stream (129 float streams, 65 Q28 streams), 48-frame packets where the case says nothing else."""
import struct

import numpy as np
import pytest

import orclib
from conftest import has_gpu
from dspi_amd import wire as W, workloads as WL
from test_gpu_pdm_out import sub_setup
from test_gpu_snapshot import context, fid, oracle, packets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FLAVORS = (W.F32_FMA, 0)
FS, B = 48000, 48
FILL = 0x5A5A5A5A
R = W.REQ


def streams_of(flavor):
    return (128 if int(flavor) else 64) + 1


class Stream:
    """one device's oracles, and what happened to them so far (replayed into a copy)"""

    def __init__(self, flavor, blob):
        self.flavor, self.blob, self.log = flavor, blob, []
        self.o = oracle(flavor, FS, blob, setup=lambda o: sub_setup(o, flavor))
        self.pdm, self.running = orclib.PdmOracle(), False

    def request(self, req, wvalue, payload):
        self.log.append(("request", req, wvalue, payload))
        self.o.vendor_set(req, wvalue, payload)

    def output_type(self, pair, kind):
        self.log.append(("output_type", pair, kind))
        assert self.o.vendor_get(R["SET_OUTPUT_TYPE"], pair | (kind << 8), 1) is not None

    def process(self, row, n, block_len, depth=16):
        self.log.append(("process", row, n, block_len, depth))
        return self.o.process(row, n, block_len, depth)[:3]

    def modulate(self, sub):
        self.log.append(("modulate", sub))
        if not self.running: self.pdm.restart(); self.running = True
        return self.pdm.run(sub)

    def copy(self):
        c = Stream(self.flavor, self.blob)
        for what, *args in self.log: getattr(c, what)(*args)
        return c


def assert_outputs(models, rows, got, n, block_len, what, depths=None, skip=(), spdif_pos=None):
    """(pairs, sub, peaks) of one call, every stream against its oracle; spdif_pos: `pairs` holds subframes from that block position.
    Returns the oracles' sub words."""
    pairs, sub, peaks = got
    subs = {}
    for s, m in enumerate(models):
        if s in skip: continue
        rp, rs, rk = m.process(rows[s], n, block_len, 16 if depths is None else int(depths[s]))
        if spdif_pos is not None: rp = np.stack([orclib.spdif_encode(rp[p], spdif_pos, FS)[0] for p in range(rp.shape[0])])
        if pairs is not None: assert np.array_equal(rp, pairs[s]), f"{what}: stream {s}: pair words differ from the oracle's"
        if sub is not None: assert np.array_equal(rs, sub[s]), f"{what}: stream {s}: sub words differ from the oracle's"
        if peaks is not None: assert np.array_equal(rk, peaks[s]), f"{what}: stream {s}: peaks differ from the oracle's"
        subs[s] = rs
    return subs


def assert_words(models, subs, words, what):
    for s, rs in subs.items():
        assert np.array_equal(models[s].modulate(rs), words[s]), f"{what}: stream {s}: PDM words differ from the oracle's"


class DeviceCall:
    """one call's device buffers, made (and waited for) before anything is launched"""

    def __init__(self, x, kind, buf, n, block_len):
        import torch
        dev, S, F = torch.device("cuda", 0), x.n_streams, n * block_len
        self.kind, self.n, self.block_len = kind, n, block_len
        self.pcm = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
        self.pairs = torch.full((S, x.P, F, 4 if kind == "spdif" else 2), FILL, dtype=torch.int32, device=dev)
        self.sub = torch.full((S, F), FILL, dtype=torch.int32, device=dev)
        self.peaks = torch.zeros((S, n, x.C), dtype=torch.int16, device=dev)
        self.words = torch.full((S, F, 8), FILL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def launch(self, x, depths=None):
        p = dict(pairs_ptr=self.pairs.data_ptr(), peaks_ptr=self.peaks.data_ptr())
        if self.kind == "pdm": x.process_pdm_device(self.pcm.data_ptr(), self.n, self.block_len, self.words.data_ptr(), **p)      # no out->sub: the library's scratch
        elif self.kind == "mixed": x.process_mixed_device(self.pcm.data_ptr(), depths, self.n, self.block_len, sub_ptr=self.sub.data_ptr(), **p)
        else: x.process_device(self.pcm.data_ptr(), self.n, self.block_len, 16, sub_ptr=self.sub.data_ptr(), spdif=self.kind == "spdif", **p)

    def outputs(self):
        pairs = self.pairs.cpu().numpy()
        return (pairs.view(np.uint32) if self.kind == "spdif" else pairs, None if self.kind == "pdm" else self.sub.cpu().numpy(), self.peaks.cpu().numpy().view(np.uint16))


def mixed_rows(p16, p24, depths, block_len, p0, p1):
    """every stream's packets [p0, p1) at its own depth, and the call's flat buffer"""
    rows = [packets(p16[s], 16, block_len, p0, p1) if depths[s] == 16 else packets(p24[s], 24, block_len, p0, p1) for s in range(len(depths))]
    return rows, np.concatenate([np.ascontiguousarray(r).reshape(-1).view(np.uint8) for r in rows])


# ---- 1. growth under flight ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("spdif", "pdm", "mixed"))
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_growth_under_flight(flavor, kind):
    """device buffers, 1 x 4 frames and then — with no synchronisation in between — 8 x 4 frames: the second call needs a larger scratch (the
    two-pass S/PDIF route's pair words; the sub words of a dspi_process_pdm call without out->sub; the widened input of a mixed call) while
    the first may still be running on the old one, which is freed under it.  Then dspi_sync; both calls' words are the oracle's."""
    S, BL, warm = streams_of(flavor), 4, 12
    blob = WL.full_chain_blob(int(flavor))
    x = context(flavor, S, FS, blob)
    sub_setup(x, flavor)
    models = [Stream(flavor, blob) for _ in range(S)]
    p16 = WL.synth_pcm16(S, warm * B + 9 * BL, FS)
    p24 = WL.pcm16_to_pcm24_bytes(p16)
    depths = np.where(np.arange(S) % 2 == 1, 24, 16).astype(np.uint8)
    # the power-on mute passes (512 samples), in calls small enough for the direct path: none of the three scratches exists afterwards
    for k in range(0, warm, 4):
        rows = packets(p16, 16, B, k, k + 4)
        got = x.process_pdm_host(rows, 4, B)
        assert_words(models, assert_outputs(models, rows, got[:3], 4, B, "warm-up"), got[3], "warm-up")
    assert x.direct_stats()["calls"] == warm // 4 and int(np.abs(got[0]).max()) > 0 and got[3].any()
    # with per-stream block positions every DSPI_OUT_SPDIF call takes the two-pass route
    if kind == "spdif": assert x.spdif_per_stream(1) is True
    tail16, tail24 = p16[:, warm * B:], p24[:, warm * B * 6:]
    calls = []
    for p0, n in ((0, 1), (1, 8)):
        rows, buf = mixed_rows(tail16, tail24, depths, BL, p0, p0 + n) if kind == "mixed" else (packets(tail16, 16, BL, p0, p0 + n), packets(tail16, 16, BL, p0, p0 + n))
        calls.append((rows, DeviceCall(x, kind, buf, n, BL)))
    for _, c in calls: c.launch(x, depths)      # back to back: nothing waits for the first call
    x.sync()
    pos = 0
    for k, (rows, c) in enumerate(calls):
        what = f"{kind}, call {k} ({c.n} x {BL} frames)"
        subs = assert_outputs(models, rows, c.outputs(), c.n, BL, what, depths=depths if kind == "mixed" else None, spdif_pos=pos if kind == "spdif" else None)
        if kind == "pdm": assert_words(models, subs, c.words.cpu().numpy().view(np.uint32), what)
        pos += c.n * BL
    x.close()


# ---- 2. every lazy buffer once, then destroy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_every_lazy_buffer_then_destroy(flavor):
    """one context of a row and a stream through every call that allocates something on first use: the three memory paths, the PDM words in
    the fade mode, a mixed call, a wire call with one I2S slot, an export and a realigning import, a move, a resize that reallocates, a
    migration into a second small context — each held to the oracle — and then both contexts are destroyed."""
    import torch
    S0 = streams_of(flavor)
    Rw = S0 - 1
    n_staged = 10 if int(flavor) else 30      # the smallest host call past the direct area's 2 MiB
    blob = WL.full_chain_blob(int(flavor))
    x = context(flavor, S0, FS, blob)
    sub_setup(x, flavor)
    models = [Stream(flavor, blob) for _ in range(S0)]
    total = n_staged + 12
    p16 = WL.synth_pcm16(2 * Rw + 3, total * B, FS)      # (the last two rows: the second context's residents)
    p24 = WL.pcm16_to_pcm24_bytes(p16)
    at = 0

    def take(n, S=None):
        nonlocal at
        rows = packets(p16[:S or x.n_streams], 16, B, at, at + n); at += n
        return rows

    # staged, direct, device
    rows = take(n_staged)
    assert x.n_streams * n_staged * B * (4 + 8 * x.P + 4) > 2 << 20
    assert_outputs(models, rows, x.process_host(rows, n_staged, B), n_staged, B, "staged")
    assert x.direct_stats()["calls"] == 0
    rows = take(1)
    assert_outputs(models, rows, x.process_host(rows, 1, B), 1, B, "direct")
    assert x.direct_stats()["calls"] == 1
    rows = take(1)
    c = DeviceCall(x, "plain", rows, 1, B); c.launch(x); x.sync()
    assert_outputs(models, rows, c.outputs(), 1, B, "device")
    # the PDM words, the fade mode on: nobody's sub goes off, so every stream's words are its plain modulator's
    assert x.pdm_fade(1) is True
    rows = take(1)
    got = x.process_pdm_host(rows, 1, B)
    assert_words(models, assert_outputs(models, rows, got[:3], 1, B, "pdm"), got[3], "pdm")
    assert got[3].any() and x.pdm_running().all()
    # 16- and 24-bit devices in one call, device buffers
    depths = np.where(np.arange(S0) % 3 == 0, 24, 16).astype(np.uint8)
    rows, buf = mixed_rows(p16, p24, depths, B, at, at + 1); at += 1
    c = DeviceCall(x, "mixed", buf, 1, B); c.launch(x, depths); x.sync()
    assert_outputs(models, rows, c.outputs(), 1, B, "mixed", depths=depths)
    # the wire layout, one I2S slot (stream 3, pair 0); the switch arms a mute, in the oracle too
    assert x.vendor_get(R["SET_OUTPUT_TYPE"], 0 | (1 << 8), 1, 3) == b"\x00"
    models[3].output_type(0, 1)
    rows = take(1)
    wire = x.process_wire_host(rows, 1, B, 16)
    for s, m in enumerate(models):
        rp, rs, rk = m.process(rows[s], 1, B)
        for p in range(x.P):
            if (s, p) == (3, 0):
                region = wire[0][s, p].reshape(-1)
                assert np.array_equal(region[:2 * B], orclib.i2s_frames(rp[p]).reshape(-1)) and not region[2 * B:].any(), "wire: the I2S slot"
            else: assert np.array_equal(wire[0][s, p], orclib.spdif_encode(rp[p], 0, FS)[0]), f"wire: stream {s} pair {p}: subframes differ from the oracle's"
        assert np.array_equal(rs, wire[1][s]) and np.array_equal(rk, wire[2][s]), f"wire: stream {s}"
    # stream 2 is copied into slot 7, realigned to its row
    head, state = x.export_streams(2, 1)
    assert x.import_streams(7, head, state, realign=True) == 1
    models[7] = models[2].copy()
    rows = take(1)
    assert_outputs(models, rows, x.process_host(rows, 1, B), 1, B, "after the import")
    # slots 1 and Rw (the partial row's stream) change places
    assert x.move_streams([(1, Rw), (Rw, 1)]) == 2
    models[1], models[Rw] = models[Rw], models[1]
    rows = take(1)
    assert_outputs(models, rows, x.process_host(rows, 1, B), 1, B, "after the move")
    # a third row: every persistent array is reallocated, the rows in use come over.  The new slots arrive paused and stay so.
    assert x.stream_capacity() == 2 * Rw
    assert x.resize_streams(2 * Rw + 1, paused=True) == 2 * Rw + 1 and x.stream_capacity() == 3 * Rw
    rows = take(1)
    got = x.process_host(rows, 1, B)
    assert_outputs(models, rows, got, 1, B, "after the resize")
    assert not got[0][S0:].any() and not got[1][S0:].any() and int(np.abs(got[0][:S0]).max()) > 0
    # stream 5 leaves for slot 1 of a second, small context
    y = context(flavor, 3, FS, blob)
    sub_setup(y, flavor)
    ymodels = [Stream(flavor, blob) for _ in range(3)]
    assert y.pdm_fade(1) is True
    y.pause_streams(1, 1)
    assert x.migrate_streams(y, [(5, 1)]) == 1
    ymodels[1] = models[5]
    rows = take(1)
    got = x.process_host(rows, 1, B)
    assert_outputs(models, rows, got, 1, B, "the source after the migration", skip={5})
    assert x.streams_paused(5, 1)[0] == 1 and not got[0][5].any()
    yrows = np.ascontiguousarray(np.stack([packets(p16[2 * Rw + 1], 16, B, at - 1, at), rows[5], packets(p16[2 * Rw + 2], 16, B, at - 1, at)]))
    got = y.process_pdm_host(yrows, 1, B)
    # (the arrival's modulator goes on running; the residents' start here)
    assert_words(ymodels, assert_outputs(ymodels, yrows, got[:3], 1, B, "the destination after the migration"), got[3], "the destination after the migration")
    assert ymodels[1].running and y.pdm_running().all()
    torch.cuda.synchronize()
    x.close(); y.close()


# ---- 3. the image table grows with its images in it ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS, ids=fid)
def test_image_table_growth_keeps_the_images(flavor):
    """the table holds the first commit's image and room for 8 more; ten streams get presets of their own, so the next commit grows it; then
    one more stream changes.  A small call: the untouched streams and the eleven changed ones are all their oracles'."""
    S = 12
    blob = WL.full_chain_blob(int(flavor))
    x = context(flavor, S, FS, blob)
    models = [Stream(flavor, blob) for _ in range(S)]
    sub_setup(x, flavor)      # (as Stream's oracles)
    p16 = WL.synth_pcm16(S, 14 * B, FS)
    assert_outputs(models, p16[:, :12 * B], x.process_host(p16[:, :12 * B], 12, B), 12, B, "the first commit")
    assert x.image_count() == 1
    for s in range(10):
        db = struct.pack("<f", -1.0 - s)
        x.vendor_set(R["SET_PREAMP"], 0, db, stream=s); models[s].request(R["SET_PREAMP"], 0, db)
    rows = packets(p16, 16, B, 12, 13)
    assert_outputs(models, rows, x.process_host(rows, 1, B), 1, B, "eleven images")
    assert x.image_count() == 11
    db = struct.pack("<f", 2.5)
    x.vendor_set(R["SET_PREAMP"], 0, db, stream=10); models[10].request(R["SET_PREAMP"], 0, db)
    rows = packets(p16, 16, B, 13, 14)
    got = x.process_host(rows, 1, B)
    assert_outputs(models, rows, got, 1, B, "one more stream")
    assert x.image_count() == 12 and int(np.abs(got[0][11]).max()) > 0
    x.close()
