"""The meter bridge on the GPU (dspi_meters_update / dspi_meters_alarms / dspi_status_all / dspi_clear_clips_list, include/dspi.h): every word is
compared with the model of tests/meters_model.py fed what the ORACLE computes for each stream — its per-packet peaks, its sticky clip flags,
its status block — never what the library itself wrote.

Shapes: a float (firmware contract) context of 130 streams — one full row of 128 and a ragged one — and a Q28 context of 70 (rows of 64).
Every stream has an input of its own: packets of 48 frames whose level changes per packet (burst, silence, a ramp over the call, a random
level) at a per-stream amplitude, under a +6 dB preamp, so that loud streams clip.  14 warm-up packets carry every device past its power-on
mute; the calls under test are 7 packets each.  The update kernel stages STAGE = 64 packets in LDS at once (dspi_meters.h
kMeterStagePackets): the long call runs 5 * 64 + 1 = 321 one-frame packets, then 64 + 1 = 65 more."""
import struct

import numpy as np
import pytest

import meters_model as M
from conftest import has_gpu
from orclib import Oracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B, NB, WARM, CALLS = 48000, 48, 7, 14, 3
STAGE = 64
HOLD, DECAY = 3, 30000
PREAMP_DB = 6.0
CASES = [(1, True, 130), (0, False, 70)]      # flavour, float contract, streams
IDS = ["f32fma-130", "q28-70"]


@pytest.fixture(scope="module", autouse=True)
def feature():
    assert hasattr(host.lib(), "dspi_meters_update"), "libdspi_mi355x has no dspi_meters_update"


def amplitude(rng):
    return 0.03 + 0.97 * rng.random() ** 3      # most streams quiet, some at full scale


def stream_input(seed, n_packets, block_len, quiet_from=None):
    """int16 [n_packets * block_len][2]: a per-stream amplitude, a per-packet level; quiet_from: from that packet on, silence"""
    rng = np.random.default_rng(seed)
    amp = amplitude(rng)
    F = n_packets * block_len
    t = np.arange(F)
    g = np.zeros(n_packets)
    for k in range(n_packets):
        kind = rng.integers(0, 4)
        g[k] = (1.0, 0.0, (k % NB + 1) / NB, rng.uniform(0.05, 0.6))[kind]
    if quiet_from is not None: g[quiet_from:] = 0.0
    g = np.repeat(g, block_len)
    x = np.stack([g * np.sin(2 * np.pi * 997 * t / FS), g * np.sin(2 * np.pi * 1501 * t / FS + 1)], axis=1)
    return np.clip(np.round(x * amp * 32767), -32768, 32767).astype(np.int16)


def new_oracle(flavor, fma):
    o = Oracle(flavor, detmath=True, fma=fma)
    o.set_rate(FS); o.set_volume(0); assert o.load_bulk(WL.full_chain_blob(flavor)) == 0
    assert o.vendor_set(W.REQ["SET_PREAMP"], 0, struct.pack("<f", PREAMP_DB)) == 0
    return o


def new_context(flavor, fma, S):
    d = Dspi(flavor, S, device=0, fma=fma)
    d.set_rate(FS); d.set_volume(0); assert d.load_bulk(WL.full_chain_blob(flavor)) == 0
    assert d.vendor_set(W.REQ["SET_PREAMP"], 0, struct.pack("<f", PREAMP_DB)) == 0
    return d


_REF = {}


def reference(flavor, fma, S):
    """Computed once per shape, shared, never changed.  pcm int16 [S][(WARM + CALLS * NB) * B][2]; per stream the oracle's peaks of every packet
    behind the warm-up [S][CALLS * NB][C], its clip flags and status block after the warm-up and after every call, its pair words of call 1
    (the second call under test); and the same for a device whose clip flags were cleared behind call 0: clip flags and status after call 1."""
    key = (flavor, fma, S)
    if key in _REF: return _REF[key]
    n = WARM + CALLS * NB
    # (every third stream falls silent in the warm-up: its tail — the chain looks ahead and delays — ends inside call 0, and what it clipped until then it does not clip again)
    pcm = np.stack([stream_input(1000 * flavor + s, n, B, quiet_from=WARM - 6 if s % 3 == 0 else None) for s in range(S)])
    o = new_oracle(flavor, fma); Cn, P = o.C, o.P; o.close()
    r = dict(pcm=pcm, peaks=np.zeros((S, CALLS * NB, Cn), dtype=np.uint16), clip=np.zeros((S, CALLS + 1), dtype=np.uint16), status=[[None] * (CALLS + 1) for _ in range(S)],
             pairs1=np.zeros((S, P, NB * B, 2), dtype=np.int32), clip1_cleared=np.zeros(S, dtype=np.uint16), status1_cleared=[None] * S)
    for s in range(S):
        for cleared in (False, True):
            o = new_oracle(flavor, fma)
            _, _, _, clip = o.process(pcm[s, :WARM * B], WARM, B)
            if not cleared: r["clip"][s, 0], r["status"][s][0] = clip, o.status()
            for c in range(2 if cleared else CALLS):
                lo = (WARM + c * NB) * B
                pairs, _, pk, clip = o.process(pcm[s, lo:lo + NB * B], NB, B)
                if cleared:
                    if c == 0: assert o.vendor_get(W.REQ["CLEAR_CLIPS"], 0, 2) == struct.pack("<H", r["clip"][s, 1])
                    else: r["clip1_cleared"][s], r["status1_cleared"][s] = clip, o.status()
                else:
                    r["peaks"][s, c * NB:(c + 1) * NB], r["clip"][s, c + 1], r["status"][s][c + 1] = pk, clip, o.status()
                    if c == 1: r["pairs1"][s] = pairs
            o.close()
    r["peaks"].setflags(write=False); r["clip"].setflags(write=False); pcm.setflags(write=False)
    _REF[key] = r
    return r


def call_pcm(ref, c):
    lo = (WARM + c * NB) * B
    return np.ascontiguousarray(ref["pcm"][:, lo:lo + NB * B])


def warmed(flavor, fma, S, ref):
    """a context behind its warm-up packets"""
    d = new_context(flavor, fma, S)
    d.process_host(np.ascontiguousarray(ref["pcm"][:, :WARM * B]), WARM, B, want_pairs=False, want_sub=False)
    return d


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else np.int32 if a.dtype == np.uint32 else a.dtype)).to(torch.device("cuda", 0))


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---- update ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,fma,S", CASES, ids=IDS)
@pytest.mark.parametrize("mem", ("device", "host"))
def test_update_follows_every_call(flavor, fma, S, mem):
    """three calls of 7 packets, each followed by the update on the same stream with no dspi_sync in between; after each, the words are the
    model's over the oracle's peaks"""
    import torch
    ref = reference(flavor, fma, S)
    d = warmed(flavor, fma, S, ref)
    want = np.zeros((S, d.C), dtype=np.uint32)
    steps = []
    if mem == "device":
        t_meters = on_device(want)
        t_peaks = torch.zeros((S, NB, d.C), dtype=torch.int16, device=t_meters.device)
        t_pcm = [on_device(call_pcm(ref, c)) for c in range(CALLS)]
        torch.cuda.synchronize()
    else: meters = want.copy()
    for c in range(CALLS):
        if mem == "device":
            d.process_device(t_pcm[c].data_ptr(), NB, B, peaks_ptr=t_peaks.data_ptr())
            d.meters_update_device(t_peaks.data_ptr(), NB, t_meters.data_ptr(), HOLD, DECAY)
            d.sync()
            got = back(t_meters, np.uint32).copy()
        else:
            _, _, peaks = d.process_host(call_pcm(ref, c), NB, B, want_pairs=False, want_sub=False)
            got = d.meters_update_host(peaks, meters, HOLD, DECAY).copy()
        want = M.update(want, ref["peaks"][:, c * NB:(c + 1) * NB], HOLD, DECAY)
        assert np.array_equal(got, want), (mem, c, np.argwhere(got != want)[:4])
        steps.append(want)
    # the input does what it was made for: holds running, holds run out and decayed levels, inside a call and across calls
    level, count = steps[-1] & 0xffff, steps[-1] >> 16
    running_max = ref["peaks"].max(axis=1)
    assert (count > 0).any() and (count == 0).any() and ((level < running_max) & (level > ref["peaks"][:, -1])).any()
    assert not np.array_equal(steps[0], steps[1]) and not np.array_equal(steps[1], steps[2])
    d.close()


@pytest.mark.parametrize("flavor,fma,S", [(1, True, 3), (1, True, 130), (0, False, 70)], ids=["f32fma-3", "f32fma-130", "q28-70"])
def test_a_long_call(flavor, fma, S):
    """one-frame packets: 5 * STAGE + 1 = 321 of them (the kernel's chunks, the last of one packet), then STAGE + 1 = 65 on the state that leaves"""
    import torch
    n_all = 5 * STAGE + 1 + STAGE + 1
    assert 5 * STAGE + 1 >= 300
    pcm = np.stack([stream_input(77 + s, n_all + 600, 1) for s in range(S)])      # (600 one-frame packets of warm-up: the power-on mute)
    d = new_context(flavor, fma, S)
    d.process_host(np.ascontiguousarray(pcm[:, :600]), 600, 1, want_pairs=False, want_sub=False)
    peaks = np.zeros((S, n_all, d.C), dtype=np.uint16)
    for s in range(S):
        o = new_oracle(flavor, fma)
        o.process(pcm[s, :600], 600, 1)
        peaks[s] = o.process(pcm[s, 600:], n_all, 1)[2]
        o.close()
    assert peaks.any()
    rng = np.random.default_rng(S)
    want = (rng.integers(0, 3000, (S, d.C)).astype(np.uint32) | rng.integers(0, 5, (S, d.C)).astype(np.uint32) << 16).astype(np.uint32)
    t_meters = on_device(want)
    lo = 600
    for K in (5 * STAGE + 1, STAGE + 1):
        t_pcm = on_device(np.ascontiguousarray(pcm[:, lo:lo + K]))
        t_peaks = torch.zeros((S, K, d.C), dtype=torch.int16, device=t_meters.device)
        torch.cuda.synchronize()
        d.process_device(t_pcm.data_ptr(), K, 1, peaks_ptr=t_peaks.data_ptr())
        d.meters_update_device(t_peaks.data_ptr(), K, t_meters.data_ptr(), 20, 32000)
        d.sync()
        want = M.update(want, peaks[:, lo - 600:lo - 600 + K], 20, 32000)
        got = back(t_meters, np.uint32)
        assert np.array_equal(got, want), (K, np.argwhere(got != want)[:4])
        lo += K
    d.close()


# ---- pauses, alarms, status blocks: one state per shape, read only ----------------------------------------------------------------------------
def paused_set(d):
    R = d.tile_streams()
    return [(1, 1), (R - 3, 4), (d.n_streams - 1, 1)]      # stream 1, a run across the first row boundary, the last stream


def paused_run(flavor, fma, S):
    """the warm-up, the pauses, then calls 0 and 1 on device buffers, each with its update, over meters prefilled with a pattern"""
    import torch
    ref = reference(flavor, fma, S)
    d = warmed(flavor, fma, S, ref)
    pauses = paused_set(d)
    for first, count in pauses: d.pause_streams(first, count)
    active = d.streams_paused() == 0
    prefill = (0x00050000 + 9000 + 23 * np.arange(S * d.C, dtype=np.uint32).reshape(S, d.C)).astype(np.uint32)
    t_meters = on_device(prefill)
    t_peaks = torch.full((S, NB, d.C), 0x5a5a, dtype=torch.int16, device=t_meters.device)
    want = prefill
    for c in range(2):
        t_pcm = on_device(call_pcm(ref, c))
        torch.cuda.synchronize()
        d.process_device(t_pcm.data_ptr(), NB, B, peaks_ptr=t_peaks.data_ptr())
        d.meters_update_device(t_peaks.data_ptr(), NB, t_meters.data_ptr(), HOLD, DECAY)
        d.sync()
        want = M.update(want, ref["peaks"][:, c * NB:(c + 1) * NB], HOLD, DECAY, active)
    # a paused stream took the warm-up only: its clip flags and status are those behind it
    clip = np.where(active, ref["clip"][:, 2], ref["clip"][:, 0]).astype(np.uint16)
    status = [ref["status"][s][2 if active[s] else 0] for s in range(S)]
    return dict(d=d, ref=ref, active=active, prefill=prefill, t_meters=t_meters, want=want, clip=clip, status=status)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def state(request):
    st = paused_run(*request.param)
    yield st
    st["d"].close()


def alarm_level(st):
    """the level of the alarm tests: the median of the streams' loudest meter, so that about half of them are at or above it"""
    return int(np.median((st["want"] & 0xffff).max(axis=1)))


def test_paused_streams_keep_their_words(state):
    got = back(state["t_meters"], np.uint32)
    active, S = state["active"], len(state["active"])
    assert (~active).sum() == 6 and not active[1] and not active[S - 1] and not active[state["d"].tile_streams() - 1] and not active[state["d"].tile_streams()]
    assert np.array_equal(got[~active], state["prefill"][~active]), "a paused stream's words were written"
    assert np.array_equal(got, state["want"]), np.argwhere(got != state["want"])[:4]
    assert not np.array_equal(got[active], state["prefill"][active])


def test_alarms_on_the_device_and_on_the_host(state):
    import torch
    d, S = state["d"], len(state["active"])
    level = alarm_level(state)
    ws, wi, wt = M.alarms(state["want"], state["clip"], level, S)
    # the condition the test was built for: between a quarter and three quarters of the streams, at least one of them by a clip bit, and a
    # paused stream among them
    assert S / 4 <= wt <= 3 * S / 4 and (state["clip"] != 0).any() and (wi >> 16).any() and (~state["active"])[ws].any(), (wt, S)
    t_meters = state["t_meters"]
    for cap in (wt // 2, wt, wt + 9):
        k = min(cap, wt)
        streams, info, total = d.meters_alarms_host(back(t_meters, np.uint32), level, cap)
        assert total == wt and streams.tolist() == ws[:k].tolist() and info.tolist() == wi[:k].tolist(), ("host", cap)
        t_streams = torch.full((cap,), -1, dtype=torch.int32, device=t_meters.device); t_info = torch.full((cap,), -1, dtype=torch.int32, device=t_meters.device)
        t_total = torch.full((1,), -1, dtype=torch.int32, device=t_meters.device)
        torch.cuda.synchronize()
        d.meters_alarms_device(t_meters.data_ptr(), level, t_streams.data_ptr(), t_info.data_ptr(), cap, t_total.data_ptr())
        d.sync()
        gs, gi = back(t_streams, np.uint32), back(t_info, np.uint32)
        assert int(back(t_total, np.uint32)[0]) == wt and gs[:k].tolist() == ws[:k].tolist() and gi[:k].tolist() == wi[:k].tolist(), ("device", cap)
        assert (gs[k:] == 0xffffffff).all() and (gi[k:] == 0xffffffff).all(), "nothing behind the list is written"
    # meters == NULL: the clipping streams alone, on either path; no info
    cs, ci, ct = M.alarms(None, state["clip"], 0, S)
    streams, info, total = d.meters_alarms_host(None, 12345)
    assert 0 < ct < wt and total == ct and streams.tolist() == cs.tolist() and info.tolist() == ci.tolist()
    t_streams = torch.full((S,), -1, dtype=torch.int32, device=t_meters.device); t_total = torch.full((1,), -1, dtype=torch.int32, device=t_meters.device)
    torch.cuda.synchronize()
    d.meters_alarms_device(0, 0, t_streams.data_ptr(), 0, S, t_total.data_ptr())
    d.sync()
    assert int(back(t_total, np.uint32)[0]) == ct and back(t_streams, np.uint32)[:ct].tolist() == cs.tolist()


def test_status_all_equals_get_status(state):
    import torch
    d, S = state["d"], len(state["active"])
    n = 2 * d.C + 4
    each = [d.status(s) for s in range(S)]
    assert each == state["status"], "dspi_get_status against the oracle, active and paused"
    assert any(b[-2:] != b"\0\0" for b in each) and any(b[:2] != b"\0\0" for b in each)
    host_blocks = d.status_all()
    assert [host_blocks[s].tobytes() for s in range(S)] == each
    part = d.status_all(S - 7, 7)
    assert [part[i].tobytes() for i in range(7)] == each[S - 7:]
    t_buf = torch.full((S * n + 1,), 0x5a, dtype=torch.uint8, device=state["t_meters"].device)
    torch.cuda.synchronize()
    assert d.status_all_device(t_buf.data_ptr(), S * n) == S
    assert d.status_all_device(t_buf.data_ptr() + 3 * n + 1, 5 * n, first=2, count=5) == 5      # (an odd address, over blocks 3..7 shifted by one byte)
    d.sync()
    got = t_buf.cpu().numpy()
    assert got[:3 * n].tobytes() == b"".join(each[:3]) and got[3 * n] == each[3][0] and got[3 * n + 1:8 * n + 1].tobytes() == b"".join(each[2:7])
    assert got[8 * n + 1:S * n].tobytes() == b"".join(each)[8 * n + 1:] and got[S * n] == 0x5a


# ---- the clear list (a state of its own: it changes the context) --------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor,fma,S", CASES, ids=IDS)
def test_clear_clips_list(flavor, fma, S):
    """the list an alarms call gave (the lower half of the alarmed streams) is cleared; those report 0, every other stream — their row neighbours
    among them — keeps its bits, and the next launch's pair words, peaks and clip flags are the oracle's after the same clears"""
    import torch
    ref = reference(flavor, fma, S)
    d = warmed(flavor, fma, S, ref)
    clip0 = ref["clip"][:, 1]      # behind call 0
    t_pcm = [on_device(call_pcm(ref, c)) for c in range(2)]
    t_peaks = torch.zeros((S, NB, d.C), dtype=torch.int16, device=t_pcm[0].device); t_pairs = torch.zeros((S, d.P, NB * B, 2), dtype=torch.int32, device=t_pcm[0].device)
    t_clip = torch.zeros(S, dtype=torch.int16, device=t_pcm[0].device)
    torch.cuda.synchronize()
    d.process_device(t_pcm[0].data_ptr(), NB, B, peaks_ptr=t_peaks.data_ptr())
    n_clipping = int((clip0 != 0).sum())
    assert n_clipping >= 4
    streams, info, total = d.meters_alarms_host(None, 0, n_clipping // 2)      # clip-only alarms: the lower half of them
    assert total == n_clipping and streams.tolist() == np.flatnonzero(clip0)[:n_clipping // 2].tolist() and (info >> 16).tolist() == clip0[streams].tolist()
    listed = np.zeros(S, dtype=bool); listed[streams] = True
    R = d.tile_streams()
    assert (clip0[~listed] != 0).any() and any((clip0[~listed & (np.arange(S) // R == s // R)] != 0).any() for s in streams), "a stream that keeps its bits shares a row with a cleared one"
    assert d.clear_clips_list(np.concatenate([streams[::-1], streams[:2]])) == len(streams) + 2      # (any order, duplicates)
    want = np.where(listed, 0, clip0).astype(np.uint16)
    for s in range(S): assert d.status(s)[-2:] == struct.pack("<H", want[s]), s
    blocks = d.status_all()
    assert [int(blocks[s, -2]) | int(blocks[s, -1]) << 8 for s in range(S)] == want.tolist()
    assert d.meters_alarms_host(None, 0)[0].tolist() == np.flatnonzero(want).tolist()
    # the following launch
    d.process_device(t_pcm[1].data_ptr(), NB, B, pairs_ptr=t_pairs.data_ptr(), peaks_ptr=t_peaks.data_ptr(), clip_ptr=t_clip.data_ptr())
    d.sync()
    after = np.where(listed, ref["clip1_cleared"], ref["clip"][:, 2]).astype(np.uint16)
    assert np.array_equal(back(t_clip, np.uint16), after), np.argwhere(back(t_clip, np.uint16) != after)[:4]
    assert np.array_equal(back(t_peaks, np.uint16), ref["peaks"][:, NB:2 * NB]) and np.array_equal(t_pairs.cpu().numpy(), ref["pairs1"])
    for s in range(S): assert d.status(s) == (ref["status1_cleared"][s] if listed[s] else ref["status"][s][2]), s
    assert (ref["clip1_cleared"][listed] != ref["clip"][listed, 2]).any(), "the clear shows in the next launch's flags"
    # an entry past the context clears nothing
    bad = np.array([int(np.flatnonzero(after)[0]), S], dtype=np.uint32)
    assert d.L.dspi_clear_clips_list(d.h, bad.ctypes.data, 2) == host.E_INVAL
    assert d.meters_alarms_host(None, 0)[0].tolist() == np.flatnonzero(after).tolist()
    d.close()
