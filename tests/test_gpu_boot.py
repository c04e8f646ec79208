"""Stream boots on the GPU (dspi_boot_streams, include/dspi.h): a listed slot becomes a device that has just been powered on, inside a
running context, and its neighbours do not notice.  Every audio comparison is with the oracle, one oracle per stream, never with another
run of the library: a booted slot's oracle is a FRESH one, built the way the slot was booted (erased flash, or the dump) and fed the
slot's packets from its packet 0 again with the requests a host makes after enumeration; every other stream's oracle is continuous.
BootSched below is test_gpu_pause.py's schedule record with that one addition.

    figures: none.  300 float streams (both contracts) / 200 Q28 streams: three rows, the last partial; 48 kHz, 48-frame packets, the full
    chain (delays and leveller on), at most 12 packets per stream."""
import ctypes as C
import struct

import numpy as np
import pytest

from conftest import has_gpu
from orclib import Oracle, PdmOracle
from dspi_amd import host, wire as W, workloads as WL
from dspi_amd.host import Dspi, DspiError
from test_boot_cpu import flash_cases
from test_gpu_snapshot import FLAVORS_WITH_KERNEL, VOL, as_input, check, context, fid, oracle
from test_gpu_realign import assert_rows_uniform
from test_gpu_pause import Sched, mixed_set, runs_of, _shape_blob
from test_gpu_move import move, streams_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no GPU")]

FS, B = 48000, 48


class BootSched(Sched):
    """Sched whose slots can be power-cycled: boot() drops the slot's record — it starts again at ITS packet 0, on the same input — and
    verify() gives such a slot a fresh oracle booted the same way."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.booted = {}                    # slot -> the dump it booted from (None: dspi_create's device)

    def fresh(self, dump):
        return Oracle(self.flavor, detmath=True, flash=dump)

    def boot(self, streams, dump=None, as_is=False, want=48):
        streams = [int(s) for s in streams]
        paused = self.d.streams_paused().astype(bool)
        assert self.d.boot_streams(streams, dump, as_is=as_is) == want
        o = self.fresh(dump); power_on = o.status(); o.close()
        assert not any(power_on[:2 * self.d.C]) and not any(power_on[-2:]), "a device that has just been powered on reports no peaks and no clips"
        for s in streams:
            self.booted[s] = dump
            self.parts[s] = []; self.hooks[s] = {}; self.pos[s] = 0; self.last_clip[s] = 0
            if paused[s]: self.frozen[s] = (power_on, 0)
            assert self.d.status(s) == power_on, f"booted stream {s}: status bytes are not the power-on ones"
        assert np.array_equal(self.d.streams_paused().astype(bool), paused), "activity belongs to the slot: a boot does not change it"

    def enumerate(self, streams, blob_on=()):
        """what a USB host does with a device that has arrived: rate and volume, and on some a whole parameter set"""
        for s in streams:
            self.request("set_rate", self.fs, stream=int(s)); self.request("set_volume", self.vol, stream=int(s))
        for s in blob_on: self.request("load_bulk", self.blob, stream=int(s))

    def verify(self, streams=None, what=""):
        for s in (range(self.d.n_streams) if streams is None else streams):
            o = self.fresh(self.booted[s]) if s in self.booted else oracle(self.flavor, self.fs, self.blob, self.vol)
            at = {p: (lambda o, rq=rq: [getattr(o, nm)(*a) for nm, a in rq]) for p, rq in self.hooks[s].items()}
            check(o, self.data[s], self.depth, self.B, self.parts[s], f"{what}{'booted ' if s in self.booted else ''}stream {s}", at=at)
            o.close()


def new_boot_sched(flavor, S, packets_total, blob=None, vol=VOL, statuses=True):
    blob = WL.full_chain_blob(flavor) if blob is None else blob
    data = as_input(WL.synth_pcm16(S, packets_total * B, FS), 16)
    return BootSched(context(flavor, S, FS, blob, vol), flavor, FS, blob, data, 16, B, vol, statuses)


def v2_dump(flavor):
    return flash_cases(flavor)[0]      # (dump, 4): a v2 directory whose default slot is 4; booting from it writes nothing and arms no mute


# ---- 1. power-on bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_power_on_bytes(flavor):
    """Every state slot, line word, ring word and PDM word of a booted stream is the word a freshly created context holds there, and no
    other column of the touched rows has changed: the exported records say so byte for byte."""
    S = streams_of(flavor)
    x = new_boot_sched(flavor, S, 6, statuses=False)
    d, R = x.d, x.d.tile_streams()
    sub = x.run(6)[1]
    d.pdm_host(sub)                                       # the modulator words are not power-on words any more
    before = d.export_streams(0, S)[1]
    booted = [10, 11, 40] + list(range(R, 2 * R)) + [S - 1]
    x.boot(booted, as_is=True)
    f = Dspi(flavor, 1, device=0)
    fresh = f.export_streams(0, 1)[1][0]
    f.close()
    after = d.export_streams(0, S)[1]
    assert not np.array_equal(before[10], fresh) and not np.array_equal(before[9], fresh)
    for s in booted: assert np.array_equal(after[s], fresh), f"booted stream {s}: {int((after[s] != fresh).sum())} words are not power-on words"
    for s in (9, 12, 2 * R): assert np.array_equal(after[s], before[s]), f"neighbour {s} was written"
    keep = np.ones(S, dtype=bool); keep[booted] = False
    assert np.array_equal(after[keep], before[keep]), "a column that was not listed was written"
    w, r = d.stream_positions(0, S)
    assert not w[booted].any() and not r[booted].any() and w[9] == 6 * B
    d.close()


# ---- 2. arrival mid-run, 7. on the latency layout -------------------------------------------------------------------------------------------
def arrival(x, plain, from_dump, blob_on=None):
    d, flavor = x.d, x.flavor
    dump, code = v2_dump(flavor)
    x.run(5)
    x.boot(plain)
    x.boot(from_dump, dump, want=code)
    assert_rows_uniform(d, "after the boots")
    w, r = d.stream_positions(0, d.n_streams)
    assert w[plain[0]] == 5 * B and r[plain[0]] == 5 * B, "a booted stream takes its row's residents' positions"
    x.enumerate(plain + from_dump, blob_on=(plain[0], from_dump[0]) if blob_on is None else blob_on)
    x.run(3); x.run(2)
    assert_rows_uniform(d, "after the continuation")
    for s in plain + from_dump: assert x.pos[s] == 5
    x.verify()


@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_arrival_mid_run(flavor):
    S = streams_of(flavor)
    x = new_boot_sched(flavor, S, 12)
    R = x.d.tile_streams()
    arrival(x, [10, 11, 40, R + 3], [2 * R + 1])
    x.d.close()


def test_arrival_on_the_latency_layout(monkeypatch):
    """a small context, which the library's size rule puts on the latency layout (the third shape: the full chain with the leveller)"""
    monkeypatch.delenv("DSPI_F32_LAYOUT", raising=False)
    flavor, S = W.F32_FMA, 40
    x = new_boot_sched(flavor, S, 12, blob=_shape_blob(flavor, 3), vol=-7 * 256)
    arrival(x, [10, 11, 25], [4], blob_on=(10, 11, 25, 4))      # (every arrival gets the context's preset: one structure, as the layout's workgroups want it)
    plan = x.d.launch_plan()
    assert plan["latency_layout"] > 0 and plan["packed_shared"] == plan["packed_per_lane_values"] == plan["packed_per_lane_values_and_bands"] == 0, plan
    x.d.close()


# ---- 3. into freed slots --------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_into_freed_slots(flavor):
    """the arrival recipe: compact one-way, boot the freed slots, set them up, resume"""
    S = streams_of(flavor)
    x = new_boot_sched(flavor, S, 12)
    d, R = x.d, x.d.tile_streams()
    dump, code = v2_dump(flavor)
    x.run(3)
    for first, count in runs_of(mixed_set(S, R)): x.pause(first, count)
    x.run(1)
    move(x, d.plan_compaction(one_way=True))
    free = np.flatnonzero(d.streams_paused())[:2].tolist()
    x.boot(free, dump, want=code)                        # (boot() checks: still paused, zero peaks and clips)
    x.run(1)                                             # they sit this one out
    for s in free: assert x.pos[s] == 0 and d.status(s) == x.frozen[s][0]
    x.enumerate(free)
    for s in free: x.resume(s, 1)
    w, r = d.stream_positions(0, S)                      # (the rows still hold the frozen copies of the one-way moves: only the ACTIVE streams share positions)
    active = ~d.streams_paused().astype(bool)
    for s in free:
        row = slice(s // R * R, min((s // R + 1) * R, S))
        assert active[s] and set(w[row][active[row]].tolist()) == {5 * B} and set(r[row][active[row]].tolist()) == {5 * B}, f"resumed arrival {s} does not stand on its row's positions"
    x.run(2); x.run(1)
    for s in free: assert x.pos[s] == 3
    x.resume(0, S)                                       # the frozen copies the one-way moves left behind go on as well
    x.run(2)
    x.verify()
    d.close()


# ---- 4. pending operations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_layouts
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_pending_operations(flavor):
    """A broadcast band change that resets a filter path and a broadcast preset-slot load (mute, zeroed lines) immediately before the boot,
    with no dspi_process in between: every other stream gets them, the booted streams do not — they left the object that carries them.  A
    preset-slot load addressed to a booted stream right after the boot lands on the new object and is applied at the next commit over the
    power-on state, as on a device that has just booted."""
    S = streams_of(flavor)
    x = new_boot_sched(flavor, S, 12)
    d, R = x.d, x.d.tile_streams()
    other = WL.full_chain_blob(flavor, max_delay_ms=3.0)
    other["preamp"]["preamp_db"][:] = (-6.0, -2.0)
    ref = oracle(flavor, FS, other); image = ref.save_slot(0); ref.close()
    band = (W.REQ["SET_EQ_PARAM"], 0, struct.pack("<BBBBfff", 0, 3, W.FILTER_LOWSHELF, 0, 300.0, 0.8, 3.0))
    x.run(3)
    x.request("vendor_set", *band)
    x.request("load_slot", image, -1)
    booted = [5, 6, R + 3]
    x.boot(booted)
    x.request("load_slot", image, -1, stream=5)
    x.enumerate(booted)
    x.run(2); x.run(2)
    assert d.image_count() == 3                          # the others', the booted pair's, stream 5's
    x.verify()
    d.close()


# ---- 5. images and plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", FLAVORS_WITH_KERNEL, ids=fid)
def test_images_and_plan(flavor):
    """a whole-context boot leaves one parameter object and, after the usual setup, the launch plan of a fresh context; twelve packets
    from power-on carry the first-boot mute (512 samples) and the beginning of the fade-in"""
    S = streams_of(flavor)
    x = new_boot_sched(flavor, S, 12, statuses=False)
    d, R = x.d, x.d.tile_streams()
    f = context(flavor, S, FS, x.blob)
    f.process_host(np.zeros((S, B, 2), dtype=np.int16), 1, B)
    fresh_plan = f.launch_plan()
    f.close()
    x.request("load_bulk", WL.full_chain_blob(flavor, max_delay_ms=3.0), stream=7)
    x.run(2)
    assert d.image_count() == 2
    x.boot(range(S))
    assert d.image_count() == 1
    x.request("set_rate", FS); x.request("set_volume", VOL); x.request("load_bulk", x.blob)
    x.run(1)
    assert d.launch_plan() == fresh_plan
    x.run(11)
    x.verify((0, R - 1, R, S - 1))
    x.boot([5, R + 5, 2 * R + 5])
    assert d.image_count() == 2
    d.close()


# ---- 6. PDM ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
@pytest.mark.parametrize("tiled", (False, True), ids=("stream-major", "tiled"))
def test_pdm(flavor, tiled):
    """dspi_pdm_modulate before and after a boot against one PdmOracle per stream: a booted stream's modulator starts again from power-on,
    its neighbours' continue"""
    S = 150 if int(flavor) else 100
    x = new_boot_sched(flavor, S, 8, statuses=False)
    d, R = x.d, x.d.tile_streams()
    nt = -(-S // R)
    pdm = [PdmOracle() for _ in range(S)]

    def modulate(sub):
        if tiled:
            t = np.zeros((nt * R, sub.shape[1]), dtype=np.int32); t[:S] = sub
            words = d.pdm_host(np.ascontiguousarray(t.reshape(nt, R, -1).transpose(0, 2, 1)), tiled=True)      # [tile][frame][8][R]
            words = words.transpose(0, 3, 1, 2).reshape(nt * R, sub.shape[1], 8)[:S]
        else: words = d.pdm_host(sub)
        for s in range(S): assert np.array_equal(pdm[s].run(sub[s]), words[s]), f"PDM words of stream {s}"

    modulate(x.run(2)[1])
    booted = [5, 6, R - 1, R, S - 1]
    x.boot(booted)
    for s in booted: pdm[s] = PdmOracle()
    x.enumerate(booted, blob_on=booted)
    modulate(x.run(2)[1]); modulate(x.run(2)[1])
    x.verify(sorted(set(booted) | {0, 4, 7, R - 2, R + 1, S - 2}))
    d.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", (W.F32_FMA, 0), ids=fid)
def test_refusals(flavor):
    S = 150
    x = new_boot_sched(flavor, S, 6, statuses=False)
    d = x.d
    dump, _ = v2_dump(flavor)
    x.run(2)
    x.pause(10, 20)
    paused, images = d.streams_paused().copy(), d.image_count()
    sel = C.c_int(-7)

    def boot(l, n=None, dump=None, length=None, flags=0):
        a = np.asarray([] if l is None else l, dtype=np.uint32)
        return d.L.dspi_boot_streams(d.h, a.ctypes.data if l is not None else None, len(a) if n is None else n, dump,
                                     (len(dump) if dump else 0) if length is None else length, flags, C.byref(sel))
    assert boot([1, 2], n=0) == host.E_INVAL
    assert boot(None, n=2) == host.E_INVAL
    assert boot([1, S]) == host.E_INVAL and boot([0xFFFFFFFF]) == host.E_INVAL
    assert boot([1, 12, 1]) == host.E_INVAL
    for flags in (0x2, 0x3, 0x100, 0x80000000): assert boot([1, 12], flags=flags) == host.E_INVAL, hex(flags)
    assert boot([1, 12], dump=dump, length=len(dump) - 1) == host.E_SHORT
    with pytest.raises(DspiError) as e: d.boot_streams([4, 4])
    assert e.value.code == host.E_INVAL
    assert sel.value == -7 and d.image_count() == images and np.array_equal(d.streams_paused(), paused)
    x.run(2)
    x.resume(0, S)
    x.run(2)
    x.verify(sorted({0, 1, 2, 4, 9, 10, 12, 29, 30, S - 1}))
    d.close()
