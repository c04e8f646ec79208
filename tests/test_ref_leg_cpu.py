"""The CPU half of the reference leg (tests/refleg.py).  The GPU parity tests hold the GPU's words to the reference's own object code
(oracle/_ref/libref_{f32,f32_fma,q28}.so) wherever the x86 build of it is a valid checker: where A, the restatement under the firmware's
saturating casts, equals X, the restatement under x86 casts.  Which streams those are is a property of presets and signals, not of the
GPU, so it is measured HERE, before anything runs on a GPU: this file replays the generators of the GPU tests — imported, never copied —
for their default parametrisation with the oracles alone (no context, no GPU) and asserts

  * X == R for every checked stream and step (refleg.Leg asserts it on every call), and
  * the share of checks that are held, per family of GPU tests.  A share below its condition means the leg has quietly stopped checking.

The conditions (the shares measured when the leg was written are in profiles/ref_leg.md):

  float fuzz presets, each contract     >= 85 % of the checked streams           Q28 fuzz presets     >= 50 %
  request sequences                     >= 60 % of stream-steps, all flavours together (a stream stays out after its first A != X)
  float test_full_chain, every other float scenario through compare(), the new float sequences: every checked stream
  Q28 chain without the leveller:       every checked stream

`pytest -s` prints every share.  Skipped where oracle/_ref is not built, as tests/test_oracle_vs_ref.py is."""
import inspect

import pytest

import refleg

pytestmark = pytest.mark.skipif(bool(refleg.missing_libs()), reason="oracle/_ref not built (needs the reference sources)")

from dspi_amd import wire as W
import test_gpu_fuzz as F
import test_gpu_parity as P

FLAVORS = {"float": 1, "fma": W.F32_FMA, "q28": 0}


def name_of(flavor) -> str:
    return "q28" if not int(flavor) else ("fma" if getattr(flavor, "fma", False) else "float")


def cases(fn):
    """the default parametrisation of a test function, from its own parametrize marks: a list of keyword dicts"""
    out = [{}]
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize": continue
        names = [n.strip() for n in m.args[0].split(",")]
        out = [{**kw, **dict(zip(names, v if len(names) > 1 else (v,)))} for kw in out for v in m.args[1]]
    return out


def replay_compare(flavor, fs, B, blocks, S, blob, vol=-20 * 256, depth=16, calls=2, check_streams=None, setup=None, first_stream=0):
    """test_gpu_parity.compare without the context: the same input, the same oracle run (with its reference leg) for the same streams"""
    data = P.compare_input(fs, B, blocks, S, depth, first_stream)
    per = blocks // calls
    for s in (check_streams if check_streams is not None else range(S)):
        P.oracle_run(flavor, fs, vol, blob, data[s], per * calls, B, depth, setup)


@pytest.fixture
def replay(monkeypatch):
    monkeypatch.setattr(P, "compare", replay_compare)
    return monkeypatch


def run(fn, monkeypatch, want=lambda flavor: True, **fixed):
    """every default case of the GPU test `fn` whose flavour `want` accepts; counted under "<fn> <flavour>"; returns those names"""
    names = []
    for kw in cases(fn):
        flavor = kw.get("flavor", fixed.get("flavor", 0 if "q28" in fn.__name__ else 1))
        if "fma" in kw: flavor = W.F32_FMA if kw["fma"] else 1
        if not want(flavor): continue
        if "monkeypatch" in inspect.signature(fn).parameters: kw["monkeypatch"] = monkeypatch
        name = f"{fn.__name__} {name_of(flavor)}"
        with refleg.scope(name): fn(**kw, **fixed)
        if name not in names: names.append(name)
    return names


def share(names, say=True):
    """(held, checks) over the scopes `names`, printed"""
    held = total = 0
    for n in names:
        h, l = refleg.shares().get(n, (0, 0))
        if say: print(f"reference leg: {n}: {h} / {h + l} held")
        held += h; total += h + l
    assert total > 0, names
    return held, total


def explain(names):
    return "; ".join(f"{t}, {lab}: saturating and x86 casts first differ in {where}" for t, lab, where in refleg.left_out() if t in names)


is_float = lambda flavor: bool(int(flavor))
is_q28 = lambda flavor: not int(flavor)


@pytest.mark.parametrize("which", sorted(FLAVORS))
def test_fuzz_presets_share(which, replay):
    held, total = share(run(F.test_random_presets, replay, lambda fl: name_of(fl) == which))
    need = 0.50 if which == "q28" else 0.85
    assert held >= need * total, f"{held} / {total} checked streams of test_random_presets ({which}) are held to the reference build; {need:.0%} asked"


def test_request_sequences_share():
    names = []
    for kw in cases(F.test_random_request_sequences):
        n = f"test_random_request_sequences {name_of(kw['flavor'])}"
        with refleg.scope(n): F.request_sequence(kw["flavor"], kw["seed"], None)
        if n not in names: names.append(n)
    held, total = share(names)
    assert held >= 0.60 * total, f"{held} / {total} stream-steps of test_random_request_sequences are held to the reference build; 60 % asked"


def test_per_stream_and_one_structure_fuzz():
    """X == R on the two fuzz tests that build their own oracles; their shares are recorded, no condition is set on them"""
    names = []
    for fn, body in ((F.test_random_preset_per_stream, F.preset_per_stream), (F.test_random_numbers_one_random_structure, F.numbers_one_structure)):
        for kw in cases(fn):
            n = f"{fn.__name__} {name_of(kw['flavor'])}"
            with refleg.scope(n): body(kw["flavor"], kw["seed"], gpu=False)
            if n not in names: names.append(n)
    share(names)


def test_float_full_chain_is_held(replay):
    names = run(P.test_full_chain, replay, is_float)
    held, total = share(names)
    assert held == total, f"test_full_chain: {held} / {total} held; {explain(names)}"


FLOAT_SCENARIOS = (P.test_config2_master_peq, P.test_ragged_packets_delay_edges, P.test_unusual_packet_lengths, P.test_long_run_wraps_delay_lines,
                   P.test_host_volume_sign_quirk_and_mute)


def test_every_other_float_scenario_is_held(replay):
    """every float scenario that goes through compare(), besides test_full_chain and the fuzz: every checked stream is held, or the
    scenario and the words in which a cast overflowed are named"""
    names = []
    for fn in FLOAT_SCENARIOS: names += run(fn, replay, is_float)
    for kw in cases(P.test_latency_layout_lines_of_disabled_outputs):      # (its compare() part: config 2's own preset)
        n = f"test_latency_layout_lines_of_disabled_outputs {name_of(kw['flavor'])}"
        with refleg.scope(n): P.config2_own_preset(kw["flavor"], kw["fs"], kw["B"], 10 if kw["B"] >= 44 else 60)
        if n not in names: names.append(n)
    held, total = share(names)
    assert held == total, f"{held} / {total} held; {explain(names)}"


def test_q28_scenarios(replay):
    """X == R on the Q28 scenarios; their shares are recorded: the limiter's cast (leveller.c:366-383) overflows on quiet samples in an x86
    build, so most streams of the Q28 full chain are left out"""
    names = run(P.test_full_chain, replay, is_q28)
    for fn in FLOAT_SCENARIOS + (P.test_q28_wave_layouts,): names += run(fn, replay, is_q28)
    share(names)


def test_q28_chain_without_leveller_is_held(replay):
    names = run(P.test_q28_chain_without_leveller_against_the_reference, replay)
    held, total = share(names)
    assert held == total, f"{held} / {total} held; {explain(names)}"


@pytest.mark.parametrize("which", sorted(FLAVORS))
def test_core1_eq_worker_mode_sequence(which):
    n = f"test_core1_eq_worker_mode {which}"
    with refleg.scope(n): P.core1_eq_worker_mode(FLAVORS[which], gpu=False)
    held, total = share([n])
    if which != "q28": assert held == total, f"{held} / {total} held; {explain([n])}"


@pytest.mark.parametrize("which", ("float", "fma"))
@pytest.mark.parametrize("case", ("audio", "minus_zero"))
def test_disabled_sub_line_sequences(which, case):
    n = f"test_latency_layout_disabled_sub_line_sequences {which}"
    before = refleg.shares().get(n, (0, 0))
    with refleg.scope(n): P.disabled_sub_line_sequence(FLAVORS[which], case, gpu=False)
    held, left = refleg.shares()[n]
    print(f"reference leg: {n} ({case}): {held - before[0]} / {held - before[0] + left - before[1]} held")
    assert left == 0, f"{left} checks left out; {explain([n])}"
