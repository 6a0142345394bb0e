"""GPU: the MR-STFT distances (csrc/mrstft.hip: L/R, sum / difference, mel, each plain and prefiltered) and the waveform distances
(csrc/waveform.hip: esr, dc, snr, sisdr, logcosh) give, bit for bit, the losses and target tables recorded in
tests/golden/audio_distance_bits.json with the library of the commit before their shared pieces -- the slot rule, the folded peak,
the FIR run, the tile tree, the host checks of a loss call -- moved into csrc/audio_distance.h.  A shared function performs the
operations of the code it replaced, in their order: the same fmaf operands in the filter's chains, the same order of the float64
adds in the tree.  So nothing may move by an ulp, and the NaN of a candidate whose slot names no target stays where it was.

The fixture is re-recorded from the commit BEFORE a change to those files (tests/golden/make_audio_distance_bits.py says how), never
from the code under test; a ROCm update is a reason to re-record as well.

Cases and runner: tests/golden/make_audio_distance_bits.py.  No case is skipped."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_audio_distance_bits", os.path.join(ROOT, "tests", "golden", "make_audio_distance_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_case_table(recorded):
    """(no GPU) the recorded file is the case table's -- every id once, every array of a case -- names the library and the commit it
    was recorded from, and the table is the coverage the kernels need"""
    assert recorded["commit"] and recorded["library"].endswith(".so")
    got = recorded["cases"]
    assert sorted(got) == sorted(gen.case_id(c) for c in CASES)
    for c in CASES:
        assert sorted(got[gen.case_id(c)]) == sorted(gen.arrays_of(c)), gen.case_id(c)
    mr = [c for c in CASES if c["family"] == "mrstft"]
    wf = [c for c in CASES if c["family"] == "waveform"]
    plain = {(c["form"], c["source"]) for c in mr if c["taps"] is None}
    for form in gen.FORMS:
        assert {(form, t) for t in gen.TAPS} <= {(c["form"], c["taps"]) for c in mr}                    # every tap set: tails 1 and 3, 0 .. 63 blocks
        for pre in (None, "aw"):                                                                        # a slot list and a bad slot
            assert {(1, 2, 0), (1, 7, 0)} <= {c["slots"] for c in mr if c["form"] == form and c["taps"] == pre and c["slots"]}
        if form != "sum-diff":
            assert {(form, s) for s in gen.MR_INPUTS} <= plain
    import mrstft_sd_cases as SDC
    assert {("sum-diff", name) for name, *_ in SDC.cases()} <= plain
    assert {c["taps"] for c in mr if c["res"] == gen.WIDE_HOP} == {None, "aw"}
    assert any(c["source"].endswith("peak-folded-2049") and c["taps"] == "aw" for c in mr)
    assert {(t, n) for t in gen.WF_TAPS for n in gen.WF_LENGTHS} <= {(c["taps"], c["n"]) for c in wf}
    for key in ("taps", "n"):   # every channel count with every tap set and with every length
        assert {(c[key], c["channels"]) for c in wf} >= {(v, ch) for v in (gen.WF_TAPS if key == "taps" else gen.WF_LENGTHS) for ch in (1, 2, 3)}
    assert any(c["fold"] for c in wf) and {(1, 2, 0), (1, 7, 0)} <= {c["slots"] for c in wf if c["slots"]}


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[gen.case_id(c) for c in CASES])
def test_bits_are_the_recorded_ones(c, recorded):
    import torch
    assert torch.cuda.is_available()
    got, want = gen.run_case(c), recorded["cases"][gen.case_id(c)]
    for name in gen.arrays_of(c):
        print(f"{gen.case_id(c)} {name}: {got[name][:16]} (recorded {want[name][:16]})")
    bad = [name for name in gen.arrays_of(c) if got[name] != want[name]]
    assert not bad, f"{bad} differ from the bits recorded with {recorded['library']} of {recorded['commit']}"
