#!/usr/bin/env python
"""Records tests/golden/audio_distance_bits.json: per case one sha256 per array -- the float32 losses as bytes, and the first half
of the target table (MR-STFT: the FFT tables and magnitudes; waveform: the filtered rows) -- of the MR-STFT distances
(csrc/mrstft.hip: L/R, sum / difference and mel, plain and prefiltered) and of the waveform distances (csrc/waveform.hip: the five
kinds).  The two files share their slot rule, folded peak, FIR run, tile tree and host checks (csrc/audio_distance.h); how that
code is arranged may change, what it computes may not.  So the fixture is recorded with the library of the commit BEFORE a change
to either file or to the header, never with the code under test, and tests/test_gpu_audio_distance_bits.py (which takes its cases
and its runner from this file) holds the library after the change to the same bits:

    tools/build_rev_lib.sh <parent rev> parent
    STITO_LIB_PATH=st-ito_amd/st_ito/_lib/ab/libstito_hip_parent.so python tests/golden/make_audio_distance_bits.py --commit <parent rev>

A ROCm update (another compiler, another libm behind logf, sqrtf, sinh and log1p) is a reason to re-record too, again from the
commit before the change at hand.  --out FILE writes elsewhere (to compare two libraries' files).

Inputs: the seeded generators of tests/mrstft_cases.py, tests/mrstft_sd_cases.py and tests/waveform_ref.py.  The tables are zeroed
and refilled before they are hashed: the padding float between two resolutions' magnitudes is written by nobody."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "audio_distance_bits.json")
for _p in ("tests", "oracle", "st-ito_amd"):
    if os.path.join(ROOT, _p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, _p))

SR = 48000
FORMS = ("lr", "sum-diff", "mel")
TAPS = ("unit", "shift", "aw", "fir255", "fir31")   # waveform_ref.tap_sets(): [1]; [0, 0, 1]; 101 taps; 255 taps; 31 asymmetric taps
# the inputs of mrstft_cases.cases() by name: the fewest samples the framing takes; n % hop = 0 for all three hops; odd lengths with 1
# and 2 channels, 3 and 5 items; a target channel on the magnitude clamp; the folded peak
MR_INPUTS = ("noise-1025-c1-p1", "noise-1200-c2-p3", "noise-2049-c1-p3", "noise-4097-c2-p5", "zero-target-channel-1025", "peak-folded-2049")
# a plan whose prefiltered tiling differs from the plain one (the span bound cuts F at hop 2000)
WIDE_HOP = ((256, 2000, 256), (512, 50, 240))
WF_TAPS = ("none", "unit", "shift", "aw", "fir255")
WF_LENGTHS = (5, 8192, 8193, 12345)   # one partial run, rows not 16-byte aligned; one whole tile; a second tile of one sample; 1.5 tiles
WF_KINDS = ("esr", "dc", "snr", "sisdr", "logcosh")


def _mr(form, taps, source, res=None, slots=None):
    return dict(family="mrstft", form=form, taps=taps, source=source, res=res, slots=slots)


def cases():
    """MR-STFT: every form, plain, over its inputs; every form x every tap set; the "aw" filter over more inputs; the wide-hop plan
    plain and prefiltered; per form, plain and prefiltered, a slot list [1, 2, 0] over three populations of 2 candidates and one whose
    slot 7 names no target (its candidates are NaN: the pattern is part of the bytes).
    Waveform (each case scores all five kinds against one table): every tap set x every length, the channel counts 1, 2, 3 going
    round so that each meets every tap set and every length; a folded peak; a slot list; a bad slot."""
    import mrstft_sd_cases as SDC
    out = []
    sd_inputs = [c[0] for c in SDC.cases()]
    for form in FORMS:
        out += [_mr(form, None, name) for name in (sd_inputs if form == "sum-diff" else MR_INPUTS)]
    per_tap = {"lr": ("noise-1025-c1-p1", "noise-4097-c2-p5"), "sum-diff": ("noise-1200-c2-p3",), "mel": ("noise-2049-c1-p3",)}
    more_aw = {"lr": ("noise-1200-c2-p3", "noise-2049-c1-p3", "zero-target-channel-1025", "peak-folded-2049"),
               "sum-diff": ("zero-target-channel-1025", "sd-peak-folded-2049", "sd-mono-target-1025"),
               "mel": ("noise-4097-c2-p5", "peak-folded-2049")}
    for form in FORMS:
        out += [_mr(form, t, name) for t in TAPS for name in per_tap[form]]
        out += [_mr(form, "aw", name) for name in more_aw[form]]
    out += [_mr("lr", t, "noise-12345-c1-p1", res=WIDE_HOP) for t in (None, "aw")]
    for form in FORMS:
        for t in (None, "aw"):
            out += [_mr(form, t, "slots-2049", slots=s) for s in ((1, 2, 0), (1, 7, 0))]
    for ti, t in enumerate(WF_TAPS):
        for li, n in enumerate(WF_LENGTHS):
            out.append(dict(family="waveform", taps=t, n=n, channels=1 + (ti + li) % 3, fold=False, slots=None))
    out.append(dict(family="waveform", taps="aw", n=8193, channels=2, fold=True, slots=None))
    out += [dict(family="waveform", taps="aw", n=8193, channels=2, fold=False, slots=s) for s in ((1, 2, 0), (1, 7, 0))]
    return out


def case_id(c):
    slots = "" if c["slots"] is None else "-slots" + "".join(str(s) for s in c["slots"])
    if c["family"] == "mrstft":
        return f"mrstft-{c['form']}-{c['taps'] or 'plain'}-{c['source']}{'-widehop' if c['res'] else ''}{slots}"
    return f"waveform-{c['taps']}-n{c['n']}-c{c['channels']}{'-fold' if c['fold'] else ''}{slots}"


def arrays_of(c):
    """The names of the arrays a case records."""
    return ("table", "loss") if c["family"] == "mrstft" else ("table",) + WF_KINDS


_MEMO = {}


def _taps(name):
    import waveform_ref as WR
    if "taps" not in _MEMO:
        _MEMO["taps"] = WR.tap_sets()
    return _MEMO["taps"][name]


def _mr_inputs(c):
    """-> x (P, C, n), y (T, C, n), norm_passes, as CPU float32 tensors"""
    import torch
    import mrstft_cases as M
    import mrstft_sd_cases as SDC
    if c["slots"] is not None:
        # 3 targets of 2 channels (what the sum / difference form takes), 3 populations of 2 candidates: mrstft_cases' estimate recipe,
        # candidates 2 k and 2 k + 1 made from target k
        y = M.noise(500, 3, 2, 2049)
        return torch.tanh(1.5 * y.repeat_interleave(2, 0) + 0.2 * M.noise(501, 6, 2, 2049)), y, 0
    if "named" not in _MEMO:
        _MEMO["named"] = {name: (x, y, norm) for name, x, y, norm in M.cases() + SDC.cases()}
    return _MEMO["named"][c["source"]]


def _hashed(table, losses):
    import torch
    torch.cuda.synchronize()
    out = {"table": hashlib.sha256(table[: table.numel() // 2].cpu().numpy().tobytes()).hexdigest()}
    for name, v in losses.items():
        out[name] = hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest()
    return out


def run_case(c):
    """-> {array name: sha256}, through the Python tables of st_ito.features (the library is _hip.LIB_PATH: STITO_LIB_PATH decides)."""
    import numpy as np
    import torch
    import waveform_ref as WR
    from st_ito import features as F
    dev = torch.device("cuda", 0)
    slots = None if c["slots"] is None else torch.tensor(c["slots"], dtype=torch.int32, device=dev)
    if c["family"] == "mrstft":
        x, y, norm = _mr_inputs(c)
        xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
        peaks = xd.abs().amax(dim=(1, 2)) if norm else None
        bank = None
        if c["form"] == "mel":
            if "bank" not in _MEMO:
                _MEMO["bank"] = F.mel_mrstft_bank(SR)
            bank = _MEMO["bank"]
        if c["taps"] is not None:
            tgt = F.PrefilteredMrstftTarget(yd, _taps(c["taps"]), kind=c["form"], resolutions=c["res"], bank=bank)
        elif c["form"] == "mel":
            tgt = F.MelMrstftTarget(yd, resolutions=c["res"], bank=bank)
        else:
            tgt = F.MrstftTarget(yd, c["res"], c["form"])
        tgt.table.zero_()
        tgt.update(yd)
        return _hashed(tgt.table, {"loss": tgt.loss(xd, peaks, norm, slots=slots)})
    taps, n, C = _taps(c["taps"]), c["n"], c["channels"]
    T, pop = (3, 6) if c["slots"] is not None else (WR.P, WR.P)
    rng = np.random.default_rng([list(WF_TAPS).index(c["taps"]), n, C, 11])
    x, y = (np.concatenate(v) for v in zip(*[WR._pair(rng, C, n) for _ in range(pop // WR.P)]))
    if c["fold"]:
        x = (x * np.float32(1.7)).astype(np.float32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y[:: pop // T].copy()).to(dev)
    peaks = xd.abs().amax(dim=(1, 2)) if c["fold"] else None
    tgt = F.WaveformTarget(yd, taps)
    tgt.table.zero_()
    tgt.update(yd)
    return _hashed(tgt.table, {k: tgt.loss(xd, peaks, int(c["fold"]), slots=slots, kind=k) for k in WF_KINDS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the revision the library was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    from st_ito import _hip
    fixture = {"library": os.path.relpath(_hip.LIB_PATH, ROOT), "commit": a.commit, "cases": {}}
    for c in cases():
        fixture["cases"][case_id(c)] = run_case(c)
    assert len(fixture["cases"]) == len(cases()), "two cases share an id"
    with open(a.out, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in fixture["cases"].values())
    print(f"recorded {len(fixture['cases'])} cases, {n} arrays, with {_hip.LIB_PATH} ({a.commit}) -> {a.out}")


if __name__ == "__main__":
    main()
