"""Host side of the waveform objectives (distance="esr", "snr", "sisdr", "logcosh" and their "-aw" forms; csrc/waveform.hip): the
float64 reference of tests/waveform_ref.py against a second formulation, the yardstick tests/test_gpu_waveform.py measures the
kernel with, the ABI declarations, the size functions, the refusals of every entry point and every driver -- all of which come
before anything needs a GPU --, the CLI, and the drivers on the CPU stand-in of tests/test_mrstft_batch_host.py.

The yardstick of a case: the float32 torch restatement (float32 conv1d, float32 sums) against the float64 reference, the largest
relative distance over esr, snr and sisdr and over the case's items.  It must stay at or below 2e-5 on every case; that is a
ceiling, not the measurement.  Measured on the case list: 2.1e-8 .. 8.8e-7 (the rows are short: the largest has 16 387 samples),
0 where every row is zero after the filter ([0, 0, 1] at one sample).  BAR_FACTOR = 4 times a case's yardstick is the GPU test's
bar for that case."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import test_mrstft_batch_host as B
import waveform_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = W.SR
NEW = ("stito_waveform_tile_samples", "stito_waveform_table_floats", "stito_waveform_workspace_bytes", "stito_waveform_target",
       "stito_waveform_loss", "stito_waveform_loss_slots")
NAMES = ("esr", "snr", "sisdr", "logcosh", "esr-aw", "snr-aw", "sisdr-aw", "logcosh-aw")
KIND_OF = {name: (name.replace("-aw", ""), "aw" if name.endswith("-aw") else None) for name in NAMES}


# ---------------------------------------------------------------------------------------------------------------------------
# the reference and the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def _second_formulation(x, y, taps, peaks, norm_passes):
    """Independent of waveform_ref.rows64: torch float64, conv1d for the filter, the formulas written out row by row with dot
    products and means."""
    xs = torch.from_numpy(W.scored32(x, peaks, norm_passes)).to(torch.float64)
    ys = torch.from_numpy(np.asarray(y, dtype=np.float32)).to(torch.float64)
    if taps is not None:
        t = torch.from_numpy(np.asarray(taps, dtype=np.float32)).to(torch.float64)[None, None]
        f = lambda a: torch.nn.functional.conv1d(a.reshape(-1, 1, a.shape[-1]), t, padding=t.shape[-1] // 2).reshape(a.shape)   # noqa: E731
        xs, ys = f(xs), f(ys)
    out = {k: [] for k in W.KINDS}
    for item in range(xs.shape[0]):
        vals = {k: [] for k in W.KINDS}
        for px, py in zip(xs[item], ys[item if ys.shape[0] > 1 else 0]):
            n = px.numel()
            d = px - py
            ey, ed = torch.dot(py, py), torch.dot(d, d)
            vals["esr"].append(ed / (ey + 1e-8))
            vals["dc"].append(d.mean() ** 2 / (ey / n + 1e-8))
            vals["snr"].append(-10.0 * torch.log10(ey / (ed + 1e-8) + 1e-8))
            xc, yc = px - px.mean(), py - py.mean()
            t_ = torch.dot(xc, yc) / (torch.dot(yc, yc) + 1e-8) * yc
            vals["sisdr"].append(-10.0 * torch.log10(torch.dot(t_, t_) / (torch.dot(xc - t_, xc - t_) + 1e-8) + 1e-8))
            nz = d[d != 0]
            vals["logcosh"].append(torch.log1p(torch.expm1(nz) ** 2 / (2.0 * torch.exp(nz)) + 1e-8).sum() / n)   # cosh - 1 = (e^d - 1)^2 / 2 e^d
        for k in W.KINDS:
            out[k].append(float(torch.stack(vals[k]).mean()))
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("tap_name", list(W.tap_sets()))
def test_reference_agrees_with_a_second_float64_formulation(tap_name):
    taps = W.tap_sets()[tap_name]
    for case in W.cases(tap_name):
        name, x, y, peaks, norm_passes = case
        ref, other = W.case_reference(tap_name, case), _second_formulation(x, y, taps, peaks, norm_passes)
        for kind in W.KINDS:
            assert ref[kind].shape == (W.P,) and np.all(np.isfinite(ref[kind])), (tap_name, name, kind, ref[kind])
            assert np.all(np.abs(ref[kind] - other[kind]) <= 1e-12 * np.maximum(np.abs(ref[kind]), 1e-300)) or \
                W.relative(other[kind], ref[kind]).max() <= 1e-12, (tap_name, name, kind, ref[kind], other[kind])


@pytest.mark.parametrize("tap_name", list(W.tap_sets()))
def test_float32_yardstick_stays_within_2e5_on_every_case(tap_name):
    yard = {c[0]: W.yardstick(tap_name, c) for c in W.cases(tap_name)}
    for name, v in yard.items():
        print(f"{tap_name:6s} {name:22s} float32 restatement vs float64: {v:.3e}   GPU bar {W.BAR_FACTOR * v:.3e}")
    assert W.BAR_FACTOR == 4.0 and W.YARD_CAP == 2e-5
    assert all(np.isfinite(v) and v <= W.YARD_CAP for v in yard.values()), yard


def test_the_case_list_is_the_family():
    for tap_name, taps in W.tap_sets().items():
        tile = W.tile_samples(taps)
        names = [c[0] for c in W.cases(tap_name)]
        assert len(set(names)) == len(names)
        for n in (1, 2, 5, tile - 1, tile, tile + 1, 2 * tile + 3):
            for channels in (1, 2, 3):
                case = [c for c in W.cases(tap_name) if c[0] == f"n{n}-c{channels}"][0]
                assert case[1].shape == case[2].shape == (W.P, channels, n) and case[1].dtype == case[2].dtype == np.float32
                assert case[3] is None and case[4] == 0
        for n in (5, tile + 1):
            zt, zc, pf = ([c for c in W.cases(tap_name) if c[0] == f"{what}-n{n}"][0] for what in ("zero-target", "zero-candidate", "peak-folded"))
            assert not zt[2].any() and zt[1].any() and not zc[1].any() and zc[2].any() and zc[4] == 1 and not zc[3].any()
            assert pf[4] == 1 and np.array_equal(pf[3], np.abs(pf[1]).max(axis=(1, 2))) and np.all(pf[3] != 1.0)
    sets = W.tap_sets()
    assert sets["none"] is None and sets["unit"].tolist() == [1.0] and sets["shift"].tolist() == [0.0, 0.0, 1.0]
    assert [len(sets[k]) for k in ("fir31", "aw", "fir255")] == [31, 101, 255]
    assert np.abs(sets["fir31"] - sets["fir31"][::-1]).max() > 1e-2
    # the family's ranges on a long unfiltered case: ESR 1e-2 .. 3e-1, SI-SDR far below 80 dB, a DC term that is there
    case = [c for c in W.cases("none") if c[0] == f"n{2 * W.tile_samples(None) + 3}-c2"][0]
    ref = W.case_reference("none", case)
    assert np.all((ref["esr"] > 1e-2) & (ref["esr"] < 3e-1)) and np.all(np.abs(ref["sisdr"]) < 40) and np.all(ref["dc"] > 1e-4)
    assert np.all(ref["dc"] <= ref["esr"])


def test_reference_properties():
    """Exact zeros of a row against itself, the polarity value, and the d == 0 rule of the log-cosh sum."""
    y = np.random.default_rng(3).uniform(-0.9, 0.9, (1, 2, 301)).astype(np.float32)
    same = W.reference(y, y, W.tap_sets()["fir31"])
    assert same["esr"][0] == 0.0 and same["dc"][0] == 0.0 and same["logcosh"][0] == 0.0 and same["snr"][0] < -60.0 and same["sisdr"][0] < -60.0
    assert W.reference(y, -y)["esr"][0] == pytest.approx(4.0, rel=1e-9)
    padded = np.concatenate([y, np.zeros_like(y)], -1)
    assert W.reference(padded, 0.5 * padded)["logcosh"][0] == pytest.approx(0.5 * W.reference(y, 0.5 * y)["logcosh"][0], rel=1e-12)
    assert W.reference(padded, 0.5 * padded)["esr"][0] == pytest.approx(W.reference(y, 0.5 * y)["esr"][0], rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_in_header_binding_library_and_integration():
    from st_ito import _hip
    header = open(os.path.join(ROOT, "include", "stito_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"^\| .*`%s`.* \| " % name, integration, re.M), f"{name} has no row in INTEGRATION.md's map"
    assert "10 = the waveform distances" in header
    assert "`stito_version_minor()` **10**" in integration
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 10
    sig = _hip.SIGNATURES
    head = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]       # kind, taps_dev, n_taps
    assert sig["stito_waveform_loss"][1] == head + sig["stito_mrstft_loss"][1][2:]
    assert sig["stito_waveform_loss_slots"][1] == head + sig["stito_mrstft_loss_slots"][1][2:]


def _p():
    return ctypes.c_void_p(64)       # not null; a refusal comes before it is used


def test_every_entry_point_refuses_on_the_host_naming_the_value():
    """STITO_E_INVALID before any launch (this test has no device): the kind, the taps, the sizes, the slot list."""
    from st_ito import _hip
    lib = _hip.lib()

    def loss(kind=0, taps=None, n_taps=0, channels=2, n=4097, norm_passes=0, peaks=None, pop=4, n_targets=1):
        return lib.stito_waveform_loss(kind, taps, n_taps, _p(), peaks, norm_passes, _p(), n_targets, pop, channels, n, _p(), _p(), 1 << 30, None)

    def slots(kind=0, taps=None, n_taps=0, channels=2, n=4097, slot_dev=None, n_slots=1, pop=4):
        return lib.stito_waveform_loss_slots(kind, taps, n_taps, _p(), None, 0, _p(), 1, slot_dev, n_slots, pop, channels, n, _p(), _p(), 1 << 30, None)

    def target(taps=None, n_taps=0, rows=2, n=4097):
        return lib.stito_waveform_target(taps, n_taps, _p(), rows, n, _p(), None)

    for kw, word in ((dict(kind=5), b"kind 5"), (dict(kind=-1), b"kind -1"), (dict(taps=_p(), n_taps=100), b"n_taps 100 must be odd"),
                     (dict(taps=_p(), n_taps=257), b"n_taps 257"), (dict(taps=_p(), n_taps=-1), b"n_taps -1"),
                     (dict(n_taps=101), b"null taps_dev"), (dict(n=0), b"0 samples"), (dict(channels=9), b"channels: 9"),
                     (dict(channels=0), b"channels: 0"), (dict(norm_passes=2), b"norm_passes 2"), (dict(norm_passes=1), b"needs the peaks"),
                     (dict(pop=0), b"pop 0"), (dict(pop=3, n_targets=2), b"not a multiple")):
        assert loss(**kw) == _hip.E_INVALID, (kw, lib.stito_last_error())
        assert word in lib.stito_last_error(), (word, lib.stito_last_error())
    for kw, word in ((dict(taps=_p(), n_taps=2), b"n_taps 2 must be odd"), (dict(n_taps=3), b"null taps_dev"), (dict(n=0), b"0 samples"),
                     (dict(rows=0), b"0 rows")):
        assert target(**kw) == _hip.E_INVALID and word in lib.stito_last_error(), (kw, lib.stito_last_error())
    assert slots() == _hip.E_INVALID and b"target_slot_dev" in lib.stito_last_error()
    assert slots(slot_dev=_p(), kind=7) == _hip.E_INVALID and b"kind 7" in lib.stito_last_error()
    assert slots(slot_dev=_p(), n_slots=3) == _hip.E_INVALID and b"not a multiple" in lib.stito_last_error()
    # a workspace that is too small is refused, not overrun
    rc = lib.stito_waveform_loss(0, None, 0, _p(), None, 0, _p(), 1, 4, 2, 4097, _p(), _p(), 8, None)
    assert rc == _hip.E_WORKSPACE and b"workspace" in lib.stito_last_error()


def test_size_functions_answer_zero_for_what_the_launches_refuse():
    from st_ito import _hip
    lib = _hip.lib()
    tile, table, ws = lib.stito_waveform_tile_samples, lib.stito_waveform_table_floats, lib.stito_waveform_workspace_bytes
    for n_taps in (0, 1, 3, 101, 255):
        t = tile(n_taps)
        assert t >= 4 and t % 4 == 0
        assert table(n_taps, 2, 12345) >= 2 * 12345 and ws(n_taps, 4, 2, 12345) > 0
        assert table(n_taps, 1, 1) > 0 and ws(n_taps, 1, 1, 1) > 0 and ws(n_taps, 1, 8, 1) > 0
        # a tile more is a partial more per row
        assert ws(n_taps, 4, 2, t + 1) == 2 * ws(n_taps, 4, 2, t) and ws(n_taps, 4, 2, t) == ws(n_taps, 4, 2, 1)
        assert table(n_taps, 2, 12345) == 2 * table(n_taps, 1, 12345)
        assert table(n_taps, 0, 12345) == 0 and table(n_taps, 2, 0) == 0 and table(n_taps, 2, -5) == 0
        assert ws(n_taps, 0, 2, 12345) == 0 and ws(n_taps, 4, 0, 12345) == 0 and ws(n_taps, 4, 9, 12345) == 0 and ws(n_taps, 4, 2, 0) == 0
    for n_taps in (2, 100, 256, 257, -1, -3):
        assert tile(n_taps) == 0 and table(n_taps, 2, 12345) == 0 and ws(n_taps, 4, 2, 12345) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# Python: refusals before the device, signatures
# ---------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_the_gpu():
    """On a machine without a GPU every one of these would otherwise fail with another error."""
    from st_ito import engine, effects as E
    from st_ito.features import WaveformTarget, compute_waveform_distance as dist
    x = torch.zeros((2, 2, 4096))
    for call in (lambda **k: dist(x, x, **k), lambda **k: WaveformTarget(x, **k)):
        with pytest.raises(ValueError, match="odd"):
            call(prefilter=np.ones(4))
        with pytest.raises(ValueError, match="at most 255"):
            call(prefilter=np.ones(257))
        with pytest.raises(ValueError, match="sample_rate"):
            call(prefilter="aw")
        with pytest.raises(ValueError, match="unknown prefilter"):
            call(prefilter="a-weighting", sample_rate=SR)
    for kind in ("l2", "ESR", "", "si-sdr", None):
        with pytest.raises(ValueError, match="kind must be one of"):
            dist(x, x, kind)
    with pytest.raises(ValueError, match="do not match"):
        dist(x, torch.zeros((2, 2, 4095)))
    with pytest.raises(ValueError, match="do not match"):
        dist(x, torch.zeros((3, 2, 4096)))
    with pytest.raises(ValueError, match="channels: 9"):
        dist(torch.zeros((1, 9, 16)), torch.zeros((1, 9, 16)))
    with pytest.raises(ValueError, match="at least 1"):
        dist(torch.zeros((1, 2, 0)), torch.zeros((1, 2, 0)))
    with pytest.raises(ValueError):
        dist(x[0], x[0])
    for kw, match in ((dict(kind="l2"), "kind must be one of"), (dict(prefilter=np.ones(2)), "odd"), (dict(prefilter=np.ones(301)), "at most 255"),
                      (dict(kind="dc", prefilter="aw-"), "unknown prefilter")):
        with pytest.raises(ValueError, match=match):
            engine.WaveformEvaluator(x[:1], SR, E.make_plugins("eq"), x[:1], **kw)
    with pytest.raises(ValueError, match="sample_rate"):
        engine.WaveformEvaluator(x[:1], None, E.make_plugins("eq"), x[:1], prefilter="aw")


def test_signatures():
    from st_ito import engine, features
    p = inspect.signature(features.compute_waveform_distance).parameters
    assert list(p) == ["x", "y", "kind", "prefilter", "sample_rate"]
    assert p["kind"].default == "esr" and p["prefilter"].default is None and p["sample_rate"].default is None
    p = inspect.signature(features.WaveformTarget.__init__).parameters
    assert list(p) == ["self", "y", "prefilter", "sample_rate", "taps_dev"] and all(p[k].default is None for k in list(p)[2:])
    p = inspect.signature(features.WaveformTarget.loss).parameters
    assert list(p) == ["self", "audio", "peaks", "norm_passes", "slots", "ws", "kind"] and p["kind"].default == "esr"
    assert list(p)[:-1] == list(inspect.signature(features.MrstftTarget.loss).parameters)
    assert list(inspect.signature(features.WaveformTarget.update).parameters) == ["self", "y"]
    assert issubclass(engine.WaveformEvaluator, engine.MrstftEvaluator)
    for name in ("evaluate", "set_static_targets", "_static_table", "_refilled_table", "_input_and_target"):
        assert getattr(engine.WaveformEvaluator, name) is getattr(engine.MrstftEvaluator, name), name
    assert engine.WaveformEvaluator._target_table is not engine.MrstftEvaluator._target_table
    p = inspect.signature(engine.WaveformEvaluator.__init__).parameters
    assert list(p)[:7] == ["self", "x", "sample_rate", "plugins", "target_audio", "kind", "prefilter"]
    assert p["kind"].default == "esr" and p["prefilter"].default is None
    assert list(features.WAVEFORM_KINDS) == list(W.KINDS) and list(features.WAVEFORM_KINDS.values()) == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------------------------------
# the drivers: refusals, the evaluator they build, the CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_names():
    from st_ito import style_transfer
    assert set(NAMES) <= set(style_transfer._AUDIO_DISTANCES) and len(set(style_transfer._AUDIO_DISTANCES)) == len(style_transfer._AUDIO_DISTANCES)
    for old in ("mrstft", "mrstft-sd", "mrstft-mel", "mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw"):
        assert old in style_transfer._AUDIO_DISTANCES
    for other in ("dc", "dc-aw", "l2", "", "aw", "sd", "mel", "ESR", "esr-sd", "si-sdr", "sisdr-mel", "log-cosh"):
        assert other not in style_transfer._AUDIO_DISTANCES
        with pytest.raises(ValueError, match="Unknown distance"):
            style_transfer._check_distance(other, SR)
    for name in NAMES:
        style_transfer._check_distance(name, SR)


def _no_evaluator(monkeypatch):
    from st_ito import engine
    B._no_evaluator(monkeypatch)
    for name in ("MelMrstftEvaluator", "PrefilteredMrstftEvaluator", "WaveformEvaluator"):
        monkeypatch.setattr(engine, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("an evaluator was built")))


def _es_args(n=4096, chs=2, tgt_chs=None, tgt_n=None, sr=SR, plugins=None):
    x = torch.rand((1, chs, n)) - 0.5
    t = torch.rand((1, tgt_chs or chs, tgt_n or n)) - 0.5
    return x, t, sr, plugins or B._plugins(), None, None


def _untouched(call, args, match):
    keep = [a.clone() for a in args[:2]]
    with pytest.raises(ValueError, match=match):
        call(*args)
    assert all(torch.equal(a, b) for a, b in zip(keep, args[:2]))


@pytest.mark.parametrize("distance", NAMES)
def test_driver_refusals_come_before_any_launch(monkeypatch, distance):
    """The rules of the audio distances, with their messages, before an input is normalised."""
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    _no_evaluator(monkeypatch)
    kw = dict(distance=distance, popsize=4, max_iters=2, seed=0)
    run = lambda **over: (lambda *a: run_es(*a, find_w0=False, **dict(kw, **over)))   # noqa: E731
    _untouched(run(), _es_args(tgt_n=4000), f"distance '{distance}' compares sample spans")
    _untouched(run(), _es_args(chs=2, tgt_chs=1), f"distance '{distance}': the target has 1 channels, the chain renders 2")
    _untouched(run(dropout=0.1), _es_args(), f"'{distance}' has no embeddings: dropout")
    _untouched(run(savepop=True), _es_args(), f"'{distance}' does not write populations")
    _untouched(run(device_es=True), _es_args(tgt_n=4000), "sample spans")
    _untouched(run(device_es=True, savepop=True), _es_args(), "savepop")
    _untouched(lambda *a: run_es(*a, find_w0=False, content_model=object(), content_embed_func=lambda *b: {}, **kw), _es_args(),
               f"'{distance}' has no embeddings: content_model")
    for other in ("l2", "", "aw", "sd", "mel", distance.upper(), distance + "-sd", distance.replace("-aw", "") + "_aw"):
        _untouched(run(distance=other), _es_args(), "Unknown distance")
    _untouched(lambda *a: run_staged_es(*a, **kw), _es_args(tgt_n=4000), "sample spans")
    _untouched(lambda *a: run_staged_es(*a, savepop=True, **kw), _es_args(), "savepop")
    _untouched(lambda *a: run_es_batch(*a, **kw), _es_args(tgt_n=4000), "target 0")
    _untouched(lambda x, t, *a: run_es_batch([x[0]], [t[0]], *a, **kw), _es_args(chs=2, tgt_chs=1), "target 0 has 1 channels")
    if distance.endswith("-aw"):          # the taps of the rate are designed on the host first
        for call in (run(), run(device_es=True), lambda *a: run_staged_es(*a, **kw), lambda *a: run_es_batch(*a, **kw)):
            _untouched(call, _es_args(sr=None), "sample_rate")


class _StandIn(B._StandInEvaluator):
    def __init__(self, *args, **kw):
        self.n_positional, self.kw = len(args), dict(kw)
        super().__init__(*args, **kw)


@pytest.fixture
def stand_in(monkeypatch):
    from st_ito import engine, style_transfer
    B._StandInEvaluator.built = []
    no = lambda *a, **k: (_ for _ in ()).throw(AssertionError("another evaluator"))   # noqa: E731
    monkeypatch.setattr(engine, "WaveformEvaluator", _StandIn)
    for name in ("MrstftEvaluator", "MelMrstftEvaluator", "PrefilteredMrstftEvaluator", "PopulationEvaluator"):
        monkeypatch.setattr(engine, name, no)
    monkeypatch.setattr(engine, "RaggedInputs", B._StandInRagged)
    monkeypatch.setattr(engine, "_current_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(style_transfer, "process_audio",
                        lambda x, w, sr, plugins, normalize_stages=False: (np.asarray(x) * np.float32(1 + float(np.sum(w)))).astype(np.float32))
    return _StandIn


@pytest.mark.parametrize("distance", NAMES)
def test_each_name_reaches_every_driver_and_builds_its_evaluator(stand_in, tmp_path, distance):
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    x, t = B._pair(0, 24000)
    x, t = torch.cat([x, 0.5 * x]), torch.cat([t, 0.5 * t])
    kw = dict(max_iters=2, popsize=4, sigma0=0.2, seed=1, distance=distance)
    run_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, find_w0=False, **kw)
    run_staged_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, run_dir=str(tmp_path), **kw)
    run_es_batch(torch.stack([x, x]), torch.stack([t, t]), SR, B._plugins(), None, None, **kw)
    run_es_batch([x, x], [t, t], SR, B._plugins(), None, None, **kw)
    assert len(stand_in.built) == 5                      # the staged ES builds one per stage
    kind, prefilter = KIND_OF[distance]
    for ev in stand_in.built:
        assert ev.n_positional == 4 and ev.kw == {"kind": kind, "prefilter": prefilter}, (distance, ev.n_positional, ev.kw)


def test_list_form_equals_run_es_on_the_stand_in(stand_in):
    from st_ito.style_transfer import run_es, run_es_batch
    lengths = [300000, 300000, 1000]
    pairs = [B._pair(b, n, silent=(b == 1)) for b, n in enumerate(lengths)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, early_stop=True, distance="esr-aw")
    res = run_es_batch(xs, ts, SR, B._plugins(), None, None, seed=7, **kw)
    assert len(stand_in.built) == 1
    for b in range(len(lengths)):
        one = run_es(xs[b].clone()[None], ts[b].clone()[None], SR, B._plugins(), None, None, find_w0=False, seed=7 + b, **kw)
        B._same_run(res[b], one)


def test_objective_flag_and_the_call_main_builds(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    from st_ito.audio_io import save_wav
    p = run_optim.build_parser()
    for name in NAMES:
        assert p.parse_args(["in.wav", "--objective", name]).objective == name and name in run_optim.AUDIO_OBJECTIVES
    assert p.parse_args(["in.wav"]).objective == "embedding"
    for other in ("dc", "aw", "esr-sd", "l2"):
        with pytest.raises(SystemExit):
            p.parse_args(["in.wav", "--objective", other])
    rng = np.random.default_rng(0)
    for name in ("in.wav", "tgt.wav"):
        save_wav(str(tmp_path / name), torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 4800)).astype(np.float32)), SR)
    calls = []

    def fake(*args, **kwargs):
        calls.append((args, kwargs))
        return {"output_audio": torch.zeros(1, 2, 4800), "params": {}, "fopt": 0.0, "num_evals": 0, "fval_history": [0.0]}

    monkeypatch.setattr(run_optim, "run_es", fake)
    monkeypatch.setattr(run_optim, "run_staged_es", fake)
    monkeypatch.setattr(run_optim, "load_param_model", lambda **k: (_ for _ in ()).throw(AssertionError("a checkpoint was loaded")))
    argv = [str(tmp_path / "in.wav"), str(tmp_path / "tgt.wav"), "--chain", "eq", "--output-dir", str(tmp_path / "out")]
    run_optim.main(argv + ["--objective", "esr"])
    run_optim.main(argv + ["--objective", "sisdr-aw", "--staged"])
    assert [kwargs["distance"] for _, kwargs in calls] == ["esr", "sisdr-aw"]
    assert all(args[4] is None and args[5] is None for args, _ in calls)        # model, embed_func
