"""Host side of the prefiltered MR-STFT objectives (distance="mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw"; csrc/mrstft.hip's PRE
variants): the ABI declarations, the refusals of every entry point, which all come before anything needs a GPU, the size functions,
the "aw" design, the CLI, the drivers on the CPU stand-in of tests/test_mrstft_batch_host.py, and the yardstick that
tests/test_gpu_mrstft_aw.py measures the kernel with.

The yardstick: over the inputs of tests/mrstft_cases.py (sum / difference: tests/mrstft_sd_cases.py), with the 48 kHz "aw" taps,
the float32 restatement (float32 conv1d, then torch.stft on the CPU) stays within 1e-4 of the float64 one, item by item.  1e-4 is a
ceiling, not the measurement.  Measured: linear 1.65e-5, sum / difference 1.50e-5, mel 8.3e-6, all three on twotone-2049, whose
bins between and above the tones sit near the magnitude clamp, where the float32 error of the filtered row is a large part of the
magnitude (the unfiltered restatements measure 3.6e-6 and 4.0e-7 on the same set).  Every case is finite.  BAR_FACTOR = 4 times the
measured maximum over the case set, for the tap set and form in use, is the GPU test's bar: 6.6e-5 / 6.0e-5 / 3.3e-5 for the "aw"
taps, 1.4e-5 for the seeded 31-tap and 255-tap filters of the GPU test (their maximum is the zero-target-channel case's 3.6e-6)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import mrstft_aw_ref as A
import test_mrstft_batch_host as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = A.SR
NEW = ("stito_mrstft_table_floats_pf", "stito_mrstft_workspace_bytes_pf", "stito_mrstft_target_pf", "stito_mrstft_loss_pf",
       "stito_mrstft_loss_slots_pf")
NAMES = ("mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw")


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
    assert "9 = the prefiltered MR-STFT distances" in header
    assert "`stito_version_minor()` **9**" in integration
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 9
    sig = _hip.SIGNATURES
    head = [ctypes.c_int, ctypes.POINTER(_hip.MelBank), ctypes.c_void_p, ctypes.c_int]       # kind, bank, taps_dev, n_taps
    assert sig["stito_mrstft_loss_pf"][1] == head + sig["stito_mrstft_loss"][1]
    assert sig["stito_mrstft_loss_slots_pf"][1] == head + sig["stito_mrstft_loss_slots"][1]
    assert sig["stito_mrstft_target_pf"][1] == head + sig["stito_mrstft_target_sd"][1]


def _taps_ptr():
    return ctypes.c_void_p(64)       # not null; a refusal comes before it is used


def test_every_entry_point_refuses_on_the_host_naming_the_value():
    """Even or out-of-range n_taps, null taps, an unknown kind, a missing bank under kind 2, a bank under the others, channels other
    than 2 under kind 1: STITO_E_INVALID from all three calls, before a device is asked anything (this test has none)."""
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    bank = _hip.MelBank()

    def statuses(kind, bank_ref, taps, n_taps, channels=2):
        return (lib.stito_mrstft_target_pf(kind, bank_ref, taps, n_taps, res, n_res, None, 1, channels, 4097, None, None),
                lib.stito_mrstft_loss_pf(kind, bank_ref, taps, n_taps, res, n_res, None, None, 0, None, 1, 1, channels, 4097, None, None, 0, None),
                lib.stito_mrstft_loss_slots_pf(kind, bank_ref, taps, n_taps, res, n_res, None, None, 0, None, 1, None, 1, 1, channels, 4097, None,
                                               None, 0, None))

    for args, word in (((0, None, _taps_ptr(), 100), b"n_taps 100 must be odd"), ((0, None, _taps_ptr(), 0), b"n_taps 0"),
                       ((0, None, _taps_ptr(), -1), b"n_taps -1"), ((1, None, _taps_ptr(), 257), b"n_taps 257"),
                       ((0, None, None, 101), b"null taps_dev"), ((3, None, _taps_ptr(), 101), b"kind 3"),
                       ((-1, None, _taps_ptr(), 101), b"kind -1"), ((2, None, _taps_ptr(), 101), b"null bank"),
                       ((0, ctypes.byref(bank), _taps_ptr(), 101), b"kind 0 takes no bank"),
                       ((1, ctypes.byref(bank), _taps_ptr(), 101), b"kind 1 takes no bank")):
        assert statuses(*args) == (_hip.E_INVALID,) * 3, (word, lib.stito_last_error())
        assert word in lib.stito_last_error(), (word, lib.stito_last_error())
    assert statuses(1, None, _taps_ptr(), 101, channels=1) == (_hip.E_INVALID,) * 3 and b"needs 2 channels, got 1" in lib.stito_last_error()
    assert statuses(1, None, _taps_ptr(), 101, channels=3) == (_hip.E_INVALID,) * 3 and b"got 3" in lib.stito_last_error()
    # good taps: the slot call still wants its slot list
    assert statuses(0, None, _taps_ptr(), 101)[2] == _hip.E_INVALID and b"target_slot_dev" in lib.stito_last_error()


def test_size_functions_answer_zero_for_what_the_launches_refuse():
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    table, ws = lib.stito_mrstft_table_floats_pf, lib.stito_mrstft_workspace_bytes_pf
    for kind, n_bins in ((0, 0), (1, 0), (2, 64)):
        assert table(kind, n_bins, 101, res, n_res, 2, 12345) > 0 and ws(kind, 101, res, n_res, 4, 2, 12345) > 0
        assert table(kind, n_bins, 1, res, n_res, 2, 12345) > 0 and table(kind, n_bins, 255, res, n_res, 2, 12345) > 0
        for n_taps in (0, 100, 256, 257, -3):
            assert table(kind, n_bins, n_taps, res, n_res, 2, 12345) == 0 and ws(kind, n_taps, res, n_res, 4, 2, 12345) == 0
        assert table(kind, n_bins, 101, res, n_res, 2, 1024) == 0 and ws(kind, 101, res, n_res, 4, 2, 1024) == 0     # too few samples
        assert table(kind, n_bins, 101, res, n_res, 0, 12345) == 0 and ws(kind, 101, res, n_res, 0, 2, 12345) == 0
    for kind in (-1, 3):
        assert table(kind, 0, 101, res, n_res, 2, 12345) == 0 and ws(kind, 101, res, n_res, 4, 2, 12345) == 0
    assert table(0, 64, 101, res, n_res, 2, 12345) == 0 and table(2, 0, 101, res, n_res, 2, 12345) == 0 and table(2, 257, 101, res, n_res, 2, 12345) == 0
    assert table(1, 0, 101, res, n_res, 3, 12345) == 0 and ws(1, 101, res, n_res, 4, 1, 12345) == 0                  # sum / difference: 2 channels
    # a hop so large that the unfiltered plan's tile would not fit the prefilter's span bound: the prefiltered plan has its own tiling
    big = (ctypes.c_int * 3)(256, 2000, 256)
    n = 400000
    assert ws(0, 101, big, 1, 1, 1, n) > lib.stito_mrstft_workspace_bytes(big, 1, 1, 1, n) > 0
    assert table(0, 0, 101, big, 1, 1, n) > lib.stito_mrstft_table_floats(big, 1, 1, n) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the taps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 44100])
def test_the_aw_design(sr):
    from scipy import signal
    from st_ito import features as F
    taps = F.mrstft_prefilter("aw", sr)
    assert taps.shape == (101,) and taps.dtype == np.float32 and np.array_equal(taps, taps[::-1])
    _, h = signal.freqz(taps.astype(np.float64), worN=[100, 1000, 4000, 10000, 20000], fs=sr)
    db = 20 * np.log10(np.abs(h))
    print(f"aw at {sr} Hz: {np.round(db, 2)} dB at 100 / 1000 / 4000 / 10000 / 20000 Hz")
    assert abs(db[1]) <= 0.5 and db[4] < -20 and -12 < db[0] < -6 and 0 < db[2] < 2
    assert np.array_equal(F.mrstft_prefilter(taps), taps) and np.array_equal(F.mrstft_prefilter(torch.from_numpy(taps)), taps)
    assert "include_nyquist" in F.mrstft_prefilter.__doc__


def test_prefilter_refusals():
    from st_ito import features as F
    for bad, match in (([], "odd"), (np.ones(4), "odd"), (np.ones(257), "at most 255"), ([1.0, np.nan, 0.0], "finite"),
                       ([1.0, np.inf, 0.0], "finite"), ("a-weighting", "unknown prefilter"), (np.ones((3, 3)), "1-D")):
        with pytest.raises(ValueError, match=match):
            F.mrstft_prefilter(bad, 48000)
    with pytest.raises(ValueError, match="sample_rate"):
        F.mrstft_prefilter("aw")
    assert F.mrstft_prefilter(np.ones(255)).shape == (255,) and F.mrstft_prefilter([2.0]).tolist() == [2.0]


def test_python_refusals_come_before_the_gpu():
    """On a machine without a GPU every one of these would otherwise fail with another error."""
    from st_ito import engine, effects as E
    from st_ito.features import PrefilteredMrstftTarget, compute_prefiltered_mrstft_distance as dist
    x = torch.zeros((2, 2, 4096))
    for call in (lambda **k: dist(x, x, **k), lambda **k: PrefilteredMrstftTarget(x, **k)):
        with pytest.raises(ValueError, match="odd"):
            call(prefilter=np.ones(4))
        with pytest.raises(ValueError, match="sample_rate"):
            call(prefilter="aw")
        with pytest.raises(ValueError, match="kind"):
            call(prefilter="aw", sample_rate=48000, kind="side")
        with pytest.raises(ValueError, match="band 0 of 128"):
            call(prefilter="aw", sample_rate=48000, kind="mel", n_bins=128)
    with pytest.raises(ValueError, match="2 channels"):
        dist(x[:, :1], x[:, :1], "aw", 48000, kind="sum-diff")
    with pytest.raises(ValueError, match="too few"):
        dist(torch.zeros((1, 2, 1024)), torch.zeros((1, 2, 1024)), "aw", 48000)
    with pytest.raises(ValueError):
        dist(x, torch.zeros((2, 2, 4095)), "aw", 48000)
    for kw, match in ((dict(prefilter=np.ones(2)), "odd"), (dict(kind="mel", n_bins=128), "band 0 of 128"), (dict(kind="m/s"), "kind")):
        with pytest.raises(ValueError, match=match):
            engine.PrefilteredMrstftEvaluator(x[:1], 48000, E.make_plugins("eq"), x[:1], **kw)


def test_signatures():
    from st_ito import engine, features
    p = inspect.signature(features.compute_prefiltered_mrstft_distance).parameters
    assert list(p) == ["x", "y", "prefilter", "sample_rate", "kind", "n_bins", "resolutions"]
    assert p["kind"].default == "lr" and p["n_bins"].default == 64 and p["sample_rate"].default is None
    assert list(inspect.signature(features.mrstft_prefilter).parameters) == ["spec", "sample_rate"]
    assert issubclass(features.PrefilteredMrstftTarget, features.MrstftTarget) and issubclass(engine.PrefilteredMrstftEvaluator, engine.MrstftEvaluator)
    for name in ("update", "loss"):
        assert getattr(features.PrefilteredMrstftTarget, name) is getattr(features.MrstftTarget, name)
    p = inspect.signature(engine.PrefilteredMrstftEvaluator.__init__).parameters
    assert list(p)[-3:] == ["kind", "prefilter", "n_bins"] and p["prefilter"].default == "aw" and p["kind"].default == "lr"


# ---------------------------------------------------------------------------------------------------------------------------
# the drivers: refusals, the evaluator they build, the CLI
# ---------------------------------------------------------------------------------------------------------------------------
def _no_evaluator(monkeypatch):
    from st_ito import engine
    B._no_evaluator(monkeypatch)
    for name in ("MelMrstftEvaluator", "PrefilteredMrstftEvaluator"):
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
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    _no_evaluator(monkeypatch)
    kw = dict(distance=distance, popsize=4, max_iters=2, seed=0)
    run = lambda **over: (lambda *a: run_es(*a, find_w0=False, **dict(kw, **over)))   # noqa: E731
    _untouched(run(), _es_args(tgt_n=4000), f"distance '{distance}' compares sample spans")
    _untouched(run(), _es_args(chs=2, tgt_chs=1), f"distance '{distance}'")
    _untouched(run(dropout=0.1), _es_args(), f"'{distance}' has no embeddings: dropout")
    _untouched(run(savepop=True), _es_args(), f"'{distance}' does not write populations")
    _untouched(run(device_es=True), _es_args(tgt_n=4000), "sample spans")
    for other in ("mrstft-AW", "aw", "mrstft_aw", "mrstft-aw-sd"):
        _untouched(run(distance=other), _es_args(), "Unknown distance")
    _untouched(lambda *a: run_staged_es(*a, **kw), _es_args(tgt_n=4000), "sample spans")
    _untouched(lambda *a: run_staged_es(*a, savepop=True, **kw), _es_args(), "savepop")
    _untouched(lambda *a: run_es_batch(*a, **kw), _es_args(tgt_n=4000), "target 0")
    every = (run(), run(device_es=True), lambda *a: run_staged_es(*a, **kw), lambda *a: run_es_batch(*a, **kw),
             lambda x, t, *a: run_es_batch([x[0]], [t[0]], *a, **kw))
    if distance == "mrstft-sd-aw":        # the 2-channel rule
        for call in every:
            _untouched(call, _es_args(chs=1), "distance 'mrstft-sd-aw' compares the sums and differences of 2 channels")
    if distance == "mrstft-mel-aw":       # the empty-band rule (n_fft 512 at 96 kHz)
        for call in every:
            _untouched(call, _es_args(sr=96000), r"mel band 0 of 64 has no non-zero weight at resolution \(512, 50, 240\) and sample rate 96000")


class _StandIn(B._StandInEvaluator):
    def __init__(self, *args, **kw):
        self.n_positional, self.kw = len(args), dict(kw)
        super().__init__(*args, **kw)


@pytest.fixture
def stand_in(monkeypatch):
    from st_ito import engine, style_transfer
    B._StandInEvaluator.built = []
    no = lambda *a, **k: (_ for _ in ()).throw(AssertionError("another evaluator"))   # noqa: E731
    monkeypatch.setattr(engine, "PrefilteredMrstftEvaluator", _StandIn)
    for name in ("MrstftEvaluator", "MelMrstftEvaluator", "PopulationEvaluator"):
        monkeypatch.setattr(engine, name, no)
    monkeypatch.setattr(engine, "RaggedInputs", B._StandInRagged)
    monkeypatch.setattr(engine, "_current_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(style_transfer, "process_audio",
                        lambda x, w, sr, plugins, normalize_stages=False: (np.asarray(x) * np.float32(1 + float(np.sum(w)))).astype(np.float32))
    return _StandIn


@pytest.mark.parametrize("distance,kind", zip(NAMES, ("lr", "sum-diff", "mel")))
def test_each_name_reaches_every_driver_and_builds_its_evaluator(stand_in, tmp_path, distance, kind):
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    x, t = B._pair(0, 24000)
    x, t = torch.cat([x, 0.5 * x]), torch.cat([t, 0.5 * t])
    kw = dict(max_iters=2, popsize=4, sigma0=0.2, seed=1, distance=distance)
    run_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, find_w0=False, **kw)
    run_staged_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, run_dir=str(tmp_path), **kw)
    run_es_batch(torch.stack([x, x]), torch.stack([t, t]), SR, B._plugins(), None, None, **kw)
    run_es_batch([x, x], [t, t], SR, B._plugins(), None, None, **kw)
    assert len(stand_in.built) == 5                      # the staged ES builds one per stage
    for ev in stand_in.built:
        assert ev.n_positional == 4 and ev.kw == {"kind": kind, "prefilter": "aw"}, (distance, ev.n_positional, ev.kw)


def test_list_form_equals_run_es_on_the_stand_in(stand_in):
    from st_ito.style_transfer import run_es, run_es_batch
    lengths = [300000, 300000, 1000]
    pairs = [B._pair(b, n, silent=(b == 1)) for b, n in enumerate(lengths)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, early_stop=True, distance="mrstft-aw")
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
    with pytest.raises(SystemExit):
        p.parse_args(["in.wav", "--objective", "aw"])
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
    run_optim.main(argv + ["--objective", "mrstft-aw"])
    run_optim.main(argv + ["--objective", "mrstft-mel-aw", "--staged"])
    assert [kwargs["distance"] for _, kwargs in calls] == ["mrstft-aw", "mrstft-mel-aw"]
    assert all(args[4] is None and args[5] is None for args, _ in calls)        # model, embed_func


# ---------------------------------------------------------------------------------------------------------------------------
# the references and the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def test_prefilter64_is_conv1d_and_the_unit_tap_is_the_unfiltered_distance():
    import mrstft_cases as M
    import st_ito_oracle as O
    taps = A.seeded_taps(31, 5)
    rows = M.noise(5, 1, 2, 1025)[0]
    want = torch.nn.functional.conv1d(rows.to(torch.float64)[:, None], torch.from_numpy(taps).to(torch.float64)[None, None], padding=15)[:, 0]
    assert np.abs(A.prefilter64(rows.numpy(), taps) - want.numpy()).max() < 1e-14
    assert np.abs(A.prefilter32(rows, taps).numpy() - want.numpy()).max() < 1e-6
    x, y = M.noise(1, 1, 2, 2049), M.noise(2, 1, 2, 2049)
    assert A.error64("lr", x, y, [1.0]) == pytest.approx(O.mrstft_error(x, y), rel=1e-12)
    assert A.error64("lr", y, y, A.aw_taps()) == 0.0 and abs(A.error64("lr", x, y, A.aw_taps()) - O.mrstft_error(x, y)) > 1e-3


@pytest.mark.parametrize("form", A.FORMS)
def test_float32_yardstick_stays_within_1e4_of_the_float64_reference(form):
    yard = A.yardstick(form, A.aw_taps())
    for name, v in yard.items():
        print(f"{form:8s} {name:28s} float32 conv1d + torch.stft vs float64: {v:.3e}")
    worst = max(yard, key=yard.get)
    print(f"{form}: yardstick {yard[worst]:.3e} ({worst}), GPU bar {A.bar(form, A.aw_taps()):.3e}")
    assert [c[0] for c in A.cases(form)] == list(yard)
    assert all(np.isfinite(v) for v in yard.values()) and A.BAR_FACTOR == 4.0
    assert max(yard.values()) < 1e-4, yard


def test_yardstick_of_the_seeded_tap_sets():
    for n_taps, seed in ((31, 5), (255, 9)):
        yard = A.yardstick("lr", A.seeded_taps(n_taps, seed))
        worst = max(yard, key=yard.get)
        print(f"{n_taps} seeded taps: yardstick {yard[worst]:.3e} ({worst}), GPU bar {A.BAR_FACTOR * yard[worst]:.3e}")
        assert all(np.isfinite(v) for v in yard.values()) and yard[worst] < 1e-4


def test_the_wrong_readings_are_far_from_the_definition():
    """What tests/test_gpu_mrstft_aw.py relies on: with a 31-tap asymmetric filter, reversed taps and reflect-then-filter move the
    float64 value by far more than the bar."""
    import mrstft_cases as M
    taps = A.seeded_taps(31, 5)
    for name in ("noise-1025-c1-p1", "noise-2049-c1-p3"):
        _, x, y, norm_passes = [c for c in M.cases() if c[0] == name][0]
        ref = A.reference("lr", taps, name, x, y, norm_passes)
        rev = np.array([A.error64("lr", a, b, taps[::-1].copy()) for a, b in A.items(x, y, norm_passes)])
        rf = np.array([A.wrong_reflect_first64("lr", a, b, taps) for a, b in A.items(x, y, norm_passes)])
        bar = A.bar("lr", taps)                      # the yardstick of this tap set over the whole case set
        print(f"{name}: bar {bar:.3e}; reversed {np.abs(rev - ref) / ref}; reflect first {np.abs(rf - ref) / ref}")
        assert np.all(np.abs(rev - ref) / ref > 10 * bar) and np.all(np.abs(rf - ref) / ref > 10 * bar)
        # with a unit tap the reflect-first reading is the definition: the helper's framing is the reference's
        assert A.wrong_reflect_first64("lr", x[:1], y[:1] if y.shape[0] > 1 else y, [1.0]) == pytest.approx(
            A.error64("lr", x[:1], y[:1] if y.shape[0] > 1 else y, [1.0]), rel=1e-12)
