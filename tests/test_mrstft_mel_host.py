"""Host side of the mel-scaled MR-STFT objective (distance="mrstft-mel"; csrc/mrstft.hip's MEL variant): the ABI declarations,
the bank and its refusals, which all come before anything needs a GPU, the CLI, the drivers on the CPU stand-in of
tests/test_mrstft_batch_host.py, and the yardstick that tests/test_gpu_mrstft_mel.py measures the kernel with.

The yardstick: over the inputs of tests/mrstft_cases.py, at 48 kHz with 64 bands, the float32 restatement (torch.stft on the CPU,
a float32 bank product) stays within 1e-5 of the float64 one, item by item.  1e-5 is what float32 allows, not what was measured:
unit roundoff 6e-8 times the 11 butterfly stages of n_fft 2048, a band sum of up to 125 terms and the float32 reductions over
frames x bands (pairwise, 14 levels) is 9e-6.  Measured: 4.0e-7 at most (the two-tone signals; <= 1.9e-7 on noise, 7.4e-8 on the
all-zero target channel).  Every case is finite.  BAR_FACTOR = 4 times the measured maximum is the GPU test's bar, so a broken
restatement cannot widen it silently."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import mrstft_cases as M
import mrstft_mel_ref as R
import test_mrstft_batch_host as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = R.SR
NEW = ("stito_mrstft_table_floats_mel", "stito_mrstft_target_mel", "stito_mrstft_loss_mel", "stito_mrstft_loss_slots_mel")


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
        assert re.search(r"^\| .*`%s`.* \| .*eval_synthetic\.py:72" % name, integration, re.M), f"{name} has no row in INTEGRATION.md's map"
    assert "`stito_version_minor()` **8**" in integration
    assert "8 = stito_mel_bank, stito_mrstft_table_floats_mel" in header and "typedef struct stito_mel_bank" in header
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 8
    sig = _hip.SIGNATURES
    # the L/R calls' arguments with the bank after n_res (the size: with n_bins there); the workspace is the L/R size function's
    for name in ("target", "loss", "loss_slots"):
        old, new = sig[f"stito_mrstft_{name}"], sig[f"stito_mrstft_{name}_mel"]
        assert new[0] == old[0] and new[1][:2] == old[1][:2] and new[1][3:] == old[1][2:] and new[1][2] == ctypes.POINTER(_hip.MelBank)
    assert sig["stito_mrstft_table_floats_mel"][1] == sig["stito_mrstft_table_floats"][1][:2] + [ctypes.c_int] + sig["stito_mrstft_table_floats"][1][2:]
    assert "stito_mrstft_workspace_bytes_mel" not in sig and "stito_mrstft_workspace_bytes holds" in header


def test_the_struct_has_the_headers_layout():
    from st_ito import _hip
    assert ctypes.sizeof(_hip.MelBank) == 8 + 5 * 8 + 8 * 8 + 8 * 4 + 8 * 4
    assert _hip.MelBank.w_offset.offset == 48 and _hip.MelBank.w_stride.offset == 112 and _hip.MelBank.w_rows.offset == 144


def test_the_mel_table_is_smaller_than_the_linear_one():
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    lin = lib.stito_mrstft_table_floats(res, n_res, 2, 12345)
    mel = lib.stito_mrstft_table_floats_mel(res, n_res, 64, 2, 12345)
    assert 0 < mel < lin
    frames = [1 + 12345 // hop for _, hop, _ in R.RESOLUTIONS]
    assert lin - mel == 2 * sum((t * (n // 2 + 1) + 1) // 2 * 2 - t * 64 for t, (n, _, _) in zip(frames, R.RESOLUTIONS))
    for n_bins in (0, -1, 257):
        assert lib.stito_mrstft_table_floats_mel(res, n_res, n_bins, 2, 12345) == 0
    assert lib.stito_mrstft_table_floats_mel(res, n_res, 64, 2, 1024) == 0            # too few samples for n_fft 2048


def _c_bank(banks, n_bins=None):
    """A stito_mel_bank over host tables; the device pointers are never read by a refused call."""
    from st_ito import _hip
    start = np.ascontiguousarray(np.stack([b[0] for b in banks]).astype(np.int32))
    length = np.ascontiguousarray(np.stack([b[1] for b in banks]).astype(np.int32))
    c = _hip.MelBank()
    c.n_bins, c.n_res = (start.shape[1] if n_bins is None else n_bins), len(banks)
    c.band_start = start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    c.band_len = length.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    c.band_start_dev = c.band_len_dev = c.weights_dev = 64           # not null; a refusal comes before any of them is used
    off = 0
    for i, b in enumerate(banks):
        c.w_offset[i], c.w_stride[i], c.w_rows[i] = off, b[2].shape[1], b[2].shape[0]
        off += b[2].size
    return c, (start, length)


def test_entry_points_refuse_a_bad_bank_on_the_host():
    """n_bins outside [1, 256], a band longer than the bins, a band that starts beyond them (or runs past them): STITO_E_INVALID
    from all three calls, naming the band, before a device is asked anything (this test has none)."""
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)

    def statuses(c):
        ref = ctypes.byref(c)
        return (lib.stito_mrstft_target_mel(res, n_res, ref, None, 1, 4097, None, None),
                lib.stito_mrstft_loss_mel(res, n_res, ref, None, None, 0, None, 1, 1, 1, 4097, None, None, 0, None),
                lib.stito_mrstft_loss_slots_mel(res, n_res, ref, None, None, 0, None, 1, None, 1, 1, 1, 4097, None, None, 0, None))

    def changed(i, m, start=None, length=None):
        bank = [tuple(a.copy() for a in b) for b in F.mel_mrstft_bank(SR)]
        if start is not None:
            bank[i][0][m] = start
        if length is not None:
            bank[i][1][m] = length
        return bank

    for bank, n_bins, word in ((changed(0, 0), 0, b"n_bins 0"), (changed(0, 0), 257, b"n_bins 257"), (changed(0, 0), -3, b"n_bins -3"),
                               (changed(2, 63, length=258), None, b"band 63 of resolution 2 (n_fft 512) is 258 bins long"),
                               (changed(0, 63, length=64), None, b"band 63 of resolution 0 (n_fft 1024) is 64 bins long"),   # 63 weight rows
                               (changed(2, 5, start=257, length=1), None, b"band 5 of resolution 2 (n_fft 512) starts at bin 257"),
                               (changed(1, 7, start=1024, length=2), None, b"band 7 of resolution 1 (n_fft 2048) starts at bin 1024 with 2"),
                               (changed(1, 7, start=-1), None, b"band 7 of resolution 1")):
        c, keep = _c_bank(bank, n_bins)
        assert statuses(c) == (_hip.E_INVALID,) * 3, (word, lib.stito_last_error())
        assert word in lib.stito_last_error(), lib.stito_last_error()
    c, keep = _c_bank(F.mel_mrstft_bank(SR))
    c.n_res = 2
    assert statuses(c) == (_hip.E_INVALID,) * 3 and b"covers 2 resolutions" in lib.stito_last_error()
    c, keep = _c_bank(F.mel_mrstft_bank(SR))                                   # a good bank: the slot call still wants its slot list
    assert statuses(c)[2] == _hip.E_INVALID and b"target_slot_dev" in lib.stito_last_error()
    assert lib.stito_mrstft_target_mel(res, n_res, None, None, 1, 4097, None, None) == _hip.E_INVALID and b"null bank" in lib.stito_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# the bank
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 44100])
def test_default_bank_has_no_empty_filter(sr):
    """64 (the default) and 80 bands at the three default resolutions; every band is one run of consecutive bins and the tables
    say what the matrix says."""
    from st_ito import features as F
    from st_ito.models.panns import _mel_filterbank
    assert F.MEL_MRSTFT_BINS == 64 and inspect.signature(F.mel_mrstft_bank).parameters["n_bins"].default == 64
    for n_bins in (64, 80):
        banks = F.mel_mrstft_bank(sr, n_bins) if n_bins != 64 else F.mel_mrstft_bank(sr)
        assert len(banks) == 3
        for (n_fft, _, _), (start, length, w) in zip(F.MRSTFT_RESOLUTIONS, banks):
            mat = _mel_filterbank(sr, n_fft, n_bins, 0.0, sr / 2)
            assert mat.shape == (n_bins, n_fft // 2 + 1) and start.dtype == length.dtype == np.int32 and w.dtype == np.float32
            assert w.shape == (length.max(), n_bins) and length.min() >= 1 and np.all(start + length <= n_fft // 2 + 1)
            back = np.zeros_like(mat)
            for m in range(n_bins):
                run = w[: length[m], m]
                assert np.all(run > 0) and np.all(w[length[m]:, m] == 0)      # one run, no hole in it; zero padded
                back[m, start[m]: start[m] + length[m]] = run
            assert np.array_equal(back, mat)
            assert start[n_bins - 1] + length[n_bins - 1] == n_fft // 2 + 1 and 0 < mat[n_bins - 1, -1] < 1e-15   # the Nyquist bin is kept


def test_banks_with_empty_filters_are_refused_naming_band_resolution_and_rate():
    from st_ito import features as F
    with pytest.raises(ValueError, match=r"band 0 of 128 .*\(512, 50, 240\).*sample rate 48000 \(13 empty"):
        F.mel_mrstft_bank(48000, 128)
    for sr, n_bins, count in ((48000, 96, 3), (44100, 96, 2), (44100, 128, 11)):
        with pytest.raises(ValueError, match=rf"\(512, 50, 240\).*sample rate {sr} \({count} empty"):
            F.mel_mrstft_bank(sr, n_bins)
    with pytest.raises(ValueError, match=r"\(256, 30, 120\).*\(7 empty"):
        F.mel_mrstft_bank(48000, 64, [(256, 30, 120)])
    with pytest.raises(ValueError, match=r"\(256, 30, 120\).*\(6 empty"):
        F.mel_mrstft_bank(44100, 64, [(1024, 120, 600), (256, 30, 120)])
    for n_bins in (0, 257, -1):
        with pytest.raises(ValueError, match="n_bins"):
            F.mel_mrstft_bank(48000, n_bins)
    with pytest.raises(ValueError, match="n_fft 300"):
        F.mel_mrstft_bank(48000, 64, [(300, 30, 120)])


def test_python_refusals_come_before_the_gpu():
    """On a machine without a GPU every one of these would otherwise fail with another error."""
    from st_ito import engine, effects as E
    from st_ito.features import MelMrstftTarget, compute_mel_mrstft_distance
    x = torch.zeros((2, 2, 4096))
    with pytest.raises(ValueError, match="band 0 of 128"):
        compute_mel_mrstft_distance(x, x, 48000, 128)
    with pytest.raises(ValueError, match="band 0 of 128"):
        MelMrstftTarget(x, 48000, 128)
    with pytest.raises(ValueError, match="band 0 of 128"):
        engine.MelMrstftEvaluator(x[:1], 48000, E.make_plugins("eq"), x[:1], n_bins=128)
    with pytest.raises(ValueError, match="n_bins"):
        compute_mel_mrstft_distance(x, x, 48000, 300)
    with pytest.raises(ValueError):
        compute_mel_mrstft_distance(x[0], x[0], 48000)                            # compute_mrstft_distance's shape rules
    with pytest.raises(ValueError):
        compute_mel_mrstft_distance(x, torch.zeros((2, 2, 4095)), 48000)
    with pytest.raises(ValueError):
        compute_mel_mrstft_distance(torch.zeros((3, 2, 4096)), x, 48000)
    with pytest.raises(ValueError, match="too few"):
        compute_mel_mrstft_distance(torch.zeros((1, 2, 1024)), torch.zeros((1, 2, 1024)), 48000)


def test_signatures():
    from st_ito import engine, features
    from st_ito.style_transfer import run_es_batch
    assert list(inspect.signature(features.compute_mel_mrstft_distance).parameters) == ["x", "y", "sample_rate", "n_bins", "resolutions"]
    p = inspect.signature(features.compute_mel_mrstft_distance).parameters
    assert p["n_bins"].default == 64 and p["resolutions"].default is None
    # the pinned ones are what they were
    assert list(inspect.signature(features.compute_mrstft_distance).parameters) == ["x", "y", "resolutions"]
    assert list(inspect.signature(features.compute_sd_mrstft_distance).parameters) == ["x", "y", "resolutions"]
    assert list(inspect.signature(features.MrstftTarget.__init__).parameters) == ["self", "y", "resolutions", "stereo"]
    params = inspect.signature(engine.MrstftEvaluator.__init__).parameters
    assert list(params)[-1] == "stereo" and params["stereo"].default == "lr"
    assert list(inspect.signature(run_es_batch).parameters)[-1] == "distance"
    assert issubclass(features.MelMrstftTarget, features.MrstftTarget) and issubclass(engine.MelMrstftEvaluator, engine.MrstftEvaluator)
    assert inspect.signature(engine.MelMrstftEvaluator.__init__).parameters["n_bins"].default == 64
    for name in ("update", "loss"):
        assert getattr(features.MelMrstftTarget, name) is getattr(features.MrstftTarget, name)
    assert list(inspect.signature(features.MelMrstftTarget.loss).parameters)[-2:] == ["slots", "ws"]   # ws: the evaluator's Workspace
    # the base class builds its tables in one place
    src = inspect.getsource(engine.MrstftEvaluator)
    assert src.count("MrstftTarget(y,") == 1 and src.count("self._target_table(y)") == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the drivers: refusals, the evaluator they build, the CLI
# ---------------------------------------------------------------------------------------------------------------------------
def _no_evaluator(monkeypatch):
    from st_ito import engine
    B._no_evaluator(monkeypatch)
    monkeypatch.setattr(engine, "MelMrstftEvaluator", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an evaluator was built")))


def _es_args(n=4096, chs=2, tgt_chs=None, tgt_n=None, sr=SR):
    x = torch.rand((1, chs, n)) - 0.5
    t = torch.rand((1, tgt_chs or chs, tgt_n or n)) - 0.5
    return x, t, sr, B._plugins(), None, None


def _untouched(call, args, match):
    keep = [a.clone() for a in args[:2]]
    with pytest.raises(ValueError, match=match):
        call(*args)
    assert all(torch.equal(a, b) for a, b in zip(keep, args[:2]))


def test_driver_refusals_come_before_any_launch(monkeypatch):
    """The pair rules, content_model, dropout and savepop as under "mrstft", with this distance's name; an empty band (n_fft 512
    at 96 kHz) before an input is normalised."""
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    _no_evaluator(monkeypatch)
    kw = dict(distance="mrstft-mel", popsize=4, max_iters=2, seed=0)
    run = lambda **over: (lambda *a: run_es(*a, find_w0=False, **dict(kw, **over)))   # noqa: E731
    _untouched(run(), _es_args(tgt_n=4000), "distance 'mrstft-mel' compares sample spans")
    _untouched(run(), _es_args(chs=2, tgt_chs=1), "distance 'mrstft-mel': the target has 1 channels, the chain renders 2")
    _untouched(lambda *a: run_es(*a, content_model=object(), content_embed_func=lambda *a: {}, **kw), _es_args(), "'mrstft-mel' has no embeddings: content_model")
    _untouched(run(dropout=0.1), _es_args(), "'mrstft-mel' has no embeddings: dropout")
    _untouched(run(savepop=True), _es_args(), "'mrstft-mel' does not write populations")
    _untouched(run(device_es=True), _es_args(tgt_n=4000), "sample spans")
    for other in ("mrstft-MEL", "mel", "mrstft_mel", ""):
        _untouched(run(distance=other), _es_args(), "Unknown distance")
    for call in (run(), run(device_es=True), lambda *a: run_staged_es(*a, **kw), lambda *a: run_es_batch(*a, **kw),
                 lambda x, t, *a: run_es_batch([x[0]], [t[0]], *a, **kw)):
        _untouched(call, _es_args(sr=96000), r"mel band 0 of 64 has no non-zero weight at resolution \(512, 50, 240\) and sample rate 96000")
    _untouched(lambda *a: run_staged_es(*a, **kw), _es_args(tgt_n=4000), "sample spans")
    _untouched(lambda *a: run_staged_es(*a, savepop=True, **kw), _es_args(), "savepop")
    _untouched(lambda *a: run_es_batch(*a, **kw), _es_args(tgt_n=4000), "target 0")
    _untouched(lambda x, t, *a: run_es_batch([x[0]], [t[0]], *a, **kw), _es_args(chs=2, tgt_chs=1), "target 0 has 1 channels")


class _StandIn(B._StandInEvaluator):
    """The stand-in evaluator, remembering the class name it was asked for and the arguments it was built with."""

    def __init__(self, *args, **kw):
        self.n_positional, self.kw = len(args), dict(kw)
        super().__init__(*args, **kw)


class _MelStandIn(_StandIn):
    pass


@pytest.fixture
def stand_in(monkeypatch):
    from st_ito import engine, style_transfer
    B._StandInEvaluator.built = []
    monkeypatch.setattr(engine, "MrstftEvaluator", _StandIn)
    monkeypatch.setattr(engine, "MelMrstftEvaluator", _MelStandIn)
    monkeypatch.setattr(engine, "RaggedInputs", B._StandInRagged)
    monkeypatch.setattr(engine, "_current_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(engine, "PopulationEvaluator", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the embedding evaluator")))
    monkeypatch.setattr(style_transfer, "process_audio",
                        lambda x, w, sr, plugins, normalize_stages=False: (np.asarray(x) * np.float32(1 + float(np.sum(w)))).astype(np.float32))
    return _StandIn


def test_each_distance_builds_its_evaluator(stand_in, tmp_path):
    """"mrstft-mel" builds engine.MelMrstftEvaluator with the four positional arguments and no keyword (n_bins is the default);
    "mrstft" and "mrstft-sd" build what they built."""
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    x, t = B._pair(0, 24000)
    x, t = torch.cat([x, 0.5 * x]), torch.cat([t, 0.5 * t])
    kw = dict(max_iters=2, popsize=4, sigma0=0.2, seed=1)
    for distance, cls, want in (("mrstft-mel", _MelStandIn, {}), ("mrstft", _StandIn, {}), ("mrstft-sd", _StandIn, {"stereo": "sum-diff"})):
        stand_in.built.clear()
        run_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, distance=distance, find_w0=False, **kw)
        run_staged_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, distance=distance, run_dir=str(tmp_path), **kw)
        run_es_batch(torch.stack([x, x]), torch.stack([t, t]), SR, B._plugins(), None, None, distance=distance, **kw)
        run_es_batch([x, x], [t, t], SR, B._plugins(), None, None, distance=distance, **kw)
        assert len(stand_in.built) == 5                      # the staged ES builds one per stage
        for ev in stand_in.built:
            assert type(ev) is cls and ev.n_positional == 4 and ev.kw == want, (distance, type(ev), ev.n_positional, ev.kw)


@pytest.mark.parametrize("random_crop,lengths", [(True, [200000, 270000, 400000]), (False, [300000, 300000, 1000])])
def test_list_form_equals_run_es_on_the_stand_in(stand_in, random_crop, lengths):
    from st_ito.style_transfer import run_es, run_es_batch
    pairs = [B._pair(b, n, silent=(b == 1)) for b, n in enumerate(lengths)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, random_crop=random_crop, early_stop=True)
    res = run_es_batch(xs, ts, SR, B._plugins(), None, None, seed=7, distance="mrstft-mel", **kw)
    ev = stand_in.built[0]
    assert len(stand_in.built) == 1 and type(ev) is _MelStandIn
    assert {how for _, how in ev.calls} == ({"moving"} if random_crop else {"static"})
    for b in range(len(lengths)):
        one = run_es(xs[b].clone()[None], ts[b].clone()[None], SR, B._plugins(), None, None, distance="mrstft-mel", find_w0=False,
                     seed=7 + b, **kw)
        B._same_run(res[b], one)
        assert res[b]["num_evals"] == (48 if b == 1 else 60)


def test_objective_flag_and_the_call_main_builds(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    from st_ito.audio_io import save_wav
    p = run_optim.build_parser()
    assert p.parse_args(["in.wav", "--objective", "mrstft-mel"]).objective == "mrstft-mel"
    assert p.parse_args(["in.wav"]).objective == "embedding"
    with pytest.raises(SystemExit):
        p.parse_args(["in.wav", "--objective", "mel"])
    assert not any("bins" in a.dest for a in p._actions)                       # no other new flag: n_bins is the default
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
    run_optim.main(argv + ["--objective", "mrstft-mel"])
    run_optim.main(argv + ["--objective", "mrstft-mel", "--staged"])
    run_optim.main(argv + ["--objective", "mrstft"])
    today = ["max_iters", "popsize", "w0", "find_w0", "sigma0", "distance", "parallel", "dropout", "savepop", "normalize_stages", "run_dir",
             "seed", "early_stop"]
    for (args, kwargs), distance in zip(calls, ("mrstft-mel", "mrstft-mel", "mrstft")):
        assert list(kwargs) == today and kwargs["distance"] == distance
        assert args[4] is None and args[5] is None        # model, embed_func


# ---------------------------------------------------------------------------------------------------------------------------
# the references and the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def test_float64_restatement_with_the_identity_bank_is_the_linear_oracle():
    """M = I |X| is |X|: the restatement's framing, window and clamp are oracle.mrstft_error's."""
    import st_ito_oracle as O
    x, y = M.noise(1, 1, 2, 2049), M.noise(2, 1, 2, 2049)
    banks = [np.eye(n // 2 + 1, dtype=np.float32) for n, _, _ in R.RESOLUTIONS]
    assert R.mel_error64(x, y, banks=banks) == pytest.approx(O.mrstft_error(x, y), rel=1e-12)
    assert R.mel_error64(y, y) == 0.0 and R.mel_error64(x, y) > 0.1
    assert abs(R.mel_error64(x, y) - O.mrstft_error(x, y)) > 1e-3            # and the mel distance is another number


def test_the_clamp_rows_no_longer_carry_a_mono_compatible_target():
    """What the distance is for: on a target with one silent channel the linear distance is carried by that row's bins on the
    clamp; band sums of a clamped row are still small against a live estimate, but the log term is taken over 64 bands a frame,
    not 257 - 1025 bins."""
    import st_ito_oracle as O
    name, x, y, norm_passes = [c for c in M.cases() if c[0] == "zero-target-channel-1025"][0]
    lin = np.array([O.mrstft_error(x[p:p + 1], y) for p in range(x.shape[0])])
    mel = R.reference(name, x, y, norm_passes)
    print(f"zero target channel: linear {lin}, mel {mel}")
    assert np.all(np.isfinite(mel)) and np.all(mel < lin)


def test_float32_yardstick_stays_within_1e5_of_the_float64_restatement():
    yard = R.yardstick()
    for name, v in yard.items():
        print(f"{name:28s} float32 torch.stft + float32 bank vs float64: {v:.3e}")
    print(f"yardstick {R.yardstick_max():.3e}, GPU bar {R.BAR_FACTOR * R.yardstick_max():.3e}")
    assert [c[0] for c in M.cases()] == list(yard) and len(yard) == 13
    assert all(np.isfinite(v) for v in yard.values())                        # every case is finite, the clamp cases included
    assert R.BAR_FACTOR == 4.0 and (R.SR, R.N_BINS) == (48000, 64)
    assert R.yardstick_max() < 1e-5, yard
