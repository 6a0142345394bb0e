"""Host side of the sum / difference MR-STFT objective (distance="mrstft-sd"; csrc/mrstft.hip's SD variant): the ABI
declarations, the refusals that come before anything needs a GPU, the CLI, the drivers' logic on the CPU stand-in of
tests/test_mrstft_batch_host.py (extended to remember how it was built), and the yardstick on the inputs of
tests/mrstft_sd_cases.py that tests/test_gpu_mrstft_sd.py measures the kernel with.

The yardstick is not a new one: the float32 restatement scripts/eval_synthetic.mrstft_error applied to (sd(x), sd(y)) has to
stay within mrstft_cases.yardstick_max() -- the L/R set's own worst case, 3.64e-6 -- of the float64 oracle on the same pair."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import mrstft_cases as M
import mrstft_sd_cases as SD
import st_ito_oracle as O
import test_mrstft_batch_host as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000
NEW = ("stito_mrstft_target_sd", "stito_mrstft_loss_sd", "stito_mrstft_loss_slots_sd")
OLD = ("stito_mrstft_table_floats", "stito_mrstft_target", "stito_mrstft_workspace_bytes", "stito_mrstft_loss", "stito_mrstft_loss_slots")


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_in_header_binding_and_library():
    from st_ito import _hip
    header = open(os.path.join(ROOT, "include", "stito_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.lib()
    for name in NEW + OLD:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in integration
    assert "7 = stito_mrstft_target_sd" in header
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 7
    sig = _hip.SIGNATURES
    # the loss calls take their L/R counterparts' arguments; the table call names targets and channels where that one names rows
    assert sig["stito_mrstft_loss_sd"] == sig["stito_mrstft_loss"]
    assert sig["stito_mrstft_loss_slots_sd"] == sig["stito_mrstft_loss_slots"]
    assert len(sig["stito_mrstft_target_sd"][1]) == len(sig["stito_mrstft_target"][1]) + 1


def test_entry_points_refuse_other_channel_counts_on_the_host():
    """Channel counts other than 2 are STITO_E_INVALID, with a message that says so, before a device is asked anything."""
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    for ch in (1, 3, 0):
        assert lib.stito_mrstft_target_sd(res, n_res, None, 1, ch, 4096, None, None) == _hip.E_INVALID
        assert b"2 channels" in lib.stito_last_error() and str(ch).encode() in lib.stito_last_error()
    assert lib.stito_mrstft_loss_slots_sd(res, n_res, None, None, 0, None, 1, None, 1, 4, 2, 4096, None, None, 0, None) == _hip.E_INVALID
    assert b"target_slot_dev" in lib.stito_last_error()
    # the sizes are those of the L/R calls at C = 2: there are no size functions of its own
    assert not any(name.endswith("_sd") and ("floats" in name or "bytes" in name) for name in _hip.SIGNATURES)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _es_args(n=4096, chs=2, tgt_chs=None, tgt_n=None):
    from st_ito import effects as E
    x = torch.rand((1, chs, n)) - 0.5
    t = torch.rand((1, tgt_chs or chs, tgt_n or n)) - 0.5
    return x, t, SR, E.make_plugins("eq-comp", with_bypass=True), None, None


def _untouched(call, args, match):
    keep = [a.clone() for a in args[:2]]
    with pytest.raises(ValueError, match=match):
        call(*args)
    assert all(torch.equal(a, b) for a, b in zip(keep, args[:2]))


def test_run_es_refusals_come_before_any_launch(monkeypatch):
    from st_ito.style_transfer import run_es
    B._no_evaluator(monkeypatch)
    kw = dict(distance="mrstft-sd", popsize=4, max_iters=1, find_w0=False, seed=0)
    run = lambda **over: (lambda *a: run_es(*a, **dict(kw, **over)))   # noqa: E731
    _untouched(run(), _es_args(chs=1), "channels")                      # a mono chain
    with pytest.raises(ValueError, match=r"2 channels.*renders 1 channels"):
        run_es(*_es_args(chs=1), **kw)
    _untouched(run(device_es=True), _es_args(chs=1), "channels")
    _untouched(run(), _es_args(tgt_n=4000), "length")
    _untouched(run(), _es_args(chs=2, tgt_chs=1), "target has 1 channels, the chain renders 2")
    _untouched(lambda *a: run_es(*a, content_model=object(), content_embed_func=lambda *a: {}, **kw), _es_args(), "content_model")
    _untouched(run(dropout=0.1), _es_args(), "dropout")
    _untouched(run(savepop=True), _es_args(), "savepop")
    for other in ("mrstft-SD", "sd", "l2", "MRSTFT", ""):
        _untouched(run(distance=other), _es_args(), "Unknown distance")


def test_run_es_batch_refusals_come_before_any_evaluator(monkeypatch):
    from st_ito.style_transfer import run_es_batch
    B._no_evaluator(monkeypatch)
    kw = dict(max_iters=1, popsize=4, seed=0, distance="mrstft-sd")
    rnd = lambda *shape: torch.rand(shape) - 0.5       # noqa: E731

    def refused(xs, ts, match, **over):
        keep = [a.clone() for a in (*xs, *ts)] if isinstance(xs, list) else [xs.clone(), ts.clone()]
        with pytest.raises(ValueError, match=match):
            run_es_batch(xs, ts, SR, B._plugins(), None, None, **dict(kw, **over))
        now = [*xs, *ts] if isinstance(xs, list) else [xs, ts]
        assert all(torch.equal(a, b) for a, b in zip(keep, now))

    for other in ("mrstft-SD", "sd", "l2"):
        refused(rnd(2, 2, 4096), rnd(2, 2, 4096), "Unknown distance", distance=other)
        refused([rnd(2, 4096)], [rnd(2, 4096)], "Unknown distance", distance=other)
    refused(rnd(2, 1, 4096), rnd(2, 1, 4096), "2 channels: the chain renders 1 channels")          # mono chain, tensor form
    refused([rnd(1, 4096), rnd(1, 5000)], [rnd(1, 4096), rnd(1, 5000)], "2 channels: the chain renders 1 channels")
    refused([rnd(2, 4096), rnd(2, 5000), rnd(2, 4096)], [rnd(2, 4096), rnd(2, 4999), rnd(2, 4096)], "target 1")
    refused(rnd(2, 2, 4096), rnd(2, 2, 4000), "target 0")
    refused([rnd(2, 4096), rnd(2, 5000)], [rnd(2, 4096), rnd(1, 5000)], "target 1 has 1 channels")
    refused(rnd(2, 2, 4096), rnd(2, 1, 4096), "channels")


def test_run_staged_es_refuses_a_stage_that_is_not_stereo(monkeypatch):
    from st_ito.style_transfer import run_staged_es
    B._no_evaluator(monkeypatch)
    kw = dict(max_iters=2, popsize=4, seed=0, distance="mrstft-sd")
    rnd = lambda *shape: torch.rand(shape) - 0.5       # noqa: E731

    def refused(x, t, match, plugins=None, **over):
        x0, t0 = x.clone(), t.clone()
        with pytest.raises(ValueError, match=match):
            run_staged_es(x, t, SR, plugins or B._plugins(), None, None, **dict(kw, **over))
        assert torch.equal(x, x0) and torch.equal(t, t0)

    # mono input into a chain that turns stereo at its second plugin: the full chain renders 2 channels, stage 0 does not
    refused(rnd(1, 1, 4096), rnd(1, 2, 4096), r"2 channels: stage 0 .* renders 1 channels", plugins=B._stereo_later_plugins())
    refused(rnd(1, 1, 4096), rnd(1, 1, 4096), "channels")
    refused(rnd(1, 2, 4096), rnd(1, 2, 4000), "length")
    refused(rnd(1, 2, 4096), rnd(1, 2, 4096), "savepop", savepop=True)
    refused(rnd(1, 2, 4096), rnd(1, 2, 4096), "Unknown distance", distance="sd")


def test_features_refuse_other_channel_counts():
    from st_ito.features import MrstftTarget, compute_sd_mrstft_distance
    for chs in (1, 3):
        x = torch.zeros((2, chs, 4096))
        with pytest.raises(ValueError, match="2 channels"):
            compute_sd_mrstft_distance(x, x)
        with pytest.raises(ValueError, match="2 channels"):
            MrstftTarget(x, stereo="sum-diff")
    x = torch.zeros((2, 2, 4096))
    with pytest.raises(ValueError):
        compute_sd_mrstft_distance(x[0], x[0])                                   # compute_mrstft_distance's shape rules
    with pytest.raises(ValueError):
        compute_sd_mrstft_distance(x, torch.zeros((2, 2, 4095)))
    with pytest.raises(ValueError):
        compute_sd_mrstft_distance(torch.zeros((3, 2, 4096)), x)
    with pytest.raises(ValueError, match="too few"):
        compute_sd_mrstft_distance(torch.zeros((1, 2, 1024)), torch.zeros((1, 2, 1024)))
    with pytest.raises(ValueError, match="stereo"):
        MrstftTarget(x, stereo="ms")
    import inspect
    from st_ito import engine, features
    assert list(inspect.signature(features.compute_mrstft_distance).parameters) == ["x", "y", "resolutions"]
    assert list(inspect.signature(compute_sd_mrstft_distance).parameters) == ["x", "y", "resolutions"]
    assert inspect.signature(MrstftTarget.__init__).parameters["stereo"].default == "lr"
    params = inspect.signature(engine.MrstftEvaluator.__init__).parameters
    assert list(params)[-1] == "stereo" and params["stereo"].default == "lr"


# ---------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_objective_flag_and_the_call_main_builds(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    from st_ito.audio_io import save_wav
    p = run_optim.build_parser()
    assert p.parse_args(["in.wav", "--objective", "mrstft-sd"]).objective == "mrstft-sd"
    assert p.parse_args(["in.wav"]).objective == "embedding"
    with pytest.raises(SystemExit):
        p.parse_args(["in.wav", "--objective", "l2"])
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
    run_optim.main(argv + ["--objective", "mrstft-sd"])
    run_optim.main(argv + ["--objective", "mrstft-sd", "--staged"])
    run_optim.main(argv + ["--objective", "mrstft"])
    today = ["max_iters", "popsize", "w0", "find_w0", "sigma0", "distance", "parallel", "dropout", "savepop", "normalize_stages", "run_dir",
             "seed", "early_stop"]
    for (args, kwargs), distance in zip(calls, ("mrstft-sd", "mrstft-sd", "mrstft")):
        assert list(kwargs) == today and kwargs["distance"] == distance
        assert args[4] is None and args[5] is None        # model, embed_func


# ---------------------------------------------------------------------------------------------------------------------------
# driver logic on the CPU stand-in
# ---------------------------------------------------------------------------------------------------------------------------
class _StandIn(B._StandInEvaluator):
    """The stand-in evaluator, remembering the arguments it was built with."""

    def __init__(self, *args, **kw):
        self.n_positional, self.kw = len(args), dict(kw)
        super().__init__(*args, **kw)


@pytest.fixture
def stand_in(monkeypatch):
    from st_ito import engine, style_transfer
    B._StandInEvaluator.built = []
    monkeypatch.setattr(engine, "MrstftEvaluator", _StandIn)
    monkeypatch.setattr(engine, "RaggedInputs", B._StandInRagged)
    monkeypatch.setattr(engine, "_current_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(engine, "PopulationEvaluator", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the embedding evaluator")))
    monkeypatch.setattr(style_transfer, "process_audio",
                        lambda x, w, sr, plugins, normalize_stages=False: (np.asarray(x) * np.float32(1 + float(np.sum(w)))).astype(np.float32))
    return _StandIn


def _pair(b, n, silent=False):
    """test_mrstft_batch_host._pair with a second channel: the chain has to render 2 under "mrstft-sd"."""
    x, t = B._pair(b, n, silent)
    return torch.cat([x, 0.5 * x]), torch.cat([t, 0.5 * t])


def _alone(x, t, b, seed, distance, **kw):
    from st_ito.style_transfer import run_es
    return run_es(x.clone()[None], t.clone()[None], SR, B._plugins(), None, None, distance=distance, find_w0=False, seed=seed + b, **kw)


def test_each_distance_builds_its_evaluator(stand_in, tmp_path):
    """"mrstft-sd" adds stereo="sum-diff"; "mrstft" keeps the four positional arguments and no keyword."""
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    x, t = _pair(0, 24000)
    kw = dict(max_iters=2, popsize=4, sigma0=0.2, seed=1)
    for distance, want in (("mrstft-sd", {"stereo": "sum-diff"}), ("mrstft", {})):
        stand_in.built.clear()
        run_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, distance=distance, find_w0=False, **kw)
        run_staged_es(x[None].clone(), t[None].clone(), SR, B._plugins(), None, None, distance=distance, run_dir=str(tmp_path), **kw)
        run_es_batch(torch.stack([x, x]), torch.stack([t, t]), SR, B._plugins(), None, None, distance=distance, **kw)
        run_es_batch([x, x], [t, t], SR, B._plugins(), None, None, distance=distance, **kw)
        assert len(stand_in.built) == 5                      # the staged ES builds one per stage
        for ev in stand_in.built:
            assert ev.n_positional == 4 and ev.kw == want, (distance, ev.n_positional, ev.kw)


@pytest.mark.parametrize("random_crop,lengths", [(True, [200000, 270000, 400000, 300000]), (False, [300000, 300000, 350000, 1000])])
def test_list_form_equals_run_es_on_the_stand_in(stand_in, random_crop, lengths):
    """The list form under "mrstft-sd" takes the paths it takes under "mrstft": moving crops, or static groups read through
    the slot list; pair 1 stops early; pair b is the run_es of pair b alone."""
    from st_ito.style_transfer import run_es_batch
    pairs = [_pair(b, n, silent=(b == 1)) for b, n in enumerate(lengths)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, random_crop=random_crop, early_stop=True)
    res = run_es_batch(xs, ts, SR, B._plugins(), None, None, seed=7, distance="mrstft-sd", **kw)
    ev = stand_in.built[0]
    assert len(stand_in.built) == 1 and ev.kw == {"stereo": "sum-diff"}
    assert {how for _, how in ev.calls} == ({"moving"} if random_crop else {"static"})
    assert any(1 in members for members, _ in ev.calls[:4]) and not any(1 in members for members, _ in ev.calls[-3:])
    for b in range(len(lengths)):
        B._same_run(res[b], _alone(xs[b], ts[b], b, 7, "mrstft-sd", **kw))
        assert res[b]["num_evals"] == (48 if b == 1 else 60)
    assert ev.rendered_candidates == 48 + 3 * 60


def test_tensor_form_equals_run_es_on_the_stand_in(stand_in):
    from st_ito.style_transfer import run_es_batch
    import inspect
    pairs = [_pair(b, 24000, silent=(b == 1)) for b in range(3)]
    xs, ts = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, early_stop=True)
    res = run_es_batch(xs, ts, SR, B._plugins(), None, None, seed=3, distance="mrstft-sd", **kw)
    ev = stand_in.built[0]
    assert all(members == [0, 1, 2] and how == "own" for members, how in ev.calls) and len(ev.calls) == 15
    for b in range(3):
        B._same_run(res[b], _alone(xs[b], ts[b], b, 3, "mrstft-sd", **kw))
        assert res[b]["num_evals"] == (48 if b == 1 else 60)
    assert list(inspect.signature(run_es_batch).parameters)[-1] == "distance"


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def test_definition_on_the_flipped_pair():
    """The reason for the distance: a render whose right channel has the opposite polarity scores 0 channel by channel."""
    g = torch.Generator().manual_seed(0)
    x = torch.tanh(torch.randn((1, 2, 4097), generator=g))
    y = x.clone()
    y[:, 1] = -x[:, 1]
    assert O.mrstft_error(x, y) == 0.0
    assert O.mrstft_error(SD.sd(x), SD.sd(y)) > 1.0


def test_float32_restatement_stays_within_the_lr_yardstick():
    names = [c[0] for c in SD.cases()]
    stereo = [c[0] for c in M.cases() if c[1].shape[1] == 2]
    assert names[:len(stereo)] == stereo and len(stereo) == 8 and "zero-candidate-1200" in stereo
    assert sorted({c[1].shape[-1] for c in M.cases() if c[0].startswith("noise") and c[1].shape[1] == 2}) == [1200, 2048, 4097, 12000]
    assert names[len(stereo):] == ["sd-mono-target-1025", "sd-antiphase-target-1025", "sd-peak-folded-2049"]
    yard, bound = SD.yardstick(), M.yardstick_max()
    for name, v in yard.items():
        print(f"{name:28s} float32 torch.stft on (sd x, sd y) vs float64 oracle: {v:.3e}  (yardstick {bound:.3e})")
    mono = SD.reference(*[c for c in SD.cases() if c[0] == "sd-mono-target-1025"][0])
    print(f"sd-mono-target-1025: oracle {mono}")
    assert np.all(mono > 1e4)                                  # the difference row on the clamp carries the item
    anti = SD.reference(*[c for c in SD.cases() if c[0] == "sd-antiphase-target-1025"][0])
    np.testing.assert_allclose(anti, mono, rtol=1e-12)         # channel 1 negated on both sides: the two rows change places
    assert len(yard) == len(names) and all(np.isfinite(v) for v in yard.values())
    assert max(yard.values()) <= bound, yard
