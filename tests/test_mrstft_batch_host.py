"""Host side of the MRSTFT objective for multi-pair batches and the staged ES: the ABI declaration of
stito_mrstft_loss_slots, the refusals of run_es_batch / run_staged_es(distance="mrstft") that come before anything needs a
GPU, the CLI, and the drivers' logic on a CPU stand-in for engine.MrstftEvaluator.

The stand-in's fitness is a deterministic function of a candidate and of ONE number of its pair's target (the target's
first sample, which survives the peak normalisation because a later sample carries the peak): whatever path a driver takes
to bring a pair's target to the evaluator -- its own tensors, a gathered crop, a static table and a slot list -- a pair's
trajectory can only equal run_es's if its candidates met its own target in every iteration."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000


def test_symbol_declared_in_header_binding_and_library():
    from st_ito import _hip
    header = open(os.path.join(ROOT, "include", "stito_hip.h")).read()
    assert re.search(r"\bstito_mrstft_loss_slots\s*\(", header)
    assert "5 = stito_mrstft_loss_slots" in header
    assert "stito_mrstft_loss_slots" in _hip.SIGNATURES
    # stito_mrstft_loss's arguments plus (target_slot_dev, n_slots)
    assert len(_hip.SIGNATURES["stito_mrstft_loss_slots"][1]) == len(_hip.SIGNATURES["stito_mrstft_loss"][1]) + 2
    lib = _hip.lib()
    getattr(lib, "stito_mrstft_loss_slots")
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 5
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "stito_mrstft_loss_slots" in integration


def test_slot_call_checks_its_arguments_on_the_host():
    """A null slot list is refused before the plan asks a device anything."""
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    assert lib.stito_mrstft_loss_slots(res, n_res, None, None, 0, None, 1, None, 1, 4, 1, 4096, None, None, 0, None) == _hip.E_INVALID
    assert b"target_slot_dev" in lib.stito_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _no_evaluator(monkeypatch):
    from st_ito import engine

    def no_evaluator(*a, **k):
        raise AssertionError("an evaluator was built")
    for name in ("MrstftEvaluator", "PopulationEvaluator", "RaggedInputs"):
        monkeypatch.setattr(engine, name, no_evaluator)


def _plugins(chain="eq-comp"):
    from st_ito import effects as E
    return E.make_plugins(chain, with_bypass=True)


def _stereo_later_plugins():
    """A mono stage, then a stereo one: a mono input leaves stage 0 mono and stage 1 stereo."""
    pl = _plugins("eq-comp")
    names = list(pl)
    pl[names[0]]["num_channels"], pl[names[1]]["num_channels"] = 1, 2
    return pl


def test_run_es_batch_refusals_come_before_any_evaluator(monkeypatch):
    from st_ito.style_transfer import run_es_batch
    _no_evaluator(monkeypatch)
    kw = dict(max_iters=1, popsize=4, seed=0, distance="mrstft")
    rnd = lambda *shape: torch.rand(shape) - 0.5       # noqa: E731  (peak < 1: a normalisation would change it)

    def refused(xs, ts, match, plugins=None, **over):
        keep = [a.clone() for a in (*xs, *ts)] if isinstance(xs, list) else [xs.clone(), ts.clone()]
        with pytest.raises(ValueError, match=match):
            run_es_batch(xs, ts, SR, plugins or _plugins(), None, None, **dict(kw, **over))
        now = [*xs, *ts] if isinstance(xs, list) else [xs, ts]
        assert all(torch.equal(a, b) for a, b in zip(keep, now))

    for other in ("l2", "MRSTFT", ""):
        refused(rnd(2, 1, 4096), rnd(2, 1, 4096), "Unknown distance", distance=other)
        refused([rnd(1, 4096)], [rnd(1, 4096)], "Unknown distance", distance=other)
    # a target whose length differs from its input's, naming the pair
    refused([rnd(1, 4096), rnd(1, 5000), rnd(1, 4096)], [rnd(1, 4096), rnd(1, 4999), rnd(1, 4096)], "target 1")
    refused(rnd(2, 1, 4096), rnd(2, 1, 4000), "target 0")
    # a target whose channel count is not the chain's output channel count
    refused([rnd(1, 4096), rnd(1, 5000)], [rnd(1, 4096), rnd(2, 5000)], "target 1 has 2 channels")
    refused(rnd(2, 1, 4096), rnd(2, 2, 4096), "channels")
    stereo = _stereo_later_plugins()
    refused([rnd(1, 4096)], [rnd(1, 4096)], "target 0 has 1 channels, the chain renders 2", plugins=stereo)
    refused(rnd(2, 1, 4096), rnd(2, 1, 4096), "the chain renders 2", plugins=stereo)


def test_run_staged_es_refusals_come_before_any_evaluator(monkeypatch):
    from st_ito.style_transfer import run_staged_es
    _no_evaluator(monkeypatch)
    kw = dict(max_iters=2, popsize=4, seed=0, distance="mrstft")
    rnd = lambda *shape: torch.rand(shape) - 0.5       # noqa: E731

    def refused(x, t, match, plugins=None, **over):
        x0, t0 = x.clone(), t.clone()
        with pytest.raises(ValueError, match=match):
            run_staged_es(x, t, SR, plugins or _plugins(), None, None, **dict(kw, **over))
        assert torch.equal(x, x0) and torch.equal(t, t0)

    refused(rnd(1, 1, 4096), rnd(1, 1, 4096), "Unknown distance", distance="l2")
    refused(rnd(1, 1, 4096), rnd(1, 1, 4000), "length")
    # mono input into a chain that turns stereo at its second plugin, stereo target: stage 0 renders mono
    refused(rnd(1, 1, 4096), rnd(1, 2, 4096), "stage 0", plugins=_stereo_later_plugins())
    # ... and with a mono target it is stage 1 that does not fit
    refused(rnd(1, 1, 4096), rnd(1, 1, 4096), "stage 1", plugins=_stereo_later_plugins())
    from st_ito.style_transfer import run_es
    with pytest.raises(ValueError) as e_run_es:
        run_es(rnd(1, 1, 4096), rnd(1, 1, 4096), SR, _plugins(), None, None, distance="mrstft", savepop=True, find_w0=False)
    for flag in ("savepop", "save_pop"):
        with pytest.raises(ValueError) as e:
            run_staged_es(rnd(1, 1, 4096), rnd(1, 1, 4096), SR, _plugins(), None, None, **dict(kw, **{flag: True}))
        assert str(e.value) == str(e_run_es.value) and "savepop" in str(e.value)


def test_run_optim_parser_keeps_the_reference_defaults():
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    p = run_optim.build_parser()
    a = p.parse_args(["in.wav", "t.wav"])
    assert (a.max_iters, a.popsize, a.max_length, a.effect_type, a.algorithm, a.metric, a.dropout) == (300, 32, 262144, "vst", "es", "param", 0.0)
    assert a.objective == "embedding" and a.staged is False and a.savepop is False
    b = p.parse_args(["in.wav", "--objective", "mrstft", "--staged"])
    assert b.objective == "mrstft" and b.staged is True
    src = open(os.path.join(ROOT, "st-ito_amd", "scripts", "run_optim.py")).read()
    assert "NotImplementedError(\"--objective mrstft" not in src      # --staged runs with this objective


# ---------------------------------------------------------------------------------------------------------------------------
# driver logic on a CPU stand-in
# ---------------------------------------------------------------------------------------------------------------------------
class _StandInEvaluator:
    """engine.MrstftEvaluator's interface on the CPU.  Fitness of candidate w of a pair whose target's first sample is a:
    mean (w - a)^2 - 0.2 per earlier evaluation of that pair (so a live pair beats its record by more than the stop rule's 0.01
    in every iteration), or the constant 1 for a pair with a < 0 (it goes stale at once and stops early).  The crop draws
    are the product's own (engine.crop_start)."""
    built = []

    def __init__(self, x, sample_rate, plugins, target_audio, **kw):
        self.plugins, self.x, self.y = plugins, x.clone(), target_audio.clone()
        self.n_inputs = x.shape[0]
        self.ndims = sum(p["num_params"] for p in plugins.values())
        self.static = {}
        self.calls = []          # (pairs, how the targets came)
        self.seen = {}           # pair -> number of its evaluations so far
        self.rendered_candidates = 0
        type(self).built.append(self)

    def set_static_targets(self, length, pairs, y):
        assert tuple(y.shape[::2]) == (len(pairs), length)
        self.static[length] = {b: float(y[k, 0, 0]) for k, b in enumerate(pairs)}

    def nan_warning(self):
        return None

    def evaluate(self, W, random_crop=False, rng=np.random, want_audio=False, dropout=0.0, parallel=False, pairs=None, x=None, y=None):
        from st_ito import engine
        W = np.asarray(W, dtype=np.float64)
        assert W.ndim == 2 and W.shape[1] == self.ndims and not want_audio and dropout == 0.0
        if x is None:       # the evaluator's own audio: one crop draw per call, as the product
            assert y is None
            start = engine.crop_start(self.x.shape[-1], random_crop, rng)
            members = list(range(self.n_inputs)) if pairs is None else list(pairs)
            firsts, how = [float(self.y[b, 0, start]) for b in members], "own"
        elif y is not None:
            assert x.shape[0] == y.shape[0] == len(pairs) and x.shape[-1] == y.shape[-1]
            members, firsts, how = list(pairs), [float(y[k, 0, 0]) for k in range(len(pairs))], "moving"
        else:
            members, firsts, how = list(pairs), [self.static[x.shape[-1]][b] for b in pairs], "static"
        per = W.shape[0] // len(members)
        assert per * len(members) == W.shape[0]
        self.calls.append((members, how))
        self.rendered_candidates += W.shape[0]
        loss = []
        for k, (b, a) in enumerate(zip(members, firsts)):
            seen = self.seen.get(b, 0)
            self.seen[b] = seen + 1
            loss += [1.0 if a < 0 else float(np.mean((w - a) ** 2)) - 0.2 * seen for w in W[k * per:(k + 1) * per]]
        return torch.tensor(loss, dtype=torch.float64), {}, None


class _StandInRagged:
    """engine.RaggedInputs on the CPU: torch slicing + zero padding."""

    def __init__(self, inputs, device):
        self.inputs = [x.clone() for x in inputs]
        self.channels = int(inputs[0].shape[0])
        self.lengths = [int(x.shape[-1]) for x in inputs]
        self.n_launches = 0

    def gather(self, pairs, starts, crop_len):
        self.n_launches += 1
        out = []
        for b, s in zip(pairs, starts):
            part = self.inputs[b][:, s:s + crop_len]
            out.append(torch.nn.functional.pad(part, (0, crop_len - part.shape[-1])))
        return torch.stack(out)


@pytest.fixture
def stand_in(monkeypatch):
    from st_ito import engine, style_transfer
    _StandInEvaluator.built = []
    monkeypatch.setattr(engine, "MrstftEvaluator", _StandInEvaluator)
    monkeypatch.setattr(engine, "RaggedInputs", _StandInRagged)
    monkeypatch.setattr(engine, "_current_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(engine, "PopulationEvaluator", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the embedding evaluator")))
    # the final render: any deterministic function of (input, solution)
    monkeypatch.setattr(style_transfer, "process_audio",
                        lambda x, w, sr, plugins, normalize_stages=False: (np.asarray(x) * np.float32(1 + float(np.sum(w)))).astype(np.float32))
    return _StandInEvaluator


def _pair(b, n, silent=False):
    """Input and target of n samples whose target keeps `first` at sample 0 -- and, because a crop may start anywhere, a ramp
    of distinct values behind it; sample n - 1 carries the peak 1."""
    x = torch.linspace(-0.5, 0.5, n).reshape(1, n) * (0.5 + 0.1 * b)
    t = (0.1 + 0.07 * b + 0.6 * torch.arange(n, dtype=torch.float32) / n).reshape(1, n)
    if silent:
        t = -t
    t[0, -1] = 1.0
    return x, t


def _same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert len(got["wopt_history"]) == len(one["wopt_history"])
    for a, b in zip(got["wopt_history"], one["wopt_history"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


def _alone(x, t, b, seed, **kw):
    from st_ito.style_transfer import run_es
    return run_es(x.clone()[None], t.clone()[None], SR, _plugins(), None, None, distance="mrstft", find_w0=False, seed=seed + b, **kw)


@pytest.mark.parametrize("random_crop,lengths", [(True, [200000, 270000, 400000, 300000]), (False, [300000, 300000, 350000, 1000])])
def test_list_form_equals_run_es_on_the_stand_in(stand_in, random_crop, lengths):
    """Pair 1 has the constant fitness: it stops after iteration 11, and from then on it is neither gathered nor scored.  Under
    random_crop the one group moves (400000 and 300000 draw their crops): targets come as gathered crops; without it there are
    three static groups whose targets were gathered once."""
    from st_ito.style_transfer import run_es_batch
    pairs = [_pair(b, n, silent=(b == 1)) for b, n in enumerate(lengths)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    keep = [a.clone() for a in (*xs, *ts)]
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, random_crop=random_crop, early_stop=True)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=7, distance="mrstft", **kw)
    assert all(torch.equal(a, b) for a, b in zip(keep, (*xs, *ts)))          # peak normalisation on clones
    ev = stand_in.built[0]
    assert len(stand_in.built) == 1
    assert {how for _, how in ev.calls} == ({"moving"} if random_crop else {"static"})
    assert any(1 in members for members, _ in ev.calls[:4]) and not any(1 in members for members, _ in ev.calls[-3:])
    for b in range(len(lengths)):
        one = _alone(xs[b], ts[b], b, 7, **kw)
        _same_run(res[b], one)
        assert res[b]["num_evals"] == (48 if b == 1 else 60)
        assert res[b]["output_audio"].shape[-1] == lengths[b]
    assert ev.rendered_candidates == 48 + 3 * 60                            # stopped pairs are no longer rendered


def test_tensor_form_equals_run_es_on_the_stand_in(stand_in):
    """No crop is drawn at this length, so the promise holds; the stopped pair keeps being evaluated (and is no longer told)."""
    from st_ito.style_transfer import run_es_batch
    n = 24000
    pairs = [_pair(b, n, silent=(b == 1)) for b in range(3)]
    xs, ts = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    x0, t0 = xs.clone(), ts.clone()
    kw = dict(max_iters=15, sigma0=0.2, popsize=4, early_stop=True)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=3, distance="mrstft", **kw)
    assert torch.equal(xs, x0) and torch.equal(ts, t0)
    ev = stand_in.built[0]
    assert all(members == [0, 1, 2] and how == "own" for members, how in ev.calls) and len(ev.calls) == 15
    for b in range(3):
        _same_run(res[b], _alone(xs[b], ts[b], b, 3, **kw))
        assert res[b]["num_evals"] == (48 if b == 1 else 60)
    # positional callers of the embedding objective are unaffected: distance is the last keyword
    import inspect
    params = list(inspect.signature(run_es_batch).parameters)
    assert params[-1] == "distance" and params[-2] == "early_stop"
    assert inspect.signature(run_es_batch).parameters["distance"].default == "cosine"


def test_staged_asks_stage_k_for_sub_chain_0_to_k(stand_in, tmp_path):
    from st_ito.style_transfer import run_staged_es
    plugins = _plugins("eq-comp")
    names = list(plugins)
    dims = [plugins[k]["num_params"] for k in names]
    x, t = _pair(0, 24000)
    res = run_staged_es(x[None].clone(), t[None].clone(), SR, plugins, None, None, max_iters=6, popsize=4, sigma0=0.2, seed=5,
                        distance="mrstft", run_dir=str(tmp_path))
    assert [list(ev.plugins) for ev in stand_in.built] == [names[:1], names[:2]]        # stage k: plugins[0 .. k]
    assert [ev.ndims for ev in stand_in.built] == [dims[0], dims[0] + dims[1]]          # composed vectors (evaluate asserts the width)
    assert [len(ev.calls) for ev in stand_in.built] == [3, 3]                           # max_iters // len(plugins) per stage
    assert res["num_evals"] == 24 and len(res["fval_history"]) == 6
    assert sorted(os.listdir(tmp_path)) == ["output_audio_stage_0.wav", "output_audio_stage_1.wav"]
    assert [len(w) for w in res["stage_wopts"]] == dims
    np.testing.assert_array_equal(res["wopt"], np.concatenate(res["stage_wopts"]))
    assert list(res) == ["output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "stage_wopts", "num_evals"]
    # stage 1 held stage 0's optimum in front of every candidate: its best fitness is that of [stage_wopts[0], stage_wopts[1]]
    a = float(stand_in.built[1].y[0, 0, 0])
    assert res["fopt"] == float(np.mean((res["wopt"] - a) ** 2)) - 0.2 * 2      # found in the stage's third evaluation
