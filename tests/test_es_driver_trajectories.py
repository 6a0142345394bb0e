"""CPU pin of the ES drivers' host logic: run_es, both forms of run_es_batch and run_staged_es are driven on deterministic
stand-ins for the GPU evaluator (a quadratic bowl per pair) and for the ragged gather, and everything they decide on the host --
selected vectors, the pre-tell histories, the iteration at which the early stop fires, the evaluation counts, the population
shapes / pairs / crop starts the evaluator is handed (so: the order of every rng draw), the evaluator's constructor keywords
and the printed text -- is compared EXACTLY with tests/golden/es_driver_trajectories.npz.

The fixture was recorded on commit 3a20368 ("Batch the ES over pairs of different lengths with per-pair crops"), before the
drivers were put on one shared loop; `python tests/test_es_driver_trajectories.py --record` rewrites it from the tree it is
run in (to be done only when a change of behaviour is intended)."""
import contextlib
import io
import json
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "es_driver_trajectories.npz")
CROP, MARGIN = 262144, 16384


class _Log:
    """What the stand-ins saw during one run, and how the bowls of that run are shaped."""
    calls = []
    scales = [1.0]      # pair b's fitness is scales[b] * |w - goal|^2: a small scale is flat enough for the early stop
    goal = None         # a fixed optimum (run_staged_es); None = pair b's target value in every dimension


class _Evaluator:
    """Stands in for engine.PopulationEvaluator.  Without `x` it applies the reference's length policy itself (literally, not
    through the product's functions) on the rng it is handed, so the log holds every draw."""

    def __init__(self, x, sr, plugins, model, target_embeds, **kw):
        self.ndims = sum(p["num_params"] for p in plugins.values())
        self.B, self.n = x.shape[0], x.shape[-1]
        self.t = target_embeds["mid"].reshape(self.B, -1)[:, 0].double().numpy()
        _Log.calls.append(["init", list(x.shape), sorted(kw), repr(kw.get("use_graph"))])

    def evaluate(self, W, random_crop=False, rng=None, want_audio=False, dropout=0.0, parallel=False, pairs=None, x=None):
        W = np.asarray(W, dtype=np.float64)
        if x is None:
            start = 0
            if not parallel and random_crop and self.n - CROP > MARGIN:
                start = int(rng.randint(MARGIN, self.n - CROP))
            starts = [start]
        else:
            assert list(pairs) == x["pairs"]
            starts = x["starts"] + [x["crop_len"]]
        members = list(range(self.B)) if pairs is None else [int(b) for b in pairs]
        per = len(W) // len(members)
        f = []
        for i, w in enumerate(W):
            b = members[i // per]
            goal = self.t[b] if _Log.goal is None else _Log.goal[: W.shape[1]]
            f.append(_Log.scales[b] * float(np.sum((w - goal) ** 2)))
        _Log.calls.append(["evaluate", list(W.shape), members if pairs is not None else None, starts, dropout, want_audio, parallel])
        return torch.tensor(f, dtype=torch.float32), None, None

    def nan_warning(self):
        return None


class _Ragged:
    """Stands in for engine.RaggedInputs: no device buffer, a gather is a record of what was asked for."""

    def __init__(self, inputs, device):
        self.lengths = [int(x.shape[-1]) for x in inputs]
        _Log.calls.append(["ragged", self.lengths, str(device.type)])

    def gather(self, pairs, starts, crop_len):
        return {"pairs": [int(b) for b in pairs], "starts": [int(s) for s in starts], "crop_len": int(crop_len)}


def _embed(t, model, sr):            # a target's "embedding" is its second sample (the first one carries the peak)
    return dict(mid=t[:, :1, 1], side=t[:, :1, 1])


def _target(value, n=8):
    t = torch.full((1, 1, n), float(value))
    t[..., 0] = 1.0
    return t


def _drive(fn, scales=(1.0,), goal=None):
    """Run fn() on the stand-ins -> (its result, the calls the stand-ins saw as JSON, its stdout)."""
    from st_ito import _hip
    from st_ito import style_transfer as ST
    _Log.calls, _Log.scales, _Log.goal = [], list(scales), goal
    out = io.StringIO()
    with contextlib.ExitStack() as stack:
        stack.enter_context(mock.patch.object(ST.engine, "PopulationEvaluator", _Evaluator))
        stack.enter_context(mock.patch.object(ST.engine, "RaggedInputs", _Ragged))
        stack.enter_context(mock.patch.object(ST, "process_audio", lambda x, w, sr, plugins: np.asarray(x)))
        stack.enter_context(mock.patch.object(ST, "parameters_to_dict", lambda w, plugins: dict(w=[float(v) for v in w])))
        # the list form asks for the current GPU device before it builds its (here: stand-in) device buffers
        stack.enter_context(mock.patch.object(_hip, "require_gpu", lambda: None))
        stack.enter_context(mock.patch.object(torch.cuda, "current_device", lambda: 0))
        stack.enter_context(contextlib.redirect_stdout(out))
        res = fn(ST)
    return res, json.dumps(_Log.calls), out.getvalue()


def _pack(prefix, res, into):
    """One result dict -> arrays.  A history entry of None (es.result before the first tell) becomes a row of NaN."""
    D = len(res["wopt"])
    into[prefix + "wopt"] = np.asarray(res["wopt"], dtype=np.float64)
    into[prefix + "fopt"] = np.float64(res["fopt"])
    into[prefix + "fval_history"] = np.asarray(res["fval_history"], dtype=np.float64)
    rows = [np.full(D, np.nan) if w is None else np.asarray(w, dtype=np.float64) for w in res["wopt_history"]]
    into[prefix + "wopt_history"] = np.concatenate(rows)      # (run_staged_es: the rows of different stages differ in length)
    into[prefix + "wopt_history_row_lengths"] = np.array([len(r) for r in rows], dtype=np.int64)
    into[prefix + "wopt_history_is_none"] = np.array([w is None for w in res["wopt_history"]])
    into[prefix + "num_evals"] = np.int64(res["num_evals"])
    into[prefix + "params"] = np.asarray(res["params"]["w"], dtype=np.float64)
    into[prefix + "output_shape"] = np.asarray(res["output_audio"].shape, dtype=np.int64)
    into[prefix + "keys"] = np.array(json.dumps(list(res)))          # in the order the driver spells them
    if "stage_wopts" in res:
        into[prefix + "stage_wopts"] = np.concatenate(res["stage_wopts"])


PLUGINS = dict(fx=dict(num_params=4))


def _run_es(scales=(1.0,), n=1000, **kw):
    def fn(ST):
        return ST.run_es(torch.ones(1, 1, n), _target(0.7), 48000, PLUGINS, None, _embed, popsize=6, sigma0=0.3, **kw)
    res, calls, text = _drive(fn, scales)
    out = {"calls": np.array(calls), "stdout": np.array(text)}
    _pack("", res, out)
    return out


def _run_batch(lengths, random_crop, as_list, max_iters=40):
    """Three or more pairs whose bowls differ in steepness, so that they stop at different iterations."""
    B = len(lengths)
    scales = [1e-3, 1.0, 30.0, 0.05, 5.0][:B]
    values = np.linspace(0.2, 0.9, B)

    def fn(ST):
        if as_list:   # targets of two lengths: those of equal shape are embedded in one call
            xs = [torch.ones(1, 1, n) if b % 2 else torch.ones(1, n) for b, n in enumerate(lengths)]
            ts = [_target(v, 8 if b % 2 else 16) for b, v in enumerate(values)]
        else:
            xs = torch.ones(B, 1, lengths[0])
            ts = torch.cat([_target(v) for v in values])
        before = [t.clone() for t in ts]
        res = ST.run_es_batch(xs, ts, 48000, PLUGINS, None, _embed, max_iters=max_iters, sigma0=0.3, popsize=6,
                              random_crop=random_crop, seed=7, early_stop=True)
        assert all(torch.equal(a, b) for a, b in zip(before, ts))       # the batch works on clones
        return res
    res, calls, text = _drive(fn, scales)
    out = {"calls": np.array(calls), "stdout": np.array(text), "n_pairs": np.int64(len(res))}
    for b, r in enumerate(res):
        _pack(f"{b}/", r, out)
    return out


def _run_staged():
    plugins = {"a": dict(num_params=3), "b": dict(num_params=2), "c": dict(num_params=4)}
    goal = np.concatenate([np.full(3, 0.2), np.full(2, 0.8), np.full(4, 0.6)])

    def fn(ST):
        return ST.run_staged_es(torch.ones(1, 1, 8), _target(0.5), 48000, plugins, None, _embed, max_iters=31, popsize=8,
                                sigma0=0.3, seed=5, run_dir=None)
    res, calls, text = _drive(fn, goal=goal)
    out = {"calls": np.array(calls), "stdout": np.array(text)}
    _pack("", res, out)
    return out


LIST_LENGTHS = [1000, CROP + MARGIN - 1000, 300000, CROP, 400000]      # both sides of 262144 and of 262144 + 16384
RUNS = {
    # find_w0 and the crop positions come out of ONE RandomState; the flat bowl stops the run early
    "es_find_w0_crop_early_stop": lambda: _run_es((1e-3,), n=300000, max_iters=30, find_w0=True, random_crop=True, seed=3),
    "es_given_w0_early_stop": lambda: _run_es((1.0,), max_iters=60, find_w0=False, w0=torch.tensor([0.2, 0.4, 0.6, 0.8]), seed=11),
    # no early stop, dropout on every iteration but the last, the pool branch's length policy (nothing drawn)
    "es_default_w0_fixed_work": lambda: _run_es((1.0,), n=300000, max_iters=5, find_w0=False, random_crop=True, parallel=True,
                                                dropout=0.25, early_stop=False, seed=2),
    "batch_tensor_long_crop": lambda: _run_batch([300000] * 3, True, False),
    "batch_tensor_long": lambda: _run_batch([300000] * 3, False, False),
    "batch_tensor_inside_margin_crop": lambda: _run_batch([CROP + MARGIN] * 3, True, False),
    "batch_tensor_short_crop": lambda: _run_batch([1000] * 4, True, False),
    "batch_list_crop": lambda: _run_batch(LIST_LENGTHS, True, True),
    "batch_list": lambda: _run_batch(LIST_LENGTHS, False, True),
    "staged": _run_staged,
}


def record():
    """The fixture: per run ONE float64 vector with every number back to back and one JSON text with its layout and the strings
    (an .npz entry costs a few hundred bytes whatever it holds, and a run has dozens)."""
    out = {}
    for name, run in RUNS.items():
        layout, chunks, text = [], [], {}
        for key, value in run().items():
            value = np.asarray(value)
            if value.dtype.kind == "U":
                text[key] = str(value)
            else:
                layout.append([key, value.dtype.str, list(value.shape)])
                chunks.append(value.astype(np.float64).ravel())     # counts and flags are small integers: exact
        out[f"{name}/values"] = np.concatenate(chunks)
        out[f"{name}/meta"] = np.array(json.dumps({"layout": layout, "text": text}))
    return out


@pytest.fixture(scope="module")
def golden():
    """The fixture unpacked again: {"run/key": array}."""
    out = {}
    with np.load(FIXTURE, allow_pickle=False) as z:
        for name in RUNS:
            meta, values, at = json.loads(str(z[f"{name}/meta"])), z[f"{name}/values"], 0
            for key, dtype, shape in meta["layout"]:
                n = int(np.prod(shape, dtype=np.int64))
                out[f"{name}/{key}"] = values[at:at + n].astype(dtype).reshape(shape)
                at += n
            assert at == len(values)
            out.update({f"{name}/{key}": np.array(value) for key, value in meta["text"].items()})
    return out


@pytest.mark.parametrize("name", list(RUNS))
def test_driver_trajectory_is_the_recorded_one(name, golden):
    got = {f"{name}/{k}": v for k, v in RUNS[name]().items()}
    assert sorted(got) == sorted(k for k in golden if k.startswith(name + "/"))
    for key, value in got.items():
        want = golden[key]
        if want.dtype.kind == "U":                      # stdout, the stand-ins' call log, the result's keys
            assert str(value) == str(want), key
        elif want.ndim == 0 and want.dtype.kind == "f":
            assert float(value) == float(want), key
        else:
            np.testing.assert_array_equal(np.asarray(value), want, err_msg=key)


def test_the_recorded_runs_cover_what_they_are_meant_to(golden):
    """The fixture itself: the early stop fired before max_iters, at different iterations for the pairs of a batch; some pairs
    drew crops and some did not; the first history entry is es.result before the first tell."""
    assert sorted({k.split("/")[0] for k in golden}) == sorted(RUNS)
    assert int(golden["es_find_w0_crop_early_stop/num_evals"]) == 6 + 12 * 6          # find_w0 + iterations 0 .. 11
    assert "Stopping early due to no improvement." in str(golden["es_find_w0_crop_early_stop/stdout"])
    assert 6 < int(golden["es_given_w0_early_stop/num_evals"]) < 60 * 6
    assert int(golden["es_default_w0_fixed_work/num_evals"]) == 5 * 6
    for name in ("batch_tensor_long_crop", "batch_tensor_long", "batch_list_crop", "batch_list"):
        n = int(golden[f"{name}/n_pairs"])
        evals = [int(golden[f"{name}/{b}/num_evals"]) for b in range(n)]
        assert n >= 3 and len(set(evals)) >= 3 and max(evals) < 40 * 6, evals
        assert bool(golden[f"{name}/0/wopt_history_is_none"][0]) and np.isinf(golden[f"{name}/0/fval_history"][0])
    starts = [c[3][0] for c in json.loads(str(golden["batch_tensor_long_crop/calls"])) if c[0] == "evaluate"]
    assert len(set(starts)) > 3 and all(MARGIN <= s < 300000 - CROP for s in starts)
    for name in ("batch_tensor_long", "batch_tensor_inside_margin_crop", "batch_tensor_short_crop"):
        assert {c[3][0] for c in json.loads(str(golden[f"{name}/calls"])) if c[0] == "evaluate"} == {0}
    drew = set()
    for c in json.loads(str(golden["batch_list_crop/calls"])):
        if c[0] == "evaluate":
            drew |= {b for b, s in zip(c[2], c[3][:-1]) if s}
    assert drew == {2, 4}                              # only the inputs with more than 16384 spare samples draw
    assert not bool(golden["staged/wopt_history_is_none"].any())     # run_staged_es records after tell


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_es_driver_trajectories.py --record")
    for p in (os.path.join(ROOT, "st-ito_amd"),):
        sys.path.insert(0, p)
    np.savez_compressed(FIXTURE, **record())
    print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
