"""GPU: the MRSTFT objective in the multi-pair drivers -- stito_mrstft_loss_slots against stito_mrstft_loss on one-target tables
(bit for bit) and against the float64 oracle (the bar of tests/test_gpu_mrstft.py: BAR_FACTOR x the float32 restatement's own
distance from the oracle), MrstftEvaluator's subset call, both forms of run_es_batch(distance="mrstft") against run_es on
every pair alone (bit for bit), the early stop through the slot list, and run_staged_es(distance="mrstft").

The ES tests render at 262144 samples because the length policy pads to that; they keep pop 4 and mono."""
import os
import sys

import numpy as np
import pytest
import torch

import mrstft_cases as M
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
CROP = 262144
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_LISTS = ([2, 0], [1, 1, 1], [0, 1, 2])
PER = 2          # candidates per population


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def bar():
    return M.BAR_FACTOR * M.yardstick_max()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the slot kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _peaks(xd):
    from st_ito import _hip
    P, C, n = xd.shape
    peaks = torch.empty(P, dtype=torch.float32, device=xd.device)
    _hip.check(_hip.lib().stito_peak(_hip.ptr(xd), P, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return peaks


def _slot_loss(dev, x, y, slots, norm_passes):
    """stito_mrstft_loss_slots of x (len(slots) * PER, C, n) against the table of y (T, C, n) -> (P,) float32 on the host."""
    from st_ito.features import MrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    sd = torch.tensor(slots, dtype=torch.int32).to(dev)
    return MrstftTarget(yd).loss(xd, _peaks(xd) if norm_passes else None, norm_passes, slots=sd).cpu().numpy()


def _plain_loss(dev, x, y, norm_passes):
    """stito_mrstft_loss of x against the table of y (T dividing P)."""
    from st_ito.features import MrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    return MrstftTarget(yd).loss(xd, _peaks(xd) if norm_passes else None, norm_passes).cpu().numpy()


_SLOT_CASES = {}


def _slot_case(n, chs, norm_passes):
    """3 targets and, per slot list, its populations of 2 (seeded; the recipe of mrstft_cases.cases()) with the float64
    reference of every candidate against the target its slot names.  Computed once."""
    key = (n, chs, norm_passes)
    if key not in _SLOT_CASES:
        y = M.noise(900 + n, 3, chs, n)
        pops, refs = {}, {}
        for i, slots in enumerate(SLOT_LISTS):
            P = len(slots) * PER
            yy = y[[s for s in slots for _ in range(PER)]]
            x = (3.0 if norm_passes else 1.0) * torch.tanh(1.5 * yy + 0.2 * M.noise(910 + n + i, P, chs, n))
            xs = M.scored(x, norm_passes)
            pops[tuple(slots)] = x
            refs[tuple(slots)] = np.array([O.mrstft_error(xs[p:p + 1], y[slots[p // PER]][None]) for p in range(P)])
        _SLOT_CASES[key] = (y, pops, refs)
    return _SLOT_CASES[key]


@pytest.mark.parametrize("n,chs,norm_passes", [(2049, 2, 0), (1025, 1, 1)])
def test_slot_lists_equal_one_target_tables_and_the_oracle(dev, bar, n, chs, norm_passes):
    y, pops, refs = _slot_case(n, chs, norm_passes)
    for slots in SLOT_LISTS:
        x, ref = pops[tuple(slots)], refs[tuple(slots)]
        got = _slot_loss(dev, x, y, slots, norm_passes)
        assert got.shape == (len(slots) * PER,) and got.dtype == np.float32
        for k, s in enumerate(slots):      # the population of slot k alone, against a table that holds only its target
            alone = _plain_loss(dev, x[k * PER:(k + 1) * PER], y[s:s + 1], norm_passes)
            assert np.array_equal(got[k * PER:(k + 1) * PER], alone), (slots, k, got, alone)
        err = np.abs(got.astype(np.float64) - ref) / np.abs(ref)
        print(f"mrstft slots {slots} n {n} c{chs} norm {norm_passes}: max rel err {err.max():.3e}  (bar {bar:.3e})")
        assert np.all(np.isfinite(got)) and err.max() <= bar, (slots, got, ref, err)
    ident = [0, 1, 2]
    assert np.array_equal(_slot_loss(dev, pops[tuple(ident)], y, ident, norm_passes), _plain_loss(dev, pops[tuple(ident)], y, norm_passes))


def test_a_slot_that_names_no_target_gives_nan_for_its_population_only(dev):
    n, chs = 2049, 2
    y, pops, _ = _slot_case(n, chs, 0)
    x = pops[(0, 1, 2)]
    good = _slot_loss(dev, x, y, [0, 1, 2], 0)
    for slots, bad in (([0, 3, 2], 1), ([-1, 1, 2], 0), ([0, 1, 2 ** 31 - 1], 2), ([0, -2 ** 31, 2], 1)):
        got = _slot_loss(dev, x, y, slots, 0)
        for k in range(3):
            part = got[k * PER:(k + 1) * PER]
            if k == bad:
                assert np.all(np.isnan(part)), (slots, got)
            else:
                assert np.array_equal(part, good[k * PER:(k + 1) * PER]), (slots, got, good)
    assert np.array_equal(_slot_loss(dev, x, y, [0, 1, 2], 0), good)          # and the library works afterwards


def test_slot_call_refuses_bad_arguments_with_a_status(dev):
    from st_ito import _hip
    from st_ito.features import _mrstft_res
    lib = _hip.lib()
    res, n_res = _mrstft_res(None)
    n, pop, C, T = 4096, 4, 2, 3
    x = torch.zeros((pop, C, n), device=dev)
    table = torch.zeros(lib.stito_mrstft_table_floats(res, n_res, T * C, n), device=dev)
    ws = torch.zeros(lib.stito_mrstft_workspace_bytes(res, n_res, pop, C, n), dtype=torch.uint8, device=dev)
    out = torch.zeros(pop, device=dev)
    slots = torch.tensor([2, 0, 1, 1], dtype=torch.int32).to(dev)
    st = _hip.stream_ptr()
    assert lib.stito_mrstft_target(res, n_res, _hip.ptr(torch.zeros((T * C, n), device=dev)), T * C, n, _hip.ptr(table), st) == 0

    def loss(n_slots=2, slot_ptr=_hip.ptr(slots), n_targets=T, nn=n, ws_bytes=None, norm=0, k=n_res, ch=C):
        return lib.stito_mrstft_loss_slots(res, k, _hip.ptr(x), None, norm, _hip.ptr(table), n_targets, slot_ptr, n_slots, pop, ch, nn,
                                           _hip.ptr(out), _hip.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, st)

    def refused(rc, code):
        msg = lib.stito_last_error().decode()
        assert rc == code and msg, (rc, msg)

    assert loss() == 0 and loss(n_slots=4) == 0 and loss(n_slots=1) == 0
    refused(loss(n_slots=0), _hip.E_INVALID)
    refused(loss(n_slots=-1), _hip.E_INVALID)
    refused(loss(n_slots=3), _hip.E_INVALID)                         # pop % n_slots
    refused(loss(slot_ptr=None), _hip.E_INVALID)
    refused(loss(n_targets=0), _hip.E_INVALID)                       # the existing checks
    refused(loss(nn=1024), _hip.E_INVALID)
    refused(loss(k=0), _hip.E_INVALID)
    refused(loss(ch=9), _hip.E_INVALID)
    refused(loss(norm=1), _hip.E_INVALID)                            # norm_passes 1 without peaks
    refused(loss(ws_bytes=ws.numel() - 1), _hip.E_WORKSPACE)
    torch.cuda.synchronize()
    assert loss() == 0                                               # and the library still works
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the evaluator's subset call
# ---------------------------------------------------------------------------------------------------------------------------
def _plugins():
    from st_ito import effects as E
    return E.make_plugins("eq-comp")


def _target_of(x, seed):
    """The product's render of x (chs, n) at seeded parameters, (chs', n) float32 on the host."""
    from st_ito.style_transfer import process_audio
    return torch.from_numpy(process_audio(x.numpy(), np.random.default_rng(seed).random(22), SR, _plugins()))


def test_evaluator_scores_a_subset_of_its_pairs(dev):
    from st_ito.engine import MrstftEvaluator, RaggedInputs
    B, P, n = 3, 4, 24000
    xs = torch.stack([O.synth_audio(820 + b, 1, n) for b in range(B)])
    ts = torch.stack([_target_of(xs[b], 30 + b) for b in range(B)])
    ev = MrstftEvaluator(xs, SR, _plugins(), ts)
    W = np.random.default_rng(9).random((B * P, 22))
    full, embeds, audio = ev.evaluate(W)
    assert embeds == {} and audio is None and ev.rendered_candidates == B * P
    assert torch.isfinite(full).all() and float(full.min()) > 0
    Wsub = np.concatenate([W[2 * P:3 * P], W[0:P]])
    sub, _, _ = ev.evaluate(Wsub, pairs=[2, 0])
    assert ev.rendered_candidates == B * P + 2 * P                              # grew by the subset only
    assert torch.equal(sub, torch.cat([full[2 * P:3 * P], full[0:P]]))
    one, _, _ = ev.evaluate(W[P:2 * P], pairs=[1])
    assert torch.equal(one, full[P:2 * P]) and ev.rendered_candidates == B * P + 3 * P
    # ready-made buffers (zero padded to 262144 by the gather kernel, as the length policy pads): static and moving targets
    ri, rt = RaggedInputs([x for x in xs], dev), RaggedInputs([t for t in ts], dev)
    static, _, _ = ev.evaluate(Wsub, pairs=[2, 0], x=ri.gather([2, 0], [0, 0], CROP))
    assert torch.equal(static, sub)
    moving, _, _ = ev.evaluate(Wsub, pairs=[2, 0], x=ri.gather([2, 0], [0, 0], CROP), y=rt.gather([2, 0], [0, 0], CROP))
    assert torch.equal(moving, sub)
    with pytest.raises(ValueError):
        ev.evaluate(Wsub, pairs=[3, 0])
    with pytest.raises(ValueError):
        ev.evaluate(Wsub, pairs=[2, 0], x=ri.gather([2], [0], CROP))
    with pytest.raises(ValueError):
        ev.evaluate(Wsub, pairs=[2, 0], y=rt.gather([2, 0], [0, 0], CROP))       # target spans without their input spans


# ---------------------------------------------------------------------------------------------------------------------------
# 3 - 5. run_es_batch(distance="mrstft") = run_es on every pair alone
# ---------------------------------------------------------------------------------------------------------------------------
def _assert_same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert len(got["wopt_history"]) == len(one["wopt_history"])
    for a, b in zip(got["wopt_history"], one["wopt_history"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


def _alone(x, t, seed, **kw):
    from st_ito.style_transfer import run_es
    return run_es(x.clone(), t.clone(), SR, _plugins(), None, None, distance="mrstft", find_w0=False, seed=seed, **kw)


@pytest.mark.parametrize("random_crop,lengths", [(True, [200000, 270000, 400000]), (False, [300000, 300000, 350000])])
def test_list_form_batch_equals_run_es_on_every_pair_alone(dev, random_crop, lengths):
    """Padded (200000), cropped at 0 (270000) and randomly cropped (400000) pairs in one group whose spans move under
    random_crop (targets gathered at the inputs' starts, the table refilled); without it two static groups (slot lists)."""
    from st_ito import engine
    from st_ito.style_transfer import run_es_batch
    P, iters, seed = 4, 3, 23
    xs = [O.synth_audio(600 + b, 1, n)[None] * (0.5 + 0.1 * b) for b, n in enumerate(lengths)]
    ts = [_target_of(x[0], 70 + b)[None] for b, x in enumerate(xs)]
    assert len(engine.plan_ragged_groups(lengths, random_crop)) == (1 if random_crop else 2)
    keep = [(x.clone(), t.clone()) for x, t in zip(xs, ts)]
    kw = dict(max_iters=iters, sigma0=0.33, popsize=P, random_crop=random_crop, early_stop=False)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=seed, distance="mrstft", **kw)
    assert len(res) == len(lengths)
    for (x0, t0), x, t in zip(keep, xs, ts):         # the caller's tensors are not modified
        assert torch.equal(x0, x) and torch.equal(t0, t)
    for b in range(len(lengths)):
        one = _alone(xs[b], ts[b], seed + b, **kw)
        _assert_same_run(res[b], one)
        assert res[b]["num_evals"] == iters * P and res[b]["output_audio"].shape[-1] == lengths[b]
        assert all(np.isfinite(f) and f > 0 for f in res[b]["fval_history"][1:])


def test_list_form_early_stop_through_the_slot_list(dev):
    """Three mono pairs in one static group.  Driving the product's _EsRun on the CPU with oracle.process_audio and
    oracle.mrstft_error (float64, input and target zero padded to 262144 as the length policy pads them) gives: pair 0 improves
    on its record by 0.67, 0.34, 0.29 at iterations 1 - 3 and misses it by 0.2 or more in each of the ten iterations that
    follow (stale count 10 at the end: not more than 10, so all 14 iterations run, 56 evaluations); the silent pair 1 has a
    constant loss (spread exactly 0), is stale from iteration 1 and stops after iteration 11 (48 evaluations) -- from then
    on the slot list names pairs 0 and 2 only; pair 2 beats its record by 0.039, 0.152, 0.036 and 0.049 at iterations 2, 5,
    12 and 13 and never counts more than 6 stale iterations (56 evaluations).  The decision closest to the stale rule's
    threshold of 0.01 is pair 2's iteration 9 (an improvement of 0.0065: stale), 3.5e-3 away; float32 moves a loss by about
    1e-6."""
    from st_ito.style_transfer import run_es_batch
    lengths = [24000, 30000, 24000]
    xs = [O.synth_audio(900 + b, 1, n)[None] for b, n in enumerate(lengths)]
    ts = [_target_of(x[0], 50 + b)[None] for b, x in enumerate(xs)]       # made before pair 1's input is replaced
    xs[1] = torch.zeros_like(xs[1])
    kw = dict(popsize=4, sigma0=0.33, max_iters=14, early_stop=True)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=40, distance="mrstft", **kw)
    for b in range(3):
        h = res[b]["fval_history"]
        print(f"pair {b}: num_evals {res[b]['num_evals']}, record after iterations 0 - 3: {h[1:5]}")
    assert [r["num_evals"] for r in res] == [56, 48, 56]
    for b in range(3):
        _assert_same_run(res[b], _alone(xs[b], ts[b], 40 + b, **kw))


def test_tensor_form_batch_equals_run_es_on_every_pair_alone(dev):
    """(2, 1, 24000): no crop is drawn at this length, so the tensor form keeps the promise too."""
    from st_ito.style_transfer import run_es_batch
    xs = torch.stack([O.synth_audio(930 + b, 1, 24000) * (0.6 + 0.2 * b) for b in range(2)])
    ts = torch.stack([_target_of(xs[b], 60 + b) for b in range(2)])
    x0, t0 = xs.clone(), ts.clone()
    kw = dict(max_iters=3, sigma0=0.33, popsize=4, early_stop=False)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=11, distance="mrstft", **kw)
    assert torch.equal(xs, x0) and torch.equal(ts, t0)
    for b in range(2):
        _assert_same_run(res[b], _alone(xs[b][None], ts[b][None], 11 + b, **kw))
        assert res[b]["num_evals"] == 12


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the staged ES
# ---------------------------------------------------------------------------------------------------------------------------
def test_staged_es_with_the_mrstft_objective(dev, tmp_path):
    from st_ito.engine import MrstftEvaluator
    from st_ito.style_transfer import run_staged_es
    x = O.synth_audio(940, 2, 24000)[None]
    t = _target_of(x[0], 80)[None]
    assert t.shape == (1, 2, 24000)
    plugins = _plugins()
    res = run_staged_es(x, t, SR, plugins, None, None, max_iters=4, popsize=4, sigma0=0.33, seed=2, distance="mrstft",
                        run_dir=str(tmp_path))
    assert list(res) == ["output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "stage_wopts", "num_evals"]
    assert res["num_evals"] == 16 and len(res["fval_history"]) == 4
    assert [len(w) for w in res["stage_wopts"]] == [18, 4]
    np.testing.assert_array_equal(res["wopt"], np.concatenate(res["stage_wopts"]))
    ev = MrstftEvaluator(x, SR, plugins, t)            # the audio run_staged_es normalised in place
    again = float(ev.evaluate([res["wopt"]])[0][0])
    print(f"mrstft staged: fopt {res['fopt']:.6f}, the full chain at wopt alone {again:.6f}")
    assert np.isfinite(res["fopt"]) and again == res["fopt"]


def test_run_optim_staged_with_the_mrstft_objective(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    from st_ito.audio_io import save_wav
    wav = tmp_path / "in.wav"
    save_wav(str(wav), O.synth_audio(950, 2, 24000), SR)
    out_dir = tmp_path / "out"
    res = run_optim.main([str(wav), "--objective", "mrstft", "--staged", "--chain", "eq-comp", "--max-iters", "2", "--popsize", "4",
                          "--seed", "3", "--output-dir", str(out_dir)])
    run_dir = out_dir / "in_to_synthetic_target_es"
    assert (run_dir / "output_audio_sigma=0.33.wav").is_file() and (run_dir / "parameters_sigma=0.33.json").is_file()
    assert res["num_evals"] == 8 and np.isfinite(res["fopt"])
