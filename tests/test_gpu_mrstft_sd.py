"""GPU: the sum / difference MR-STFT distance (csrc/mrstft.hip's SD variant; distance="mrstft-sd") -- accuracy against the
float64 oracle on (sd(x), sd(y)) over the set of tests/mrstft_sd_cases.py, bit for bit against the L/R kernel on sums and
differences formed by torch, the polarity property that motivates it, independence of a candidate's bits from the batch
around it, the slot list, and the objective in the evaluator and in every ES driver.

The bar is the L/R kernel's: relative error <= BAR_FACTOR x mrstft_cases.yardstick_max() (about 1.45e-5) -- the same float32
evaluation plus one addition per sample.  Every case prints its measured error next to the bar (run with -s);
profiles/mrstft_sd_edges.txt records them.

The ES tests render at 262144 samples because the length policy pads to that (run_es alone is given parallel=True and renders
its few thousand samples as they are); they keep pop 4."""
import numpy as np
import pytest
import torch

import mrstft_cases as M
import mrstft_sd_cases as SD
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
CASES = {c[0]: c for c in SD.cases()}
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


def _peaks(xd):
    from st_ito import _hip
    P, C, n = xd.shape
    peaks = torch.empty(P, dtype=torch.float32, device=xd.device)
    _hip.check(_hip.lib().stito_peak(_hip.ptr(xd), P, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return peaks


def _loss(dev, x, y, norm_passes=0, slots=None, stereo="sum-diff"):
    """The loss of x (P, 2, n) against the table of y (T, 2, n) in the given mode -> (P,) float32 on the host."""
    from st_ito.features import MrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    sl = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
    return MrstftTarget(yd, stereo=stereo).loss(xd, _peaks(xd) if norm_passes else None, norm_passes, slots=sl).cpu().numpy()


def _rel(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_accuracy_against_float64_oracle(dev, bar, name):
    _, x, y, norm_passes = CASES[name]
    got, ref = _loss(dev, x, y, norm_passes), SD.reference(name, x, y, norm_passes)
    err = _rel(got, ref)
    print(f"mrstft-sd {name:28s} items {len(ref)}  max rel err {err.max():.3e}  (bar {bar:.3e})  loss {got.min():.6g} .. {got.max():.6g}")
    assert np.all(np.isfinite(got)) and err.max() <= bar, (name, got, ref, err)


def test_mono_and_antiphase_targets_are_mirror_images(dev):
    """Channel 1 negated on both sides swaps the sum row and the difference row: the same per-row sums, added in the other
    order, so the same bits -- and the mono-compatible target's clamp row carries the item (order 1e5)."""
    mono, anti = CASES["sd-mono-target-1025"], CASES["sd-antiphase-target-1025"]
    a, b = _loss(dev, mono[1], mono[2]), _loss(dev, anti[1], anti[2])
    print(f"mrstft-sd mono target {a}  antiphase target {b}")
    assert np.array_equal(a, b) and np.all(a > 1e4)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[3] == 0])
def test_bit_for_bit_the_lr_kernel_on_torch_sums_and_differences(dev, name):
    """Without peak folding the loader computes L * 1 + R * 1 and L * 1 - R * 1: the float32 operations of sd32."""
    from st_ito.features import compute_mrstft_distance, compute_sd_mrstft_distance
    _, x, y, _ = CASES[name]
    xd, yd = x.to(dev), y.to(dev)
    got = compute_sd_mrstft_distance(xd, yd)
    want = compute_mrstft_distance(SD.sd32(xd), SD.sd32(yd))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (x.shape[0],)
    assert torch.equal(got, want), (name, got, want)
    assert torch.equal(compute_sd_mrstft_distance(x, y), got.cpu())          # host tensors in, host tensor out


def test_the_polarity_flip_that_the_lr_distance_cannot_see(dev, bar):
    from st_ito.features import compute_mrstft_distance, compute_sd_mrstft_distance
    x = M.noise(0, 1, 2, 4097)
    y = x.clone()
    y[:, 1] = -x[:, 1]
    lr = float(compute_mrstft_distance(x, y)[0])
    got = float(compute_sd_mrstft_distance(x, y)[0])
    ref = O.mrstft_error(SD.sd(x), SD.sd(y))
    print(f"mrstft-sd polarity flip: L/R {lr}, sum/diff {got:.6f} (oracle {ref:.6f}, rel err {abs(got - ref) / ref:.3e}, bar {bar:.3e})")
    assert lr == 0.0
    assert got > 1.0 and abs(got - ref) / ref <= bar
    assert _loss(dev, y, y).tolist() == [0.0]                        # loss(y, table(y)) is exactly 0 in this mode too
    assert _loss(dev, torch.cat([y, x, y]), y).tolist()[::2] == [0.0, 0.0]


def test_bitwise_independent_of_the_batch_around_it(dev):
    """The same candidate has the same bits at every position of batches of 1, 3 and 5, with one target and with its own."""
    n = 4097
    cand, tgt = M.noise(600, 1, 2, n), M.noise(601, 1, 2, n)
    others, other_t = M.noise(602, 5, 2, n), M.noise(603, 5, 2, n)
    alone = _loss(dev, cand, tgt)[0]
    assert np.isfinite(alone) and alone > 0
    assert alone != _loss(dev, cand, tgt, stereo="lr")[0]              # and it is not the L/R distance
    for size in (3, 5):
        for pos in range(size):
            xb = others[:size].clone()
            xb[pos] = cand[0]
            assert _loss(dev, xb, tgt)[pos] == alone, (size, pos)
            tb = other_t[:size].clone()
            tb[pos] = tgt[0]
            assert _loss(dev, xb, tb)[pos] == alone, (size, pos)


def test_slot_lists_equal_one_target_tables(dev, bar):
    """A subset and a reordering of the targets reproduce what each population gets against a table of its own target."""
    n = 2049
    y = M.noise(900 + n, 3, 2, n)
    for i, slots in enumerate(SLOT_LISTS):
        P = len(slots) * PER
        yy = y[[s for s in slots for _ in range(PER)]]
        x = 3.0 * torch.tanh(1.5 * yy + 0.2 * M.noise(910 + n + i, P, 2, n))
        got = _loss(dev, x, y, 1, slots=slots)
        assert got.shape == (P,) and got.dtype == np.float32
        for k, s in enumerate(slots):
            alone = _loss(dev, x[k * PER:(k + 1) * PER], y[s:s + 1], 1)
            assert np.array_equal(got[k * PER:(k + 1) * PER], alone), (slots, k, got, alone)
        xs = SD.sd(M.scored(x, 1))
        ref = np.array([O.mrstft_error(xs[p:p + 1], SD.sd(y[slots[p // PER]][None])) for p in range(P)])
        err = _rel(got, ref)
        print(f"mrstft-sd slots {slots}: max rel err {err.max():.3e}  (bar {bar:.3e})")
        assert err.max() <= bar
        if slots == [0, 1, 2]:
            assert np.array_equal(got, _loss(dev, x, y, 1))                    # the identity map is the plain call
            for bad_slots, bad in (([0, 3, 2], 1), ([-1, 1, 2], 0)):           # a slot that names no target: NaN, for it only
                part = _loss(dev, x, y, 1, slots=bad_slots)
                for k in range(3):
                    sl = slice(k * PER, (k + 1) * PER)
                    assert np.all(np.isnan(part[sl])) if k == bad else np.array_equal(part[sl], got[sl]), (bad_slots, part)
            assert np.array_equal(_loss(dev, x, y, 1, slots=slots), got)       # and the library works afterwards


def test_bad_channel_counts_return_a_status(dev):
    from st_ito import _hip
    from st_ito.features import _mrstft_res
    lib = _hip.lib()
    res, n_res = _mrstft_res(None)
    n, pop = 4096, 4
    x = torch.zeros((pop, 3, n), device=dev)
    table = torch.zeros(lib.stito_mrstft_table_floats(res, n_res, 3, n), device=dev)
    ws = torch.zeros(lib.stito_mrstft_workspace_bytes(res, n_res, pop, 3, n), dtype=torch.uint8, device=dev)
    out = torch.zeros(pop, device=dev)
    slots = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _hip.stream_ptr()
    for ch in (1, 3):
        for rc in (lib.stito_mrstft_target_sd(res, n_res, _hip.ptr(x), 1, ch, n, _hip.ptr(table), st),
                   lib.stito_mrstft_loss_sd(res, n_res, _hip.ptr(x), None, 0, _hip.ptr(table), 1, pop, ch, n, _hip.ptr(out), _hip.ptr(ws),
                                            ws.numel(), st),
                   lib.stito_mrstft_loss_slots_sd(res, n_res, _hip.ptr(x), None, 0, _hip.ptr(table), 1, _hip.ptr(slots), 1, pop, ch, n,
                                                  _hip.ptr(out), _hip.ptr(ws), ws.numel(), st)):
            assert rc == _hip.E_INVALID and b"2 channels" in lib.stito_last_error(), (ch, rc, lib.stito_last_error())
    assert lib.stito_mrstft_target_sd(res, n_res, _hip.ptr(x), 1, 2, n, _hip.ptr(table), st) == 0     # (1, 2, n) fits the buffers
    assert lib.stito_mrstft_loss_sd(res, n_res, _hip.ptr(x), None, 0, _hip.ptr(table), 1, pop, 2, n, _hip.ptr(out), _hip.ptr(ws),
                                    ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the evaluator and the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _plugins(chain="eq-comp"):
    from st_ito import effects as E
    if chain == "eq-reverb":     # a chain ending in the reverb, whose width and spread act on the relation of the channels
        return E.make_plugins([("ParametricEQ", E.BasicParametricEQ, 1), ("Reverb", E.BasicReverb, 2)])
    return E.make_plugins(chain)


def _ndims(plugins):
    return sum(p["num_params"] for p in plugins.values())


def _target_of(x, seed, chain="eq-comp"):
    """The product's render of x (chs, n) at seeded parameters, (2, n) float32 on the host."""
    from st_ito.style_transfer import process_audio
    plugins = _plugins(chain)
    return torch.from_numpy(process_audio(x.numpy(), np.random.default_rng(seed).random(_ndims(plugins)), SR, plugins))


def _stereo(seed, n, scale=1.0):
    return O.synth_audio(seed, 2, n) * scale


def _assert_same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert len(got["wopt_history"]) == len(one["wopt_history"])
    for a, b in zip(got["wopt_history"], one["wopt_history"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


@pytest.mark.parametrize("chain", ["eq-comp", "eq-reverb"])
def test_evaluator_against_the_oracle_on_its_own_render(dev, bar, chain):
    """The evaluator's fitness is the oracle's distance between the sums and differences of the normalised render it hands back
    and of the target; the L/R evaluator gives other numbers on the same render."""
    from st_ito.engine import MrstftEvaluator
    n = 8192
    x = _stereo(1300, n)[None]
    plugins = _plugins(chain)
    target = _target_of(x[0], 7, chain)[None]
    assert target.shape == (1, 2, n)
    ev = MrstftEvaluator(x, SR, plugins, target, stereo="sum-diff")
    W = list(np.random.default_rng(3).random((4, _ndims(plugins))))
    loss, embeds, audio = ev.evaluate(W, parallel=True, want_audio=True)
    assert embeds == {} and loss.shape == (4,) and audio.shape == (4, 2, n)
    ref = np.array([O.mrstft_error(SD.sd(audio[p:p + 1].cpu()), SD.sd(target)) for p in range(4)])
    err = _rel(loss.cpu().numpy(), ref)
    print(f"mrstft-sd evaluator {chain}: fitness {loss.tolist()}  max rel err {err.max():.3e}  (bar {bar:.3e})")
    assert err.max() <= bar
    lr = MrstftEvaluator(x, SR, plugins, target).evaluate(W, parallel=True)[0]
    assert not torch.equal(lr, loss)
    with pytest.raises(ValueError, match="2 channels"):
        MrstftEvaluator(x[:, :1], SR, _plugins("eq-comp"), target[:, :1], stereo="sum-diff")


@pytest.mark.parametrize("chain", ["eq-comp", "eq-reverb"])
def test_run_es_equals_a_hand_stepped_run(dev, chain):
    from st_ito.engine import MrstftEvaluator
    from st_ito.style_transfer import _EsRun, run_es
    n, P, iters, seed = 6000, 4, 3, 5
    x = _stereo(1310, n, 0.7)[None]
    plugins = _plugins(chain)
    t = _target_of(x[0], 8, chain)[None]
    xin, tin = x.clone(), t.clone()
    res = run_es(xin, tin, SR, plugins, None, None, distance="mrstft-sd", popsize=P, max_iters=iters, sigma0=0.33, seed=seed,
                 find_w0=False, parallel=True)
    assert list(res) == ["output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "num_evals"]
    assert res["num_evals"] == P * iters and res["output_audio"].shape == (2, n)
    ev = MrstftEvaluator(xin, SR, plugins, tin, stereo="sum-diff")     # the audio run_es normalised in place
    run = _EsRun(np.full(_ndims(plugins), 0.5), 0.33, P, seed)
    for it in range(iters):
        run.tell(ev.evaluate(run.ask(), parallel=True)[0].tolist(), it)
    np.testing.assert_array_equal(res["wopt"], run.es.result[0])
    assert res["fopt"] == run.es.result[1] and res["fval_history"] == run.fval_history
    assert np.isfinite(res["fopt"]) and res["fopt"] > 0
    lr = run_es(x.clone(), t.clone(), SR, plugins, None, None, distance="mrstft", popsize=P, max_iters=iters, sigma0=0.33, seed=seed,
                find_w0=False, parallel=True)
    assert lr["fopt"] != res["fopt"]                                 # "mrstft" is still the other distance


def test_run_es_on_the_device_does_not_depend_on_sync_every(dev):
    from st_ito.style_transfer import run_es
    n = 6000
    x = _stereo(1320, n, 0.7)[None]
    plugins = _plugins("eq-reverb")
    t = _target_of(x[0], 9, "eq-reverb")[None]
    kw = dict(distance="mrstft-sd", popsize=4, max_iters=4, sigma0=0.33, seed=3, find_w0=False, parallel=True, device_es=True)
    a = run_es(x.clone(), t.clone(), SR, plugins, None, None, sync_every=1, **kw)
    b = run_es(x.clone(), t.clone(), SR, plugins, None, None, sync_every=4, **kw)
    _assert_same_run(a, b)
    assert a["num_evals"] == 16 and np.isfinite(a["fopt"]) and a["fopt"] > 0


def test_staged_es(dev, tmp_path):
    from st_ito.engine import MrstftEvaluator
    from st_ito.style_transfer import run_staged_es
    n = 6000
    x = _stereo(1330, n)[None]
    plugins = _plugins("eq-reverb")
    t = _target_of(x[0], 10, "eq-reverb")[None]
    res = run_staged_es(x, t, SR, plugins, None, None, max_iters=4, popsize=4, sigma0=0.33, seed=2, distance="mrstft-sd",
                        run_dir=str(tmp_path))
    assert res["num_evals"] == 16 and len(res["fval_history"]) == 4
    assert [len(w) for w in res["stage_wopts"]] == [p["num_params"] for p in plugins.values()]
    ev = MrstftEvaluator(x, SR, plugins, t, stereo="sum-diff")         # the audio run_staged_es normalised in place
    again = float(ev.evaluate([res["wopt"]])[0][0])
    assert np.isfinite(res["fopt"]) and again == res["fopt"]


def _alone(x, t, seed, **kw):
    from st_ito.style_transfer import run_es
    return run_es(x.clone(), t.clone(), SR, _plugins(), None, None, distance="mrstft-sd", find_w0=False, seed=seed, **kw)


def test_tensor_form_batch_equals_run_es_on_every_pair_alone(dev):
    from st_ito.style_transfer import run_es_batch
    xs = torch.stack([_stereo(1340 + b, 8192, 0.6 + 0.2 * b) for b in range(2)])
    ts = torch.stack([_target_of(xs[b], 60 + b) for b in range(2)])
    x0, t0 = xs.clone(), ts.clone()
    kw = dict(max_iters=3, sigma0=0.33, popsize=4, early_stop=False)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=11, distance="mrstft-sd", **kw)
    assert torch.equal(xs, x0) and torch.equal(ts, t0)
    for b in range(2):
        _assert_same_run(res[b], _alone(xs[b][None], ts[b][None], 11 + b, **kw))
        assert res[b]["num_evals"] == 12 and np.isfinite(res[b]["fopt"]) and res[b]["fopt"] > 0


@pytest.mark.parametrize("random_crop,lengths", [(True, [6000, 8192, 262144 + 16384 + 500]), (False, [6000, 8192, 6000])])
def test_list_form_batch_equals_run_es_on_every_pair_alone(dev, random_crop, lengths):
    """One length group either way.  Under random_crop the long pair draws its crops, so the group's spans move: the targets
    are gathered at the inputs' starts and the table is refilled.  Without it nothing moves: one static table, read through
    the slot list.  Pair 1 is silent (a constant loss): it is stale from iteration 1 and stops after iteration 11, and from
    then on it is neither gathered nor scored."""
    from st_ito import engine
    from st_ito.style_transfer import run_es_batch
    P, seed = 4, 23
    xs = [_stereo(1350 + b, n, 0.5 + 0.1 * b)[None] for b, n in enumerate(lengths)]
    ts = [_target_of(x[0], 70 + b)[None] for b, x in enumerate(xs)]       # made before pair 1's input is replaced
    xs[1] = torch.zeros_like(xs[1])
    assert len(engine.plan_ragged_groups(lengths, random_crop)) == 1
    keep = [(x.clone(), t.clone()) for x, t in zip(xs, ts)]
    kw = dict(max_iters=13, sigma0=0.33, popsize=P, random_crop=random_crop, early_stop=True)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=seed, distance="mrstft-sd", **kw)
    for (x0, t0), x, t in zip(keep, xs, ts):         # the caller's tensors are not modified
        assert torch.equal(x0, x) and torch.equal(t0, t)
    print(f"mrstft-sd list form random_crop={random_crop}: num_evals {[r['num_evals'] for r in res]}")
    assert res[1]["num_evals"] == 12 * P
    for b in range(len(lengths)):
        _assert_same_run(res[b], _alone(xs[b], ts[b], seed + b, **kw))
        assert res[b]["output_audio"].shape[-1] == lengths[b]
        assert all(np.isfinite(f) and f > 0 for f in res[b]["fval_history"][1:])


def test_a_mono_chain_is_refused(dev):
    from st_ito.style_transfer import run_es, run_es_batch, run_staged_es
    x = O.synth_audio(1360, 1, 6000)[None]
    t = _target_of(x[0], 12)[None]
    assert t.shape == (1, 1, 6000)
    for call in (lambda: run_es(x.clone(), t.clone(), SR, _plugins(), None, None, distance="mrstft-sd", popsize=4, max_iters=1, find_w0=False),
                 lambda: run_staged_es(x.clone(), t.clone(), SR, _plugins(), None, None, distance="mrstft-sd", popsize=4, max_iters=2),
                 lambda: run_es_batch(x.clone(), t.clone(), SR, _plugins(), None, None, max_iters=1, popsize=4, distance="mrstft-sd"),
                 lambda: run_es_batch([x[0].clone()], [t[0].clone()], SR, _plugins(), None, None, max_iters=1, popsize=4, distance="mrstft-sd")):
        with pytest.raises(ValueError, match="2 channels.*renders 1 channels"):
            call()
