"""GPU: the mel-scaled MR-STFT distance (csrc/mrstft.hip's MEL variant; distance="mrstft-mel") -- accuracy against the float64
restatement of tests/mrstft_mel_ref.py on every input of tests/mrstft_cases.py (48 kHz, 64 bands), loss(y, table(y)) == 0, the
identity bank against the linear kernel, independence of a candidate's bits from the batch, the number of targets and the slot
list around it, the folded peak, and the objective in the evaluator and in every ES driver.

The bar is BAR_FACTOR = 4 times the yardstick of tests/test_mrstft_mel_host.py (the float32 torch restatement's largest relative
distance from the float64 one over the same inputs: 4.0e-7, so the bar is 1.6e-6).  Every case prints its measured error next to
the bar (run with -s); profiles/mrstft_mel_edges.txt records them.

The batch drivers pad to 262144 samples (the length policy); run_es alone is given parallel=True where nothing asks otherwise and
renders its few thousand samples as they are.  Populations of 4 - 8, 2 - 3 iterations."""
import numpy as np
import pytest
import torch

import mrstft_cases as M
import mrstft_mel_ref as R
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = R.SR
CASES = {c[0]: c for c in M.cases()}
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
    return R.BAR_FACTOR * R.yardstick_max()


def _peaks(xd):
    from st_ito import _hip
    P, C, n = xd.shape
    peaks = torch.empty(P, dtype=torch.float32, device=xd.device)
    _hip.check(_hip.lib().stito_peak(_hip.ptr(xd), P, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return peaks


def _loss(dev, x, y, norm_passes=0, slots=None, **kw):
    """The loss of x (P, C, n) against the mel table of y (T, C, n) -> (P,) float32 on the host."""
    from st_ito.features import MelMrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    sl = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
    tgt = MelMrstftTarget(yd, SR, **kw) if "bank" not in kw else MelMrstftTarget(yd, **kw)
    return tgt.loss(xd, _peaks(xd) if norm_passes else None, norm_passes, slots=sl).cpu().numpy()


def _rel(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. - 5. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_accuracy_against_the_float64_reference(dev, bar, name):
    """Every case, the folded peak of the norm_passes 1 cases included (their reference is taken on normalised audio)."""
    _, x, y, norm_passes = CASES[name]
    got, ref = _loss(dev, x, y, norm_passes), R.reference(name, x, y, norm_passes)
    err = _rel(got, ref)
    print(f"mrstft-mel {name:28s} items {len(ref)}  max rel err {err.max():.3e}  (bar {bar:.3e})  loss {got.min():.6g} .. {got.max():.6g}")
    assert got.shape == (x.shape[0],) and got.dtype == np.float32
    assert np.all(np.isfinite(got)) and err.max() <= bar, (name, got, ref, err)


def test_compute_mel_mrstft_distance_is_that_loss(dev):
    from st_ito.features import compute_mel_mrstft_distance
    _, x, y, _ = CASES["noise-1200-c2-p3"]
    got = compute_mel_mrstft_distance(x.to(dev), y.to(dev), SR)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (3,)
    assert np.array_equal(got.cpu().numpy(), _loss(dev, x, y))
    assert torch.equal(compute_mel_mrstft_distance(x, y, SR), got.cpu())                        # host tensors in, host tensor out
    assert torch.equal(compute_mel_mrstft_distance(x, y, SR, 64, R.RESOLUTIONS), got.cpu())     # the defaults, said
    other = compute_mel_mrstft_distance(x, y, SR, 32)
    assert torch.isfinite(other).all() and not torch.equal(other, got.cpu())


@pytest.mark.parametrize("name", ["noise-2049-c1-p3", "noise-4097-c2-p5", "twotone-2049", "zero-target-channel-1025"])
def test_loss_of_the_target_against_its_own_table_is_exactly_zero(dev, name):
    _, _, y, _ = CASES[name]
    y = y if y.shape[0] > 1 else torch.cat([y, 0.5 * y.flip(-1)])
    assert _loss(dev, y, y).tolist() == [0.0] * y.shape[0]
    got = _loss(dev, torch.cat([y[:1], y[:1]]), y[:1])                # one target, two candidates
    assert got.tolist() == [0.0, 0.0]


def _identity_bank(n_fft):
    bins = n_fft // 2 + 1
    return (np.arange(bins, dtype=np.int32), np.ones(bins, np.int32), np.ones((1, bins), np.float32))


@pytest.mark.parametrize("name", ["noise-2049-c1-p3", "noise-1200-c2-p3"])
def test_identity_bank_gives_the_linear_kernels_loss(dev, name):
    """n_bins = n_fft / 2 + 1 <= 256 allows n_fft 256 only.  Band k is bin k with weight 1.0: fma(1, |X|, 0) is |X|, so the terms
    are the linear kernel's float32 values and only the order of the float64 additions differs (lanes own other columns): at most
    about 1e5 x 2^-53 relative, far below half a float32 ulp, so the float32 results differ by at most one ulp."""
    from st_ito.features import MrstftTarget
    _, x, y, _ = CASES[name]
    res = [(256, 30, 120), (256, 64, 256)]
    got = _loss(dev, x, y, resolutions=res, bank=[_identity_bank(256)] * 2)
    lin = MrstftTarget(y.to(dev), res).loss(x.to(dev)).cpu().numpy()
    print(f"mrstft-mel identity bank {name}: {got}  linear {lin}  ulps {np.abs(got - lin) / np.spacing(lin)}")
    assert np.all(np.isfinite(lin)) and np.all(lin > 0)
    assert np.all(np.abs(got - lin) <= np.spacing(lin))
    ref = np.array([R.mel_error64(x[p:p + 1], y[p:p + 1] if y.shape[0] > 1 else y, resolutions=res, banks=[np.eye(129, dtype=np.float32)] * 2)
                    for p in range(x.shape[0])])
    assert _rel(got, ref).max() <= 1e-5                               # and it is that distance (float32 against float64)


def test_same_bits_whatever_is_around_the_candidate(dev):
    """Alone; at every position of larger batches; under n_targets 1 and 3; under a permuted slot list; next to slots that name no
    target, which give NaN for their population only."""
    n = 4097
    cand, tgt = M.noise(700, 1, 2, n), M.noise(701, 1, 2, n)
    others, other_t = M.noise(702, 6, 2, n), M.noise(703, 3, 2, n)
    alone = _loss(dev, cand, tgt)[0]
    assert np.isfinite(alone) and alone > 0
    for size in (3, 6):
        for pos in range(size):
            xb = others[:size].clone()
            xb[pos] = cand[0]
            assert _loss(dev, xb, tgt)[pos] == alone, (size, pos)                       # n_targets 1
            k = pos // (size // 3)
            tb = other_t.clone()
            tb[k] = tgt[0]
            assert _loss(dev, xb, tb)[pos] == alone, (size, pos)                        # n_targets 3: its own in slot k
    # three populations of PER candidates; the candidate sits in population 1 and its target in table slot 2
    xb = others.clone()
    xb[PER] = cand[0]
    tb = other_t.clone()
    tb[2] = tgt[0]
    plain = _loss(dev, xb, tb[[0, 2, 1]])
    for slots in ([0, 2, 1], [1, 2, 0], [2, 2, 2]):
        got = _loss(dev, xb, tb, slots=slots)
        assert got[PER] == alone and np.all(np.isfinite(got)), (slots, got)
    assert np.array_equal(_loss(dev, xb, tb, slots=[0, 2, 1]), plain)                   # a slot list is the table it describes
    for bad_slots, bad in (([-1, 2, 1], 0), ([0, 2, 3], 2)):                            # -1 and n_targets
        part = _loss(dev, xb, tb, slots=bad_slots)
        for k in range(3):
            sl = slice(k * PER, (k + 1) * PER)
            assert np.all(np.isnan(part[sl])) if k == bad else np.array_equal(part[sl], plain[sl]), (bad_slots, part)
    assert np.array_equal(_loss(dev, xb, tb, slots=[0, 2, 1]), plain)                   # and the library works afterwards


def test_folded_peak_against_the_reference_on_normalised_audio(dev, bar):
    """norm_passes 1 on loud stereo audio, three targets through a slot list."""
    n = 2049
    y = M.noise(900, 3, 2, n)
    slots = [2, 0, 1]
    x = 3.0 * torch.tanh(1.5 * y[[s for s in slots for _ in range(PER)]] + 0.2 * M.noise(910, 3 * PER, 2, n))
    got = _loss(dev, x, y, 1, slots=slots)
    xs = M.scored(x, 1)
    ref = np.array([R.mel_error64(xs[p:p + 1], y[slots[p // PER]][None]) for p in range(3 * PER)])
    err = _rel(got, ref)
    print(f"mrstft-mel folded peak, slots {slots}: max rel err {err.max():.3e}  (bar {bar:.3e})")
    assert err.max() <= bar
    assert not np.array_equal(got, _loss(dev, x, y, 0, slots=slots))                    # the unnormalised audio scores otherwise


def test_a_bad_bank_returns_a_status(dev):
    """n_bins outside [1, 256], a band longer than the bins, a band that starts beyond them: STITO_E_INVALID, and the library
    works afterwards."""
    from st_ito import _hip
    from st_ito.features import MelMrstftTarget, _DeviceMelBank, mel_mrstft_bank
    lib = _hip.lib()
    n = 4097
    y = M.noise(800, 1, 1, n).to(dev)
    good = MelMrstftTarget(y, SR)
    want = good.loss(y).tolist()
    assert want == [0.0]
    st = _hip.stream_ptr()

    def status(bank, n_bins=None):
        b = _DeviceMelBank(bank, dev)
        if n_bins is not None:
            b.c.n_bins = n_bins
        out = torch.zeros(1, device=dev)
        ws = torch.zeros(lib.stito_mrstft_workspace_bytes(good.res, good.n_res, 1, 1, n), dtype=torch.uint8, device=dev)
        rcs = (lib.stito_mrstft_target_mel(good.res, good.n_res, b.ref, _hip.ptr(y), 1, n, _hip.ptr(good.table), st),
               lib.stito_mrstft_loss_mel(good.res, good.n_res, b.ref, _hip.ptr(y), None, 0, _hip.ptr(good.table), 1, 1, 1, n, _hip.ptr(out),
                                         _hip.ptr(ws), ws.numel(), st))
        return rcs, lib.stito_last_error()

    def changed(i, m, start=None, length=None):
        bank = [tuple(a.copy() for a in b) for b in mel_mrstft_bank(SR)]
        if start is not None:
            bank[i][0][m] = start
        if length is not None:
            bank[i][1][m] = length
        return bank

    for bank, n_bins, word in ((changed(0, 0), 0, b"n_bins"), (changed(0, 0), 257, b"n_bins"),
                               (changed(2, 63, length=258), None, b"band 63"),          # n_fft 512 has 257 bins
                               (changed(2, 5, start=257, length=1), None, b"band 5"),
                               (changed(1, 7, start=-1), None, b"band 7")):
        rcs, msg = status(bank, n_bins)
        assert rcs == (_hip.E_INVALID, _hip.E_INVALID) and word in msg, (rcs, msg)
    torch.cuda.synchronize()
    assert good.update(y).loss(y).tolist() == want


# ---------------------------------------------------------------------------------------------------------------------------
# 6. - 8. the evaluator and the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _plugins(chain="eq-comp"):
    from st_ito import effects as E
    return E.make_plugins(chain)


def _ndims(plugins):
    return sum(p["num_params"] for p in plugins.values())


def _target_of(x, w, chain="eq-comp"):
    """The product's own render of x (chs, n) at w, peak normalised, (chs', n) float32 on the host."""
    from st_ito.style_transfer import process_audio
    return torch.from_numpy(process_audio(x.numpy(), np.asarray(w), SR, _plugins(chain)))


def _seeded_target(x, seed, chain="eq-comp"):
    return _target_of(x, np.random.default_rng(seed).random(_ndims(_plugins(chain))), chain)


def _assert_same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert len(got["wopt_history"]) == len(one["wopt_history"])
    for a, b in zip(got["wopt_history"], one["wopt_history"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


@pytest.fixture(scope="module")
def objective_case():
    """12345 samples through EQ -> compressor; eight parameter vectors, the target is the product's render at the last."""
    n = 12345
    x = O.synth_audio(1234, 1, n)
    W = np.random.default_rng(11).random((8, _ndims(_plugins())))
    return x[None], W, _target_of(x, W[7])[None]


def test_objective_through_the_evaluator(dev, bar, objective_case):
    """The fitness at w* is the smallest of the population and within the bar of 0; every other fitness is the float64
    reference's distance between the normalised render the evaluator hands back and the target."""
    from st_ito.engine import MelMrstftEvaluator, MrstftEvaluator
    x, W, target = objective_case
    ev = MelMrstftEvaluator(x, SR, _plugins(), target)
    loss, embeds, audio = ev.evaluate(list(W), parallel=True, want_audio=True)
    assert isinstance(ev, MrstftEvaluator) and ev.n_bins == 64
    assert embeds == {} and loss.shape == (8,) and loss.dtype == torch.float32 and audio.shape == (8, 1, x.shape[-1])
    got = loss.cpu().numpy().astype(np.float64)
    ref = np.array([R.mel_error64(audio[p:p + 1].cpu(), target) for p in range(8)])
    err = _rel(got[:7], ref[:7])
    print(f"mrstft-mel objective: fitness {got}\n  max rel err {err.max():.3e}, at w* {got[7]:.3e} (reference {ref[7]:.3e})  (bar {bar:.3e})")
    assert int(np.argmin(got)) == 7 and abs(got[7]) <= bar
    assert np.all(got[:7] - got[7] > bar) and err.max() <= bar
    lin = MrstftEvaluator(x, SR, _plugins(), target).evaluate(list(W), parallel=True)[0]
    assert not torch.equal(lin, loss)                                  # "mrstft" is still the other distance


def test_run_es_with_the_mel_objective(dev, objective_case):
    from st_ito.engine import MelMrstftEvaluator
    from st_ito.style_transfer import run_es
    x, _, target = objective_case
    plugins = _plugins()
    xin, tin = x.clone(), target.clone()
    res = run_es(xin, tin, SR, plugins, None, None, distance="mrstft-mel", popsize=8, max_iters=3, seed=0, find_w0=False, parallel=True)
    assert list(res) == ["output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "num_evals"]
    assert res["num_evals"] == 24 and len(res["fval_history"]) == 3 and res["output_audio"].shape == (1, x.shape[-1])
    ev = MelMrstftEvaluator(xin, SR, plugins, tin)                     # the audio run_es normalised in place
    f0 = float(ev.evaluate([np.full(_ndims(plugins), 0.5)], parallel=True)[0][0])
    again = float(ev.evaluate([res["wopt"]], parallel=True)[0][0])
    print(f"mrstft-mel run_es: fitness at w0 {f0:.6f} -> fopt {res['fopt']:.6f} in 3 iterations of 8")
    assert np.isfinite(res["fopt"]) and 0 < res["fopt"] <= f0
    assert again == res["fopt"]                                        # bit for bit, alone
    lin = run_es(x.clone(), target.clone(), SR, plugins, None, None, distance="mrstft", popsize=8, max_iters=3, seed=0, find_w0=False,
                 parallel=True)
    assert lin["fopt"] != res["fopt"]


def _alone(x, t, seed, chain="eq-comp", **kw):
    from st_ito.style_transfer import run_es
    return run_es(x.clone(), t.clone(), SR, _plugins(chain), None, None, distance="mrstft-mel", find_w0=False, seed=seed, **kw)


def test_tensor_form_batch_equals_run_es_on_every_pair_alone(dev):
    from st_ito.style_transfer import run_es_batch
    xs = torch.stack([O.synth_audio(1340 + b, 2, 8192) * (0.6 + 0.2 * b) for b in range(2)])
    ts = torch.stack([_seeded_target(xs[b], 60 + b) for b in range(2)])
    x0, t0 = xs.clone(), ts.clone()
    kw = dict(max_iters=3, sigma0=0.33, popsize=4, early_stop=False)
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=11, distance="mrstft-mel", **kw)
    assert torch.equal(xs, x0) and torch.equal(ts, t0)
    for b in range(2):
        _assert_same_run(res[b], _alone(xs[b][None], ts[b][None], 11 + b, **kw))
        assert res[b]["num_evals"] == 12 and np.isfinite(res[b]["fopt"]) and res[b]["fopt"] > 0


@pytest.mark.parametrize("random_crop,lengths", [(True, [6000, 8192, 262144 + 16384 + 500]), (False, [6000, 12345, 6000])])
def test_list_form_batch_equals_run_es_on_every_pair_alone(dev, random_crop, lengths):
    """One length group either way: under random_crop the long pair draws its crops, so the targets are gathered at the inputs'
    starts and the table is refilled; without it nothing moves and one static table is read through the slot list."""
    from st_ito import engine
    from st_ito.style_transfer import run_es_batch
    xs = [O.synth_audio(1350 + b, 1, n)[None] * (0.5 + 0.1 * b) for b, n in enumerate(lengths)]
    ts = [_seeded_target(x[0], 70 + b, "eq")[None] for b, x in enumerate(xs)]
    assert len(engine.plan_ragged_groups(lengths, random_crop)) == 1
    keep = [(x.clone(), t.clone()) for x, t in zip(xs, ts)]
    kw = dict(max_iters=3, sigma0=0.33, popsize=4, random_crop=random_crop, early_stop=False)
    res = run_es_batch([x[0] for x in xs], [t[0] for t in ts], SR, _plugins("eq"), None, None, seed=23, distance="mrstft-mel", **kw)
    for (x0, t0), x, t in zip(keep, xs, ts):         # the caller's tensors are not modified
        assert torch.equal(x0, x) and torch.equal(t0, t)
    for b in range(len(lengths)):
        _assert_same_run(res[b], _alone(xs[b], ts[b], 23 + b, "eq", **kw))
        assert res[b]["output_audio"].shape[-1] == lengths[b] and res[b]["num_evals"] == 12
        assert all(np.isfinite(f) and f > 0 for f in res[b]["fval_history"][1:])


def test_staged_es_and_device_es(dev, tmp_path):
    from st_ito.engine import MelMrstftEvaluator
    from st_ito.style_transfer import run_es, run_staged_es
    n = 6000
    x = O.synth_audio(1330, 2, n)[None]
    plugins = _plugins()
    t = _seeded_target(x[0], 10)[None]
    res = run_staged_es(x, t, SR, plugins, None, None, max_iters=4, popsize=4, sigma0=0.33, seed=2, distance="mrstft-mel",
                        run_dir=str(tmp_path))
    assert len(plugins) == 2 and len(res["stage_wopts"]) == 2
    assert [len(w) for w in res["stage_wopts"]] == [p["num_params"] for p in plugins.values()]
    assert res["num_evals"] == 16 and len(res["fval_history"]) == 4
    ev = MelMrstftEvaluator(x, SR, plugins, t)                         # the audio run_staged_es normalised in place
    assert np.isfinite(res["fopt"]) and float(ev.evaluate([res["wopt"]])[0][0]) == res["fopt"]
    kw = dict(distance="mrstft-mel", popsize=4, max_iters=3, sigma0=0.33, seed=3, find_w0=False, parallel=True, device_es=True)
    a = run_es(x.clone(), t.clone(), SR, plugins, None, None, sync_every=1, **kw)
    b = run_es(x.clone(), t.clone(), SR, plugins, None, None, sync_every=3, **kw)
    _assert_same_run(a, b)
    assert a["num_evals"] == 12 and np.isfinite(a["fopt"]) and a["fopt"] > 0
