"""GPU: the prefiltered MR-STFT distances (csrc/mrstft.hip's PRE variants; distance="mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw") --
accuracy against the float64 reference of tests/mrstft_aw_ref.py on every input of tests/mrstft_cases.py (the sum / difference form:
tests/mrstft_sd_cases.py) with the 48 kHz "aw" taps, the filter's orientation and the order of filtering and reflect padding,
degenerate and longest tap sets, loss(y, table(y)) == 0, independence of a candidate's bits from what is around it, the folded
peak, and the objective in the evaluator and in every ES driver.

The bar of a (form, tap set) is BAR_FACTOR = 4 times the yardstick tests/test_mrstft_aw_host.py bounds: the float32 torch
restatement's largest relative distance from the float64 one over the inputs in use.  Every case prints its measured error next to
the bar (run with -s); profiles/mrstft_aw_edges.txt records them.  The folded peak (item 6 of the list above) is part of the
accuracy test: the "peak-folded" and "zero-candidate" cases are scored with norm_passes 1 against float64 of the normalised signal.

Populations of 4, 2 iterations, 4097 and 6000 samples through the "eq" chain."""
import numpy as np
import pytest
import torch

import mrstft_aw_ref as A
import mrstft_cases as M
import mrstft_sd_cases as SDC
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = A.SR
CASES = {form: {c[0]: c for c in A.cases(form)} for form in A.FORMS}
PER = 2
DISTANCE = {"lr": "mrstft-aw", "sum-diff": "mrstft-sd-aw", "mel": "mrstft-mel-aw"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def aw():
    return A.aw_taps(SR)


def _peaks(xd):
    from st_ito import _hip
    P, C, n = xd.shape
    peaks = torch.empty(P, dtype=torch.float32, device=xd.device)
    _hip.check(_hip.lib().stito_peak(_hip.ptr(xd), P, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return peaks


def _loss(dev, form, taps, x, y, norm_passes=0, slots=None):
    """The loss of x (P, C, n) against the prefiltered table of y (T, C, n) -> (P,) float32 on the host."""
    from st_ito.features import PrefilteredMrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    sl = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
    tgt = PrefilteredMrstftTarget(yd, taps, SR, kind=form)
    return tgt.loss(xd, _peaks(xd) if norm_passes else None, norm_passes, slots=sl).cpu().numpy()


def _plain(dev, form, x, y):
    """The unfiltered entry points' loss of the same form."""
    from st_ito.features import MelMrstftTarget, MrstftTarget
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    tgt = MelMrstftTarget(yd, SR) if form == "mel" else MrstftTarget(yd, None, "sum-diff" if form == "sum-diff" else "lr")
    return tgt.loss(xd).cpu().numpy()


def _rel(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. - 6. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", [(f, n) for f in A.FORMS for n in CASES[f]])
def test_accuracy_against_the_float64_reference(dev, aw, form, name):
    """Every case, the folded peak of the norm_passes 1 cases included (their reference is taken on normalised audio)."""
    _, x, y, norm_passes = CASES[form][name]
    bar = A.bar(form, aw)
    got, ref = _loss(dev, form, aw, x, y, norm_passes), A.reference(form, aw, name, x, y, norm_passes)
    err = _rel(got, ref)
    print(f"{DISTANCE[form]:13s} {name:28s} items {len(ref)}  max rel err {err.max():.3e}  (bar {bar:.3e})  loss {got.min():.6g} .. {got.max():.6g}")
    assert got.shape == (x.shape[0],) and got.dtype == np.float32
    assert np.all(np.isfinite(got)) and err.max() <= bar, (form, name, got, ref, err)


def test_compute_prefiltered_mrstft_distance_is_that_loss(dev, aw):
    from st_ito.features import compute_prefiltered_mrstft_distance as dist
    _, x, y, _ = CASES["lr"]["noise-1200-c2-p3"]
    for form in A.FORMS:
        got = dist(x.to(dev), y.to(dev), "aw", SR, kind=form)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (3,)
        assert np.array_equal(got.cpu().numpy(), _loss(dev, form, aw, x, y))
        assert torch.equal(dist(x, y, aw, SR, kind=form), got.cpu())          # host tensors in, host tensor out; the taps as an array
        assert not np.array_equal(got.cpu().numpy(), _plain(dev, form, x, y))  # and the filter does something


@pytest.mark.parametrize("name", ["noise-1025-c1-p1", "noise-2049-c1-p3"])
def test_orientation_and_the_order_of_filter_and_padding(dev, name):
    """A 31-tap asymmetric filter.  The definition correlates (taps[k] meets x[i + k - c]) and reflects the FILTERED row; reversed
    taps and reflect-then-filter are other functions, 2e-3 or more away on these inputs -- asserted here in float64, so that the
    bar cannot be passed by either of them."""
    taps = A.seeded_taps(31, 5)
    assert np.abs(taps - taps[::-1]).max() > 1e-2
    _, x, y, norm_passes = CASES["lr"][name]
    bar = A.bar("lr", taps)
    ref = A.reference("lr", taps, name, x, y, norm_passes)
    reversed_ = np.array([A.error64("lr", a, b, taps[::-1].copy()) for a, b in A.items(x, y, norm_passes)])
    reflect_first = np.array([A.wrong_reflect_first64("lr", a, b, taps) for a, b in A.items(x, y, norm_passes)])
    got = _loss(dev, "lr", taps, x, y, norm_passes)
    err = _rel(got, ref)
    print(f"31 asymmetric taps {name}: max rel err {err.max():.3e} (bar {bar:.3e}); reversed taps {_rel(reversed_, ref).min():.3e}, "
          f"reflect first {_rel(reflect_first, ref).min():.3e} away")
    assert _rel(reversed_, ref).min() > 10 * bar and _rel(reflect_first, ref).min() > 10 * bar
    assert err.max() <= bar, (got, ref)


@pytest.mark.parametrize("form", A.FORMS)
def test_degenerate_taps(dev, form):
    """[1.0] is the unfiltered distance; [0, 0, 1] is the unfiltered distance of the rows shifted left by one sample with a zero
    appended.  fma(1, x, 0) is x, so the terms are the plain kernel's; the plans may tile differently, so the float64 tile sums may
    be added in another order: one float32 ulp."""
    _, x, y, _ = CASES[form]["noise-1200-c2-p3"]
    plain = _plain(dev, form, x, y)
    got = _loss(dev, form, np.array([1.0], np.float32), x, y)
    assert np.all(np.abs(got - plain) <= np.spacing(plain)), (got, plain)
    shift = lambda a: torch.cat([a[..., 1:], torch.zeros_like(a[..., :1])], -1)    # noqa: E731
    plain = _plain(dev, form, shift(x), shift(y))
    got = _loss(dev, form, np.array([0.0, 0.0, 1.0], np.float32), x, y)
    print(f"{DISTANCE[form]} [0, 0, 1]: {got} plain on the shifted rows {plain}")
    assert np.all(np.abs(got - plain) <= np.spacing(plain)), (got, plain)
    assert not np.array_equal(got, _plain(dev, form, x, y))


def test_a_plan_whose_tiling_differs_from_the_unfiltered_one(dev):
    """hop 2000 at n_fft 256: the unfiltered plan takes 8 frames a tile, the prefilter's span bound allows 4, so table scratch and
    workspace have other sizes -- and the unit tap still gives the unfiltered loss to one ulp, the target's own table exactly 0."""
    from st_ito import _hip
    from st_ito.features import MrstftTarget, PrefilteredMrstftTarget
    res = [(256, 2000, 256), (512, 50, 240)]
    _, x, y, _ = CASES["lr"]["noise-12345-c1-p1"]
    xd, yd = x.to(dev), y.to(dev)
    lin, pf = MrstftTarget(yd, res), PrefilteredMrstftTarget(yd, [1.0], resolutions=res)
    assert pf._workspace_bytes(1) > lin._workspace_bytes(1) > 0 and pf.table.numel() > lin.table.numel()
    plain, got = lin.loss(xd).cpu().numpy(), pf.loss(xd).cpu().numpy()
    assert np.all(np.isfinite(plain)) and np.all(np.abs(got - plain) <= np.spacing(plain)), (got, plain)
    aw = PrefilteredMrstftTarget(yd, "aw", SR, resolutions=res)
    assert aw.loss(yd).tolist() == [0.0] and np.isfinite(aw.loss(xd).item()) and aw.loss(xd).item() != got[0]
    ws = torch.zeros(lin._workspace_bytes(1), dtype=torch.uint8, device=dev)        # the unfiltered size is refused, not overrun
    out = torch.zeros(1, device=dev)
    rc = _hip.lib().stito_mrstft_loss_pf(*aw._head(), aw.res, aw.n_res, _hip.ptr(xd), None, 0, _hip.ptr(aw.table), 1, 1, 1, 12345, _hip.ptr(out),
                                         _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
    assert rc == _hip.E_WORKSPACE


@pytest.mark.parametrize("name", ["noise-1200-c2-p3", "noise-4097-c2-p5"])
def test_255_taps_stay_within_the_bar(dev, name):
    taps = A.seeded_taps(255, 9)
    _, x, y, norm_passes = CASES["lr"][name]
    bar = A.bar("lr", taps)
    err = _rel(_loss(dev, "lr", taps, x, y, norm_passes), A.reference("lr", taps, name, x, y, norm_passes))
    print(f"255 taps {name}: max rel err {err.max():.3e} (bar {bar:.3e})")
    assert err.max() <= bar


@pytest.mark.parametrize("form", A.FORMS)
@pytest.mark.parametrize("name", ["noise-4097-c2-p5", "twotone-2049", "zero-target-channel-1025"])
def test_loss_of_the_target_against_its_own_table_is_exactly_zero(dev, aw, form, name):
    _, _, y, _ = CASES["lr"][name]
    y = y if y.shape[0] > 1 else torch.cat([y, 0.5 * y.flip(-1)])
    assert _loss(dev, form, aw, y, y).tolist() == [0.0] * y.shape[0]
    assert _loss(dev, form, aw, torch.cat([y[:1], y[:1]]), y[:1]).tolist() == [0.0, 0.0]      # one target, two candidates


@pytest.mark.parametrize("form", A.FORMS)
def test_same_bits_whatever_is_around_the_candidate(dev, aw, form):
    """Alone; at the first and the last position of a population of 5; under a permuted and a repeating slot list; next to slots
    that name no target, which give NaN for their population only."""
    n = 4097
    cand, tgt = M.noise(700, 1, 2, n), M.noise(701, 1, 2, n)
    others, other_t = M.noise(702, 6, 2, n), M.noise(703, 3, 2, n)
    alone = _loss(dev, form, aw, cand, tgt)[0]
    assert np.isfinite(alone) and alone > 0
    for pos in (0, 4):
        xb = others[:5].clone()
        xb[pos] = cand[0]
        assert _loss(dev, form, aw, xb, tgt)[pos] == alone, pos
    xb = others.clone()            # three populations of PER candidates; the candidate in population 1, its target in table slot 2
    xb[PER] = cand[0]
    tb = other_t.clone()
    tb[2] = tgt[0]
    plain = _loss(dev, form, aw, xb, tb[[0, 2, 1]])
    for slots in ([0, 2, 1], [1, 2, 0], [2, 2, 2]):
        got = _loss(dev, form, aw, xb, tb, slots=slots)
        assert got[PER] == alone and np.all(np.isfinite(got)), (slots, got)
    assert np.array_equal(_loss(dev, form, aw, xb, tb, slots=[0, 2, 1]), plain)
    for bad_slots, bad in (([-1, 2, 1], 0), ([0, 2, 3], 2)):
        part = _loss(dev, form, aw, xb, tb, slots=bad_slots)
        for k in range(3):
            sl = slice(k * PER, (k + 1) * PER)
            assert np.all(np.isnan(part[sl])) if k == bad else np.array_equal(part[sl], plain[sl]), (bad_slots, part)


def test_folded_peak_is_not_the_unnormalised_score(dev, aw):
    _, x, y, norm_passes = CASES["lr"]["peak-folded-2049"]
    assert norm_passes == 1
    assert not np.array_equal(_loss(dev, "lr", aw, x, y, 1), _loss(dev, "lr", aw, x, y, 0))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the evaluator and the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _plugins(chain="eq"):
    from st_ito import effects as E
    return E.make_plugins(chain)


def _ndims(plugins):
    return sum(p["num_params"] for p in plugins.values())


def _seeded_target(x, seed, chain="eq"):
    from st_ito.style_transfer import process_audio
    w = np.random.default_rng(seed).random(_ndims(_plugins(chain)))
    return torch.from_numpy(process_audio(x.numpy(), w, SR, _plugins(chain)))


def _assert_same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


@pytest.fixture(scope="module")
def pair():
    x = O.synth_audio(1234, 2, 4097)
    return x[None], _seeded_target(x, 3)[None]


@pytest.mark.parametrize("form", A.FORMS)
def test_objective_through_the_evaluator(dev, aw, pair, form):
    """The evaluator's fitness is the distance function's value on the normalised render it hands back."""
    from st_ito.engine import MrstftEvaluator, PrefilteredMrstftEvaluator
    from st_ito.features import compute_prefiltered_mrstft_distance as dist
    x, target = pair
    W = np.random.default_rng(11).random((4, _ndims(_plugins())))
    ev = PrefilteredMrstftEvaluator(x, SR, _plugins(), target, kind=form, prefilter="aw")
    loss, embeds, audio = ev.evaluate(list(W), parallel=True, want_audio=True)
    assert isinstance(ev, MrstftEvaluator) and embeds == {} and loss.shape == (4,) and audio.shape == (4, 2, 4097)
    assert ev._taps_dev is not None and ev._taps_dev.is_cuda and ev._taps_dev.numel() == 101
    want = dist(audio, target.to(dev), "aw", SR, kind=form)
    bar = A.bar(form, aw)
    err = _rel(loss.cpu().numpy(), want.cpu().numpy().astype(np.float64))
    print(f"{DISTANCE[form]} evaluator {loss.cpu().numpy()} distance of the render {want.cpu().numpy()} rel {err.max():.3e} (bar {bar:.3e})")
    assert torch.isfinite(loss).all() and err.max() <= bar


@pytest.mark.parametrize("form", A.FORMS)
def test_run_es_host_and_device(dev, pair, form):
    from st_ito.style_transfer import run_es
    x, target = pair
    kw = dict(distance=DISTANCE[form], popsize=4, max_iters=2, sigma0=0.33, seed=0, find_w0=False, parallel=True)
    res = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, **kw)
    assert res["num_evals"] == 8 and np.isfinite(res["fopt"]) and res["fopt"] > 0
    plain = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, **dict(kw, distance=DISTANCE[form][:-3]))
    assert plain["fopt"] != res["fopt"]
    on_dev = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, device_es=True, **kw)
    assert on_dev["num_evals"] == 8 and np.isfinite(on_dev["fopt"]) and on_dev["fopt"] > 0


def test_staged_es_runs(dev, pair, tmp_path):
    from st_ito.style_transfer import run_staged_es
    x, target = pair
    res = run_staged_es(x.clone(), target.clone(), SR, _plugins(), None, None, max_iters=2, popsize=4, sigma0=0.33, seed=2,
                        distance="mrstft-aw", run_dir=str(tmp_path))
    assert np.isfinite(res["fopt"]) and res["fopt"] > 0 and res["num_evals"] == 8


def test_ragged_batch_equals_run_es_on_every_pair_alone(dev):
    from st_ito.style_transfer import run_es, run_es_batch
    xs = [O.synth_audio(1350 + b, 1, n) * (0.5 + 0.1 * b) for b, n in enumerate((4097, 6000))]
    ts = [_seeded_target(x, 70 + b) for b, x in enumerate(xs)]
    kw = dict(max_iters=2, sigma0=0.33, popsize=4, early_stop=False, distance="mrstft-aw")
    res = run_es_batch(xs, ts, SR, _plugins(), None, None, seed=23, **kw)
    for b in range(2):
        one = run_es(xs[b][None].clone(), ts[b][None].clone(), SR, _plugins(), None, None, find_w0=False, seed=23 + b, **kw)
        _assert_same_run(res[b], one)
        assert res[b]["num_evals"] == 8 and np.isfinite(res[b]["fopt"]) and res[b]["fopt"] > 0
