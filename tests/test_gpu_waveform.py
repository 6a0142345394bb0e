"""GPU: the waveform distances (csrc/waveform.hip; kinds esr, dc, snr, sisdr, logcosh; distance="esr", "snr", "sisdr", "logcosh" and
their "-aw" forms) -- accuracy against the float64 reference of tests/waveform_ref.py on every case of its list and every kind,
exact zeros of the target against its own table, degenerate tap sets, the filter's orientation, independence of a candidate's bits
from what is around it, NaN containment, the folded peak, and the objective in the evaluator and in every ES driver.

The bar of a case is BAR_FACTOR = 4 times its yardstick (tests/test_waveform_host.py bounds it): the float32 torch restatement's
largest relative distance from the float64 reference over esr, snr and sisdr.  esr, snr, sisdr and logcosh are held to it
relative to the reference, dc to bar x esr_ref absolute (dc <= esr always, and its own value can be arbitrarily small).  Every case
prints its measured errors next to its bar (run with -s); profiles/waveform_edges.txt records them.

Populations of 4, 2 iterations, 4097 and 6000 samples through the "eq" chain."""
import numpy as np
import pytest
import torch

import st_ito_oracle as O
import waveform_ref as W

pytestmark = pytest.mark.gpu
SR = W.SR
TAPS = W.tap_sets()
NAMES = ("esr", "snr", "sisdr", "logcosh", "esr-aw", "snr-aw", "sisdr-aw", "logcosh-aw")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _t(a, dev):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).contiguous()


def _table(dev, y, taps):
    from st_ito.features import WaveformTarget
    return WaveformTarget(_t(y, dev), taps)


def _loss(dev, kind, taps, x, y, peaks=None, norm_passes=0, slots=None, table=None):
    """The loss of x (P, C, n) against the table of y (T, C, n) -> (P,) float32 on the host."""
    tgt = _table(dev, y, taps) if table is None else table
    sl = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
    pk = None if peaks is None else _t(peaks, dev)
    return tgt.loss(_t(x, dev), pk, norm_passes, slots=sl, kind=kind).cpu().numpy()


def _err(kind, got, ref):
    """The figure held to the bar: relative to the reference; dc: absolute, in units of esr_ref."""
    got = np.asarray(got, dtype=np.float64)
    if kind == "dc":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(got == ref["dc"], 0.0, np.abs(got - ref["dc"]) / ref["esr"])
    return W.relative(got, ref[kind])


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_name", list(TAPS))
def test_accuracy_against_the_float64_reference(dev, tap_name):
    """Every case of the tap set and every kind; the norm_passes 1 cases fold their peak in the kernel."""
    failures = []
    for case in W.cases(tap_name):
        name, x, y, peaks, norm_passes = case
        ref, bar = W.case_reference(tap_name, case), W.bar(tap_name, case)
        table = _table(dev, y, TAPS[tap_name])
        errs = {}
        for kind in W.KINDS:
            got = _loss(dev, kind, TAPS[tap_name], x, y, peaks, norm_passes, table=table)
            assert got.shape == (x.shape[0],) and got.dtype == np.float32 and np.all(np.isfinite(got)), (tap_name, name, kind, got)
            errs[kind] = float(_err(kind, got, ref).max())
            if not errs[kind] <= bar:
                failures.append((tap_name, name, kind, errs[kind], bar, got.tolist(), ref[kind].tolist()))
        print(f"{tap_name:6s} {name:22s} bar {bar:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert not failures, failures


@pytest.mark.parametrize("tap_name", list(TAPS))
def test_target_against_its_own_table_is_exactly_zero(dev, tap_name):
    for name in ("n5-c2", f"n{W.tile_samples(TAPS[tap_name]) + 1}-c3", f"n{2 * W.tile_samples(TAPS[tap_name]) + 3}-c1"):
        _, _, y, _, _ = [c for c in W.cases(tap_name) if c[0] == name][0]
        table = _table(dev, y, TAPS[tap_name])
        for kind in ("esr", "dc", "logcosh"):
            assert _loss(dev, kind, TAPS[tap_name], y, y, table=table).tolist() == [0.0] * y.shape[0], (tap_name, name, kind)
        one = _table(dev, y[:1], TAPS[tap_name])                          # one target, two candidates
        assert _loss(dev, "esr", TAPS[tap_name], np.concatenate([y[:1], y[:1]]), y[:1], table=one).tolist() == [0.0, 0.0]


def test_degenerate_taps(dev):
    """[1.0]: fma(1, x, 0) is x, the unfiltered call to one float32 ulp.  [0, 0, 1]: the unfiltered call on the rows shifted left by
    one sample with a zero appended."""
    tile = W.tile_samples(None)
    _, x, y, _, _ = [c for c in W.cases("none") if c[0] == f"n{tile + 1}-c2"][0]
    shift = lambda a: np.concatenate([a[..., 1:], np.zeros_like(a[..., :1])], -1)    # noqa: E731
    for kind in W.KINDS:
        plain = _loss(dev, kind, None, x, y)
        got = _loss(dev, kind, TAPS["unit"], x, y)
        assert np.all(np.abs(got - plain) <= np.spacing(np.abs(plain))), (kind, got, plain)
        shifted = _loss(dev, kind, None, shift(x), shift(y))
        got = _loss(dev, kind, TAPS["shift"], x, y)
        assert np.all(np.abs(got - shifted) <= np.spacing(np.abs(shifted))), (kind, got, shifted)
        assert not np.array_equal(got, plain)


def test_filter_orientation(dev):
    """The definition correlates: taps[k] meets row[i + k - c].  The reversed asymmetric FIR is another function, more than
    100 bars away in float64 and on the device -- on rows shorter than c, where the orientation decides WHICH taps meet the row (on
    long rows of white noise these sums see little but the filter's magnitude response, which reversal keeps)."""
    taps = TAPS["fir31"]
    assert np.abs(taps - taps[::-1]).max() > 1e-2
    case = [c for c in W.cases("fir31") if c[0] == "n5-c2"][0]
    _, x, y, _, _ = case
    ref, bar = W.case_reference("fir31", case), W.bar("fir31", case)
    rev = W.reference(x, y, taps[::-1].copy())
    for kind in ("esr", "snr", "sisdr", "logcosh"):
        got = _loss(dev, kind, taps, x, y)
        got_rev = _loss(dev, kind, taps[::-1].copy(), x, y)
        print(f"fir31 {kind}: reversed taps {W.relative(rev[kind], ref[kind]).min():.3e} away in float64, "
              f"{W.relative(got_rev, ref[kind]).min():.3e} on the device (bar {bar:.2e})")
        assert W.relative(rev[kind], ref[kind]).min() > 100 * bar and W.relative(got_rev, ref[kind]).min() > 100 * bar
        assert W.relative(got, ref[kind]).max() <= bar


@pytest.mark.parametrize("tap_name", ["none", "aw"])
def test_same_bits_whatever_is_around_the_candidate(dev, tap_name):
    """Alone; at every position of a batch of 6; under the slot lists [0], [2, 0], [1, 1, 0] against 3 targets; next to a slot of
    -1 or 3, which gives NaN for its population only."""
    taps = TAPS[tap_name]
    n = W.tile_samples(taps) + 5
    rng = np.random.default_rng(700)
    u = lambda *shape: rng.uniform(-0.9, 0.9, shape).astype(np.float32)    # noqa: E731
    cand, tgt, others, other_t = u(1, 2, n), u(1, 2, n), u(6, 2, n), u(3, 2, n)
    for kind in ("esr", "sisdr", "logcosh"):
        alone = _loss(dev, kind, taps, cand, tgt)[0]
        assert np.isfinite(alone) and alone != 0
        for pos in range(6):
            xb = others.copy()
            xb[pos] = cand[0]
            assert _loss(dev, kind, taps, xb, tgt)[pos] == alone, (kind, pos)
        tb = other_t.copy()
        tb[0] = tgt[0]
        table = _table(dev, tb, taps)
        for slots in ([0], [2, 0], [1, 1, 0]):       # the candidate opens the population that reads target 0
            k = slots.index(0)
            xb = others[:2 * len(slots)].copy()
            xb[2 * k] = cand[0]
            got = _loss(dev, kind, taps, xb, tb, slots=slots, table=table)
            assert got[2 * k] == alone and np.all(np.isfinite(got)), (kind, slots, got)
        xb = others.copy()
        xb[4] = cand[0]
        plain = _loss(dev, kind, taps, xb, tb, slots=[1, 1, 0], table=table)
        for bad_slots, bad in (([-1, 1, 0], 0), ([1, 3, 0], 1)):
            part = _loss(dev, kind, taps, xb, tb, slots=bad_slots, table=table)
            for k in range(3):
                sl = slice(2 * k, 2 * k + 2)
                assert np.all(np.isnan(part[sl])) if k == bad else np.array_equal(part[sl], plain[sl]), (kind, bad_slots, part)
            assert part[4] == alone


@pytest.mark.parametrize("tap_name", ["none", "fir31"])
def test_a_nan_stays_in_its_candidate(dev, tap_name):
    taps = TAPS[tap_name]
    n = W.tile_samples(taps) + 1
    _, x, y, _, _ = [c for c in W.cases(tap_name) if c[0] == f"n{n}-c2"][0]
    x3, y3 = np.concatenate([x, x[:1]]), np.concatenate([y, y[:1]])
    for kind in W.KINDS:
        clean = _loss(dev, kind, taps, x3, y3)
        for where in (0, n - 1):
            bad = x3.copy()
            bad[1, 1, where] = np.nan
            got = _loss(dev, kind, taps, bad, y3)
            assert np.isnan(got[1]) and got[0] == clean[0] and got[2] == clean[2], (kind, where, got, clean)


@pytest.mark.parametrize("tap_name", ["none", "aw"])
def test_folded_peak_agrees_with_the_call_on_a_normalised_copy(dev, tap_name):
    case = [c for c in W.cases(tap_name) if c[0] == f"peak-folded-n{W.tile_samples(TAPS[tap_name]) + 1}"][0]
    _, x, y, peaks, norm_passes = case
    assert norm_passes == 1
    bar = W.bar(tap_name, case)
    for kind in W.KINDS:
        folded = _loss(dev, kind, TAPS[tap_name], x, y, peaks, 1)
        copy = _loss(dev, kind, TAPS[tap_name], W.scored32(x, peaks, 1), y)
        raw = _loss(dev, kind, TAPS[tap_name], x, y)
        assert W.relative(folded, copy.astype(np.float64)).max() <= bar, (kind, folded, copy)
        assert kind == "sisdr" or not np.array_equal(folded, raw), (kind, folded, raw)        # sisdr does not see a scale


def test_compute_waveform_distance_is_that_loss(dev):
    from st_ito.features import compute_waveform_distance as dist
    _, x, y, _, _ = [c for c in W.cases("aw") if c[0] == "n5-c2"][0]
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    for kind in W.KINDS:
        got = dist(xt.to(dev), yt.to(dev), kind, "aw", SR)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (W.P,)
        assert np.array_equal(got.cpu().numpy(), _loss(dev, kind, TAPS["aw"], x, y))
        assert torch.equal(dist(xt, yt, kind, TAPS["aw"]), got.cpu())        # host tensors in, host tensor out; the taps as an array
        assert torch.equal(dist(xt[:1], yt[:1], kind, "aw", SR), got[:1].cpu())
    assert np.array_equal(dist(xt, yt[:1]).numpy(), _loss(dev, "esr", None, x, y[:1]))   # y of batch 1, the defaults


# ---------------------------------------------------------------------------------------------------------------------------
# the evaluator and the drivers
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


def _close_to_the_distance_of_the_render(kind, loss, audio, target, taps):
    """The evaluator scores x * (1 / peak), the audio it hands back is x / peak: one float32 rounding per sample apart, an error of
    the yardstick's kind.  Held to 4 yardsticks of that audio, relative -- a dB value relative to at least 10 / ln 10 dB, which is
    what a relative error of the power ratio moves it by."""
    got, want = loss.cpu().numpy().astype(np.float64), W.reference(audio.cpu().numpy(), target.cpu().numpy(), taps)[kind]
    bar = W.BAR_FACTOR * W.yardstick_of(audio.cpu().numpy(), target.cpu().numpy(), taps)
    scale = np.maximum(np.abs(want), 10.0 / np.log(10.0)) if kind in ("snr", "sisdr") else np.abs(want)
    print(f"evaluator {kind}: {got} float64 of the render {want} (bar {bar:.2e})")
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bar * scale), (kind, got, want, bar)


@pytest.mark.parametrize("kind,prefilter", [("esr", None), ("sisdr", "aw"), ("logcosh", None), ("snr", "aw")])
def test_objective_through_the_evaluator(dev, kind, prefilter):
    """The evaluator's fitness is the distance of the normalised render it hands back; and it has the same bits (a candidate's bits
    do not depend on its batch) for all pairs, under pairs=, x= / y=, and for a population that is already on the device."""
    from st_ito.engine import MrstftEvaluator, WaveformEvaluator
    xs = torch.stack([O.synth_audio(1234 + b, 2, 6000) for b in range(2)])
    ts = torch.stack([_seeded_target(x, 3 + b) for b, x in enumerate(xs)])
    Wp = np.random.default_rng(11).random((8, _ndims(_plugins())))
    ev = WaveformEvaluator(xs, SR, _plugins(), ts, kind=kind, prefilter=prefilter)
    assert isinstance(ev, MrstftEvaluator)
    loss, embeds, audio = ev.evaluate(list(Wp), parallel=True, want_audio=True)
    assert embeds == {} and loss.shape == (8,) and audio.shape == (8, 2, 6000) and torch.isfinite(loss).all()
    taps = None if prefilter is None else TAPS[prefilter]
    for b in range(2):
        _close_to_the_distance_of_the_render(kind, loss[4 * b:4 * b + 4], audio[4 * b:4 * b + 4], ts[b:b + 1], taps)
    if prefilter is not None:
        assert ev._taps_dev is not None and ev._taps_dev.is_cuda and ev._taps_dev.numel() == 101
    one, _, _ = ev.evaluate(Wp[4:], parallel=True, pairs=[1])
    assert torch.equal(one, loss[4:])
    xd, td = xs.to(dev), ts.to(dev)
    moving, _, _ = ev.evaluate(Wp[:4], pairs=[0], x=xd[:1].contiguous(), y=td[:1].contiguous())
    assert torch.equal(moving, loss[:4])
    static, _, _ = ev.evaluate(Wp[4:], pairs=[1], x=xd[1:].contiguous())
    assert torch.equal(static, loss[4:])
    on_dev, _, _ = ev.evaluate(torch.from_numpy(Wp).to(dev), parallel=True)
    assert torch.equal(on_dev, loss)
    with pytest.raises(ValueError, match="dropout"):
        ev.evaluate(list(Wp), dropout=0.1)


def test_evaluator_with_random_crop(dev):
    """One crop for input and target: the fitness is the distance of the render of the crop to the target's crop at the same start."""
    from st_ito import engine
    from st_ito.features import compute_waveform_distance as dist
    n = engine.CROP_LEN + 3 * engine.CROP_MARGIN
    x = O.synth_audio(77, 1, n)[None]
    t = (0.7 * torch.roll(x, 3, -1) + 0.01).contiguous()
    Wp = np.random.default_rng(12).random((2, _ndims(_plugins())))
    ev = engine.WaveformEvaluator(x, SR, _plugins(), t, kind="esr")
    loss, _, audio = ev.evaluate(list(Wp), random_crop=True, rng=np.random.RandomState(5), want_audio=True)
    start = engine.crop_start(n, True, np.random.RandomState(5))
    assert start >= engine.CROP_MARGIN and audio.shape == (2, 1, engine.CROP_LEN)
    _close_to_the_distance_of_the_render("esr", loss, audio, t[..., start:start + engine.CROP_LEN], None)
    elsewhere = dist(audio, t[..., :engine.CROP_LEN].to(dev), "esr")
    assert torch.all((loss - elsewhere).abs() > 1e-3 * loss.abs())


def test_polarity_is_seen(dev):
    """A target equal to the input with both channels negated: esr is 4 (d = 2 x), where the MR-STFT distance is exactly 0."""
    from st_ito.features import compute_mrstft_distance, compute_waveform_distance
    x = O.synth_audio(1234, 2, 4097)[None]
    x = x / x.abs().max()
    bar = W.BAR_FACTOR * W.yardstick_of(x.numpy(), -x.numpy())
    esr = compute_waveform_distance(x.to(dev), (-x).to(dev), "esr").item()
    print(f"polarity: esr {esr!r} (bar {bar:.2e}), mrstft {compute_mrstft_distance(x.to(dev), (-x).to(dev)).item()!r}")
    assert abs(esr - 4.0) <= bar * 4.0
    assert compute_mrstft_distance(x.to(dev), (-x).to(dev)).item() == 0.0
    assert compute_waveform_distance(x.to(dev), x.to(dev), "esr").item() == 0.0


@pytest.mark.parametrize("distance", NAMES)
def test_run_es(dev, pair, distance):
    from st_ito.style_transfer import run_es
    x, target = pair
    kw = dict(distance=distance, popsize=4, max_iters=2, sigma0=0.33, seed=0, find_w0=False, parallel=True)
    res = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, **kw)
    assert res["num_evals"] == 8 and np.isfinite(res["fopt"])
    if distance in ("esr", "esr-aw", "logcosh", "logcosh-aw"):
        assert res["fopt"] > 0
    if distance in ("esr", "sisdr-aw"):
        on_dev = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, device_es=True, **kw)
        assert on_dev["num_evals"] == 8 and np.isfinite(on_dev["fopt"])
    if distance.endswith("-aw"):
        plain = run_es(x.clone(), target.clone(), SR, _plugins(), None, None, **dict(kw, distance=distance[:-3]))
        assert plain["fopt"] != res["fopt"]


@pytest.mark.parametrize("distance", ["esr", "snr-aw"])
def test_staged_es_runs(dev, pair, tmp_path, distance):
    from st_ito.style_transfer import run_staged_es
    x, target = pair
    res = run_staged_es(x.clone(), target.clone(), SR, _plugins(), None, None, max_iters=2, popsize=4, sigma0=0.33, seed=2,
                        distance=distance, run_dir=str(tmp_path))
    assert np.isfinite(res["fopt"]) and res["num_evals"] == 8


@pytest.mark.parametrize("distance", ["esr", "sisdr", "logcosh-aw"])
def test_batch_equals_run_es_on_every_pair_alone(dev, distance):
    """The list form (4097 and 6000 samples) and the tensor form: pair b is bit for bit run_es of pair b alone."""
    from st_ito.style_transfer import run_es, run_es_batch
    xs = [O.synth_audio(1350 + b, 1, n) * (0.5 + 0.1 * b) for b, n in enumerate((4097, 6000))]
    ts = [_seeded_target(x, 70 + b) for b, x in enumerate(xs)]
    kw = dict(max_iters=2, sigma0=0.33, popsize=4, early_stop=False, distance=distance)
    res = run_es_batch([x.clone() for x in xs], [t.clone() for t in ts], SR, _plugins(), None, None, seed=23, **kw)
    for b in range(2):
        one = run_es(xs[b][None].clone(), ts[b][None].clone(), SR, _plugins(), None, None, find_w0=False, seed=23 + b, **kw)
        _assert_same_run(res[b], one)
        assert res[b]["num_evals"] == 8 and np.isfinite(res[b]["fopt"])
    xb = torch.stack([xs[0], 0.8 * xs[0].flip(-1)])
    tb = torch.stack([ts[0], _seeded_target(xb[1], 75)])
    res = run_es_batch(xb.clone(), tb.clone(), SR, _plugins(), None, None, seed=31, **kw)
    for b in range(2):
        one = run_es(xb[b][None].clone(), tb[b][None].clone(), SR, _plugins(), None, None, find_w0=False, seed=31 + b, **kw)
        _assert_same_run(res[b], one)
