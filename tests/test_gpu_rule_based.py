"""The PST benchmark's baselines on the GPU: run_rule_based (csrc/matcheq.hip + the mean-spectrum mode and raw meter of
features.hip) kernel by kernel through the C ABI and end to end against the restatement of tests/rule_based_ref.py,
run_random against the oracle's render, and run_pst_benchmark with every built method.  Every case prints its measured
error next to its bar (run with -s)."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.signal
import torch

import rule_based_ref as R
import st_ito_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:A window was not provided")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _report(name, err, bar):
    print(f"[rule-based] {name}: err {err:.3e} (bar {bar:.0e})")
    assert err <= bar, (name, err, bar)   # a NaN fails here too


def _ulps32(got, ref64):
    """|got - ref| in float32 ulps of the correctly rounded reference (ulp of the smallest normal near zero)."""
    ref32 = np.asarray(ref64, dtype=np.float32)
    return float((np.abs(np.asarray(got, np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32))).max())


def _sig(kind, seed, chs, n, sr):
    x, t = R.case_signals(seed, chs, n, sr)
    if kind == "compressed":      # a saturated target: loud for its peak, so the climb takes 40 or more steps
        t = np.tanh(2.0 * t / np.abs(t).max()).astype(np.float32)
    elif kind == "quiet":         # a target that fades in: quieter than the input, no step
        t = (t * np.linspace(0, 1, n, dtype=np.float32) ** 8).astype(np.float32)
    elif kind == "square":        # crest factor 1: no compression reaches it, 160 steps to -80 dB
        t = np.sign(t).astype(np.float32)
    return x, t


# ---------------------------------------------------------------- kernel by kernel
@pytest.mark.parametrize("chs, n, n_fft", [(2, 48000, 16384), (1, 24000, 16384), (2, 9000, 2048), (1, 40000, 32768), (2, 16385, 32768)])
def test_mean_spectrum(dev, chs, n, n_fft):
    from st_ito import matcheq
    x = np.stack([R.peak_normalize(R.case_signals(40 + i, chs, n, 48000)[i % 2]) for i in range(3)])
    got = matcheq.mean_spectrum(torch.from_numpy(x).to(dev), n_fft).cpu().numpy()
    err = max(float(np.abs(got[b] - R.average_spectrum(x[b], n_fft)).max() / np.abs(R.average_spectrum(x[b], n_fft)).max())
              for b in range(3))
    _report(f"mean spectrum chs={chs} n={n} n_fft={n_fft} (x row max)", err, 1e-5)


@pytest.mark.parametrize("n", [8193, 1025, 2000, 16385])
def test_savgol(dev, n):
    from st_ito import matcheq
    rng = np.random.default_rng(n)
    rows = (np.abs(rng.standard_normal((4, n))) * np.logspace(-3, 2, 4)[:, None]).astype(np.float32)
    rows[1] = np.cumsum(rows[1]).astype(np.float32)      # a smooth ramp: edges dominated by the polynomial fit
    got = matcheq.savgol(torch.from_numpy(rows).to(dev)).cpu().numpy()
    ref = np.stack([scipy.signal.savgol_filter(r, 1025, 2) for r in rows])
    assert ref.dtype == np.float32
    _report(f"savgol n={n} (float32 ulps)", _ulps32(got, ref.astype(np.float64)), 1.0)


@pytest.mark.parametrize("n_taps, sr", [(2048, 48000), (2048, 44100), (16, 48000), (17, 48000), (4096, 48000), (1000, 22050)])
def test_firwin2(dev, n_taps, sr):
    from st_ito import matcheq
    rng = np.random.default_rng(n_taps)
    nb = 8193
    num = scipy.signal.savgol_filter(np.abs(rng.standard_normal((3, nb))).astype(np.float32) + 0.1, 1025, 2, axis=-1)
    den = scipy.signal.savgol_filter(np.abs(rng.standard_normal((3, nb))).astype(np.float32) + 0.1, 1025, 2, axis=-1)
    got = matcheq.firwin2(torch.from_numpy(num).to(dev), torch.from_numpy(den).to(dev), sr, n_taps).cpu().numpy()
    err = 0.0
    for b in range(3):
        ref = R.design_taps(den[b], num[b], sr, n_taps)
        err = max(err, float(np.abs(got[b] - ref).max() / np.abs(ref).max()))
    _report(f"firwin2 n_taps={n_taps} sr={sr} (x max|tap|)", err, 1e-13)


@pytest.mark.parametrize("bs, chs, n, n_taps", [(2, 2, 1000, 2048), (2, 1, 48000, 2048), (1, 2, 480000, 2048), (1, 2, 1440000, 2048),
                                                (3, 2, 5000, 17), (1, 1, 70000, 4096)])
def test_fir(dev, bs, chs, n, n_taps):
    from st_ito import matcheq
    rng = np.random.default_rng(n + n_taps)
    x = (rng.standard_normal((bs, chs, n)) * 0.3).astype(np.float32)
    x[0, 0, n // 3: n // 3 + 100] = 0.0
    taps = rng.standard_normal((bs, n_taps)) * np.hamming(n_taps) / np.sqrt(n_taps)
    got = matcheq.fir(torch.from_numpy(x).to(dev), torch.from_numpy(taps).to(dev)).cpu().numpy()
    worst = 0.0
    for b in range(bs):
        ref = scipy.signal.lfilter(taps[b], [1.0], x[b])
        d = np.abs(got[b].astype(np.float64) - ref.astype(np.float32).astype(np.float64))
        ok_abs = np.abs(got[b].astype(np.float64) - ref) <= 1e-12
        u = np.where(ok_abs, 0.0, d / np.spacing(np.abs(ref.astype(np.float32))))
        worst = max(worst, float(u.max()))
    _report(f"FIR bs={bs} chs={chs} n={n} taps={n_taps} (float32 ulps, 1e-12 abs near zero)", worst, 1.0)


@pytest.mark.parametrize("chs, n, sr", [(2, 48000, 48000), (1, 44100, 44100), (2, 19200, 48000), (1, 100000, 48000)])
def test_lufs_raw(dev, chs, n, sr):
    from st_ito import matcheq
    from st_ito.loudness import integrated_loudness
    x = np.stack([R.case_signals(50 + i, chs, n, sr)[0] * np.float32(10.0 ** -i) for i in range(4)])
    x[3, :, n // 4: n // 2] = 0.0
    got = matcheq.lufs_raw(torch.from_numpy(x).to(dev), sr).cpu().numpy()
    assert got.dtype == np.float64
    ref = np.array([integrated_loudness(x[b].T, sr) for b in range(4)])
    with np.errstate(invalid="ignore"):
        d = np.where(got == ref, 0.0, np.abs(got - ref))   # equal infinities (a silent item) count as exact
    _report(f"raw LUFS chs={chs} n={n} sr={sr} (LU)", float(d.max()), 1e-6)


# ---------------------------------------------------------------- end to end
def _compare(name, x, t, sr):
    """run_rule_based on copies of (bs, chs, n) x / t against the restatement: step counts where the trace keeps 1e-3 LU from
    the 0.25 LU decision, outputs within 1e-4 of the peak, and the caller's tensors normalised in place."""
    from st_ito.style_transfer import run_rule_based
    ref = R.run_rule_based(x, t, sr)
    xt, tt = torch.from_numpy(x.copy()), torch.from_numpy(t.copy())
    got = run_rule_based(xt, tt, sr, None, None)["output_audio"]
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == x.shape
    assert torch.equal(xt, torch.from_numpy(ref["inputs"])) and torch.equal(tt, torch.from_numpy(ref["targets"]))
    g = got.numpy()
    for b in range(x.shape[0]):
        margin = float(np.abs(np.asarray(ref["deltas"][b]) - 0.25).min())
        err = float(np.abs(g[b] - ref["output"][b]).max() / np.abs(ref["output"][b]).max())
        print(f"[rule-based] {name} item {b}: restatement steps {ref['steps'][b]} (margin {margin:.3e} LU), output err {err:.3e} "
              "(bar 1e-04 x peak)")
        assert margin > 1e-3, "choose signals whose trace stays clear of the decision"
        assert err <= 1e-4
    return got, ref


def test_rule_based_stereo_48k_compressed_target(dev):
    x, t = _sig("compressed", 31, 2, 48000, 48000)
    got, ref = _compare("stereo 48k compressed", x[None], t[None], 48000)
    assert ref["steps"][0] >= 40


def test_rule_based_mono_44k(dev):
    x, t = _sig("compressed", 32, 1, 44100, 44100)
    _, ref = _compare("mono 44.1k compressed", x[None], t[None], 44100)
    assert ref["steps"][0] >= 40
    x, t = _sig("quiet", 33, 1, 44100, 44100)
    _, ref = _compare("mono 44.1k quieter target", x[None], t[None], 44100)
    assert ref["steps"][0] == 0


def test_rule_based_unreachable_target_runs_160_steps(dev):
    from st_ito import matcheq
    x, t = _sig("square", 34, 2, 48000, 48000)
    _, ref = _compare("stereo 48k unreachable", x[None], t[None], 48000)
    assert ref["steps"][0] == 160
    # the climb's own state: 160 steps, threshold at -80 dB
    y = torch.from_numpy(ref["eq"][0]["filtered"][None].copy()).to(dev)
    matcheq.peak_normalize_(y)
    ts = matcheq.peak_normalize_(torch.from_numpy(t[None].copy()).to(dev))
    steps, delta, thr = matcheq.hill_climb_(y, matcheq.lufs_raw(y, 48000), matcheq.lufs_raw(ts, 48000), 48000)
    assert int(steps[0]) == 160 and float(thr[0]) == -80.0 and float(delta[0]) > 0.25


def test_rule_based_batch_equals_single_items(dev):
    """Three items with 0, 40+ and 160 steps advance in lockstep; every item's output is bit for bit its single-item call's."""
    from st_ito.style_transfer import run_rule_based
    pairs = [_sig("quiet", 61, 2, 48000, 48000), _sig("compressed", 31, 2, 48000, 48000), _sig("square", 34, 2, 48000, 48000)]
    x = np.stack([p[0] for p in pairs])
    t = np.stack([p[1] for p in pairs])
    batch = run_rule_based(torch.from_numpy(x.copy()), torch.from_numpy(t.copy()), 48000, None, None)["output_audio"]
    for b in range(3):
        single = run_rule_based(torch.from_numpy(x[b:b + 1].copy()), torch.from_numpy(t[b:b + 1].copy()), 48000, None, None)["output_audio"]
        assert torch.equal(batch[b], single[0]), b
    ref = R.run_rule_based(x, t, 48000)
    assert ref["steps"][0] == 0 and ref["steps"][1] >= 40 and ref["steps"][2] == 160
    err = float(np.abs(batch.numpy() - ref["output"]).max() / np.abs(ref["output"]).max())
    _report("batch of 3 against the restatement (x peak)", err, 1e-4)


def test_rule_based_all_zero_item_is_nan_and_alone(dev):
    """An all-zero item: 0 / 0 in its response makes its output NaN, as in the reference (torch.max propagates NaN, and so
    does the peak kernel); the other item is untouched by it and the call ends."""
    from st_ito.style_transfer import run_rule_based
    x, t = _sig("compressed", 31, 2, 48000, 48000)
    xs = np.stack([np.zeros_like(x), x])
    ts = np.stack([np.zeros_like(t), t])
    out = run_rule_based(torch.from_numpy(xs), torch.from_numpy(ts), 48000, None, None)["output_audio"]
    alone = run_rule_based(torch.from_numpy(x[None].copy()), torch.from_numpy(t[None].copy()), 48000, None, None)["output_audio"]
    assert bool(torch.isnan(out[0]).all())
    assert torch.equal(out[1], alone[0])


def test_rule_based_bad_shapes(dev):
    from st_ito.style_transfer import run_rule_based
    for shape, sr in (((1, 3, 48000), 48000), ((1, 2, 14400), 48000), ((1, 2, 8192), 16000)):
        x = torch.rand(*shape)
        with pytest.raises(ValueError):
            run_rule_based(x, x.clone(), sr, None, None)


# ---------------------------------------------------------------- run_random
def test_run_random_against_the_oracle(dev):
    from st_ito.effects import BasicCompressor, BasicParametricEQ, BasicReverb
    from st_ito.style_transfer import load_plugins, run_random
    one = lambda cls, nch: {"class_path": cls, "num_params": None, "num_channels": nch, "fixed_parameters": {}}  # noqa: E731
    plugins = load_plugins({"ParametricEQ": one(BasicParametricEQ, 1), "Compressor": one(BasicCompressor, 1),
                            "Reverb": one(BasicReverb, 2)})[0]
    oplugins = O.make_plugins(["ParametricEQ", "Compressor", "Reverb"], with_bypass=True)
    D = sum(p["num_params"] for p in plugins.values())
    x = O.synth_audio(71, 2, 48000)
    torch.manual_seed(99)
    res = run_random(x[None].clone(), x[None].clone(), 48000, plugins, None)
    torch.manual_seed(99)
    w = torch.rand(D)
    ref = O.process_audio(x.numpy(), w.numpy(), 48000, oplugins)
    ref_params = O.parameters_to_dict(w.numpy(), oplugins)
    for plug in ref_params:
        for k, v in ref_params[plug].items():
            assert res["param_dict"][plug][k] == pytest.approx(float(v), rel=1e-12, abs=0), (plug, k)
    _report("run_random audio vs oracle.process_audio", float(np.abs(res["output_audio"][0].numpy() - ref).max()), 2e-5)


# ---------------------------------------------------------------- the harness
def _harness():
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import eval_pst
    return eval_pst


def test_eval_pst_all_methods(dev, tmp_path):
    eval_pst = _harness()
    from st_ito.utils import make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    pairs = eval_pst.synthetic_pairs(2, 1.0, eval_pst.get_plugins("mastering-pb"))
    res = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins("mastering-pb"), pm, str(tmp_path), max_iters=2, popsize=6,
                                     random_crop=False, seed=3, tag="m", methods=("input", "random", "rule-based", "style-es"))
    assert list(res) == ["input", "random", "rule-based", "style-es (param-panns)"]
    for m, r in res.items():
        assert len(r["style_features"]) == 2 and len(r["time_elapsed"]) == 2, m
        assert all(-1.0 <= v <= 1.0 for v in r["style_features"]), m
    for i in range(2):
        for stem in ("input", "random", "rule-based", "style-es", "target"):
            assert (tmp_path / f"{i:02d}_{stem}_m.wav").exists(), (i, stem)
        assert (tmp_path / f"{i:02d}_style-es_m.json").exists()
        assert not (tmp_path / f"{i:02d}_random_m.json").exists()
    with pytest.raises(NotImplementedError):
        eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins("mastering-pb"), pm, str(tmp_path), methods=("deepafx-st",))


def test_eval_pst_default_methods_unchanged(dev, tmp_path):
    eval_pst = _harness()
    from st_ito.utils import make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    pairs = eval_pst.synthetic_pairs(2, 1.0, eval_pst.get_plugins("mastering-pb"))
    kw = dict(max_iters=2, popsize=6, random_crop=False, seed=3, tag="m")
    a = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins("mastering-pb"), pm, str(tmp_path / "a"), **kw)
    b = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins("mastering-pb"), pm, str(tmp_path / "b"), methods=("input", "style-es"), **kw)
    assert list(a) == list(b) == ["input", "style-es (param-panns)"]
    for m in a:
        assert a[m]["style_features"] == b[m]["style_features"]
    for i in range(2):
        pa = json.load(open(tmp_path / "a" / f"{i:02d}_style-es_m.json"))
        pb = json.load(open(tmp_path / "b" / f"{i:02d}_style-es_m.json"))
        assert pa == pb
