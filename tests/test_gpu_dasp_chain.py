"""GPU tests of the dasp-pytorch effect family as chain stages (STITO_FX_DASP_EQ / _DASP_COMPRESSOR / _DASP_DISTORTION, the
"autodiff" chain, the apply_* call surface) against tests/dasp_ref64.py: the float64 restatement that applies its filters by FFT
like the library, pinned on the CPU by tests/test_dasp_ref64.py.

Bars: 2e-5 of the output peak per stage (the single-effect bar of DESIGN.md section 2), 1e-4 of the peak for the five-stage chain
(the soak's chain bar).  Every figure is printed before it is asserted.

Run with:  python -m pytest tests/test_gpu_dasp_chain.py -m gpu -s
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import dasp_ref64 as R

pytestmark = pytest.mark.gpu
SR = 48000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 3, 37, 511, 512, 513, 4096, 100003, 262144)   # 2, 3, 37: N = 4 .. 128, where I - A^N is closest to singular
STAGE_BAR = 2e-5
CHAIN_BAR = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _audio(seed, chs, n):
    """noise + a 20 Hz and a 1 kHz tone, correlated right channel, float32, peak below 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    left = 0.15 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 20 * t + 0.3) + 0.2 * np.sin(2 * np.pi * 1000 * t)
    chans = [left] + ([0.6 * left + 0.1 * rng.standard_normal(n)] if chs == 2 else [])
    return torch.from_numpy(np.stack(chans).astype(np.float32))


def _stage_params(stage):
    """seeded random draws plus every range corner: for the EQ the eight corners of (gain, frequency, Q) on all six sections at
    once (the 20 Hz / Q 10 / +18 dB corner among them), for the compressor all 64, for the distortion both"""
    n_par = {"eq": 18, "comp": 6, "dist": 1}[stage]
    draws = np.random.default_rng({"eq": 100, "comp": 200, "dist": 300}[stage]).random((4, n_par))
    if stage == "eq":
        corners = [list(c) * 6 for c in itertools.product((0.0, 1.0), repeat=3)]
    else:
        corners = [list(c) for c in itertools.product((0.0, 1.0), repeat=n_par)]
    return torch.from_numpy(np.concatenate([draws, np.array(corners)], 0))


def _rel_errors(got, ref):
    """per item: max |got - ref| over the item / the item's reference peak (an all-zero reference must be met exactly)"""
    got, ref = got.double(), ref.double()
    bs = ref.shape[0]
    diff = (got - ref).abs().reshape(bs, -1).amax(1)
    peak = ref.abs().reshape(bs, -1).amax(1)
    return torch.where(peak > 0, diff / peak.clamp(min=1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), diff))


@pytest.mark.parametrize("chs", [1, 2])
@pytest.mark.parametrize("stage", ["eq", "comp", "dist"])
def test_stage_vs_ref64(dev, stage, chs):
    from st_ito import effects as E
    fn, ref_fn = {"eq": (E.apply_parametric_eq, R.parametric_eq), "comp": (E.apply_compressor, R.compressor),
                  "dist": (E.apply_distortion, R.distortion)}[stage]
    P = _stage_params(stage)
    worst = {}
    for n in LENGTHS:
        x = _audio(7 + n % 97, chs, n)[None].repeat(P.shape[0], 1, 1).contiguous()
        got = fn(x, P, SR)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (P.shape[0], chs, n)
        err = _rel_errors(got.cpu(), ref_fn(x, P, SR))
        worst[n] = (float(err.max()), int(err.argmax()))
        print(f"{stage} chs={chs} n={n}: worst error {worst[n][0]:.2e} of peak (parameter set {worst[n][1]} of {P.shape[0]})")
    for n, (e, i) in worst.items():
        assert e < STAGE_BAR, (stage, chs, n, i, e)


@pytest.mark.parametrize("chs", [1, 2])
def test_stages_and_chain_vs_ref64_with_different_audio_per_item(dev, chs):
    """The apply_* path hands the render as many inputs as candidates.  Here every item has its own audio, so a stage that paired
    item b's parameters with another item's samples would miss ref64; same parameter sets and bars as above."""
    from st_ito import effects as E
    n = 4099
    for stage, fn, ref_fn in (("eq", E.apply_parametric_eq, R.parametric_eq), ("comp", E.apply_compressor, R.compressor),
                              ("dist", E.apply_distortion, R.distortion)):
        P = _stage_params(stage)
        x = torch.stack([_audio(500 + 3 * b, chs, n) * (0.4 + 0.6 * (b % 5) / 4) for b in range(P.shape[0])])
        err = _rel_errors(fn(x, P, SR).cpu(), ref_fn(x, P, SR))
        print(f"{stage} chs={chs} n={n}, audio differs per item: worst error {float(err.max()):.2e} of peak (item {int(err.argmax())} of {P.shape[0]})")
        assert float(err.max()) < STAGE_BAR, (stage, chs, err)
    W = torch.from_numpy(np.random.default_rng(9).random((8, 51)))
    x = torch.stack([_audio(700 + b, chs, n) for b in range(8)])
    ref = R.complex_autodiff_processor(x, W, SR, E.NoiseShapedReverb(sample_rate=SR, seed=0).noise_bank)
    err = _rel_errors(E.apply_complex_autodiff_processor(x, W, SR).cpu(), ref)
    print(f"autodiff chain chs={chs} n={n}, audio differs per item: per-item error of peak max {float(err.max()):.2e}")
    assert float(err.max()) < CHAIN_BAR, err


def _chain_inputs(n=100003, pop=32, chs=2):
    x = _audio(31, chs, n)
    W = np.random.default_rng(5).random((pop, 51))
    return x, W


def test_autodiff_chain_vs_ref64_pop32(dev):
    """EQ -> compressor -> distortion -> noise-shaped reverb -> gain, one render of 32 candidates, each against ref64."""
    from st_ito import effects as E, engine
    for chs in (1, 2):
        x, W = _chain_inputs(chs=chs)
        pp = E.make_plugins("autodiff")
        audio, peaks = engine.render_population(pp, x.to(dev), torch.from_numpy(W).to(dev), SR)
        assert tuple(audio.shape) == (32, 2, x.shape[-1])
        bank = pp["Reverb"]["instance"].noise_bank
        ref = R.complex_autodiff_processor(x[None].repeat(32, 1, 1), torch.from_numpy(W), SR, bank)
        err = _rel_errors(audio.cpu(), ref)
        print(f"autodiff chain chs={chs}: per-candidate error of peak max {float(err.max()):.2e} median {float(err.median()):.2e}")
        assert float(err.max()) < CHAIN_BAR, err
        np.testing.assert_allclose(peaks.cpu().numpy(), audio.abs().amax(dim=(1, 2)).cpu().numpy(), rtol=0, atol=0)


def test_eq_cross_check_against_the_float32_library_arithmetic(dev):
    """ref64's precision="float32" mode runs the library's own float32 FFT pipeline.  With every cutoff >= 100 Hz that pipeline is
    well conditioned (below, it is not: DESIGN.md section 2), so the kernel must agree with it to the larger of 2e-5 and twice the
    distance the float32 mode itself has from float64 -- twice because both sides carry float32 rounding.  That distance is
    measured here, printed, and written to $STITO_MEASURE_DIR/dasp_eq_float32_cross_check.txt when that is set (the figure in
    profiles/dasp_chain.txt comes from there)."""
    from st_ito import effects as E
    rng = np.random.default_rng(17)
    P = rng.random((6, 18))
    lo = (100.0 - 20.0) / (20000.0 - 20.0)
    P[:, 1::3] = lo + (1 - lo) * P[:, 1::3]   # cutoffs 100 .. 20 000 Hz
    P = torch.from_numpy(P)
    x = torch.from_numpy((0.3 * rng.standard_normal((1, 1, 262144))).astype(np.float32)).repeat(6, 1, 1).contiguous()
    ref64, ref32 = R.parametric_eq(x, P, SR), R.parametric_eq(x, P, SR, precision="float32")
    own = float(_rel_errors(ref32, ref64).max())
    got = E.apply_parametric_eq(x, P, SR).cpu()
    e32, e64 = float(_rel_errors(got, ref32).max()), float(_rel_errors(got, ref64).max())
    bar = max(STAGE_BAR, 2 * own)
    line = (f"dasp EQ, six draws, cutoffs >= 100 Hz, n = 262144: float32 library arithmetic vs float64 {own:.2e}; "
            f"kernel vs float32 mode {e32:.2e} (bar {bar:.2e}); kernel vs float64 {e64:.2e}")
    print(line)
    if os.environ.get("STITO_MEASURE_DIR"):
        with open(os.path.join(os.environ["STITO_MEASURE_DIR"], "dasp_eq_float32_cross_check.txt"), "w") as f:
            f.write(line + "\n")
    assert e32 < bar, (e32, bar)


def test_fitness_and_audio_independent_of_batch_position_and_size(dev):
    """pop 1 against pop 32, bit for bit."""
    import st_ito_oracle as O
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    x = O.synth_audio(21, 2, 100000)[None]
    tgt = O.synth_audio(22, 2, 100000)[None]
    te = get_param_embeds(tgt, pm, SR)
    ev = PopulationEvaluator(x, SR, E.make_plugins("autodiff"), pm, te)
    W = np.random.default_rng(0).random((32, 51))
    full, _, audio = ev.evaluate(W, want_audio=True)
    full, audio = full.cpu().numpy(), audio.cpu().numpy()
    rev = ev.evaluate(W[::-1].copy())[0].cpu().numpy()[::-1]
    np.testing.assert_array_equal(full, rev)
    for i in (0, 13, 31):
        l1, _, a1 = ev.evaluate(W[i:i + 1], want_audio=True)
        assert l1.cpu().numpy()[0] == full[i], i
        np.testing.assert_array_equal(a1.cpu().numpy()[0], audio[i])


def test_apply_functions_equal_the_chain_render(dev):
    from st_ito import effects as E, engine
    x = torch.stack([_audio(40 + b, 2, 30011) for b in range(4)])
    W = torch.from_numpy(np.random.default_rng(8).random((4, 51)))
    pp = E.make_plugins("autodiff")
    ref, _ = engine.render_population(pp, x.to(dev), W.to(dev), SR)
    got = E.apply_complex_autodiff_processor(x, W, SR)
    assert torch.equal(got, ref)
    # stage by stage, the apply_* functions compose to the same chain: same kernels, same float32 hand-offs
    y = E.apply_parametric_eq(x, W[:, :18], SR)
    y = E.apply_compressor(y, W[:, 18:24], SR)
    y = E.apply_distortion(y, W[:, 24:25], SR)
    y = E.apply_reverb(y, W[:, 25:50], SR)
    y = E.apply_gain(y, W[:, 50:51], SR)
    assert torch.equal(y, ref)
    assert not torch.equal(E.apply_reverb(x, W[:, 25:50], SR, seed=1), E.apply_reverb(x, W[:, 25:50], SR))
    # the classes' .process goes through the same render
    inst = E.DaspCompressor(threshold_db=-30.0, ratio=8.0, attack_ms=5.0, knee_db=6.0, makeup_gain_db=3.0)
    raw = torch.tensor([[p.raw_value for p in inst.parameters.values()]], dtype=torch.float64)
    np.testing.assert_array_equal(inst.process(x[0].numpy(), SR), E.apply_compressor(x[:1], raw, SR)[0].cpu().numpy())


def test_apply_cache_is_per_device_and_bounded(dev):
    """A sweep over reverb seeds must not keep one filtered noise bank per seed alive."""
    from st_ito import effects as E
    x, p = torch.zeros(1, 1, 64), torch.full((1, 25), 0.5, dtype=torch.float64)
    for seed in range(E._APPLY_PLUGINS_MAX + 3):
        E.apply_reverb(x, p, SR, seed=seed)
    assert len(E._APPLY_PLUGINS) <= E._APPLY_PLUGINS_MAX
    assert all(k[-1] == str(torch.device("cuda", torch.cuda.current_device())) for k in E._APPLY_PLUGINS)
    assert next(reversed(E._APPLY_PLUGINS))[2] == E._APPLY_PLUGINS_MAX + 2   # the newest entry stays


def test_run_es_on_the_autodiff_chain_is_reproducible(dev):
    import st_ito_oracle as O
    from st_ito import effects as E
    from st_ito.style_transfer import run_es
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    assert run_optim.build_parser().parse_args(["a.wav", "b.wav", "--chain", "autodiff"]).chain == "autodiff"
    with pytest.raises(NotImplementedError):
        run_optim.main(["a.wav", "b.wav", "--algorithm", "autodiff", "--chain", "autodiff"])
    pm = make_synthetic_param_model(0)
    x = O.synth_audio(5, 2, 70000)[None]
    tgt = O.synth_audio(6, 2, 70000)[None]
    runs = [run_es(x.clone(), tgt.clone(), SR, E.make_plugins("autodiff"), pm, get_param_embeds, max_iters=3, popsize=16,
                   find_w0=False, seed=4) for _ in range(2)]
    print("autodiff chain run_es fopt", runs[0]["fopt"])
    assert runs[0]["wopt"].shape == (51,) and -1.0 <= runs[0]["fopt"] <= 1.0
    assert np.float64(runs[0]["fopt"]).tobytes() == np.float64(runs[1]["fopt"]).tobytes()
    np.testing.assert_array_equal(runs[0]["wopt"], runs[1]["wopt"])
