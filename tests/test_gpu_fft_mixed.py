"""The mixed-radix bark spectrum (csrc/fft_mixed.hip: stito_barkspectrum_mixed behind compute_barkspectrum(mixed_radix=True)
and get_mir_feature_embeds(binding="reference")) against the float64 reference tests/feature_ref64.barkspectrum, which
tests/test_fft_mixed_host.py pins against torch.stft.

Batches are built like those of tests/test_gpu_feature_edges.py -- seeded noise plus a sine, amplitudes 60 dB apart -- with
three items, the third all silent; mono and stereo inputs.  The silent item is compared exactly: log(1e-8) in every band, a
constant row after normalisation, the same bits as the radix-2 kernel gives for silence.  Every case prints its measured
maximum error next to its bar (run with -s).

The bar against float64 is the project's BAR_BARK = 5e-6 absolute on the normalised row, at every length tested: the largest
error measured on an MI355X was 3.1e-7, at fft 420 (profiles/fft_mixed.txt has the figure per length), so no length needed
the wider bar that tests/test_gpu_feature_edges.BAR_ABS would have allowed.
"""
from functools import partial

import numpy as np
import pytest
import torch

import feature_ref64 as R
import st_ito_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:At least one bark filterbank")]

BAR_BARK = 5e-6
N_BANDS = 24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _batch3(seed, chs, n, sr=48000):
    """(3, chs, n) float32: noise plus a tone, item 1 60 dB below item 0, item 2 all silent."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.1 * rng.standard_normal((3, chs, n))
    x += 0.3 * np.sin(2 * np.pi * rng.uniform(50.0, 5000.0, (3, 1, 1)) * t + rng.uniform(0.0, 6.3, (3, chs, 1)))
    x *= np.array([1.0, 1e-3, 0.0])[:, None, None]
    return torch.from_numpy(x.astype(np.float32))


def _fb(fft, sr=44100):
    from st_ito.features import barkscale_fbanks
    return barkscale_fbanks(fft // 2 + 1, 20.0, 20000.0, N_BANDS, sr)


_silent_rows = {}


def _silent_row(n_cols):
    """The radix-2 kernel's row for a silent item: log(1e-8) in every band, normalised."""
    if n_cols not in _silent_rows:
        from st_ito import features as PF
        mode = "mono" if n_cols == N_BANDS else "stereo"
        _silent_rows[n_cols] = PF.compute_barkspectrum(torch.zeros(1, 2, 200), fft_size=256, mode=mode)[0]
    return _silent_rows[n_cols]


def _check(name, got, x, fft, mode, fb=None):
    """got (3, n_cols) float32 tensor of the batch x: items 0 and 1 within the bar of float64, item 2 exact."""
    ref = R.barkspectrum(x, _fb(fft) if fb is None else fb, fft, mode)
    g = got.cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    err = float(np.abs(g[:2] - ref[:2]).max())
    print(f"[fft-mixed] {name}: max err {err:.3e} (bar {BAR_BARK:.0e})")
    assert err <= BAR_BARK, (name, err, BAR_BARK)   # a NaN fails here too
    silent = got[2].cpu()
    assert bool((silent == silent[0]).all()) and torch.equal(silent, _silent_row(got.shape[1])), (name, silent)
    assert abs(float(silent[0]) + got.shape[1] ** -0.5) < 1e-7


# ---------------------------------------------------------------- 1. each radix alone and mixed
@pytest.mark.parametrize("fft", [162, 250, 686, 384, 420, 1000, 30870])
@pytest.mark.parametrize("mode", ["mono", "stereo", "mid-side"])
def test_each_radix_alone_and_mixed(dev, fft, mode):
    """3^4, 5^3, 7^3, 2^7 3, 2^2 3 5 7, 2^3 5^3, 2 3^2 5 7^3; n at the reflect minimum (T = 3, every sample of the first frame
    reflected) and at 5 hops + 3 (the last frame partly reflected)."""
    from st_ito import features as PF
    for i, n in enumerate((fft // 2 + 1, 5 * (fft // 4) + 3)):
        x = _batch3(fft + i, 2, n)
        got = PF.compute_barkspectrum(x, fft_size=fft, mode=mode, mixed_radix=True)
        _check(f"fft {fft} n {n} {mode} chs 2", got, x, fft, mode)
        if mode == "mono":
            xm = x[:, :1].contiguous()
            got = PF.compute_barkspectrum(xm, fft_size=fft, mode=mode, mixed_radix=True)
            _check(f"fft {fft} n {n} {mode} chs 1", got, xm, fft, mode)


# ---------------------------------------------------------------- 2. the audio rates
@pytest.mark.parametrize("fft", [44100, 48000, 96000])
def test_audio_rates(dev, fft):
    """n at the reflect minimum (mono and stereo inputs) and at the ES crop length 262144 (T = 11 at 96000)."""
    from st_ito import features as PF
    for chs, n in ((1, fft // 2 + 1), (2, fft // 2 + 1), (2, 262144)):
        x = _batch3(fft + chs, chs, n)
        got = PF.compute_barkspectrum(x, fft_size=fft, mode="mono", mixed_radix=True)
        _check(f"fft {fft} n {n} mono chs {chs}", got, x, fft, "mono")


# ---------------------------------------------------------------- 3. refusals
def test_refusals(dev):
    from st_ito import features as PF
    x = torch.ones((1, 2, 60000))
    for bad in (11025, 154, 98304, 96002):          # odd; 2 7 11; 7-smooth but past the range; in neither
        with pytest.raises(NotImplementedError, match=str(bad)):
            PF.compute_barkspectrum(x, fft_size=bad, mode="mono", mixed_radix=True)
    for fft in (250, 48000):
        with pytest.raises(ValueError):
            PF.compute_barkspectrum(torch.ones((1, 2, fft // 2)), fft_size=fft, mode="stereo", mixed_radix=True)
        PF.compute_barkspectrum(torch.ones((1, 2, fft // 2 + 1)), fft_size=fft, mode="stereo", mixed_radix=True)
    with pytest.raises(NotImplementedError):
        PF.compute_barkspectrum(x, fft_size=48000, mode="mono", mixed_radix=False)
    with pytest.raises(NotImplementedError):
        PF.compute_barkspectrum(x, 48000, mode="mono")
    with pytest.raises(ValueError):
        PF.compute_barkspectrum(torch.ones((1, 1, 60000)), fft_size=48000, mode="stereo", mixed_radix=True)   # needs two channels


# ---------------------------------------------------------------- 4. the unchanged path
@pytest.mark.parametrize("fft", [4096, 32768])
def test_power_of_two_is_not_rerouted(dev, fft):
    from st_ito import features as PF
    x = _batch3(fft, 2, 40001)
    for mode in ("mono", "mid-side"):
        assert torch.equal(PF.compute_barkspectrum(x, fft_size=fft, mode=mode, mixed_radix=True),
                           PF.compute_barkspectrum(x, fft_size=fft, mode=mode, mixed_radix=False))


# ---------------------------------------------------------------- 5. determinism and batch independence
def test_deterministic_and_batch_independent(dev):
    from st_ito import features as PF
    x = _batch3(5, 2, 60001)
    for mode in ("mono", "mid-side"):
        a = PF.compute_barkspectrum(x, fft_size=48000, mode=mode, mixed_radix=True)
        assert torch.equal(a, PF.compute_barkspectrum(x, fft_size=48000, mode=mode, mixed_radix=True))
        assert torch.equal(a[:1], PF.compute_barkspectrum(x[:1], fft_size=48000, mode=mode, mixed_radix=True))
        assert torch.equal(a[1:2], PF.compute_barkspectrum(x[1:2].contiguous(), fft_size=48000, mode=mode, mixed_radix=True))


# ---------------------------------------------------------------- 6. the reference's binding
def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("sr", [48000, 44100])
def test_mir_feature_embeds_reference_binding(dev, sr):
    """utils.py:83 literally: fft_size = sample_rate, the filterbank at its default 44.1 kHz whatever the rate."""
    from st_ito.utils import get_mir_feature_embeds, load_mir_feature_extractor
    model = load_mir_feature_extractor()
    x = _batch3(sr, 2, 30000, sr)
    ref_b = get_mir_feature_embeds(x, model, sr, binding="reference")
    wrap = get_mir_feature_embeds(x, model, sr, binding="wrappers")
    assert {k: tuple(v.shape) for k, v in ref_b.items()} == {"lufs": (3, 1), "rms": (3, 2), "crest": (3, 2),
                                                             "barkspectrum": (3, 24), "spectral_centroid": (3, 20)}
    _check(f"mir reference binding sr {sr}", ref_b["barkspectrum"], x, sr, "mono", fb=_fb(sr, 44100))
    for k in ("lufs", "rms", "crest", "spectral_centroid"):
        assert _same(ref_b[k], wrap[k]), k
    assert _same(wrap["barkspectrum"], get_mir_feature_embeds(x, model, sr)["barkspectrum"])      # the default has not moved
    assert not _same(ref_b["barkspectrum"][:2], wrap["barkspectrum"][:2])                           # and the two do differ
    with pytest.raises(ValueError):
        get_mir_feature_embeds(x, model, sr, binding="x")


# ---------------------------------------------------------------- 7. through the ES
def test_reference_binding_as_embed_func_of_the_evaluator(dev):
    from st_ito import effects as E
    from st_ito import features as PF
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_mir_feature_embeds, load_mir_feature_extractor
    model = load_mir_feature_extractor()
    embed = partial(get_mir_feature_embeds, binding="reference")
    n = 262144
    x = O.synth_audio(71, 2, n)[None]
    tgt = (O.synth_audio(72, 2, n) * 0.5)[None]
    te = embed(tgt, model, 48000)
    ev = PopulationEvaluator(x, 48000, E.make_plugins("eq-comp"), model, te, embed_func=embed)
    assert not ev.fused                                     # a partial is not get_param_embeds: the generic path
    W = np.random.default_rng(9).random((4, 22))
    loss, emb, audio = ev.evaluate(W, want_audio=True)
    assert loss.shape == (4,) and bool(torch.isfinite(loss).all())
    alone = PF.compute_barkspectrum(audio[:1], fft_size=48000, mixed_radix=True, mode="mono")
    assert torch.equal(emb["barkspectrum"][:1].cpu(), alone.cpu())
