"""The audio-feature kernels of csrc/features.hip (MIR and MFCC metrics) against the float64 references of
tests/feature_ref64.py at their edge shapes: every FFT size of the bark spectrum, lengths at each kernel's
minimum and at frame / block boundaries, fewer than 10 centroid frames (overlapping pooling windows), more
than 64 items (the second block of k_l2norm_rows and k_lufs_gate), 30 s inputs, and MFCC statistics far
beyond the frame count that once had to fit the LDS.

Calls go through the product's entry points (st_ito.features, MFCCExtractor / get_mfcc_feature_embeds) or,
for stito_mfcc_stats in isolation, the C ABI.  Batches hold items at scales from 1e-4 to 1e3, one all-zero
item, one with a silent stretch and, when stereo, one with a silent channel.  Every case prints its measured
maximum error next to its bar (run with -s); the bars are the suite's existing ones for these functions.
"""
import numpy as np
import pytest
import torch

import feature_ref64 as R
import st_ito_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:At least one bark filterbank")]

BAR_BARK, BAR_RMS_REL, BAR_ABS, BAR_LUFS = 5e-6, 2e-6, 2e-5, 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _check(name, got, ref, bar, rel=False):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    with np.errstate(invalid="ignore"):
        d = np.where(got == ref, 0.0, np.abs(got - ref))   # equal infinities (silent LUFS) count as exact
    if rel:
        d = d / np.abs(ref)
    err = float(d.max())
    print(f"[feature-edges] {name}: max {'rel ' if rel else ''}err {err:.3e} (bar {bar:.0e})")
    assert err <= bar, (name, err, bar)   # a NaN fails here too


def _batch(seed, count, chs, n, sr=48000):
    """(count, chs, n) float32: noise plus a tone per item, scales spread over 1e-4 .. 1e3; item 0 all zero,
    item 1 silent over its middle third, item 2 (stereo) with a silent right channel."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.1 * rng.standard_normal((count, chs, n))
    x += 0.3 * np.sin(2 * np.pi * rng.uniform(50.0, 5000.0, (count, 1, 1)) * t + rng.uniform(0.0, 6.3, (count, chs, 1)))
    x *= rng.permutation(np.logspace(-4, 3, count))[:, None, None]
    x[0] = 0.0
    if count > 1:
        x[1, :, n // 3:2 * n // 3] = 0.0
    if count > 2 and chs == 2:
        x[2, 1] = 0.0
    return torch.from_numpy(x.astype(np.float32))


def _fb(fft, sr):
    from st_ito.features import barkscale_fbanks
    return barkscale_fbanks(fft // 2 + 1, 20.0, 20000.0, 24, sr)


def _bark_modes(x):
    """(mode, input): mono of a stereo input, mono of a mono input, stereo, mid-side."""
    return [("mono", x), ("mono", x[:, :1].contiguous()), ("stereo", x), ("mid-side", x)]


# ---------------------------------------------------------------- bark spectrum (k_stft_feature MODE 0)
@pytest.mark.parametrize("fft", [128 << i for i in range(9)])
def test_barkspectrum_every_fft_size(dev, fft):
    """Both k_stft_feature instantiations (256 threads below 4096, 1024 from 4096; 16 bins per thread + Nyquist at 32768)
    at the reflect minimum n = fft/2 + 1 and at k * hop - 1, k * hop, k * hop + 1; 44.1 and 48 kHz filterbanks."""
    from st_ito import features as PF
    hop = fft // 4
    for i, n in enumerate((fft // 2 + 1, 7 * hop - 1, 7 * hop, 7 * hop + 1)):
        sr = (44100, 48000)[i % 2]
        x = _batch(100 + i, 6, 2, n, sr)
        for mode, xx in _bark_modes(x):
            got = PF.compute_barkspectrum(xx, fft_size=fft, sample_rate=sr, mode=mode).numpy()
            ref = R.barkspectrum(xx, _fb(fft, sr), fft, mode)
            _check(f"bark fft {fft} n {n} sr {sr} {mode} chs {xx.shape[1]}", got, ref, BAR_BARK)


@pytest.mark.parametrize("fft", [2048, 4096])
def test_barkspectrum_batch70(dev, fft):
    """70 items: the second 64-row block of k_l2norm_rows."""
    from st_ito import features as PF
    x = _batch(7, 70, 2, 30001)
    for mode in ("mono", "mid-side"):
        got = PF.compute_barkspectrum(x, fft_size=fft, sample_rate=48000, mode=mode).numpy()
        _check(f"bark fft {fft} 70 items {mode}", got, R.barkspectrum(x, _fb(fft, 48000), fft, mode), BAR_BARK)


@pytest.mark.parametrize("fft", [128, 32768])
def test_barkspectrum_30s(dev, fft):
    """1 440 000 samples (30 s at 48 kHz): 45 001 frames summed in float32 per bin at fft 128, 176 at 32768.  Four items
    (zero, silent stretch, silent channel, plain) rather than 70, to keep the float64 STFT of the reference short."""
    from st_ito import features as PF
    x = _batch(8, 4, 2, 1440000)
    for mode in ("mono", "mid-side"):
        got = PF.compute_barkspectrum(x, fft_size=fft, sample_rate=48000, mode=mode).numpy()
        _check(f"bark fft {fft} 30 s {mode}", got, R.barkspectrum(x, _fb(fft, 48000), fft, mode), BAR_BARK)


# ---------------------------------------------------------------- spectral centroid (k_stft_feature MODE 1 + k_centroid_pool)
@pytest.mark.parametrize("sr", [48000, 44100, 22050, 11025])
def test_spectral_centroid_edges(dev, sr):
    """T = n // 1024 + 1 from 2 to 11 frames (below 10 the adaptive pooling windows overlap), the reflect minimum
    n = 1025, and 480 001 samples at 48 kHz; at 11 025 Hz sr // 2 differs from sr / 2.  Silent stretches give NaN
    frames that are scrubbed before the pooling; the all-zero item is NaN everywhere."""
    from st_ito import features as PF
    ns = (1025, 2047, 2048, 5000, 10239, 10240) + ((480001,) if sr == 48000 else ())
    for n in ns:
        for chs in (1, 2):
            x = _batch(200 + n % 97, 5, chs, n, sr)
            got = PF.compute_spectral_centroid(x, sr).numpy()
            _check(f"centroid n {n} sr {sr} chs {chs}", got, R.spectral_centroid(x, sr), BAR_ABS)


def test_spectral_centroid_batch70(dev):
    """70 stereo items: 140 rows through k_centroid_pool and its second workgroup."""
    from st_ito import features as PF
    x = _batch(9, 70, 2, 10240, 44100)
    _check("centroid 70 items", PF.compute_spectral_centroid(x, 44100).numpy(), R.spectral_centroid(x, 44100), BAR_ABS)


# ---------------------------------------------------------------- RMS and crest factor (k_rms_crest)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1440000])
def test_rms_crest_edges(dev, n):
    """Lengths below, at and above the 256-thread stride, and 30 s.  One item at amplitude 1e-6 (mean square under the
    1e-8 clamp) and one at 1e3 besides the batch's spread; the silent item and silent channel hit the crest factor's
    1e-8 clamps (-160 dB).  70 items, 4 at 1 440 000 samples."""
    from st_ito import features as PF
    count = 70 if n < 1440000 else 4
    for chs in (1, 2):
        x = _batch(300 + n % 101, count, chs, n)
        x[3] = torch.from_numpy(np.random.default_rng(n).standard_normal((chs, n)).astype(np.float32)) * (1e-6 if count > 4 else 1e3)
        if count > 4:
            x[4] = torch.from_numpy(np.random.default_rng(n + 1).standard_normal((chs, n)).astype(np.float32)) * 1e3
        _check(f"rms n {n} chs {chs}", PF.compute_rms_energy(x).numpy(), R.rms_energy(x), BAR_RMS_REL, rel=True)
        _check(f"crest n {n} chs {chs}", PF.compute_crest_factor(x).numpy(), R.crest_factor(x), BAR_ABS)


# ---------------------------------------------------------------- integrated loudness (k_lufs_*)
def _one_block_item(n, sr, rng):
    """Quiet everywhere (|x| < 1e-8: normalised to about -40 dB) but for a burst in [0, 0.1 s), which only gating
    block 0 contains: exactly one block passes the relative gate."""
    x = 1e-10 * rng.standard_normal((2, n))
    x[:, :int(0.1 * sr)] = 0.5 * rng.standard_normal((2, int(0.1 * sr)))
    return torch.from_numpy(x.astype(np.float32))


def test_lufs_edges(dev):
    """Exactly 0.4 s (one block; one sample less raises), lengths at 44.1 kHz whose block count and block edges are
    rounded, 30 s stereo, and 70 items (the second block of k_lufs_gate) with a silent item and an item of which only
    one block passes the relative gate."""
    from st_ito import features as PF
    rng = np.random.default_rng(11)
    for sr in (48000, 44100):
        n = int(0.4 * sr)
        for chs in (1, 2):
            x = _batch(400 + chs, 3, chs, n, sr)
            _check(f"lufs 0.4 s sr {sr} chs {chs}", PF.compute_lufs(x, sr).numpy()[:, 0], R.lufs(x, sr), BAR_LUFS)
            with pytest.raises(ValueError):
                PF.compute_lufs(x[:, :, :n - 1].contiguous(), sr)
    for n in (19845, 24255, 54419, 100003):     # (n / sr - 0.4) / 0.1 = 0.5, 1.5, 8.34, 18.68 blocks past the first
        x = _batch(410 + n % 7, 4, 2, n, 44100)
        _check(f"lufs n {n} sr 44100", PF.compute_lufs(x, 44100).numpy()[:, 0], R.lufs(x, 44100), BAR_LUFS)
    x = _batch(420, 3, 2, 1440000)[1:]
    _check("lufs 30 s stereo", PF.compute_lufs(x, 48000).numpy()[:, 0], R.lufs(x, 48000), BAR_LUFS)
    x = _batch(430, 70, 2, 96000)
    x[5] = _one_block_item(96000, 48000, rng)
    ref = R.lufs(x, 48000)
    assert ref[0] == float("-inf") and abs(ref[5] - R.lufs(x[5:6, :, :19200], 48000)[0]) < 1e-9   # the cases are what they claim
    _check("lufs 70 items", PF.compute_lufs(x, 48000).numpy()[:, 0], ref, BAR_LUFS)


# ---------------------------------------------------------------- MFCC statistics (k_mfcc_stats)
def _mfcc_stats_abi(dev, lm, n_items, dct, top_db=80.0):
    from st_ito import _hip
    S, T, M = lm.shape
    K = dct.shape[1]
    lm_d, dct_d = lm.to(dev).contiguous(), dct.to(dev).contiguous()
    out = torch.empty((n_items, (S // n_items) * 3 * K), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().stito_mfcc_stats(_hip.ptr(lm_d), n_items, S // n_items, T, M, _hip.ptr(dct_d), K, top_db, _hip.ptr(out),
                                           _hip.stream_ptr()))
    return out.cpu().numpy()


def _synthetic_logmel(rng, n_items, chs, T, M):
    """dB values mostly between -200 and -40 with a per-frame level; each item's maximum (0 dB) sits in channel 0
    only, so the 80 dB floor (-80 dB) clamps most bins of every channel."""
    lm = rng.uniform(-200.0, -40.0, (n_items, chs, T, M)) + rng.uniform(-20.0, 20.0, (n_items, chs, T, 1))
    lm = np.minimum(lm, -1.0)
    lm[:, 0, rng.integers(T), rng.integers(M)] = 0.0
    return torch.from_numpy(lm.reshape(n_items * chs, T, M).astype(np.float32))


@pytest.mark.parametrize("T", [2, 3, 1310, 1311, 1405, 5000])
def test_mfcc_stats_abi(dev, T):
    """stito_mfcc_stats alone: frame counts on both sides of 1310 (the most that fit the LDS at n_mfcc 25 before the
    kernel streamed its frames) up to 5000; n_mfcc 1, 25, 32; n_mels 40 and 128; one and two channels."""
    rng = np.random.default_rng(T)
    for M in (40, 128):
        for K in (1, 25, 32):
            dct = torch.from_numpy(R.dct_ortho(K, M).astype(np.float32))
            for chs in (1, 2):
                lm = _synthetic_logmel(rng, 3, chs, T, M)
                _check(f"mfcc stats T {T} n_mels {M} n_mfcc {K} chs {chs}", _mfcc_stats_abi(dev, lm, 3, dct), R.mfcc_stats(lm, 3, dct), BAR_ABS)


def test_mfcc_stats_abi_batch70_and_limits(dev):
    """70 items (the second block of k_l2norm_rows); n_mfcc 33 is unsupported, a single frame is invalid."""
    rng = np.random.default_rng(70)
    dct = torch.from_numpy(R.dct_ortho(25, 128).astype(np.float32))
    lm = _synthetic_logmel(rng, 70, 2, 300, 128)
    _check("mfcc stats 70 items", _mfcc_stats_abi(dev, lm, 70, dct), R.mfcc_stats(lm, 70, dct), BAR_ABS)
    with pytest.raises(NotImplementedError):
        _mfcc_stats_abi(dev, lm[:2], 1, torch.from_numpy(R.dct_ortho(33, 128).astype(np.float32)))
    with pytest.raises(ValueError):
        _mfcc_stats_abi(dev, lm[:2, :1], 1, dct)


@pytest.fixture(scope="module")
def mfcc_model(dev):
    from st_ito.utils import load_mfcc_feature_extractor
    return load_mfcc_feature_extractor()


@pytest.mark.parametrize("midside", [False, True])
def test_mfcc_embeds_30s_and_minimum(dev, mfcc_model, midside):
    """get_mfcc_feature_embeds on 30 s stereo at 48 kHz (1405 frames: run_es embeds its whole target, and 30 s once
    raised "frames do not fit the LDS") and at its minimum length of 3072 samples (two frames), against the oracle's
    mfcc_feature_embeds; 3071 samples raise."""
    from st_ito.utils import get_mfcc_feature_embeds
    for n in (1440000, 3072):
        x = _batch(500 + n % 13, 3, 2, n)
        got = get_mfcc_feature_embeds(x, mfcc_model, 48000, midside=midside)["mono"].numpy()
        _check(f"mfcc embeds n {n} midside {midside}", got, O.mfcc_feature_embeds(x, 48000, midside=midside).numpy(), BAR_ABS)
    with pytest.raises(ValueError):
        get_mfcc_feature_embeds(torch.ones((1, 2, 3071)), mfcc_model, 48000, midside=midside)


def test_below_minimum_lengths_raise(dev):
    """Each entry point below its documented minimum: bark n <= fft/2 (reflect padding), centroid n <= 1024, RMS / crest
    n = 0 (LUFS below 0.4 s and MFCC below two frames: in their tests above)."""
    from st_ito import features as PF
    for fft in (128, 32768):
        with pytest.raises(ValueError):
            PF.compute_barkspectrum(torch.ones((1, 2, fft // 2)), fft_size=fft, sample_rate=48000, mode="stereo")
        PF.compute_barkspectrum(torch.ones((1, 2, fft // 2 + 1)), fft_size=fft, sample_rate=48000, mode="stereo")
    with pytest.raises(ValueError):
        PF.compute_spectral_centroid(torch.ones((1, 1, 1024)), 48000)
    with pytest.raises(ValueError):
        PF.compute_rms_energy(torch.ones((1, 2, 0)))
