"""CPU pins of the float64 feature references in tests/feature_ref64.py, which the GPU edge tests
(tests/test_gpu_feature_edges.py) trust: against the vectors the reference's own code produced
(tests/golden/features.npz, at the bars the GPU test of those vectors uses) and against the oracle's
float32 restatements at edge shapes.  A wrong reference fails here, not on the GPU machine."""
import os

import numpy as np
import pytest
import torch

import feature_ref64 as R
import st_ito_oracle as O

SR = 48000


def _fb(fft, sr, n_bands=24):
    from st_ito.features import barkscale_fbanks
    return barkscale_fbanks(fft // 2 + 1, 20.0, 20000.0, n_bands, sr)


def test_ref64_vs_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "features.npz"))
    x = torch.stack([O.synth_audio(int(sd), 2, int(g["n"])) * float(sc) for sd, sc in zip(g["seeds"], g["scales"])])
    for fft in (32768, 4096):
        for mode in ("mono", "stereo", "mid-side"):
            got = R.barkspectrum(x, _fb(fft, SR), fft, mode)
            np.testing.assert_allclose(got, g[f"bark_{fft}_{mode.replace('-', '')}"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(R.rms_energy(x), g["rms"], rtol=2e-6)
    np.testing.assert_allclose(R.crest_factor(x), g["crest"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("fft,n,mode,chs,sr", [(128, 65, "mid-side", 2, 44100), (128, 32 * 7 + 1, "mono", 2, 48000),
                                               (1024, 256 * 9 - 1, "mono", 1, 44100), (4096, 1024 * 5, "stereo", 2, 48000),
                                               (32768, 16385, "mid-side", 2, 48000)])
def test_barkspectrum_ref64_vs_oracle(fft, n, mode, chs, sr):
    x = torch.stack([O.synth_audio(10 + i, chs, n) * s for i, s in enumerate((1e-3, 1.0, 30.0))])
    x[2, -1] = 0.0                                              # a silent channel (mid = side = L)
    ref = O.compute_barkspectrum(x, fft_size=fft, sample_rate=sr, mode=mode).numpy()
    np.testing.assert_allclose(R.barkspectrum(x, _fb(fft, sr), fft, mode), ref, rtol=0, atol=5e-6)


@pytest.mark.parametrize("n,sr,chs", [(1025, 48000, 2), (2048, 11025, 1), (5000, 22050, 2), (10239, 44100, 1), (10240, 11025, 2)])
def test_spectral_centroid_ref64_vs_oracle(n, sr, chs):
    x = torch.stack([O.synth_audio(20 + i, chs, n) for i in range(3)])
    x[1] = 0.0                                                  # all-silent item: every frame NaN, scrubbed
    x[2, :, n // 3:] = 0.0                                      # silent stretch
    ref = O.compute_spectral_centroid(x, sr).numpy()
    np.testing.assert_allclose(R.spectral_centroid(x, sr), ref, rtol=0, atol=2e-5)


def test_adaptive_avg_pool_ref64_vs_torch():
    for T in range(1, 40):
        v = np.random.default_rng(T).random((3, T))
        ref = torch.nn.functional.adaptive_avg_pool1d(torch.from_numpy(v), 10).numpy()
        np.testing.assert_allclose(R.adaptive_avg_pool1d(v, 10), ref, rtol=1e-14, atol=0)


@pytest.mark.parametrize("n,chs", [(1, 2), (2, 1), (257, 2), (4099, 2)])
def test_rms_crest_ref64_vs_oracle(n, chs):
    x = torch.stack([O.synth_audio(30 + i, chs, n) * s for i, s in enumerate((1e3, 1e-6, 1.0, 0.0))])
    x[2, -1] = 0.0                                              # a silent channel
    np.testing.assert_allclose(R.rms_energy(x), O.compute_rms_energy(x).numpy(), rtol=2e-6)
    np.testing.assert_allclose(R.crest_factor(x), O.compute_crest_factor(x).numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("n", [3072, 100000])
def test_mfcc_ref64_vs_oracle(n):
    x = torch.stack([O.synth_audio(40, 2, n), 0.05 * O.synth_audio(41, 2, n)])
    x[1, :, n // 2:] = 0.0                                      # 1e-10 clamp and 80 dB floor
    x[0, 1] = 0.0                                               # one silent channel: side = mid
    for midside in (False, True):
        ref = O.mfcc_feature_embeds(x, SR, midside=midside).numpy()
        np.testing.assert_allclose(R.mfcc_feature_embeds(x, SR, midside=midside), ref, rtol=0, atol=2e-5)


def test_lufs_ref64_vs_host_meter():
    """The wrapper (normalisation, mono duplication) around the oracle's meter against the product's host meter
    st_ito.loudness on the same normalised signal; the 400 ms minimum of the oracle's meter."""
    from st_ito.loudness import integrated_loudness
    x = torch.stack([O.synth_audio(50, 2, 54419), 0.3 * O.synth_audio(51, 2, 54419)])
    x[1, :, 20000:] *= 1e-10                                   # normalised to ~-40 dB: under the relative gate
    got = R.lufs(x, 44100)
    for b in range(2):
        xn = (x[b] / x[b].abs().max(dim=0)[0].clamp(min=1e-8)[None]).double()
        assert abs(got[b] - integrated_loudness(xn.numpy().T, 44100)) < 1e-6
    xm = x[:, :1]
    np.testing.assert_allclose(R.lufs(xm, 44100), R.lufs(torch.cat([xm, xm], 1), 44100), rtol=0, atol=1e-12)
    assert np.isfinite(R.lufs(x[:, :, :17640], 44100)).all()
    with pytest.raises(ValueError):
        R.lufs(x[:, :, :17639], 44100)
