"""Float64 references of the hand-crafted audio features (st_ito/features.py, utils.py MFCC statistics),
written from the reference's published definitions in plain numpy.  The GPU edge tests
(tests/test_gpu_feature_edges.py) compare the HIP kernels with these; tests/test_feature_ref64.py pins
them on the CPU against tests/golden/features.npz and the oracle first.

Every function takes float32 or float64 input (a torch tensor or an ndarray, (bs, chs, n) unless stated)
and computes in float64 from there on.  Integrated loudness is the oracle's (oracle/st_ito_oracle.py),
which is independent of the product's host meter.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import st_ito_oracle as O


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _normalize_rows(e: np.ndarray) -> np.ndarray:
    """torch.nn.functional.normalize(p=2, dim=-1): x / max(||x||, 1e-12)."""
    return e / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-12)


def _frames(sig: np.ndarray, n_fft: int, hop: int, center: bool) -> np.ndarray:
    """(n,) -> (T, n_fft) frames of torch.stft: centred frames pad n_fft/2 on both sides by reflection."""
    if center:
        sig = np.pad(sig, (n_fft // 2, n_fft // 2), mode="reflect")
    return sliding_window_view(sig, n_fft)[::hop]


def _stft_mag(sig: np.ndarray, n_fft: int, hop: int, window: np.ndarray, center: bool = True) -> np.ndarray:
    """|STFT| (T, n_fft / 2 + 1) of one float64 signal."""
    return np.abs(np.fft.rfft(_frames(sig, n_fft, hop, center) * window, axis=-1))


def feature_signals(x: np.ndarray, mode: str):
    """features.py:196-206 on (bs, chs, n): mono = channel mean; stereo = L, R; mid-side = L+R, L-R (no halving)."""
    if mode == "mono":
        return [x.mean(axis=1)]
    if mode == "stereo":
        return [x[:, 0], x[:, 1]]
    if mode == "mid-side":
        return [x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]]
    raise ValueError(f"Invalid mode {mode}")


def barkspectrum(x, fb, fft_size: int = 32768, mode: str = "mid-side") -> np.ndarray:
    """compute_barkspectrum (features.py:166-232) -> (bs, n_signals * n_bands).  fb is the host's
    barkscale_fbanks(fft_size // 2 + 1, ...) matrix (n_freqs, n_bands).  Rectangular window, centred with
    reflect padding, hop fft_size / 4; mean |X| over frames; fb; log(. + 1e-8); the signals are concatenated
    on the last axis of (bs, n_bands, 1), so the flattened row is band-major; rows L2-normalised."""
    x, fbT = _f64(x), _f64(fb).T
    win = np.ones(fft_size)
    outs = []
    for sig in feature_signals(x, mode):
        m = np.stack([_stft_mag(s, fft_size, fft_size // 4, win).mean(axis=0) for s in sig])   # (bs, n_freqs)
        outs.append(np.log(m @ fbT.T + 1e-8))                                                   # (bs, n_bands)
    return _normalize_rows(np.stack(outs, axis=-1).reshape(x.shape[0], -1))


def rms_energy(x) -> np.ndarray:
    """compute_rms_energy (features.py:235-245) -> (bs, chs)."""
    x = _f64(x)
    return np.sqrt(np.maximum(np.mean(x * x, axis=-1), 1e-8))


def crest_factor(x) -> np.ndarray:
    """compute_crest_factor (features.py:248-264) -> (bs, chs) in dB.  Its "peak normalise" takes the max over
    the channel axis: every sample (pair) is divided by its own largest magnitude, clamped at 1e-8."""
    x = _f64(x)
    xn = x / np.maximum(np.abs(x).max(axis=1, keepdims=True), 1e-8)
    num = np.abs(xn).max(axis=-1)
    den = np.maximum(rms_energy(xn), 1e-8)
    return 20.0 * np.log10(np.maximum(num / den, 1e-8))


def adaptive_avg_pool1d(v: np.ndarray, out: int) -> np.ndarray:
    """torch.nn.functional.adaptive_avg_pool1d on the last axis: window i = [floor(i T / out), ceil((i + 1) T / out))."""
    T = v.shape[-1]
    return np.stack([v[..., (i * T) // out:-((-(i + 1) * T) // out)].mean(axis=-1) for i in range(out)], axis=-1)


def spectral_centroid(x, sample_rate: float) -> np.ndarray:
    """compute_spectral_centroid (features.py:302-333) with torchaudio.transforms.SpectralCentroid(sr, n_fft 2048,
    hop 1024): periodic Hann window, centred with reflect padding, magnitude; centroid per frame
    sum(f |X|) / sum(|X|) with f = linspace(0, sr // 2, 1025); nan_to_num; adaptive_avg_pool1d(10); / (sr / 2).
    -> (bs, chs * 10)."""
    x = _f64(x)
    bs, chs, n = x.shape
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(2048) / 2048.0)
    freqs = np.linspace(0.0, float(int(sample_rate) // 2), 1025)
    sc = np.empty((bs, chs, n // 1024 + 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(bs):
            for c in range(chs):
                X = _stft_mag(x[b, c], 2048, 1024, win)
                sc[b, c] = (X @ freqs) / X.sum(axis=-1)
    sc = np.nan_to_num(sc, nan=0.0, posinf=0.0, neginf=0.0)
    return adaptive_avg_pool1d(sc, 10).reshape(bs, -1) / (sample_rate / 2)


def mfcc_stats(logmel, n_items: int, dct, top_db: float = 80.0) -> np.ndarray:
    """The statistics half of get_mfcc_feature_embeds (utils.py:116-159 over torchaudio's MFCC) on a dB mel
    spectrogram logmel (n_items * channels, T, n_mels): clamp at (max over the item's channels, bands and frames)
    - top_db; DCT with dct (n_mels, n_mfcc); per coefficient mean, unbiased std and max over frames; per channel
    [mean | std | max], channels concatenated, rows L2-normalised -> (n_items, channels * 3 * n_mfcc)."""
    lm, d = _f64(logmel), _f64(dct)
    S, T, M = lm.shape
    lm = lm.reshape(n_items, S // n_items, T, M)
    floor = lm.max(axis=(1, 2, 3), keepdims=True) - top_db
    c = np.maximum(lm, floor) @ d                                                   # (items, chs, T, K)
    emb = np.concatenate([c.mean(axis=2), c.std(axis=2, ddof=1), c.max(axis=2)], axis=-1)
    return _normalize_rows(emb.reshape(n_items, -1))


def htk_mel_fbanks(n_freqs: int, n_mels: int, sample_rate: int) -> np.ndarray:
    """torchaudio.functional.melscale_fbanks(n_freqs, 0, sr // 2, n_mels, sr, norm=None, mel_scale="htk"), float64."""
    all_freqs = np.linspace(0.0, float(sample_rate // 2), n_freqs)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + float(sample_rate // 2) / 700.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = np.diff(f_pts)
    slopes = f_pts[None, :] - all_freqs[:, None]
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))


def dct_ortho(n_mfcc: int, n_mels: int) -> np.ndarray:
    """torchaudio.functional.create_dct(n_mfcc, n_mels, "ortho") -> (n_mels, n_mfcc)."""
    n = np.arange(n_mels, dtype=np.float64)
    d = np.cos(np.pi / n_mels * (n[None, :] + 0.5) * np.arange(n_mfcc, dtype=np.float64)[:, None])
    d[0] *= 1.0 / np.sqrt(2.0)
    return (d * np.sqrt(2.0 / n_mels)).T


def logmel_db(sig: np.ndarray, sample_rate: int = 48000, n_fft: int = 2048, hop: int = 1024, n_mels: int = 128) -> np.ndarray:
    """torchaudio MelSpectrogram(center=False, power 2, periodic Hann, HTK bands) -> 10 log10(clamp(., 1e-10)),
    (T, n_mels) for one signal: the log-mel that stito_logmel hands to stito_mfcc_stats, in float64."""
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    P = _stft_mag(_f64(sig), n_fft, hop, win, center=False) ** 2
    return 10.0 * np.log10(np.maximum(P @ htk_mel_fbanks(n_fft // 2 + 1, n_mels, sample_rate), 1e-10))


def mfcc_feature_embeds(x, sample_rate: int = 48000, midside: bool = False, n_mfcc: int = 25) -> np.ndarray:
    """get_mfcc_feature_embeds (utils.py:116-159) at 48 kHz: mono (channel mean) or mid / side (L+R, L-R)."""
    x = _f64(x)
    sig = np.stack([x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]], axis=1) if (x.shape[1] == 2 and midside) else x.mean(axis=1, keepdims=True)
    bs, c2, _ = sig.shape
    lm = np.stack([logmel_db(sig[b, c], sample_rate) for b in range(bs) for c in range(c2)])
    return mfcc_stats(lm, bs, dct_ortho(n_mfcc, lm.shape[-1]))


def lufs(x, sample_rate: float) -> np.ndarray:
    """compute_lufs (features.py:267-299) -> (bs,): per-sample cross-channel normalisation x / max_c |x| (clamped at
    1e-8), mono duplicated to two channels, then the oracle's BS.1770-4 integrated loudness of each item."""
    x = _f64(x)
    xn = x / np.maximum(np.abs(x).max(axis=1, keepdims=True), 1e-8)
    if xn.shape[1] == 1:
        xn = np.concatenate([xn, xn], axis=1)
    return np.array([O.integrated_loudness(xn[b].T, sample_rate) for b in range(xn.shape[0])])
