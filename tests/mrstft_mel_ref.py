"""The references behind tests/test_mrstft_mel_host.py and tests/test_gpu_mrstft_mel.py: the mel-scaled multi-resolution STFT
distance (distance="mrstft-mel"; auraloss.freq.MultiResolutionSTFTLoss(scale="mel", n_bins=, sample_rate=), restated, unpinned)
in float64 numpy and in float32 torch, on the inputs of tests/mrstft_cases.py as they are, at 48 kHz with 64 bands.

Per resolution (n_fft, hop, win): torch.stft's framing (centred, reflect padding of n_fft / 2, the periodic Hann of `win` points in
the middle of the frame, one-sided), |X| = sqrt(max(re^2 + im^2, 1e-8)), M = F |X| with F = librosa.filters.mel(sr, n_fft,
n_mels=n_bins) -- the product's float32 bank models.panns._mel_filterbank(sr, n_fft, n_bins, 0, sr / 2), pinned against
transformers in tests/test_frontend_pins.py --, then per (item, channel) row over frames x n_bins
    sc = || M_y - M_x ||_F / || M_y ||_F,   lm = mean | ln M_x - ln M_y |,
and an item's loss is the mean over resolutions of the mean over its channels of sc + lm.

`yardstick()` is the relative distance of the float32 restatement (torch.stft on the CPU, a float32 bank product) from the float64
one, item by item; the host test bounds it and the GPU test's bar is BAR_FACTOR times its maximum: the kernel is a third float32
evaluation, with another FFT factorisation and the band sums as chains of fmas."""
import numpy as np
import torch

import mrstft_cases as M

SR = 48000
N_BINS = 64
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
BAR_FACTOR = 4.0

_BANKS = {}


def bank(sr, n_fft, n_bins):
    """F (n_bins, n_fft / 2 + 1) float32, as the product builds it."""
    key = (sr, n_fft, n_bins)
    if key not in _BANKS:
        from st_ito.models.panns import _mel_filterbank
        _BANKS[key] = _mel_filterbank(float(sr), n_fft, n_bins, 0.0, float(sr) / 2)
    return _BANKS[key]


def magnitudes64(rows, n_fft, hop, win):
    """rows (R, n) float64 -> clamped magnitudes (R, frames, n_fft / 2 + 1) float64, torch.stft's framing."""
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo:lo + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    p = np.pad(rows, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    n_frames = 1 + (p.shape[1] - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    z = np.fft.rfft(p[:, idx] * w, axis=-1)
    return np.sqrt(np.maximum(z.real ** 2 + z.imag ** 2, 1e-8))


def mel_error64(x, y, sr=SR, n_bins=N_BINS, resolutions=RESOLUTIONS, banks=None) -> float:
    """One item: x, y (1, C, n) tensors (x the estimate) -> the loss in float64.  banks: F per resolution in the place of the mel
    banks (any (bands, bins) matrices)."""
    xs = x.reshape(-1, x.shape[-1]).numpy().astype(np.float64)
    ys = y.reshape(-1, y.shape[-1]).numpy().astype(np.float64)
    total = 0.0
    for i, (n_fft, hop, win) in enumerate(resolutions):
        F = (bank(sr, n_fft, n_bins) if banks is None else banks[i]).astype(np.float64)
        xm = magnitudes64(xs, n_fft, hop, win) @ F.T      # (rows, frames, bands)
        ym = magnitudes64(ys, n_fft, hop, win) @ F.T
        sc = np.mean(np.linalg.norm(ym - xm, axis=(1, 2)) / np.linalg.norm(ym, axis=(1, 2)))
        total += sc + np.mean(np.abs(np.log(xm) - np.log(ym)))
    return float(total / len(resolutions))


def mel_error32(x, y, sr=SR, n_bins=N_BINS, resolutions=RESOLUTIONS) -> float:
    """The same in float32: torch.stft on the CPU, the bank as a float32 matrix product, float32 norms and means."""
    xs, ys = x.reshape(-1, x.shape[-1]).to(torch.float32), y.reshape(-1, y.shape[-1]).to(torch.float32)
    total = 0.0
    for n_fft, hop, win in resolutions:
        F = torch.from_numpy(bank(sr, n_fft, n_bins))
        mags = []
        for s in (xs, ys):
            z = torch.stft(s, n_fft, hop, win, torch.hann_window(win), return_complex=True)     # (rows, bins, frames)
            mags.append(torch.matmul(F, torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=1e-8))))
        xm, ym = mags
        sc = (torch.linalg.norm(ym - xm, dim=(-2, -1)) / torch.linalg.norm(ym, dim=(-2, -1))).mean()
        total = total + sc + torch.mean(torch.abs(torch.log(xm) - torch.log(ym)))
    return float(total / len(resolutions))


def _items(x, y, norm_passes):
    xs = M.scored(x, norm_passes)
    return [(xs[p:p + 1], y[p:p + 1] if y.shape[0] > 1 else y) for p in range(x.shape[0])]


_REF, _YARD = {}, {}


def reference(name, x, y, norm_passes):
    """mel_error64 item by item, computed once per case of mrstft_cases.cases()."""
    if name not in _REF:
        _REF[name] = np.array([mel_error64(a, b) for a, b in _items(x, y, norm_passes)])
    return _REF[name]


def yardstick():
    """{case: relative distance of mel_error32 from mel_error64, the largest over its items}"""
    if not _YARD:
        for name, x, y, norm_passes in M.cases():
            ref = reference(name, x, y, norm_passes)
            got = np.array([mel_error32(a, b) for a, b in _items(x, y, norm_passes)])
            _YARD[name] = float(np.max(np.abs(got - ref) / np.abs(ref)))
    return _YARD


def yardstick_max():
    return max(yardstick().values())
