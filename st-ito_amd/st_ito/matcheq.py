"""Host side of the rule-based style-transfer baseline (reference st_ito/style_transfer.py:163-278, run_rule_based): the
tables the kernels of csrc/matcheq.hip need -- built once per shape and device, like the filterbanks and K-weighting
coefficients of st_ito.features -- and thin calls into the C ABI on the current stream.

Every function takes and returns device tensors; there is no CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.signal
import torch

from . import _hip
from .features import _lufs_tables, _twiddle

_cache = {}
PEAK_GAIN = float(np.float32(10 ** (-12 / 20)))  # -12 dBFS: the reference scales float32 audio by this float32 factor
MAX_CLIMB_STEPS = 160  # threshold 0 dB down to -80 dB in 0.5 dB steps (style_transfer.py:256, 268)


def _check_audio(x: torch.Tensor):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3):
        raise ValueError("expected a contiguous (bs, chs, seq_len) float32 tensor on the GPU")


def mean_spectrum(x: torch.Tensor, n_fft: int) -> torch.Tensor:
    """get_average_spectrum (style_transfer.py:168-181) of every item: (bs, chs, n) -> (bs, n_fft // 2 + 1) float32."""
    _check_audio(x)
    bs, chs, n = x.shape
    out = torch.empty((bs, n_fft // 2 + 1), dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().stito_mean_spectrum(_hip.ptr(x), bs, chs, n, n_fft, _hip.ptr(_twiddle(n_fft, x.device)), _hip.ptr(out),
                                              _hip.stream_ptr()))
    return out


def savgol_tables(window: int, polyorder: int, dev):
    """(coefficients in correlation order (window,), edge operator (window, window)) float64 on `dev`: scipy's savgol_coeffs
    reversed, and row r = the weights that np.polyfit(arange(window), x, polyorder) evaluated at r puts on x (what
    savgol_filter's mode "interp" does at the first and last window // 2 points)."""
    key = ("sg", window, polyorder, str(dev))
    if key not in _cache:
        c = scipy.signal.savgol_coeffs(window, polyorder)[::-1].copy()
        t = np.arange(window, dtype=np.float64)
        fit = np.polyfit(t, np.eye(window), polyorder)  # (polyorder + 1, window): the fit of every unit vector
        E = np.zeros((window, window))
        for row in fit:  # np.polyval's Horner scheme, one column per unit vector
            E = E * t[:, None] + row[None, :]
        _cache[key] = (torch.from_numpy(c).to(dev), torch.from_numpy(np.ascontiguousarray(E)).to(dev))
    return _cache[key]


def savgol(rows: torch.Tensor, window: int = 1025, polyorder: int = 2) -> torch.Tensor:
    """smooth_spectrum (style_transfer.py:163-165) of every row of (R, n) float32 -> (R, n) float32."""
    if not (rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2):
        raise ValueError("expected a contiguous (rows, n) float32 tensor on the GPU")
    c, E = savgol_tables(window, polyorder, rows.device)
    out = torch.empty_like(rows)
    _hip.check(_hip.lib().stito_savgol(_hip.ptr(rows), rows.shape[0], rows.shape[1], _hip.ptr(c), window, _hip.ptr(E), _hip.ptr(out),
                                       _hip.stream_ptr()))
    return out


def firwin2_tables(n_freq: int, sample_rate: float, n_taps: int, dev):
    """The float64 grids and window of scipy.signal.firwin2(n_taps, np.linspace(0, 1, n_freq) * (sr / 2), gain, fs=sr):
    (freq, grid, window, phase_b, inv_nyq).  Both grids come from numpy: they agree at every 4th point only up to rounding."""
    key = ("fw", n_freq, float(sample_rate), n_taps, str(dev))
    if key not in _cache:
        freq = np.linspace(0, 1.0, num=n_freq) * (sample_rate / 2)
        nyq = 0.5 * sample_rate
        n_grid = 1 + 2 ** int(math.ceil(math.log(n_taps, 2)))
        grid = np.linspace(0.0, nyq, n_grid)
        window = scipy.signal.get_window("hamming", n_taps, fftbins=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        _cache[key] = (t(freq), t(grid), t(window), -(n_taps - 1) / 2. * np.pi, 1.0 / nyq)
    return _cache[key]


def firwin2(num: torch.Tensor, den, sample_rate: float, n_taps: int) -> torch.Tensor:
    """Taps (bs, n_taps) float64 of the matched EQ (style_transfer.py:231-240): gain = num / den in float32 with the last
    bin 0, or num itself when den is None (then its last bin must already be 0 for an even n_taps, as scipy demands)."""
    bs, n_freq = num.shape
    freq, grid, window, phase_b, inv_nyq = firwin2_tables(n_freq, sample_rate, n_taps, num.device)
    taps = torch.empty((bs, n_taps), dtype=torch.float64, device=num.device)
    _hip.check(_hip.lib().stito_firwin2(_hip.ptr(num), _hip.ptr(den), bs, n_freq, _hip.ptr(freq), _hip.ptr(grid), grid.numel(), n_taps,
                                        phase_b, inv_nyq, _hip.ptr(window), _hip.ptr(taps), _hip.stream_ptr()))
    return taps


def fir(x: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """scipy.signal.lfilter(taps[b], [1.0], x[b]) per item and channel, float64 sums, float32 result."""
    _check_audio(x)
    bs, chs, n = x.shape
    y = torch.empty_like(x)
    taps = taps.contiguous()
    _hip.check(_hip.lib().stito_fir(_hip.ptr(x), bs, chs, n, _hip.ptr(taps), taps.shape[1], _hip.ptr(y), _hip.stream_ptr()))
    return y


def peak_normalize_(x: torch.Tensor, clamp_min: float = 1e-8, gain: float = PEAK_GAIN) -> torch.Tensor:
    """In place, per item: x = x / max|x| (clamped to clamp_min when > 0) * gain, float32 (style_transfer.py:220-223)."""
    _check_audio(x)
    bs, chs, n = x.shape
    peaks = torch.empty(bs, dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().stito_peak_normalize(_hip.ptr(x), bs, chs, n, clamp_min, gain, _hip.ptr(peaks), _hip.stream_ptr()))
    return x


def _meter_args(n: int, sample_rate: float, bs: int, dev):
    row, lo, hi, n_blocks = _lufs_tables(n, float(sample_rate), dev)
    return row[None, :].repeat(bs, 1).contiguous(), lo, hi, n_blocks, 1.0 / (0.400 * float(sample_rate))


def lufs_raw(x: torch.Tensor, sample_rate: float) -> torch.Tensor:
    """pyloudnorm.Meter(sr).integrated_loudness of every item on its raw channels -> (bs,) float64 (style_transfer.py:250-252)."""
    _check_audio(x)
    bs, chs, n = x.shape
    coef, lo, hi, n_blocks, inv_len = _meter_args(n, sample_rate, bs, x.device)
    L = _hip.lib()
    ws = torch.empty(L.stito_lufs_raw_workspace_bytes(bs, chs, n, n_blocks), dtype=torch.uint8, device=x.device)
    out = torch.empty(bs, dtype=torch.float64, device=x.device)
    _hip.check(L.stito_lufs_raw(_hip.ptr(x), bs, chs, n, _hip.ptr(coef), _hip.ptr(lo), _hip.ptr(hi), n_blocks, inv_len, _hip.ptr(out),
                                _hip.ptr(ws), ws.numel(), _hip.stream_ptr()))
    return out


def hill_climb_(x: torch.Tensor, input_lufs: torch.Tensor, target_lufs: torch.Tensor, sample_rate: float,
                max_steps: int = MAX_CLIMB_STEPS):
    """The compressor hill-climb of style_transfer.py:254-268 for every item at once, in place on x (bs, chs, n): an item's
    audio ends as its last pass's output.  The host loop stops as soon as no item is active (one flag read per step).
    -> (steps (bs,) int32, delta (bs,) float64, threshold (bs,) float64) on the device."""
    _check_audio(x)
    bs, chs, n = x.shape
    dev = x.device
    coef, lo, hi, n_blocks, inv_len = _meter_args(n, sample_rate, bs, dev)
    thr = torch.empty(bs, dtype=torch.float64, device=dev)
    delta = torch.empty(bs, dtype=torch.float64, device=dev)
    active = torch.empty(bs, dtype=torch.int32, device=dev)
    steps = torch.empty(bs, dtype=torch.int32, device=dev)
    L = _hip.lib()
    sp = _hip.stream_ptr()
    _hip.check(L.stito_climb_init(_hip.ptr(input_lufs), _hip.ptr(target_lufs), bs, _hip.ptr(thr), _hip.ptr(delta), _hip.ptr(active),
                                  _hip.ptr(steps), sp))
    ws = torch.empty(L.stito_climb_workspace_bytes(bs, chs, n, n_blocks), dtype=torch.uint8, device=dev)
    for _ in range(max_steps):
        if not bool(active.any()):
            break
        _hip.check(L.stito_climb_step(_hip.ptr(x), bs, chs, n, float(sample_rate), _hip.ptr(coef), _hip.ptr(lo), _hip.ptr(hi), n_blocks,
                                      inv_len, _hip.ptr(target_lufs), _hip.ptr(thr), _hip.ptr(delta), _hip.ptr(active), _hip.ptr(steps),
                                      _hip.ptr(ws), ws.numel(), sp))
    return steps, delta, thr
