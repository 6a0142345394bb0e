"""Hand-crafted audio features of the reference (st_ito/features.py), computed on the MI355X
through libstito_hip (csrc/features.hip): same function names, arguments and output shapes.

Only host-side setup lives here: the bark filterbank matrix and the FFT twiddle tables (built once
per (fft_size, sample_rate) and cached on the device, like packed weights).  compute_lufs measures on
the host exactly like the reference does (pyloudnorm there, st_ito.loudness here).
"""
from __future__ import annotations

import functools
import math
import warnings

import numpy as np
import torch

from . import _hip

_MODES = {"mono": 0, "stereo": 1, "mid-side": 2}
_cache = {}


def _hz_to_bark(freqs: float, bark_scale: str = "traunmuller") -> float:
    """reference features.py:39-67."""
    if bark_scale not in ["schroeder", "traunmuller", "wang"]:
        raise ValueError('bark_scale should be one of "schroeder", "traunmuller" or "wang".')
    if bark_scale == "wang":
        return 6.0 * math.asinh(freqs / 600.0)
    elif bark_scale == "schroeder":
        return 7.0 * math.asinh(freqs / 650.0)
    barks = ((26.81 * freqs) / (1960.0 + freqs)) - 0.53
    if barks < 2:
        barks += 0.15 * (2 - barks)
    elif barks > 20.1:
        barks += 0.22 * (barks - 20.1)
    return barks


def _bark_to_hz(barks: torch.Tensor, bark_scale: str = "traunmuller") -> torch.Tensor:
    """reference features.py:70-101, including its if / elif between the two end corrections."""
    if bark_scale not in ["schroeder", "traunmuller", "wang"]:
        raise ValueError('bark_scale should be one of "traunmuller", "schroeder" or "wang".')
    if bark_scale == "wang":
        return 600.0 * torch.sinh(barks / 6.0)
    elif bark_scale == "schroeder":
        return 650.0 * torch.sinh(barks / 7.0)
    barks = barks.clone()
    if any(barks < 2):
        idx = barks < 2
        barks[idx] = (barks[idx] - 0.3) / 0.85
    elif any(barks > 20.1):
        idx = barks > 20.1
        barks[idx] = (barks[idx] + 4.422) / 1.22
    return 1960 * ((barks + 0.53) / (26.28 - barks))


def _create_triangular_filterbank_from(all_freqs: torch.Tensor, f_pts: torch.Tensor) -> torch.Tensor:
    """Triangles between consecutive points of f_pts, (n_freqs, len(f_pts) - 2) -- reference features.py:10-36."""
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    return torch.max(torch.zeros(1), torch.min((-1.0 * slopes[:, :-2]) / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))


def barkscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_barks: int, sample_rate: int,
                     bark_scale: str = "traunmuller") -> torch.Tensor:
    """Triangular bark filterbank (n_freqs, n_barks) -- reference features.py:10-36, 109-163."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_bark(f_min, bark_scale), _hz_to_bark(f_max, bark_scale), n_barks + 2)
    f_pts = _bark_to_hz(m_pts, bark_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    fb = torch.max(torch.zeros(1), torch.min((-1.0 * slopes[:, :-2]) / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))
    if (fb.max(dim=0).values == 0.0).any():
        warnings.warn("At least one bark filterbank has all zero values. "
                      f"The value for `n_barks` ({n_barks}) may be set too high. "
                      f"Or, the value for `n_freqs` ({n_freqs}) may be set too low.")
    return fb


def _twiddle(n_fft: int, device) -> torch.Tensor:
    key = ("tw", n_fft, str(device))
    if key not in _cache:
        k = np.arange(n_fft // 2, dtype=np.float64)
        tw = np.stack([np.cos(-2.0 * np.pi * k / n_fft), np.sin(-2.0 * np.pi * k / n_fft)], 1).astype(np.float32)
        _cache[key] = torch.from_numpy(tw).to(device).contiguous()
    return _cache[key]


def _gpu(x: torch.Tensor):
    _hip.require_gpu()
    if x.dim() != 3:
        raise ValueError("expected (bs, chs, seq_len)")
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return x.detach().to(dev, torch.float32).contiguous(), dev


def fft_mixed_plan(fft_size: int):
    """(na, nb, radices of na, radices of nb) of the four-step factorisation fft_size / 2 = na * nb that
    stito_barkspectrum_mixed uses (stito_fft_mixed_plan: host only, no GPU needed).  NotImplementedError for a length
    that is odd, outside [128, 96000] or has a prime factor above 7."""
    import ctypes

    na, nb, rad = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 32)()
    n = _hip.lib().stito_fft_mixed_plan(int(fft_size), ctypes.byref(na), ctypes.byref(nb), rad, 32)
    if n < 0:
        _hip.check(n)
    rad, ra, prod = list(rad[:n]), [], 1
    while prod < na.value:
        ra.append(rad[len(ra)])
        prod *= ra[-1]
    return na.value, nb.value, ra, rad[len(ra):]


def mixed_tables_host(fft_size: int) -> np.ndarray:
    """The tables of stito_barkspectrum_mixed (layout: include/stito_hip.h) as (na + nb + 2 N2, 2) float32 (re, im): the
    roots of the length-na and length-nb transforms, the four-step twiddle exp(-2 pi i n2 k1 / N2) at n2 * na + k1, and
    the unpacking twiddle exp(-2 pi i k / fft_size).  Angles are reduced in integers, cos / sin taken in float64, then
    rounded once -- like _twiddle."""
    na, nb, _, _ = fft_mixed_plan(fft_size)
    N2 = na * nb

    def roots(idx, n):
        a = -2.0 * np.pi * (np.asarray(idx, dtype=np.int64) % n).astype(np.float64) / n
        return np.stack([np.cos(a), np.sin(a)], 1)

    four = np.arange(nb, dtype=np.int64)[:, None] * np.arange(na, dtype=np.int64)[None, :]   # [n2][k1]
    return np.concatenate([roots(np.arange(na), na), roots(np.arange(nb), nb), roots(four.reshape(-1), N2),
                           roots(np.arange(N2), fft_size)]).astype(np.float32)


def _mixed_tables(fft_size: int, device) -> torch.Tensor:
    key = ("mixed", fft_size, str(device))
    if key not in _cache:
        _cache[key] = torch.from_numpy(mixed_tables_host(fft_size)).to(device).contiguous()
    return _cache[key]


def _is_lds_size(fft_size: int) -> bool:
    """A power of two in [128, 32768]: the lengths k_stft_feature transforms in LDS."""
    return not (fft_size & (fft_size - 1)) and 128 <= fft_size <= 32768


def compute_barkspectrum(x: torch.Tensor, fft_size: int = 32768, n_bands: int = 24, sample_rate: int = 44100,
                         f_min: float = 20.0, f_max: float = 20000.0, mode: str = "mid-side", mixed_radix: bool = False,
                         **kwargs):
    """Bark spectrum embedding (bs, n_signals * n_bands), L2-normalised -- reference features.py:166-232.
    fft_size must be a power of two <= 32768 here (the transform runs in LDS), unless mixed_radix=True: then every even
    length in [128, 96000] with no prime factor above 7 is accepted (44 100, 48 000, ...: the mixed-radix four-step
    kernel of csrc/fft_mixed.hip); the powers of two in [128, 32768] still go to the LDS kernel, bit for bit."""
    if mode not in _MODES:
        raise ValueError(f"Invalid mode {mode}")
    if not _is_lds_size(fft_size):
        if not mixed_radix:
            raise NotImplementedError(f"fft_size {fft_size}: only powers of two in [128, 32768] are built")
        fft_mixed_plan(fft_size)  # NotImplementedError naming the length, before anything touches the GPU
    xin, dev = _gpu(x)
    bs, chs, n = xin.shape
    key = ("fb", fft_size, n_bands, sample_rate, f_min, f_max, str(dev))
    if key not in _cache:
        _cache[key] = barkscale_fbanks(fft_size // 2 + 1, f_min, f_max, n_bands, sample_rate).T.contiguous().to(dev)
    n_sig = 1 if mode == "mono" else 2
    out = torch.empty((bs, n_sig * n_bands), dtype=torch.float32, device=dev)
    L = _hip.lib()
    if _is_lds_size(fft_size):
        _hip.check(L.stito_barkspectrum(_hip.ptr(xin), bs, chs, n, _MODES[mode], fft_size, _hip.ptr(_twiddle(fft_size, dev)),
                                        _hip.ptr(_cache[key]), n_bands, _hip.ptr(out), _hip.stream_ptr()))
    else:
        tables = _mixed_tables(fft_size, dev)
        ws = _hip.scratch(L.stito_barkspectrum_mixed_workspace_bytes(bs, n_sig, fft_size), dev)
        _hip.check(L.stito_barkspectrum_mixed(_hip.ptr(xin), bs, chs, n, _MODES[mode], fft_size, _hip.ptr(tables), tables.shape[0],
                                              _hip.ptr(_cache[key]), n_bands, _hip.ptr(out), _hip.ptr(ws), ws.numel(),
                                              _hip.stream_ptr()))
    return out.to(x.device).type_as(x)


def _rms_crest(x: torch.Tensor):
    xin, dev = _gpu(x)
    bs, chs, n = xin.shape
    rms = torch.empty((bs, chs), dtype=torch.float32, device=dev)
    crest = torch.empty((bs, chs), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().stito_rms_crest(_hip.ptr(xin), bs, chs, n, _hip.ptr(rms), _hip.ptr(crest), _hip.stream_ptr()))
    return rms.to(x.device).type_as(x), crest.to(x.device).type_as(x)


def compute_rms_energy(x: torch.Tensor, **kwargs):
    """(bs, chs) -- reference features.py:235-245."""
    return _rms_crest(x)[0]


def compute_crest_factor(x: torch.Tensor, **kwargs):
    """(bs, chs) in dB -- reference features.py:248-264 (its per-sample cross-channel normalisation included)."""
    return _rms_crest(x)[1]


def compute_lufs(x: torch.Tensor, sample_rate: float, **kwargs):
    """(bs, 1) -- reference features.py:267-299: per-sample cross-channel normalisation, mono duplicated, integrated
    loudness (pyloudnorm there; the same BS.1770-4 measurement on the GPU here: stito_lufs -- K-weighting through the
    effect chain's float64 biquad cascade, gated block energies in float64; st_ito.loudness is its host restatement)."""
    xin, dev = _gpu(x)
    bs, chs, n = xin.shape
    sr = float(sample_rate)
    T_g = 0.400
    row, lo, hi, n_blocks = _lufs_tables(n, sr, dev)
    coef = row[None, :].repeat(bs, 1).contiguous()
    L = _hip.lib()
    ws = torch.empty(L.stito_lufs_workspace_bytes(bs, n, n_blocks), dtype=torch.uint8, device=dev)
    out = torch.empty((bs, 1), dtype=torch.float32, device=dev)
    _hip.check(L.stito_lufs(_hip.ptr(xin), bs, chs, n, _hip.ptr(coef), _hip.ptr(lo), _hip.ptr(hi), n_blocks, 1.0 / (T_g * sr),
                            _hip.ptr(out), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()))
    return out.to(x.device).type_as(x)


def _lufs_tables(n: int, sr: float, dev):
    """The meter's device tables for n samples at sr (pyloudnorm's 400 ms blocks at 75 % overlap): the K-weighting row
    (32 doubles: the two biquads, then identity sections), block edges lo / hi (int32, the library's int() of float
    products) and the block count.  Raises like the meter when n is shorter than one block."""
    from .loudness import _k_weighting

    T_g, step = 0.400, 0.25
    if n < T_g * sr:
        raise ValueError("Audio must have length greater than the block size.")
    key = ("lufs", n, sr, str(dev))
    if key not in _cache:
        row = np.zeros(32)
        row[0:30:5] = 1.0  # identity sections
        for k, (b, a) in enumerate(_k_weighting(sr)):
            row[5 * k:5 * k + 5] = [b[0], b[1], b[2], a[1], a[2]]
        n_blocks = int(np.round(((n / sr - T_g) / (T_g * step))) + 1)
        lo = np.array([int(T_g * (j * step) * sr) for j in range(n_blocks)], dtype=np.int32)       # pyloudnorm's block edges
        hi = np.array([int(T_g * (j * step + 1) * sr) for j in range(n_blocks)], dtype=np.int32)
        hi = np.minimum(hi, n)
        _cache[key] = (torch.from_numpy(row).to(dev), torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), n_blocks)
    return _cache[key]


def compute_spectral_centroid(x: torch.Tensor, sample_rate: float, *args, **kwargs):
    """(bs, chs * 10) -- reference features.py:302-333 (torchaudio SpectralCentroid, n_fft 2048, hop 1024)."""
    xin, dev = _gpu(x)
    bs, chs, n = xin.shape
    key = ("hann", 2048, str(dev))
    if key not in _cache:
        _cache[key] = torch.hann_window(2048, periodic=True, dtype=torch.float64).to(torch.float32).to(dev)
    L = _hip.lib()
    ws = torch.empty(L.stito_spectral_centroid_workspace_bytes(bs, chs, n), dtype=torch.uint8, device=dev)
    out = torch.empty((bs, chs * 10), dtype=torch.float32, device=dev)
    _hip.check(L.stito_spectral_centroid(_hip.ptr(xin), bs, chs, n, float(sample_rate), _hip.ptr(_cache[key]),
                                         _hip.ptr(_twiddle(2048, dev)), _hip.ptr(out), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()))
    return out.to(x.device).type_as(x)


# --------------------------------------------------------------------------------------------
# multi-resolution STFT distance (csrc/mrstft.hip)
# --------------------------------------------------------------------------------------------
MRSTFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))  # auraloss's defaults: (n_fft, hop, win)


def _mrstft_res(resolutions):
    """(ctypes int array of the (n_fft, hop, win) triples, their number); ValueError for what the kernel cannot take."""
    import ctypes

    res = [tuple(int(v) for v in r) for r in (MRSTFT_RESOLUTIONS if resolutions is None else resolutions)]
    if not 1 <= len(res) <= 8 or any(len(r) != 3 for r in res):
        raise ValueError("resolutions must be 1 .. 8 triples (n_fft, hop, win)")
    for n_fft, hop, win in res:
        if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft {n_fft} must be a power of two in [256, 4096]")
        if hop < 1 or not 1 <= win <= n_fft:
            raise ValueError(f"hop {hop} / win {win} do not fit n_fft {n_fft}")
    flat = [v for r in res for v in r]
    return (ctypes.c_int * len(flat))(*flat), len(res)


def _mrstft_check_length(n: int, resolutions) -> None:
    """torch.stft's condition for reflect padding: more samples than half the largest n_fft."""
    res = MRSTFT_RESOLUTIONS if resolutions is None else resolutions
    half = max(int(r[0]) for r in res) // 2
    if int(n) <= half:
        raise ValueError(f"{int(n)} samples are too few for the reflect padding of n_fft {2 * half} (more than {half} are needed)")


def _mrstft_stereo(stereo, channels) -> bool:
    """True for stereo="sum-diff", False for "lr"; ValueError for anything else and for sum / difference of other than 2 channels."""
    if stereo not in ("lr", "sum-diff"):
        raise ValueError(f"stereo must be 'lr' or 'sum-diff', got {stereo!r}")
    if stereo == "sum-diff" and int(channels) != 2:
        raise ValueError(f"the sum / difference distance needs 2 channels, got {int(channels)}")
    return stereo == "sum-diff"


class _TargetTable:
    """What the target tables of the audio distances (MR-STFT, waveform) share: the shape of y (T, C, n), a device table that
    `update` refills for another y of that shape, and the scaffolding of `loss`.  A kind of table states its hooks: `_name` (of
    the table in messages, of its scratch in a Workspace), `_table_floats()`, `_workspace_bytes(pop)`, `_fill(y)` -- the call
    that writes the table -- and `_loss_calls(...)` -> (the plain loss call, the one with a slot list), functools.partials that
    already carry every argument in front of audio_dev."""

    def __init__(self, y: torch.Tensor):
        self.n_targets, self.channels, self.n = (int(v) for v in y.shape)
        floats = self._table_floats()
        if floats <= 0:
            raise ValueError(f"no {self._name} table for {tuple(y.shape)} audio")
        self.table = torch.empty(floats, dtype=torch.float32, device=y.device)
        self.update(y)

    def update(self, y: torch.Tensor):
        """One launch sequence on the current stream: the table of y (same shape as at construction, float32, on the table's GPU)."""
        if tuple(y.shape) != (self.n_targets, self.channels, self.n) or not y.is_cuda or y.dtype != torch.float32:
            raise ValueError(f"target audio must be a float32 GPU tensor of shape {(self.n_targets, self.channels, self.n)}")
        self._fill(y.contiguous())
        return self

    def _taps_ptr(self):
        """The table's prefilter taps (self.taps, host float32, or None) on its device -> their pointer, or None: uploaded at the
        first call, unless the constructor was handed a tensor that already holds them (self._taps_dev)."""
        if self.taps is None:
            return None
        if self._taps_dev is None:
            self._taps_dev = torch.from_numpy(self.taps).to(self.table.device)
        assert self._taps_dev.is_cuda and self._taps_dev.dtype == torch.float32 and self._taps_dev.numel() == self.taps.size
        return _hip.ptr(self._taps_dev)

    def _loss(self, audio: torch.Tensor, peaks, norm_passes: int, slots, ws, *head) -> torch.Tensor:
        """`loss` of every kind of table; head: what the kind's `_loss_calls` takes."""
        if audio.dim() != 3 or tuple(audio.shape[1:]) != (self.channels, self.n):
            raise ValueError(f"audio must be (P, {self.channels}, {self.n}), got {tuple(audio.shape)}")
        assert audio.is_cuda and audio.dtype == torch.float32
        audio = audio.contiguous()
        P = audio.shape[0]
        ws = _hip.scratch(self._workspace_bytes(P), audio.device, ws, self._name.lower())
        out = torch.empty(P, dtype=torch.float32, device=audio.device)
        plain, with_slots = self._loss_calls(*head)
        front = (_hip.ptr(audio), _hip.ptr(peaks), int(norm_passes), _hip.ptr(self.table), self.n_targets)
        back = (P, self.channels, self.n, _hip.ptr(out), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
        if slots is None:
            _hip.check(plain(*front, *back))
            return out
        if not (slots.is_cuda and slots.dtype == torch.int32 and slots.dim() == 1 and slots.is_contiguous()):
            raise ValueError("slots must be a contiguous 1-D int32 tensor on the GPU")
        _hip.check(with_slots(*front, _hip.ptr(slots), slots.numel(), *back))
        return out


def _check_pair(x: torch.Tensor, y: torch.Tensor) -> None:
    """The shapes every compute_*_distance takes: estimate x (B, C, n), reference y (B, C, n) or (1, C, n)."""
    if x.dim() != 3 or y.dim() != 3:
        raise ValueError("expected (bs, chs, seq_len)")
    if y.shape[0] not in (1, x.shape[0]) or tuple(y.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} do not match (y may have batch 1)")


class MrstftTarget(_TargetTable):
    """The target side of the distance on the device: the table stito_mrstft_target writes for y (T, C, n) -- FFT tables,
    clamped magnitudes per (row, resolution), sum |Y|^2 -- in a buffer that `update` refills for another y of the same shape.
    stereo="sum-diff": the rows of a target are its L + R and L - R (stito_mrstft_target_sd) and `loss` forms the same two rows of
    every candidate in its loader -- auraloss's SumAndDifferenceSTFTLoss with both weights 1; 2-channel audio only."""

    _name = "MRSTFT"

    def __init__(self, y: torch.Tensor, resolutions=None, stereo: str = "lr"):
        self.res, self.n_res = _mrstft_res(resolutions)
        if y.dim() != 3:
            raise ValueError("expected (n_targets, chs, seq_len)")
        self.sum_diff = _mrstft_stereo(stereo, y.shape[1])
        _mrstft_check_length(y.shape[-1], resolutions)
        self.resolutions = resolutions
        super().__init__(y)

    # _TargetTable's hooks; MelMrstftTarget and PrefilteredMrstftTarget override them
    def _table_floats(self) -> int:
        return _hip.lib().stito_mrstft_table_floats(self.res, self.n_res, self.n_targets * self.channels, self.n)

    def _workspace_bytes(self, pop: int) -> int:
        return _hip.lib().stito_mrstft_workspace_bytes(self.res, self.n_res, pop, self.channels, self.n)

    def _fill(self, y: torch.Tensor) -> None:
        L = _hip.lib()
        if self.sum_diff:
            _hip.check(L.stito_mrstft_target_sd(self.res, self.n_res, _hip.ptr(y), self.n_targets, self.channels, self.n,
                                                _hip.ptr(self.table), _hip.stream_ptr()))
        else:
            _hip.check(L.stito_mrstft_target(self.res, self.n_res, _hip.ptr(y), self.n_targets * self.channels, self.n,
                                             _hip.ptr(self.table), _hip.stream_ptr()))

    def _loss_calls(self):
        L = _hip.lib()
        calls = (L.stito_mrstft_loss_sd, L.stito_mrstft_loss_slots_sd) if self.sum_diff else (L.stito_mrstft_loss, L.stito_mrstft_loss_slots)
        return tuple(functools.partial(c, self.res, self.n_res) for c in calls)

    def loss(self, audio: torch.Tensor, peaks=None, norm_passes: int = 0, slots=None, ws=None) -> torch.Tensor:
        """audio (P, C, n) float32 on the GPU, P a multiple of the number of targets (candidate p against target p // (P // T))
        -> (P,) float32.  norm_passes 1: audio[p] / clip(peaks[p], 1e-8) is what gets scored, folded into the kernel's loader.
        slots: (K,) int32 on the GPU, P a multiple of K -- the K stacked populations are scored against the targets slots[k] of
        the table (stito_mrstft_loss_slots: any subset, any order; a slot that names no target gives NaN).  A sum / difference
        table goes through the _sd entry points, same arguments.  ws: the evaluator's engine.Workspace the kernels' scratch comes
        from (None: allocated for this call on the current stream)."""
        return self._loss(audio, peaks, norm_passes, slots, ws)


def compute_mrstft_distance(x: torch.Tensor, y: torch.Tensor, resolutions=None) -> torch.Tensor:
    """auraloss.freq.MultiResolutionSTFTLoss()(x[b], y[b]) per item -> (B,) float32 on x's device (the library's batch value is
    the mean of these); x (B, C, n) the estimate, y (B, C, n) or (1, C, n) the reference.  resolutions: triples (n_fft, hop,
    win), default auraloss's (1024, 120, 600), (2048, 240, 1200), (512, 50, 240).  One fused kernel per resolution
    (stito_mrstft_loss): the spectra never reach HBM."""
    return _mrstft_distance(x, y, resolutions, "lr")


def compute_sd_mrstft_distance(x: torch.Tensor, y: torch.Tensor, resolutions=None) -> torch.Tensor:
    """auraloss.freq.SumAndDifferenceSTFTLoss()(x[b], y[b]) per item with both weights 1 (restated, unpinned): the distance of
    compute_mrstft_distance applied to [L + R, L - R] (no factor 1/2) of the estimate and of the reference.  Same shape rules;
    x and y must have 2 channels.  The sums and differences are formed in the kernel's loader (stito_mrstft_loss_sd)."""
    return _mrstft_distance(x, y, resolutions, "sum-diff")


def _mrstft_distance(x, y, resolutions, stereo):
    _check_pair(x, y)
    _mrstft_stereo(stereo, x.shape[1])
    _mrstft_res(resolutions)
    _mrstft_check_length(x.shape[-1], resolutions)
    xin, dev = _gpu(x)
    yin = y.detach().to(dev, torch.float32).contiguous()
    return MrstftTarget(yin, resolutions, stereo).loss(xin).to(x.device)


# --------------------------------------------------------------------------------------------
# its mel-scaled form (csrc/mrstft.hip's MEL variant)
# --------------------------------------------------------------------------------------------
MEL_MRSTFT_BINS = 64


def mel_mrstft_bank(sample_rate, n_bins: int = MEL_MRSTFT_BINS, resolutions=None):
    """The banks of auraloss's scale="mel" for a set of resolutions, built and checked on the host (no GPU needed): per
    resolution librosa.filters.mel(sr=sample_rate, n_fft=n_fft, n_mels=n_bins) -- Slaney scale and norm, fmin 0, fmax sr / 2:
    models.panns._mel_filterbank -- as (start (n_bins,) int32, length (n_bins,) int32, weights (longest run, n_bins) float32):
    band m is the run of bins [start[m], start[m] + length[m]) from its first to its last non-zero weight, weight j of the run
    at weights[j, m] (the interleaved layout of _hip.mel_tables).  ValueError for n_bins outside [1, 256] and for a band with no
    non-zero weight (ln 0 on both sides: NaN in auraloss), naming the band, the resolution and the sample rate."""
    from .models.panns import _mel_filterbank

    _mrstft_res(resolutions)
    n_bins = int(n_bins)
    if not 1 <= n_bins <= 256:
        raise ValueError(f"n_bins {n_bins} must be in [1, 256]")
    if not float(sample_rate) > 0:
        raise ValueError(f"sample_rate {sample_rate} must be positive")
    banks = []
    for n_fft, hop, win in (MRSTFT_RESOLUTIONS if resolutions is None else resolutions):
        n_fft = int(n_fft)
        F = _mel_filterbank(float(sample_rate), n_fft, n_bins, 0.0, float(sample_rate) / 2)   # (n_bins, n_fft / 2 + 1) float32
        start, length = np.zeros(n_bins, np.int32), np.zeros(n_bins, np.int32)
        for m in range(n_bins):
            nz = np.nonzero(F[m])[0]
            if len(nz) == 0:
                empty = [k for k in range(n_bins) if not F[k].any()]
                raise ValueError(f"mel band {m} of {n_bins} has no non-zero weight at resolution ({n_fft}, {int(hop)}, {int(win)}) and "
                                 f"sample rate {sample_rate} ({len(empty)} empty bands: {empty}): its ln 0 would be NaN; use fewer bands")
            start[m], length[m] = nz[0], nz[-1] + 1 - nz[0]
        weights = np.zeros((int(length.max()), n_bins), np.float32)
        for m in range(n_bins):
            weights[: length[m], m] = F[m, start[m]: start[m] + length[m]]
        banks.append((start, length, weights))
    return banks


class _DeviceMelBank:
    """A host bank (the triples of mel_mrstft_bank, or a test's) as the stito_mel_bank the calls take, with its device tables."""

    def __init__(self, banks, device):
        import ctypes

        n_bins = len(banks[0][0])
        self.start = np.ascontiguousarray(np.stack([np.asarray(b[0], np.int32) for b in banks]))
        self.length = np.ascontiguousarray(np.stack([np.asarray(b[1], np.int32) for b in banks]))
        weights = [np.ascontiguousarray(b[2], dtype=np.float32) for b in banks]
        assert self.start.shape == self.length.shape == (len(banks), n_bins) and all(w.ndim == 2 for w in weights)
        self.start_dev = torch.from_numpy(self.start).to(device)
        self.length_dev = torch.from_numpy(self.length).to(device)
        self.weights_dev = torch.from_numpy(np.concatenate([w.reshape(-1) for w in weights])).to(device)
        c = self.c = _hip.MelBank()
        c.n_bins, c.n_res = n_bins, len(banks)
        c.band_start = self.start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        c.band_len = self.length.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        c.band_start_dev, c.band_len_dev = self.start_dev.data_ptr(), self.length_dev.data_ptr()
        c.weights_dev = self.weights_dev.data_ptr()
        off = 0
        for i, w in enumerate(weights):
            c.w_offset[i], c.w_stride[i], c.w_rows[i] = off, w.shape[1], w.shape[0]
            off += w.size
        self.ref = ctypes.byref(c)


class MelMrstftTarget(MrstftTarget):
    """MrstftTarget for the mel-scaled distance (auraloss.freq.MultiResolutionSTFTLoss(scale="mel", n_bins=, sample_rate=),
    restated, unpinned): the table holds frames x n_bins band sums M = F |Y| per (row, resolution) and `loss` takes both terms
    between band sums, the candidates' formed in the kernel from magnitudes that stay in LDS.  Channels are compared L/R.  The
    bank is mel_mrstft_bank's (refused there, before anything is launched, when a band is empty), or `bank`: a list of
    (start, length, weights) per resolution in that layout."""

    def __init__(self, y: torch.Tensor, sample_rate=None, n_bins: int = MEL_MRSTFT_BINS, resolutions=None, bank=None):
        if bank is None:
            if sample_rate is None:
                raise ValueError("MelMrstftTarget needs a sample_rate (or a bank)")
            bank = mel_mrstft_bank(sample_rate, n_bins, resolutions)
        self._host_bank = bank
        self.n_bins = len(bank[0][0])
        self._bank = None
        super().__init__(y, resolutions, "lr")

    def _device_bank(self):
        if self._bank is None:
            self._bank = _DeviceMelBank(self._host_bank, self.table.device)
        return self._bank

    def _table_floats(self) -> int:
        return _hip.lib().stito_mrstft_table_floats_mel(self.res, self.n_res, self.n_bins, self.n_targets * self.channels, self.n)

    def _fill(self, y: torch.Tensor) -> None:
        _hip.check(_hip.lib().stito_mrstft_target_mel(self.res, self.n_res, self._device_bank().ref, _hip.ptr(y),
                                                      self.n_targets * self.channels, self.n, _hip.ptr(self.table), _hip.stream_ptr()))

    def _loss_calls(self):
        L, bank = _hip.lib(), self._device_bank().ref
        return tuple(functools.partial(c, self.res, self.n_res, bank) for c in (L.stito_mrstft_loss_mel, L.stito_mrstft_loss_slots_mel))


def compute_mel_mrstft_distance(x: torch.Tensor, y: torch.Tensor, sample_rate, n_bins: int = MEL_MRSTFT_BINS,
                                resolutions=None) -> torch.Tensor:
    """auraloss.freq.MultiResolutionSTFTLoss(scale="mel", n_bins=n_bins, sample_rate=sample_rate)(x[b], y[b]) per item (restated,
    unpinned) -> (B,) float32 on x's device, with compute_mrstft_distance's shape rules: the magnitudes of every frame are summed
    into n_bins Slaney mel bands before the spectral convergence and the log-magnitude term are taken, so the near-silent bins
    above a few kHz no longer carry the loss.  ValueError, before anything touches the GPU, for a bank with an empty band."""
    _check_pair(x, y)
    bank = mel_mrstft_bank(sample_rate, n_bins, resolutions)
    _mrstft_check_length(x.shape[-1], resolutions)
    xin, dev = _gpu(x)
    yin = y.detach().to(dev, torch.float32).contiguous()
    return MelMrstftTarget(yin, resolutions=resolutions, bank=bank).loss(xin).to(x.device)


# --------------------------------------------------------------------------------------------
# the prefiltered forms (csrc/mrstft.hip's PRE variants): an FIR in the kernel's loader
# --------------------------------------------------------------------------------------------
MRSTFT_PREFILTER_MAX_TAPS = 255
_PREFILTER_KINDS = {"lr": 0, "sum-diff": 1, "mel": 2}


def _a_weighting_fir(sample_rate, n_taps: int = 101) -> np.ndarray:
    """The "aw" design, float64: the analogue A-weighting prototype (corner frequencies 20.598997, 107.65265, 737.86223 and
    12194.217 Hz, +1.9997 dB at 1 kHz) through the bilinear transform, its magnitude response on 512 frequencies, and a
    frequency-sampling FIR of n_taps taps fitted to that magnitude."""
    from scipy import signal

    f1, f2, f3, f4 = 20.598997, 107.65265, 737.86223, 12194.217
    num = [(2 * np.pi * f4) ** 2 * 10 ** (1.9997 / 20), 0.0, 0.0, 0.0, 0.0]
    den = np.polymul([1.0, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1.0, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    den = np.polymul(np.polymul(den, [1.0, 2 * np.pi * f3]), [1.0, 2 * np.pi * f2])
    b, a = signal.bilinear(num, den, fs=float(sample_rate))
    w, h = signal.freqz(b, a, worN=512, fs=float(sample_rate), include_nyquist=True)
    return signal.firwin2(n_taps, w, np.abs(h), fs=float(sample_rate))


def mrstft_prefilter(spec, sample_rate=None) -> np.ndarray:
    """The taps of a prefilter of the MR-STFT distances, float32, built and checked on the host (no GPU needed).  spec: "aw" --
    the 101-tap A-weighting FIR of auraloss's perceptual_weighting=True at `sample_rate` (restated, unpinned: auraloss is not
    installed here), designed in float64 and rounded once -- or a 1-D array of taps, used as they are.  The filter is applied as
    torch.nn.functional.conv1d(x, taps, padding=len(taps) // 2): cross-correlation, zero padding, same length.

    The "aw" recipe evaluates the response with scipy.signal.freqz(..., include_nyquist=True): this project's choice, because
    scipy.signal.firwin2 wants the frequency grid to end at sample_rate / 2 and raises without it.  101 taps cannot reach
    A-weighting's -19 dB at 100 Hz (-8.5 dB at 48 kHz): a property of that filter, not a defect of this one.

    ValueError for an even or empty length, more than 255 taps, non-finite values, an unknown name, or "aw" without a rate."""
    if isinstance(spec, str):
        if spec != "aw":
            raise ValueError(f"unknown prefilter {spec!r}: 'aw' or a 1-D array of taps")
        if sample_rate is None or not float(sample_rate) > 0:
            raise ValueError(f"prefilter 'aw' is designed for a sample rate: sample_rate is {sample_rate!r}")
        taps = _a_weighting_fir(sample_rate)
    else:
        taps = np.asarray(spec.detach().cpu() if isinstance(spec, torch.Tensor) else spec, dtype=np.float64)
        if taps.ndim != 1:
            raise ValueError(f"prefilter taps must be 1-D, got shape {taps.shape}")
    if taps.size < 1 or taps.size % 2 == 0:
        raise ValueError(f"a prefilter has an odd number of taps (it is centred on tap len // 2), got {taps.size}")
    if taps.size > MRSTFT_PREFILTER_MAX_TAPS:
        raise ValueError(f"a prefilter has at most {MRSTFT_PREFILTER_MAX_TAPS} taps, got {taps.size}")
    if not np.all(np.isfinite(taps)):
        raise ValueError("prefilter taps must be finite")
    return np.ascontiguousarray(taps.astype(np.float32))


class PrefilteredMrstftTarget(MrstftTarget):
    """MrstftTarget for a distance on prefiltered rows (auraloss's perceptual_weighting=True with prefilter="aw"; restated,
    unpinned): target and candidates go through the FIR `prefilter` (mrstft_prefilter's argument; "aw" needs sample_rate) after
    the peak normalisation and, under kind "sum-diff", after [L + R, L - R] are formed, and before the STFT, whose reflect padding
    reflects the filtered row.  The filter runs in the fused kernel's loader (stito_mrstft_loss_pf): no filtered copy of the
    population is written.  kind: "lr" (compute_mrstft_distance's), "sum-diff" (compute_sd_mrstft_distance's; 2 channels) or "mel"
    (compute_mel_mrstft_distance's: sample_rate and n_bins, or `bank`, as MelMrstftTarget takes them).  The taps are uploaded once
    and live as long as the object; taps_dev: a device tensor that already holds exactly these taps (an evaluator's)."""

    def __init__(self, y: torch.Tensor, prefilter, sample_rate=None, kind: str = "lr", n_bins: int = MEL_MRSTFT_BINS, resolutions=None,
                 bank=None, taps_dev=None):
        if kind not in _PREFILTER_KINDS:
            raise ValueError(f"kind must be one of {sorted(_PREFILTER_KINDS)}, got {kind!r}")
        self.kind = kind
        self.taps = mrstft_prefilter(prefilter, sample_rate)
        self._host_bank = self._bank = None
        self.n_bins = 0
        if kind == "mel":
            if bank is None:
                if sample_rate is None:
                    raise ValueError("kind 'mel' needs a sample_rate (or a bank)")
                bank = mel_mrstft_bank(sample_rate, n_bins, resolutions)
            self._host_bank, self.n_bins = bank, len(bank[0][0])
        elif bank is not None:
            raise ValueError(f"kind {kind!r} takes no bank")
        self._taps_dev = taps_dev
        super().__init__(y, resolutions, "sum-diff" if kind == "sum-diff" else "lr")

    def _head(self):
        """(kind, bank or None, taps_dev, n_taps): what every prefiltered call takes first."""
        bank = None
        if self.kind == "mel":
            if self._bank is None:
                self._bank = _DeviceMelBank(self._host_bank, self.table.device)
            bank = self._bank.ref
        return _PREFILTER_KINDS[self.kind], bank, self._taps_ptr(), int(self.taps.size)

    def _table_floats(self) -> int:
        return _hip.lib().stito_mrstft_table_floats_pf(_PREFILTER_KINDS[self.kind], self.n_bins, int(self.taps.size), self.res, self.n_res,
                                                       self.n_targets * self.channels, self.n)

    def _workspace_bytes(self, pop: int) -> int:
        return _hip.lib().stito_mrstft_workspace_bytes_pf(_PREFILTER_KINDS[self.kind], int(self.taps.size), self.res, self.n_res, pop,
                                                          self.channels, self.n)

    def _fill(self, y: torch.Tensor) -> None:
        _hip.check(_hip.lib().stito_mrstft_target_pf(*self._head(), self.res, self.n_res, _hip.ptr(y), self.n_targets, self.channels,
                                                     self.n, _hip.ptr(self.table), _hip.stream_ptr()))

    def _loss_calls(self):
        L, head = _hip.lib(), self._head()
        return tuple(functools.partial(c, *head, self.res, self.n_res) for c in (L.stito_mrstft_loss_pf, L.stito_mrstft_loss_slots_pf))


def compute_prefiltered_mrstft_distance(x: torch.Tensor, y: torch.Tensor, prefilter, sample_rate=None, kind: str = "lr",
                                        n_bins: int = MEL_MRSTFT_BINS, resolutions=None) -> torch.Tensor:
    """compute_mrstft_distance (kind "lr"), compute_sd_mrstft_distance ("sum-diff") or compute_mel_mrstft_distance ("mel") of
    estimate and reference after both went through the FIR `prefilter` -- with "aw", auraloss's perceptual_weighting=True
    (restated, unpinned) -> (B,) float32 on x's device.  Same shape rules as those; sample_rate is needed for "aw" and for "mel".
    Every ValueError -- the taps, the kind, an empty mel band, the shapes -- comes before anything touches the GPU."""
    if kind not in _PREFILTER_KINDS:
        raise ValueError(f"kind must be one of {sorted(_PREFILTER_KINDS)}, got {kind!r}")
    taps = mrstft_prefilter(prefilter, sample_rate)
    _check_pair(x, y)
    _mrstft_stereo("sum-diff" if kind == "sum-diff" else "lr", x.shape[1])
    bank = None
    if kind == "mel":
        if sample_rate is None:
            raise ValueError("kind 'mel' needs a sample_rate")
        bank = mel_mrstft_bank(sample_rate, n_bins, resolutions)
    _mrstft_res(resolutions)
    _mrstft_check_length(x.shape[-1], resolutions)
    xin, dev = _gpu(x)
    yin = y.detach().to(dev, torch.float32).contiguous()
    return PrefilteredMrstftTarget(yin, taps, kind=kind, resolutions=resolutions, bank=bank).loss(xin).to(x.device)


# --------------------------------------------------------------------------------------------
# waveform distances (csrc/waveform.hip): ESR, DC, SNR, SI-SDR, log-cosh in one pass over the rows
# --------------------------------------------------------------------------------------------
WAVEFORM_KINDS = {"esr": 0, "dc": 1, "snr": 2, "sisdr": 3, "logcosh": 4}
WAVEFORM_MAX_CHANNELS = 8


def _waveform_kind(kind) -> int:
    if kind not in WAVEFORM_KINDS:
        raise ValueError(f"kind must be one of {sorted(WAVEFORM_KINDS)}, got {kind!r}")
    return WAVEFORM_KINDS[kind]


def _waveform_taps(prefilter, sample_rate):
    """None for no prefilter, else mrstft_prefilter's float32 taps (same refusals)."""
    return None if prefilter is None else mrstft_prefilter(prefilter, sample_rate)


def _waveform_check_shape(channels: int, n: int) -> None:
    if not 1 <= int(channels) <= WAVEFORM_MAX_CHANNELS:
        raise ValueError(f"Invalid number of channels: {int(channels)}")
    if int(n) < 1:
        raise ValueError(f"{int(n)} samples: the waveform distances need at least 1")


class WaveformTarget(_TargetTable):
    """The target side of the waveform distances on the device, the shape of MrstftTarget: the table stito_waveform_target writes for
    y (T, C, n) -- the rows after the prefilter (a copy of y without one) and their float64 sums -- in a buffer that `update` refills
    for another y of the same shape.  prefilter: None, or mrstft_prefilter's argument ("aw" needs sample_rate): target and
    candidates go through that FIR after the peak normalisation, in the kernel (no filtered copy of the population is written).
    One table serves every kind: `loss(..., kind=)` picks esr, dc, snr, sisdr or logcosh (auraloss.time's ESRLoss, DCLoss, SNRLoss,
    SISDRLoss, LogCoshLoss, restated, parity unpinned; the formulas stand in include/stito_hip.h).  taps_dev: a device tensor that
    already holds exactly these taps (an evaluator's)."""

    _name = "waveform"

    def __init__(self, y: torch.Tensor, prefilter=None, sample_rate=None, taps_dev=None):
        self.taps = _waveform_taps(prefilter, sample_rate)
        self.n_taps = 0 if self.taps is None else int(self.taps.size)
        if y.dim() != 3:
            raise ValueError("expected (n_targets, chs, seq_len)")
        _waveform_check_shape(y.shape[1], y.shape[2])
        self._taps_dev = taps_dev
        super().__init__(y)

    def _table_floats(self) -> int:
        return _hip.lib().stito_waveform_table_floats(self.n_taps, self.n_targets * self.channels, self.n)

    def _workspace_bytes(self, pop: int) -> int:
        return _hip.lib().stito_waveform_workspace_bytes(self.n_taps, pop, self.channels, self.n)

    def _fill(self, y: torch.Tensor) -> None:
        _hip.check(_hip.lib().stito_waveform_target(self._taps_ptr(), self.n_taps, _hip.ptr(y), self.n_targets * self.channels, self.n,
                                                    _hip.ptr(self.table), _hip.stream_ptr()))

    def _loss_calls(self, kind: int):
        L, taps = _hip.lib(), self._taps_ptr()
        return tuple(functools.partial(c, kind, taps, self.n_taps) for c in (L.stito_waveform_loss, L.stito_waveform_loss_slots))

    def loss(self, audio: torch.Tensor, peaks=None, norm_passes: int = 0, slots=None, ws=None, kind: str = "esr") -> torch.Tensor:
        """audio (P, C, n) float32 on the GPU -> (P,) float32, candidate p against target p // (P // T); peaks / norm_passes / slots /
        ws: as MrstftTarget.loss (the folded peak normalisation, the slot list of stito_waveform_loss_slots, the evaluator's
        engine.Workspace).  kind: "esr", "dc", "snr", "sisdr" or "logcosh"."""
        return self._loss(audio, peaks, norm_passes, slots, ws, _waveform_kind(kind))


def compute_waveform_distance(x: torch.Tensor, y: torch.Tensor, kind: str = "esr", prefilter=None, sample_rate=None) -> torch.Tensor:
    """The waveform distance `kind` ("esr", "dc", "snr", "sisdr", "logcosh": auraloss.time's losses, restated, unpinned) of
    estimate x (B, C, n) and reference y (B, C, n) or (1, C, n), per item -> (B,) float32 on x's device: the mean over the item's
    channels.  prefilter: None, or mrstft_prefilter's argument -- both sides go through that FIR first (ESR behind a pre-emphasis
    filter); "aw" needs sample_rate.  Every ValueError -- the kind, the taps, the shapes -- comes before anything touches the GPU."""
    _waveform_kind(kind)
    taps = _waveform_taps(prefilter, sample_rate)
    _check_pair(x, y)
    _waveform_check_shape(x.shape[1], x.shape[2])
    xin, dev = _gpu(x)
    yin = y.detach().to(dev, torch.float32).contiguous()
    return WaveformTarget(yin, taps).loss(xin, kind=kind).to(x.device)
