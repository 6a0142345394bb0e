"""The float64 reference of the waveform distances (csrc/waveform.hip; distance="esr", "snr", "sisdr", "logcosh" and kind "dc"),
their float32 restatement -- the yardstick -- and the case list of tests/test_waveform_host.py and tests/test_gpu_waveform.py.

Definitions (include/stito_hip.h).  A row is one channel of one item: x the candidate's row after the peak normalisation, the
float32 product x * r with r = float32(1) / max(peak, 1e-8) in float32, then widened; y the target's.  With taps (float32, odd
length, c = len // 2) both become p[i] = sum_k taps[k] row[i + k - c], row zero outside [0, n); without, p = row.  d = p_x - p_y,
eps = 1e-8:
    esr = sum d^2 / (sum p_y^2 + eps)            dc = (sum d / n)^2 / (sum p_y^2 / n + eps)
    snr = -10 log10(sum p_y^2 / (sum d^2 + eps) + eps)
    sisdr = -10 log10(sum t^2 / (sum res^2 + eps) + eps), x' = p_x - mean p_x, y' = p_y - mean p_y, alpha = sum x'y' / (sum y'^2 + eps),
            t = alpha y', res = x' - t
    logcosh = (1 / n) sum ln(cosh d + eps), a sample with d == 0 adding 0
and an item's value is the mean over its rows.  The reference is numpy float64 on the float32 inputs and the float32 taps widened.
The d == 0 rule is how the definitions' two statements about log-cosh hold together: the formula, and that zero padding (d = 0
there) adds nothing to the sums, which is also what makes logcosh of y against itself 0; read literally the formula would add
ln(1 + eps) = 1e-8 per such sample.  The float32 restatement needs no rule: 1 + 1e-8 is 1 in float32.  The term is evaluated as
log1p(2 sinh^2(d / 2) + eps), which is ln(cosh d + eps) without rounding cosh d - 1 away against the 1.

A case is (name, x (P, C, n), y (P, C, n), peaks (P,) or None, norm_passes); the family: y uniform noise of amplitude 0.9,
x = 0.8 y + 0.3 (y delayed by one sample) + 0.05 noise + 0.02 -- ESR 1e-2 .. 3e-1, SI-SDR far below 80 dB, a DC term that is not
degenerate -- at n in {1, 2, 5, tile - 1, tile, tile + 1, 2 tile + 3} x channels {1, 2, 3}, tile the kernel's own
(stito_waveform_tile_samples), and three more at n = 5 and n = tile + 1: an all-zero target, an all-zero candidate under
norm_passes 1 (peak 0), and a peak-folded candidate.  The all-zero candidate meets a QUIET target (sum y^2 of the order of eps):
against a target of ordinary level its snr is -10 log10(1 + O(eps)), a few 1e-8 dB, which no float32 holds to a relative bar."""
import numpy as np
import torch

SR = 48000
EPS = 1e-8
KINDS = ("esr", "dc", "snr", "sisdr", "logcosh")
YARD_KINDS = ("esr", "snr", "sisdr")
BAR_FACTOR = 4.0
YARD_CAP = 2e-5
CHANNELS = (1, 2, 3)
P = 2   # items per case


def seeded_taps(n_taps, seed):
    """An asymmetric filter: seeded normal taps under a Hann window, unit l1 norm."""
    g = np.random.default_rng(seed).standard_normal(n_taps) * np.hanning(n_taps + 2)[1:-1]
    return (g / np.abs(g).sum()).astype(np.float32)


def tap_sets():
    """{name: float32 taps or None}, in the order the tests go through them."""
    from st_ito import features as F
    return {"none": None, "unit": np.array([1.0], np.float32), "shift": np.array([0.0, 0.0, 1.0], np.float32),
            "fir31": seeded_taps(31, 5), "aw": F.mrstft_prefilter("aw", SR), "fir255": seeded_taps(255, 9)}


def tile_samples(taps) -> int:
    from st_ito import _hip
    tile = _hip.lib().stito_waveform_tile_samples(0 if taps is None else len(taps))
    assert tile >= 4
    return tile


def lengths(taps):
    tile = tile_samples(taps)
    return (1, 2, 5, tile - 1, tile, tile + 1, 2 * tile + 3)


def _pair(rng, channels, n):
    y = rng.uniform(-0.9, 0.9, (P, channels, n))
    delayed = np.concatenate([np.zeros((P, channels, 1)), y[..., :-1]], axis=-1)
    x = 0.8 * y + 0.3 * delayed + 0.05 * rng.uniform(-1.0, 1.0, y.shape) + 0.02
    return x.astype(np.float32), y.astype(np.float32)


_CASES = {}


def cases(tap_name):
    """The cases of one tap set (its tile decides the lengths), built once."""
    if tap_name not in _CASES:
        taps = tap_sets()[tap_name]
        index = list(tap_sets()).index(tap_name)
        tile = tile_samples(taps)
        out = []
        for n in lengths(taps):
            for channels in CHANNELS:
                rng = np.random.default_rng([index, n, channels])
                x, y = _pair(rng, channels, n)
                out.append((f"n{n}-c{channels}", x, y, None, 0))
        for n in (5, tile + 1):
            rng = np.random.default_rng([index, n, 77])
            x, y = _pair(rng, 2, n)
            out.append((f"zero-target-n{n}", x, np.zeros_like(y), None, 0))
            quiet = (y * np.float32(1e-4 / np.sqrt(n))).astype(np.float32)
            out.append((f"zero-candidate-n{n}", np.zeros_like(x), quiet, np.zeros(P, np.float32), 1))
            loud = (x * np.float32(1.7)).astype(np.float32)
            out.append((f"peak-folded-n{n}", loud, y, np.abs(loud).max(axis=(1, 2)).astype(np.float32), 1))
        _CASES[tap_name] = out
    return _CASES[tap_name]


def scored32(x, peaks, norm_passes):
    """The candidate rows as the loss scores them, float32: x * (1 / max(peak, 1e-8)), both operations in float32."""
    x = np.asarray(x, dtype=np.float32)
    if not norm_passes:
        return x
    r = np.float32(1.0) / np.maximum(np.asarray(peaks, dtype=np.float32), np.float32(1e-8))
    return (x * r[:, None, None]).astype(np.float32)


def prefilter64(rows, taps):
    """rows (..., n) -> float64 of the same shape: conv1d(rows, taps, padding=len(taps) // 2) on the widened values; None: rows."""
    rows = np.asarray(rows, dtype=np.float64)
    if taps is None:
        return rows
    t = np.asarray(taps, dtype=np.float32).astype(np.float64)
    c = len(t) // 2
    flat = rows.reshape(-1, rows.shape[-1])
    return np.stack([np.correlate(np.pad(r, (c, c)), t, mode="valid") for r in flat]).reshape(rows.shape)


def rows64(px, py):
    """px, py (..., n) float64 -> {kind: (...,)}: the five values of every row."""
    n = px.shape[-1]
    d = px - py
    sy2 = np.sum(py * py, axis=-1)
    sd2 = np.sum(d * d, axis=-1)
    out = {"esr": sd2 / (sy2 + EPS), "dc": (np.sum(d, axis=-1) / n) ** 2 / (sy2 / n + EPS)}
    with np.errstate(divide="ignore", over="ignore"):
        out["snr"] = -10.0 * np.log10(sy2 / (sd2 + EPS) + EPS)
        xc = px - np.mean(px, axis=-1, keepdims=True)
        yc = py - np.mean(py, axis=-1, keepdims=True)
        alpha = np.sum(xc * yc, axis=-1, keepdims=True) / (np.sum(yc * yc, axis=-1, keepdims=True) + EPS)
        t = alpha * yc
        res = xc - t
        out["sisdr"] = -10.0 * np.log10(np.sum(t * t, axis=-1) / (np.sum(res * res, axis=-1) + EPS) + EPS)
        out["logcosh"] = np.sum(np.where(d == 0.0, 0.0, np.log1p(2.0 * np.sinh(0.5 * d) ** 2 + EPS)), axis=-1) / n
    return out


def reference(x, y, taps=None, peaks=None, norm_passes=0):
    """x (P, C, n), y (P or 1, C, n) float32 -> {kind: (P,) float64}: the mean over an item's rows."""
    px = prefilter64(scored32(x, peaks, norm_passes), taps)
    py = prefilter64(np.asarray(y, dtype=np.float32), taps)
    return {k: v.mean(axis=-1) for k, v in rows64(px, np.broadcast_to(py, px.shape)).items()}


def restated32(x, y, taps=None, peaks=None, norm_passes=0):
    """The float32 restatement, torch on the CPU: float32 conv1d, every sum, mean, log and cosh in float32 -> {kind: (P,) float32}."""
    xs = torch.from_numpy(scored32(x, peaks, norm_passes))
    ys = torch.from_numpy(np.asarray(y, dtype=np.float32)).expand(xs.shape)
    if taps is not None:
        t = torch.from_numpy(np.asarray(taps, dtype=np.float32))[None, None]
        shape = xs.shape
        xs = torch.nn.functional.conv1d(xs.reshape(-1, 1, shape[-1]), t, padding=t.shape[-1] // 2).reshape(shape)
        ys = torch.nn.functional.conv1d(ys.reshape(-1, 1, shape[-1]), t, padding=t.shape[-1] // 2).reshape(shape)
    eps = torch.tensor(EPS, dtype=torch.float32)
    n = xs.shape[-1]
    d = xs - ys
    sy2, sd2 = (ys * ys).sum(-1), (d * d).sum(-1)
    out = {"esr": sd2 / (sy2 + eps), "dc": (d.sum(-1) / n) ** 2 / (sy2 / n + eps), "snr": -10.0 * torch.log10(sy2 / (sd2 + eps) + eps)}
    xc, yc = xs - xs.mean(-1, keepdim=True), ys - ys.mean(-1, keepdim=True)
    alpha = (xc * yc).sum(-1, keepdim=True) / ((yc * yc).sum(-1, keepdim=True) + eps)
    t = alpha * yc
    res = xc - t
    out["sisdr"] = -10.0 * torch.log10((t * t).sum(-1) / ((res * res).sum(-1) + eps) + eps)
    out["logcosh"] = torch.log(torch.cosh(d) + eps).sum(-1) / n
    return {k: v.mean(-1).numpy() for k, v in out.items()}


def relative(got, ref):
    """|got - ref| / |ref| elementwise, 0 where both are equal (0 against 0, 80 dB against 80 dB)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))


_REF, _YARD = {}, {}


def case_reference(tap_name, case):
    """reference() of a case, computed once and shared."""
    name, x, y, peaks, norm_passes = case
    if (tap_name, name) not in _REF:
        _REF[tap_name, name] = reference(x, y, tap_sets()[tap_name], peaks, norm_passes)
    return _REF[tap_name, name]


def yardstick_of(x, y, taps=None, peaks=None, norm_passes=0, ref=None) -> float:
    """The largest relative distance of the float32 restatement from the reference over esr, snr, sisdr and the items."""
    ref = reference(x, y, taps, peaks, norm_passes) if ref is None else ref
    got = restated32(x, y, taps, peaks, norm_passes)
    return float(max(relative(got[k], ref[k]).max() for k in YARD_KINDS))


def yardstick(tap_name, case) -> float:
    """yardstick_of a case, computed once."""
    name, x, y, peaks, norm_passes = case
    if (tap_name, name) not in _YARD:
        _YARD[tap_name, name] = yardstick_of(x, y, tap_sets()[tap_name], peaks, norm_passes, case_reference(tap_name, case))
    return _YARD[tap_name, name]


def bar(tap_name, case) -> float:
    """The GPU test's bar of a case: BAR_FACTOR times its yardstick."""
    return BAR_FACTOR * yardstick(tap_name, case)
