"""The references behind tests/test_mrstft_aw_host.py and tests/test_gpu_mrstft_aw.py: the prefiltered multi-resolution STFT
distances (distance="mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw"; auraloss's perceptual_weighting=True, restated, unpinned) in
float64 numpy and in float32 torch, on the inputs of tests/mrstft_cases.py (the sum / difference form: tests/mrstft_sd_cases.py).

Order of steps, on estimate and reference alike: the peak normalisation of the case (mrstft_cases.scored), under the
sum / difference form the rows [L + R, L - R], the prefilter p[i] = sum_k taps[k] x[i + k - c] with x zero outside the row
(`prefilter64`: np.correlate on the zero-padded float64 row, the taps being the float32 taps widened), and then the float64
functions that exist: mrstft_mel_ref.mel_error64 with identity banks (the linear forms) or with the mel banks.  Its reflect
padding therefore reflects the FILTERED row.

The yardstick of a (form, tap set) is the float32 restatement -- float32 torch conv1d, then scripts/eval_synthetic.mrstft_error,
respectively mrstft_mel_ref.mel_error32 -- against that, relative, item by item; the host test bounds it and the GPU test's bar
is BAR_FACTOR times the maximum measured for the tap set and form in use: the kernel is a third float32 evaluation, with another
summation order.  `wrong_reflect_first64` and reversed taps are the two misreadings the GPU test tells apart from the definition."""
import numpy as np
import torch

import mrstft_cases as M
import mrstft_mel_ref as R
import mrstft_sd_cases as SDC

SR = 48000
BAR_FACTOR = 4.0
FORMS = ("lr", "sum-diff", "mel")


def aw_taps(sr=SR):
    from st_ito import features as F
    return F.mrstft_prefilter("aw", sr)


def seeded_taps(n_taps, seed):
    """An asymmetric filter: seeded normal taps under a Hann window, unit l1 norm."""
    g = np.random.default_rng(seed).standard_normal(n_taps) * np.hanning(n_taps + 2)[1:-1]
    return (g / np.abs(g).sum()).astype(np.float32)


def prefilter64(rows, taps):
    """rows (R, n) float64, taps float32 -> (R, n) float64: conv1d(rows, taps, padding=len(taps) // 2)."""
    t = np.asarray(taps, dtype=np.float32).astype(np.float64)
    c = len(t) // 2
    return np.stack([np.correlate(np.pad(r, (c, c)), t, mode="valid") for r in np.asarray(rows, dtype=np.float64)])


def prefilter32(rows, taps):
    """rows (R, n) float32 tensor -> (R, n) float32: torch's conv1d."""
    t = torch.from_numpy(np.asarray(taps, dtype=np.float32))
    return torch.nn.functional.conv1d(rows[:, None, :], t[None, None, :], padding=len(t) // 2)[:, 0]


def cases(form):
    return SDC.cases() if form == "sum-diff" else M.cases()


def _rows64(a, form):
    a = SDC.sd(a) if form == "sum-diff" else a.to(torch.float64)
    return a.reshape(-1, a.shape[-1]).numpy()


_IDENTITY = [np.eye(n // 2 + 1, dtype=np.float32) for n, _, _ in R.RESOLUTIONS]


def error64(form, x, y, taps, sr=SR) -> float:
    """One item: x, y (1, C, n) tensors (x the estimate as the loss scores it) -> the loss in float64."""
    xp = torch.from_numpy(prefilter64(_rows64(x, form), taps))[None]
    yp = torch.from_numpy(prefilter64(_rows64(y, form), taps))[None]
    return R.mel_error64(xp, yp, sr=sr, banks=None if form == "mel" else _IDENTITY)


def error32(form, x, y, taps, sr=SR) -> float:
    """The float32 restatement: (float32 sums and differences,) float32 conv1d, then the float32 distance that existed."""
    if form == "sum-diff":
        x, y = SDC.sd32(x), SDC.sd32(y)
    xp = prefilter32(x.reshape(-1, x.shape[-1]).to(torch.float32), taps)[None]
    yp = prefilter32(y.reshape(-1, y.shape[-1]).to(torch.float32), taps)[None]
    if form == "mel":
        return R.mel_error32(xp, yp, sr=sr)
    return float(M._S().mrstft_error(xp, yp))


def wrong_reflect_first64(form, x, y, taps, sr=SR) -> float:
    """NOT the definition: per resolution the RAW row is reflect padded by n_fft / 2 and the filter runs over the padded row (zero
    beyond its ends), then framing, window and the two terms as in the definition -- what a loader that reflects first and filters
    afterwards computes.  With the unit tap it is the definition."""
    t = np.asarray(taps, dtype=np.float32).astype(np.float64)
    c = len(t) // 2
    total = 0.0
    for n_fft, hop, win in R.RESOLUTIONS:
        w = np.zeros(n_fft)
        lo = (n_fft - win) // 2
        w[lo:lo + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
        mags = []
        for a in (x, y):
            padded = np.pad(_rows64(a, form), ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
            full = np.stack([np.correlate(np.pad(r, (c, c)), t, mode="valid") for r in padded])
            n_frames = 1 + (full.shape[1] - n_fft) // hop
            idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
            z = np.fft.rfft(full[:, idx] * w, axis=-1)
            mags.append(np.sqrt(np.maximum(z.real ** 2 + z.imag ** 2, 1e-8)))
        xm, ym = mags
        if form == "mel":
            F = R.bank(sr, n_fft, R.N_BINS).astype(np.float64)
            xm, ym = xm @ F.T, ym @ F.T
        sc = np.mean(np.linalg.norm(ym - xm, axis=(1, 2)) / np.linalg.norm(ym, axis=(1, 2)))
        total += sc + np.mean(np.abs(np.log(xm) - np.log(ym)))
    return float(total / len(R.RESOLUTIONS))


def items(x, y, norm_passes):
    xs = M.scored(x, norm_passes)
    return [(xs[p:p + 1], y[p:p + 1] if y.shape[0] > 1 else y) for p in range(x.shape[0])]


_REF, _YARD = {}, {}


def _key(taps):
    return np.asarray(taps, dtype=np.float32).tobytes()


def reference(form, taps, name, x, y, norm_passes):
    """error64 item by item, computed once per (form, tap set, case)."""
    k = (form, _key(taps), name)
    if k not in _REF:
        _REF[k] = np.array([error64(form, a, b, taps) for a, b in items(x, y, norm_passes)])
    return _REF[k]


def yardstick(form, taps, names=None):
    """{case: relative distance of error32 from error64, the largest over its items}, over the form's cases (or the named ones)."""
    out = {}
    for name, x, y, norm_passes in cases(form):
        if names is not None and name not in names:
            continue
        k = (form, _key(taps), name)
        if k not in _YARD:
            ref = reference(form, taps, name, x, y, norm_passes)
            got = np.array([error32(form, a, b, taps) for a, b in items(x, y, norm_passes)])
            _YARD[k] = float(np.max(np.abs(got - ref) / np.abs(ref)))
        out[name] = _YARD[k]
    return out


def bar(form, taps, names=None):
    """The GPU test's bar for a tap set and form: BAR_FACTOR times the yardstick's maximum over the cases in use."""
    return BAR_FACTOR * max(yardstick(form, taps, names).values())
