"""Restatement of the reference's run_rule_based (st_ito/style_transfer.py:184-278) on the CPU, for the tests of the GPU
baseline (tests/test_rule_based_ref.py, tests/test_gpu_rule_based.py).

Float64 where the reference is float64 and float32 where it is float32: the average spectrum is torch.stft on float32 (as
the reference computes it), the smoothing, the firwin2 design and the FIR filter are scipy's own functions, the compressor is
the C restatement of juce::dsp::Compressor<float> (oracle_compressor, physical parameters, one channel at a time), the meter
the BS.1770-4 integrated loudness of the oracle.  Besides the output, every item reports a trace of its hill-climb: the step
count and delta (target - output loudness) before the first step and after every step.
"""
import numpy as np
import scipy.signal
import torch

import st_ito_oracle as O

GAIN32 = np.float32(10 ** (-12 / 20))


def peak_normalize(x: np.ndarray, clamp: bool = True) -> np.ndarray:
    """x / max|x| (clamped to 1e-8 when `clamp`; a NaN peak stays NaN) * 10^(-12/20), every operation in float32."""
    x = np.asarray(x, dtype=np.float32)
    m = np.max(np.abs(x))
    if clamp and not np.isnan(m):
        m = max(m, np.float32(1e-8))
    return (x / np.float32(m)).astype(np.float32) * GAIN32


def average_spectrum(x: np.ndarray, n_fft: int = 16384) -> np.ndarray:
    """Mean over frames of |STFT| (rectangular window, hop n_fft / 4, centred, reflect pad, 1 / sqrt(n_fft)) of the item's
    mono mix (a stereo item is averaged over its channels first) -> (n_fft // 2 + 1,) float32."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    if t.shape[0] == 2:
        t = t.mean(dim=0, keepdim=True)
    X = torch.stft(t, n_fft, return_complex=True, normalized=True)
    return X.abs().mean(dim=-1).view(-1).numpy()


def smooth(H: np.ndarray) -> np.ndarray:
    return scipy.signal.savgol_filter(H, 1025, 2)


def design_taps(sm_in: np.ndarray, sm_ref: np.ndarray, sample_rate: int, n_taps: int = 2048) -> np.ndarray:
    """The matched EQ: gain = sm_ref / sm_in (float32) with no gain at Nyquist, as a linear-phase FIR by firwin2."""
    gain = sm_ref / sm_in
    gain[-1] = 0.0
    grid = np.linspace(0, 1.0, num=len(gain)) * (sample_rate / 2)
    return scipy.signal.firwin2(n_taps, grid, gain, fs=sample_rate)


def fir(taps: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Causal FIR of every channel in float64, rounded to float32 once."""
    return scipy.signal.lfilter(taps, [1.0], np.asarray(x, dtype=np.float32)).astype(np.float32)


def eq_half(x: np.ndarray, t: np.ndarray, sample_rate: int, n_fft: int = 16384, n_taps: int = 2048) -> dict:
    """x, t: one item each, already at -12 dBFS.  -> the intermediate results of the matched EQ."""
    spec_in, spec_ref = average_spectrum(x, n_fft), average_spectrum(t, n_fft)
    sm_in, sm_ref = smooth(spec_in), smooth(spec_ref)
    taps = design_taps(sm_in, sm_ref, sample_rate, n_taps)
    return dict(spec_in=spec_in, spec_ref=spec_ref, sm_in=sm_in, sm_ref=sm_ref, taps=taps, filtered=fir(taps, x))


def compress(x: np.ndarray, sample_rate: int, threshold_db: float) -> np.ndarray:
    """Compressor(threshold, ratio 3, attack 1 ms, release 100 ms), every channel with its own envelope."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    for c in range(x.shape[0]):
        O._lib().oracle_compressor(O._fp(x[c]), O._fp(y[c]), x.shape[1], float(sample_rate), float(threshold_db), 3.0, 1.0, 100.0)
    return y


def loudness(x: np.ndarray, sample_rate: int) -> float:
    return O.integrated_loudness(np.asarray(x, dtype=np.float64).T, sample_rate)


def hill_climb(x: np.ndarray, target_lufs: float, sample_rate: int):
    """-> (output, steps, deltas): deltas[0] before the first step, deltas[k] after step k."""
    delta = target_lufs - loudness(x, sample_rate)
    deltas = [delta]
    threshold = 0.0
    out = x
    while delta > 0.25 and threshold > -80.0:
        out = compress(out, sample_rate, threshold)
        out = (out / np.max(np.abs(out))).astype(np.float32) * GAIN32
        delta = target_lufs - loudness(out, sample_rate)
        deltas.append(delta)
        threshold -= 0.5
    return out, len(deltas) - 1, deltas


def run_rule_based(input_audio: np.ndarray, target_audio: np.ndarray, sample_rate: int, n_fft: int = 16384, n_taps: int = 2048):
    """(bs, chs, n) float32 arrays (left untouched) -> dict(output (bs, chs, n) float32, inputs / targets at -12 dBFS,
    steps (bs,), deltas: a list per item, eq: the matched-EQ intermediates per item)."""
    outs, xs, ts, steps, deltas, eqs = [], [], [], [], [], []
    for b in range(input_audio.shape[0]):
        x = peak_normalize(input_audio[b])
        t = peak_normalize(target_audio[b])
        eq = eq_half(x, t, sample_rate, n_fft, n_taps)
        y = peak_normalize(eq["filtered"])
        out, k, d = hill_climb(y, loudness(t, sample_rate), sample_rate)
        outs.append(out); xs.append(x); ts.append(t); steps.append(k); deltas.append(d); eqs.append(eq)
    return dict(output=np.stack(outs), inputs=np.stack(xs), targets=np.stack(ts), steps=np.array(steps), deltas=deltas, eq=eqs)


def case_signals(seed: int, chs: int, n: int, sample_rate: int):
    """A seeded (input, target) pair of one item each, float32 (chs, n): the oracle's synthetic signal, and another one with
    its spectrum tilted by a two-tap FIR so that the matched EQ has something to match."""
    x = O.synth_audio(seed, chs, n, sr=sample_rate).numpy()
    t = O.synth_audio(seed + 1000, chs, n, sr=sample_rate).numpy().astype(np.float64)
    t = scipy.signal.lfilter([1.0, 0.85], [1.0], t, axis=-1).astype(np.float32)
    return x, t


# the fixture's cases: (seed, channels, samples, sample rate)
GOLDEN_CASES = [(11, 2, 48000, 48000), (12, 1, 24000, 48000), (13, 2, 22050, 44100)]
GOLDEN_STRIDE = 4  # filtered audio is recorded at every 4th sample (the file stays far below 1 MiB)
