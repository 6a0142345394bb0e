"""Float64 torch-CPU restatement of the five dasp-pytorch functions behind the reference's apply_* family (st_ito/effects.py:
532-706: gain, distortion, compressor, parametric_eq, noise_shaped_reverberation), restated from the library's published
algorithm -- dasp-pytorch is an un-vendored, un-pinned dependency: PARITY UNPINNED.  The filters are applied by FFT exactly as
the library applies them (sosfilt_via_fsm / lfilter_via_fsm: H sampled on n_fft = 2^ceil(log2(2 n - 1)) points, circular over
n_fft), which makes this reference independent of the GPU kernels' formulation (a time-domain recursion started from the
periodic state).  precision="float32" runs the same code in the library's own dtype.

All parameters are the raw [0, 1] values of the reference's call surface, (bs, num_params); audio is (bs, chs, n).

Two places where float64 does not replace the library's float32:
  * the audio and the noise bank are float32 data;
  * the compressor's alpha_A.  The library holds it as a float32 tensor, so the filter it runs IS the one with a float32
    coefficient.  precision="float64" evaluates exp(-log 9 / (fs attack / 1000)) in float64 and rounds it to float32 once (what the
    kernel does, so that both land on the same float32: an ulp of a coefficient next to 1 is 3e-4 of a 250 ms time constant);
    precision="float32" evaluates it with float32 tensor operations like the library.

eq_periodic_start / onepole_periodic_start are numpy prototypes of the kernels' formulation, pinned against the FFT form in
tests/test_dasp_ref64.py."""
import math

import numpy as np
import torch

LOOKAHEAD = 512
EQ_RANGES = [(-18.0, 18.0), (20.0, 20000.0), (0.1, 10.0)] * 6
COMP_RANGES = [(-60.0, 0.0), (1.0, 20.0), (0.1, 250.0), (10.0, 2000.0), (1.0, 24.0), (0.0, 24.0)]
EQ_KINDS = ["low_shelf", "peaking", "peaking", "peaking", "peaking", "high_shelf"]


def _dtype(precision):
    return {"float64": torch.float64, "float32": torch.float32}[precision]


def denormalize(p, lo, hi):
    return p * (hi - lo) + lo


def fft_len(n: int) -> int:
    """2^ceil(log2(2 n - 1)) in integers."""
    return 1 << (2 * n - 2).bit_length()


def biquad(gain_db, freq, q, sample_rate, kind):
    """dasp_pytorch.signal.biquad (RBJ cookbook), tensors (bs,) -> b, a (bs, 3) normalised by a0."""
    A = 10 ** (gain_db / 40.0)
    w0 = 2 * math.pi * (freq / sample_rate)
    alpha = torch.sin(w0) / (2 * q)
    cw = torch.cos(w0)
    sA = torch.sqrt(A)
    if kind == "high_shelf":
        b0 = A * ((A + 1) + (A - 1) * cw + 2 * sA * alpha)
        b1 = -2 * A * ((A - 1) + (A + 1) * cw)
        b2 = A * ((A + 1) + (A - 1) * cw - 2 * sA * alpha)
        a0 = (A + 1) - (A - 1) * cw + 2 * sA * alpha
        a1 = 2 * ((A - 1) - (A + 1) * cw)
        a2 = (A + 1) - (A - 1) * cw - 2 * sA * alpha
    elif kind == "low_shelf":
        b0 = A * ((A + 1) - (A - 1) * cw + 2 * sA * alpha)
        b1 = 2 * A * ((A - 1) - (A + 1) * cw)
        b2 = A * ((A + 1) - (A - 1) * cw - 2 * sA * alpha)
        a0 = (A + 1) + (A - 1) * cw + 2 * sA * alpha
        a1 = -2 * ((A - 1) + (A + 1) * cw)
        a2 = (A + 1) + (A - 1) * cw - 2 * sA * alpha
    else:
        b0 = 1 + alpha * A
        b1 = -2 * cw
        b2 = 1 - alpha * A
        a0 = 1 + alpha / A
        a1 = -2 * cw
        a2 = 1 - alpha / A
    b = torch.stack([b0, b1, b2], dim=-1) / a0[:, None]
    a = torch.stack([a0, a1, a2], dim=-1) / a0[:, None]
    return b, a


def eq_sos(params, sample_rate, precision="float64"):
    """(bs, 18) raw parameters -> (bs, 6, 6) sections [b0 b1 b2 1 a1 a2] in apply_parametric_eq's order and ranges."""
    p = params.to(_dtype(precision))
    sos = []
    for s in range(6):
        v = [denormalize(p[:, 3 * s + k], *EQ_RANGES[3 * s + k]) for k in range(3)]
        b, a = biquad(v[0], v[1], v[2], sample_rate, EQ_KINDS[s])
        sos.append(torch.cat([b, a], dim=-1))
    return torch.stack(sos, dim=1)


def sosfilt_via_fsm(sos, x):
    """dasp_pytorch.signal.sosfilt_via_fsm: sos (bs, sections, 6), x (bs, chs, n)."""
    n = x.shape[-1]
    n_fft = fft_len(n)
    H = torch.ones(sos.shape[0], n_fft // 2 + 1, dtype=torch.complex128 if sos.dtype == torch.float64 else torch.complex64)
    for s in range(sos.shape[1]):
        H = H * (torch.fft.rfft(sos[:, s, :3], n_fft) / torch.fft.rfft(sos[:, s, 3:], n_fft))
    return torch.fft.irfft(torch.fft.rfft(x, n_fft) * H[:, None], n_fft)[..., :n]


def parametric_eq(x, params, sample_rate, precision="float64"):
    return sosfilt_via_fsm(eq_sos(params, sample_rate, precision), x.to(_dtype(precision)))


def compressor_alpha(attack_ms, sample_rate, precision="float64"):
    """alpha_A as a float32 value held in the working dtype (see the module docstring)."""
    if precision == "float32":
        att = attack_ms.to(torch.float32)
        return torch.exp(-torch.log(torch.tensor([9.0], dtype=torch.float32)) / (sample_rate * (att / 1e3)))
    att = attack_ms.to(torch.float64)
    return torch.exp(-math.log(9.0) / (sample_rate * (att / 1e3))).to(torch.float32).to(torch.float64)


def compressor(x, params, sample_rate, precision="float64", eps=1e-8, lookahead_samples=LOOKAHEAD):
    """dasp_pytorch.compressor as apply_compressor calls it: side chain = channel sum, soft-knee gain computer, one one-pole with
    the attack constant applied by lfilter_via_fsm (release_ms is computed from and never used), make-up, look-ahead = the signal
    rolled by 512 samples with its first 512 zeroed, the gain not delayed."""
    dt = _dtype(precision)
    bs, chs, n = x.shape
    p = params.to(dt)
    thr, ratio, att, _rel, knee, makeup = (denormalize(p[:, k], *COMP_RANGES[k]).view(bs, 1, 1) for k in range(6))
    x = x.to(dt)
    alpha = compressor_alpha(att, sample_rate, precision)
    x_db = 20 * torch.log10(torch.abs(x.sum(dim=1, keepdim=True)).clamp(eps))
    x_sc = x_db.clone()
    idx = torch.logical_and(x_db >= (thr - knee / 2), x_db <= (thr + knee / 2))
    below = x_db + ((1 / ratio) - 1) * ((x_db - thr + (knee / 2)) ** 2) / (2 * knee)
    x_sc[idx] = below[idx]
    idx = x_db > (thr + knee / 2)
    above = thr + ((x_db - thr) / ratio)
    x_sc[idx] = above[idx]
    g_c = (x_sc - x_db)[:, 0, :]
    b = torch.cat([1 - alpha, torch.zeros_like(alpha)], dim=-1).view(bs, 2)
    a = torch.cat([torch.ones_like(alpha), -alpha], dim=-1).view(bs, 2)
    n_fft = fft_len(n)
    H = torch.fft.rfft(b, n_fft) / torch.fft.rfft(a, n_fft)
    g_s = torch.fft.irfft(torch.fft.rfft(g_c, n_fft) * H, n_fft)[..., :n].view(bs, 1, n) + makeup
    if lookahead_samples > 0:
        x = torch.roll(x, lookahead_samples, dims=-1)
        x[:, :, :lookahead_samples] = 0
    return x * (10 ** (g_s / 20.0))


def distortion(x, params, sample_rate=None, precision="float64"):
    dt = _dtype(precision)
    drive = denormalize(params.to(dt)[:, 0], 0.0, 48.0).view(-1, 1, 1)
    return torch.tanh(x.to(dt) * (10 ** (drive / 20.0)))


def gain(x, params, sample_rate=None, precision="float64"):
    dt = _dtype(precision)
    g = denormalize(params.to(dt)[:, 0], -48.0, 48.0).view(-1, 1, 1)
    return x.to(dt) * (10 ** (g / 20.0))


def noise_shaped_reverberation(x, params, noise_bank, precision="float64"):
    """dasp_pytorch.noise_shaped_reverberation with the band-filtered noise (2, 12, taps) as an input: band gains, decays
    (* 10 + 1) and mix used raw; mono is copied to stereo; causal convolution with the impulse response, cut to n."""
    dt = _dtype(precision)
    bs, chs, n = x.shape
    p = params.to(dt)
    taps = noise_bank.shape[-1]
    t = torch.linspace(0, 1, steps=taps, dtype=dt)
    env = torch.exp(-(p[:, 12:24] * 10.0 + 1.0).view(bs, 1, 12, 1) * t.view(1, 1, 1, -1))
    ir = (noise_bank.to(dt)[None] * env * p[:, :12].view(bs, 1, 12, 1)).mean(dim=2)  # (bs, 2, taps)
    x = x.to(dt)
    if chs == 1:
        x = x.repeat(1, 2, 1)
    n_fft = 1 << (n + taps - 2).bit_length()
    y = torch.fft.irfft(torch.fft.rfft(x, n_fft) * torch.fft.rfft(ir, n_fft), n_fft)[..., :n]
    mix = p[:, 24].view(bs, 1, 1)
    return (1 - mix) * x + mix * y


def complex_autodiff_processor(x, params, sample_rate, noise_bank, precision="float64"):
    """apply_complex_autodiff_processor: EQ -> compressor -> distortion -> reverb -> gain on (bs, 51) raw parameters."""
    y = parametric_eq(x, params[:, :18], sample_rate, precision)
    y = compressor(y, params[:, 18:24], sample_rate, precision)
    y = distortion(y, params[:, 24:25], sample_rate, precision)
    y = noise_shaped_reverberation(y, params[:, 25:50], noise_bank, precision)
    return gain(y, params[:, 50:51], sample_rate, precision)


# ---- numpy prototypes of the kernels' formulation ---------------------------------------------------------------------------
def _sos_step(sos, x, z):
    """One direct-form-II-transposed step of the cascade (scipy.signal.sosfilt's), z: 2 states per section."""
    for k, s in enumerate(sos):
        y = s[0] * x + z[2 * k]
        z[2 * k] = s[1] * x - s[4] * y + z[2 * k + 1]
        z[2 * k + 1] = s[2] * x - s[5] * y
        x = y
    return x


def eq_periodic_start(sos, x):
    """The first n samples of circular filtering over N = fft_len(n) as the causal recursion started from
    s* = (I - A^N)^-1 A^(N - n) s_n (s_n: the zero-state state after the n samples); n == 1: rfft(b, 1) keeps b0 only, s* = 0."""
    sos = np.asarray(sos, dtype=np.float64)
    n, N, m = len(x), fft_len(len(x)), 2 * len(sos)
    A = np.zeros((m, m))
    for k in range(m):
        e = np.zeros(m)
        e[k] = 1.0
        _sos_step(sos, 0.0, e)
        A[:, k] = e
    z = np.zeros(m)
    for v in x:
        _sos_step(sos, float(v), z)
    s0 = np.zeros(m) if n == 1 else np.linalg.solve(np.eye(m) - np.linalg.matrix_power(A, N), np.linalg.matrix_power(A, N - n) @ z)
    z, y = s0.copy(), np.empty(n)
    for i, v in enumerate(x):
        y[i] = _sos_step(sos, float(v), z)
    return y


def onepole_periodic_start(alpha, g_c):
    """g[i] = alpha g[i - 1] + (1 - alpha) g_c[i] started from g* = alpha^(N - n) g_n / (1 - alpha^N)."""
    n, N = len(g_c), fft_len(len(g_c))
    g = 0.0
    for v in g_c:
        g = alpha * g + (1 - alpha) * v
    g = 0.0 if n == 1 else alpha ** (N - n) * g / (1 - alpha ** N)   # (n == 1: rfft(b, 1) / rfft(a, 1) = 1 - alpha, no wrap)
    out = np.empty(n)
    for i, v in enumerate(g_c):
        g = alpha * g + (1 - alpha) * v
        out[i] = g
    return out
