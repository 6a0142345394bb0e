"""The input set behind tests/test_mrstft_host.py and tests/test_gpu_mrstft.py, generated from seeds: estimate / reference
pairs for the multi-resolution STFT distance at the lengths where the framing changes (n % hop = 0 and != 0 for the hops
120, 240 and 50; 1025 samples is the fewest torch.stft accepts at n_fft 2048: 5 frames at hop 240), mono and stereo, with
1, 3 and 5 items, plus the inputs that sit on the magnitude clamp.

`yardstick_max()` is the largest relative distance over the set between the two restatements of the loss that existed
before the kernel -- scripts/eval_synthetic.mrstft_error (float32 torch.stft on the CPU) and oracle.mrstft_error
(float64 numpy) -- item by item.  The host test bounds it; the GPU test's bar is four times it: the kernel is another
float32 evaluation, with a different FFT factorisation and the peak division folded into its loader as a multiplication.
"""
import os
import sys

import numpy as np
import torch

import st_ito_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1025, 1200, 2047, 2048, 2049, 4097, 12345, 12000)
BAR_FACTOR = 4.0


def _S():
    p = os.path.join(ROOT, "st-ito_amd", "scripts")
    if p not in sys.path:
        sys.path.insert(0, p)
    import eval_synthetic
    return eval_synthetic


def noise(seed, items, chs, n):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(torch.randn((items, chs, n), generator=g))


def two_tone(seed, items, chs, n):
    """Two sinusoids with 1e-3 of noise: the bins between the tones sit near the magnitude clamp."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 48000.0
    tone = 0.5 * torch.sin(2 * np.pi * 440.0 * t) + 0.25 * torch.sin(2 * np.pi * 5000.0 * t)
    return (tone[None, None, :] + 1e-3 * torch.randn((items, chs, n), generator=g, dtype=torch.float64)).to(torch.float32)


def cases():
    """[(name, x (P, C, n), y (P or 1, C, n), norm_passes)]: x the estimate, y the reference.  norm_passes 1: the estimate that is
    scored is x / clip(max|x|, 1e-8) per item."""
    out = []
    for i, n in enumerate(LENGTHS):
        chs, items = 1 + i % 2, (1, 3, 5)[i % 3]
        y = noise(100 + i, 1 if i % 4 == 0 else items, chs, n)
        x = torch.tanh(1.5 * noise(100 + i, items, chs, n) + 0.2 * noise(200 + i, items, chs, n))
        out.append((f"noise-{n}-c{chs}-p{items}", x, y, 0))
    for i, n in enumerate((2049, 12345)):
        y = two_tone(300 + i, 1, 2, n)
        x = 0.8 * two_tone(310 + i, 3, 2, n)
        out.append((f"twotone-{n}", x, y, 0))
    # an all-zero target channel: every |Y| of that row is the clamp 1e-4, so its convergence term is ~1e5 and carries the item.  The
    # property does not depend on the length, so the case has the fewest samples the framing accepts.  (The float32 restatement
    # sums the row's constant 1e-8 in float32, an error that grows with the number of bins: 3.6e-6 of the loss here, 1.1e-5 at
    # 4097 samples; the kernel sums in float64.)
    y = noise(400, 1, 2, 1025)
    y[:, 1] = 0.0
    out.append(("zero-target-channel-1025", noise(401, 3, 2, 1025), y, 0))
    out.append(("zero-candidate-1200", torch.zeros((1, 2, 1200)), noise(402, 1, 2, 1200), 1))
    x = 3.0 * noise(403, 5, 1, 2049)
    out.append(("peak-folded-2049", x, noise(404, 1, 1, 2049), 1))
    return out


def scored(x, norm_passes):
    """The estimate as the loss sees it: process_audio's joint peak normalisation when norm_passes is 1."""
    if not norm_passes:
        return x
    return x / x.abs().amax(dim=(1, 2), keepdim=True).clamp(min=1e-8)


_REF = {}


def reference(name, x, y, norm_passes):
    """oracle.mrstft_error item by item (float64), computed once per case."""
    if name not in _REF:
        xs = scored(x, norm_passes)
        _REF[name] = np.array([O.mrstft_error(xs[p:p + 1], y[p:p + 1] if y.shape[0] > 1 else y) for p in range(x.shape[0])])
    return _REF[name]


_YARD = {}


def yardstick():
    """{case: relative distance of the float32 torch.stft restatement from the float64 oracle, the largest over its items}"""
    if not _YARD:
        S = _S()
        for name, x, y, norm_passes in cases():
            ref = reference(name, x, y, norm_passes)
            xs = scored(x, norm_passes)
            got = np.array([float(S.mrstft_error(xs[p:p + 1], y[p:p + 1] if y.shape[0] > 1 else y)) for p in range(x.shape[0])])
            _YARD[name] = float(np.max(np.abs(got - ref) / np.abs(ref)))
    return _YARD


def yardstick_max():
    return max(yardstick().values())
