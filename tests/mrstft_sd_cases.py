"""The input set behind tests/test_mrstft_sd_host.py and tests/test_gpu_mrstft_sd.py: the stereo members of
tests/mrstft_cases.py plus the inputs that are special to the sum / difference distance, and its float64 reference.

The reference needs nothing new: the sum / difference distance IS the MR-STFT distance of [L + R, L - R], so it is
oracle.mrstft_error(sd(x), sd(y)) item by item, sd taken in float64 of the estimate as the loss scores it
(mrstft_cases.scored).  The yardstick is the one of the L/R distance, mrstft_cases.yardstick_max(), unchanged: `yardstick()`
here only measures the float32 restatement scripts/eval_synthetic.mrstft_error(sd(x), sd(y)) against it on this set.

The two clamp inputs have 1025 samples, the fewest the framing accepts, like mrstft_cases' zero-target-channel case and for
its reason: a row that sits entirely on the clamp makes the float32 restatement add the constant 1e-8 in float32, an error
that grows with the number of bins and is the restatement's, not the definition's."""
import numpy as np
import torch

import mrstft_cases as M
import st_ito_oracle as O


def sd(a):
    """(P, 2, n) -> float64 (P, 2, n): [L + R, L - R], no factor 1/2."""
    a = a.to(torch.float64)
    return torch.stack([a[:, 0] + a[:, 1], a[:, 0] - a[:, 1]], 1)


def sd32(a):
    """The same transform in float32, on a's device: what the kernel's loader does when no peak is folded in."""
    return torch.stack([a[:, 0] + a[:, 1], a[:, 0] - a[:, 1]], 1)


def cases():
    """[(name, x (P, 2, n), y (P or 1, 2, n), norm_passes)], the format of mrstft_cases.cases()."""
    out = [c for c in M.cases() if c[1].shape[1] == 2]
    # a mono-compatible target, L = R: its difference row is all zeros, every |Y| of it is the clamp 1e-4, so its convergence
    # term is of order 1e5 and carries the item -- the definition then demands a mono render
    y = M.noise(410, 1, 2, 1025)
    y[:, 1] = y[:, 0]
    x = M.noise(411, 3, 2, 1025)
    out.append(("sd-mono-target-1025", x, y, 0))
    # R = -L: the same for the sum row.  It is the pair above with channel 1 negated on both sides, which swaps the sum row and
    # the difference row of estimate and reference alike: the two cases have the same loss, a property the tests check as well.
    # (Every row that is wholly on the clamp puts the float32 restatement at about 3.6e-6 at this length, where the yardstick's
    # own worst case sits: this pair measures 3.56e-6, an independently seeded R = -L target measured 3.70e-6 against 3.64e-6.)
    x, y = x.clone(), y.clone()
    x[:, 1], y[:, 1] = -x[:, 1], -y[:, 1]
    out.append(("sd-antiphase-target-1025", x, y, 0))
    # (the all-zero candidate with peak folding is a stereo member of mrstft_cases already: zero-candidate-1200)
    out.append(("sd-peak-folded-2049", 3.0 * M.noise(415, 5, 2, 2049), M.noise(416, 1, 2, 2049), 1))
    return out


_REF = {}


def reference(name, x, y, norm_passes):
    """oracle.mrstft_error(sd(scored x), sd(y)) item by item (float64), computed once per name."""
    if name not in _REF:
        xs, ys = sd(M.scored(x, norm_passes)), sd(y)
        _REF[name] = np.array([O.mrstft_error(xs[p:p + 1], ys[p:p + 1] if ys.shape[0] > 1 else ys) for p in range(x.shape[0])])
    return _REF[name]


_YARD = {}


def yardstick():
    """{case: relative distance of the float32 restatement on (sd(x), sd(y)) from the float64 reference, the largest over its items}"""
    if not _YARD:
        S = M._S()
        for name, x, y, norm_passes in cases():
            ref = reference(name, x, y, norm_passes)
            xs, ys = sd(M.scored(x, norm_passes)), sd(y)
            got = np.array([float(S.mrstft_error(xs[p:p + 1], ys[p:p + 1] if ys.shape[0] > 1 else ys)) for p in range(x.shape[0])])
            _YARD[name] = float(np.max(np.abs(got - ref) / np.abs(ref)))
    return _YARD
