"""Float64 reference of the stage between the log-mel front end and the embedding tail: the Cnn14 trunk (twelve 3x3 convs
with batch norm or identity and ReLU, five 2x2 average poolings), the pooling head (mean over mel, then max over time
plus mean over time) and the two linear layers -- panns.py:250-281 in eval mode, restated with torch.nn.functional on
double tensors taken from a state_dict.  It is not the oracle's nn.Module; tests/test_trunk_ref64.py pins the two against
each other on the CPU, and tests/test_gpu_trunk_edges.py compares stito_cnn14_forward with this one.

Also here, because the CPU and the GPU file must use the same ones: the model variants, the case list, the seeded map
builder, the comparison rule (check_rows) with its bar, and the inputs and the rule of the stito_bn_fold test.
profiles/trunk_edges.txt holds the measurements behind the bars.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import st_ito_oracle as O

SR = 48000
# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
# variant -> (embed_dim, mel_bins, use_batchnorm); the weights are O.fill_deterministic(model, SEEDS[variant])
VARIANTS = {
    "A": (512, 128, True),    # the AFx-Rep shape
    "B": (65, 64, True),      # a 2-wide final map; the last 64-wide FC output block holds one output
    "C": (512, 40, True),     # widths 40, 20, 10, 5, 2, 1: an odd width under a pooling, a 1-wide final map
    "D": (1000, 33, False),   # an odd width at the first layer; identity BN; 16 FC output blocks, the last one partial
}
SEEDS = {"A": 0, "B": 1, "C": 2, "D": 3}
FRAMES = {"A": (32, 33, 63, 64, 95, 127, 150), "B": (32, 63, 150), "C": (32, 63, 150), "D": (32, 63, 150)}
BATCHES_SHORT = ((1, 1), (1, 2), (7, 2), (8, 1), (9, 2), (17, 1))   # (n_cand, channels) at T <= 63
BATCHES_LONG = ((1, 2), (3, 2), (9, 1))                             # at larger T
T_SHORT = 63
T_REFUSED, MELS_REFUSED = 31, 31                                    # five floor-halvings of 31 leave nothing
N_KINDS = 9

# The bar of check_rows: per output row, max |got - ref| / max |ref|.  10 x the float32 oracle's (O.Cnn14.trunk on the CPU)
# own worst row error against this reference over cases(), measured by tests/test_trunk_ref64.py
# (profiles/trunk_edges.txt section 1): 4, the headroom the front-end and tail bars take over their float32 oracle, times
# 2.5 for the float32 Winograd F(4x4,3x3) transforms (profiles/round3_trunk_accuracy.txt: 1.68e-6 against 6.8e-7).
# torch's float32 convolutions sum in an order that depends on the number of threads, so this is the worst over runs with
# 1, 2, 4, 8 and 16 threads: 7.609e-07 (1 thread, case B-T63-17x1, a dB-range stream); 5.84e-07 .. 6.40e-07 with 2 to 16.
ORACLE32_WORST = 7.61e-7
BAR_TRUNK = 10 * ORACLE32_WORST
# the float64 reference against the stored float32 goldens (tests/golden/cnn14_trunk_*.npz), same row rule: 4 x measured
GOLDEN_WORST = 3.41e-7   # measured 3.403e-07 (batchnorm, mid_mono)
BAR_GOLDEN = 4 * GOLDEN_WORST
# stito_bn_fold: 4 x the worst error of the same expression in numpy float32 on bn_fold_inputs() (scale relative to |scale|,
# shift relative to |b| + |m scale|), measured by tests/test_trunk_ref64.py
BN_FOLD32_SCALE, BN_FOLD32_SHIFT = 1.18e-7, 1.58e-7   # measured 1.176e-07, 1.577e-07
BAR_BN_SCALE, BAR_BN_SHIFT = 4 * BN_FOLD32_SCALE, 4 * BN_FOLD32_SHIFT
BN_FOLD_N = (1, 64, 255, 256, 257, 2048)
TRANSPOSE_SHAPES = ((1, 1), (1, 2048), (65, 2048), (31, 33), (33, 31), (1000, 2048))


def batches(T: int):
    return BATCHES_SHORT if T <= T_SHORT else BATCHES_LONG


def cases(variants=("A", "B", "C", "D")):
    """Every (variant, T, n_cand, channels)."""
    return [(v, T, n, c) for v in variants for T in FRAMES[v] for n, c in batches(T)]


def case_id(case) -> str:
    v, T, n, c = case
    return f"{v}-T{T}-{n}x{c}"


# ---------------------------------------------------------------------------------------------------------------
# models and maps
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_model(variant: str):
    """The oracle's float32 Cnn14 of a variant with seeded weights, eval mode (input norm "none": the trunk tests feed maps)."""
    E, M, bn = VARIANTS[variant]
    return O.fill_deterministic(O.Cnn14(E, SR, 2048, 1024, M, 20, 20000, bn, "none"), SEEDS[variant]).eval()


def first_kind(T: int, n_cand: int, channels: int) -> int:
    """Kind of stream 0 of a batch: it moves with the case, so that the one- and two-stream batches differ."""
    return (T + 2 * n_cand + channels) % N_KINDS


def stream_kinds(T: int, n_cand: int, channels: int):
    k0 = first_kind(T, n_cand, channels)
    return [(k0 + s) % N_KINDS for s in range(n_cand * channels)]


def maps(T: int, M: int, n_cand: int, channels: int) -> np.ndarray:
    """(n_cand * channels, T, M) float32 log-mel maps; stream s is of kind stream_kinds()[s]:
      0 uniform noise in [-1, 1] (the minmax range)      1 the same x 1e-3            2 constant -1 (silence under minmax)
      3 all zero                                         4 noise, one cell set to 40  5 uniform in [-100, 40] (input norm "none")
      6 constant -100 (silence under "none")             7 zero but the four corners (1.0), the last row and the last column (noise)
      8 noise x 1e3"""
    rng = np.random.default_rng(100000 * T + 1000 * M + 10 * n_cand + channels)
    out = np.zeros((n_cand * channels, T, M))
    for s, kind in enumerate(stream_kinds(T, n_cand, channels)):
        noise = rng.uniform(-1.0, 1.0, (T, M))
        cell = (int(rng.integers(T)), int(rng.integers(M)))
        if kind == 0:
            out[s] = noise
        elif kind == 1:
            out[s] = noise * 1e-3
        elif kind == 2:
            out[s] = -1.0
        elif kind == 4:
            out[s] = noise
            out[s][cell] = 40.0
        elif kind == 5:
            out[s] = -30.0 + 70.0 * noise
        elif kind == 6:
            out[s] = -100.0
        elif kind == 7:
            out[s, -1, :] = noise[-1, :]
            out[s, :, -1] = noise[:, -1]
            out[s, [0, 0, -1, -1], [0, -1, 0, -1]] = 1.0
        elif kind == 8:
            out[s] = noise * 1e3
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def trunk64(sd, x, n_cand: int, channels: int, eps: float = 1e-5):
    """x (n_cand * channels, T, M) -> (mid (n_cand, E), side (n_cand, E), features (n_cand * channels, 2048)), float64 numpy.
    sd: a Cnn14 state_dict (any dtype); a block without bn tensors has identity in their place (use_batchnorm=False)."""
    d = lambda k: sd[k].detach().cpu().double()   # noqa: E731
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(x, dtype=np.float64))[:, None]
        for b in range(1, 7):
            for j in (1, 2):
                x = F.conv2d(x, d(f"conv_block{b}.conv{j}.weight"), padding=1)
                bn = f"conv_block{b}.bn{j}."
                if bn + "weight" in sd:
                    scale = d(bn + "weight") / torch.sqrt(d(bn + "running_var") + eps)
                    x = (x - d(bn + "running_mean")[:, None, None]) * scale[:, None, None] + d(bn + "bias")[:, None, None]
                x = torch.relu(x)
            if b < 6:
                x = F.avg_pool2d(x, 2)
        x = x.mean(dim=3)
        feat = x.max(dim=2).values + x.mean(dim=2)
        f = feat.view(n_cand, channels, -1)
        mid = f[:, 0] @ d("fc_mid.weight").T + d("fc_mid.bias")
        side = mid if channels == 1 else f[:, 1] @ d("fc_side.weight").T + d("fc_side.bias")
    return mid.numpy(), side.numpy(), feat.numpy()


@functools.lru_cache(maxsize=None)
def reference(variant: str, T: int, n_cand: int, channels: int):
    """(maps float32, mid, side, features) of a case, computed once and shared by every test that runs it; do not write to them."""
    x = maps(T, VARIANTS[variant][1], n_cand, channels)
    return (x,) + trunk64(oracle_model(variant).state_dict(), x, n_cand, channels)


# ---------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------
def row_errors(got, ref) -> np.ndarray:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


def check_rows(name: str, mid, side, ref_mid, ref_side, feat, bias_mid, bias_side, channels: int, bar: float | None = None) -> float:
    """Per output row (candidate; mid or side): max |got - ref| / max |ref| <= bar (BAR_TRUNK).  A row whose reference features
    are all exactly zero is the FC bias and must equal it to 1 ulp of float32.  No row is exempt.  Prints and returns the
    worst row error."""
    bar = BAR_TRUNK if bar is None else bar
    mid, side = np.asarray(mid), np.asarray(side)
    assert np.isfinite(mid).all() and np.isfinite(side).all(), name
    e = np.stack([row_errors(mid, ref_mid), row_errors(side, ref_side)], axis=1)     # (n_cand, 2)
    f = np.asarray(feat).reshape(mid.shape[0], channels, -1)
    n_bias = 0
    for kind, (got, bias) in enumerate(((mid, bias_mid), (side, bias_side if channels == 2 else bias_mid))):   # mono: side = mid
        zero = (f[:, kind if channels == 2 else 0] == 0).all(axis=1)
        b32 = np.asarray(bias, dtype=np.float32)
        for r in np.nonzero(zero)[0]:
            n_bias += 1
            off = np.abs(np.asarray(got[r], dtype=np.float32) - b32) / np.spacing(np.abs(b32))
            assert off.max() <= 1.0, (name, "bias row", int(r), ("mid", "side")[kind], float(off.max()))
    worst = np.unravel_index(e.argmax(), e.shape)
    print(f"[trunk-edges] {name}: worst row error {e.max():.3e} (bar {bar:.2e}) at candidate {int(worst[0])} {('mid', 'side')[worst[1]]}; "
          f"bias-only rows {n_bias}")
    assert e.max() <= bar, (name, float(e.max()), bar, tuple(int(i) for i in worst))
    return float(e.max())


# ---------------------------------------------------------------------------------------------------------------
# stito_bn_fold
# ---------------------------------------------------------------------------------------------------------------
def bn_fold_inputs(n: int):
    """[(gamma, beta, mean, var, eps)] float32 arrays of length n: gamma of both signs, variances 1e-12 .. 1e2 under eps
    1e-5, means of 1e3 with small beta (the shift is -mean * scale, beta nearly cancels out of it); then eps 0 with
    variance exactly 1."""
    rng = np.random.default_rng(n)
    g = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    b = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    m = (1e3 * rng.standard_normal(n)).astype(np.float32)
    v = rng.permutation(np.logspace(-12, 2, n)).astype(np.float32) if n > 1 else np.array([1e-12], dtype=np.float32)
    return [(g, b, m, v, 1e-5), (g, b, m, np.ones(n, dtype=np.float32), 0.0)]


def bn_fold64(g, b, m, v, eps: float):
    g, b, m, v = (np.asarray(a, dtype=np.float64) for a in (g, b, m, v))
    scale = g / np.sqrt(v + eps)
    return scale, b - m * scale


def bn_fold_errors(scale, shift, g, b, m, v, eps: float):
    """(worst scale error relative to |scale|, worst shift error relative to |b| + |m scale|) against float64."""
    rs, rh = bn_fold64(g, b, m, v, eps)
    f64 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    es = np.abs(f64(scale) - rs) / np.abs(rs)
    eh = np.abs(f64(shift) - rh) / (np.abs(f64(b)) + np.abs(f64(m) * rs))
    return float(es.max()), float(eh.max())
