"""Float64 references of the two ends of the evaluate step, in plain numpy: the log-mel front end (stito_logmel:
peak passes, mid / side, reflect padding, periodic Hann, power spectrum, mel bands, 10 log10 with the 1e-10 clamp,
input norm) and the embedding-to-fitness tail (stito_embed_loss, stito_neg_cosine).  The GPU edge tests
(tests/test_gpu_frontend_edges.py) compare the HIP kernels with these; tests/test_frontend_ref64.py pins them on the
CPU first, against the oracle, the golden log-mels and torch in float64.

Also here, because the CPU and the GPU file must use the same ones: the seeded batch builder, the case lists and the
comparison rule for log-mels (check_logmel).  profiles/frontend_edges.txt holds the measurements behind EPS_UNRESOLVED
and the tail bars.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
AFX = (2048, 1024, 128)   # the AFx-Rep front end: n_fft, hop, n_mels
AFX_LENGTHS = (1025, 1536, 2047, 2048, 2049, 2050, 3071, 3072, 3073, 4095, 4096, 4097, 5120, 16383, 16384, 16385, 17409)
OTHER_FRONT_ENDS = ((64, 32, 20), (128, 32, 40), (512, 128, 40), (512, 160, 64), (1024, 512, 64), (4096, 2048, 128))
PEAKS = (0.0, 1e-9, 1e-8, 3e-8, 1.0, 1e3)   # the peak-pass batch: item i is scaled to peak PEAKS[i] (float32 values)
TAIL_E = (1, 2, 63, 64, 65, 255, 256, 257, 512, 1000)
TAIL_CAND = (1, 3, 70)

BAR_MINMAX, BAR_DB = 2e-5, 2e-3   # test_logmel_vs_oracle_and_golden's bars: the [-1, 1] scale; dB ("none", "batchnorm")
RESOLVED_DB = -60.0               # a cell is resolved when its float64 band power is within this of the frame's strongest band
UNRESOLVED_CAP = 0.01             # at most this share of the cells of noise-bearing streams may be unresolved
# unresolved cells, power domain, relative to the frame's strongest band: four times the float32 oracle's own worst
# value on these inputs (8.6e-11, measured by tests/test_frontend_ref64.py; see profiles/frontend_edges.txt)
EPS_UNRESOLVED = 4 * 8.6e-11
# the tail: four times the worst error of torch's own float32 F.normalize / cosine_similarity against float64 on
# tail_inputs() (measured by tests/test_frontend_ref64.py: 9.3e-8 on the unit rows, 1.1e-7 on the losses)
BAR_TAIL_EMB, BAR_TAIL_LOSS = 4 * 9.3e-8, 4 * 1.1e-7


def other_lengths(n_fft: int, hop: int):
    return sorted({n_fft // 2 + 1, n_fft - 1, n_fft, n_fft + 1, 3 * hop + 1, 8 * hop})


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def batch(seed: int, n: int, chs: int = 2, count: int = 6, sr: int = 48000) -> np.ndarray:
    """(count, chs, n) float32.  Every item is 0.1 white noise plus a 0.3 tone (its own frequency, a phase per channel);
    item 0 is all zero, item 1 has its middle third zeroed, item 2 (stereo) a silent right channel, item 3 (stereo)
    left == right, item 4 is noise plus unit impulses at samples 0, 1, n - 2, n - 1 (stereo: 0 and n - 2 land in mid,
    1 and n - 1 in side), item 5 is times 1e3; with more than six items, items 5.. are scaled 1e3 down to 1e-4."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.1 * rng.standard_normal((count, chs, n))
    tone = 0.3 * np.sin(2 * np.pi * rng.uniform(50.0, 5000.0, (count, 1, 1)) * t + rng.uniform(0.0, 6.3, (count, chs, 1)))
    tone[4] = 0.0
    x += tone
    x[0] = 0.0
    x[1, :, n // 3:2 * n // 3] = 0.0
    if chs == 2:
        x[2, 1] = 0.0
        x[3, 1] = x[3, 0]
    edge = np.array([0, 1, n - 2, n - 1])
    x[4, 0, edge] += 1.0
    if chs == 2:
        x[4, 1, edge] += np.array([1.0, -1.0, 1.0, -1.0])
    x[5:] *= np.logspace(3, -4, count - 5)[:, None, None] if count > 6 else 1e3
    return x.astype(np.float32)


def batch_streams(chs: int, count: int = 6):
    """(all-silent streams, noise-bearing streams) of batch(): stream = item * chs + (0 mid, 1 side).  Silent: the zero
    item and the side of the left == right item.  Noise-bearing (the cap applies): items 1, 2 and 5.. ."""
    silent = list(range(chs)) + ([3 * chs + 1] if chs == 2 else [])
    noise = [i * chs + c for i in (1, 2) + tuple(range(5, count)) for c in range(chs)]
    return silent, noise


def peak_batch(seed: int, n: int, chs: int = 2) -> np.ndarray:
    """batch() without its special items, item i rescaled so that its float32 peak is float32(PEAKS[i]) exactly."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000
    x = 0.1 * rng.standard_normal((len(PEAKS), chs, n))
    x += 0.3 * np.sin(2 * np.pi * rng.uniform(50.0, 5000.0, (len(PEAKS), 1, 1)) * t + rng.uniform(0.0, 6.3, (len(PEAKS), chs, 1)))
    out = np.empty(x.shape, dtype=np.float32)
    for i, pk in enumerate(PEAKS):
        y = (x[i] * (pk / np.abs(x[i]).max())).astype(np.float32)
        y.flat[np.abs(x[i]).argmax()] = np.float32(pk) * np.sign(x[i].flat[np.abs(x[i]).argmax()])
        assert np.abs(y).max() == np.float32(pk)
        out[i] = y
    return out


# ---------------------------------------------------------------------------------------------------------------
# log-mel front end
# ---------------------------------------------------------------------------------------------------------------
def bn_eval_affine(weight, bias, mean, var, eps: float):
    """BatchNorm in eval mode as v * scale + shift."""
    scale = _f64(weight) / np.sqrt(_f64(var) + eps)
    return scale, _f64(bias) - _f64(mean) * scale


def logmel(x, n_fft: int, hop: int, melW, norm: str, bn_scale=None, bn_shift=None, norm_passes: int = 0, center: bool = True):
    """x (B, C, n) -> (log-mel (B * C, T, n_mels) after the input norm, band powers P of the same shape before the log).
    Streams are ordered mid, side per item (one stream per mono item).  melW is the product's own (n_fft / 2 + 1, n_mels)
    float32 table, cast up."""
    x = _f64(x).copy()
    B, C, n = x.shape
    for _ in range(norm_passes):     # x[b] /= x[b].abs().max().clamp(1e-8), the second pass on the result of the first
        x /= np.maximum(np.abs(x).max(axis=(1, 2), keepdims=True), 1e-8)
    if C == 2:
        x = np.stack([(x[:, 0] + x[:, 1]) / 2, (x[:, 0] - x[:, 1]) / 2], axis=1)
    elif C != 1:
        raise ValueError(f"Invalid number of channels: {C}")
    sig = x.reshape(B * C, n)
    if center:
        sig = np.pad(sig, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    frames = sliding_window_view(sig, n_fft, axis=-1)[:, ::hop]                      # (S, T, n_fft)
    P = (np.abs(np.fft.rfft(frames * win, axis=-1)) ** 2) @ _f64(melW)
    lm = 10.0 * np.log10(np.maximum(P, 1e-10))
    if norm == "minmax":
        lm = (np.clip(lm, -80.0, 40.0) + 80.0) / 120.0 * 2.0 - 1.0
    elif norm == "batchnorm":
        lm = lm * _f64(bn_scale) + _f64(bn_shift)
    elif norm != "none":
        raise ValueError(f"Invalid input_norm: {norm}")
    return lm, P


def check_logmel(name: str, got, ref, P, norm: str, silent=(), noise=(), melW=None, eps: float = EPS_UNRESOLVED) -> dict:
    """The comparison rule.  Per (stream, frame) Pmax is the largest float64 band power; a cell is resolved when
    P >= 10^(RESOLVED_DB / 10) * Pmax.
      resolved cells:    |got - ref| <= BAR_MINMAX ("minmax") or BAR_DB (dB; "none", "batchnorm");
      unresolved cells:  only under "none", in the power domain: |10^(got / 10) - max(P, 1e-10)| <= eps * max(Pmax, 1e-10);
      all-silent streams (`silent`): every cell equals the clamp value exactly (-100 dB, -1.0 under minmax);
      bands with no bin at all (a zero column of melW): as all-silent -- their power is 0 by construction, not by
                         cancellation, so the clamp value is owed exactly (under "batchnorm", where no exact value is
                         defined, they are held to BAR_DB like resolved cells); they count neither as resolved nor towards
                         the cap.  Only the (64, 32, 20) and (128, 32, 40) front ends have such bands (4 of 20, 7 of 40: the
                         mel spacing at the bottom is finer than their bins); counted, they would be 20 % / 18 % of the
                         noise-bearing cells whatever the input, so no input could meet the cap;
      cap:               on the streams in `noise` at most UNRESOLVED_CAP of the (non-empty-band) cells are unresolved.
    Prints the measured figures next to their bars and returns them."""
    got, ref, P = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(P, dtype=np.float64)
    assert got.shape == ref.shape == P.shape, (name, got.shape, ref.shape, P.shape)
    bar = BAR_MINMAX if norm == "minmax" else BAR_DB
    empty = np.zeros(P.shape, dtype=bool)
    if melW is not None:
        empty[..., ~(_f64(melW) != 0.0).any(axis=0)] = True
    Pmax = P.max(axis=-1, keepdims=True)
    resolved = (P >= 10.0 ** (RESOLVED_DB / 10.0) * Pmax) & ~empty
    unresolved = ~resolved & ~empty
    d = np.abs(got - ref)
    exact = {"none": -100.0, "minmax": -1.0}.get(norm)
    held = resolved if exact is not None else resolved | empty
    err = float(d[held].max()) if held.any() else 0.0
    worst = np.unravel_index(np.where(held, np.nan_to_num(d, nan=np.inf), -1.0).argmax(), d.shape)
    ratio = 0.0
    if norm == "none" and unresolved.any():
        r = np.abs(10.0 ** (got / 10.0) - np.maximum(P, 1e-10)) / np.maximum(Pmax, 1e-10)
        ratio = float(r[unresolved].max())
    sil_bad = 0
    if exact is not None:
        sil = empty.copy()
        sil[list(silent)] = True
        sil_bad = int((got[sil] != exact).sum())
        if sil_bad:
            print(f"[frontend-edges] {name}: off the clamp by up to {np.abs(got[sil] - exact).max():.3e}, e.g. {got[sil][got[sil] != exact][0]!r}")
    nz = np.zeros(P.shape, dtype=bool)
    nz[list(noise)] = True
    nz &= ~empty
    share = float(unresolved[nz].mean()) if nz.any() else 0.0
    print(f"[frontend-edges] {name}: resolved max err {err:.3e} (bar {bar:.0e}) at {tuple(int(i) for i in worst)}; "
          f"unresolved {int(unresolved.sum())} cells, power ratio {ratio:.3e} (eps {eps:.1e}); "
          f"noise-stream unresolved share {share:.4f} (cap {UNRESOLVED_CAP}); silent cells off the clamp {sil_bad}")
    assert np.isfinite(got).all(), name
    assert err <= bar, (name, err, bar, worst)
    assert ratio <= eps, (name, ratio, eps)
    assert sil_bad == 0, (name, sil_bad)
    assert share <= UNRESOLVED_CAP, (name, share)
    return {"err": err, "ratio": ratio, "unresolved": int(unresolved.sum()), "share": share}


# ---------------------------------------------------------------------------------------------------------------
# embeddings -> fitness
# ---------------------------------------------------------------------------------------------------------------
def _normalize64(e):
    return e / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-12)        # F.normalize, eps 1e-12


def _cos64(a, b):
    """torch.cosine_similarity: a.b / (max(|a|, 1e-8) max(|b|, 1e-8)) over the last axis."""
    na, nb = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)
    return (a * b).sum(axis=-1) / (np.maximum(na, 1e-8) * np.maximum(nb, 1e-8))


def _finite(*arrs) -> bool:
    return all(a is None or np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in arrs)


def embed_loss(mid, side, tmid=None, tside=None):
    """(normalised mid, normalised side, loss or None): NaN scrub, F.normalize, mean over {mid, side} of
    -cosine_similarity to the (E,) targets.  Finite inputs: float64.  Inputs with NaN or +-inf: the reference's own
    float32 semantics in its own order, with torch on the CPU (the overflow of v * v to inf is part of it):
    `if isnan(mid).any(): mid = nan_to_num(mid)  elif isnan(side).any(): side = nan_to_num(side)`, then F.normalize,
    then the cosine."""
    if _finite(mid, side, tmid, tside):
        m, s = _normalize64(_f64(mid)), _normalize64(_f64(side))
        if tmid is None:
            return m, s, None
        return m, s, ((-_cos64(m, _f64(tmid)[None])) + (-_cos64(s, _f64(tside)[None]))) / 2.0
    import torch
    import torch.nn.functional as F
    m, s = torch.as_tensor(np.asarray(mid, dtype=np.float32)), torch.as_tensor(np.asarray(side, dtype=np.float32))
    if torch.isnan(m).any():
        m = torch.nan_to_num(m)
    elif torch.isnan(s).any():
        s = torch.nan_to_num(s)
    m, s = F.normalize(m, p=2, dim=-1), F.normalize(s, p=2, dim=-1)
    if tmid is None:
        return m.numpy(), s.numpy(), None
    tm, ts = torch.as_tensor(np.asarray(tmid, dtype=np.float32))[None], torch.as_tensor(np.asarray(tside, dtype=np.float32))[None]
    loss = torch.stack([-F.cosine_similarity(m, tm, dim=-1), -F.cosine_similarity(s, ts, dim=-1)]).mean(dim=0)
    return m.numpy(), s.numpy(), loss.numpy()


def neg_cosine(emb, tgt, weight: float, prior=None):
    """prior + weight * -cosine_similarity(emb[c], tgt) (prior None: 0); float64 for finite inputs, torch float32 otherwise."""
    if _finite(emb, tgt, prior):
        v = weight * -_cos64(_f64(emb), _f64(tgt)[None])
        return v if prior is None else _f64(prior) + v
    import torch
    import torch.nn.functional as F
    e, t = torch.as_tensor(np.asarray(emb, dtype=np.float32)), torch.as_tensor(np.asarray(tgt, dtype=np.float32))[None]
    v = np.float32(weight) * -F.cosine_similarity(e, t, dim=-1).numpy()
    return v if prior is None else np.asarray(prior, dtype=np.float32) + v


def tail_inputs(E: int, n_cand: int, seed: int = 0):
    """(mid, side, tmid, tside) float32: rows of scales spread over 1e-15 .. 1e15 (seeded order); in mid, row 0 is all
    zero and (from three rows) row 1 has norm 1e-13, below the normalise eps; in side the same two rows sit at the end."""
    rng = np.random.default_rng(1000 * E + n_cand + seed)
    out = []
    for flip in (False, True):
        v = rng.standard_normal((n_cand, E)) * rng.permutation(np.logspace(-15, 15, n_cand))[:, None]
        zero, tiny = (n_cand - 1, n_cand - 2) if flip else (0, 1)
        if n_cand >= 3:
            v[tiny] = rng.standard_normal(E)
            v[tiny] *= 1e-13 / np.linalg.norm(v[tiny])
        if n_cand >= 3 or not flip:
            v[zero] = 0.0
        out.append(v.astype(np.float32))
    t = rng.standard_normal((2, E)).astype(np.float32)
    return out[0], out[1], t[0], t[1]
