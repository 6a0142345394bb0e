"""CPU pins of tests/frontend_ref64.py, which the GPU edge tests (tests/test_gpu_frontend_edges.py) trust.

The float64 log-mel against the float32 oracle (oracle/st_ito_oracle.py: torchlibrosa's matrix DFT in torch) on the very
inputs and through the very comparison rule (frontend_ref64.check_logmel) the GPU file uses: the oracle has to pass the
rule with the suite's bars, which proves that the rule and the inputs are ones a correct float32 front end satisfies --
and against the golden log-mels the reference's own code produced.  The tail references against torch in float64.

Measured here (see profiles/frontend_edges.txt): the oracle's worst unresolved-cell power ratio is 8.6e-11 of the frame's
strongest band (EPS_UNRESOLVED = 4 x that); torch's float32 F.normalize / cosine_similarity are within 9.3e-8 (unit rows)
and 1.1e-7 (losses) of float64 on tail_inputs() (the tail bars = 4 x those).  Run with -s to see every figure."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_ref64 as R
import st_ito_oracle as O

SR = 48000


@functools.lru_cache(maxsize=3)
def _oracle(norm="none", front=R.AFX):
    """The oracle's Cnn14 with the given front end and input norm: the seeded AFx-Rep stand-in (non-trivial bn0
    statistics), or O.Cnn14 for another front end (only "none" there: its trunk and bn0 are not used)."""
    if front == R.AFX:
        return O.make_synthetic_model(0, input_norm=norm)
    assert norm == "none"
    return O.Cnn14(512, SR, front[0], front[1], front[2], 20, 20000, True, norm).eval()


def _tables(om):
    bn = om.bn0
    sc, sh = R.bn_eval_affine(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
    return om.logmel_extractor.melW.detach().numpy(), sc, sh


def _oracle_logmel(om, x, norm_passes=0):
    x = torch.from_numpy(np.array(x))
    for _ in range(norm_passes):
        for b in range(x.shape[0]):
            x[b] /= x[b].abs().max().clamp(1e-8)
    with torch.no_grad():
        lm = om.logmel(x)
    return lm.numpy().reshape(x.shape[0] * x.shape[1], -1, lm.shape[-1])


def _pin(name, om, front, norm, x, silent=(), noise=(), norm_passes=0):
    melW, sc, sh = _tables(om)
    ref, P = R.logmel(x, front[0], front[1], melW, norm, sc, sh, norm_passes)
    return R.check_logmel(name, _oracle_logmel(om, x, norm_passes), ref, P, norm, silent, noise, melW)


@pytest.mark.parametrize("norm", ["none", "minmax", "batchnorm"])
def test_logmel_ref64_vs_oracle_afx(norm):
    """The AFx-Rep group (both kernels' lengths), stereo and mono."""
    for n in R.AFX_LENGTHS:
        for chs in (2, 1):
            _pin(f"oracle afx {norm} n {n} chs {chs}", _oracle(norm), R.AFX, norm, R.batch(n, n, chs), *R.batch_streams(chs))


@pytest.mark.parametrize("norm", ["none", "minmax", "batchnorm"])
def test_logmel_ref64_vs_oracle_batch_sizes(norm):
    x = R.batch(12, 4097, 2, 12)
    _pin(f"oracle afx {norm} 12 items", _oracle(norm), R.AFX, norm, x, *R.batch_streams(2, 12))
    _pin(f"oracle afx {norm} one item", _oracle(norm), R.AFX, norm, R.batch(2048, 2048, 2)[1:2], (), (0, 1))


@pytest.mark.parametrize("norm_passes", [0, 1, 2])
def test_logmel_ref64_vs_oracle_peak_passes(norm_passes):
    """Peaks 0 and 1e-9 make the second pass live (1e-9 / 1e-8 = 0.1, then / 0.1); the peak-0 item stays at the clamp."""
    x = R.peak_batch(7, 4097)
    for norm in ("none", "minmax", "batchnorm"):
        _pin(f"oracle afx {norm} passes {norm_passes}", _oracle(norm), R.AFX, norm, x, (0, 1), (), norm_passes)
    lm, _ = R.logmel(x, 2048, 1024, _tables(_oracle())[0], "none", norm_passes=norm_passes)
    if norm_passes == 2:   # both passes bring every audible item to peak 1: the same log-mel whatever the item's scale was
        one, _ = R.logmel(x[1:] / np.abs(x[1:]).max(axis=(1, 2), keepdims=True).astype(np.float64), 2048, 1024,
                          _tables(_oracle())[0], "none")
        assert np.abs(lm[2:] - one).max() < 1e-6
    if norm_passes == 0:
        assert (lm[:4] == -100.0).all()   # peaks 0 and 1e-9: every band below the 1e-10 clamp


@pytest.mark.parametrize("front", R.OTHER_FRONT_ENDS)
def test_logmel_ref64_vs_oracle_other_front_ends(front):
    om = _oracle("none", front)
    for n in R.other_lengths(front[0], front[1]):
        for chs in (2, 1):
            _pin(f"oracle {front} n {n} chs {chs}", om, front, "none", R.batch(n + front[0], n, chs), *R.batch_streams(chs))


@pytest.mark.parametrize("mels", [256, 264])
def test_logmel_ref64_vs_oracle_n_mels_limit(mels):
    front = (2048, 1024, mels)
    _pin(f"oracle n_mels {mels}", _oracle("none", front), front, "none", R.batch(mels, 4097, 2), *R.batch_streams(2))


def test_noise_cap_on_reference_alone():
    """The cap, on the float64 reference alone: with 0.1 noise under a 0.3 tone no band of a noise-bearing stream is 60 dB
    below its frame's strongest one."""
    melW = _tables(_oracle())[0]
    for n in R.AFX_LENGTHS:
        for chs in (2, 1):
            _, P = R.logmel(R.batch(n, n, chs), 2048, 1024, melW, "none")
            noise = R.batch_streams(chs)[1]
            live = (melW != 0).any(axis=0)
            share = (P[noise][..., live] < 1e-6 * P[noise].max(axis=-1, keepdims=True)).mean()
            assert share <= R.UNRESOLVED_CAP, (n, chs, share)


@pytest.mark.parametrize("norm", ["minmax", "batchnorm", "none"])
def test_logmel_ref64_vs_golden(golden_dir, norm):
    """The log-mels the reference's own front end produced (stereo input of the trunk vectors), at the suite's bars."""
    g = np.load(os.path.join(golden_dir, f"cnn14_trunk_{norm}.npz"))
    melW, sc, sh = _tables(_oracle(norm))
    lm, _ = R.logmel(g["x"], 2048, 1024, melW, norm, sc, sh)
    err = np.abs(lm - g["logmel"].reshape(lm.shape)).max()
    print(f"[frontend-edges] float64 vs golden {norm}: max err {err:.3e}")
    assert err < (R.BAR_MINMAX if norm == "minmax" else R.BAR_DB)


# ---------------------------------------------------------------- the tail
def _torch64_tail(mid, side, tmid, tside):
    m, s = (F.normalize(torch.from_numpy(v).double(), p=2, dim=-1) for v in (mid, side))
    tm, ts = torch.from_numpy(tmid).double()[None], torch.from_numpy(tside).double()[None]
    return m.numpy(), s.numpy(), ((-F.cosine_similarity(m, tm, dim=-1) - F.cosine_similarity(s, ts, dim=-1)) / 2).numpy()


@pytest.mark.parametrize("n_cand", R.TAIL_CAND)
def test_tail_ref64_vs_torch64_and_float32_bar(n_cand):
    """embed_loss / neg_cosine against torch's float64 F.normalize / cosine_similarity (the eps rules included: zero
    rows, the norm-1e-13 row, rows of norm below 1e-8, a zero target), and the measurement behind the tail bars:
    torch's own float32 against float64 on these inputs, printed next to a quarter of the bars (the figures the bars were
    derived from on one host; they move with torch's reduction order, so the assertion is the bars themselves)."""
    worst_e = worst_l = 0.0
    for E in R.TAIL_E:
        mid, side, tm, ts = R.tail_inputs(E, n_cand)
        m, s, loss = R.embed_loss(mid, side, tm, ts)
        m64, s64, l64 = _torch64_tail(mid, side, tm, ts)
        np.testing.assert_allclose(m, m64, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(s, s64, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(loss, l64, rtol=0, atol=1e-14)
        assert (m[0] == 0).all() and np.isfinite(loss).all()
        if n_cand >= 3:
            assert abs(np.linalg.norm(m[1]) - 0.1) < 1e-6            # norm 1e-13 over the 1e-12 eps (float32 inputs)
        zl = R.embed_loss(mid, side, 0 * tm, 0 * ts)[2]
        assert (zl == 0).all()
        for emb, t in ((mid, tm), (side, ts)):                       # raw rows: tiny ones sit under the cosine's 1e-8 eps
            ref = -F.cosine_similarity(torch.from_numpy(emb).double(), torch.from_numpy(t).double()[None], dim=-1).numpy()
            np.testing.assert_allclose(R.neg_cosine(emb, t, 1.0), ref, rtol=0, atol=1e-14)
            prior = np.linspace(-1, 1, n_cand)
            np.testing.assert_allclose(R.neg_cosine(emb, t, 1 / 3, prior), prior + ref / 3, rtol=0, atol=1e-14)
            l32 = -F.cosine_similarity(torch.from_numpy(emb), torch.from_numpy(t)[None], dim=-1).numpy()
            worst_l = max(worst_l, float(np.abs(l32 - ref).max()))
        m32, s32 = F.normalize(torch.from_numpy(mid), p=2, dim=-1), F.normalize(torch.from_numpy(side), p=2, dim=-1)
        l32 = ((-F.cosine_similarity(m32, torch.from_numpy(tm)[None], dim=-1) - F.cosine_similarity(s32, torch.from_numpy(ts)[None], dim=-1)) / 2).numpy()
        worst_e = max(worst_e, float(np.abs(m32.numpy() - m).max()), float(np.abs(s32.numpy() - s).max()))
        worst_l = max(worst_l, float(np.abs(l32 - loss).max()))
    print(f"[frontend-edges] torch float32 tail vs float64, n_cand {n_cand}: unit rows {worst_e:.3e} (bar / 4 = {R.BAR_TAIL_EMB / 4:.1e}), "
          f"losses {worst_l:.3e} (bar / 4 = {R.BAR_TAIL_LOSS / 4:.1e})")
    assert worst_e <= R.BAR_TAIL_EMB and worst_l <= R.BAR_TAIL_LOSS


def test_tail_nonfinite_reference_order():
    """The float32 restatement: NaN in mid scrubs all of mid (its infs become +-FLT_MAX, whose squares overflow: that row
    normalises to 0) and leaves side alone; NaN in side only scrubs side; an inf without any NaN is not scrubbed."""
    mid, side, tm, ts = R.tail_inputs(65, 3)
    a = mid.copy(); a[2, 5] = np.nan; a[1, 3] = np.inf
    b = side.copy(); b[0, 7] = np.nan
    m, s, loss = R.embed_loss(a, b, tm, ts)
    assert m.dtype == np.float32 and (m[1] == 0).all() and np.isfinite(m).all()
    assert np.isnan(s[0]).all() and np.isnan(loss[0]) and np.isfinite(loss[1:]).all()
    m, s, loss = R.embed_loss(mid, b, tm, ts)
    assert np.isfinite(s).all() and np.isfinite(loss).all()
    a = mid.copy(); a[2, 5] = -np.inf
    m, s, loss = R.embed_loss(a, side, tm, ts)
    assert np.isnan(m[2, 5]) and (m[2, :5] == 0).all() and np.isnan(loss[2]) and np.isfinite(loss[:2]).all()
