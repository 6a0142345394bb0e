"""The two ends of the evaluate step against the float64 references of tests/frontend_ref64.py at their edges: the log-mel
front end (stito_logmel: k_logmel and k_logmel_wave of csrc/frontend.hip, through Cnn14.logmel) and the
embedding-to-fitness tail (stito_embed_loss, stito_neg_cosine of csrc/cnn14.hip, through the C ABI).

Front end.  Batches of six seeded items (frontend_ref64.batch: all zero, a silent stretch, a silent right channel,
left == right, impulses at samples 0, 1, n - 2, n - 1, times 1e3), compared by frontend_ref64.check_logmel: cells within
60 dB of their frame's strongest band are held to the suite's bars (2e-5 on the minmax scale, 2e-3 dB); weaker cells are
checked under "none" in the power domain against eps = 3.44e-10 of the frame's strongest band, four times the float32
oracle's own worst value (8.6e-11, measured on the CPU by tests/test_frontend_ref64.py, where the oracle passes this very
rule on these very inputs); all-silent streams and bands without a bin sit on the clamp exactly; on the noise-bearing
streams at most 1 % of the cells may be unresolved.  Every case prints its measured figures next to its bars (run with -s).

Tail.  E from 1 to 1000 and 1, 3, 70 candidates, rows at scales 1e-15 .. 1e15, zero rows, a row under the normalise eps,
a zero target, the normalise-only form, the accumulate / weight form of stito_neg_cosine; bars are four times the error
of torch's own float32 F.normalize / cosine_similarity against float64 on the same inputs (9.3e-8 on the unit rows,
1.1e-7 on the losses).  NaN / inf cases against the reference's float32 semantics restated with torch.

profiles/frontend_edges.txt records the measurements behind eps and the tail bars and the errors measured on the GPU.
"""
import numpy as np
import pytest
import torch

import frontend_ref64 as R
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
NORMS = ("none", "minmax", "batchnorm")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _product(dev, front, norm="none", state=None):
    from st_ito.models.panns import Cnn14
    pm = Cnn14(512, SR, front[0], front[1], front[2], 20, 20000, True, norm)
    if state is not None:
        pm.load_state_dict(state)
    return pm.eval().to(dev)


@pytest.fixture(scope="module")
def afx(dev):
    """The AFx-Rep model with the oracle's seeded weights (non-trivial bn0 statistics); the input norm is set per case."""
    return _product(dev, R.AFX, "none", O.make_synthetic_model(0).state_dict())


def _set_norm(pm, norm):
    if pm.input_norm != norm:
        pm.input_norm = norm
        pm._invalidate()    # the front-end tables are rebuilt with the norm
    return pm


def _tables(pm):
    bn = pm.bn0
    sc, sh = R.bn_eval_affine(bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.running_mean.cpu(), bn.running_var.cpu(), bn.eps)
    return pm.logmel_extractor.melW.detach().cpu().numpy(), sc, sh


_REFS = {}


def _ref(key, pm, x, norm, norm_passes=0):
    """The float64 reference of a case, computed once and shared by the tests that run the same input."""
    key = (key, norm, norm_passes)
    if key not in _REFS:
        melW, sc, sh = _tables(pm)
        _REFS[key] = R.logmel(x, pm.window_size, pm.hop_size, melW, norm, sc, sh, norm_passes)
    return _REFS[key]


def _peaks(dev, xd):
    from st_ito import _hip
    B, C, n = xd.shape
    peaks = torch.empty(B, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().stito_peak(_hip.ptr(xd), B, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return peaks


def _case(dev, name, key, pm, x, norm, silent=(), noise=(), norm_passes=None):
    xd = torch.from_numpy(x).to(dev).contiguous()
    if norm_passes is None:
        got = pm.logmel(xd)
    else:
        got = pm.logmel(xd, _peaks(dev, xd), norm_passes)
    ref, P = _ref(key, pm, x, norm, norm_passes or 0)
    return R.check_logmel(name, got.cpu().numpy(), ref, P, norm, silent, noise, _tables(pm)[0])


# ---------------------------------------------------------------- AFx-Rep front end (2048 / 1024 / 128 mels)
@pytest.mark.parametrize("norm", NORMS)
def test_logmel_afx_lengths(dev, afx, norm):
    """k_logmel below 2048 samples, k_logmel_wave from there: every hop reflected (2048), the last wave of a candidate
    holding 1, 2 or 3 of its four frames, workgroups whose later waves return early, 16 frames (one full workgroup) and
    17; odd lengths put the right channel and every other item off 8-byte alignment (the mono batch: item 1), 2050 is
    8-byte but not 16-byte aligned."""
    _set_norm(afx, norm)
    for n in R.AFX_LENGTHS:
        for chs in (2, 1):
            _case(dev, f"afx {norm} n {n} chs {chs}", ("afx", n, chs), afx, R.batch(n, n, chs), norm, *R.batch_streams(chs))


@pytest.mark.parametrize("norm", NORMS)
def test_logmel_afx_general_kernel(dev, afx, norm, monkeypatch):
    """The lengths from 2048 up again on k_logmel (STITO_LOGMEL_GENERIC=1), against float64 and not against the other
    kernel: its 16-byte (n % 4 == 0), 8-byte (n % 2 == 0) and scalar load paths, interior and reflected frames."""
    monkeypatch.setenv("STITO_LOGMEL_GENERIC", "1")
    _set_norm(afx, norm)
    for n in R.AFX_LENGTHS:
        for chs in (2, 1):
            if n >= 2048:
                _case(dev, f"afx general {norm} n {n} chs {chs}", ("afx", n, chs), afx, R.batch(n, n, chs), norm, *R.batch_streams(chs))


@pytest.mark.parametrize("norm", NORMS)
def test_logmel_afx_batch_sizes(dev, afx, norm):
    """Twelve items at scales 1e-4 .. 1e3 without normalisation, and one item alone."""
    _set_norm(afx, norm)
    _case(dev, f"afx {norm} 12 items", "afx12", afx, R.batch(12, 4097, 2, 12), norm, *R.batch_streams(2, 12))
    _case(dev, f"afx {norm} one item", "afx1", afx, R.batch(2048, 2048, 2)[1:2], norm, (), (0, 1))


@pytest.mark.parametrize("norm_passes", [0, 1, 2])
def test_logmel_afx_peak_passes(dev, afx, norm_passes, monkeypatch):
    """Items at peaks 0, 1e-9, exactly 1e-8, 3e-8, 1 and 1e3 (from stito_peak); with two passes the peaks 0 and 1e-9 make
    the second divisor differ from 1.  The reference does the passes literally in float64; the peak-0 item sits on the
    clamp under every setting.  Both kernels."""
    x = R.peak_batch(7, 4097)
    for norm in NORMS:
        _set_norm(afx, norm)
        for generic in ("0", "1"):
            monkeypatch.setenv("STITO_LOGMEL_GENERIC", generic)
            _case(dev, f"afx {norm} passes {norm_passes} generic {generic}", "peaks", afx, x, norm, (0, 1), (), norm_passes)


# ---------------------------------------------------------------- other front ends (k_logmel)
@pytest.mark.parametrize("front", R.OTHER_FRONT_ENDS)
def test_logmel_other_front_ends(dev, front):
    """n_fft 64 and 128 (the smallest; log2(n_fft / 2) odd and even), 512 with a hop that does and one that does not divide
    n_fft / 2, 1024, 4096 (the largest), each from its minimum length n_fft / 2 + 1."""
    pm = _product(dev, front)
    for n in R.other_lengths(front[0], front[1]):
        for chs in (2, 1):
            _case(dev, f"{front} n {n} chs {chs}", (front, n, chs), pm, R.batch(n + front[0], n, chs), "none", *R.batch_streams(chs))


@pytest.mark.parametrize("mels", [256, 264])
def test_logmel_n_mels_limit(dev, mels):
    """256 bands is the last size in k_logmel_wave's task table; 264 has to take k_logmel."""
    pm = _product(dev, (2048, 1024, mels))
    _case(dev, f"n_mels {mels}", ("mels", mels), pm, R.batch(mels, 4097, 2), "none", *R.batch_streams(2))


def test_logmel_refuses_too_short(dev, afx):
    """n = n_fft / 2 cannot be reflect-padded."""
    with pytest.raises(ValueError):
        afx.logmel(torch.ones((2, 2, 1024), device=dev))
    pm = _product(dev, (64, 32, 20))
    with pytest.raises(ValueError):
        pm.logmel(torch.ones((1, 1, 32), device=dev))
    pm.logmel(torch.ones((1, 1, 33), device=dev))


# ---------------------------------------------------------------- the tail
SENTINEL = 1234.5


def _err(name, got, ref, bar):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= bar, (name, err, bar)   # a NaN fails here too
    return err


def _embed_loss_abi(dev, mid, side, tmid=None, tside=None):
    """-> (mid, side, loss, flags mask: bit 0 NaN in mid, bit 1 NaN in side) after stito_embed_loss; the loss buffer is
    pre-filled with SENTINEL and the flag words with garbage."""
    from st_ito import _hip
    md, sd = torch.from_numpy(mid).to(dev).contiguous(), torch.from_numpy(side).to(dev).contiguous()
    tm = None if tmid is None else torch.from_numpy(tmid).to(dev)
    ts = None if tside is None else torch.from_numpy(tside).to(dev)
    loss = torch.full((mid.shape[0],), SENTINEL, dtype=torch.float32, device=dev)
    flags = torch.full((2,), 7, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().stito_embed_loss(_hip.ptr(md), _hip.ptr(sd), mid.shape[0], mid.shape[1], _hip.ptr(tm), _hip.ptr(ts),
                                           _hip.ptr(loss), _hip.ptr(flags), _hip.stream_ptr()))
    fl = flags.cpu().numpy()
    assert set(fl.tolist()) <= {0, 1}
    return md.cpu().numpy(), sd.cpu().numpy(), loss.cpu().numpy(), int(fl[0]) | int(fl[1]) << 1


@pytest.mark.parametrize("n_cand", R.TAIL_CAND)
def test_embed_loss_edges(dev, n_cand):
    """E off and on the multiples of 64 and 256 (strided loops, block_sum_256 with idle waves), 70 candidates with their
    own rows; rows at scales 1e-15 .. 1e15; an all-zero row stays zero with a finite loss; a row of norm 1e-13 is divided
    by the 1e-12 eps; a zero target gives loss 0; without targets the loss buffer is left alone.  The cosine's own 1e-8 eps
    inside k_embed_loss cannot bite here: after the normalise every non-zero row has norm 1 (0.1 for the norm-1e-13 row),
    and zero rows and the zero target have a zero dot product under any eps; a row whose normalised norm fell under 1e-8
    would need entries near 1e-21, whose float32 squares are denormal.  That eps is exercised on k_neg_cosine's raw rows
    (test_neg_cosine_accumulate), the same expression."""
    worst_e = worst_l = 0.0
    for E in R.TAIL_E:
        mid, side, tm, ts = R.tail_inputs(E, n_cand)
        rm, rs, rl = R.embed_loss(mid, side, tm, ts)
        gm, gs, gl, fl = _embed_loss_abi(dev, mid, side, tm, ts)
        worst_e = max(worst_e, _err(f"mid E {E}", gm, rm, R.BAR_TAIL_EMB), _err(f"side E {E}", gs, rs, R.BAR_TAIL_EMB))
        worst_l = max(worst_l, _err(f"loss E {E}", gl, rl, R.BAR_TAIL_LOSS))
        assert fl == 0 and (gm[0] == 0).all() and (gs[-1] == 0).all() == (n_cand >= 3) and np.isfinite(gl).all()
        _, _, zl, _ = _embed_loss_abi(dev, mid, side, 0 * tm, 0 * ts)
        assert (zl == 0).all(), zl
        nm, ns, nl, _ = _embed_loss_abi(dev, mid, side)
        assert (nl == np.float32(SENTINEL)).all() and np.array_equal(nm, gm) and np.array_equal(ns, gs)
    print(f"[frontend-edges] embed_loss n_cand {n_cand}: unit rows max err {worst_e:.3e} (bar {R.BAR_TAIL_EMB:.1e}), "
          f"loss max err {worst_l:.3e} (bar {R.BAR_TAIL_LOSS:.1e})")


@pytest.mark.parametrize("n_cand", R.TAIL_CAND)
def test_neg_cosine_accumulate(dev, n_cand):
    """accumulate = 0 over a NaN-filled loss buffer (a finite result: the old value is not read), then two more entries
    with accumulate = 1, all at weight 1 / 3: the mean of three distances, against float64.  Raw rows: the tiny ones sit
    under the cosine's 1e-8 eps, the zero rows give 0."""
    from st_ito import _hip
    worst = 0.0
    for E in R.TAIL_E:
        a, b, ta, tb = R.tail_inputs(E, n_cand)
        c, _, tc, _ = R.tail_inputs(E, n_cand, seed=1)
        loss = torch.full((n_cand,), float("nan"), dtype=torch.float32, device=dev)
        ref = None
        for i, (emb, tgt) in enumerate(((a, ta), (b, tb), (c, tc))):
            ed, td = torch.from_numpy(emb).to(dev), torch.from_numpy(tgt).to(dev)
            _hip.check(_hip.lib().stito_neg_cosine(_hip.ptr(ed), n_cand, E, _hip.ptr(td), 1.0 / 3.0, int(i > 0), _hip.ptr(loss),
                                                   _hip.stream_ptr()))
            ref = R.neg_cosine(emb, tgt, 1.0 / 3.0, ref)
            got = loss.cpu().numpy()
            assert np.isfinite(got).all(), (E, i, got)
            worst = max(worst, _err(f"neg_cosine E {E} entry {i}", got, ref, R.BAR_TAIL_LOSS))
    print(f"[frontend-edges] neg_cosine n_cand {n_cand}: max err {worst:.3e} (bar {R.BAR_TAIL_LOSS:.1e})")


def _same32(name, got, ref, bar):
    """Against the float32 restatement: identical where it is 0, +-1 or non-finite, within the bar elsewhere."""
    got, ref = np.asarray(got), np.asarray(ref)
    special = ~np.isfinite(ref) | (ref == 0) | (np.abs(ref) == 1)
    assert np.array_equal(got[special], ref[special], equal_nan=True), (name, got[special], ref[special])
    return _err(name, got[~special], ref[~special], bar) if (~special).any() else 0.0


@pytest.mark.parametrize("E", [512, 65])
def test_embed_loss_nonfinite(dev, E):
    """The reference's scrub, `if isnan(mid).any(): mid = nan_to_num(mid)  elif isnan(side).any(): side = nan_to_num(side)`,
    over the whole batch, then F.normalize and the cosine in float32: scrubbed infs become +-FLT_MAX, whose squares
    overflow, so their row normalises to 0; an unscrubbed inf gives NaN.  flags: bit 0 NaN in mid, bit 1 NaN in side."""
    mid, side, tm, ts = R.tail_inputs(E, 3)

    def put(v, *cells):
        v = v.copy()
        for r, c, val in cells:
            v[r, c] = val
        return v

    cases = {
        "NaN in one mid row": (put(mid, (2, 5, np.nan)), side, 1),
        "NaN in side only": (mid, put(side, (0, E - 1, np.nan)), 2),
        "NaN in both": (put(mid, (2, 0, np.nan)), put(side, (1, 3, np.nan)), 3),
        "+-inf in a mid row, NaN elsewhere in mid": (put(mid, (1, 2, np.inf), (1, E - 2, -np.inf), (2, 7, np.nan)), side, 1),
        "inf without NaN": (put(mid, (2, 4, np.inf)), put(side, (0, 1, -np.inf)), 0),
    }
    for name, (a, b, want_flags) in cases.items():
        rm, rs, rl = R.embed_loss(a, b, tm, ts)
        gm, gs, gl, fl = _embed_loss_abi(dev, a, b, tm, ts)
        em, es = _same32(f"{name}: mid", gm, rm, R.BAR_TAIL_EMB), _same32(f"{name}: side", gs, rs, R.BAR_TAIL_EMB)
        el = _same32(f"{name}: loss", gl, rl, R.BAR_TAIL_LOSS)
        print(f"[frontend-edges] embed_loss E {E} {name}: flags {fl}, unit rows max err {max(em, es):.3e} (bar {R.BAR_TAIL_EMB:.1e}), "
              f"loss max err {el:.3e} (bar {R.BAR_TAIL_LOSS:.1e}), loss {gl}")
        assert fl == want_flags, (name, fl)
        if name == "NaN in one mid row":
            assert np.isfinite(gm).all() and np.isfinite(gl).all()
        if name == "NaN in both":
            assert np.isfinite(gm).all() and np.isnan(gs[1]).all() and np.isnan(gl[1]) and np.isfinite(gl[[0, 2]]).all()
