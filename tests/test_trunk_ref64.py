"""CPU pins of tests/trunk_ref64.py, which the GPU edge tests (tests/test_gpu_trunk_edges.py) trust.

The float64 trunk reference against the oracle's own nn.Module cast to double (two independent restatements of
panns.py:250-281) and against the stored golden embeddings; the measurement behind BAR_TRUNK -- the float32 oracle through
the very comparison rule on the very case list the GPU file uses; the coverage of the seeded map builder; the
measurement behind the stito_bn_fold bars.  Run with -s to see every figure; profiles/trunk_edges.txt records them."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import trunk_ref64 as R
import st_ito_oracle as O


def _biases(om):
    return om.fc_mid.bias.detach().numpy(), om.fc_side.bias.detach().numpy()


# one large and the short cases of A; every frame count of the others
SAMPLE = [c for c in R.cases() if (c[0] != "A" and c[2:] in ((9, 2), (3, 2))) or c in (("A", 33, 7, 2), ("A", 63, 8, 1), ("A", 95, 1, 2))]


@functools.lru_cache(maxsize=None)
def _oracle64(v):
    return copy.deepcopy(R.oracle_model(v)).double()


@pytest.mark.parametrize("case", SAMPLE, ids=R.case_id)
def test_ref64_vs_oracle_in_double(case):
    """Independent restatements: functional on state_dict tensors here, the nn.Module's own forward there."""
    v, T, n, c = case
    x, mid, side, _ = R.reference(*case)
    om = _oracle64(v)
    with torch.no_grad():
        omid, oside = om.trunk(torch.from_numpy(x).double()[:, None], n, c)
    err = max(R.row_errors(omid.numpy(), mid).max(), R.row_errors(oside.numpy(), side).max())
    print(f"[trunk-edges] float64 reference vs oracle.double() {R.case_id(case)}: {err:.3e}")
    assert err <= 1e-12, (case, err)
    if c == 1:
        assert np.array_equal(mid, side)


def test_ref64_vs_golden(golden_dir):
    """The embeddings the reference's own code produced in float32, from the log-mel of the oracle's front end in float64:
    the float32 distance, 4 x the worst measured value."""
    worst = 0.0
    for norm in ("minmax", "batchnorm", "none"):
        g = np.load(os.path.join(golden_dir, f"cnn14_trunk_{norm}.npz"))
        om = O.make_synthetic_model(int(g["seed"]), input_norm=norm).double()
        with torch.no_grad():
            lm = om.logmel(torch.from_numpy(g["x"]).double())[:, 0].numpy()
            lm1 = om.logmel(torch.from_numpy(g["x_mono"]).double())[:, 0].numpy()
        sd = om.state_dict()
        mid, side, _ = R.trunk64(sd, lm, 2, 2, om.conv_block1.bn1.eps)
        mono, mono_side, _ = R.trunk64(sd, lm1, 1, 1, om.conv_block1.bn1.eps)
        assert np.array_equal(mono, mono_side)
        errs = [R.row_errors(g["mid"], mid).max(), R.row_errors(g["side"], side).max(), R.row_errors(g["mid_mono"], mono).max()]
        print(f"[trunk-edges] float64 reference vs golden {norm}: mid {errs[0]:.3e}, side {errs[1]:.3e}, mid_mono {errs[2]:.3e} "
              f"(bar {R.BAR_GOLDEN:.2e} = 4 x {R.GOLDEN_WORST:.2e})")
        worst = max(worst, *errs)
    print(f"[trunk-edges] float64 reference vs golden: worst {worst:.3e}")
    assert worst <= R.BAR_GOLDEN, worst


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_bar_measurement_float32_oracle(variant):
    """The float32 oracle through check_rows on the complete case list: it passes the rule (so a correct float32 trunk can),
    and its worst row error is what BAR_TRUNK is ten times of -- a change of the case list that moves the floor shows here."""
    om = R.oracle_model(variant)
    bm, bs = _biases(om)
    worst = 0.0
    for case in R.cases((variant,)):
        _, T, n, c = case
        x, mid, side, feat = R.reference(*case)
        with torch.no_grad():
            omid, oside = om.trunk(torch.from_numpy(x)[:, None], n, c)
        worst = max(worst, R.check_rows(f"float32 oracle {R.case_id(case)}", omid.numpy(), oside.numpy(), mid, side, feat, bm, bs, c))
    print(f"[trunk-edges] float32 oracle, variant {variant}: worst row error {worst:.3e} (BAR_TRUNK / 10 = {R.ORACLE32_WORST:.2e})")
    assert worst <= R.BAR_TRUNK / 10 * 1.05, (variant, worst)


def test_case_list_and_builder_coverage():
    """Every map kind occurs at the mid and at the side position of a stereo batch and in a mono batch somewhere in the
    case list, for every variant; every batch of nine or more streams holds all kinds; the kinds are what maps() says."""
    assert len(R.cases()) == (3 * 6 + 4 * 3) + 3 * (2 * 6 + 3) == 75   # A: 3 short and 4 long frame counts; B, C, D: 2 and 1
    for v in R.VARIANTS:
        seen = {0: set(), 1: set(), "mono": set()}
        for _, T, n, c in R.cases((v,)):
            kinds = R.stream_kinds(T, n, c)
            if n * c >= 9:
                assert set(kinds) == set(range(R.N_KINDS))
            for s, k in enumerate(kinds):
                seen[s % 2 if c == 2 else "mono"].add(k)
        assert all(s == set(range(R.N_KINDS)) for s in seen.values()), (v, seen)
    x = R.maps(33, 40, 9, 2)
    k = R.stream_kinds(33, 9, 2)
    at = lambda kind: x[k.index(kind)]   # noqa: E731
    assert np.abs(at(0)).max() <= 1 and at(0).std() > 0.5 and np.abs(at(1)).max() <= 1e-3 and at(1).std() > 5e-4
    assert (at(2) == -1).all() and (at(3) == 0).all() and (at(6) == -100).all()
    assert (at(4) == 40).sum() == 1 and np.sort(np.abs(at(4)).ravel())[-2] <= 1
    assert at(5).min() < -95 and at(5).max() > 35 and at(5).min() >= -100 and at(5).max() <= 40
    assert (at(7)[:-1, :-1] != 0).sum() == 1 and at(7)[0, 0] == 1 and at(7)[0, -1] == 1 and at(7)[-1, 0] == 1 and at(7)[-1, -1] == 1
    assert (at(7)[-1, 1:-1] != 0).all() and (at(7)[1:-1, -1] != 0).all()
    assert np.abs(at(8)).max() > 900
    assert np.array_equal(x, R.maps(33, 40, 9, 2))


def test_zero_stream_of_variant_d_is_the_bias():
    """Identity BN: an all-zero map has all-zero features, so its output row is the FC bias -- the rows check_rows holds to
    1 ulp.  With batch norm the shifts make the same stream's features non-zero."""
    om = R.oracle_model("D")
    x, mid, side, feat = R.reference("D", 32, 9, 2)
    k = R.stream_kinds(32, 9, 2)
    s = k.index(3)
    assert (feat[s] == 0).all()
    ref = (mid if s % 2 == 0 else side)[s // 2]
    bias = (om.fc_mid if s % 2 == 0 else om.fc_side).bias.detach().double().numpy()
    assert np.array_equal(ref, bias)
    _, _, _, feat_a = R.reference("C", 32, 9, 2)
    assert (feat_a[R.stream_kinds(32, 9, 2).index(3)] != 0).any()


def test_bn_fold_float32_measurement():
    """The measurement behind the stito_bn_fold bars: g / sqrt(v + eps) and b - m scale in numpy float32 against float64."""
    ws = wh = 0.0
    for n in R.BN_FOLD_N:
        for g, b, m, v, eps in R.bn_fold_inputs(n):
            sc = g / np.sqrt(v + np.float32(eps))
            sh = b - m * sc
            assert sc.dtype == np.float32 and sh.dtype == np.float32
            es, eh = R.bn_fold_errors(sc, sh, g, b, m, v, eps)
            ws, wh = max(ws, es), max(wh, eh)
            assert (g < 0).any() or n == 1
    print(f"[trunk-edges] numpy float32 bn fold vs float64: scale {ws:.3e} (bar / 4 = {R.BN_FOLD32_SCALE:.2e}), "
          f"shift {wh:.3e} (bar / 4 = {R.BN_FOLD32_SHIFT:.2e})")
    assert ws <= R.BAR_BN_SCALE / 4 * 1.05 and wh <= R.BAR_BN_SHIFT / 4 * 1.05
