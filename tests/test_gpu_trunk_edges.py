"""stito_cnn14_forward -- twelve conv layers, the pooling head k_head, the linear layers k_fc -- against the float64 reference
of tests/trunk_ref64.py at edge map shapes, through st_ito.models.panns.Cnn14; and stito_bn_fold / stito_transpose on their
own.

Four model variants (trunk_ref64.VARIANTS: 128, 64, 40 and 33 mels; embed_dim 512, 65, 512, 1000; the last one without
batch norm), frame counts from the minimum 32 up, odd at every pooling level (63 -> 31 -> 15 -> 7 -> 3 -> 1), batches that
leave k_fc's 8-candidate group partly empty, mono and stereo, and nine kinds of seeded maps per batch (trunk_ref64.maps:
noise at 1, 1e-3 and 1e3, constants -1 and -100, all zero, an outlier cell, the dB range, a map that is zero but for its
border).  The rule (trunk_ref64.check_rows): per output row max |got - ref| / max |ref| <= BAR_TRUNK, ten times the float32
oracle's own worst row error on the same cases (measured on the CPU by tests/test_trunk_ref64.py); a row whose reference
features are all zero equals the FC bias to 1 ulp; no row is exempt.  Every case prints its figures and the algorithm
each conv layer was given and whether the layer's map takes it (run with -s).

profiles/trunk_edges.txt records the measurements behind the bars, the errors measured on the GPU and the break checks.
"""
import numpy as np
import pytest
import torch

import trunk_ref64 as R
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
CHANS = (1, 64, 128, 256, 512, 1024, 2048)
ALGO_NAMES = {0: "direct", 1: "f2", 2: "f4", 3: "f4pre", 4: "split", 5: "split2", 8: "f2reg", 9: "split3"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _fresh(dev, variant, **config):
    """A new product model of a variant with the oracle's seeded weights; config: schedule attributes set before prepare()."""
    from st_ito.models.panns import Cnn14
    E, M, bn = R.VARIANTS[variant]
    pm = Cnn14(E, R.SR, 2048, 1024, M, 20, 20000, bn, "none")
    pm.load_state_dict(R.oracle_model(variant).state_dict())
    pm.eval().to(dev)
    for k, v in config.items():
        assert hasattr(pm, k), k
        setattr(pm, k, v)
    pm.prepare()
    return pm


_MODELS = {}


def _default(dev, variant):
    """The variant's model on the default configuration, built once for the module."""
    if variant not in _MODELS:
        _MODELS[variant] = _fresh(dev, variant)
    return _MODELS[variant]


def _biases(variant):
    om = R.oracle_model(variant)
    return om.fc_mid.bias.detach().numpy(), om.fc_side.bias.detach().numpy()


def _forward(pm, x, n_cand, channels, ws=None, ws_bytes=None):
    """stito_cnn14_forward as Cnn14.trunk() calls it, over NaN-prefilled outputs -> (return code, mid, side)."""
    from st_ito import _hip
    W, _, _ = pm._ensure()
    L = _hip.lib()
    T = x.shape[1]
    assert x.shape == (n_cand * channels, T, pm.mel_bins) and x.dtype == torch.float32 and x.is_contiguous()
    mid = torch.full((n_cand, pm.embed_dim), NAN, dtype=torch.float32, device=x.device)
    side = torch.full((n_cand, pm.embed_dim), NAN, dtype=torch.float32, device=x.device)
    if ws is None:
        ws = pm._workspace(L.stito_cnn14_workspace_bytes(W, n_cand * channels, T))
        ws_bytes = ws.numel()
    rc = L.stito_cnn14_forward(W, _hip.ptr(x), n_cand, channels, T, _hip.ptr(mid), _hip.ptr(side), _hip.ptr(ws), ws_bytes, _hip.stream_ptr())
    return rc, mid, side


def _layers(pm, S, T):
    """Per conv layer: the algorithm prepare() gave it, with '!' where this map does not take it (Trunk::conv falls back)."""
    from st_ito import _hip
    W, _, _ = pm._ensure()
    L = _hip.lib()
    H, Wd = [T], [pm.mel_bins]
    for _ in range(5):
        H.append(H[-1] // 2); Wd.append(Wd[-1] // 2)
    out = []
    for i in range(12):
        blk, j = divmod(i, 2)
        algo = int(W.conv_wino_algo[i]) if W.conv_wino_dev[i] else 0
        ok = L.stito_conv3x3_supported(S, H[blk], Wd[blk], CHANS[blk + j], CHANS[blk + 1], int(j == 1 and blk < 5), algo)
        out.append(ALGO_NAMES[algo] + ("" if ok else "!"))
    return f"maps {H[0]}x{Wd[0]} .. {H[5]}x{Wd[5]}, convs " + " ".join(out) + (" fused1" if W.conv1_f2reg_w_dev else "")


def _run_case(dev, pm, case, tag=""):
    from st_ito import _hip
    v, T, n, c = case
    x, ref_mid, ref_side, feat = R.reference(*case)
    print(f"[trunk-edges] {tag}{R.case_id(case)}: {_layers(pm, n * c, T)}")
    rc, mid, side = _forward(pm, torch.from_numpy(x).to(dev), n, c)
    _hip.check(rc)
    assert not torch.isnan(mid).any() and not torch.isnan(side).any(), R.case_id(case)
    if c == 1:
        assert torch.equal(mid, side)
    return R.check_rows(f"{tag}{R.case_id(case)}", mid.cpu().numpy(), side.cpu().numpy(), ref_mid, ref_side, feat, *_biases(v), c)


# ---------------------------------------------------------------- the trunk against float64
@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_trunk_vs_ref64(dev, case):
    """Every (variant, T, batch) on the default configuration."""
    _run_case(dev, _default(dev, case[0]), case)


SCHEDULES = {
    "direct": dict(conv_algo=0),
    "winograd_f2": dict(conv_algo=1),
    "float32_f4_pre": dict(conv_split=False),
    "float32_f4_in_kernel": dict(conv_split=False, conv_pre_min_cout=0),
    "no_f2reg": dict(conv_f2reg=False),
    "no_fuse1": dict(conv_fuse1=False),
    "chunk4_convs_2_6": dict(trunk_chunk=4, trunk_chunk_convs=(2, 6)),
}
SCHEDULE_CASES = {"A": [("A", 32, 9, 2), ("A", 63, 9, 2), ("A", 150, 3, 2)], "C": [("C", 63, 9, 2)]}


@pytest.mark.parametrize("variant", list(SCHEDULE_CASES))
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_trunk_other_schedules_vs_ref64(dev, schedule, variant):
    """The other conv algorithms and schedules, each held to float64 and not to another configuration: the direct kernel
    and F(2x2,3x3) everywhere, float32 F(4x4,3x3) with the input transform hoisted and in-kernel, the 64-input-channel
    layers without the register-resident kernel, conv_block1 as two launches, convs 2 .. 6 depth-first over chunks of
    four streams (18 streams: a last chunk of two)."""
    from st_ito import _hip
    assert (_hip.CONV_DIRECT, _hip.CONV_WINOGRAD) == (0, 1)
    pm = _fresh(dev, variant, **SCHEDULES[schedule])
    for case in SCHEDULE_CASES[variant]:
        assert case in R.cases()
        _run_case(dev, pm, case, f"{schedule} ")


@pytest.mark.parametrize("case,gain", [(("A", 63, 9, 2), 1.0), (("D", 63, 9, 2), 1.0), (("D", 150, 3, 2), 1.0), (("D", 63, 9, 2), 256.0)],
                         ids=lambda v: R.case_id(v) if isinstance(v, tuple) else f"x{v:g}")
def test_trunk_direct_layers_among_split_layers_vs_ref64(dev, case, gain):
    """Convs 3 and 8 without a Winograd packing (conv_wino_dev / conv_alt_dev NULL, as the C ABI allows): they run the direct
    kernel, which reports no per-stream maxima, in front of split-precision layers that scale their input by them -- conv 4
    and conv 9 have to scan their input themselves, while the layers around them still hand their maxima on.  On the
    default configuration every layer of every case above reports, so only this test sees the hand-off change its source.
    The last case is the variant-D batch times 256 (identity BN: the activations grow with the input, up to 2.6e5 at the
    x 1e3 stream): under a stale scale -- the zeroed maxima buffer reads as "scale 1" -- the f16 operands overflow there,
    whereas at log-mel magnitudes a scale of 1 happens to be harmless (profiles/trunk_edges.txt, section 5 f)."""
    from st_ito import _hip
    v, T, n, c = case
    pm = _fresh(dev, v)
    W, _, _ = pm._ensure()
    for i in (3, 8):
        W.conv_wino_dev[i] = None
        W.conv_alt_dev[i] = None
    if gain == 1.0:
        _run_case(dev, pm, case, "direct convs 3 and 8 ")
        return
    x = R.reference(*case)[0] * np.float32(gain)
    ref_mid, ref_side, feat = R.trunk64(R.oracle_model(v).state_dict(), x, n, c)
    rc, mid, side = _forward(pm, torch.from_numpy(x).to(dev), n, c)
    _hip.check(rc)
    R.check_rows(f"direct convs 3 and 8 {R.case_id(case)} x {gain:g}", mid.cpu().numpy(), side.cpu().numpy(), ref_mid, ref_side, feat, *_biases(v), c)


@pytest.mark.parametrize("variant", ["A", "C"])
def test_trunk_rows_do_not_depend_on_the_batch(dev, variant):
    """Candidates 0, 4 and 8 of the (9, 2) batch at T = 63 evaluated alone (n_cand = 1: a k_fc group with one candidate, two
    streams instead of 18 in every conv launch -- the six-sweep split layers switch to the two-sweep kernel) give the rows
    they had in the batch, bit for bit."""
    from st_ito import _hip
    pm = _default(dev, variant)
    x = torch.from_numpy(R.reference(variant, 63, 9, 2)[0]).to(dev)
    rc, mid, side = _forward(pm, x, 9, 2)
    _hip.check(rc)
    print(f"[trunk-edges] {variant} batch of 18 streams: {_layers(pm, 18, 63)}")
    print(f"[trunk-edges] {variant} batch of  2 streams: {_layers(pm, 2, 63)}")
    for cand in (0, 4, 8):
        rc, m1, s1 = _forward(pm, x[2 * cand:2 * cand + 2].contiguous(), 1, 2)
        _hip.check(rc)
        assert torch.equal(m1[0], mid[cand]) and torch.equal(s1[0], side[cand]), (variant, cand)


@pytest.mark.parametrize("case", [("A", 32, 9, 2), ("C", 63, 9, 2), ("D", 150, 3, 2)], ids=R.case_id)
def test_trunk_workspace_is_enough_and_not_exceeded(dev, case):
    """With exactly stito_cnn14_workspace_bytes the forward passes the rule and leaves the 4096 bytes behind the workspace
    alone; with one byte less it returns STITO_E_WORKSPACE before writing anything."""
    from st_ito import _hip
    v, T, n, c = case
    pm = _default(dev, v)
    W, _, _ = pm._ensure()
    need = _hip.lib().stito_cnn14_workspace_bytes(W, n * c, T)
    x, ref_mid, ref_side, feat = R.reference(*case)
    xd = torch.from_numpy(x).to(dev)
    ws = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0   # the forward aligns its workspace pointer up to 256 bytes
    ws[:need] = 0xFF                  # NaN bit patterns where the forward reads before it writes
    tail = (torch.arange(4096, device=dev) % 251).to(torch.uint8)
    ws[need:] = tail
    rc, mid, side = _forward(pm, xd, n, c, ws, need)
    _hip.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], tail), "the forward wrote behind its workspace"
    R.check_rows(f"exact workspace {R.case_id(case)}", mid.cpu().numpy(), side.cpu().numpy(), ref_mid, ref_side, feat, *_biases(v), c)
    rc, mid, side = _forward(pm, xd, n, c, ws, need - 1)
    assert rc == _hip.E_WORKSPACE, rc
    assert "workspace too small" in _hip.lib().stito_last_error().decode()
    assert torch.isnan(mid).all() and torch.isnan(side).all()


def test_trunk_refuses_too_short(dev):
    """31 frames or 31 mels leave nothing after five floor-halvings: the reference's avg_pool2d error, as STITO_E_INVALID
    (ValueError through Cnn14.trunk) before anything is written.  32 x 32, the smallest accepted map, passes the rule."""
    from st_ito import _hip
    from st_ito.models.panns import Cnn14
    pm = _default(dev, "A")
    x = torch.zeros((2, R.T_REFUSED, 128), device=dev)
    rc, mid, side = _forward(pm, x, 1, 2)
    assert rc == _hip.E_INVALID and "Calculated output size is too small" in _hip.lib().stito_last_error().decode()
    assert torch.isnan(mid).all() and torch.isnan(side).all()
    with pytest.raises(ValueError, match="Calculated output size is too small"):
        pm.trunk(x, 1, 2)
    for mels in (R.MELS_REFUSED, 32):
        om = O.fill_deterministic(O.Cnn14(64, R.SR, 2048, 1024, mels, 20, 20000, False, "none"), 5).eval()
        pn = Cnn14(64, R.SR, 2048, 1024, mels, 20, 20000, False, "none")
        pn.load_state_dict(om.state_dict())
        pn.eval().to(dev)
        xm = R.maps(32, mels, 1, 2)
        rc, mid, side = _forward(pn, torch.from_numpy(xm).to(dev), 1, 2)
        if mels == R.MELS_REFUSED:
            assert rc == _hip.E_INVALID and "Calculated output size is too small" in _hip.lib().stito_last_error().decode()
            assert torch.isnan(mid).all() and torch.isnan(side).all()
        else:
            _hip.check(rc)
            ref_mid, ref_side, feat = R.trunk64(om.state_dict(), xm, 1, 2)
            R.check_rows("32 x 32 map", mid.cpu().numpy(), side.cpu().numpy(), ref_mid, ref_side, feat, om.fc_mid.bias.detach().numpy(),
                         om.fc_side.bias.detach().numpy(), 2)


def test_variant_d_end_to_end_through_forward(dev):
    """The Python surface: pm(x) on two seconds of stereo audio with use_batchnorm=False and input_norm="none", against the
    float64 reference fed with the product's own log-mel."""
    pm = _default(dev, "D")
    assert pm.input_norm == "none" and not pm.use_batchnorm
    x = torch.stack([O.synth_audio(90 + i, 2, 2 * R.SR) for i in range(3)]).to(dev)
    mid, side = pm(x)
    lm = pm.logmel(x)
    assert lm.shape == (6, 94, 33)
    ref_mid, ref_side, feat = R.trunk64(R.oracle_model("D").state_dict(), lm.cpu().numpy(), 3, 2)
    R.check_rows("variant D end to end", mid.cpu().numpy(), side.cpu().numpy(), ref_mid, ref_side, feat, *_biases("D"), 2)


# ---------------------------------------------------------------- stito_bn_fold, stito_transpose
GUARD = 5   # elements behind every output that must stay NaN


@pytest.mark.parametrize("n", R.BN_FOLD_N)
def test_bn_fold_vs_float64(dev, n):
    """scale = g / sqrt(v + eps), shift = b - m scale against float64: gamma of both signs, variances down to 1e-12 under eps
    1e-5, eps 0 with variance 1, means of 1e3 against a small beta; sizes around the 256-thread block.  Bars: four times the
    error of the same expression in numpy float32 (tests/test_trunk_ref64.py).  Null pointers: exactly 1 and 0."""
    from st_ito import _hip
    L = _hip.lib()

    def fold(args, eps):
        scale = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev)
        shift = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev)
        _hip.check(L.stito_bn_fold(*[_hip.ptr(a) for a in args], eps, n, _hip.ptr(scale), _hip.ptr(shift), _hip.stream_ptr()))
        scale, shift = scale.cpu().numpy(), shift.cpu().numpy()
        assert np.isnan(scale[n:]).all() and np.isnan(shift[n:]).all(), "written past n"
        return scale[:n], shift[:n]

    for g, b, m, v, eps in R.bn_fold_inputs(n):
        scale, shift = fold([torch.from_numpy(a).to(dev) for a in (g, b, m, v)], eps)
        es, eh = R.bn_fold_errors(scale, shift, g, b, m, v, eps)
        print(f"[trunk-edges] bn_fold n {n} eps {eps}: scale {es:.3e} (bar {R.BAR_BN_SCALE:.2e}), shift {eh:.3e} (bar {R.BAR_BN_SHIFT:.2e})")
        assert es <= R.BAR_BN_SCALE and eh <= R.BAR_BN_SHIFT, (n, eps, es, eh)   # a NaN fails here too
    scale, shift = fold([None] * 4, 0.0)
    assert (scale == 1.0).all() and (shift == 0.0).all()


@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_SHAPES)
def test_transpose_bitwise(dev, rows, cols):
    """(rows, cols) -> (cols, rows) bit for bit, every element written and none behind the end; sizes off the 32 x 32 tile."""
    from st_ito import _hip
    a = torch.from_numpy(np.random.default_rng(rows * 4096 + cols).standard_normal((rows, cols)).astype(np.float32)).to(dev)
    out = torch.full((rows * cols + GUARD,), NAN, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().stito_transpose(_hip.ptr(a), rows, cols, _hip.ptr(out), _hip.stream_ptr()))
    assert torch.isnan(out[rows * cols:]).all(), "written past the end"
    assert torch.equal(out[:rows * cols].view(cols, rows), a.t().contiguous())
