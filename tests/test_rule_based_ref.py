"""CPU side of the PST benchmark's baselines: the restatement of run_rule_based (tests/rule_based_ref.py) pinned to what the
reference's own functions produced (tests/golden/rule_based_eq.npz, tests/golden/make_golden_rule_based.py), run_random's
host logic with the render stubbed out, and run_rule_based's argument checks (made before any GPU work)."""
import os

import numpy as np
import pytest
import torch

import rule_based_ref as R
import st_ito_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rule_based_eq.npz")
BAR_REL = 1e-12


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("case", range(len(R.GOLDEN_CASES)))
def test_eq_half_matches_the_reference_fixture(case):
    """Average spectra, smoothed spectra, firwin2 taps and the filtered audio of the restatement against the reference's
    functions on the same seeded inputs: within 1e-12 of each record's largest magnitude."""
    seed, chs, n, sr = R.GOLDEN_CASES[case]
    g = np.load(GOLDEN)
    x, t = R.case_signals(seed, chs, n, sr)
    eq = R.eq_half(R.peak_normalize(x), R.peak_normalize(t), sr)
    for k in ("spec_in", "spec_ref", "sm_in", "sm_ref", "taps"):
        err = _rel(eq[k], g[f"c{case}_{k}"])
        print(f"[rule-based ref] case {case} {k}: rel err {err:.2e} (bar {BAR_REL:.0e})")
        assert err <= BAR_REL, (k, err)
    err = _rel(eq["filtered"][:, ::R.GOLDEN_STRIDE], g[f"c{case}_filtered"])
    print(f"[rule-based ref] case {case} filtered: rel err {err:.2e} (bar {BAR_REL:.0e})")
    assert err <= BAR_REL


def test_restatement_climbs_only_while_the_target_is_louder():
    """The hill-climb's trace: no step when the target is quieter than the input; otherwise the last delta is the first one
    at or under 0.25 LU, or the threshold ran out at 160 steps."""
    x, t = R.case_signals(21, 2, 24000, 48000)
    quiet = R.run_rule_based(t[None], (x * np.linspace(0, 1, x.shape[1], dtype=np.float32) ** 8)[None], 48000)
    assert quiet["steps"][0] == 0 and len(quiet["deltas"][0]) == 1
    loud = R.run_rule_based(x[None], np.sign(t)[None].astype(np.float32), 48000)
    k, d = int(loud["steps"][0]), loud["deltas"][0]
    assert k >= 1 and len(d) == k + 1 and all(v > 0.25 for v in d[:-1])
    assert d[-1] <= 0.25 or k == 160


def _plugins():
    from st_ito.effects import BasicCompressor, BasicParametricEQ, BasicReverb
    from st_ito.style_transfer import load_plugins
    one = lambda cls, nch: {"class_path": cls, "num_params": None, "num_channels": nch, "fixed_parameters": {}}  # noqa: E731
    plugins = {"ParametricEQ": one(BasicParametricEQ, 1), "Compressor": one(BasicCompressor, 1), "Reverb": one(BasicReverb, 2)}
    return load_plugins(plugins)[0]


def test_run_random_draws_one_vector_from_the_global_generator(monkeypatch):
    """run_random (reference style_transfer.py:138-160): w = torch.rand(total_num_params) from torch's global generator, the
    input's batch dimension dropped for the render and put back on the output, param_dict = parameters_to_dict(w)."""
    from st_ito import style_transfer as ST
    seen = {}

    def fake_render(x, w, sr, plugins, normalize_stages=False):
        seen["x"], seen["w"], seen["sr"] = np.asarray(x), np.asarray(w), sr
        return np.asarray(x, dtype=np.float32) * 0.5

    monkeypatch.setattr(ST.engine, "process_audio_gpu", fake_render)
    plugins = _plugins()
    D = sum(p["num_params"] for p in plugins.values())
    x = O.synth_audio(5, 2, 4096)[None]
    torch.manual_seed(1234)
    res = ST.run_random(x.clone(), x.clone(), 48000, plugins, None)
    torch.manual_seed(1234)
    w = torch.rand(D)
    np.testing.assert_array_equal(seen["w"], w.numpy())
    assert seen["x"].shape == (2, 4096) and seen["sr"] == 48000
    assert tuple(res["output_audio"].shape) == (1, 2, 4096)
    np.testing.assert_array_equal(res["output_audio"][0].numpy(), x[0].numpy() * 0.5)
    ref = O.parameters_to_dict(w.numpy(), O.make_plugins(["ParametricEQ", "Compressor", "Reverb"], with_bypass=True))
    assert list(res["param_dict"]) == list(ref)
    for plug in ref:
        assert list(res["param_dict"][plug]) == list(ref[plug])
        for k, v in ref[plug].items():
            assert res["param_dict"][plug][k] == pytest.approx(float(v), rel=1e-12, abs=0), (plug, k)


def test_run_input_returns_the_input():
    from st_ito.style_transfer import run_input
    x = torch.zeros(1, 2, 16)
    assert run_input(x, x, 48000, {}, None)["output_audio"] is x


@pytest.mark.parametrize("shape, sr, n_fft, err", [
    ((1, 3, 48000), 48000, 16384, ValueError),       # 3 channels: firwin2 / the meter fail in the reference
    ((1, 2, 12000), 48000, 16384, ValueError),       # 0.25 s: shorter than the meter's 400 ms block
    ((1, 2, 8000), 16000, 16384, ValueError),        # n <= n_fft / 2: reflect padding fails
    ((2, 48000), 48000, 16384, ValueError),          # not (bs, chs, n)
    ((1, 2, 48000), 48000, 12000, NotImplementedError),
])
def test_run_rule_based_rejects_shapes_it_cannot_process(shape, sr, n_fft, err):
    from st_ito.style_transfer import run_rule_based
    x = torch.rand(*shape)
    before = x.clone()
    with pytest.raises(err):
        run_rule_based(x, x.clone(), sr, {}, None, n_fft=n_fft)
    assert torch.equal(x, before)   # nothing normalised before the check


def test_eval_pst_method_names():
    """--methods maps onto the reference's result keys; the default stays input + style-es."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "st-ito_amd", "scripts"))
    import eval_pst
    assert list(eval_pst.METHODS.values()) == ["input", "random", "rule-based", "style-es (param-panns)"]
    assert tuple(eval_pst.DEFAULT_METHODS) == ("input", "style-es")
    with pytest.raises(NotImplementedError):
        eval_pst.run_pst_benchmark([], {}, None, "/nonexistent-never-created", methods=("input", "deepafx-st"))
