"""Host side of the multi-resolution STFT objective (csrc/mrstft.hip): the ABI declarations, the refusals that come before
anything needs a GPU, the CLI flag, and the yardstick that tests/test_gpu_mrstft.py measures the kernel with.

The yardstick: over the seeded input set of tests/mrstft_cases.py the float32 restatement scripts/eval_synthetic.mrstft_error
(torch.stft on the CPU) stays within 1e-5 of the float64 oracle.mrstft_error, item by item -- measured 3.6e-6 at most (the
all-zero target channel; 2.1e-6 on the two-tone signals whose off-tone bins sit near the clamp, <= 1.2e-6 on noise).  Four
times that maximum is the GPU test's bar, so a broken restatement cannot widen it silently.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import mrstft_cases as M

ROOT = M.ROOT
SYMBOLS = ("stito_mrstft_table_floats", "stito_mrstft_target", "stito_mrstft_workspace_bytes", "stito_mrstft_loss")


def test_symbols_declared_in_header_and_binding():
    from st_ito import _hip
    header = open(os.path.join(ROOT, "include", "stito_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/stito_hip.h"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
    assert "4 = stito_mrstft_table_floats" in header
    lib = _hip.lib()
    for name in SYMBOLS:
        getattr(lib, name)
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 4


def test_size_functions_on_the_host():
    """The plan behind both sizes asks no device: the defaults at 262144 samples are 3 588 681 magnitudes per row, and
    arguments the launches refuse give 0."""
    from st_ito import _hip, features as F
    lib = _hip.lib()
    res, n_res = F._mrstft_res(None)
    per_row = 1025 * 1093 + 513 * 2185 + 257 * 5243
    assert per_row == 3588681
    one, two = (lib.stito_mrstft_table_floats(res, n_res, r, 262144) for r in (1, 2))
    assert per_row <= two - one <= per_row + 1024            # + sums, tile scratch, padding to even
    assert lib.stito_mrstft_workspace_bytes(res, n_res, 256, 2, 262144) > 0
    assert lib.stito_mrstft_table_floats(res, n_res, 1, 1024) == 0 and lib.stito_mrstft_table_floats(res, n_res, 1, 1025) > 0
    assert lib.stito_mrstft_table_floats(res, 0, 1, 4096) == 0 and lib.stito_mrstft_table_floats(res, 9, 1, 4096) == 0
    for bad in ((1000, 100, 500), (128, 10, 100), (8192, 100, 500), (1024, 120, 1025), (1024, 0, 600)):
        arr = (ctypes.c_int * 3)(*bad)
        assert lib.stito_mrstft_table_floats(arr, 1, 1, 20000) == 0, bad
        assert lib.stito_mrstft_workspace_bytes(arr, 1, 4, 2, 20000) == 0, bad


def test_compute_mrstft_distance_refusals():
    from st_ito.features import compute_mrstft_distance
    x = torch.zeros((2, 2, 4096))
    with pytest.raises(ValueError):
        compute_mrstft_distance(x[0], x[0])                                   # not (B, C, n)
    with pytest.raises(ValueError):
        compute_mrstft_distance(x, torch.zeros((2, 1, 4096)))                 # channel mismatch
    with pytest.raises(ValueError):
        compute_mrstft_distance(x, torch.zeros((2, 2, 4095)))                 # length mismatch
    with pytest.raises(ValueError):
        compute_mrstft_distance(torch.zeros((3, 2, 4096)), x)                 # batch neither equal nor 1
    with pytest.raises(ValueError):
        compute_mrstft_distance(torch.zeros((1, 2, 1024)), torch.zeros((1, 2, 1024)))   # torch.stft's own condition
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(1024), 2048, 240, 1200, torch.hann_window(1200), return_complex=True)
    with pytest.raises(ValueError):
        compute_mrstft_distance(x, x, resolutions=[(1000, 100, 500)])
    with pytest.raises(ValueError):
        compute_mrstft_distance(x, x, resolutions=[(1024, 120, 2048)])
    with pytest.raises(ValueError):
        compute_mrstft_distance(x, x, resolutions=[])


def _es_args(n=4096, chs=1, tgt_chs=None, tgt_n=None):
    from st_ito import effects as E
    x = torch.rand((1, chs, n)) - 0.5
    t = torch.rand((1, tgt_chs or chs, tgt_n or n)) - 0.5
    return x, t, 48000, E.make_plugins("eq-comp", with_bypass=True), None, None


def test_run_es_refusals_come_before_any_launch(monkeypatch):
    """Every refusal of distance="mrstft" is raised before an evaluator exists; the inputs are still un-normalised then."""
    from st_ito import engine
    from st_ito.style_transfer import run_es

    def no_evaluator(*a, **k):
        raise AssertionError("an evaluator was built")
    monkeypatch.setattr(engine, "MrstftEvaluator", no_evaluator)
    monkeypatch.setattr(engine, "PopulationEvaluator", no_evaluator)
    kw = dict(distance="mrstft", popsize=4, max_iters=1, find_w0=False, seed=0)
    a = _es_args(tgt_n=4000)
    before = a[0].clone()
    with pytest.raises(ValueError, match="length"):
        run_es(*a, **kw)
    assert torch.equal(a[0], before)
    with pytest.raises(ValueError, match="channels"):
        run_es(*_es_args(chs=1, tgt_chs=2), **kw)
    with pytest.raises(ValueError, match="content_model"):
        run_es(*_es_args(), content_model=object(), content_embed_func=lambda *a: {}, **kw)
    with pytest.raises(ValueError, match="dropout"):
        run_es(*_es_args(), dropout=0.1, **kw)
    with pytest.raises(ValueError, match="savepop"):
        run_es(*_es_args(), savepop=True, **kw)
    for other in ("l2", "MRSTFT", ""):
        with pytest.raises(ValueError, match="Unknown distance"):
            run_es(*_es_args(), **dict(kw, distance=other))


def test_chain_out_channels_is_the_library_rule():
    from st_ito import _hip, effects as E, engine
    for chain in ("eq-comp", "basic", "bench5"):
        pl = E.make_plugins(chain)
        for c_in in (1, 2):
            descs, _ = engine.compile_chain(pl)
            assert engine.chain_out_channels(pl, c_in) == _hip.lib().stito_chain_out_channels(descs, len(pl), c_in)


def test_objective_flag():
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    p = run_optim.build_parser()
    assert p.parse_args(["in.wav"]).objective == "embedding"
    assert p.parse_args(["in.wav", "--objective", "mrstft"]).objective == "mrstft"
    with pytest.raises(SystemExit):
        p.parse_args(["in.wav", "--objective", "l2"])
    a = p.parse_args(["in.wav", "t.wav"])     # the reference's flags keep their defaults
    assert (a.max_iters, a.popsize, a.max_length, a.effect_type, a.algorithm, a.metric, a.dropout) == (300, 32, 262144, "vst", "es", "param", 0.0)


def test_float32_yardstick_stays_within_1e5_of_the_oracle():
    yard = M.yardstick()
    for name, v in yard.items():
        print(f"{name:28s} float32 torch.stft vs float64 oracle: {v:.3e}")
    assert len(yard) == len(M.cases()) and all(np.isfinite(v) for v in yard.values())
    assert M.yardstick_max() < 1e-5, yard
