"""Host side of the device-resident CMA-ES (csrc/cmaes.hip): the ABI declarations, the layout function's size query and its
refusals, what run_es(device_es=True) refuses before it touches its inputs, the pure-Python restatement of the generator's
integer stage that the GPU test uses as its reference, and the CLI flag.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import device_es_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stito_cmaes_state_bytes", "stito_cmaes_state_offsets", "stito_cmaes_init", "stito_cmaes_ask", "stito_cmaes_tell",
           "stito_cmaes_eigen", "stito_cmaes_export", "stito_cmaes_import", "stito_cmaes_status", "stito_cmaes_normals")


def test_abi_declares_the_device_es():
    from st_ito import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stito_hip.h")).read(), flags=re.S)
    lib = _hip.lib()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/stito_hip.h"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 6


def test_state_bytes_is_the_layout_and_refuses_unsupported_sizes():
    from st_ito import _hip, cmaes
    lib = _hip.lib()
    size = cmaes.device_es_state_bytes
    assert size(2, 2, 1) > 0
    assert size(36, 32, 100) < size(37, 32, 100) and size(36, 32, 100) < size(36, 33, 100) and size(36, 32, 100) < size(36, 32, 101)
    assert size(128, 1024, 300) % 8 == 0
    for N, lam, what in ((1, 8, "N = 1"), (129, 8, "N = 129"), (8, 1, "popsize 1"), (8, 1025, "popsize 1025")):
        assert lib.stito_cmaes_state_bytes(N, lam, 10) == _hip.E_UNSUPPORTED and what.encode() in lib.stito_last_error()
        with pytest.raises(NotImplementedError, match=what):
            size(N, lam, 10)
        with pytest.raises(NotImplementedError, match=what):   # the class refuses before it looks for a GPU
            cmaes.DeviceCMAEvolutionStrategy(np.full(N, 0.5), 0.1, {"bounds": [0, 1], "popsize": lam}, max_iters=10)
    # the offsets the binding reads are the same function's: consecutive fields, `persist` in front of the scratch words
    off = (_hip.c_int64 * 18)()
    assert lib.stito_cmaes_state_offsets(5, 8, 10, off, 18) == 18
    o = dict(zip(cmaes._DEV_FIELDS, off))
    assert o["ints"] == 0 and o["reals"] == o["n_ints"] == 17 and o["mean"] == 33 and o["C"] - o["weights"] == 8 and o["B"] - o["C"] == 25
    assert o["log_x"] - o["log_f"] == 10 and o["persist"] - o["log_disp"] == 10 * o["disp_row"] and o["persist"] * 8 < size(5, 8, 10)
    assert lib.stito_cmaes_state_offsets(5, 8, 10, off, 4) == _hip.E_INVALID


def test_run_es_refuses_before_it_touches_its_inputs(monkeypatch):
    from st_ito import effects as E, style_transfer as ST
    x, t = torch.rand(1, 1, 4000) * 0.3, torch.rand(1, 1, 4000) * 0.2
    x0, t0 = x.clone(), t.clone()
    plugins = E.make_plugins("eq")
    kw = dict(distance="mrstft", popsize=4, max_iters=3, device_es=True)
    with pytest.raises(ValueError, match="savepop"):
        ST.run_es(x, t, 48000, plugins, None, None, savepop=True, **kw)
    with pytest.raises(ValueError, match="sync_every"):
        ST.run_es(x, t, 48000, plugins, None, None, sync_every=0, **kw)
    with pytest.raises(ValueError, match="max_iters"):   # the host ES accepts 0; the device state is sized by it
        ST.run_es(x, t, 48000, plugins, None, None, **dict(kw, max_iters=0))
    with pytest.raises(NotImplementedError, match="popsize 1025"):
        ST.run_es(x, t, 48000, plugins, None, None, **dict(kw, popsize=1025))
    monkeypatch.setattr(ST, "_dist_info", lambda: (None, 0, 2))
    with pytest.raises(ValueError, match="world larger than 1"):
        ST.run_es(x, t, 48000, plugins, None, None, **kw)
    assert torch.equal(x, x0) and torch.equal(t, t0)   # not even peak-normalised


def test_generator_restatement_is_pinned():
    assert R.mix(0) == 0xE220A8397B1DCDAF          # splitmix64's published first output from state 0
    assert R.bits(0, 0, 0) == 2558736989570252433
    assert R.bits(12345, 7, 0) == 11788477536669367492
    assert R.bits(1, 2, 3) == 3042388159972110417
    assert R.bits(12345, 7, 1) != R.bits(12345, 8, 0) != R.bits(12346, 7, 0)
    assert R.normal(R.bits(12345, 7, 0)) == pytest.approx(-0.8756213038032866, abs=1e-15)
    z = np.array([R.normal(R.bits(5, 0, e)) for e in range(4096)])
    assert abs(z.mean()) < 5 / 64 and abs((z ** 2).mean() - 1) < 5 * np.sqrt(2 / 4096)


def test_cli_flag(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import run_optim
    from st_ito.audio_io import save_wav
    a = run_optim.build_parser().parse_args(["a.wav", "b.wav", "--device-es", "--sync-every", "8"])
    assert a.device_es and a.sync_every == 8
    a = run_optim.build_parser().parse_args(["a.wav", "b.wav"])
    assert not a.device_es and a.sync_every == 4
    with pytest.raises(ValueError, match="--staged"):
        run_optim.main(["a.wav", "b.wav", "--device-es", "--staged"])
    # the call main() builds: without the flag exactly the keywords it always passed
    rng = np.random.default_rng(0)
    for name in ("in.wav", "tgt.wav"):
        save_wav(str(tmp_path / name), torch.from_numpy(rng.uniform(-0.5, 0.5, (1, 4800)).astype(np.float32)), 48000)
    calls = []

    def fake_run_es(*args, **kwargs):
        calls.append(kwargs)
        return {"output_audio": torch.zeros(1, 1, 4800), "params": {}, "fopt": 0.0, "num_evals": 0, "fval_history": [0.0]}

    monkeypatch.setattr(run_optim, "run_es", fake_run_es)
    argv = [str(tmp_path / "in.wav"), str(tmp_path / "tgt.wav"), "--objective", "mrstft", "--chain", "eq", "--output-dir", str(tmp_path / "out")]
    run_optim.main(argv)
    run_optim.main(argv + ["--device-es", "--sync-every", "2"])
    today = ["max_iters", "popsize", "w0", "find_w0", "sigma0", "distance", "parallel", "dropout", "savepop", "normalize_stages", "run_dir",
             "seed", "early_stop"]
    assert list(calls[0]) == today
    assert list(calls[1]) == today + ["device_es", "sync_every"] and calls[1]["device_es"] is True and calls[1]["sync_every"] == 2
