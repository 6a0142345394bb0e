"""The compressor as one kernel (k_comp_stage, compressor.hip: block functions, boundary scan and VCA as wave roles of one
workgroup) must give the BITS of the three-pass path it replaces (k_comp_blockfn / k_comp_blockscan / k_comp_apply, selected
by STITO_COMP_FUSED=0): the same operations on the same values, only kept in LDS instead of HBM.  GPU tests, plus the check
that the scan wave's generated source is what its generator prints."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000
G = 64           # blocks per segment of k_comp_stage (comp_stage.inc: STITO_COMP_STAGE_G)
SEG = 15 * G     # samples per segment

LENGTHS = [1, 14, 15, 16, 31, SEG - 1, SEG, SEG + 1, 2 * SEG + 7, 3 * SEG, 4003]
POPS = [1, 3, 5]

# (threshold_db, ratio, attack_ms, release_ms) as fractions of their ranges (-80..0 dB, 1..20, 0.1..100 ms, 10..1000 ms)
CORNERS = np.array([
    [0.5, 0.5, 1.0, 0.0],    # attack 100 ms > release 10 ms: the scan runs on z = -y (sg = -1)
    [0.3, 0.5, 0.0, 0.0],    # both time constants at the short end (at a few Hz both one-pole constants are 0: CB_CMIN, attack = release)
    [0.3, 0.5, 1.0, 1.0],    # both at the long end
    [0.5, 0.0, 0.3, 0.3],    # ratio 1
    [1.0, 0.5, 0.2, 0.2],    # threshold 0 dB, above a signal below full scale: the gain is exactly 1
    [0.0, 1.0, 0.0, 1.0],    # lowest threshold, highest ratio, fastest attack, slowest release
    [0.41, 0.77, 0.13, 0.58],
    [0.85, 0.15, 0.66, 0.02],
])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()
    return torch.device("cuda", 0)


def _inputs(C, L):
    rng = np.random.default_rng(1000 + 7 * L + C)
    noise = (rng.uniform(-1.0, 1.0, (C, L)) * 0.999).astype(np.float32)
    burst = np.zeros((C, L), np.float32)
    b0 = 13 if L > 18 else 0    # five samples across the first block boundary where the signal is long enough
    burst[:, b0:b0 + 5] = noise[:, b0:b0 + 5]
    return {"noise": noise, "silence": np.zeros((C, L), np.float32), "burst": burst}


@pytest.mark.gpu
@pytest.mark.parametrize("ns", ["", "2"], ids=["ns-default", "ns-2"])
@pytest.mark.parametrize("C", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("chain,sr", [("comp", SR), ("comp", 100.0), ("comp", 4.0), ("eq-comp", SR)],
                         ids=["comp-48k", "comp-100Hz", "comp-4Hz", "eq-comp-48k"])
def test_fused_compressor_is_bit_identical_to_the_three_passes(dev, monkeypatch, chain, sr, C, ns):
    """Every length around the block (15) and segment (15 G) edges, odd stream counts (with STITO_COMP_NS=2 the last workgroup
    is half filled), mono and stereo, the parameter corners as rows of the population, noise / silence / a five-sample burst.
    At 100 Hz the attack constant underflows to 0 (CB_CMIN); at 4 Hz attack and release both do (attack = release exactly)."""
    from st_ito import effects as E
    from st_ito.engine import render_population
    spec = [("Compressor", E.BasicCompressor, 1)]
    if chain == "eq-comp":
        spec = [("ParametricEQ", E.BasicParametricEQ, 1)] + spec
    plugins = E.make_plugins(spec)
    D = sum(p["num_params"] for p in plugins.values())
    rng = np.random.default_rng(3)
    if ns:
        monkeypatch.setenv("STITO_COMP_NS", ns)
    n_checked = 0
    for L in LENGTHS:
        for name, x_np in _inputs(C, L).items():
            x = torch.from_numpy(x_np).to(dev)
            for P in POPS:
                for off in range(0, len(CORNERS), P):
                    W = rng.random((P, D))
                    W[:, D - 4:] = CORNERS[(off + np.arange(P)) % len(CORNERS)]
                    Wd = torch.from_numpy(W).to(dev)
                    monkeypatch.delenv("STITO_COMP_FUSED", raising=False)
                    fused = render_population(plugins, x, Wd, sr)[0].cpu().numpy()
                    monkeypatch.setenv("STITO_COMP_FUSED", "0")
                    three = render_population(plugins, x, Wd, sr)[0].cpu().numpy()
                    np.testing.assert_array_equal(fused, three, err_msg=f"L={L} input={name} pop={P} corners from {off}")
                    n_checked += 1
    assert n_checked == len(LENGTHS) * 3 * (8 + 3 + 2)


@pytest.mark.gpu
def test_fused_compressor_under_graph_replay_matches_eager_launches(dev):
    """bench5 chain, pop 4, 2 s stereo: eager calls and graph replays with new parameters each give the same loss and embeddings."""
    import st_ito_oracle as O
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    n = 2 * SR
    x = O.synth_audio(41, 2, n)[None]
    tgt = O.synth_audio(42, 2, n)[None]
    pp = E.make_plugins("bench5")
    te = get_param_embeds(tgt, pm, SR)
    ev = PopulationEvaluator(x, SR, pp, pm, te, use_graph=False)
    evg = PopulationEvaluator(x, SR, pp, pm, te, capture_after=1)
    rng = np.random.default_rng(9)
    for rep in range(5):
        W = rng.random((4, 45))
        le, ee, _ = ev.evaluate(W)
        lg, eg, _ = evg.evaluate(W)
        assert len(evg._graphs) == (0 if rep < 1 else 1)   # one eager call, then the capture and its replays
        np.testing.assert_array_equal(le.cpu().numpy(), lg.cpu().numpy(), err_msg=f"replay {rep}")
        np.testing.assert_array_equal(ee["mid"].cpu().numpy(), eg["mid"].cpu().numpy())
        np.testing.assert_array_equal(ee["side"].cpu().numpy(), eg["side"].cpu().numpy())


def test_comp_stage_inc_is_its_generators_output(tmp_path):
    """st-ito_amd/csrc/comp_stage.inc is committed and must be, byte for byte, what `gen_comp_scan_asm.py stage` prints."""
    gen = os.path.join(ROOT, "tools", "gen", "gen_comp_scan_asm.py")
    run = subprocess.run([sys.executable, gen, "stage"], cwd=tmp_path, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    committed = open(os.path.join(ROOT, "st-ito_amd", "csrc", "comp_stage.inc"), "rb").read()
    assert run.stdout == committed, ("st-ito_amd/csrc/comp_stage.inc is not what its generator prints; regenerate it: "
                                     "python tools/gen/gen_comp_scan_asm.py stage > st-ito_amd/csrc/comp_stage.inc")
    assert not list(tmp_path.iterdir()), "the generator wrote a file: it is meant to print to stdout only"
