"""The FX-Encoder on the GPU against its float64 restatement (tests/fx_encoder_ref64.py): single fused layers at the shapes where
the kernels can go wrong, whole stacks, batch independence, get_fx_encoder_embeds and run_es.

The bar of a case family is BAR_FACTOR = 4 times the family's yardstick d32: the largest max-abs distance, over the family's
cases, of the SAME restatement run in float32 on the CPU from the float64 one.  The factor is the project's standing allowance
for a different summation order; d32 is computed here, at run time, never from the GPU result.  Every case prints its error, the
family's d32 and the bar (run with -s); with STITO_MEASURE_DIR set the table is also written there as fx_encoder_edges.txt, which
is how profiles/fx_encoder_edges.txt was recorded."""
import functools
import os

import numpy as np
import pytest
import torch

import fx_encoder_ref64 as R

pytestmark = pytest.mark.gpu
BAR_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_encoder_toy.npz")
REPORT = []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    yield torch.device("cuda", 0)
    out = os.environ.get("STITO_MEASURE_DIR")
    if out and REPORT:
        with open(os.path.join(out, "fx_encoder_edges.txt"), "w") as f:
            f.write("FX-Encoder on the GPU against float64 (tests/test_gpu_fx_encoder.py): max-abs error per case, the family's d32\n"
                    "(float32 CPU restatement against float64, largest over the family) and the bar = 4 x d32\n\n")
            f.write("\n".join(REPORT) + "\n")


def report(family, case, err, d32, ref_max):
    line = f"{family:8s} {case:58s} err {err:.3e}  d32 {d32:.3e}  bar {BAR_FACTOR * d32:.3e}  max|ref| {ref_max:.3g}"
    REPORT.append(line)
    print(line)


# ---------------------------------------------------------- single layers ---------------------------------------------------------- #
# (cin, cout, K, stride, L, B, residual).  N tiles of the implicit GEMM: 256 columns for cout <= 32, else 128; cin 2 with a kernel
# and stride of the network runs on the vector ALU in tiles of 1024 outputs.
LAYER_CASES = [
    (2, 2, 25, 1, 13, 1, True),       # vector ALU; L = r_pad + 1: the two reflections overlap
    (2, 16, 25, 4, 4101, 2, False),   # vector ALU, stride 4, L not a multiple of it, 1026 outputs = two tiles
    (2, 1, 10, 2, 6, 3, False),       # vector ALU, even kernel, L = r_pad + 1
    (2, 33, 15, 2, 257, 1, False),
    (2, 2, 5, 1, 1025, 3, True),      # vector ALU, one output into the second tile
    (2, 5, 7, 3, 50, 3, False),       # cin 2 at a kernel the vector-ALU kernel does not have: the GEMM
    (5, 1, 25, 4, 13, 1, False),      # GEMM, L = r_pad + 1
    (5, 5, 10, 1, 6, 3, True),        # L = r_pad + 1 with K = 10, residual, items of 6 columns inside one tile
    (5, 33, 25, 4, 509, 1, False),    # 128 outputs: exactly one N tile
    (5, 33, 25, 4, 513, 1, False),    # one tile + 1
    (5, 33, 25, 4, 505, 1, False),    # one tile - 1
    (5, 1, 15, 2, 511, 1, False),     # 256 outputs: one tile of the narrow-M kernel
    (5, 1, 15, 2, 513, 1, False),
    (5, 1, 15, 2, 509, 1, False),
    (33, 33, 10, 1, 100, 3, True),    # tiles straddle the items at columns 100 and 200
    (33, 65, 10, 2, 199, 3, False),
    (33, 128, 5, 1, 129, 1, False),
    (33, 1, 5, 2, 171, 3, False),     # 86 outputs per item: 258 columns, two tiles, both item boundaries in the first
    (33, 130, 5, 1, 64, 2, False),    # two M tiles, the second nearly empty
    (64, 64, 15, 1, 131, 3, True),    # 960 reduction indices: four accumulator segments
    (64, 65, 15, 2, 255, 1, False),
    (64, 128, 25, 4, 1001, 3, False),
    (64, 33, 5, 1, 127, 1, False),
    (64, 1, 10, 2, 301, 3, False),
]


def layer_id(c):
    return "cin{}_cout{}_K{}_s{}_L{}_B{}{}".format(*c[:6], "_res" if c[6] else "")


def layer_inputs(c):
    cin, cout, k, s, n, b, res = c
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + k + n + 1)
    return R.random_layer(g, cin, cout, k), torch.randn(b, cin, n, generator=g)


@functools.lru_cache(maxsize=None)
def layer_family():
    """{case: (float64 reference, d of the float32 restatement)} and the family's d32."""
    refs = {}
    for c in LAYER_CASES:
        p, x = layer_inputs(c)
        ref = R.layer(x, p, c[3], c[6])
        assert float(ref.abs().max()) > 0.5, c   # a case whose ReLU left nothing would check nothing
        refs[c] =(ref, float((R.layer(x, p, c[3], c[6], dtype=torch.float32).double() - ref).abs().max()))
    return refs, max(d for _, d in refs.values())


def run_layer(c, dev, x=None):
    from st_ito.models.fx_encoder import conv1d_layer, fold_batch_norm
    p, x0 = layer_inputs(c)
    x = x0 if x is None else x
    scale, shift = fold_batch_norm(p["bias"], p["gamma"], p["beta"], p["mean"], p["var"])
    return conv1d_layer(x.to(dev), p["weight"], scale, shift, c[3], c[6]).cpu()


@pytest.mark.parametrize("case", LAYER_CASES, ids=layer_id)
def test_single_layer(dev, case):
    refs, d32 = layer_family()
    ref = refs[case][0]
    got = run_layer(case, dev)
    assert got.shape == ref.shape and (ref.shape[2] == -(-case[4] // case[3]))
    err = float((got.double() - ref).abs().max())
    report("layer", layer_id(case), err, d32, float(ref.abs().max()))
    assert err <= BAR_FACTOR * d32


@pytest.mark.parametrize("case", [(33, 65, 10, 2, 199, 3, False), (2, 16, 25, 4, 4101, 2, False), (64, 64, 15, 1, 131, 3, True)], ids=layer_id)
def test_single_layer_item_alone_has_the_same_bits(dev, case):
    _, x = layer_inputs(case)
    assert torch.equal(run_layer(case, dev)[1], run_layer(case, dev, x[1:2])[0])


# -------------------------------------------------------------- stacks -------------------------------------------------------------- #
MIDDLE = dict(channels=[16, 32, 64, 128], kernels=[25, 25, 15, 15], strides=[4, 4, 2, 2])


def golden_net():
    from st_ito.models.fx_encoder import FXencoder
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd:")}
    m = FXencoder(channels=list(z["channels"]), kernels=list(z["kernels"]), strides=list(z["strides"]))
    m.load_state_dict(sd)   # rounded to float32 here, as the float32 restatement rounds them
    return m, torch.from_numpy(z["x"]), torch.from_numpy(z["y"]), R.blocks_from_state_dict(sd, z["strides"])


@functools.lru_cache(maxsize=None)
def stack_family():
    """name -> (model, input, float64 reference, d of the float32 restatement); the parameters are made on the CPU, the models
    move to the GPU when they first run."""
    from st_ito.models.fx_encoder import FXencoder
    from st_ito.utils import make_synthetic_fx_encoder
    fam = {}
    m, x, y_recorded, golden_blocks = golden_net()
    fam["golden-toy_L211_B3"] = [m, x.float(), golden_blocks]   # the reference is the recorded output: float64 parameters and input
    mid = make_synthetic_fx_encoder(5, **MIDDLE).cpu()
    fam["middle_L4099_B3"] = [mid, torch.randn(3, 2, 4099, generator=torch.Generator().manual_seed(6)), R.blocks_from_model(mid)]
    big = make_synthetic_fx_encoder(7).cpu()
    n = big.min_input_length()
    fam[f"default_L{n}_B2"] = [big, torch.randn(2, 2, n, generator=torch.Generator().manual_seed(8)), R.blocks_from_model(big)]
    for name, v in fam.items():
        x64 = x if name.startswith("golden") else v[1]
        ref = R.stack(x64, v[2])
        v[2:] = [ref, float((R.stack(x64, v[2], dtype=torch.float32).double() - ref).abs().max())]
    assert float((fam["golden-toy_L211_B3"][2] - y_recorded).abs().max()) < 1e-12
    assert isinstance(big, FXencoder) and big.embed_dim == 2048
    return fam, max(v[3] for v in fam.values())


@pytest.mark.parametrize("which", [0, 1, 2], ids=["golden-toy", "middle", "default-shortest"])
def test_stack(dev, which):
    fam, d32 = stack_family()
    name = list(fam)[which]
    model, x, ref, _ = fam[name]
    if which == 2:   # one sample shorter is refused by name before anything is launched
        with pytest.raises(ValueError, match=r"encoder\.\d+\.conv[12]"):
            model(x[..., :-1].to(dev))
    got = model.to(dev)(x.to(dev)).cpu()
    assert got.shape == ref.shape == (x.shape[0], model.embed_dim)
    err = float((got.double() - ref).abs().max())
    report("stack", name, err, d32, float(ref.abs().max()))
    if which == 2:
        model.cpu()
        model._prepared = None   # 325 MB of packed weights: not kept for the rest of the session
    assert err <= BAR_FACTOR * d32


def test_stack_item_alone_has_the_same_bits(dev):
    fam, _ = stack_family()
    model, x = fam["middle_L4099_B3"][:2]
    model.to(dev)
    assert torch.equal(model(x.to(dev))[1], model(x[1:2].to(dev))[0])
    assert torch.equal(model(torch.cat([x[2:], x[1:2], x[:1], x[1:2]]).to(dev))[3], model(x[1:2].to(dev))[0])


# ------------------------------------------------------ get_fx_encoder_embeds ------------------------------------------------------ #
def embed_inputs():
    g = torch.Generator().manual_seed(11)
    x = 0.3 * torch.randn(3, 2, 16384, generator=g)
    x[0] *= 2.5   # item 0 holds the batch's peak
    return x


@functools.lru_cache(maxsize=None)
def embed_family():
    """case -> (input at 48 kHz, peak mode, float64 reference, d of the float32 restatement), on the product's own resampled audio."""
    from st_ito.audio_io import resample
    fam, _ = stack_family()
    blocks = R.blocks_from_model(fam["middle_L4099_B3"][0])
    x = embed_inputs()
    half = x.clone()
    half[0] *= 0.5
    mono = x[:, :1].contiguous()
    cases = {"stereo_batch": (x, "batch"), "stereo_item": (x, "item"), "stereo_batch_item0-halved": (half, "batch"),
             "stereo_item_item0-halved": (half, "item"), "mono_batch": (mono, "batch")}
    out = {}
    for name, (a, peak) in cases.items():
        r = resample(a.cuda(), 48000, 44100).cpu()
        assert r.shape[-1] == 15053
        ref = R.embeds(r, blocks, peak)
        out[name] = (a, peak, ref, float((R.embeds(r, blocks, peak, dtype=torch.float32).double() - ref).abs().max()))
    return out, max(v[3] for v in out.values())


def test_get_fx_encoder_embeds(dev):
    from st_ito.utils import get_fx_encoder_embeds
    model = stack_family()[0]["middle_L4099_B3"][0].to(dev)
    fam, d32 = embed_family()
    got = {}
    for name, (a, peak, ref, _) in fam.items():
        before = a.clone()
        e = get_fx_encoder_embeds(a, model, 48000, peak=peak)
        assert set(e) == {"stereo"} and e["stereo"].shape == (3, 128) and e["stereo"].dtype == a.dtype and e["stereo"].device == a.device
        assert torch.equal(a, before)
        got[name] = e["stereo"]
        err = float((got[name].double() - ref).abs().max())
        report("embeds", name, err, d32, float(ref.abs().max()))
        assert err <= BAR_FACTOR * d32
    # peak="batch" couples the items: halving item 0 moves item 1, by what the float64 restatement says (held to the bar above)
    ref_move = float((fam["stereo_batch_item0-halved"][2][1] - fam["stereo_batch"][2][1]).abs().max())
    assert ref_move > 100 * BAR_FACTOR * d32 and not torch.equal(got["stereo_batch_item0-halved"][1], got["stereo_batch"][1])
    # peak="item" does not: item 1 keeps its bits
    assert torch.equal(got["stereo_item_item0-halved"][1:], got["stereo_item"][1:])
    # mono == stereo with L = R, and a float64 input gets float64 back
    x = fam["stereo_batch"][0]
    lr = x[:, :1].repeat(1, 2, 1)
    assert torch.equal(get_fx_encoder_embeds(lr, model, 48000)["stereo"], got["mono_batch"])
    assert get_fx_encoder_embeds(x[:1].double().to(dev), model, 44100)["stereo"].dtype == torch.float64
    with pytest.raises(ValueError):
        get_fx_encoder_embeds(x, model, 48000, peak="none")


# ----------------------------------------------------------- ES integration ----------------------------------------------------------- #
def test_run_es_with_the_fx_encoder(dev):
    from st_ito import effects as E
    from st_ito.audio_io import resample
    from st_ito.style_transfer import run_es
    from st_ito.utils import get_fx_encoder_embeds, make_synthetic_fx_encoder
    model = make_synthetic_fx_encoder(5, **MIDDLE)
    g = torch.Generator().manual_seed(21)
    x, tgt = 0.5 * torch.randn(1, 2, 16384, generator=g), 0.2 * torch.randn(1, 2, 16384, generator=g)
    res = run_es(x, tgt, 48000, E.make_plugins("eq"), model, get_fx_encoder_embeds, max_iters=2, popsize=4, find_w0=False, sigma0=0.33,
                 seed=3, early_stop=False)
    assert {"output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "num_evals"} <= set(res)
    assert np.isfinite(res["fopt"]) and -1.0 <= res["fopt"] <= 1.0 and len(res["wopt"]) == 18 and len(res["fval_history"]) >= 1
    assert float(tgt.abs().max()) == 1.0   # run_es peak-normalised the target in place
    fresh = make_synthetic_fx_encoder(5, **MIDDLE)
    r = resample(tgt.to(dev), 48000, 44100)
    assert torch.equal(get_fx_encoder_embeds(tgt, model, 48000)["stereo"], fresh(r / r.abs().max().clamp(1e-8)).cpu())
