"""GPU: edge cases and full-size properties of the hot path -- error behaviour of the C ABI as the
Python layer surfaces it (same exception types as the reference), ragged/short inputs, and the
BASELINE.json sizes checked through size-independent properties."""
import os

import numpy as np
import pytest
import torch

import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def pm(dev):
    from st_ito.utils import make_synthetic_param_model
    return make_synthetic_param_model(0)


def test_error_paths(dev, pm):
    from st_ito import effects as E, engine, _hip
    from st_ito.utils import get_param_embeds
    pp = E.make_plugins("eq-comp")
    x = O.synth_audio(1, 2, 20000).to(dev)
    W = torch.rand(3, 22, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):                      # wrong parameter-vector length
        engine.render_population(pp, x, W[:, :21], SR)
    with pytest.raises(ValueError):                      # empty population
        engine.render_population(pp, x, W[:0], SR)
    with pytest.raises(ValueError):                      # 3 channels (panns.py:219-228 "Invalid number of channels")
        pm(torch.zeros(1, 3, 70000))
    with pytest.raises(ValueError):                      # too short for five 2x2 poolings (torch raises in avg_pool2d)
        get_param_embeds(O.synth_audio(2, 2, 8000)[None], pm, SR)
    lib = _hip.lib()
    assert lib.stito_conv3x3_supported(4, 16, 16, 12, 64, 0, 0) == 0   # cin not a multiple of the K chunk
    rc = lib.stito_conv3x3_bn_relu(None, None, None, None, None, 4, 16, 16, 12, 64, 0, 0, None)
    assert rc != 0 and len(lib.stito_last_error()) > 0                  # status code + message, no crash
    # the hoisted-transform algorithm on a shape it does not cover (cout not a multiple of 256): refused before any launch
    rc = lib.stito_conv3x3_bn_relu_ws(None, None, None, None, None, 4, 16, 16, 64, 64, 0, 3, None, 0, None)
    assert rc == _hip.E_UNSUPPORTED and b"256" in lib.stito_last_error()
    # reverb declared mono is a spec error like the reference's channel handling (run_optim.py:401-406)
    bad = E.make_plugins([("Reverb", E.BasicReverb, 1)])
    with pytest.raises(ValueError):
        engine.render_population(bad, x[:1], torch.rand(1, 4, dtype=torch.float64, device=dev), SR)


def test_part_populations_into_one_buffer_on_two_streams_are_the_single_call(dev):
    """render_population(out=): two half populations rendered into slices of one buffer, each on its own HIP stream with the
    workspace allocated per call on that stream (what tools/render_split_bench.py times), give bitwise the audio and peaks of one call."""
    from st_ito import effects as E, engine
    pp = E.make_plugins("bench5")
    chain = engine.compile_chain(pp, False)
    x = O.synth_audio(5, 2, 70001).to(dev)
    W = torch.from_numpy(np.random.default_rng(3).random((6, chain[1]))).to(dev)
    ref_a, ref_p = engine.render_population(pp, x, W, SR, chain=chain)
    audio, peaks = torch.zeros_like(ref_a), torch.zeros_like(ref_p)
    main = torch.cuda.current_stream(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for i, (p0, p1) in enumerate(((0, 2), (2, 6))):
        streams[i].wait_stream(main)
        with torch.cuda.stream(streams[i]):
            engine.render_population(pp, x, W[p0:p1], SR, chain=chain, out=(audio[p0:p1], peaks[p0:p1]))
    for s in streams:
        main.wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(audio, ref_a) and torch.equal(peaks, ref_p)
    with pytest.raises(AssertionError):                  # a buffer of the wrong shape is refused
        engine.render_population(pp, x, W, SR, chain=chain, out=(audio[:3], peaks[:3]))


def test_short_and_ragged_lengths(dev):
    """Lengths that are not multiples of any tile (scalar fallbacks), shorter than one reverb tile,
    and a single sample."""
    from st_ito import effects as E, engine
    kinds = ["ParametricEQ", "Compressor", "Distortion", "Delay", "Reverb"]
    op = O.make_plugins(kinds)
    pp = E.make_plugins("basic")
    rng = np.random.default_rng(5)
    for n in (1, 7, 191, 4097):
        x = (0.5 * rng.standard_normal((2, n))).astype(np.float32)
        W = rng.random((2, 31))
        got, peaks = engine.render_population(pp, torch.from_numpy(x).to(dev), torch.from_numpy(W).to(dev), SR)
        for p in range(2):
            widx, y = 0, x
            for name, plugin in op.items():
                for pn in plugin["parameter_names"]:
                    plugin["instance"].parameters[pn].raw_value = W[p][widx]; widx += 1
                if plugin["num_channels"] == 1:
                    y = np.concatenate((plugin["instance"].process(y[0:1], SR), plugin["instance"].process(y[1:2], SR)), 0)
                else:
                    y = plugin["instance"].process(y, SR)
            # five effects in series on full-scale white noise (compressor -> up to +48 dB tanh drive): 1e-4 of peak
            np.testing.assert_allclose(got[p].cpu().numpy(), y, rtol=0, atol=1e-4 * max(1.0, np.abs(y).max()))
            assert abs(peaks[p].item() - np.abs(y).max()) <= 1e-4 * max(1.0, np.abs(y).max())


def test_full_size_config1_properties(dev, pm):
    """BASELINE.json configs[1] at full size (pop 256, 10 s stereo, 5-effect chain) through
    size-independent properties: candidates evaluated inside the full batch are bitwise the ones
    evaluated alone; normalised audio peaks at exactly 1; losses are finite cosines; an identity
    chain setting (0 dB EQs, ratio-1 compressor, dry reverb, 0 dB gain) returns the input."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds
    n, P = 480000, 256
    x = O.synth_audio(1234, 2, n)[None]
    tgt = O.synth_audio(4321, 2, n)[None]
    pp = E.make_plugins("bench5")
    ev = PopulationEvaluator(x, SR, pp, pm, get_param_embeds(tgt, pm, SR))
    W = np.random.default_rng(2025).random((P, 45))
    # identity candidate: raw values of the defaults, but compressor ratio 1, reverb wet 0 (dry 1), gain 0 dB
    ident = np.array([p.raw_value for pl in pp.values() for p in pl["instance"].parameters.values()])
    ident[18 + 1] = 0.0          # ratio -> 1
    ident[22 + 2] = 0.0          # wet_dry -> 0 (dry level 1 -> JUCE dry gain 2: see below)
    W[0] = ident
    loss, emb, audio = ev.evaluate(W, want_audio=True)
    lossn = loss.cpu().numpy()
    assert lossn.shape == (P,) and np.isfinite(lossn).all() and (np.abs(lossn) <= 1.0001).all()
    pk = audio.abs().amax(dim=(1, 2)).cpu().numpy()
    np.testing.assert_array_equal(pk, np.ones(P, np.float32))           # x / max|x| peaks at exactly 1
    # dry-only Freeverb scales by dry*2 = 2 (juce::Reverb dryScaleFactor); after peak normalisation: the input
    xin = x[0] / x[0].abs().max()
    assert (audio[0].cpu() - xin).abs().max().item() < 2e-6
    for idx in (1, 100, 255):
        l1, e1, _ = ev.evaluate(W[idx:idx + 1])
        assert l1.item() == lossn[idx]
        assert torch.equal(e1["mid"][0], emb["mid"][idx]) and torch.equal(e1["side"][0], emb["side"][idx])


def test_full_size_config3_per_gpu_share_properties(dev, pm):
    """BASELINE.json configs[3]: one GPU's share of the 8-GPU job (pop 2048 sharded 256 per GPU, 48 kHz stereo 30 s,
    T = 1407 frames) at full size through size-independent properties: finite cosine losses, normalised audio peaks at
    exactly 1, and three candidates of the batch are bitwise the ones evaluated alone (so the share a rank computes does
    not depend on what else is in its batch -- the property the sharding relies on)."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds
    n, P = 1440000, 256
    x = O.synth_audio(1234, 2, n)[None]
    tgt = O.synth_audio(4321, 2, n)[None]
    ev = PopulationEvaluator(x, SR, E.make_plugins("bench5"), pm, get_param_embeds(tgt, pm, SR))
    W = np.random.default_rng(2026).random((P, 45))
    loss, emb, audio = ev.evaluate(W, want_audio=True)
    lossn = loss.cpu().numpy()
    assert lossn.shape == (P,) and np.isfinite(lossn).all() and (np.abs(lossn) <= 1.0001).all()
    assert audio.shape == (P, 2, n)
    pk = audio.abs().amax(dim=(1, 2)).cpu().numpy()
    np.testing.assert_array_equal(pk, np.ones(P, np.float32))
    del audio
    for idx in (0, 131, 255):
        l1, e1, _ = ev.evaluate(W[idx:idx + 1])
        assert l1.item() == lossn[idx]
        assert torch.equal(e1["mid"][0], emb["mid"][idx]) and torch.equal(e1["side"][0], emb["side"][idx])


def test_get_param_embeds_normalises_the_callers_tensor_like_the_reference(dev, pm):
    """reference utils.py:457, 473-474: `x.type_as(model parameter)` is x itself when dtype and device type already match
    and no resampling happens, so the per-item peak normalisation lands in the CALLER's tensor.  The HIP model always
    lives on the GPU; `model.reference_device` says where the reference's model would live."""
    from st_ito.utils import get_param_embeds
    x0 = 0.3 * O.synth_audio(5, 2, 50000)[None].repeat(2, 1, 1)
    x0[1] *= 0.5
    want = x0.clone()
    for b in range(2):
        want[b] /= want[b].abs().max().clamp(1e-8)
    # a model built directly lives on the GPU: a CPU tensor is copied by the reference (untouched) ...
    assert getattr(pm, "reference_device", None) in (None, "cuda")
    pm.reference_device = "cuda"
    x = x0.clone()
    e_cpu = get_param_embeds(x, pm, SR)
    assert torch.equal(x, x0)
    # ... a float32 GPU tensor is normalised in place
    xg = x0.clone().to(dev)
    e_gpu = get_param_embeds(xg, pm, SR)
    assert torch.equal(xg.cpu(), want)
    assert torch.equal(e_gpu["mid"].cpu(), e_cpu["mid"])
    # the model load_param_model(use_gpu=False) returns stands for a CPU model: the CPU tensor is normalised in place
    pm.reference_device = "cpu"
    try:
        x = x0.clone()
        e2 = get_param_embeds(x, pm, SR)
        assert torch.equal(x, want) and torch.equal(e2["mid"], e_cpu["mid"])
        xd = x0.clone().double()      # dtype change -> copy -> untouched
        get_param_embeds(xd, pm, SR)
        assert torch.equal(xd, x0.double())
        x441 = x0.clone()             # resampled -> copy -> untouched
        get_param_embeds(x441, pm, 44100)
        assert torch.equal(x441, x0)
    finally:
        pm.reference_device = "cuda"


def test_get_param_embeds_takes_an_expanded_view(dev, pm):
    """An expanded (stride-0) batch cannot be divided in place (torch raises): the embeddings still come back and equal
    those of the materialised batch; make_synthetic_param_model records reference_device like load_param_model does."""
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    assert make_synthetic_param_model(1).reference_device == "cuda"
    one = (0.4 * O.synth_audio(9, 2, 48000)[None]).to(dev)
    view = one.expand(3, -1, -1)
    e_view = get_param_embeds(view, pm, SR)
    e_full = get_param_embeds(view.clone(), pm, SR)
    assert torch.equal(e_view["mid"], e_full["mid"]) and torch.equal(e_view["side"], e_full["side"])


def test_dropout_leaves_the_content_entries_alone(dev, pm):
    """style_transfer.py:545-568: F.dropout hits the style embeddings only; the content embeddings are scored undropped with
    weight 2.  Generic-metric path with a fake embed_func whose style and content entries are the same vectors: with the same
    RNG state the fitness is (-cos(drop(e), t) + 2 (-cos(e, t))) / 2."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    P, dim = 5, 96
    g = torch.Generator().manual_seed(3)
    emb = torch.randn((P, dim), generator=g).to(dev)
    tgt = torch.randn((1, dim), generator=g).to(dev)

    def fake(x, m, sr):
        return {"a": emb[: x.shape[0]], "__content__:a": emb[: x.shape[0]]}

    x = O.synth_audio(4, 2, 30000)[None]
    x /= x.abs().max()
    ev = PopulationEvaluator(x, SR, E.make_plugins("eq"), pm, {"a": tgt, "__content__:a": tgt}, embed_func=fake,
                             entry_weights={"__content__:a": 2.0})
    W = np.random.default_rng(0).random((P, ev.ndims))
    torch.manual_seed(11)
    got = ev.evaluate(W, dropout=0.5)[0].cpu()
    torch.manual_seed(11)
    ed = torch.nn.functional.dropout(emb, p=0.5, training=True)
    cos = torch.nn.functional.cosine_similarity
    want = (-cos(ed, tgt.expand(P, -1)) - 2.0 * cos(emb, tgt.expand(P, -1))).cpu() / 2.0
    assert torch.allclose(got, want, atol=2e-6), (got, want)


def test_parallel_flag_keeps_the_reference_length_policy(dev):
    """reference style_transfer.py:499-502: with parallel=True the pool renders x as it is -- no zero padding to 262144
    samples, no crop -- so a short input is evaluated on its own length.  Serial branch: padded (517-518)."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds
    from st_ito.models.panns import Cnn14
    om = O.make_synthetic_model(0)
    pm = Cnn14(512, SR, 2048, 1024, 128, 20, 20000, True, "minmax")   # the oracle model's weights
    pm.load_state_dict(om.state_dict())
    pm.eval().to(dev)
    n = 60000
    x = O.synth_audio(21, 2, n)[None]
    tgt = O.synth_audio(22, 2, n)[None]
    kinds = ["ParametricEQ", "Compressor"]
    op = O.make_plugins(kinds)
    W = np.random.default_rng(3).random((3, 22))
    ev = PopulationEvaluator(x, SR, E.make_plugins("eq-comp"), pm, get_param_embeds(tgt.clone(), pm, SR))
    l_par, _, a_par = ev.evaluate(W, parallel=True, want_audio=True)
    l_ser, _, a_ser = ev.evaluate(W, parallel=False, want_audio=True)
    assert a_par.shape[-1] == n and a_ser.shape[-1] == 262144
    te_ref = O.get_param_embeds(tgt.clone(), om, SR)
    f_ser, _, _ = O.evaluate(list(W), x, SR, op, te_ref, om)                    # the oracle's serial branch pads
    audios = torch.stack([torch.from_numpy(O.process_audio(x[0].numpy(), w, SR, op)) for w in W])
    emb = O.get_param_embeds(audios, om, SR)                                     # the pool branch: no padding
    f_par = np.mean([(-torch.cosine_similarity(emb[k], te_ref[k], dim=-1)).numpy() for k in emb], axis=0)
    assert np.abs(l_ser.cpu().numpy() - np.array(f_ser)).max() < 1e-4
    assert np.abs(l_par.cpu().numpy() - f_par).max() < 1e-4
    assert np.abs(l_par.cpu().numpy() - l_ser.cpu().numpy()).max() > 1e-5        # the two policies do differ on a short input


def test_config3_length_30s(dev, pm):
    """BASELINE.json configs[3] per-candidate shape (48 kHz stereo 30 s, T = 1407 frames): the
    whole path runs at that length and agrees with the oracle on one candidate."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.models.panns import Cnn14
    from st_ito.utils import get_param_embeds
    n = 1440000
    om = O.make_synthetic_model(0)
    x = O.synth_audio(77, 2, n)[None]
    tgt = O.synth_audio(78, 2, n)[None]
    kinds = ["ParametricEQ", "Compressor", "Reverb", "ParametricEQ", "Gain"]
    W = np.random.default_rng(6).random((2, 45))
    te = get_param_embeds(tgt, pm, SR)
    loss, _, _ = PopulationEvaluator(x, SR, E.make_plugins("bench5"), pm, te).evaluate(W)
    te_ref = O.get_param_embeds(tgt.clone(), om, SR)
    f_ref, _, _ = O.evaluate([W[0]], x, SR, O.make_plugins(kinds), te_ref, om)
    assert abs(loss[0].item() - f_ref[0]) < 1e-4 * max(1.0, abs(f_ref[0]))
    assert np.isfinite(loss.cpu().numpy()).all()


def test_resample_front_door_vs_oracle(dev, pm):
    """utils.py:462-463: get_param_embeds resamples to 48 kHz when handed another rate (the README path with 44.1 kHz
    files).  stito_resample_sinc against the oracle's restatement of torchaudio.functional.resample (library defaults)
    on 44.1k -> 48k, 48k -> 44.1k, 96k -> 48k and an awkward ratio; then the embeddings of 44.1 kHz audio against the
    oracle's get_param_embeds at the same rate."""
    from st_ito.audio_io import resample
    from st_ito.utils import get_param_embeds
    g = torch.Generator().manual_seed(0)
    for o, n_, length in ((44100, 48000, 44100), (48000, 44100, 50001), (96000, 48000, 30000), (22050, 48000, 7777), (44100, 48000, 1)):
        x = torch.randn(2, 2, length, generator=g)
        got = resample(x, o, n_)
        ref = O.resample_sinc(x, o, n_)
        assert got.shape == ref.shape and got.device == x.device
        assert (got - ref).abs().max().item() < 2e-6 * max(1.0, ref.abs().max().item()), (o, n_)
    assert resample(x, 48000, 48000) is x
    gpu_in = resample(x.to(dev), 44100, 48000)
    assert gpu_in.is_cuda                                  # stays on the caller's device
    om = O.make_synthetic_model(0)
    pm2 = type(pm)(512, SR, 2048, 1024, 128, 20, 20000, True, "minmax")
    pm2.load_state_dict(om.state_dict())
    pm2.eval().to(dev)
    a = O.synth_audio(3, 2, 88200)[None]
    e = get_param_embeds(a.clone(), pm2, 44100)
    e_ref = O.get_param_embeds(a.clone(), om, 44100)
    for k in ("mid", "side"):
        assert (e[k] - e_ref[k]).abs().max() / e_ref[k].abs().max() < 1e-4


@pytest.mark.parametrize("split", ["0", "1"])
def test_freeverb_tile_and_ring_edges_vs_oracle(dev, split, monkeypatch):
    """(Both forms of the kernel: one workgroup per candidate, STITO_REVERB_SPLIT=0, and one per (candidate, channel) + the mix pass,
    = 1, which small populations take by default.)  k_reverb's round-5 structure at its seams: signal lengths around the 192-sample tile and the four-tile staging ring (the tile
    count is padded to whole turns of the ring; the ring is loaded by inline-asm loads with hand-counted waits; samples past the
    end are zeroed where the ring is consumed), comb lines whose runs cross the end of the circular buffer (junk / mirror padding:
    room size 1 keeps every comb busy for the whole signal), both delay-line geometries (48 kHz and 44.1 kHz), mono and stereo
    input: every render within the reverb's 2e-5 bar of the oracle (measured 3e-7)."""
    from st_ito import effects as E, engine
    monkeypatch.setenv("STITO_REVERB_SPLIT", split)
    rng = np.random.default_rng(0)
    worst = 0.0
    for sr in (48000, 44100):
        for n in (1, 5, 191, 192, 193, 767, 768, 769, 1537, 4099, 30011):
            for chs in (1, 2):
                x = (0.5 * rng.standard_normal((chs, n))).astype(np.float32)
                op = O.make_plugins(["Reverb"])
                pp = E.make_plugins([("Reverb", E.BasicReverb, 2)])
                W = rng.random((3, 4))
                W[0] = [1.0, 0.0, 1.0, 1.0]
                W[1] = [0.0, 1.0, 0.0, 0.0]
                audio, peaks = engine.render_population(pp, torch.from_numpy(x).to(dev), torch.from_numpy(W).to(dev), sr)
                got = engine.normalize_audio_(audio, peaks).cpu().numpy()
                for p in range(3):
                    err = np.abs(got[p] - O.process_audio(x.copy(), W[p], sr, op)).max()
                    worst = max(worst, err)
                    assert err < 2e-5, (sr, n, chs, p, err)
    print(f"reverb edge sweep: worst |err| {worst:.2e} of peak")


def test_freeverb_per_channel_workgroups_are_bitwise_the_one_workgroup_kernel(dev, monkeypatch):
    """Round 6 (VERDICT r5 next #4b): a small population runs Freeverb as TWO workgroups per candidate -- each channel's eight combs
    and all-pass chain on its own CU, the wet / dry mix in a pointwise pass with the same two fused multiply-adds -- and must get the
    bits of the one-workgroup kernel a large population runs: a candidate's audio (and fitness) may not depend on the batch it is
    evaluated in.  Reverb first in the chain (shared input), behind a mono stage (up-mixed input, in place), mono and stereo input,
    lengths around the tile / ring seams, 48 kHz and 44.1 kHz geometries."""
    from st_ito import effects as E, engine
    rng = np.random.default_rng(3)
    chains = {"reverb": [("Reverb", E.BasicReverb, 2)],
              "comp+reverb+gain": [("Compressor", E.BasicCompressor, 1), ("Reverb", E.BasicReverb, 2), ("Gain", E.BasicGain, 1)],
              "bench5": "bench5"}
    for name, spec in chains.items():
        for sr in (48000, 44100):
            for n, chs in ((1, 1), (193, 2), (769, 1), (4099, 2), (100003, 2)):
                x = torch.from_numpy((0.5 * rng.standard_normal((chs, n))).astype(np.float32)).to(dev)
                pp = E.make_plugins(spec)
                D = sum(p["num_params"] for p in pp.values())
                W = torch.from_numpy(rng.random((5, D))).to(dev)
                outs = {}
                for split in ("0", "1"):
                    monkeypatch.setenv("STITO_REVERB_SPLIT", split)
                    audio, peaks = engine.render_population(pp, x, W, sr)
                    outs[split] = (audio.clone(), peaks.clone())
                assert torch.isfinite(outs["0"][0]).all()
                assert torch.equal(outs["0"][0], outs["1"][0]) and torch.equal(outs["0"][1], outs["1"][1]), (name, sr, n, chs)
