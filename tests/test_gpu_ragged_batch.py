"""GPU: the ragged multi-pair batch -- stito_gather_crops against torch slicing, the list form of run_es_batch against run_es
on every pair alone (bit for bit), the evaluator's subset path, and the PST harness on pairs of unequal length."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
CROP = 262144
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()
    return torch.device("cuda", 0)


def _expected_crop(x: torch.Tensor, start: int, crop_len: int) -> torch.Tensor:
    """torch slicing + zero padding: samples [start, start + crop_len) of (chs, n), zeros past the end."""
    part = x[:, start:start + crop_len]
    return torch.nn.functional.pad(part, (0, crop_len - part.shape[-1]))


@pytest.mark.parametrize("chs", [1, 2])
@pytest.mark.parametrize("crop_len", [1000, CROP])
def test_gather_crops_equals_torch_slicing_bit_for_bit(dev, chs, crop_len):
    from st_ito.engine import RaggedInputs
    g = torch.Generator().manual_seed(100 * chs + crop_len % 97)
    # lengths below / equal to / above crop_len -- odd ones too, so that channel 1 of a pair starts off a 16-byte boundary
    lengths = [crop_len // 3, crop_len - 1, crop_len, crop_len + 5, crop_len + 4096, 2 * crop_len + 37, crop_len + 1024]
    xs = [torch.randn(chs, n, generator=g) for n in lengths]
    ri = RaggedInputs(xs, dev)
    tail = lambda b: max(0, lengths[b] - crop_len)   # noqa: E731  (start = length - crop_len: the last full crop)
    cases = [
        (list(range(len(xs))), [0] * len(xs)),                                            # everything at 0
        (list(range(len(xs))), [tail(b) for b in range(len(xs))]),                         # length - crop_len
        ([5, 3, 6], [3, 1, 777]),                                                          # odd starts; strict subset, out of order
        ([6, 0, 4, 2], [1024, 0, 4096, 0]),                                                # aligned starts, subset, out of order
        ([5, 1], [crop_len + 100, 0]),                                                     # a crop that runs off the end
        ([4], [4095]),
    ]
    for pairs, starts in cases:
        out = ri.gather(pairs, starts, crop_len)
        assert out.shape == (len(pairs), chs, crop_len) and out.dtype == torch.float32 and out.is_contiguous()
        want = torch.stack([_expected_crop(xs[b], s, crop_len) for b, s in zip(pairs, starts)])
        assert torch.equal(out.cpu(), want), (pairs, starts)
    first = ri.gather([0, 1], [0, 0], crop_len)
    assert first.data_ptr() == out.data_ptr()            # the buffer is persistent: every call refills the same memory
    assert ri.n_launches == len(cases) + 1
    with pytest.raises(ValueError):
        ri.gather([len(xs)], [0], crop_len)
    with pytest.raises(ValueError):
        ri.gather([0], [lengths[0]], crop_len)
    with pytest.raises(ValueError):
        ri.gather([5, 5], [0, 8], crop_len)       # one start per pair and call


def test_gather_crops_c_abi_guards(dev):
    """The entry point itself: a slot that names no pair and a pair that does not lie inside the packed buffer give zeros
    (nothing outside the buffer is read); bad arguments are refused on the host."""
    from st_ito import _hip
    L = _hip.lib()
    packed = torch.arange(1, 41, dtype=torch.float32, device=dev)                   # two mono inputs: 24 and 16 samples
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)                  # noqa: E731
    off, length, start = i64([0, 24, 30]), i64([24, 16, 16]), i64([2, 1, 0])         # "pair" 2 would run 6 samples past the end
    slots = torch.tensor([1, 7, 2, -1, 0], dtype=torch.int32, device=dev)
    out = torch.full((5, 1, 20), -5.0, device=dev)
    call = lambda n_pairs, n_slots, chs, crop: L.stito_gather_crops(                 # noqa: E731
        _hip.ptr(packed), packed.numel(), _hip.ptr(off), _hip.ptr(length), _hip.ptr(start), n_pairs, _hip.ptr(slots), n_slots, chs,
        crop, _hip.ptr(out), _hip.stream_ptr())
    _hip.check(call(3, 5, 1, 20))
    got = out.cpu()[:, 0]
    want = torch.zeros(5, 20)
    want[0, :15] = torch.arange(26, 41, dtype=torch.float32)
    want[4] = torch.arange(3, 23, dtype=torch.float32)
    assert torch.equal(got, want)
    for bad in ((0, 5, 1, 20), (3, 0, 1, 20), (3, 5, 3, 20), (3, 5, 1, 0)):
        with pytest.raises(ValueError):
            _hip.check(call(*bad))


def _ragged_pairs(lengths, seed0):
    xs = [O.synth_audio(seed0 + b, 2, n)[None] * (0.5 + 0.1 * b) for b, n in enumerate(lengths)]
    ts = [O.synth_audio(seed0 + 50 + b, 2, n - 7000 * (b + 1))[None] * (0.3 + 0.2 * b) for b, n in enumerate(lengths)]
    return xs, ts


def _assert_same_run(got, one):
    np.testing.assert_array_equal(got["wopt"], one["wopt"])
    assert got["fopt"] == one["fopt"] and got["fval_history"] == one["fval_history"]
    assert len(got["wopt_history"]) == len(one["wopt_history"])
    for a, b in zip(got["wopt_history"], one["wopt_history"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got["num_evals"] == one["num_evals"]
    assert torch.equal(got["output_audio"], one["output_audio"])
    assert got["params"] == one["params"]


@pytest.mark.parametrize("random_crop,lengths", [(True, [200000, 270000, 400000]), (False, [300000, 300000, 350000])])
def test_list_form_batch_equals_run_es_on_every_pair_alone(dev, random_crop, lengths):
    """Padded (200000), cropped at 0 (270000: spare <= 16384) and randomly cropped (400000) pairs in one group under
    random_crop; without it {300000, 300000, 350000} make two groups.  run_es is the unchanged single-pair driver."""
    from st_ito import effects as E, engine
    from st_ito.style_transfer import run_es, run_es_batch
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    P, iters, seed = 4, 4, 23
    xs, ts = _ragged_pairs(lengths, 600)
    assert len(engine.plan_ragged_groups(lengths, random_crop)) == (1 if random_crop else 2)
    keep = [(x.clone(), t.clone()) for x, t in zip(xs, ts)]
    res = run_es_batch(xs, ts, SR, E.make_plugins("bench5"), pm, get_param_embeds, max_iters=iters, sigma0=0.33, popsize=P,
                       random_crop=random_crop, seed=seed, early_stop=False)
    assert len(res) == len(lengths)
    for (x0, t0), x, t in zip(keep, xs, ts):         # the caller's tensors are not modified
        assert torch.equal(x0, x) and torch.equal(t0, t)
    for b in range(len(lengths)):
        one = run_es(xs[b].clone(), ts[b].clone(), SR, E.make_plugins("bench5"), pm, get_param_embeds, max_iters=iters, popsize=P,
                     find_w0=False, sigma0=0.33, random_crop=random_crop, seed=seed + b, early_stop=False)
        _assert_same_run(res[b], one)
        assert res[b]["num_evals"] == iters * P and res[b]["output_audio"].shape[-1] == lengths[b]
    # (chs, n) tensors are accepted as well, with the same results
    res2 = run_es_batch([x[0] for x in xs], [t[0] for t in ts], SR, E.make_plugins("bench5"), pm, get_param_embeds, max_iters=2,
                        sigma0=0.33, popsize=P, random_crop=random_crop, seed=seed, early_stop=False)
    for b in range(len(lengths)):
        assert res2[b]["fval_history"] == res[b]["fval_history"][:2]


def test_list_form_early_stop_equals_run_es(dev, capsys):
    """With the seeded random Cnn14 the candidates of a population differ by about 2e-5 in loss, far below the 0.01 the stop
    rule asks for: every pair goes stale from iteration 1 and stops after iteration 11 (12 evaluated populations)."""
    from st_ito import effects as E
    from st_ito.style_transfer import run_es, run_es_batch
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    P, seed, lengths = 4, 31, [100000, 290000, 120000]
    xs, ts = _ragged_pairs(lengths, 700)
    res = run_es_batch(xs, ts, SR, E.make_plugins("eq-comp"), pm, get_param_embeds, max_iters=16, sigma0=0.33, popsize=P,
                       random_crop=True, seed=seed, early_stop=True)
    for b in range(len(lengths)):
        one = run_es(xs[b].clone(), ts[b].clone(), SR, E.make_plugins("eq-comp"), pm, get_param_embeds, max_iters=16, popsize=P,
                     find_w0=False, sigma0=0.33, random_crop=True, seed=seed + b, early_stop=True)
        print(f"pair {b}: batch num_evals {res[b]['num_evals']}, run_es num_evals {one['num_evals']}, "
              f"spread of the last history {max(one['fval_history'][1:]) - min(one['fval_history'][1:]):.3e}")
        _assert_same_run(res[b], one)
        assert res[b]["num_evals"] == 12 * P          # stale at iterations 1 .. 11 -> stops after iteration 11


def test_evaluator_scores_a_subset_of_its_pairs(dev):
    """evaluate(W_subset, pairs=[2, 0]) returns bit for bit the rows evaluate(W_all) returns for pairs 2 and 0, renders only
    the subset's candidates, and accepts a ready-made (gathered) input buffer."""
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator, RaggedInputs
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    B, P, n = 3, 4, 90000
    xs = torch.stack([O.synth_audio(800 + b, 2, n) for b in range(B)])
    ts = torch.stack([O.synth_audio(850 + b, 2, n) * (0.4 + 0.2 * b) for b in range(B)])
    ev = PopulationEvaluator(xs, SR, E.make_plugins("bench5"), pm, get_param_embeds(ts.clone(), pm, SR), use_graph=False)
    W = np.random.default_rng(8).random((B * P, 45))
    full, emb, _ = ev.evaluate(W)
    assert ev.rendered_candidates == B * P
    Wsub = np.concatenate([W[2 * P:3 * P], W[0:P]])
    sub, emb_sub, _ = ev.evaluate(Wsub, pairs=[2, 0])
    assert ev.rendered_candidates == B * P + 2 * P
    assert torch.equal(sub, torch.cat([full[2 * P:3 * P], full[0:P]]))
    assert torch.equal(emb_sub["mid"], torch.cat([emb["mid"][2 * P:3 * P], emb["mid"][0:P]]))
    one, _, _ = ev.evaluate(W[P:2 * P], pairs=[1])
    assert torch.equal(one, full[P:2 * P]) and ev.rendered_candidates == B * P + 3 * P
    # the same through a gathered buffer (zero padded to 262144 by the kernel, as _input pads)
    ri = RaggedInputs([x for x in xs], dev)
    buf, _, _ = ev.evaluate(Wsub, pairs=[2, 0], x=ri.gather([2, 0], [0, 0], CROP))
    assert torch.equal(buf, sub)
    with pytest.raises(ValueError):
        ev.evaluate(Wsub, pairs=[3, 0])
    with pytest.raises(ValueError):
        ev.evaluate(Wsub, pairs=[2, 0], x=ri.gather([2], [0], CROP))


def test_ragged_batch_pair_against_the_oracle_loop(dev, tmp_path):
    """The pairs and tolerances of test_eval_pst_harness_against_the_oracle_loop (tests/test_gpu_es.py), through
    run_pst_benchmark(batched=True): the two examples differ in length, so they go through the list form.  The long example
    (48 kHz stereo, 300000 samples: the random crop draws a start every iteration) is compared with the oracle's
    run_pst_example: selected vector bit-identical, metrics within 1e-4, written audio within 1e-4 at -22 LUFS."""
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import eval_pst
    from st_ito import cmaes
    from st_ito.audio_io import load_wav
    from st_ito.models.panns import Cnn14
    om = O.make_synthetic_model(0)
    pm = Cnn14(512, SR, 2048, 1024, 128, 20, 20000, True, "minmax")
    pm.load_state_dict(om.state_dict())
    pm = pm.eval().to(dev)
    kinds = ["ParametricEQ", "Compressor", "Reverb"]     # = mastering-pb
    D = sum(p_["num_params"] for p_ in O.make_plugins(kinds).values())

    def target_of(sig, seed):
        w = np.random.default_rng(seed).random(D) * 0.6
        return torch.from_numpy(O.process_audio(sig.numpy(), w, SR, O.make_plugins(kinds)))

    a44 = O.synth_audio(301, 1, 50000, sr=44100)
    pairs = [("short44k", a44, 44100, target_of(O.synth_audio(302, 2, 60000), 1), 48000),
             ("long48k", O.synth_audio(303, 2, 300000), 48000, target_of(O.synth_audio(304, 2, 290000), 2), 48000)]
    kw = dict(max_iters=3, popsize=6, sigma0=0.33, random_crop=True, seed=5)
    got = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins("mastering-pb"), pm, str(tmp_path / "pst"), tag="mastering-pb",
                                     batched=True, **kw)
    es_name = "style-es (param-panns)"
    assert len(got[es_name]["time_elapsed"]) == 2 and got[es_name]["time_elapsed"][0] == got[es_name]["time_elapsed"][1]
    idx = 1
    name, xin, xsr, tg, tsr = pairs[idx]
    ref = O.run_pst_example(xin.clone(), xsr, tg.clone(), tsr, O.make_plugins(kinds, with_bypass=True), om,
                            cmaes.CMAEvolutionStrategy, max_iters=3, popsize=6, sigma0=0.33, random_crop=True, seed=5 + idx)
    params = json.load(open(tmp_path / "pst" / f"{idx:02d}_style-es_mastering-pb.json"))
    ref_params = ref["es"]["params"]
    for plug in ref_params:      # the selected vector, through parameters_to_dict on both sides
        for k, v in ref_params[plug].items():
            assert params[plug][k] == pytest.approx(float(v), rel=0, abs=0), (idx, plug, k)
    print(f"metric {got[es_name]['style_features'][idx]} oracle {ref['metric']}")
    assert abs(got[es_name]["style_features"][idx] - ref["metric"]) < 1e-4
    assert abs(got["input"]["style_features"][idx] - ref["input_metric"]) < 1e-4
    for stem, want in ((f"{idx:02d}_style-es_mastering-pb.wav", ref["audio"]), (f"{idx:02d}_input_mastering-pb.wav", ref["input_audio"]),
                       (f"{idx:02d}_target_mastering-pb.wav", ref["target_audio"])):
        y, sr = load_wav(str(tmp_path / "pst" / stem))
        assert sr == SR and tuple(y.shape) == tuple(want.shape[1:])
        assert np.abs(y.numpy() - want[0].numpy()).max() < 1e-4, stem
        assert abs(O.integrated_loudness(y.numpy().T, sr) - (-22.0)) < 0.01


def test_pst_harness_batched_on_ragged_pairs_equals_sequential(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
    import eval_pst
    from st_ito.utils import make_synthetic_param_model
    pm = make_synthetic_param_model(0)
    chain = "mastering-pb"
    pairs = [eval_pst.synthetic_pairs(1, sec, eval_pst.get_plugins(chain))[0] for sec in (2.0, 6.5, 3.0)]
    pairs = [(f"ragged{i}",) + p[1:] for i, p in enumerate(pairs)]
    assert len({p[1].shape[-1] for p in pairs}) == 3 and max(p[1].shape[-1] for p in pairs) - CROP > 16384
    kw = dict(max_iters=3, popsize=6, random_crop=True, seed=9, tag=chain)
    r_seq = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins(chain), pm, str(tmp_path / "seq"), **kw)
    r_bat = eval_pst.run_pst_benchmark(pairs, eval_pst.get_plugins(chain), pm, str(tmp_path / "bat"), batched=True, **kw)
    es = "style-es (param-panns)"
    assert list(r_bat) == list(r_seq) == ["input", es]
    assert r_seq[es]["style_features"] == r_bat[es]["style_features"] and len(r_bat[es]["style_features"]) == 3
    assert r_seq["input"]["style_features"] == r_bat["input"]["style_features"]
    assert len(set(r_bat[es]["time_elapsed"])) == 1       # wall time of the batch / number of pairs
    for i in range(3):
        assert json.load(open(tmp_path / "seq" / f"{i:02d}_style-es_{chain}.json")) == json.load(open(tmp_path / "bat" / f"{i:02d}_style-es_{chain}.json"))
