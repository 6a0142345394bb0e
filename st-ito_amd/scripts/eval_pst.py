#!/usr/bin/env python
"""Production-style-transfer benchmark harness on the MI355X path -- the ES arm of the reference's
scripts/eval/eval_pst.py (get_plugins 206-650 for the pedalboard chains, run_pst_benchmark 652-903,
method settings 974-991: popsize 128, 32 iterations, sigma0 0.33, find_w0 False, random_crop True).

Differences, all stated: only the `*-pb` chains (Basic* effects) are built -- the VST chains need
binary plugins.  Of the methods (945-991) `input`, `random`, `rule-based` and `style-es` are built
(`--methods`, default `input style-es`); DeepAFx-ST needs a trained checkpoint and its package, which
do not exist here.  The examples come from `--pairs file` (one "input.wav<TAB>target.wav" per line,
relative to --root-dir) or `--synthetic N`; the reference's hard-coded file lists are its own
dataset and are not reproduced.  With `--batched` the examples are optimised together by run_es_batch
(BASELINE.json configs[2]) instead of one after the other: as one tensor when they all have one shape, as
lists (per-pair random crops, one GPU batch per evaluate-time length) when their lengths differ.

    python st-ito_amd/scripts/eval_pst.py --chain general-pb --synthetic 4 --max-iters 8 --popsize 32
    python st-ito_amd/scripts/eval_pst.py --chain general-pb --synthetic 2 --methods input random rule-based style-es
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import OrderedDict
from datetime import datetime

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def get_plugins(chain_type: str):
    """The pedalboard ("-pb") chains of eval_pst.py:269-301, 559-645.  guitar-pb lists
    "ParametricEQ" twice in one dict literal there, so the second entry replaces the first in
    place: the chain really is Compressor, ParametricEQ, Distortion, Reverb."""
    from st_ito.effects import BasicCompressor, BasicDelay, BasicDistortion, BasicParametricEQ, BasicReverb

    one = lambda cls: {"class_path": cls, "num_params": None, "num_channels": 1, "fixed_parameters": {}}
    two = lambda cls: {"class_path": cls, "num_params": None, "num_channels": 2, "fixed_parameters": {}}
    if chain_type == "general-pb":
        return OrderedDict(Distortion=one(BasicDistortion), ParametricEQ=one(BasicParametricEQ),
                           Compressor=one(BasicCompressor), Delay=two(BasicDelay), Reverb=two(BasicReverb))
    elif chain_type == "mastering-pb":
        return OrderedDict(ParametricEQ=one(BasicParametricEQ), Compressor=one(BasicCompressor), Reverb=two(BasicReverb))
    elif chain_type == "vocals-pb":
        return OrderedDict(ParametricEQ=one(BasicParametricEQ), Compressor=one(BasicCompressor),
                           Distortion=one(BasicDistortion), Delay=two(BasicDelay), Reverb=two(BasicReverb))
    elif chain_type == "guitar-pb":
        return OrderedDict(Compressor=one(BasicCompressor), ParametricEQ=one(BasicParametricEQ),
                           Distortion=one(BasicDistortion), Reverb=two(BasicReverb))
    raise ValueError(f"Unknown chain_type: {chain_type}")


def prepare_pair(input_audio: torch.Tensor, input_sr: int, target_audio: torch.Tensor, target_sr: int,
                 fade_samples: int = 32768):
    """eval_pst.py:705-748: resample to 48 kHz, make stereo, add the batch dim, fade in."""
    from st_ito.audio_io import resample
    from st_ito.utils import apply_fade_in

    if input_sr != 48000:
        input_audio = resample(input_audio, input_sr, 48000)
    if target_sr != 48000:
        target_audio = resample(target_audio, target_sr, 48000)
    min_len = min(input_audio.shape[1], target_audio.shape[1], 262144)
    if input_audio.shape[0] == 1:
        input_audio = input_audio.repeat(2, 1)
    if target_audio.shape[0] == 1:
        target_audio = target_audio.repeat(2, 1)
    # apply_fade_in works in place (utils.py:31-43); the caller's tensors are left alone
    return (apply_fade_in(input_audio.unsqueeze(0).clone(), fade_samples),
            apply_fade_in(target_audio.unsqueeze(0).clone(), fade_samples), min_len)


def style_distance(a: torch.Tensor, b: torch.Tensor, model, sr: int) -> float:
    """Mean over {mid, side} of cosine_similarity (the harness reports the similarity itself,
    eval_pst.py:811-836)."""
    from st_ito.utils import get_param_embeds

    ea, eb = get_param_embeds(a, model, sr), get_param_embeds(b, model, sr)
    return float(torch.stack([torch.cosine_similarity(ea[k], eb[k], dim=1) for k in ea]).mean())


def fx_encoder_similarity(a: torch.Tensor, b: torch.Tensor, fx_model, sr: int) -> float:
    """cosine_similarity of the FX-Encoder embeddings, scored like style_distance.  The reference's eval_pst.py imports
    load_fx_encoder_model / get_fx_encoder_embeds (24-25) without listing the encoder among its metrics: this entry is an
    extension.  Each side is embedded on its own, so each is normalised by its own peak."""
    from st_ito.utils import get_fx_encoder_embeds

    ea, eb = get_fx_encoder_embeds(a, fx_model, sr)["stereo"], get_fx_encoder_embeds(b, fx_model, sr)["stereo"]
    return float(torch.cosine_similarity(ea, eb, dim=1).mean())


# --methods choice -> the reference's result key (eval_pst.py:945-991)
METHODS = OrderedDict([("input", "input"), ("random", "random"), ("rule-based", "rule-based"), ("style-es", "style-es (param-panns)")])
DEFAULT_METHODS = ("input", "style-es")


def run_pst_benchmark(pairs, plugins, model, out_dir: str, max_iters: int = 32, popsize: int = 128, sigma0: float = 0.33,
                      random_crop: bool = True, seed: int = None, batched: bool = False, tag: str = "pb",
                      methods=DEFAULT_METHODS, fx_model=None):
    """pairs: list of (name, input (chs, n), input_sr, target (chs, n), target_sr).  Returns the results dict
    the reference dumps to JSON: per method, per metric, one value per example (+ time_elapsed).  fx_model: an FXencoder, or
    None; with one every result is also scored by fx_encoder_similarity under "fx_encoder".

    methods: any of "input", "random", "rule-based", "style-es" (results in that order, under the reference's keys).  Every
    method gets clones of the prepared pair; its time_elapsed is the wall time of its call, like the reference's (757-763;
    the input arm records 0).  Like the reference, only a method that returns "params" (the ES) writes a .json."""
    from st_ito.audio_io import save_wav
    from st_ito.loudness import normalize_loudness
    from st_ito.style_transfer import load_plugins, run_es, run_es_batch, run_random, run_rule_based
    from st_ito.utils import get_param_embeds

    for m in methods:
        if m in ("deepafx-st", "deepafx-st+"):
            raise NotImplementedError(f"method {m!r} needs a trained DeepAFx-ST checkpoint and its package; not built here")
        if m not in METHODS:
            raise ValueError(f"Unknown method {m!r}: choose from {list(METHODS)}")
    methods = [m for m in METHODS if m in methods]
    os.makedirs(out_dir, exist_ok=True)
    plugins, _, _ = load_plugins(plugins)
    sr = 48000
    prepared = [(name,) + prepare_pair(x, xsr, t, tsr) for name, x, xsr, t, tsr in pairs]
    results = {METHODS[m]: {"time_elapsed": [], "style_features": [], **({} if fx_model is None else {"fx_encoder": []})} for m in methods}

    def timed(fn, *a, **k):
        t0 = time.time()
        r = fn(*a, **k)
        return r, time.time() - t0

    es_out = [None] * len(prepared)
    if "style-es" in methods and batched:
        # pairs of one shape go as (B, chs, n) tensors, as before; files of different lengths as lists (per-pair crops, one GPU
        # batch per evaluate-time length)
        same = len({(p[1].shape, p[2].shape) for p in prepared}) == 1 and prepared[0][1].shape == prepared[0][2].shape
        xs, ts = [p[1] for p in prepared], [p[2] for p in prepared]
        t0 = time.time()
        res = run_es_batch(torch.cat(xs) if same else xs, torch.cat(ts) if same else ts, sr, plugins, model,
                           get_param_embeds, max_iters=max_iters, sigma0=sigma0, popsize=popsize, random_crop=random_crop, seed=seed)
        dt = (time.time() - t0) / len(prepared)
        es_out = [(r, dt) for r in res]
    for idx, (name, xin, tgt, min_len) in enumerate(prepared):
        outs = OrderedDict()
        for m in methods:
            if m == "input":
                outs[m] = (xin[0], 0.0, None)
            elif m == "random":
                r, dt = timed(run_random, xin.clone(), tgt.clone(), sr, plugins, None)
                outs[m] = (r["output_audio"][0], dt, None)
            elif m == "rule-based":
                r, dt = timed(run_rule_based, xin.clone(), tgt.clone(), sr, plugins, None)
                outs[m] = (r["output_audio"][0], dt, None)
            else:
                if es_out[idx] is None:
                    es_out[idx] = timed(run_es, xin.clone(), tgt.clone(), sr, plugins, model, get_param_embeds, max_iters=max_iters,
                                        sigma0=sigma0, popsize=popsize, find_w0=False, random_crop=random_crop, distance="cosine",
                                        dropout=0.0, seed=None if seed is None else seed + idx)
                outs[m] = (es_out[idx][0]["output_audio"], es_out[idx][1], es_out[idx][0]["params"])
        for m, (out_audio, elapsed, params) in outs.items():
            method = METHODS[m]
            results[method]["time_elapsed"].append(elapsed)
            results[method]["style_features"].append(style_distance(out_audio[None], tgt, model, sr))
            if fx_model is not None:
                results[method]["fx_encoder"].append(fx_encoder_similarity(out_audio[None], tgt, fx_model, sr))
            stem = f"{idx:02d}_{method.split(' ')[0]}_{tag}"
            if params is not None:
                with open(os.path.join(out_dir, stem + ".json"), "w") as f:
                    json.dump(params, f, indent=2)
            out_audio, _ = normalize_loudness(out_audio[:, :min_len], sr, -22.0)   # eval_pst.py:843-853
            save_wav(os.path.join(out_dir, stem + ".wav"), out_audio, sr)
        tgt_n, _ = normalize_loudness(tgt[0][:, :min_len], sr, -22.0)
        save_wav(os.path.join(out_dir, f"{idx:02d}_target_{tag}.wav"), tgt_n, sr)
    print()
    for method, res in results.items():
        print(f"{method}:\n\tstyle_features: {np.mean(res['style_features'])}")
        if fx_model is not None:
            print(f"\tfx_encoder: {np.mean(res['fx_encoder'])}")
    with open(os.path.join(out_dir, f"results_{datetime.now().strftime('%Y-%m-%d_%H-%M-%S')}.json"), "w") as f:
        json.dump(results, f, indent=2)
    return results


def synthetic_pairs(n: int, seconds: float, plugins):
    """Inputs: seeded noise + tones (the bench's recipe); targets: another signal through the same
    chain at random parameters, so that a perfect match exists in the search space."""
    from st_ito.style_transfer import load_plugins, process_audio
    import copy

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from bench import synth_audio

    pl, D, _ = load_plugins(copy.deepcopy(plugins))
    ns = int(seconds * 48000)
    out = []
    for i in range(n):
        w = np.random.default_rng(100 + i).random(D) * 0.5  # bypass slots stay < 0.5 (they are dead anyway)
        tgt = torch.from_numpy(process_audio(synth_audio(500 + i, 2, ns).numpy(), w, 48000, pl))
        out.append((f"synthetic{i}", synth_audio(400 + i, 2, ns), 48000, tgt, 48000))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chain", default="general-pb", choices=["general-pb", "mastering-pb", "vocals-pb", "guitar-pb"])
    ap.add_argument("--pairs", help="text file: input<TAB>target per line")
    ap.add_argument("--root-dir", default=".")
    ap.add_argument("--synthetic", type=int, default=0, help="use N synthetic pairs instead of files")
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--max-iters", type=int, default=32)
    ap.add_argument("--popsize", type=int, default=128)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--ckpt", default=None, help="AFx-Rep checkpoint; omitted: seeded random weights")
    ap.add_argument("--methods", nargs="+", default=list(DEFAULT_METHODS), choices=list(METHODS) + ["deepafx-st"],
                    help="methods to run (deepafx-st: not built, raises)")
    ap.add_argument("--output-dir", default=os.path.join("output", "pst"))
    ap.add_argument("--metrics", nargs="*", default=[], choices=["fx_encoder"],
                    help="further scores of every result next to style_features; fx_encoder: cosine similarity of FX-Encoder embeddings")
    ap.add_argument("--fx-ckpt", default=None, help="FX-Encoder checkpoint for --metrics fx_encoder; omitted: seeded random weights")
    a = ap.parse_args(argv)

    from st_ito.audio_io import load_wav
    from st_ito.utils import load_fx_encoder_model, load_param_model, make_synthetic_fx_encoder, make_synthetic_param_model

    model = load_param_model(a.ckpt, use_gpu=True) if a.ckpt else make_synthetic_param_model(0)
    fx_model = None
    if "fx_encoder" in a.metrics:
        fx_model = load_fx_encoder_model(use_gpu=True, ckpt_path=a.fx_ckpt) if a.fx_ckpt else make_synthetic_fx_encoder(0)
    plugins = get_plugins(a.chain)
    if a.synthetic:
        pairs = synthetic_pairs(a.synthetic, a.seconds, plugins)
    elif a.pairs:
        pairs = []
        for line in open(a.pairs):
            if line.strip():
                i, t = line.rstrip("\n").split("\t")
                (x, xsr), (y, ysr) = load_wav(os.path.join(a.root_dir, i)), load_wav(os.path.join(a.root_dir, t))
                pairs.append((os.path.basename(i), x, xsr, y, ysr))
    else:
        ap.error("give --pairs or --synthetic N")
    return run_pst_benchmark(pairs, plugins, model, os.path.join(a.output_dir, a.chain), a.max_iters, a.popsize,
                             seed=a.seed, batched=a.batched, tag=a.chain, methods=a.methods, fx_model=fx_model)


if __name__ == "__main__":
    main()
