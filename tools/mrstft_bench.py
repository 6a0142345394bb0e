#!/usr/bin/env python
"""Timing of the multi-resolution STFT objective at the bench shape (256 candidates x stereo x 262144 samples, the
general-pb chain of scripts/eval_pst.py), medians of --reps calls after warm-up:
  (a) stito_mrstft_loss alone (HIP events), and the target table's build;
  (b) the whole evaluate step with this objective next to the cosine / AFx-Rep step of the same process (wall time
      around a final synchronise);
  (c) the composition that was possible before the kernel: render_population + normalize_audio_ +
      scripts/eval_synthetic.mrstft_error (torch.stft on the GPU) over the population, in the largest chunks that fit
      memory -- which yields one mean per chunk; per candidate (what an objective needs) it is one call per candidate.
    python tools/mrstft_bench.py [--pop 256] [--reps 20] [--out profiles/mrstft_objective.txt]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))
sys.path.insert(0, os.path.join(ROOT, "st-ito_amd", "scripts"))
import numpy as np
import torch


def events_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import eval_pst
    import eval_synthetic as S
    from st_ito import engine
    from st_ito.features import MrstftTarget
    from st_ito.style_transfer import load_plugins, process_audio
    from st_ito.utils import get_param_embeds, make_synthetic_param_model

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with contextlib.redirect_stdout(io.StringIO()):
        plugins, D, _ = load_plugins(eval_pst.get_plugins("general-pb"))
    g = torch.Generator().manual_seed(0)
    t = torch.arange(a.n, dtype=torch.float64) / 48000.0
    left = 0.1 * torch.randn(a.n, generator=g, dtype=torch.float64) + 0.2 * torch.sin(2 * np.pi * 110 * t) + 0.1 * torch.sin(2 * np.pi * 440 * t)
    x = torch.stack([left, 0.7 * left + 0.03 * torch.randn(a.n, generator=g, dtype=torch.float64)]).to(torch.float32)
    x /= x.abs().max()
    rng = np.random.default_rng(0)
    target = torch.from_numpy(process_audio(x.numpy(), rng.random(D), 48000, plugins))[None]
    W = rng.random((a.pop, D))
    say(f"# tools/mrstft_bench.py: pop {a.pop}, stereo, {a.n} samples, general-pb chain (D = {D}), median [min .. max] of {a.reps} calls, "
        f"{torch.cuda.get_device_name(0)}")

    # (a) the kernel alone
    xd, Wd = x.to(dev), torch.from_numpy(W).to(dev)
    audio, peaks = engine.render_population(plugins, xd, Wd, 48000)
    tgt = MrstftTarget(target.to(dev))
    tgt.loss(audio, peaks, 1)
    torch.cuda.synchronize()
    ms = events_ms(lambda: tgt.loss(audio, peaks, 1), a.reps)
    rows = a.pop * audio.shape[1]
    say(f"(a) stito_mrstft_loss alone (3 resolution launches + the sum): {ms[0]:.3f} ms [{ms[1]:.3f} .. {ms[2]:.3f}]  "
        f"= {ms[0] * 1e3 / rows:.2f} us per (candidate, channel) row; audio {audio.numel() * 4 / 1e6:.0f} MB, table {tgt.table.numel() * 4 / 1e6:.1f} MB")
    ms = events_ms(lambda: tgt.update(target.to(dev)), a.reps)
    say(f"    stito_mrstft_target ({audio.shape[1]} rows): {ms[0]:.3f} ms [{ms[1]:.3f} .. {ms[2]:.3f}]")

    # (b) the evaluate step, both objectives
    ev = engine.MrstftEvaluator(x[None], 48000, plugins, target)
    ev.evaluate(W)
    ms_m = wall_ms(lambda: ev.evaluate(W)[0], a.reps)
    say(f"(b) evaluate step, MRSTFT objective (render + loss): {ms_m[0]:.2f} ms [{ms_m[1]:.2f} .. {ms_m[2]:.2f}]")
    model = make_synthetic_param_model(seed=0).to(dev)
    te = get_param_embeds(target.clone(), model, 48000)
    pe = engine.PopulationEvaluator(x[None], 48000, plugins, model, te, use_graph=False)
    pe.evaluate(W)
    ms_c = wall_ms(lambda: pe.evaluate(W)[0], a.reps)
    say(f"    evaluate step, cosine / AFx-Rep objective (render + log-mel + Cnn14 + loss, eager): {ms_c[0]:.2f} ms [{ms_c[1]:.2f} .. {ms_c[2]:.2f}]"
        f"  -> ratio {ms_c[0] / ms_m[0]:.2f}")
    ms_r = wall_ms(lambda: engine.render_population(plugins, xd, Wd, 48000), a.reps)
    say(f"    render_population alone: {ms_r[0]:.2f} ms [{ms_r[1]:.2f} .. {ms_r[2]:.2f}]")

    # (c) the composition on torch.stft
    td = target.to(dev)
    reps_c = max(3, a.reps // 4)

    def score(au, chunk):
        return [S.mrstft_error(au[p:p + chunk], td.expand(min(chunk, a.pop - p), -1, -1)) for p in range(0, a.pop, chunk)]

    def compose(chunk):
        return score(engine.normalize_audio_(*engine.render_population(plugins, xd, Wd, 48000)), chunk)

    au = engine.normalize_audio_(*engine.render_population(plugins, xd, Wd, 48000))
    chunk = None
    for c in (a.pop, 128, 64, 32, 16, 8, 4, 2, 1):
        if c > a.pop:
            continue
        try:
            score(au, c)
            torch.cuda.synchronize()
            chunk = c
            break
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
    ms_s = wall_ms(lambda: score(au, chunk), reps_c)
    say(f"(c) scripts/eval_synthetic.mrstft_error (float32 torch.stft on the GPU) over the normalised population, chunks of {chunk} "
        f"(one mean per chunk): {ms_s[0]:.2f} ms [{ms_s[1]:.2f} .. {ms_s[2]:.2f}] of {reps_c} calls")
    ms_1 = wall_ms(lambda: score(au, 1), reps_c)
    say(f"    the same, one call per candidate (per-candidate values, what an objective needs): {ms_1[0]:.2f} ms [{ms_1[1]:.2f} .. {ms_1[2]:.2f}]")
    ms_w = wall_ms(lambda: compose(chunk), reps_c)
    say(f"    whole composition render_population + normalize_audio_ + scoring in chunks of {chunk}: {ms_w[0]:.2f} ms [{ms_w[1]:.2f} .. {ms_w[2]:.2f}]")
    got = tgt.loss(*engine.render_population(plugins, xd, Wd, 48000), 1)
    ref = torch.stack(score(au, 1))
    say(f"    same numbers: max |fused - torch.stft| / torch.stft over the population = {float(((got - ref).abs() / ref.abs()).max()):.2e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
