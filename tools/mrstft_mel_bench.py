#!/usr/bin/env python
"""Timing of the mel-scaled MR-STFT objective next to the linear (L/R) one at the bench shape (256 candidates x stereo x 262144
samples, the general-pb chain of scripts/eval_pst.py), the two alternating call by call in one process, medians of --reps
calls after warm-up:
  (a) stito_mrstft_loss and stito_mrstft_loss_mel alone (HIP events) on the same rendered population, and the two table builds;
  (b) the whole evaluate step (render + loss; wall time around a final synchronise) of MrstftEvaluator and MelMrstftEvaluator;
  (c) where the mel kernel's time goes: the same kernel with every band cut to its first bin (the magnitudes are still written
      back into the FFT buffer and 64 bands a frame still go through the two terms, but the banded dot products are one fma
      each), so (mel - cut) is the band sums and (cut - linear) everything else -- which is negative when the 64 logarithms a
      frame that replace n_fft / 2 + 1 save more than the write-back costs.
--trace runs only the two loss kernels, --reps times each, for a `rocprofv3 --kernel-trace --stats -- python
tools/mrstft_mel_bench.py --trace` run of its own: k_mrstft<false, false, false> is the linear kernel, k_mrstft<false, false,
true> the mel one.
    python tools/mrstft_mel_bench.py [--pop 256] [--reps 20] [--out profiles/mrstft_mel.txt]"""
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


def alternating_ms(fns, reps, wall=False):
    """[(median, min, max)] per function, the functions called in turn reps times: device events around each call, or the host
    clock around a call that ends in a synchronise."""
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            if wall:
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t) * 1e3)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                out[k].append(e0.elapsed_time(e1))
    return [(statistics.median(v), min(v), max(v)) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--trace", action="store_true", help="only the two loss kernels, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import eval_pst
    from st_ito import engine
    from st_ito.features import MelMrstftTarget, MrstftTarget, mel_mrstft_bank
    from st_ito.style_transfer import load_plugins, process_audio

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with contextlib.redirect_stdout(io.StringIO()):
        plugins, D, _ = load_plugins(eval_pst.get_plugins("general-pb"))
    # the input, target and population of tools/mrstft_bench.py
    g = torch.Generator().manual_seed(0)
    t = torch.arange(a.n, dtype=torch.float64) / 48000.0
    left = 0.1 * torch.randn(a.n, generator=g, dtype=torch.float64) + 0.2 * torch.sin(2 * np.pi * 110 * t) + 0.1 * torch.sin(2 * np.pi * 440 * t)
    x = torch.stack([left, 0.7 * left + 0.03 * torch.randn(a.n, generator=g, dtype=torch.float64)]).to(torch.float32)
    x /= x.abs().max()
    rng = np.random.default_rng(0)
    target = torch.from_numpy(process_audio(x.numpy(), rng.random(D), 48000, plugins))[None]
    W = rng.random((a.pop, D))
    say(f"# tools/mrstft_mel_bench.py: pop {a.pop}, stereo, {a.n} samples, general-pb chain (D = {D}), 48 kHz, 64 bands, linear and mel "
        f"alternating call by call, median [min .. max] of {a.reps} calls each, {torch.cuda.get_device_name(0)}")

    xd, Wd, td = x.to(dev), torch.from_numpy(W).to(dev), target.to(dev)
    audio, peaks = engine.render_population(plugins, xd, Wd, 48000)
    bank = mel_mrstft_bank(48000)
    cut = [(s, np.ones_like(n), w[:1].copy()) for s, n, w in bank]          # every band: its first bin only
    lin, mel, short = MrstftTarget(td), MelMrstftTarget(td, bank=bank), MelMrstftTarget(td, bank=cut)
    calls = [lambda: lin.loss(audio, peaks, 1), lambda: mel.loss(audio, peaks, 1)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    if a.trace:
        alternating_ms(calls, a.reps)
        return

    # (a) the kernels alone
    ms_lin, ms_mel = alternating_ms(calls, a.reps)
    rows = a.pop * 2
    say(f"(a) stito_mrstft_loss alone (3 resolution launches + the sum):      {ms_lin[0]:.3f} ms [{ms_lin[1]:.3f} .. {ms_lin[2]:.3f}]  "
        f"= {ms_lin[0] * 1e3 / rows:.2f} us per row")
    say(f"    stito_mrstft_loss_mel alone (the same launches, MEL kernel):    {ms_mel[0]:.3f} ms [{ms_mel[1]:.3f} .. {ms_mel[2]:.3f}]  "
        f"= {ms_mel[0] * 1e3 / rows:.2f} us per row  -> {ms_mel[0] / ms_lin[0]:.3f} x the linear kernel")
    t_lin, t_mel = alternating_ms([lambda: lin.update(td), lambda: mel.update(td)], a.reps)
    say(f"    stito_mrstft_target / stito_mrstft_target_mel (2 rows): {t_lin[0]:.3f} ms [{t_lin[1]:.3f} .. {t_lin[2]:.3f}] / "
        f"{t_mel[0]:.3f} ms [{t_mel[1]:.3f} .. {t_mel[2]:.3f}]; table {lin.table.numel() * 4 / 2 ** 20:.2f} / {mel.table.numel() * 4 / 2 ** 20:.2f} MiB")

    # (b) the evaluate steps
    ev_lin = engine.MrstftEvaluator(x[None], 48000, plugins, target)
    ev_mel = engine.MelMrstftEvaluator(x[None], 48000, plugins, target)
    steps = [lambda: ev_lin.evaluate(W)[0], lambda: ev_mel.evaluate(W)[0]]
    for fn in steps:
        fn()
    e_lin, e_mel = alternating_ms(steps, a.reps, wall=True)
    say(f"(b) evaluate step (render + loss), linear objective: {e_lin[0]:.2f} ms [{e_lin[1]:.2f} .. {e_lin[2]:.2f}]")
    say(f"    evaluate step (render + loss), mel objective:    {e_mel[0]:.2f} ms [{e_mel[1]:.2f} .. {e_mel[2]:.2f}]  -> {e_mel[0] / e_lin[0]:.3f} x")

    # (c) the phases of the mel kernel
    short.loss(audio, peaks, 1)
    c_lin, c_mel, c_cut = alternating_ms(calls + [lambda: short.loss(audio, peaks, 1)], a.reps)
    say(f"(c) linear {c_lin[0]:.3f} ms, mel {c_mel[0]:.3f} ms, mel with every band cut to one bin {c_cut[0]:.3f} ms: the band sums "
        f"(longest runs {[int(n.max()) for _, n, _ in bank]} bins at n_fft 1024 / 2048 / 512, one lane per band) take "
        f"{c_mel[0] - c_cut[0]:.3f} ms; magnitudes written back + 64 terms a frame in the place of n_fft / 2 + 1: {c_cut[0] - c_lin[0]:+.3f} ms")
    got = mel.loss(audio, peaks, 1)
    say(f"    losses over the population: mel {float(got.min()):.4f} .. {float(got.max()):.4f}, linear "
        f"{float(lin.loss(audio, peaks, 1).min()):.4f} .. {float(lin.loss(audio, peaks, 1).max()):.4f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
