#!/usr/bin/env python
"""Timing of the prefiltered MR-STFT objectives next to the plain ones at the bench shape (256 candidates x stereo x 262144 samples,
the general-pb chain of scripts/eval_pst.py, the 101-tap "aw" filter at 48 kHz), prefiltered and plain alternating call by call in
one process, medians of --reps calls after warm-up, for the linear and for the mel distance:
  (a) the loss calls alone (HIP events) on the same rendered population, the table builds and the sizes;
  (b) the whole evaluate step (render + loss; wall time around a final synchronise) of the four evaluators;
  (c) where the prefiltered kernel's time goes: the same kernel with ONE tap (the raw run is still staged, the outputs still go
      through registers and two more barriers, the span is still laid out through the reflection, but a chain is one fma), so
      (101 taps - 1 tap) is the filter's fmas and LDS reads and (1 tap - plain) the loader's extra passes.
--trace runs only the four loss calls, --reps times each, for a `rocprofv3 --kernel-trace --stats -- python
tools/mrstft_aw_bench.py --trace` run of its own: k_mrstft<false, false, MEL, true> are the prefiltered kernels.
    python tools/mrstft_aw_bench.py [--pop 256] [--reps 20] [--out profiles/mrstft_aw.txt]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", os.path.join("st-ito_amd", "scripts"), "st-ito_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
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
    ap.add_argument("--trace", action="store_true", help="only the loss kernels, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    import eval_pst
    from st_ito import _hip, engine
    from st_ito.features import MelMrstftTarget, MrstftTarget, PrefilteredMrstftTarget, mel_mrstft_bank
    from st_ito.style_transfer import load_plugins, process_audio

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
    say(f"# tools/mrstft_aw_bench.py: pop {a.pop}, stereo, {a.n} samples, general-pb chain (D = {D}), 48 kHz, the 101-tap 'aw' prefilter, "
        f"plain and prefiltered alternating call by call, median [min .. max] of {a.reps} calls each, {torch.cuda.get_device_name(0)}")

    xd, Wd, td = x.to(dev), torch.from_numpy(W).to(dev), target.to(dev)
    audio, peaks = engine.render_population(plugins, xd, Wd, 48000)
    bank = mel_mrstft_bank(48000)
    lin, mel = MrstftTarget(td), MelMrstftTarget(td, bank=bank)
    lin_aw = PrefilteredMrstftTarget(td, "aw", 48000)
    mel_aw = PrefilteredMrstftTarget(td, "aw", 48000, kind="mel", bank=bank)
    lin_1 = PrefilteredMrstftTarget(td, [1.0])
    calls = [lambda: lin.loss(audio, peaks, 1), lambda: lin_aw.loss(audio, peaks, 1), lambda: mel.loss(audio, peaks, 1),
             lambda: mel_aw.loss(audio, peaks, 1)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    if a.trace:
        alternating_ms(calls, a.reps)
        return

    # (a) the kernels alone
    ms = alternating_ms(calls, a.reps)
    for k, name in ((0, "linear"), (2, "mel")):
        p, f = ms[k], ms[k + 1]
        say(f"({'a' if k == 0 else ' '}) {name:6s} loss call alone (3 resolution launches + the sum), plain: {p[0]:.3f} ms [{p[1]:.3f} .. {p[2]:.3f}]   "
            f"prefiltered: {f[0]:.3f} ms [{f[1]:.3f} .. {f[2]:.3f}]  -> {f[0] / p[0]:.3f} x, +{f[0] - p[0]:.3f} ms")
    t_lin, t_aw = alternating_ms([lambda: lin.update(td), lambda: lin_aw.update(td)], a.reps)
    say(f"    stito_mrstft_target / stito_mrstft_target_pf (2 rows): {t_lin[0]:.3f} / {t_aw[0]:.3f} ms; table {lin.table.numel() * 4 / 2 ** 20:.2f} / "
        f"{lin_aw.table.numel() * 4 / 2 ** 20:.2f} MiB; workspace {lin._workspace_bytes(a.pop) / 2 ** 20:.2f} / {lin_aw._workspace_bytes(a.pop) / 2 ** 20:.2f} MiB")

    # (b) the evaluate steps
    evs = [engine.MrstftEvaluator(x[None], 48000, plugins, target), engine.PrefilteredMrstftEvaluator(x[None], 48000, plugins, target),
           engine.MelMrstftEvaluator(x[None], 48000, plugins, target),
           engine.PrefilteredMrstftEvaluator(x[None], 48000, plugins, target, kind="mel")]
    steps = [(lambda ev=ev: ev.evaluate(W)[0]) for ev in evs]
    for fn in steps:
        fn()
    es = alternating_ms(steps, a.reps, wall=True)
    for k, name in ((0, "linear"), (2, "mel")):
        p, f = es[k], es[k + 1]
        say(f"({'b' if k == 0 else ' '}) evaluate step (render + loss), {name:6s} plain: {p[0]:.2f} ms [{p[1]:.2f} .. {p[2]:.2f}]   prefiltered: {f[0]:.2f} ms "
            f"[{f[1]:.2f} .. {f[2]:.2f}]  -> {f[0] / p[0]:.3f} x")

    # (c) the phases of the prefiltered loader
    lin_1.loss(audio, peaks, 1)
    c_lin, c_aw, c_one = alternating_ms([calls[0], calls[1], lambda: lin_1.loss(audio, peaks, 1)], a.reps)
    say(f"(c) linear: plain {c_lin[0]:.3f} ms, 101 taps {c_aw[0]:.3f} ms, the same kernel with one tap {c_one[0]:.3f} ms: the taps' fmas and LDS "
        f"reads take {c_aw[0] - c_one[0]:.3f} ms, the loader's extra passes (raw run staged, outputs through registers, span laid out "
        f"through the reflection, three more barriers) {c_one[0] - c_lin[0]:+.3f} ms")
    got = lin_aw.loss(audio, peaks, 1)
    say(f"    losses over the population: mrstft-aw {float(got.min()):.4f} .. {float(got.max()):.4f}, mrstft "
        f"{float(lin.loss(audio, peaks, 1).min()):.4f} .. {float(lin.loss(audio, peaks, 1).max()):.4f}; library {os.path.basename(_hip.LIB_PATH)}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
