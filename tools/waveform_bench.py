#!/usr/bin/env python
"""Timing of the waveform objectives next to the MR-STFT one at the bench shape (256 candidates x stereo x 262144 samples, the
general-pb chain of scripts/eval_pst.py, 48 kHz), "esr", "esr-aw" (the 101-tap "aw" filter) and "mrstft" alternating call by call in
one process, medians of --reps calls after warm-up:
  (a) the loss calls alone (HIP events) on the same rendered population -- also "logcosh", whose term is a float64 sinh and log1p per
      sample, and the same filtered kernel with ONE tap --, the table builds and the sizes;
  (b) the render alone and the whole evaluate step (render + loss; wall time around a final synchronise) of the three evaluators,
      and what the unfiltered step spends beyond its render.
--trace runs only the loss calls, --reps times each, for a `rocprofv3 --kernel-trace --stats -- python tools/waveform_bench.py
--trace` run of its own: k_waveform<false, PRE, LC> are the candidate kernels.
    python tools/waveform_bench.py [--pop 256] [--reps 20] [--out profiles/waveform_objective.txt]"""
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
    from st_ito.features import MrstftTarget, WaveformTarget
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
    say(f"# tools/waveform_bench.py: pop {a.pop}, stereo, {a.n} samples, general-pb chain (D = {D}), 48 kHz, 'esr' / 'esr-aw' (101 taps) / "
        f"'mrstft' alternating call by call, median [min .. max] of {a.reps} calls each, {torch.cuda.get_device_name(0)}")

    xd, Wd, td = x.to(dev), torch.from_numpy(W).to(dev), target.to(dev)
    audio, peaks = engine.render_population(plugins, xd, Wd, 48000)
    mr, wf, wf_aw, wf_1 = MrstftTarget(td), WaveformTarget(td), WaveformTarget(td, "aw", 48000), WaveformTarget(td, [1.0])
    calls = [lambda: wf.loss(audio, peaks, 1), lambda: wf_aw.loss(audio, peaks, 1), lambda: mr.loss(audio, peaks, 1),
             lambda: wf.loss(audio, peaks, 1, kind="logcosh"), lambda: wf_aw.loss(audio, peaks, 1, kind="logcosh"),
             lambda: wf_1.loss(audio, peaks, 1)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    if a.trace:
        alternating_ms(calls, a.reps)
        return

    # (a) the kernels alone
    ms = alternating_ms(calls, a.reps)
    fmt = lambda v: f"{v[0]:.3f} ms [{v[1]:.3f} .. {v[2]:.3f}]"   # noqa: E731
    read_mb = audio.numel() * 4 / 1e6
    say(f"(a) loss call alone (the pass over the rows + the final launch), esr: {fmt(ms[0])} = {read_mb / ms[0][0] / 1e3:.2f} TB/s of the "
        f"{read_mb:.0f} MB it reads once   esr-aw: {fmt(ms[1])}   mrstft (3 resolution launches + the sum): {fmt(ms[2])}")
    say(f"    mrstft / esr {ms[2][0] / ms[0][0]:.1f} x, mrstft / esr-aw {ms[2][0] / ms[1][0]:.1f} x; logcosh: {fmt(ms[3])}, logcosh-aw: {fmt(ms[4])}; "
        f"the filtered kernel with one tap: {fmt(ms[5])}, so 101 taps' fmas and LDS reads take {ms[1][0] - ms[5][0]:.3f} ms and staging the "
        f"run in LDS {ms[5][0] - ms[0][0]:+.3f} ms")
    t_wf, t_aw, t_mr = alternating_ms([lambda: wf.update(td), lambda: wf_aw.update(td), lambda: mr.update(td)], a.reps)
    L = _hip.lib()
    say(f"    stito_waveform_target plain / 101 taps, stito_mrstft_target (2 rows): {t_wf[0]:.3f} / {t_aw[0]:.3f} / {t_mr[0]:.3f} ms; table "
        f"{wf.table.numel() * 4 / 2 ** 20:.2f} / {wf_aw.table.numel() * 4 / 2 ** 20:.2f} / {mr.table.numel() * 4 / 2 ** 20:.2f} MiB; workspace "
        f"{L.stito_waveform_workspace_bytes(0, a.pop, 2, a.n) / 2 ** 20:.2f} / {L.stito_waveform_workspace_bytes(101, a.pop, 2, a.n) / 2 ** 20:.2f} / "
        f"{mr._workspace_bytes(a.pop) / 2 ** 20:.2f} MiB; tile {L.stito_waveform_tile_samples(0)} samples")

    # (b) the render alone and the evaluate steps
    evs = [engine.WaveformEvaluator(x[None], 48000, plugins, target, kind="esr"),
           engine.WaveformEvaluator(x[None], 48000, plugins, target, kind="esr", prefilter="aw"),
           engine.MrstftEvaluator(x[None], 48000, plugins, target)]
    ws, chain = engine.Workspace(), engine.compile_chain(plugins)
    steps = [lambda: engine.render_population(plugins, xd, Wd, 48000, chain, ws=ws)] + [(lambda ev=ev: ev.evaluate(W)[0]) for ev in evs]
    for fn in steps:
        fn()
    r_dev = alternating_ms(steps[:1], a.reps)[0]
    es = alternating_ms(steps, a.reps, wall=True)
    say(f"(b) render alone (population already on the device): {fmt(r_dev)} on the device, {es[0][0]:.2f} ms wall [{es[0][1]:.2f} .. {es[0][2]:.2f}]")
    say(f"    evaluate step (upload of W + render + loss), esr: {es[1][0]:.2f} ms [{es[1][1]:.2f} .. {es[1][2]:.2f}]   esr-aw: {es[2][0]:.2f} ms "
        f"[{es[2][1]:.2f} .. {es[2][2]:.2f}]   mrstft: {es[3][0]:.2f} ms [{es[3][1]:.2f} .. {es[3][2]:.2f}]  -> mrstft / esr {es[3][0] / es[1][0]:.2f} x, "
        f"mrstft / esr-aw {es[3][0] / es[2][0]:.2f} x")
    over = es[1][0] - es[0][0]
    say(f"    the esr step is {es[1][0] / es[0][0]:.3f} x its render's wall time: +{over:.3f} ms, of which the loss call's kernels are {ms[0][0]:.3f} ms "
        f"and the rest ({over - ms[0][0]:+.3f} ms) the upload of W, the slot-free launches' host time and the result's allocation")
    got, got_aw, got_mr = wf.loss(audio, peaks, 1), wf_aw.loss(audio, peaks, 1), mr.loss(audio, peaks, 1)
    say(f"    losses over the population: esr {float(got.min()):.4f} .. {float(got.max()):.4f}, esr-aw {float(got_aw.min()):.4f} .. "
        f"{float(got_aw.max()):.4f}, mrstft {float(got_mr.min()):.4f} .. {float(got_mr.max()):.4f}; library {os.path.basename(_hip.LIB_PATH)}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
