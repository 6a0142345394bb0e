#!/usr/bin/env python
"""Timing of the sum / difference MR-STFT objective next to the L/R one at the bench shape (256 candidates x stereo x 262144
samples, the general-pb chain of scripts/eval_pst.py), the two alternating call by call in one process, medians of --reps
calls after warm-up:
  (a) stito_mrstft_loss and stito_mrstft_loss_sd alone (HIP events) on the same rendered population, and the two table builds;
  (b) the whole evaluate step (render + loss; wall time around a final synchronise) of MrstftEvaluator(stereo="lr") and
      MrstftEvaluator(stereo="sum-diff");
  (c) that the sum / difference loss is the L/R loss of sums and differences formed by torch (within float32: the peak is
      folded in before the addition here and after it there).
--trace runs only the two loss kernels, --reps times each, for a `rocprofv3 --kernel-trace --stats -- python
tools/mrstft_sd_bench.py --trace` run of its own (`--output-format csv` for a readable table): k_mrstft<false, false> is the
L/R kernel, k_mrstft<false, true> the sum / difference one.
    python tools/mrstft_sd_bench.py [--pop 256] [--reps 20] [--out profiles/mrstft_sd.txt]"""
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
    from st_ito.features import MrstftTarget
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
    say(f"# tools/mrstft_sd_bench.py: pop {a.pop}, stereo, {a.n} samples, general-pb chain (D = {D}), L/R and sum / difference alternating "
        f"call by call, median [min .. max] of {a.reps} calls each, {torch.cuda.get_device_name(0)}")

    xd, Wd, td = x.to(dev), torch.from_numpy(W).to(dev), target.to(dev)
    audio, peaks = engine.render_population(plugins, xd, Wd, 48000)
    assert audio.shape[1] == 2
    lr, sd = MrstftTarget(td), MrstftTarget(td, stereo="sum-diff")
    calls = [lambda: lr.loss(audio, peaks, 1), lambda: sd.loss(audio, peaks, 1)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    if a.trace:
        alternating_ms(calls, a.reps)
        return

    # (a) the kernels alone
    ms_lr, ms_sd = alternating_ms(calls, a.reps)
    rows = a.pop * 2
    say(f"(a) stito_mrstft_loss alone (3 resolution launches + the sum):    {ms_lr[0]:.3f} ms [{ms_lr[1]:.3f} .. {ms_lr[2]:.3f}]  "
        f"= {ms_lr[0] * 1e3 / rows:.2f} us per row")
    say(f"    stito_mrstft_loss_sd alone (the same launches, SD loader):    {ms_sd[0]:.3f} ms [{ms_sd[1]:.3f} .. {ms_sd[2]:.3f}]  "
        f"= {ms_sd[0] * 1e3 / rows:.2f} us per row  -> {ms_sd[0] / ms_lr[0]:.3f} x the L/R kernel")
    t_lr, t_sd = alternating_ms([lambda: lr.update(td), lambda: sd.update(td)], a.reps)
    say(f"    stito_mrstft_target / stito_mrstft_target_sd (2 rows): {t_lr[0]:.3f} ms [{t_lr[1]:.3f} .. {t_lr[2]:.3f}] / "
        f"{t_sd[0]:.3f} ms [{t_sd[1]:.3f} .. {t_sd[2]:.3f}]")

    # (b) the evaluate steps
    ev_lr = engine.MrstftEvaluator(x[None], 48000, plugins, target)
    ev_sd = engine.MrstftEvaluator(x[None], 48000, plugins, target, stereo="sum-diff")
    steps = [lambda: ev_lr.evaluate(W)[0], lambda: ev_sd.evaluate(W)[0]]
    for fn in steps:
        fn()
    e_lr, e_sd = alternating_ms(steps, a.reps, wall=True)
    say(f"(b) evaluate step (render + loss), L/R objective:              {e_lr[0]:.2f} ms [{e_lr[1]:.2f} .. {e_lr[2]:.2f}]")
    say(f"    evaluate step (render + loss), sum / difference objective: {e_sd[0]:.2f} ms [{e_sd[1]:.2f} .. {e_sd[2]:.2f}]  "
        f"-> {e_sd[0] / e_lr[0]:.3f} x")

    # (c) the same numbers as the L/R kernel on torch's sums and differences of the normalised population
    got = sd.loss(audio, peaks, 1)
    au = engine.normalize_audio_(audio.clone(), peaks)
    sums = lambda v: torch.stack([v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]], 1)   # noqa: E731
    ref = MrstftTarget(sums(td)).loss(sums(au))
    say(f"(c) max |sum/diff kernel - L/R kernel on torch's sums and differences| / the latter over the population = "
        f"{float(((got - ref).abs() / ref.abs()).max()):.2e}; losses {float(got.min()):.4f} .. {float(got.max()):.4f} "
        f"(L/R objective: {float(lr.loss(audio, peaks, 1).min()):.4f} .. {float(lr.loss(audio, peaks, 1).max()):.4f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
