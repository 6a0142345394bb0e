#!/usr/bin/env python
"""Timing of compute_barkspectrum(mode="mono") on one PST population, (128, 2, 262144): fft_size 32768 through the radix-2
kernel that transforms a frame in LDS (the yardstick), 44100 and 48000 through the mixed-radix four-step kernel
(csrc/fft_mixed.hip).  Each length is warmed up, then timed as the median of --reps calls between device events; the time
per frame divides by items * (n // hop + 1).  There is no gate: the parent of the mixed-radix kernel cannot run its lengths.

The result replaces everything from the "# ---- timings" line on in profiles/fft_mixed.txt (what stands above it -- the
errors measured by tests/test_gpu_fft_mixed.py -- is kept).
    python tools/fft_mixed_bench.py [--pop 128] [--reps 20] [--out profiles/fft_mixed.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))
import torch
from st_ito import features as F

MARK = "# ---- timings"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_mixed.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fft_mixed_bench: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    n = 262144
    x = torch.randn(a.pop, 2, n, device=dev, generator=torch.Generator(dev).manual_seed(0)) * 0.1
    lines = [MARK + f" (tools/fft_mixed_bench.py, {torch.cuda.get_device_name(0)}): compute_barkspectrum(mode=\"mono\") on ({a.pop}, 2, {n}),",
             f"# median of {a.reps} calls between device events after {a.warmup} warm-up calls; min and max of the same calls beside it",
             "# fft_size  kernel       frames/item  ms/call (min .. max)        us/frame (ms/call over items * frames/item)"]
    for fft in (32768, 44100, 48000):
        call = lambda: F.compute_barkspectrum(x, fft_size=fft, mode="mono", mixed_radix=True)  # noqa: E731  (32768: the LDS kernel)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        T = n // (fft // 4) + 1
        med = statistics.median(ms)
        lines.append(f"  {fft:<8d}  {'radix-2 LDS ' if fft == 32768 else 'mixed-radix '} {T:<11d}  {med:8.3f} ({min(ms):.3f} .. {max(ms):.3f})   "
                     f"{med * 1e3 / (a.pop * T):8.3f}")
        print(lines[-1])
    head = ""
    if os.path.exists(a.out):
        head = open(a.out).read().split(MARK)[0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
