#!/usr/bin/env python
"""Render time of the "autodiff" chain (dasp EQ -> dasp compressor -> dasp distortion -> noise-shaped reverb -> gain) next to the
"bench5" chain on the same device: pop 256, 48 kHz stereo, 10 s.

    python tools/dasp_chain_bench.py [--pop 256] [--seconds 10] [--reps 5] [--timeout 600] [--out profiles/dasp_chain.txt]

The script starts itself once more as a child under `rocprofv3 --kernel-trace --stats` (a fresh process: this one never opens the
GPU), which renders both chains and prints HIP-event times per render; the per-kernel times come from the trace's kernel table
(rocpd .db), averaged per launch.  The child runs under `timeout -k 10 <--timeout>`.  With --out the result becomes section 2 of
that file: whatever the file holds from the line that starts with "2. Time" on is replaced, so a second run does not pile up."""
import argparse
import glob
import os
import re
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))
    import numpy as np
    import torch
    from st_ito import effects as E, engine
    dev = torch.device("cuda", 0)
    n = int(a.seconds * SR)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.5 * rng.standard_normal((2, n))).astype(np.float32)).to(dev)
    for chain in ("autodiff", "bench5"):
        plugins = E.make_plugins(chain)
        D = sum(p["num_params"] for p in plugins.values())
        W = torch.from_numpy(rng.random((a.pop, D))).to(dev)
        compiled = engine.compile_chain(plugins)
        engine.render_population(plugins, x, W, SR, chain=compiled)   # warm-up (counted in the trace's averages too)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for s, e in ev:
            s.record()
            engine.render_population(plugins, x, W, SR, chain=compiled)
            e.record()
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) for s, e in ev]
        print(f"render {chain:9s} pop {a.pop} x 2 ch x {n} samples: {np.mean(ms):8.3f} ms per render (min {min(ms):.3f}, {a.reps} renders, "
              f"HIP events, incl. the final peak pass)", flush=True)


def short(name):
    """kernel name without namespace, parameter list and return type; template arguments kept"""
    name = name.split("(")[0].replace("stito::", "").replace("void ", "")
    return name.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the profiled child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = [f"2. Time: tools/dasp_chain_bench.py --pop {a.pop} --seconds {a.seconds:g} --reps {a.reps} ({SR} Hz stereo in, one device)", ""]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--pop", str(a.pop), "--seconds", str(a.seconds), "--reps", str(a.reps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(f"{' '.join(cmd)} failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
        lines += [l for l in res.stdout.splitlines() if l.startswith("render ")]
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if not dbs:
            sys.exit(f"no rocpd database under {tmp}:\n{res.stderr}")
        per = {}
        for name, dur in sqlite3.connect(dbs[0]).cursor().execute("select name, duration from kernels order by start"):
            t = per.setdefault(short(name), [0, 0.0])
            t[0] += 1
            t[1] += dur / 1e3
    lines.append("")
    lines.append(f"{'kernel':60s} {'launches':>8s} {'us per launch':>14s}   (rocprofv3 --kernel-trace, both chains, warm-up renders included)")
    for name, (cnt, us) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{name[:60]:60s} {cnt:8d} {us / cnt:14.1f}")
    text = "\n".join(("   " + l).rstrip() for l in lines)[3:] + "\n"
    print(text, end="")
    if a.out:
        head = open(a.out).read() if os.path.exists(a.out) else ""
        cut = next((m.start() for m in re.finditer(r"^2\. Time", head, re.M)), len(head))
        head = head[:cut].rstrip("\n")
        with open(a.out, "w") as f:
            f.write((head + "\n\n" if head else "") + text)


if __name__ == "__main__":
    main()
