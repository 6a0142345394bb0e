#!/usr/bin/env python
"""Host ES against device ES (run_es(device_es=True)) at the reference's two operating points, whole run_es calls:

  CLI default   pop 32, basic chain, stereo 5 s padded to 262144 samples, find_w0, 24 iterations (scripts/run_optim.py:304-306)
  PST harness   pop 128, general-pb chain, stereo 262144 samples, 32 iterations (scripts/eval/eval_pst.py:974-991)

both with early_stop=False and the synthetic Cnn14.  One process alternates the two ways, --rounds times each after one warm run
of each, stdout redirected; the figure is the median wall time of a call divided by its iterations (the find_w0 batch counts as
one more evaluate step in both).  Then the device ES kernels alone, by HIP events: ask, tell (update + the lazy decomposition,
which runs every iteration at these sizes) and the decomposition by itself, next to the 0.65 ms of host time between two passes
that profiles/README.md records for the host ES.  profiles/device_es.txt holds a recorded run.

    python tools/device_es_bench.py [--rounds 3] [--points cli,pst] [--sync-every 1,4,32]
"""
import argparse
import contextlib
import copy
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "st-ito_amd"), os.path.join(ROOT, "st-ito_amd", "scripts"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

from st_ito import cmaes, effects as E  # noqa: E402
from st_ito.style_transfer import load_plugins, process_audio, run_es  # noqa: E402
from st_ito.utils import get_param_embeds, make_synthetic_param_model  # noqa: E402
from st_ito_oracle import synth_audio  # noqa: E402

SR = 48000


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def timed_run(x, tg, plugins, model, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = quiet(run_es, x.clone(), tg.clone(), SR, plugins, model, get_param_embeds, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def point(label, plugins, pop, iters, seconds, find_w0, model, rounds, sync_list):
    plugins, D, _ = quiet(load_plugins, plugins)
    n = int(seconds * SR)
    x = synth_audio(300, 2, n)[None]
    tg = torch.from_numpy(process_audio(synth_audio(301, 2, n).numpy(), np.random.default_rng(3).random(D), SR, plugins))[None]
    base = dict(max_iters=iters, popsize=pop, sigma0=0.33, find_w0=find_w0, seed=11, early_stop=False)
    ways = [("host ES", base)] + [(f"device ES, sync_every {k}", dict(base, device_es=True, sync_every=k)) for k in sync_list]
    for _, kw in ways[:2]:   # warm: packing, workspaces, the first launch of every kernel
        timed_run(x, tg, plugins, model, dict(kw, max_iters=2))
    times = {name: [] for name, _ in ways}
    fopt = {}
    for _ in range(rounds):
        for name, kw in ways:
            dt, r = timed_run(x, tg, plugins, model, kw)
            times[name].append(dt)
            fopt[name] = r["fopt"]
    steps = iters + (1 if find_w0 else 0)
    print(f"{label}: D = {D}, pop {pop}, {iters} iterations{' + find_w0' if find_w0 else ''}, median [min .. max] of {rounds} run_es calls")
    for name, _ in ways:
        t = sorted(times[name])
        print(f"  {name:28s} {statistics.median(t) / steps * 1e3:7.3f} ms per step  [{t[0] / steps * 1e3:.3f} .. {t[-1] / steps * 1e3:.3f}]   "
              f"call {statistics.median(t) * 1e3:7.1f} ms   fopt {fopt[name]:.4f}", flush=True)
    return D


def kernel_times(D, pop, reps=40):
    """ask / tell / decomposition of a (D, pop) state by HIP events, median of `reps` iterations on a moving sphere fitness."""
    dev = torch.device("cuda", torch.cuda.current_device())
    es = cmaes.DeviceCMAEvolutionStrategy(np.full(D, 0.5), 0.33, {"bounds": [0, 1], "popsize": pop, "seed": 1}, max_iters=2 * reps + 8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_ask, t_tell, t_tell_busy = [], [], []
    load = torch.randn(4096, 4096, device=dev)
    for it in range(2 * reps + 8):
        W = es.ask_device()
        f = ((W - 0.3) ** 2).sum(dim=1).float()
        if it % 2:   # every other iteration right behind a few milliseconds of full-device work, as in the ES loop
            for _ in range(4):
                load @ load
        ev[1].record()
        es.tell_device(f)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 8:
            (t_tell_busy if it % 2 else t_tell).append(ev[1].elapsed_time(ev[2]))
    # ask on a fresh state (the one above is full, so frozen)
    es2 = cmaes.DeviceCMAEvolutionStrategy(np.full(D, 0.5), 0.33, {"bounds": [0, 1], "popsize": pop, "seed": 1}, max_iters=4)
    for it in range(reps):
        ev[0].record()
        es2.ask_device()
        ev[1].record()
        torch.cuda.synchronize()
        t_ask.append(ev[0].elapsed_time(ev[1]))
    # the decomposition alone: the host's next update of C on the exported state, undecomposed, imported again
    host = es.to_host()
    t_eig, sweeps = [], []
    for k in range(5):
        h = copy.deepcopy(host)
        h.eigeneval = h.counteval + 10 ** 9
        for _ in range(k + 1):
            Wh = h.ask()
            h.tell(Wh, [float(((w - 0.3) ** 2).sum()) for w in Wh])
        d = cmaes.DeviceCMAEvolutionStrategy.from_host(h, max_iters=2)
        ev[0].record()
        d.eigen_device()
        ev[1].record()
        torch.cuda.synchronize()
        if k:   # (the first launch sets the kernel's LDS attribute)
            t_eig.append(ev[0].elapsed_time(ev[1]))
            sweeps.append(d.export()["sweeps"])
    med = statistics.median
    print(f"  device ES kernels, N = {D}, popsize {pop} (HIP events, median of {reps}): ask {med(t_ask) * 1e3:.1f} us, tell + decomposition "
          f"{med(t_tell) * 1e3:.1f} us on an idle device, {med(t_tell_busy) * 1e3:.1f} us right behind full-device work; the decomposition alone, 1 - 4 updates of C behind: {', '.join(f'{t * 1e3:.1f} us ({s} sweeps)' for t, s in zip(t_eig, sweeps))}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", default="cli,pst")
    ap.add_argument("--sync-every", default="1,4,32")
    a = ap.parse_args()
    sync_list = [int(v) for v in a.sync_every.split(",")]
    model = make_synthetic_param_model(seed=0, input_norm="minmax")
    print(f"# tools/device_es_bench.py --rounds {a.rounds}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if "cli" in a.points:
        D = point("CLI default", E.make_plugins("basic"), 32, 24, 5.0, True, model, a.rounds, sync_list)
        kernel_times(D, 32)
    if "pst" in a.points:
        from eval_pst import get_plugins
        D = point("PST harness", get_plugins("general-pb"), 128, 32, 262144 / SR, False, model, a.rounds, sync_list)
        kernel_times(D, 128)


if __name__ == "__main__":
    main()
