#!/usr/bin/env python
"""Ragged PST batch against the sequential loop: N synthetic (input, target) pairs of different lengths (default 8, spread over
6 - 12 s, stereo, general-pb, popsize 128, 32 iterations, random_crop=True) optimised by the list form of run_es_batch and by
run_es on one pair after the other -- same process, alternating, both with and without the early stop -- with the results
compared field by field (they must be identical: same seeds, same crops, same bits).  Wall times are host clocks around calls
that end with the result on the host (every iteration fetches its fitness).  Prints one JSON line.

    python tools/pst_batch_bench.py > profiles/pst_ragged_batch.txt
"""
from __future__ import annotations

import argparse
import contextlib
import copy
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "st-ito_amd"), os.path.join(ROOT, "st-ito_amd", "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_pairs(n_pairs: int, min_s: float, max_s: float, plugins):
    """Inputs: the bench's seeded noise + tones; targets: another signal (its own length) through the chain at random parameters."""
    from bench import synth_audio
    from st_ito.style_transfer import load_plugins, process_audio
    pl, D, _ = load_plugins(copy.deepcopy(plugins))
    secs = np.linspace(min_s, max_s, n_pairs)
    xs, ts = [], []
    for i, s in enumerate(secs):
        n = int(s * 48000) + 17 * i          # odd lengths too: the files of the benchmark are not multiples of anything
        m = int(secs[(i + 3) % n_pairs] * 48000) + 5 * i
        w = np.random.default_rng(100 + i).random(D) * 0.5
        xs.append(synth_audio(400 + i, 2, n)[None])
        ts.append(torch.from_numpy(process_audio(synth_audio(500 + i, 2, m).numpy(), w, 48000, pl))[None])
    return xs, ts


def identical(a, b) -> bool:
    return (np.array_equal(a["wopt"], b["wopt"]) and a["fopt"] == b["fopt"] and a["fval_history"] == b["fval_history"]
            and a["num_evals"] == b["num_evals"] and torch.equal(a["output_audio"], b["output_audio"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=6.0)
    ap.add_argument("--max-seconds", type=float, default=12.0)
    ap.add_argument("--chain", default="general-pb")
    ap.add_argument("--popsize", type=int, default=128)
    ap.add_argument("--max-iters", type=int, default=32)
    ap.add_argument("--sigma0", type=float, default=0.33)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2, help="timed (batch, sequential) rounds per early_stop setting")
    a = ap.parse_args(argv)

    import eval_pst
    from st_ito.style_transfer import load_plugins, run_es, run_es_batch
    from st_ito.utils import get_param_embeds, make_synthetic_param_model

    if not torch.cuda.is_available():
        raise SystemExit("pst_batch_bench: needs a GPU (there is no CPU path to time)")
    model = make_synthetic_param_model(0)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        plugins, _, _ = load_plugins(eval_pst.get_plugins(a.chain))
        xs, ts = make_pairs(a.pairs, a.min_seconds, a.max_seconds, eval_pst.get_plugins(a.chain))
    kw = dict(sigma0=a.sigma0, popsize=a.popsize, random_crop=True)

    def batch(iters, early_stop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = run_es_batch(xs, ts, 48000, plugins, model, get_param_embeds, max_iters=iters, seed=a.seed, early_stop=early_stop, **kw)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def sequential(iters, early_stop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = [run_es(x.clone(), t.clone(), 48000, plugins, model, get_param_embeds, max_iters=iters, find_w0=False,
                        seed=a.seed + b, early_stop=early_stop, **kw) for b, (x, t) in enumerate(zip(xs, ts))]
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    batch(2, False)          # warm-up of every shape both sides use (packed weights, workspaces, code objects)
    sequential(2, False)
    out = {"tool": "pst_batch_bench", "device": torch.cuda.get_device_name(0), "pairs": a.pairs, "chain": a.chain,
           "input_samples": [int(x.shape[-1]) for x in xs], "target_samples": [int(t.shape[-1]) for t in ts],
           "popsize": a.popsize, "max_iters": a.max_iters, "random_crop": True, "seed": a.seed, "repeats": a.repeats}
    for early_stop in (False, True):
        tb, tq, same = [], [], True
        for _ in range(a.repeats):
            rb, dt = batch(a.max_iters, early_stop)
            tb.append(round(dt, 4))
            rq, dt = sequential(a.max_iters, early_stop)
            tq.append(round(dt, 4))
            same = same and all(identical(x, y) for x, y in zip(rb, rq))
        out[f"early_stop_{str(early_stop).lower()}"] = {
            "batch_s": tb, "sequential_s": tq, "batch_over_sequential": round(min(tb) / min(tq), 4),
            "batch_s_per_pair": round(min(tb) / a.pairs, 4), "sequential_s_per_pair": round(min(tq) / a.pairs, 4),
            "num_evals": [r["num_evals"] for r in rb], "identical": bool(same)}
    print(json.dumps(out))
    return 0 if all(out[k]["identical"] for k in ("early_stop_false", "early_stop_true")) else 1


if __name__ == "__main__":
    sys.exit(main())
