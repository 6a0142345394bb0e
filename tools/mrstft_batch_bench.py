#!/usr/bin/env python
"""The MRSTFT objective in the ragged batch against the sequential loop: N synthetic pairs of different lengths (default 8,
spread over 6 - 12 s, stereo, general-pb, popsize 128, 32 iterations, random_crop=True), each target the product's own render
of its input at seeded parameters (sample-aligned, as the objective needs), optimised by the list form of
run_es_batch(distance="mrstft") and by run_es(distance="mrstft") on one pair after the other -- same process, alternating, two
rounds each, with and without the early stop -- with the results compared field by field (they must be identical: same
seeds, same crops, same bits).  Wall times are host clocks around calls that end with the result on the host (every
iteration fetches its fitness).  Library calls per iteration of the batch are counted on the host in one extra, untimed run.

    python tools/mrstft_batch_bench.py [--out profiles/mrstft_batch.txt]
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
    """Inputs: the bench's seeded noise + tones; targets: the same input through the chain at seeded parameters."""
    from bench import synth_audio
    from st_ito.style_transfer import load_plugins, process_audio
    pl, D, _ = load_plugins(copy.deepcopy(plugins))
    xs, ts = [], []
    for i, s in enumerate(np.linspace(min_s, max_s, n_pairs)):
        n = int(s * 48000) + 17 * i          # odd lengths too
        w = np.random.default_rng(100 + i).random(D) * 0.5
        x = synth_audio(400 + i, 2, n)
        xs.append(x[None])
        ts.append(torch.from_numpy(process_audio(x.numpy(), w, 48000, pl))[None])
    return xs, ts


def identical(a, b) -> bool:
    return (np.array_equal(a["wopt"], b["wopt"]) and a["fopt"] == b["fopt"] and a["fval_history"] == b["fval_history"]
            and a["num_evals"] == b["num_evals"] and torch.equal(a["output_audio"], b["output_audio"]))


@contextlib.contextmanager
def counted_calls():
    """Counts the batch's library calls on the host: gathers, renders, table refills, losses."""
    from st_ito import engine, features
    counts = {"stito_gather_crops": 0, "stito_render_population_multi": 0, "stito_mrstft_target": 0, "stito_mrstft_loss(_slots)": 0}
    saved = (engine.RaggedInputs.gather, engine.render_population, features.MrstftTarget.update, features.MrstftTarget.loss)

    def wrap(fn, key):
        def inner(*a, **k):
            counts[key] += 1
            return fn(*a, **k)
        return inner

    engine.RaggedInputs.gather = wrap(saved[0], "stito_gather_crops")
    engine.render_population = wrap(saved[1], "stito_render_population_multi")
    features.MrstftTarget.update = wrap(saved[2], "stito_mrstft_target")
    features.MrstftTarget.loss = wrap(saved[3], "stito_mrstft_loss(_slots)")
    try:
        yield counts
    finally:
        engine.RaggedInputs.gather, engine.render_population, features.MrstftTarget.update, features.MrstftTarget.loss = saved


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
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)

    import eval_pst
    from st_ito.style_transfer import load_plugins, run_es, run_es_batch

    if not torch.cuda.is_available():
        raise SystemExit("mrstft_batch_bench: needs a GPU (there is no CPU path to time)")
    with contextlib.redirect_stdout(io.StringIO()):
        plugins, _, _ = load_plugins(eval_pst.get_plugins(a.chain))
        xs, ts = make_pairs(a.pairs, a.min_seconds, a.max_seconds, eval_pst.get_plugins(a.chain))
    kw = dict(sigma0=a.sigma0, popsize=a.popsize, random_crop=True, distance="mrstft")

    def batch(iters, early_stop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = run_es_batch(xs, ts, 48000, plugins, None, None, max_iters=iters, seed=a.seed, early_stop=early_stop, **kw)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def sequential(iters, early_stop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = [run_es(x.clone(), t.clone(), 48000, plugins, None, None, max_iters=iters, find_w0=False, seed=a.seed + b,
                        early_stop=early_stop, **kw) for b, (x, t) in enumerate(zip(xs, ts))]
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    batch(2, False)          # warm-up of every shape both sides use (workspaces, tables, code objects)
    sequential(2, False)
    lines = [f"# tools/mrstft_batch_bench.py on {torch.cuda.get_device_name(0)}: {a.pairs} stereo pairs of "
             f"{[int(x.shape[-1]) for x in xs]} samples, {a.chain}, popsize {a.popsize}, {a.max_iters} iterations, random_crop=True, "
             f"seed {a.seed}; distance=\"mrstft\"; wall seconds of {a.repeats} alternating rounds"]
    out = {"tool": "mrstft_batch_bench", "pairs": a.pairs, "popsize": a.popsize, "max_iters": a.max_iters}
    for early_stop in (False, True):
        tb, tq, same = [], [], True
        for _ in range(a.repeats):
            rb, dt = batch(a.max_iters, early_stop)
            tb.append(round(dt, 4))
            rq, dt = sequential(a.max_iters, early_stop)
            tq.append(round(dt, 4))
            same = same and all(identical(x, y) for x, y in zip(rb, rq))
        key = f"early_stop_{str(early_stop).lower()}"
        out[key] = {"batch_s": tb, "sequential_s": tq, "batch_over_sequential": round(min(tb) / min(tq), 4),
                    "num_evals": [r["num_evals"] for r in rb], "identical": bool(same)}
        lines.append(f"early_stop={early_stop}: batch {tb} s, sequential run_es loop {tq} s, best batch / best sequential "
                     f"{min(tb) / min(tq):.3f}; num_evals {out[key]['num_evals']}; results identical: {same}")
    with counted_calls() as counts:
        batch(a.max_iters, False)
    per_iter = {k: round(v / a.max_iters, 2) for k, v in counts.items()}
    out["library_calls_per_iteration"] = per_iter
    lines.append(f"library calls per iteration of the batch (early_stop=False; one group, spans move): {per_iter} -- a gather is 1 launch, "
                 "a table refill 2 per resolution + 1, a loss 1 per resolution + 1, the render depends on the chain")
    lines.append(json.dumps(out))
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report + "\n")
    return 0 if all(out[k]["identical"] for k in ("early_stop_false", "early_stop_true")) else 1


if __name__ == "__main__":
    sys.exit(main())
