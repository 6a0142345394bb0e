"""What the device CMA-ES tests share (tests/test_device_es_host.py, tests/test_gpu_device_es.py): a pure-Python restatement of
the library's counter-based generator, the host-side stepping that produces the states the device imports, and the error report.

The generator (csrc/cmaes.hip): bits(seed, iteration, e) is output e of the splitmix64 stream whose state starts at
mix(mix(seed) ^ iteration); the deviate is sqrt(-2 ln u1) cos(2 pi u2) with u1, u2 the high and low 32 bits, each (k + 0.5) / 2^32.
"""
import math
import os

import numpy as np

M64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def mix(x: int) -> int:
    x = (x + GOLDEN_GAMMA) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def bits(seed: int, iteration: int, e: int) -> int:
    key = mix(mix(seed & M64) ^ iteration)
    return mix((key + e * GOLDEN_GAMMA) & M64)


def normal(b: int) -> float:
    u1 = ((b >> 32) + 0.5) / 4294967296.0
    u2 = ((b & 0xFFFFFFFF) + 0.5) / 4294967296.0
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


def host_es(x0, sigma0, lam, seed=1):
    from st_ito import cmaes
    return cmaes.CMAEvolutionStrategy(x0, sigma0, {"bounds": [0, 1], "popsize": lam, "seed": seed})


def host_hsig(es) -> bool:
    """hsig of the tell the host strategy has just made, from its state (the class does not keep it)."""
    return bool(np.linalg.norm(es.ps) / math.sqrt(1 - (1 - es.cs) ** (2 * es.countiter)) / es.chiN < 1.4 + 2 / (es.N + 1))


def ellipsoid(N):
    scale = 10.0 ** (6 * np.arange(N) / (N - 1))
    return lambda w: float((scale * (np.asarray(w) - 0.5) ** 2).sum())


def step_to_axis_ratio(N, lam, ratio=1e2, seed=3, limit=20000):
    """The host strategy stepped on the 1e6-conditioned ellipsoid until D.max() / D.min() exceeds `ratio`."""
    es = host_es(np.full(N, 0.2), 0.3, lam, seed)
    f = ellipsoid(N)
    while es.D.max() / es.D.min() <= ratio:
        assert es.countiter < limit
        W = es.ask()
        es.tell(W, [f(w) for w in W])
    return es


STATE_KEYS = ("mean", "sigma", "pc", "ps", "C", "B", "D", "invsqrtC", "eigeneval", "counteval", "countiter", "best_x", "best_f", "best_evals")


def save_state(es, path):
    np.savez_compressed(path, **{k: np.asarray(getattr(es, k)) for k in STATE_KEYS})


def load_state(path, N, lam):
    """A host strategy carrying a recorded state (tests/golden/make_device_es_states.py wrote it)."""
    es = host_es(np.full(N, 0.2), 0.3, lam)
    with np.load(path) as z:
        for k in STATE_KEYS:
            v = z[k]
            setattr(es, k, v.copy() if v.ndim else (int(v) if v.dtype.kind == "i" else float(v)))
    return es


# ---- the error report: every test prints its figures; STITO_DEVICE_ES_REPORT=<file> also appends them there -------------------------
def report(line: str):
    print(line)
    path = os.environ.get("STITO_DEVICE_ES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
