"""The device-resident CMA-ES (csrc/cmaes.hip, cmaes.DeviceCMAEvolutionStrategy, run_es(device_es=True)) against the host
CMAEvolutionStrategy in float64: one step from a fresh state over a grid of sizes, the Jacobi eigendecomposition from imported
states and on each side of the sizes at which its buffers leave LDS, one tell from those ill-conditioned states, the stable
ordering, every region of the bound transform, both hsig branches, twenty iterations in lockstep, the generator, the frozen
state, a tell without an ask, a captured iteration replayed, a sanity floor on what it optimises, and device-resident W into
both evaluators.

The bars are derived, not measured: the two sides differ in the order of float64 sums over at most max(N, popsize) terms, so a
quantity agrees to 1e-12 of its largest magnitude (about 100 n eps); the eigendecomposition's bars come from its 1e-15 stopping
rule times N.  Every test prints its worst figures (run with -s; STITO_DEVICE_ES_REPORT=<file> collects them):
profiles/device_es.txt holds a recorded run.
"""
import copy
import os

import numpy as np
import pytest
import torch

import device_es_ref as R
import st_ito_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
NS, LAMS = (2, 5, 37, 64, 65, 128), (2, 3, 4, 32, 65)
BAR = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from st_ito import _hip
    _hip.lib()  # must load: no silent fallback
    return torch.device("cuda", 0)


def _device(x0, sigma0, lam, **kw):
    from st_ito import cmaes
    return cmaes.DeviceCMAEvolutionStrategy(x0, sigma0, {"bounds": [0, 1], "popsize": lam, "seed": 1}, **kw)


def _rel(got, want):
    """max |got - want| over the largest magnitude of the quantity (1 where that is zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    scale = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0)


def _compare_state(es, s, W_host=None, W_dev=None):
    """Relative errors of the device export `s` against the host strategy `es`; integers and best_evals must be equal."""
    errs = {k: _rel(s[k], getattr(es, k)) for k in ("mean", "ps", "pc", "C")}
    errs["sigma"] = abs(s["sigma"] - es.sigma) / es.sigma
    if W_host is not None:
        errs["W"] = _rel(W_dev, W_host)
    if es.best_x is not None:
        errs["best_x"] = _rel(s["best_x"], es.best_x)
    assert s["best_f"] == es.best_f or (np.isinf(s["best_f"]) and np.isinf(es.best_f))
    assert (s["best_evals"], s["counteval"], s["countiter"], s["eigeneval"]) == (es.best_evals, es.counteval, es.countiter, es.eigeneval)
    return errs


# ---- 1. one step from a fresh state ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_step(dev):
    """Every (N, popsize) of the grid: ask and tell on both sides from the same deviates and the same distinct fitness values.
    -> {(N, lam): (errors, host hsig, device hsig)}"""
    out = {}
    for N in NS:
        for lam in LAMS:
            rng = np.random.default_rng(1000 * N + lam)
            x0 = 0.2 + 0.6 * rng.random(N)
            z = rng.standard_normal((lam, N))
            f = (0.37 * rng.permutation(lam) + 0.11).astype(np.float32)
            es = R.host_es(x0, 0.3, lam)
            es._z_next = z
            W = np.array(es.ask())
            es.tell(list(W), f.astype(np.float64).tolist())
            d = _device(x0, 0.3, lam, max_iters=2)
            Wd = d.ask_device(z).cpu().numpy()
            d.tell_device(torch.from_numpy(f).to(dev))
            s = d.export()
            out[(N, lam)] = (_compare_state(es, s, W, Wd), R.host_hsig(es), bool(s["hsig"]))
    worst = {}
    for errs, _, _ in out.values():
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    R.report("one step from a fresh state, worst relative error over the grid: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    return out


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("N", NS)
def test_one_step_from_a_fresh_state(one_step, N, lam):
    errs, _, _ = one_step[(N, lam)]
    assert all(v <= BAR for v in errs.values()), errs


# ---- 2. the eigendecomposition from imported states ------------------------------------------------------------------------------
def _eigen_figures(d, C_in):
    d.eigen_device()
    s = d.export()
    C = np.triu(C_in) + np.triu(C_in, 1).T
    np.testing.assert_array_equal(s["C"], C)   # the decomposition symmetrises C from its upper triangle, like the host, and leaves it
    B, D, inv = s["B"], s["D"], s["invsqrtC"]
    N = len(D)
    ev = np.linalg.eigvalsh(C)
    return {"recon": np.abs((B * D[None, :] ** 2) @ B.T - C).max() / np.abs(C).max(),
            "orth": np.abs(B.T @ B - np.eye(N)).max(),
            "invsqrt": np.abs(inv @ C @ inv - np.eye(N)).max() / (ev.max() / ev.min()),
            "eigvals": np.abs(np.sort(D ** 2) - ev).max() / ev.max(),
            "sweeps": s["sweeps"]}


@pytest.fixture(scope="module")
def ellipsoid_states():
    """Host strategies whose axis ratio has passed 1e2 on the 1e6-conditioned ellipsoid (N = 128: the recorded state)."""
    out = {5: R.step_to_axis_ratio(5, 8), 37: R.step_to_axis_ratio(37, 16), 128: R.load_state(os.path.join(GOLDEN, "device_es_n128.npz"), 128, 64)}
    for es in out.values():
        assert es.D.max() / es.D.min() > 1e2
    return out


def _decompose_the_next_update(es, N):
    """The device decomposition of the host's NEXT update of C -- not the C that B and D already belong to -- left undecomposed
    by the host and imported: the warm start every tell of a run makes."""
    from st_ito import cmaes
    es = copy.deepcopy(es)
    es.eigeneval = es.counteval + 10 ** 9   # keeps the host from decomposing it
    W = es.ask()
    f = R.ellipsoid(N)
    es.tell(W, [f(w) for w in W])
    es.eigeneval = es.counteval
    fig = _eigen_figures(cmaes.DeviceCMAEvolutionStrategy.from_host(es, max_iters=2), es.C)
    R.report(f"eigendecomposition, imported state N = {N} (cond {np.linalg.cond(es.C):.1e}): " + "  ".join(f"{k} {v:.2e}" if k != "sweeps" else f"sweeps {v}" for k, v in fig.items()))
    assert fig["recon"] <= BAR and fig["orth"] <= BAR and fig["invsqrt"] <= BAR and fig["eigvals"] <= BAR, fig
    assert fig["sweeps"] < 30


@pytest.mark.parametrize("N", (5, 37, 128))
def test_eigendecomposition_of_an_imported_state(dev, ellipsoid_states, N):
    _decompose_the_next_update(ellipsoid_states[N], N)


@pytest.mark.parametrize("N", (81, 82, 96, 97))
def test_eigendecomposition_at_the_placement_thresholds(dev, N):
    """The decomposition keeps its two work matrices and the rotated copy of B in LDS up to N = 81, the two work matrices up to 96
    and one above: each side of both thresholds, from a state a few host iterations away from the identity (the placement, not
    the conditioning, is what these sizes are about)."""
    es = R.host_es(np.full(N, 0.2), 0.3, 16, seed=4)
    f = R.ellipsoid(N)
    for _ in range(3):
        W = es.ask()
        es.tell(W, [f(w) for w in W])
    _decompose_the_next_update(es, N)


@pytest.fixture(scope="module")
def imported_tells(dev, ellipsoid_states):
    """A device tell from each ill-conditioned state (ask pending when imported), the host told the same float32 fitness.
    -> {N: (errors, host hsig, device hsig)}"""
    from st_ito import cmaes
    out = {}
    for N, es in ellipsoid_states.items():
        es = copy.deepcopy(es)
        W = es.ask()
        fn = R.ellipsoid(N)
        f = np.array([fn(w) for w in W], np.float32)
        d = cmaes.DeviceCMAEvolutionStrategy.from_host(es, max_iters=2)
        d.tell_device(torch.from_numpy(f).to(dev))
        es.tell(W, f.astype(np.float64).tolist())
        out[N] = (_compare_state(es, d.export()), R.host_hsig(es), bool(d.export()["hsig"]))
        R.report(f"one tell from the imported state N = {N}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(out[N][0].items())))
    return out


@pytest.mark.parametrize("N", (5, 37, 128))
def test_one_tell_from_an_imported_state(imported_tells, N):
    """Ordering, the Mahalanobis rescaling, ps through a non-identity invsqrtC and hsig from a state whose axis ratio is above 1e2."""
    errs, _, _ = imported_tells[N]
    assert all(v <= BAR for v in errs.values()), errs


def test_eigendecomposition_single_rotation_and_diagonal(dev):
    from st_ito import cmaes
    es = R.host_es(np.array([0.4, 0.6]), 0.3, 4)
    es.C = np.array([[2.0, 0.75], [0.75, 1.0]])
    fig = _eigen_figures(cmaes.DeviceCMAEvolutionStrategy.from_host(es, max_iters=2), es.C)
    assert max(fig["recon"], fig["orth"], fig["invsqrt"], fig["eigvals"]) <= BAR and fig["sweeps"] == 1, fig
    es = R.host_es(np.full(7, 0.5), 0.3, 6)
    es.C = np.diag(np.arange(1.0, 8.0) ** 2)
    d = cmaes.DeviceCMAEvolutionStrategy.from_host(es, max_iters=2)
    fig = _eigen_figures(d, es.C)
    assert max(fig["recon"], fig["orth"], fig["invsqrt"], fig["eigvals"]) <= BAR and fig["sweeps"] == 0, fig
    np.testing.assert_array_equal(d.export()["B"], np.eye(7))


# ---- 3. ordering ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")
ORDER_CASES = {
    "ties": [3.0, 1.0, 2.0, 1.0, 3.0, 2.0, 1.0, 0.5],
    "one_nan": [3.0, NAN, 2.0, 1.0, 4.0, 6.0, 5.0, 0.5],
    "several_nan": [NAN, 1.0, NAN, 1.0, 0.25, NAN, 5.0, NAN],
    "all_equal": [2.0] * 8,
}


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_ordering_is_numpys_stable_argsort(dev, name):
    f = np.array(ORDER_CASES[name], np.float32)
    N, lam = 5, len(f)
    rng = np.random.default_rng(7)
    x0, z = 0.2 + 0.6 * rng.random(N), rng.standard_normal((lam, N))
    es = R.host_es(x0, 0.3, lam)
    es._z_next = z
    W = es.ask()
    es.tell(W, f.astype(np.float64).tolist())
    d = _device(x0, 0.3, lam, max_iters=2)
    d.ask_device(z)
    d.tell_device(torch.from_numpy(f).to(dev))
    errs = _compare_state(es, d.export())
    assert all(v <= BAR for v in errs.values()), errs


# ---- 4. bounds -----------------------------------------------------------------------------------------------------------------
def test_every_region_of_the_bound_transform(dev):
    N, lam = 3, 256
    x0 = np.array([0.0, 1.0, 0.5])
    z = np.random.default_rng(4).standard_normal((lam, N))
    es = R.host_es(x0, 2.0, lam)
    es._z_next = z
    W = np.array(es.ask())
    g, bt = es._geno, es.boundary
    lo, hi = bt.lb - bt.al, bt.ub + bt.au
    v = lo + np.mod(g - lo, 2 * (hi - lo))
    regions = {"identity": (g >= bt.lb + bt.al) & (g <= bt.ub - bt.au), "lower quadratic": (g >= lo) & (g < bt.lb + bt.al),
               "upper quadratic": (g <= hi) & (g > bt.ub - bt.au), "shifted": ((g < lo) | (g > hi)) & (v <= hi),
               "mirrored": ((g < lo) | (g > hi)) & (v > hi)}
    assert all(m.any() for m in regions.values()), {k: int(m.sum()) for k, m in regions.items()}
    Wd = _device(x0, 2.0, lam, max_iters=2).ask_device(z).cpu().numpy()
    assert Wd.min() >= 0.0 and Wd.max() <= 1.0
    err = np.abs(Wd - W).max()
    R.report(f"bound transform, {', '.join(f'{k} {int(m.sum())}' for k, m in regions.items())}: max |W - host| {err:.2e}")
    assert err <= 1e-15


# ---- 5. both hsig branches -----------------------------------------------------------------------------------------------------
def test_both_hsig_branches(dev, one_step, imported_tells):
    from st_ito import cmaes
    seen = [(h, g) for _, h, g in one_step.values()] + [(h, g) for _, h, g in imported_tells.values()]
    # a run whose steps keep pointing the same way (a far optimum, a small step size) lengthens ps until hsig turns false: the host
    # state just before that tell, ask pending, is imported
    N, lam = 5, 8
    es = R.host_es(np.full(N, 0.05), 0.01, lam, seed=2)
    target = np.full(N, 0.9)
    for _ in range(200):
        W = es.ask()
        f = [float(((w - target) ** 2).sum()) for w in W]
        before = copy.deepcopy(es)
        es.tell(W, f)
        if not R.host_hsig(es):
            break
    assert not R.host_hsig(es)
    d = cmaes.DeviceCMAEvolutionStrategy.from_host(before, max_iters=2)
    f32 = np.array(f, np.float32)   # what tell takes; both sides are told these values
    d.tell_device(torch.from_numpy(f32).to(dev))
    before.tell(W, f32.astype(np.float64).tolist())
    s = d.export()
    seen.append((R.host_hsig(before), bool(s["hsig"])))
    errs = _compare_state(before, s)
    assert all(v <= BAR for v in errs.values()), errs
    assert any(h for h, _ in seen) and any(not h for h, _ in seen)
    assert all(h == g for h, g in seen)


# ---- 6. twenty iterations in lockstep ------------------------------------------------------------------------------------------
def test_twenty_iterations_in_lockstep(dev):
    """The same deviates every iteration means the same steps y = (z o D) B^T: the order and the signs of the eigenpairs are free
    (numpy's eigh and the Jacobi sweeps choose their own), so from the second iteration on the device is handed the host's z
    expressed in ITS eigenbasis, z' = y B_dev / D_dev -- an orthogonal change of coordinates, exact to rounding."""
    N, lam, seed = 37, 32, 0
    rng = np.random.default_rng(seed)
    x0 = rng.random(N)
    es, d = R.host_es(x0, 0.3, lam), _device(x0, 0.3, lam, max_iters=20)
    gap, lines = np.inf, []
    s = d.export()
    for it in range(20):
        z = rng.standard_normal((lam, N))
        es._z_next = z
        y = z * es.D[None, :] @ es.B.T
        z = y @ s["B"] / s["D"][None, :]
        W = es.ask()
        f = np.array([((w - 0.3) ** 2).sum() for w in W]).astype(np.float32).astype(np.float64)   # tell takes float32
        gap = min(gap, float(np.diff(np.sort(f)).min()))
        es.tell(W, f.tolist())
        Wd = d.ask_device(z)
        d.tell_device(((Wd - 0.3) ** 2).sum(dim=1))
        s = d.export()
        e = (_rel(s["mean"], es.mean), abs(s["sigma"] - es.sigma) / es.sigma, _rel(s["C"], es.C))
        lines.append(f"  iteration {it + 1:2d}: mean {e[0]:.2e}  sigma {e[1]:.2e}  C {e[2]:.2e}")
    # the seed's condition: a rounding difference cannot reorder the ranks (float32 fitness: the gap is far above its resolution too)
    assert gap > 1e-9 and gap > 1e-6, gap
    R.report(f"twenty iterations in lockstep (N {N}, popsize {lam}, smallest fitness gap {gap:.1e}), relative error after each:\n" + "\n".join(lines))
    assert max(e) <= 1e-9, e
    assert s["countiter"] == es.countiter == 20 and s["done"] == 20


# ---- 7. the generator ----------------------------------------------------------------------------------------------------------
def _normals(dev, seed, iteration, first, count, want_bits=False):
    from st_ito import _hip
    z = torch.empty(count, dtype=torch.float64, device=dev)
    b = torch.empty(count, dtype=torch.int64, device=dev) if want_bits else None
    _hip.check(_hip.lib().stito_cmaes_normals(seed, iteration, first, count, _hip.ptr(z), _hip.ptr(b), _hip.stream_ptr()))
    return (z.cpu().numpy(), b.cpu().numpy().view(np.uint64)) if want_bits else z.cpu().numpy()


def test_generator(dev):
    seed, it, n = 12345, 7, 32 * 37
    z, b = _normals(dev, seed, it, 0, n, want_bits=True)
    # however lambda x N is cut, the same bits
    parts = np.concatenate([_normals(dev, seed, it, a, c) for a, c in ((0, 1), (1, 36), (37, 600), (637, n - 637))])
    np.testing.assert_array_equal(parts, z)
    assert not np.array_equal(_normals(dev, seed + 1, it, 0, n), z) and not np.array_equal(_normals(dev, seed, it + 1, 0, n), z)
    # the integer stage is the Python restatement, exactly; the float stage to the libraries' log and cos
    assert [int(v) for v in b[:64]] == [R.bits(seed, it, e) for e in range(64)]
    assert np.abs(z[:64] - np.array([R.normal(int(v)) for v in b[:64]])).max() <= 1e-14
    # the strategy's own stream is this one, keyed by its countiter
    d = _device(np.full(37, 0.5), 0.1, 32, max_iters=2)
    d2 = _device(np.full(37, 0.5), 0.1, 32, max_iters=2)
    W_own = d.ask_device().clone()
    assert torch.equal(d2.ask_device(_normals(dev, d.seed, 0, 0, n).reshape(32, 37)), W_own)
    # moments over 2^20 deviates, within five standard errors
    m = 1 << 20
    z = _normals(dev, 99, 0, 0, m)
    mean, var, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    R.report(f"generator, 2^20 deviates: mean {mean:+.2e}  variance {var:.5f}  fourth moment {m4:.4f}")
    assert abs(mean) <= 5 / np.sqrt(m) and abs(var - 1) <= 5 * np.sqrt(2 / m) and abs(m4 - 3) <= 5 * np.sqrt(96 / m)


# ---- 8. the frozen state -------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.fixture(scope="module")
def short_pair():
    from st_ito import effects as E
    from st_ito.style_transfer import process_audio
    x = O.synth_audio(1234, 1, 24000)[None]
    plugins = E.make_plugins("eq")
    target = torch.from_numpy(process_audio(x[0].numpy(), np.random.default_rng(5).random(18), SR, plugins))[None]
    return x, target


def test_result_does_not_depend_on_sync_every(dev, short_pair, capsys):
    from st_ito import effects as E
    from st_ito.style_transfer import run_es
    x, target = short_pair
    res = [run_es(x.clone(), target.clone(), SR, E.make_plugins("eq"), None, None, distance="mrstft", popsize=4, max_iters=30, seed=3,
                  device_es=True, sync_every=k) for k in (1, 4, 30)]
    assert list(res[0]) == ["output_audio", "params", "fopt", "wopt", "fval_history", "wopt_history", "num_evals"]
    assert res[0]["fval_history"][0] == float("inf") and res[0]["wopt_history"][0] is None
    assert len(res[0]["fval_history"]) == (res[0]["num_evals"] - 4) // 4 and np.isfinite(res[0]["fopt"])
    assert _same(res[0], res[1]) and _same(res[0], res[2])
    assert "Iterat #Fevals" in capsys.readouterr().out


def test_early_stop_counts_like_the_host(dev, short_pair):
    from st_ito import effects as E
    from st_ito.style_transfer import run_es
    _, target = short_pair
    silent = torch.zeros(1, 1, 24000)
    kw = dict(distance="mrstft", popsize=4, max_iters=30, seed=3, early_stop=True)
    host = run_es(silent.clone(), target.clone(), SR, E.make_plugins("eq"), None, None, **kw)
    got = run_es(silent.clone(), target.clone(), SR, E.make_plugins("eq"), None, None, device_es=True, sync_every=4, **kw)
    assert got["num_evals"] == host["num_evals"] == 4 + 12 * 4   # find_w0, then iteration 0 and eleven stale ones
    assert len(got["fval_history"]) == len(host["fval_history"])


def test_a_frozen_state_ignores_ask_and_tell(dev):
    d = _device(np.full(6, 0.5), 0.2, 8, max_iters=40, early_stop=True)
    f = torch.full((8,), 1.0, device=dev)
    for _ in range(12):
        d.ask_device()
        d.tell_device(f)
    assert d.status() == {"iterations": 12, "stale": 11, "stopped": True, "counteval": 96}
    s, W = d.export(), d.W.clone()
    for _ in range(3):
        d.ask_device()
        d.tell_device(f - 5.0)
    d.eigen_device()   # the forced decomposition honours the freeze too
    assert _same(s, d.export()) and torch.equal(W, d.W)
    # a state that has logged max_iters iterations is frozen the same way
    d = _device(np.full(6, 0.5), 0.2, 8, max_iters=2)
    for k in range(4):
        d.ask_device()
        d.tell_device(f - k)
        if k == 1:
            s = d.export()
    assert _same(s, d.export()) and d.status()["iterations"] == 2


def test_a_tell_without_an_ask_stores_nothing(dev):
    """Through the C ABI, past the wrapper's own check: after a tell the genotype words are spent, and a second tell must not
    update from them."""
    from st_ito import _hip
    d = _device(np.full(6, 0.5), 0.2, 8, max_iters=4)
    f = torch.arange(8, device=dev, dtype=torch.float32)
    d.ask_device()
    d.tell_device(f)
    s = d.export()
    assert s["asked"] == 0 and s["done"] == 1
    _hip.check(_hip.lib().stito_cmaes_tell(_hip.ptr(d.state), *d._dims, _hip.ptr(f), _hip.stream_ptr()))
    assert _same(s, d.export())
    d.ask_device()
    assert d.export()["asked"] == 1


def test_a_captured_iteration_replays(dev):
    """ask -> fitness -> tell captured into one hipGraph after an eager iteration (which sets the decomposition kernel's LDS
    attribute): nothing host-side changes between iterations -- the iteration number lives in the state -- so three replays are
    three iterations, bit for bit those of eager launches."""
    N, lam = 37, 32
    x0 = 0.2 + 0.6 * np.random.default_rng(3).random(N)
    a, b = _device(x0, 0.3, lam, max_iters=8), _device(x0, 0.3, lam, max_iters=8)

    def step(d):
        W = d.ask_device()
        d.tell_device(((W - 0.3) ** 2).sum(dim=1).float())

    step(a)
    step(b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(a)
    for _ in range(3):
        g.replay()
        step(b)
    sa, sb = a.export(), b.export()
    assert sa["done"] == sb["done"] == 4 and sa["countiter"] == 4
    assert _same(sa, sb) and torch.equal(a.W, b.W)


# ---- 9. it optimises -----------------------------------------------------------------------------------------------------------
def test_it_optimises(dev):
    from st_ito import effects as E
    from st_ito.engine import MrstftEvaluator
    from st_ito.style_transfer import process_audio, run_es
    spec = [("Gain", E.BasicGain, 1), ("ParametricEQ", E.BasicParametricEQ, 1)]
    x = O.synth_audio(77, 1, 24000)[None]
    target = torch.from_numpy(process_audio(x[0].numpy(), np.random.default_rng(9).random(19), SR, E.make_plugins(spec)))[None]
    kw = dict(distance="mrstft", popsize=16, max_iters=40, seed=5, find_w0=False, early_stop=False)
    xin, tin = x.clone(), target.clone()
    host = run_es(xin, tin, SR, E.make_plugins(spec), None, None, **kw)
    got = run_es(x.clone(), target.clone(), SR, E.make_plugins(spec), None, None, device_es=True, **kw)
    f0 = float(MrstftEvaluator(xin, SR, E.make_plugins(spec), tin).evaluate([np.full(19, 0.5)])[0][0])
    R.report(f"it optimises (gain + eq, popsize 16, 40 iterations): f(w0) {f0:.4f}  host fopt {host['fopt']:.4f}  device fopt {got['fopt']:.4f}")
    assert host["fopt"] < f0
    assert f0 - got["fopt"] >= 0.5 * (f0 - host["fopt"])
    assert got["num_evals"] == host["num_evals"] == 640


# ---- 10. device W into the evaluators ------------------------------------------------------------------------------------------
def _refusals(ev, D, dev):
    for bad in (torch.rand(4, D + 1, dtype=torch.float64, device=dev), torch.rand(D, dtype=torch.float64, device=dev)):
        with pytest.raises(ValueError, match=rf"parameter vectors must be \(P, {D}\)"):
            ev.evaluate(bad)
    with pytest.raises(ValueError, match=rf"parameter vectors must be \(P, {D}\)"):
        ev.evaluate(np.zeros((4, D + 1)))
    for bad in (torch.rand(4, D, dtype=torch.float32, device=dev), torch.rand(4, D, dtype=torch.float64),
                torch.rand(D, 4, dtype=torch.float64, device=dev).t()):
        with pytest.raises(ValueError, match="contiguous .* float64 tensor on the GPU"):
            ev.evaluate(bad)


def test_device_W_into_the_mrstft_evaluator(dev, short_pair):
    from st_ito import effects as E
    from st_ito.engine import MrstftEvaluator
    x, target = short_pair
    ev = MrstftEvaluator(x, SR, E.make_plugins("eq"), target)
    W = np.random.default_rng(2).random((6, 18))
    a = ev.evaluate(W, parallel=True)[0]
    b = ev.evaluate(torch.from_numpy(W).to(dev), parallel=True)[0]
    assert torch.equal(a, b)
    _refusals(ev, 18, dev)


def test_device_W_into_the_population_evaluator(dev):
    from st_ito import effects as E
    from st_ito.engine import PopulationEvaluator
    from st_ito.utils import get_param_embeds, make_synthetic_param_model
    pm = make_synthetic_param_model(0).to(dev)
    x, tgt = O.synth_audio(31, 2, 70000)[None], O.synth_audio(32, 2, 70000)[None]
    te = get_param_embeds(tgt, pm, SR)
    pp = E.make_plugins("eq")
    W = np.random.default_rng(1).random((5, 18))
    Wd = torch.from_numpy(W).to(dev)
    eager = PopulationEvaluator(x, SR, pp, pm, te, use_graph=False)
    la, ea, _ = eager.evaluate(W)
    lb, eb, _ = eager.evaluate(Wd)
    assert torch.equal(la, lb) and torch.equal(ea["mid"], eb["mid"]) and torch.equal(ea["side"], eb["side"])
    graph = PopulationEvaluator(x, SR, pp, pm, te, use_graph=True, capture_after=0)
    for _ in range(2):   # the capturing call, then a replay
        lg, eg, _ = graph.evaluate(Wd)
        assert graph._graphs and torch.equal(la, lg) and torch.equal(ea["mid"], eg["mid"])
    ln, _, _ = graph.evaluate(W)
    assert torch.equal(la, ln)
    _refusals(eager, 18, dev)
