"""CPU tests of the ragged multi-pair batch's host side: the crop rule, the group planner, the length policy and the argument
checks of both evaluators, and the list-form validation of run_es_batch (all of which run before anything touches the GPU)."""
import numpy as np
import pytest
import torch

CROP, MARGIN = 262144, 16384
LENGTHS = [1000, CROP, CROP + MARGIN, CROP + MARGIN + 1, 600000]


class _CountingRng:
    """A RandomState that counts its randint calls."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.calls = []

    def randint(self, lo, hi):
        self.calls.append((lo, hi))
        return self.rs.randint(lo, hi)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("random_crop", [False, True])
def test_crop_start_is_the_literal_rule(n, random_crop):
    from st_ito.engine import CROP_LEN, crop_start
    assert CROP_LEN == CROP
    rng, ref = _CountingRng(7), np.random.RandomState(7)
    got = [crop_start(n, random_crop, rng) for _ in range(5)]
    if random_crop and n - CROP > MARGIN:
        want = [int(ref.randint(MARGIN, n - CROP)) for _ in range(5)]
        assert rng.calls == [(MARGIN, n - CROP)] * 5
        assert all(MARGIN <= s < n - CROP for s in got)
    else:
        want = [0] * 5
        assert rng.calls == []       # a pair that needs no draw consumes none
    assert got == want and all(type(s) is int for s in got)


def test_crop_start_draw_sequence_interleaves_with_pairs_that_draw_nothing():
    """Two pairs on ONE seeded generator: the short one must leave the long one's sequence untouched."""
    from st_ito.engine import crop_start
    rng, ref = np.random.RandomState(11), np.random.RandomState(11)
    got = []
    for _ in range(4):
        assert crop_start(270000, True, rng) == 0      # spare 7856 <= 16384: cropped at 0, no draw
        assert crop_start(1000, True, rng) == 0
        got.append(crop_start(400000, True, rng))
    assert got == [int(ref.randint(MARGIN, 400000 - CROP)) for _ in range(4)]
    # the smallest input that draws has exactly one possible start
    assert crop_start(CROP + MARGIN + 1, True, np.random.RandomState(0)) == MARGIN


def _bare_evaluator(name, x, ndims=3):
    """An evaluator without the library: only what its length policy and its argument checks read."""
    from st_ito import engine
    ev = object.__new__(getattr(engine, name))
    ev.x_full, ev._x_padded, ev.n_inputs, ev.ndims = x, None, x.shape[0], ndims
    if name == "MrstftEvaluator":
        ev.y_full, ev._y_padded = x + 0.5, None
    return ev


def _span_case(evaluator, n, random_crop, parallel):
    """An evaluator's own audio under the length policy (CPU tensors: the methods only slice and pad) against the two pure
    functions on a twin generator: the same samples -- for input and target alike -- and the same NUMBER of draws: afterwards
    the generators are in the same state."""
    from st_ito.engine import crop_start, eval_length
    x = torch.arange(2 * n, dtype=torch.float32).reshape(1, 2, n)
    ev = _bare_evaluator(evaluator, x)
    both = evaluator == "MrstftEvaluator"
    full = (x, ev.y_full) if both else (x,)
    rng, twin = np.random.RandomState(3), np.random.RandomState(3)
    outs = []
    for _ in range(3):
        got = ev._input_and_target(random_crop, rng, parallel)[:2] if both else (ev._input(random_crop, rng, parallel),)
        outs.append(got)
        if parallel:                                   # the pool branch: the audio as it is, nothing drawn
            assert all(g is f for g, f in zip(got, full))
        else:
            s, length = crop_start(n, random_crop, twin), eval_length(n, random_crop)
            for f, g in zip(full, got):
                want = f[..., s:s + length]
                want = torch.nn.functional.pad(want, (0, length - want.shape[-1]))
                assert g.shape == want.shape and torch.equal(g, want) and g.is_contiguous()
        a, b = rng.get_state(), twin.get_state()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    for k, f in enumerate(full):
        if not parallel and n < CROP:
            assert outs[0][k] is outs[1][k] is outs[2][k]      # padded once: a captured graph reads the buffer by address
        if not parallel and (n == CROP or (n > CROP and not random_crop)):
            assert outs[0][k] is f                             # returned as it is, without a copy


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("random_crop", [False, True])
@pytest.mark.parametrize("parallel", [False, True])
def test_evaluator_input_is_crop_start_and_eval_length(n, random_crop, parallel):
    """PopulationEvaluator._input."""
    _span_case("PopulationEvaluator", n, random_crop, parallel)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("random_crop", [False, True])
@pytest.mark.parametrize("parallel", [False, True])
def test_mrstft_evaluator_cuts_input_and_target_to_one_span(n, random_crop, parallel):
    """MrstftEvaluator._input_and_target: the same test, and the target receives the samples that the input receives."""
    _span_case("MrstftEvaluator", n, random_crop, parallel)


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the checks of a ready-made buffer then see its dtype, layout and shape."""
    is_cuda = property(lambda self: True)


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)


# (W, pairs, x, y) -> the ValueError; two inputs of 2 channels, 3 parameters
BAD_ARGUMENTS = {
    "wrong width": ((np.zeros((4, 2)), None, None, None), r"parameter vectors must be \(P, 3\), got \(4, 2\)"),
    "not a matrix": ((np.zeros(3), None, None, None), r"parameter vectors must be \(P, 3\), got \(3,\)"),
    "empty population": ((np.zeros((0, 3)), None, None, None), "0 candidates cannot be split over 2 inputs"),
    "P no multiple of the pairs": ((np.zeros((5, 3)), None, None, None), "5 candidates cannot be split over 2 inputs"),
    "P no multiple of the listed pairs": ((np.zeros((4, 3)), [1, 0, 1], None, None), "4 candidates cannot be split over 3 inputs"),
    "pair out of range": ((np.zeros((4, 3)), [0, 2], None, None), r"pairs \[0, 2\] do not name inputs 0 \.\. 1"),
    "negative pair": ((np.zeros((4, 3)), [-1], None, None), r"pairs \[-1\] do not name inputs 0 \.\. 1"),
    "empty pair list": ((np.zeros((4, 3)), [], None, None), r"pairs \[\] do not name inputs 0 \.\. 1"),
    "x leading dimension": ((np.zeros((4, 3)), [1], _gpu(2, 2, 64), None), r"x must be a contiguous \(1, chs, n\) float32 tensor on the GPU"),
    "x leading dimension, all pairs": ((np.zeros((4, 3)), None, _gpu(1, 2, 64), None), r"x must be a contiguous \(2, chs, n\) float32"),
    "x dtype": ((np.zeros((4, 3)), None, _gpu(2, 2, 64, dtype=torch.float64), None), r"x must be a contiguous \(2, chs, n\) float32"),
    "x not contiguous": ((np.zeros((4, 3)), None, _gpu(2, 2, 128)[..., ::2], None), r"x must be a contiguous \(2, chs, n\) float32"),
    "x not on the GPU": ((np.zeros((4, 3)), None, torch.zeros(2, 2, 64), None), r"x must be a contiguous \(2, chs, n\) float32"),
    "y without x": ((np.zeros((4, 3)), [0, 1], None, _gpu(2, 2, 64)), r"y \(ready-made target spans\) needs x"),
    "y of another length": ((np.zeros((4, 3)), [0, 1], _gpu(2, 2, 64), _gpu(2, 2, 63)), "y has 63 samples, x 64"),
    "y leading dimension": ((np.zeros((4, 3)), [0], _gpu(1, 2, 64), _gpu(2, 2, 64)), r"y must be a contiguous \(1, chs, n\) float32 tensor on the GPU"),
}


@pytest.mark.parametrize("evaluator,case", [(ev, case) for case, (args, _) in BAD_ARGUMENTS.items()
                                            for ev in ("PopulationEvaluator", "MrstftEvaluator")
                                            if args[3] is None or ev == "MrstftEvaluator"])      # only MrstftEvaluator takes y
def test_evaluators_refuse_the_same_arguments_with_the_same_words(evaluator, case):
    """Both evaluators, built without the library, are fed the same bad W / pairs / x (and y, for the one that takes it): the
    same ValueError from both, raised before anything is drawn from the generator or asked of a GPU."""
    (W, pairs, x, y), text = BAD_ARGUMENTS[case]
    ev = _bare_evaluator(evaluator, torch.zeros(2, 2, 300000))        # long enough for random_crop to draw a start
    rng = _CountingRng(0)
    with pytest.raises(ValueError, match=text):
        ev.evaluate(W, random_crop=True, rng=rng, pairs=pairs, x=x, **({} if y is None else {"y": y}))
    assert rng.calls == []


def test_eval_length_and_group_planner():
    from st_ito.engine import eval_length, plan_ragged_groups
    for n in LENGTHS:
        assert eval_length(n, True) == CROP
        assert eval_length(n, False) == (CROP if n <= CROP else n)
    assert plan_ragged_groups([200000, 270000, 400000, 1000], True) == [(CROP, [0, 1, 2, 3])]   # random_crop: one group
    assert plan_ragged_groups([300000, 300000, 350000], False) == [(300000, [0, 1]), (350000, [2])]
    # short files (and files of exactly 262144 samples) join the 262144 group; groups come in order of their first pair
    assert plan_ragged_groups([300000, 1000, CROP, 300000, 200000], False) == [(300000, [0, 3]), (CROP, [1, 2, 4])]
    assert plan_ragged_groups([5], False) == [(CROP, [0])]
    with pytest.raises(ValueError):
        plan_ragged_groups([1000, 0], True)


def test_list_form_validation_raises_before_any_gpu_call(monkeypatch):
    from st_ito import _hip, engine
    from st_ito.style_transfer import run_es_batch

    def no_gpu(*a, **k):
        raise AssertionError("validation must not reach the GPU")

    monkeypatch.setattr(_hip, "lib", no_gpu)
    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    monkeypatch.setattr(engine, "PopulationEvaluator", no_gpu)
    embed = no_gpu
    st = lambda n: torch.zeros(1, 2, n)                     # noqa: E731
    call = lambda xs, ts: run_es_batch(xs, ts, 48000, {}, None, embed, max_iters=1, popsize=4)   # noqa: E731
    with pytest.raises(ValueError, match="2 inputs but 1 targets"):
        call([st(100), st(200)], [st(100)])
    with pytest.raises(ValueError, match="empty"):
        call([], [])
    with pytest.raises(ValueError, match="mixed channel counts"):
        call([st(100), torch.zeros(1, 1, 200)], [st(100), st(50)])
    with pytest.raises(ValueError, match="both be lists"):
        call([st(100)], torch.zeros(1, 2, 100))
    with pytest.raises(ValueError, match="input 1"):
        call([st(100), torch.zeros(2, 2, 100)], [st(100), st(100)])     # a batch of two is not one pair
    with pytest.raises(ValueError, match="target 0"):
        call([st(100)], [torch.zeros(100)])
    with pytest.raises(ValueError, match="input 0"):
        call([torch.zeros(2, 0)], [st(100)])


def test_binding_declares_the_gather_symbol():
    from st_ito import _hip
    assert "stito_gather_crops" in _hip.SIGNATURES and len(_hip.SIGNATURES["stito_gather_crops"][1]) == 12
    lib = _hip.lib()
    assert lib.stito_version_minor() >= 1
    # argument checks happen on the host, before any launch
    assert lib.stito_gather_crops(None, 0, None, None, None, 0, None, 0, 2, 4, None, None) == _hip.E_INVALID
    assert b"stito_gather_crops" in lib.stito_last_error()
