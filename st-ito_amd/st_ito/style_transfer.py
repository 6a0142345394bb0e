"""Inference-time optimisation (ES) of the reference, st_ito/style_transfer.py: `load_plugins`
(17-42), `process_audio` (45-115), `parameters_to_dict` (324-359), `savepop_to_disk` (362-396)
and `run_es` (399-692), with the evaluate-population step on the MI355X; `run_staged_es` is the fixed variant
of scripts/run_optim.py:39-234 on the same evaluate step.

The baselines of the production-style-transfer benchmark are built too: `run_input` (116-135), `run_random` (138-160:
one random parameter vector through the GPU render) and `run_rule_based` (163-278: matched-EQ design and FIR filtering,
then a compressor threshold hill-climb, every item of the batch at once on the GPU -- csrc/matcheq.hip, st_ito.matcheq),
with the reference's `get_average_spectrum` and `smooth_spectrum`.  `run_deepafx_st` is not: it needs a trained
DeepAFx-ST checkpoint and its package.  `run_es_batch` is an extension (BASELINE.json configs[2]): several (input,
target) pairs optimised together, every iteration evaluating their populations in one GPU batch (or one per input length).

The three ES drivers share one statement of each rule: `_EsRun` is one CMA-ES trajectory with the reference's bookkeeping
(617-670: pre-tell histories, evaluation count, the stale counter of the early stop) and the result dict; `_agree_on_seed`,
`_peak_normalize_` and `_chain_dims` are the steps every driver takes before its first iteration.  `run_es` steps one `_EsRun`,
`run_es_batch` a list of them, `run_staged_es` builds one per stage and keeps run_optim.py's own post-tell histories.  The
objective (`distance`) is likewise said once for all three: `_check_distance`, `_check_mrstft_pairs` (what distance="mrstft"
and "mrstft-sd" ask of a pair) and `_make_evaluator`, the one place that picks the engine's evaluator; the loops see losses only.
"""
from __future__ import annotations

import os
from typing import List

import numpy as np
import torch

from . import cmaes as cma
from . import engine


# ------- audio processing methods -------
def load_plugins(plugins: dict):
    """Instantiate every plugin of the dict and record its parameter layout (reference style_transfer.py:17-42).

    Fills plugin["instance"], plugin["parameter_names"] -- the (dead) "our_bypass" slot first, then the instance's
    parameters in their own order -- and plugin["num_params"]; returns (plugins, total number of slots, the initial raw
    values slot by slot), printing each parameter like the reference does."""
    init_params: List[float] = []
    for plugin_name, plugin in plugins.items():
        if "vst_filepath" in plugin:
            raise NotImplementedError("VST plugins (pedalboard.load_plugin) are not supported in this build")
        if "class_path" not in plugin:
            raise ValueError("Plugin must contain 'vst_filepath' or 'class_path'.")
        instance = plugin["class_path"]()
        raw = {name: prm.raw_value for name, prm in instance.parameters.items()}
        for name, value in raw.items():
            print(f"{plugin_name}: {name} = {value}")
        print()
        plugin["instance"] = instance
        plugin["parameter_names"] = ["our_bypass", *raw]
        plugin["num_params"] = 1 + len(raw)
        init_params += [0.0, *raw.values()]
    return plugins, len(init_params), init_params


def process_audio(x: np.ndarray, w: np.ndarray, sr: int, plugins: List[dict], normalize_stages: bool = False):
    """Process audio with plugins and provided parameters on [0, 1] (reference
    style_transfer.py:45-115).  x: (chs, num_samples) float32, w: (num_params,).  Rendered on the
    GPU by stito_render_population + stito_normalize_audio; normalize_stages (106-107) adds a joint
    peak normalisation after every plugin (STITO_FX_FLAG_NORMALIZE_AFTER)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().numpy()
    out = engine.process_audio_gpu(x, w, sr, plugins, normalize_stages=normalize_stages)
    # side effect of the reference's loop (71-87): the plugin instances end up holding the values they were rendered with (raw
    # slot for a free parameter, set_value of the fixed one) -- scripts/eval/eval_case_study.py:372-388 reads them back after a
    # dummy call.  The GPU render takes its values from w, so they are written here, on the host.
    _write_parameters(w, plugins)
    return out


def _write_parameters(w, plugins):
    """Walk w over the plugins' slots and leave every value in its Parameter; -> the values in the parameters' own units."""
    values = {}
    slot = iter(w)
    for plugin_name, plugin in plugins.items():
        mine = values.setdefault(plugin_name, {})
        fixed = plugin["fixed_parameters"]
        for name in plugin["parameter_names"]:
            raw = next(slot)  # every name consumes its slot, fixed or not
            if name == "our_bypass":
                mine[name] = raw
                continue
            prm = engine._instance_of(plugin).parameters[name]
            if name in fixed:
                prm.set_value(fixed[name])
            else:
                prm.raw_value = raw
            mine[name] = prm.get_value() if hasattr(prm, "get_value") else prm.raw_value
    return values


def parameters_to_dict(w: np.ndarray, plugins: List[dict]):
    """{plugin: {parameter: value in its own unit}} for a vector on [0, 1] (reference style_transfer.py:324-359).

    Like the reference this WRITES the values into the plugin instances on the way (raw value for a free slot,
    `set_value` of the fixed value for a fixed one); "our_bypass" is reported as the raw slot."""
    return _write_parameters(w, plugins)


def savepop_to_disk(iteration, fvals, output_embeds, output_audios, run_dir: str, sample_rate: int, first: int = 0):
    """reference style_transfer.py:362-396: one wav per candidate, sorted by fitness.

    `fvals` is the full population's fitness; `output_audios` holds candidates [first, first + len)
    of it -- under torch.distributed every rank passes its own shard and writes only its own
    candidates' files, named by their rank in the global ordering, so the directory ends up with the
    same files a single process writes (no audio is communicated).

    STATED DEVIATION, one switch away from parity: the reference zips (fvals, output_audios, output_embeds) and run_es hands
    it the embedding DICT, whose iteration yields its keys -- so the reference writes only as many files as the dict has
    entries (two for AFx-Rep: candidates 0 and 1 of the population, ranked among themselves).  The default here writes the
    whole population, which is what the flag promises; STITO_SAVEPOP_REFERENCE=1 reproduces the reference's files exactly
    (tests/test_host_logic.py against a fixture the reference's own function produced)."""
    from .audio_io import save_wav

    pop_dir = os.path.join(run_dir, f"pop_{iteration}")
    os.makedirs(pop_dir, exist_ok=True)
    members = range(len(fvals))
    if os.environ.get("STITO_SAVEPOP_REFERENCE") == "1":
        members = range(min(len(fvals), len(output_embeds)))   # zip() stops at the shortest: the dict's keys
    order = sorted(members, key=lambda i: fvals[i])
    for idx, i in enumerate(order):
        if not first <= i < first + len(output_audios):
            continue
        audio = output_audios[i - first]
        audio = audio / torch.max(torch.abs(audio)).clamp(min=1e-8)
        save_wav(os.path.join(pop_dir, f"output_audio_pop_{idx}_fval_{fvals[i]:0.4e}.wav"), audio.cpu(), sample_rate)


# ------ baselines of the PST benchmark ------
def run_input(input_audio: torch.Tensor, target_audio: torch.Tensor, sample_rate: int, plugins: List[dict], model: torch.nn.Module,
              *args, **kwargs):
    """The unprocessed input (reference style_transfer.py:121-135)."""
    bs, chs, seq_len = input_audio.shape
    return {"output_audio": input_audio}


def run_random(input_audio: torch.Tensor, target_audio: torch.Tensor, sample_rate: int, plugins: List[dict], model: torch.nn.Module,
               *args, **kwargs):
    """One random parameter vector (reference style_transfer.py:138-160): w = torch.rand(total_num_params) from torch's global
    CPU generator, rendered by process_audio on the GPU.  input_audio (1, chs, seq_len)."""
    bs, chs, seq_len = input_audio.shape
    total_num_params = sum([plugin["num_params"] for plugin in plugins.values()])
    w = torch.rand(total_num_params)
    output_audio = process_audio(input_audio.squeeze(0), w.numpy(), sample_rate, plugins)
    output_audio = torch.from_numpy(output_audio).unsqueeze(0)
    return {"output_audio": output_audio, "param_dict": parameters_to_dict(w.numpy(), plugins)}


def smooth_spectrum(H):
    """scipy.signal.savgol_filter(H, 1025, 2) (reference style_transfer.py:163-165) of a spectrum or a (rows, bins) stack, on the
    GPU (float64 sums, float32 result).  A numpy array comes back as a numpy array, a tensor as a tensor on its device."""
    from . import matcheq

    as_numpy = not isinstance(H, torch.Tensor)
    h = torch.as_tensor(np.asarray(H) if as_numpy else H)
    dev = h.device if h.is_cuda else engine._current_device()
    rows = h.detach().to(dev, torch.float32).reshape(-1, h.shape[-1]).contiguous()
    out = matcheq.savgol(rows).reshape(h.shape)
    return out.cpu().numpy() if as_numpy else out.to(h.device)


def get_average_spectrum(x: torch.Tensor, n_fft: int = 16384):
    """Mean over STFT frames of |X| (reference style_transfer.py:168-181): x (chs, seq_len), a stereo signal averaged to mono
    first; torch.stft(n_fft, hop n_fft // 4, rectangular window, centred, reflect pad, normalized=True).  Prints x.shape like
    the reference.  -> (n_fft // 2 + 1,) float32 on x's device, computed on the GPU."""
    from . import matcheq

    print(x.shape)
    _check_rule_based_shape(x[None], n_fft, None, "x")
    dev = x.device if x.is_cuda else engine._current_device()
    xs = x.detach().to(dev, torch.float32)[None].contiguous()
    return matcheq.mean_spectrum(xs, n_fft)[0].to(x.device)


def _check_rule_based_shape(x: torch.Tensor, n_fft: int, sample_rate, name: str):
    """The shapes run_rule_based can process: (bs, 1 or 2, n) with n > n_fft / 2 (reflect padding) and, for the loudness meter,
    n >= 0.4 s."""
    if x.dim() != 3:
        raise ValueError(f"{name}: expected (bs, chs, seq_len), got {tuple(x.shape)}")
    bs, chs, n = x.shape
    if chs not in (1, 2):
        raise ValueError(f"{name}: {chs} channels; the matched EQ is defined for mono or stereo audio")
    if n_fft & (n_fft - 1) or not 2048 <= n_fft <= 32768:
        raise NotImplementedError(f"n_fft {n_fft}: only powers of two in [2048, 32768] are built")
    if n <= n_fft // 2:
        raise ValueError(f"{name}: {n} samples; reflect padding needs more than n_fft // 2 = {n_fft // 2}")
    if sample_rate is not None and n < 0.400 * sample_rate:
        raise ValueError(f"{name}: {n} samples are shorter than the loudness meter's 400 ms block")


def run_rule_based(input_audio: torch.Tensor, target_audio: torch.Tensor, sample_rate: int, plugins: List[dict],
                   model: torch.nn.Module, n_fft: int = 16384, n_taps: int = 2048, **kwargs):
    """Rule-based style transfer baseline (reference style_transfer.py:184-278): per item, a matched EQ -- the ratio of the
    target's and the input's smoothed average spectra, designed as an n_taps linear-phase FIR by firwin2 and applied to every
    channel -- then a compressor (ratio 3, attack 1 ms, release 100 ms) whose threshold walks down from 0 dB in 0.5 dB steps,
    each pass compressing the previous pass's output, until the output is within 0.25 LU of the target's loudness or the
    threshold reaches -80 dB.

    Like the reference, every item of input_audio and target_audio is peak-normalised to -12 dBFS IN PLACE first.  From
    there the audio stays on the GPU and all items run together (the hill-climb in lockstep, each item with its own
    threshold and stopping step).  plugins and model are not used.  -> {"output_audio": (bs, chs, seq_len) float32 CPU}."""
    from . import matcheq

    _check_rule_based_shape(input_audio, n_fft, sample_rate, "input_audio")
    _check_rule_based_shape(target_audio, n_fft, sample_rate, "target_audio")
    bs = input_audio.shape[0]
    if target_audio.shape[0] != bs:
        raise ValueError(f"input_audio has {bs} items, target_audio {target_audio.shape[0]}")
    if not 16 <= n_taps <= 4096:
        raise NotImplementedError(f"n_taps {n_taps}: only 16 .. 4096 are built")
    dev = engine._current_device()

    def normalised(a):  # peak normalise to -12 dBFS on the GPU, then write back into the caller's tensor
        g = matcheq.peak_normalize_(a.detach().to(dev, torch.float32).contiguous())
        if g.data_ptr() != a.data_ptr():
            with torch.no_grad():
                a.copy_(g)
        return g

    xs, ts = normalised(input_audio), normalised(target_audio)
    for b in range(bs):  # get_average_spectrum prints the shape of every signal it is given
        print(input_audio[b].shape)
        print(target_audio[b].shape)
    # ------------ design the matched EQ ------------
    sm = matcheq.savgol(torch.cat([matcheq.mean_spectrum(ts, n_fft), matcheq.mean_spectrum(xs, n_fft)]))
    taps = matcheq.firwin2(sm[:bs].contiguous(), sm[bs:].contiguous(), sample_rate, n_taps)
    y = matcheq.peak_normalize_(matcheq.fir(xs, taps))
    # ------------ dynamics: the threshold hill-climb ------------
    matcheq.hill_climb_(y, matcheq.lufs_raw(y, sample_rate), matcheq.lufs_raw(ts, sample_rate), sample_rate)
    return {"output_audio": y.cpu()}


# ----------- Evolutionary Strategies ------------
def _dist_info():
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def shard_bounds(popsize: int, rank: int, world: int):
    """Candidates [lo, hi) of the ask() batch owned by `rank` (contiguous, near-equal shards)."""
    base, rem = divmod(popsize, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_fitness(local: torch.Tensor, popsize: int) -> torch.Tensor:
    """All-gather the per-rank fitness shards into candidate order (RCCL when the tensors are on
    the GPU, gloo on CPU).  Shards may differ by one element, so pad to the largest."""
    dist, rank, world = _dist_info()
    # a one-rank group skips the collective unless STITO_FORCE_COLLECTIVE=1 (tests/test_gpu_es.py pushes a step through RCCL's
    # communicator setup and all_gather_into_tensor on the one GPU a test box has)
    if world == 1 and not (dist is not None and os.environ.get("STITO_FORCE_COLLECTIVE") == "1"):
        return local
    per = (popsize + world - 1) // world
    buf = torch.full((per,), float("inf"), dtype=local.dtype, device=local.device)
    buf[: local.numel()] = local
    out = torch.empty((world, per), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out.view(-1), buf)
    parts = []
    for r in range(world):
        lo, hi = shard_bounds(popsize, r, world)
        parts.append(out[r, : hi - lo])
    return torch.cat(parts)


def sharded_evaluate(W, eval_local, while_waiting=None):
    """Evaluate a population across the ranks of the default process group.

    `eval_local(W_shard) -> (loss tensor (n_local,), embeds, audios)` is called with this rank's
    contiguous shard of W; the per-rank fitness vectors are all-gathered into candidate order, so
    every rank returns the same full fitness list (and its own shard's embeds/audios).  `while_waiting()` runs on the host
    after the shard's GPU work has been queued and before the fitness download waits for it."""
    _, rank, world = _dist_info()
    P = len(W)
    lo, hi = shard_bounds(P, rank, world)
    loss, embeds, audios = eval_local(W[lo:hi])
    if while_waiting is not None:
        while_waiting()
    return gather_fitness(loss, P).tolist(), embeds, audios


def _agree_on_seed(seed):
    """`seed`, or for an unseeded run under torch.distributed a seed that rank 0 draws and broadcasts: the ranks step replicas of
    one CMA-ES state (or own different pairs whose seeds must not depend on the sharding), so every seeded draw -- CMA-ES,
    find_w0, crop positions -- has to agree.  A single-rank run enters no collective and stays unseeded."""
    dist, rank, world = _dist_info()
    if world > 1 and seed is None:
        box = [int(np.random.SeedSequence().generate_state(1)[0] & 0x7FFFFFFF) if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        seed = box[0]
    return seed


def _peak_normalize_(audio: torch.Tensor) -> torch.Tensor:
    """In place: audio /= max|audio| (reference 452-453)."""
    audio /= torch.max(torch.abs(audio)).clamp(min=1e-8)
    return audio


def _chain_dims(evaluator, plugins) -> int:
    """Number of parameter slots of the plugins, which must be what the compiled chain consumes."""
    total_num_params = sum([plugin["num_params"] for plugin in plugins.values()])
    if evaluator.ndims != total_num_params:
        raise ValueError(f"plugins declare {total_num_params} params, chain consumes {evaluator.ndims}")
    return total_num_params


def _es_result(output_audio, wopt, fopt, fval_history, wopt_history, num_evals, plugins, **extra):
    """The dict every ES driver returns; a driver's own entries (run_staged_es: stage_wopts) go in front of num_evals."""
    return {
        "output_audio": output_audio,
        "params": parameters_to_dict(wopt, plugins),
        "fopt": fopt,
        "wopt": wopt,
        "fval_history": fval_history,
        "wopt_history": wopt_history,
        **extra,
        "num_evals": num_evals,
    }


class _EsRun:
    """One CMA-ES trajectory and its bookkeeping (reference 614-673): the strategy, the population of the last ask(), the
    histories, the evaluation count and the early-stop counter.  Every driver steps its trajectories through this class, which
    is what makes "pair b of a batch is bitwise the run_es of pair b alone" a matter of construction."""

    @staticmethod
    def strategy(w0, sigma0, popsize, seed):
        """The CMA-ES of the reference (614, 624): bounds [0, 1], seeded when a seed is given."""
        opts = {"bounds": [0, 1], "popsize": popsize}
        if seed is not None:
            opts["seed"] = seed
        return cma.CMAEvolutionStrategy(w0, sigma0, opts)

    def __init__(self, w0, sigma0, popsize, seed):
        self.es = self.strategy(w0, sigma0, popsize, seed)
        self.W = None
        self.fval_history = []
        self.wopt_history = []
        self.n_evals = 0
        self.stale = 0          # consecutive iterations without improvement
        self.active = True      # a batch clears it when the pair stops early

    def ask(self):
        self.W = self.es.ask()
        return self.W

    def tell(self, fvals, iteration) -> bool:
        """Record the best so far -- the PRE-tell result like the reference, so entry 0 is (None, inf) -- then tell.  -> whether
        the iteration was stale (reference 655-670): its best candidate did not beat the best value on record by more than 0.01;
        the first iteration never counts."""
        self.n_evals += len(self.W)
        self.wopt_history.append(self.es.result[0])
        self.fval_history.append(self.es.result[1])
        self.es.tell(self.W, fvals)
        stale = iteration > 0 and min(fvals) - min(self.fval_history) > -0.01
        self.stale = self.stale + 1 if stale else 0
        return stale

    def result(self, output_audio, plugins):
        """The result dict, given the render of the current solution es.result[0]."""
        wopt, fopt = self.es.result[0], self.es.result[1]
        return _es_result(output_audio, wopt, fopt, self.fval_history, self.wopt_history, self.n_evals, plugins)


def run_es(
    input_audio: torch.Tensor,
    target_audio: torch.Tensor,
    sample_rate: int,
    plugins: List[dict],
    model: torch.nn.Module,
    embed_func: callable,
    content_model: torch.nn.Module = None,
    content_embed_func: callable = None,
    max_iters: int = 100,
    w0: torch.Tensor = None,
    find_w0: bool = True,
    sigma0: float = 0.1,
    distance: str = "cosine",
    random_crop: bool = False,
    popsize: int = 32,
    parallel: bool = False,
    dropout: float = 0.0,
    savepop: bool = False,
    run_dir: str = ".",
    seed: int = None,
    early_stop: bool = True,
    device_es: bool = False,
    sync_every: int = 4,
    *args,
    **kwargs,
):
    """Run CMA-ES optimization to find the best parameters (reference style_transfer.py:399-692).

    Same arguments and result dict as the reference.  `parallel` selects the reference's pool branch (499-502), whose only
    observable difference is the length policy: the candidates are rendered from the input as it is (no zero padding to
    262144 samples, no random crop); the whole population is rendered on the GPU at once either way.  Extensions: `seed` (CMA-ES + find_w0 RNG; the
    reference is unseeded) and `early_stop` (False disables the break of lines 655-670 for fixed
    work benchmarks).  Under torch.distributed each rank evaluates a contiguous shard of the
    population and the fitness scalars are all-gathered; the CMA-ES state is replicated.

    device_es=True steps the CMA-ES on the GPU (cmaes.DeviceCMAEvolutionStrategy): ask -> evaluate -> tell are enqueued `sync_every`
    iterations at a time and the host reads one status record per batch, where it also prints the iterations' disp lines.  Same
    update rule, the library's own random stream: NOT the trajectory the host ES walks from the same seed.  Single rank only and no
    savepop; max_iters must be at least 1 (the host ES accepts 0); find_w0 is the host-drawn population it always was.  NaN
    warnings are printed once per batch, for all of its passes."""
    _check_distance(distance, sample_rate)
    if device_es:
        _check_device_es(plugins, popsize, max_iters, savepop, sync_every)
    if content_model is not None and content_embed_func is None:
        raise ValueError("content_model needs a content_embed_func")
    bs, chs, seq_len = input_audio.shape
    if distance in _AUDIO_DISTANCES:
        _check_mrstft_pairs(input_audio, target_audio, plugins, "the target", distance=distance)
        if content_model is not None:
            raise ValueError(f"distance '{distance}' has no embeddings: content_model cannot be used with it")
        if dropout > 0:
            raise ValueError(f"distance '{distance}' has no embeddings: dropout must be 0")
        _check_mrstft_savepop(savepop, distance)
    seed = _agree_on_seed(seed)
    rng = np.random.RandomState(seed) if seed is not None else np.random

    # peak normalize (in place like the reference, 452-453)
    _peak_normalize_(input_audio)
    _peak_normalize_(target_audio)

    options = dict(max_iters=max_iters, w0=w0, find_w0=find_w0, sigma0=sigma0, random_crop=random_crop, popsize=popsize,
                   parallel=parallel, dropout=dropout, savepop=savepop, run_dir=run_dir, seed=seed, rng=rng, early_stop=early_stop,
                   device_es=device_es, sync_every=sync_every)
    if distance in _AUDIO_DISTANCES:
        # the objective is the distance to the target AUDIO: no model, no embedding, nothing to compute once but the target's
        # magnitude table, which the evaluator builds for the span it evaluates
        evaluator = _make_evaluator(distance, input_audio, sample_rate, plugins, None, target_audio)
        return _es_loop(evaluator, input_audio, sample_rate, plugins, **options)

    # compute target embedding (only once)
    target_embed = embed_func(target_audio, model, sample_rate)

    # content branch (468-473, 537-542, 560-568): a second embedding of the same rendered audio, scored against the TARGET's
    # content embedding with twice the weight.  It rides on the generic-metric path: one embedding dict with the content
    # entries under a prefix, the mean over all entries with weight 2 on those.
    eval_embed_func, eval_targets, entry_weights = embed_func, target_embed, None
    _CP = "__content__:"
    if content_model is not None:
        target_content_embeds = content_embed_func(target_audio, content_model, sample_rate)
        eval_targets = dict(target_embed)
        eval_targets.update({_CP + k: v for k, v in target_content_embeds.items()})
        entry_weights = {_CP + k: 2.0 for k in target_content_embeds}

        def eval_embed_func(x, m, sr):
            e = dict(embed_func(x, m, sr))
            e.update({_CP + k: v for k, v in content_embed_func(x, content_model, sr).items()})
            return e

    # (run_optim.py:608 passes normalize_stages=...; the reference's run_es swallows it in **kwargs and its evaluate
    # never forwards it to process_audio, so the population is rendered without per-stage normalisation here too)
    evaluator = _make_evaluator(distance, input_audio, sample_rate, plugins, model, eval_targets, embed_func=eval_embed_func,
                                entry_weights=entry_weights)
    if content_model is not None:  # the reference hands back the style embeddings only (573)
        with_content = evaluator.evaluate

        def style_only(W, **kw):
            loss, embeds, audios = with_content(W, **kw)
            return loss, {k: v for k, v in embeds.items() if not k.startswith(_CP)}, audios

        evaluator.evaluate = style_only
    return _es_loop(evaluator, input_audio, sample_rate, plugins, **options)


def _check_device_es(plugins, popsize, max_iters, savepop, sync_every):
    """What run_es(device_es=True) refuses, said before an input is normalised or anything launched."""
    if _dist_info()[2] > 1:
        raise ValueError("device_es steps ONE CMA-ES state on one GPU: it cannot run under a torch.distributed world larger than 1")
    if savepop:
        raise ValueError("device_es keeps the populations on the device: savepop is not supported")
    if int(sync_every) < 1:
        raise ValueError(f"sync_every must be at least 1, got {sync_every}")
    if int(max_iters) < 1:
        raise ValueError(f"device_es logs its iterations in a state sized by max_iters: it must be at least 1, got {max_iters}")
    cma.device_es_state_bytes(sum(plugin["num_params"] for plugin in plugins.values()), popsize, max_iters)


# the objectives that compare the rendered AUDIO with the target's: "mrstft" channel by channel, "mrstft-sd" on [L + R, L - R],
# "mrstft-mel" channel by channel on mel-band sums of the magnitudes; "-aw": the same three on rows that went through the A-weighting
# FIR of the sample rate first (auraloss's perceptual_weighting=True; engine.PrefilteredMrstftEvaluator)
_PREFILTERED_DISTANCES = {"mrstft-aw": "lr", "mrstft-sd-aw": "sum-diff", "mrstft-mel-aw": "mel"}   # name -> the evaluator's kind
# the waveform distances (engine.WaveformEvaluator, csrc/waveform.hip): sample against sample, so polarity and alignment count;
# name -> (the evaluator's kind, its prefilter).  "dc" is a kind of features.compute_waveform_distance only.
_WAVEFORM_DISTANCES = {name + suffix: (name, prefilter) for suffix, prefilter in (("", None), ("-aw", "aw"))
                       for name in ("esr", "snr", "sisdr", "logcosh")}
_AUDIO_DISTANCES = ("mrstft", "mrstft-sd", "mrstft-mel") + tuple(_PREFILTERED_DISTANCES) + tuple(_WAVEFORM_DISTANCES)


def _check_distance(distance, sample_rate=None):
    """The name -- and, under "mrstft-mel" and "mrstft-mel-aw", the bank of the sample rate, built on the host: a band with no bin
    is a ValueError here, before an input is normalised or anything launched; so are the "-aw" taps of that rate."""
    if distance != "cosine" and distance not in _AUDIO_DISTANCES:
        raise ValueError(f"Unknown distance: {distance}")
    if distance in ("mrstft-mel", "mrstft-mel-aw"):
        from . import features

        features.mel_mrstft_bank(sample_rate)
    if distance in _PREFILTERED_DISTANCES or _WAVEFORM_DISTANCES.get(distance, (None, None))[1] == "aw":
        from . import features

        features.mrstft_prefilter("aw", sample_rate)


def _check_mrstft_pairs(input_audios, target_audios, plugins, target="target {b}", chain="the chain", distance="mrstft"):
    """The pair rule of the audio distances, said before anything is launched: they compare sample spans of the render and of
    the target, so a target has its input's length and the chain's output channel count -- which is 2 under "mrstft-sd", the
    distance of sums and differences of two channels.  input_audios / target_audios: lists of (chs, n), or the rows of (B, chs,
    n) tensors; target / chain: what the messages call the two sides."""
    if len(target_audios) != len(input_audios):
        raise ValueError(f"distance '{distance}': {len(input_audios)} inputs but {len(target_audios)} targets")
    for b, (x, t) in enumerate(zip(input_audios, target_audios)):
        who = target.format(b=b)
        if t.dim() != 2 or t.shape[-1] != x.shape[-1]:
            raise ValueError(f"distance '{distance}' compares sample spans: {who} {tuple(t.shape)} must have the length of its input "
                             f"{tuple(x.shape)}")
        c_out = engine.chain_out_channels(plugins, x.shape[0])
        if distance in ("mrstft-sd", "mrstft-sd-aw") and c_out != 2:
            raise ValueError(f"distance '{distance}' compares the sums and differences of 2 channels: {chain} renders {c_out} channels "
                             f"from input {b}'s {x.shape[0]}")
        if t.shape[0] != c_out:
            raise ValueError(f"distance '{distance}': {who} has {t.shape[0]} channels, {chain} renders {c_out}")


def _check_mrstft_savepop(savepop, distance="mrstft"):
    if savepop:
        raise ValueError(f"distance '{distance}' does not write populations: savepop is not supported")


def _make_evaluator(distance, x, sample_rate, plugins, model, target, **kw):
    """The one place that turns `distance` into an evaluator, both resolved through `engine` when called.  target: the target
    embeddings ("cosine"; kw: PopulationEvaluator's embed_func, entry_weights, use_graph) or the target audio ("mrstft",
    "mrstft-sd", "mrstft-mel" and their "-aw" forms, and the waveform distances "esr", "snr", "sisdr", "logcosh" with theirs, which
    embed nothing and launch eagerly: kw has nothing to say to them)."""
    if distance == "mrstft":
        return engine.MrstftEvaluator(x, sample_rate, plugins, target)
    if distance == "mrstft-sd":
        return engine.MrstftEvaluator(x, sample_rate, plugins, target, stereo="sum-diff")
    if distance == "mrstft-mel":
        return engine.MelMrstftEvaluator(x, sample_rate, plugins, target)
    if distance in _PREFILTERED_DISTANCES:
        return engine.PrefilteredMrstftEvaluator(x, sample_rate, plugins, target, kind=_PREFILTERED_DISTANCES[distance], prefilter="aw")
    if distance in _WAVEFORM_DISTANCES:
        kind, prefilter = _WAVEFORM_DISTANCES[distance]
        return engine.WaveformEvaluator(x, sample_rate, plugins, target, kind=kind, prefilter=prefilter)
    return engine.PopulationEvaluator(x, sample_rate, plugins, model, target, **kw)


def _es_loop(evaluator, input_audio, sample_rate, plugins, *, max_iters, w0, find_w0, sigma0, random_crop, popsize, parallel, dropout,
             savepop, run_dir, seed, rng, early_stop, device_es=False, sync_every=4):
    """run_es from its first evaluation on (reference 574-692), for whichever evaluator the distance chose: only losses are
    seen here, so find_w0, the seeded draws, the early stop and the rank sharding are the same for every objective."""
    _, rank, world = _dist_info()
    total_num_params = _chain_dims(evaluator, plugins)

    def evaluate(W, dropout: float = 0.0, want_audio: bool = False, while_waiting=None):
        """GPU replacement of the reference's evaluate closure (474-573)."""
        out = sharded_evaluate(W, lambda Ws: evaluator.evaluate(Ws, random_crop=random_crop, rng=rng,
                                                                want_audio=want_audio, dropout=dropout, parallel=parallel),
                               while_waiting)
        warn = evaluator.nan_warning()  # after the fitness download: no extra synchronisation
        if warn:
            print(warn)
        return out

    # setup CMA-ES
    if find_w0:
        print("Finding the best w0...")
        tmp_w0s = [rng.rand(total_num_params) for _ in range(popsize)]
        fvals, output_embeds, output_audios = evaluate(tmp_w0s, dropout=dropout, want_audio=savepop)
        print(fvals)
        w0 = tmp_w0s[int(np.argmin(fvals))]
        if savepop:
            savepop_to_disk(-1, fvals, output_embeds, output_audios, run_dir, sample_rate,
                            first=shard_bounds(len(fvals), rank, world)[0])
    else:
        if w0 is None:
            w0 = np.ones(total_num_params) * 0.5
        else:
            w0 = w0.numpy() if isinstance(w0, torch.Tensor) else np.asarray(w0)

    init_param_dict = parameters_to_dict(w0, plugins)
    print(init_param_dict)

    if device_es:
        return _device_es_iterations(evaluator, input_audio, sample_rate, plugins, w0, popsize if find_w0 else 0, max_iters=max_iters,
                                     sigma0=sigma0, random_crop=random_crop, popsize=popsize, parallel=parallel, dropout=dropout,
                                     seed=seed, rng=rng, early_stop=early_stop, sync_every=sync_every)

    run = _EsRun(w0, sigma0, popsize, seed)
    run.n_evals = popsize if find_w0 else 0

    for iteration in range(max_iters):
        W = run.ask()
        # (the next generation's normal deviates are drawn on the host while the GPU evaluates this one)
        fvals, output_embeds, output_audios = evaluate(
            W, dropout=(dropout if (iteration + 1) < max_iters else 0.0), want_audio=savepop, while_waiting=run.es.prefetch)
        if savepop:
            savepop_to_disk(iteration, fvals, output_embeds, output_audios, run_dir, sample_rate,
                            first=shard_bounds(len(fvals), rank, world)[0])
        stale = run.tell(fvals, iteration)
        if rank == 0:
            run.es.disp()
        if stale and rank == 0:
            print(f"Solution has not improved for {run.stale} iterations.")
        if early_stop and run.stale > 10:
            print("Stopping early due to no improvement.")
            break

    # render the current solution on the full (un-padded) input, like the reference (676-678)
    output_audio = torch.from_numpy(process_audio(input_audio.squeeze(0).cpu().numpy(), run.es.result[0], sample_rate, plugins))
    return run.result(output_audio, plugins)


def _device_es_iterations(evaluator, input_audio, sample_rate, plugins, w0, n_evals, *, max_iters, sigma0, random_crop, popsize, parallel,
                          dropout, seed, rng, early_stop, sync_every):
    """_es_loop's iterations with the strategy on the device: nothing crosses to the host inside a batch of `sync_every`
    iterations -- the population goes from ask to the evaluator and the loss to tell as device tensors -- and the state freezes
    itself at the early stop, so iterations enqueued after it change nothing and the result does not depend on sync_every."""
    opts = {"bounds": [0, 1], "popsize": popsize}
    if seed is not None:
        opts["seed"] = seed
    es = cma.DeviceCMAEvolutionStrategy(w0, sigma0, opts, max_iters=max_iters, early_stop=early_stop)
    enqueued = shown = n_stale = 0
    while enqueued < max_iters:
        flags = None   # the NaN flags of the batch's passes, added up on the device: one warning per batch, none lost
        for _ in range(min(int(sync_every), max_iters - enqueued)):
            W = es.ask_device()
            loss, _, _ = evaluator.evaluate(W, random_crop=random_crop, rng=rng, want_audio=False,
                                            dropout=(dropout if (enqueued + 1) < max_iters else 0.0), parallel=parallel)
            es.tell_device(loss)
            enqueued += 1
            fl = evaluator.nan_flags()
            flags = fl if flags is None or fl is None else flags + fl
        status = es.status()
        warn = evaluator.nan_warning(flags) if flags is not None else None
        if warn:
            print(warn)
        before, rows = es.log_rows(shown, status["iterations"])
        for i, (line, f_before, f_it) in enumerate(zip(es.disp_lines(rows=rows), before, rows[:, 2]), start=shown):
            print(line)
            stale = i > 0 and f_it - f_before > -0.01
            n_stale = n_stale + 1 if stale else 0
            if stale:
                print(f"Solution has not improved for {n_stale} iterations.")
        shown = status["iterations"]
        if status["stopped"]:
            print("Stopping early due to no improvement.")
            break
    state = es.export()
    fval_history, wopt_history = es.logs(state)
    wopt, fopt = (state["best_x"] if state["best_f"] < float("inf") else None), state["best_f"]
    output_audio = torch.from_numpy(process_audio(input_audio.squeeze(0).cpu().numpy(), wopt, sample_rate, plugins))
    return _es_result(output_audio, wopt, fopt, fval_history, wopt_history, n_evals + state["done"] * popsize, plugins)


def run_staged_es(
    input_audio: torch.Tensor,
    target_audio: torch.Tensor,
    sample_rate: int,
    plugins: List[dict],
    model: torch.nn.Module,
    embed_func: callable,
    normalization: str = "peak",
    max_iters: int = 100,
    w0: torch.Tensor = None,
    popsize: int = 10,
    sigma0: float = 0.1,
    distance: str = "cosine",
    parallel: bool = False,
    save_pop: bool = False,
    savepop: bool = False,
    run_dir: str = ".",
    seed: int = None,
    *args,
    **kwargs,
):
    """Stage-wise CMA-ES (reference scripts/run_optim.py:39-234, `--staged`): stage k optimises ONLY the
    parameters of plugin k on the sub-chain plugins[0..k], with the earlier plugins held at their stage optima;
    every stage starts from 0.5 in its own dimensions and gets max_iters // len(plugins) iterations (147-188).

    The reference variant cannot run as written (it calls an undefined `parameters_to_dict`, writes to a global
    `run_dir`, takes the cosine of the embedding *dict*, adds a fourth dimension to the target, and returns a
    tuple where its caller reads a dict).  This is the fixed variant on the GPU evaluate step: the stage's
    candidates are the reference's composed vectors `[wopt_overall, w]` (161-166), rendered and scored by
    PopulationEvaluator like run_es does (same length policy, same loss: mean over the embed_func dict of
    -cosine), input and target peak-normalised in place like run_es (452-453), population sharded over the
    ranks like run_es.  Returns run_es's dict; fval_history / wopt_history hold the stage-local best after
    every tell (181-185), `stage_wopts` the per-stage optima.  Stage k's CMA-ES is seeded with seed + k.

    distance="mrstft": every stage scores its sub-chain's render against the full target AUDIO with an engine.MrstftEvaluator
    (model and embed_func may be None, nothing is embedded); everything else is as above.  Every stage's sub-chain must
    render the target's channel count, and savepop is refused as run_es refuses it for this objective.  distance="mrstft-sd"
    is the same with the sum / difference distance: every stage's sub-chain must render 2 channels; distance="mrstft-mel" is
    distance="mrstft" on mel-band sums of the magnitudes (engine.MelMrstftEvaluator).  "mrstft-aw", "mrstft-sd-aw" and "mrstft-mel-aw"
    are those three on rows that went through the A-weighting FIR of the sample rate first (engine.PrefilteredMrstftEvaluator).
    "esr", "snr", "sisdr", "logcosh" and their "-aw" forms score every stage's render with a waveform distance
    (engine.WaveformEvaluator) under the same rules."""
    _check_distance(distance, sample_rate)
    savepop = bool(savepop or save_pop)
    names = list(plugins.keys())
    if distance in _AUDIO_DISTANCES:  # every stage compares its sub-chain's render with the full target
        for stage_idx in range(len(names)):
            _check_mrstft_pairs(input_audio, target_audio, {k: plugins[k] for k in names[: stage_idx + 1]}, "the target",
                                f"stage {stage_idx} ({names[stage_idx]})", distance=distance)
        _check_mrstft_savepop(savepop, distance)
    _, rank, world = _dist_info()
    seed = _agree_on_seed(seed)
    _peak_normalize_(input_audio)
    _peak_normalize_(target_audio)
    target = embed_func(target_audio, model, sample_rate) if distance == "cosine" else target_audio

    iters_per_stage = max_iters // len(plugins)
    wopt_overall, fopt = None, float("inf")
    fval_history, wopt_history, stage_wopts = [], [], []
    n_evals = 0
    output_audio = None
    for stage_idx in range(len(plugins)):
        stage_plugins = {k: plugins[k] for k in names[: stage_idx + 1]}
        print(f"Optimizing stage {stage_idx} ({list(stage_plugins.keys())})")
        n_stage = plugins[names[stage_idx]]["num_params"]
        evaluator = _make_evaluator(distance, input_audio, sample_rate, stage_plugins, model, target, embed_func=embed_func)
        _chain_dims(evaluator, stage_plugins)
        es = _EsRun.strategy(np.ones(n_stage) * 0.5, sigma0, popsize, None if seed is None else seed + stage_idx)
        for iteration in range(iters_per_stage):
            W = es.ask()
            if stage_idx > 0:
                W_stage = [np.concatenate([wopt_overall, w]) for w in W]
            else:
                W_stage = W
            fvals, _, output_audios = sharded_evaluate(W_stage, lambda Ws: evaluator.evaluate(Ws, want_audio=savepop))
            n_evals += len(W)
            # run_optim.py 181-185: the histories hold the result AFTER tell and no stage stops early, so a stage steps the bare
            # strategy and not an _EsRun with its pre-tell bookkeeping
            es.tell(W, fvals)
            if rank == 0:
                es.disp()
            if savepop:  # 171-179: one file per candidate, overwritten every iteration of the stage
                from .audio_io import save_wav

                lo = shard_bounds(len(fvals), rank, world)[0]
                for j, audio in enumerate(output_audios):
                    audio = audio / torch.max(torch.abs(audio)).clamp(min=1e-8)
                    save_wav(os.path.join(run_dir, f"output_audio_stage_{stage_idx}_pop_{lo + j}_fval_{fvals[lo + j]:0.3f}.wav"),
                             audio.cpu(), sample_rate)
            fval_history.append(es.result[1])
            wopt_history.append(es.result[0])
        wopt, fopt = es.result[0], es.result[1]
        if wopt is None:  # max_iters < len(plugins): no iteration ran
            wopt = np.ones(n_stage) * 0.5
        stage_wopts.append(wopt)
        wopt_overall = wopt if wopt_overall is None else np.concatenate([wopt_overall, wopt])
        output_audio = torch.from_numpy(process_audio(input_audio.squeeze(0).cpu().numpy(), wopt_overall, sample_rate, stage_plugins))
        if rank == 0 and run_dir is not None and os.path.isdir(run_dir):
            from .audio_io import save_wav

            save_wav(os.path.join(run_dir, f"output_audio_stage_{stage_idx}.wav"), output_audio, sample_rate)
    return _es_result(output_audio, wopt_overall, fopt, fval_history, wopt_history, n_evals, plugins, stage_wopts=stage_wopts)


def run_es_batch(
    input_audios: torch.Tensor,
    target_audios: torch.Tensor,
    sample_rate: int,
    plugins: List[dict],
    model: torch.nn.Module,
    embed_func: callable,
    max_iters: int = 100,
    sigma0: float = 0.1,
    popsize: int = 32,
    random_crop: bool = False,
    seed: int = None,
    early_stop: bool = True,
    distance: str = "cosine",
):
    """ES over B independent (input, target) pairs at once -- BASELINE.json configs[2].

    The reference optimises its examples one after the other (scripts/eval/eval_pst.py:691-765)
    and its evaluate closure assumes one input (style_transfer.py:520).  Here every pair keeps its
    own CMA-ES trajectory (an _EsRun seeded seed + pair index, stepped exactly as run_es steps its one) and each iteration
    evaluates the populations, stacked pair-major as (n * popsize, D), on the GPU; pair b's candidates read input b and
    are scored against target b.  Two forms of the call, which differ only in how an iteration's populations reach the GPU:

    Tensors -- input_audios / target_audios (B, chs, seq_len), all pairs the same length and channel count.  One crop
    position per iteration, drawn from RandomState(seed), serves all pairs, and pairs that stop early (same rule as run_es,
    lines 655-670) keep being evaluated with their last population but are no longer told.  A pair's trajectory is bitwise
    the one `run_es(find_w0=False, seed=seed + b)` produces for it alone AS LONG AS NO CROP IS DRAWN (random_crop=False, or
    seq_len <= 262144 + 16384).

    Lists -- two lists of B tensors (1, chs, n_b) or (chs, n_b): the inputs share a channel count and may differ in length,
    the targets may differ in length from their inputs and from each other (the PST benchmark's files).  Pair b draws its
    own crop positions from RandomState(seed + b) (engine.crop_start: one draw per iteration while the pair is active, none
    when the rule needs none); pairs are grouped by evaluate-time length (engine.plan_ragged_groups: everything is 262144
    samples under random_crop or when the file is shorter) and every group is one GPU batch per iteration, its inputs cut
    out of one packed device buffer by stito_gather_crops; pairs that have stopped are no longer gathered, rendered or
    embedded.  The bitwise promise above holds for this form ALWAYS, `random_crop=True` on long inputs included.  The
    launches are eager (no graph replay).

    In both forms each pair is peak-normalised on its own, on clones: the caller's tensors are not modified; the targets are
    embedded once, those of equal shape in one call, and a pair's target embedding is flattened to one row per entry (as the
    evaluator flattens the candidates' embeddings), whatever shape embed_func gives it.  Under torch.distributed the PAIRS are
    sharded over the ranks (no collective until the final gather); every rank returns the full list of B result
    dicts.  An unseeded multi-rank
    run agrees on rank 0's draw of a seed first, so that a pair's trajectory does not depend on the rank that owns it (an
    unseeded run has no defined trajectory anyway, and a single-rank run enters no collective).

    distance="mrstft": the objective of run_es(distance="mrstft") -- the multi-resolution STFT distance of the rendered audio to
    the target AUDIO (engine.MrstftEvaluator); model and embed_func may be None and nothing is embedded.  A target must have
    its input's length and the chain's output channel count.  Both forms work and keep the promise above, against
    `run_es(x_b, t_b, ..., None, None, distance="mrstft", find_w0=False, seed=seed + b)`.  In the list form the targets are
    packed like the inputs (a second engine.RaggedInputs); a length group whose spans can move (random_crop with a member
    that draws its crops) cuts the active pairs' target crops at the same starts as their inputs, one more gather per
    iteration, and refills the target table from them; a group whose spans cannot move gathers its targets once, its table
    is built once, and pairs that stop drop out of it through the slot list of stito_mrstft_loss_slots.

    distance="mrstft-sd": the same on both forms and on every path of the list form, with the distance taken between the sums
    and differences of the two channels (MrstftEvaluator(stereo="sum-diff")); the chain must render exactly 2 channels.

    distance="mrstft-mel": the same again with the distance taken between 64 mel-band sums of the magnitudes
    (engine.MelMrstftEvaluator), channels compared L/R; any channel count the chain renders.

    distance="mrstft-aw", "mrstft-sd-aw", "mrstft-mel-aw": the three above with render and target A-weighted first -- auraloss's
    perceptual_weighting=True, the 101-tap FIR of features.mrstft_prefilter("aw", sample_rate), applied in the loss kernel's loader
    (engine.PrefilteredMrstftEvaluator); the 2-channel rule and the empty-band rule of their plain forms hold.

    distance="esr", "snr", "sisdr", "logcosh" and each with "-aw": the waveform distances of engine.WaveformEvaluator (error-to-signal
    ratio, SNR, scale-invariant SDR, log-cosh; "-aw": behind the same A-weighting FIR), sample against sample, on both forms and on
    every path of the list form, under the rules of distance="mrstft"; any channel count the chain renders."""
    _check_distance(distance, sample_rate)
    ragged = isinstance(input_audios, (list, tuple)) or isinstance(target_audios, (list, tuple))
    if ragged:
        input_audios, target_audios = _check_ragged_pairs(input_audios, target_audios)
    elif input_audios.dim() != 3 or target_audios.dim() != 3 or input_audios.shape[0] != target_audios.shape[0]:
        raise ValueError("input_audios and target_audios must be (B, chs, seq_len) with the same B")
    if distance in _AUDIO_DISTANCES:
        _check_mrstft_pairs(input_audios, target_audios, plugins, distance=distance)
    dist, rank, world = _dist_info()
    seed = _agree_on_seed(seed)
    B_all = len(input_audios)
    lo, hi = shard_bounds(B_all, rank, world)
    results = [None] * B_all
    if hi > lo:
        if ragged:
            xs = [a.detach().to("cpu", torch.float32).clone() for a in input_audios[lo:hi]]
            ts = [a.detach().to("cpu", torch.float32).clone() for a in target_audios[lo:hi]]
        else:
            xs, ts = input_audios[lo:hi].clone(), target_audios[lo:hi].clone()
        for a in (*xs, *ts):  # every pair on its own (run_es 452-453); the rows of a tensor are views of the clone
            _peak_normalize_(a)
        target = ts  # the audio distances: the audio itself
        if distance == "cosine":
            # target embeddings, once: targets of equal shape in one embed_func call
            by_shape, rows = {}, [None] * len(ts)
            for b, t in enumerate(ts):
                by_shape.setdefault(tuple(t.shape), []).append(b)
            for members in by_shape.values():
                emb = embed_func(torch.stack([ts[b] for b in members]), model, sample_rate)
                for k, b in enumerate(members):
                    rows[b] = {name: v.detach().reshape(len(members), -1)[k] for name, v in emb.items()}
            target = {name: torch.stack([row[name] for row in rows]) for name in rows[0]}

        def make_evaluator(x, y=None, **kw):  # y: the list form's stand-in for the target audio (it brings its buffers)
            return _make_evaluator(distance, x, sample_rate, plugins, model, target if y is None else y, embed_func=embed_func, **kw)

        def rng_of(s):  # unseeded: the global generator, not a fresh one
            return np.random if s is None else np.random.RandomState(s)

        pair_seeds = [None if seed is None else seed + lo + b for b in range(hi - lo)]  # CMA-ES and, in the list form, crops
        if ragged:
            evaluator, submit = _ragged_form(make_evaluator, xs, ts if distance in _AUDIO_DISTANCES else None, random_crop,
                                             [rng_of(s) for s in pair_seeds])
        else:
            evaluator, submit = _tensor_form(make_evaluator, xs, random_crop, rng_of(seed))
        w0 = np.ones(_chain_dims(evaluator, plugins)) * 0.5
        runs = [_EsRun(w0, sigma0, popsize, s) for s in pair_seeds]
        for iteration in range(max_iters):
            if not any(run.active for run in runs):
                break
            for run in runs:
                if run.active:
                    run.ask()
            pending = submit(runs)  # [(pair indices, loss tensor)]: everything queued before any fitness is fetched
            for run in runs:  # the next generation's normal deviates, drawn while the GPU works (as run_es does)
                if run.active:
                    run.es.prefetch()
            for members, loss in pending:
                fv = loss.tolist()
                for k, b in enumerate(members):
                    if runs[b].active:
                        runs[b].tell(fv[k * popsize:(k + 1) * popsize], iteration)
                        runs[b].active = not (early_stop and runs[b].stale > 10)
        for b, run in enumerate(runs):
            out = torch.from_numpy(process_audio(xs[b].cpu().numpy(), run.es.result[0], sample_rate, plugins))
            results[lo + b] = run.result(out, plugins)
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, [(i, r) for i, r in enumerate(results) if r is not None])
        for part in gathered:
            for i, r in part:
                results[i] = r
    return results


def _tensor_form(make_evaluator, xs, random_crop, rng):
    """-> (evaluator, submit) of run_es_batch's tensor form, for either objective: ALL pairs every iteration, a stopped pair
    re-submitting its last population -- the input buffer keeps its shape, so the evaluator's graph replay stays eligible -- and
    one crop position for all (inputs and, under "mrstft", targets alike), drawn by the evaluator from the one rng."""
    evaluator = make_evaluator(xs)

    def submit(runs):
        loss, _, _ = evaluator.evaluate(np.concatenate([np.asarray(run.W) for run in runs], 0), random_crop=random_crop, rng=rng)
        return [(range(len(runs)), loss)]

    return evaluator, submit


def _ragged_form(make_evaluator, xs, ts, random_crop, rngs):
    """-> (evaluator, submit) of run_es_batch's list form: per length group the ACTIVE pairs only, each with a crop position of
    its own from its own rng, cut out of the packed inputs by one gather.

    ts: the target audio, for an objective that compares audio ("mrstft"; None under "cosine"), packed like the inputs.  A group
    whose spans can move -- random_crop, and a member long enough to draw its crops -- cuts the active pairs' target crops at the
    starts of their inputs (one more gather per iteration) and the evaluator refills its table from them.  In any other group
    every span is [0, eval_len) for good: the targets are gathered once, before the first iteration, the table is built once,
    and pairs that have stopped drop out through the slot list."""
    device = engine._current_device()
    ragged = engine.RaggedInputs(xs, device)
    targets = None if ts is None else engine.RaggedInputs(ts, device)
    # the evaluator never reads its own audio on this path (every call brings its gathered buffers): one-sample stand-ins
    stand_in = lambda audios: torch.zeros((len(audios), audios[0].shape[0], 1))  # noqa: E731
    evaluator = make_evaluator(stand_in(xs), None if ts is None else stand_in(ts), use_graph=False)
    groups = engine.plan_ragged_groups(ragged.lengths, random_crop)
    moving = set()  # the evaluate-time lengths whose target spans move
    if targets is not None:
        for eval_len, members in groups:
            if random_crop and any(ragged.lengths[b] - engine.CROP_LEN > engine.CROP_MARGIN for b in members):
                moving.add(eval_len)
            else:
                evaluator.set_static_targets(eval_len, members, targets.gather(members, [0] * len(members), eval_len))

    def submit(runs):
        pending = []
        for eval_len, members in groups:  # one gather (two with moving targets) + one evaluate per group
            act = [b for b in members if runs[b].active]
            if not act:
                continue
            starts = [engine.crop_start(ragged.lengths[b], random_crop, rngs[b]) for b in act]
            buffers = {"x": ragged.gather(act, starts, eval_len)}
            if eval_len in moving:
                buffers["y"] = targets.gather(act, starts, eval_len)
            loss, _, _ = evaluator.evaluate(np.concatenate([np.asarray(runs[b].W) for b in act], 0), pairs=act, **buffers)
            pending.append((act, loss))
        return pending

    return evaluator, submit


def _check_ragged_pairs(input_audios, target_audios):
    """Validation of the list form of run_es_batch (host only) -> ([(chs, n_b)], [(chs_t, m_b)]) views of the caller's tensors."""
    if not isinstance(input_audios, (list, tuple)) or not isinstance(target_audios, (list, tuple)):
        raise ValueError("input_audios and target_audios must both be lists (or both (B, chs, seq_len) tensors)")
    if len(input_audios) == 0 or len(target_audios) == 0:
        raise ValueError("input_audios and target_audios must not be empty")
    if len(input_audios) != len(target_audios):
        raise ValueError(f"{len(input_audios)} inputs but {len(target_audios)} targets")

    def as_2d(a, what, b):
        if not isinstance(a, torch.Tensor):
            raise ValueError(f"{what} {b}: expected a tensor, got {type(a).__name__}")
        if a.dim() == 3 and a.shape[0] == 1:
            a = a[0]
        if a.dim() != 2 or a.shape[0] not in (1, 2) or a.shape[1] == 0:
            raise ValueError(f"{what} {b}: expected (1, chs, n) or (chs, n) with 1 or 2 channels, got {tuple(a.shape)}")
        return a

    xs = [as_2d(a, "input", b) for b, a in enumerate(input_audios)]
    ts = [as_2d(a, "target", b) for b, a in enumerate(target_audios)]
    if len({x.shape[0] for x in xs}) != 1:
        raise ValueError(f"inputs have mixed channel counts {[x.shape[0] for x in xs]}")
    return xs, ts
