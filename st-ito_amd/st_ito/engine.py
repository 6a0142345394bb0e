"""Host-side orchestration of the HIP hot path: plugin dict -> chain descriptor, population
rendering, embedding, loss.  Everything numeric happens in libstito_hip; torch only owns the
buffers and the stream.

Reference call sites replaced: the loop `for w in W: process_audio(...)`, the `embed_func` call
and the cosine loss in run_es.evaluate (st_ito/style_transfer.py:504-573).

The evaluate step exists per objective -- PopulationEvaluator (embeddings, -cosine) and MrstftEvaluator (MRSTFT distance to the
target audio) -- on one base, _Evaluator, which holds what does not depend on the objective: the compiled chain, the inputs,
the length policy applied to tensors (eval_span / cut_to_span) and the checks of evaluate's arguments.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _hip

CROP_LEN = 262144  # style_transfer.py:505
CROP_MARGIN = 16384  # style_transfer.py:506-514: a crop start is drawn only when more than this many samples are spare


def _current_device() -> torch.device:
    """The GPU that this process works on; without one there is nothing to fall back to."""
    _hip.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


# --------------------------------------------------------------------------------------------
# length policy of the evaluate step (style_transfer.py:505-518), as pure host functions
# --------------------------------------------------------------------------------------------
def crop_start(n: int, random_crop: bool, rng=np.random) -> int:
    """Crop position of one evaluate call on an input of n samples: rng.randint(16384, n - 262144) when random_crop and more
    than 16384 samples are spare, else 0 -- and then nothing is drawn from rng."""
    spare = int(n) - CROP_LEN
    if random_crop and spare > CROP_MARGIN:
        return int(rng.randint(CROP_MARGIN, spare))
    return 0


def eval_length(n: int, random_crop: bool) -> int:
    """Samples per candidate that evaluate renders for an input of n samples: 262144 (zero padded, or cropped), or all n of a
    longer input without random_crop."""
    return CROP_LEN if (random_crop or int(n) <= CROP_LEN) else int(n)


def eval_span(n: int, random_crop: bool, rng=np.random, parallel: bool = False) -> Tuple[int, int]:
    """(start, length) of the samples that one evaluate call reads of an n-sample signal: length == n -- as it is; length < n --
    the crop [start, start + length); length > n -- zero padded to 262144.  Draws from rng exactly as crop_start does.  The
    reference's parallel=True branch (499-502) hands the signal to the pool as it is: no padding, no crop, nothing drawn."""
    if parallel:
        return 0, int(n)
    return crop_start(n, random_crop, rng), eval_length(n, random_crop)


def cut_to_span(t: torch.Tensor, span: Tuple[int, int], padded: Optional[torch.Tensor] = None):
    """t (..., n) cut to a span of eval_span -> (t itself (no copy), a contiguous crop, or t zero padded; the padded copy to keep).
    The caller hands the kept copy back in as `padded`: it is built once, and every call returns the same buffer (a captured
    graph reads it by address)."""
    start, length = span
    n = t.shape[-1]
    if length == n:
        return t, padded
    if length < n:
        return t[..., start:start + length].contiguous(), padded
    if padded is None:
        padded = torch.nn.functional.pad(t, (0, length - n)).contiguous()
    return padded, padded


def plan_ragged_groups(lengths, random_crop: bool) -> List[Tuple[int, List[int]]]:
    """Pairs of a ragged batch that can share one GPU pass: [(evaluate-time length, [pair indices in ascending order])], groups
    in order of their first pair.  With random_crop there is one group (everything is 262144 samples)."""
    groups: Dict[int, List[int]] = {}
    for b, n in enumerate(lengths):
        if int(n) <= 0:
            raise ValueError(f"input {b} is empty")
        groups.setdefault(eval_length(n, random_crop), []).append(b)
    return list(groups.items())


class RaggedInputs:
    """The inputs of a ragged batch on the device, uploaded once: one packed float32 buffer with every (chs, n_b) input back to
    back (each starting on a 16-byte boundary), their offsets and lengths, and per evaluate-time length one persistent
    (pairs, chs, length) buffer that stito_gather_crops refills -- one launch per call."""

    def __init__(self, inputs: List[torch.Tensor], device: torch.device):
        _hip.require_gpu()
        if not inputs:
            raise ValueError("no inputs")
        self.device = device
        self.channels = int(inputs[0].shape[0])
        self.lengths = [int(x.shape[-1]) for x in inputs]
        offsets, total = [], 0
        for x in inputs:
            if x.dim() != 2 or x.shape[0] != self.channels:
                raise ValueError("inputs must be (chs, n) with one channel count")
            offsets.append(total)
            total += (x.numel() + 3) // 4 * 4
        host = torch.zeros(total, dtype=torch.float32)
        for off, x in zip(offsets, inputs):
            host[off:off + x.numel()] = x.detach().to(torch.float32).reshape(-1)
        self.packed = host.to(device)
        self.offset = torch.tensor(offsets, dtype=torch.int64, device=device)
        self.length = torch.tensor(self.lengths, dtype=torch.int64, device=device)
        self.start = torch.zeros(len(inputs), dtype=torch.int64, device=device)
        self._slots = torch.zeros(len(inputs), dtype=torch.int32, device=device)
        self._out: Dict[int, torch.Tensor] = {}
        self.n_launches = 0

    def gather(self, pairs: List[int], starts: List[int], crop_len: int) -> torch.Tensor:
        """(len(pairs), chs, crop_len): samples [start, start + crop_len) of the listed inputs, zeros past their ends (a pair has ONE
        start per call, so it is listed at most once).  The result is a view of a buffer that the next gather of the same crop_len overwrites (same stream: ordered)."""
        n_pairs, k = len(self.lengths), len(pairs)
        if k == 0 or len(set(pairs)) != k or len(starts) != k or any(not 0 <= b < n_pairs for b in pairs):
            raise ValueError(f"gather: pairs {list(pairs)} / starts {list(starts)} do not name inputs 0 .. {n_pairs - 1}")
        if any(s < 0 or s >= self.lengths[b] for b, s in zip(pairs, starts)):
            raise ValueError(f"gather: a crop start lies outside its input ({list(starts)})")
        buf = self._out.get(crop_len)
        if buf is None:
            buf = self._out[crop_len] = torch.empty((n_pairs, self.channels, crop_len), dtype=torch.float32, device=self.device)
        st = np.zeros(n_pairs, dtype=np.int64)
        st[list(pairs)] = starts
        self.start.copy_(torch.from_numpy(st))
        self._slots[:k].copy_(torch.tensor(list(pairs), dtype=torch.int32))
        out = buf[:k]
        _hip.check(_hip.lib().stito_gather_crops(_hip.ptr(self.packed), self.packed.numel(), _hip.ptr(self.offset), _hip.ptr(self.length),
                                                 _hip.ptr(self.start), n_pairs, _hip.ptr(self._slots), k, self.channels, crop_len,
                                                 _hip.ptr(out), _hip.stream_ptr()))
        self.n_launches += 1
        return out


# --------------------------------------------------------------------------------------------
# plugin dict (reference schema) -> stito_fx_desc[]
# --------------------------------------------------------------------------------------------
def _instance_of(plugin: dict):
    if "instance" not in plugin:
        if "vst_filepath" in plugin:
            raise NotImplementedError("VST plugins (pedalboard.load_plugin) are not supported in this build; "
                                      "use --effect-type basic")
        elif "class_path" in plugin:
            plugin["instance"] = plugin["class_path"]()
        else:
            raise ValueError("Plugin must contain 'vst_filepath' or 'class_path'.")
    return plugin["instance"]


def compile_chain(plugins: Dict[str, dict], normalize_stages: bool = False) -> Tuple[ctypes.Array, int]:
    """Compile the reference's `plugins` dict into the C chain descriptor.

    Mirrors how process_audio walks the dict (style_transfer.py:65-92): every name in
    plugin["parameter_names"] consumes one slot of w; "our_bypass" is consumed and ignored;
    names listed in plugin["fixed_parameters"] take the fixed value (via Parameter.set_value)
    but still consume their slot."""
    descs = (_hip.FxDesc * max(1, len(plugins)))()
    descs._keep = []  # device buffers the descriptor points into
    off = 0
    for i, (plugin_name, plugin) in enumerate(plugins.items()):
        if "vst_filepath" in plugin and "class_path" not in plugin:
            raise NotImplementedError("VST plugins are not supported in this build; use --effect-type basic")
        inst = _instance_of(plugin)
        kind = getattr(inst, "KIND", -1)
        if kind < 0:
            raise ValueError(f"Plugin {plugin_name}: {type(inst).__name__} is not an effect of this build")
        names = list(plugin.get("parameter_names") or list(inst.parameters.keys()))
        has_bypass = 1 if (names and names[0] == "our_bypass") else 0
        real = names[has_bypass:]
        if "our_bypass" in real or real != list(inst.parameters.keys()):
            raise ValueError(f"Plugin {plugin_name}: parameter_names {names} do not match {list(inst.parameters)}")
        d = descs[i]
        d.kind, d.num_channels, d.w_offset, d.has_bypass = kind, int(plugin["num_channels"]), off, has_bypass
        if d.num_channels not in (1, 2):
            raise ValueError(f"Plugin {plugin_name}: num_channels must be 1 or 2")
        mask = 0
        for p, name in enumerate(real):
            if name in plugin.get("fixed_parameters", {}):
                prm = inst.parameters[name]
                prm.set_value(plugin["fixed_parameters"][name])  # asserts the range like the reference
                d.fixed_raw[p] = prm.raw_value
                mask |= 1 << p
        d.fixed_mask = mask
        d.flags = _hip.FX_FLAG_NORMALIZE_AFTER if normalize_stages else 0  # style_transfer.py:106-107
        if kind == _hip.FX_NOISE_REVERB:  # the band-filtered noise bank is an input of the stage
            bank = inst.noise_bank_device(_current_device())
            descs._keep.append(bank)
            d.aux_dev, d.aux_len = bank.data_ptr(), bank.shape[-1]
        off += len(names)
    return descs, off


def chain_out_channels(plugins: Dict[str, dict], in_channels: int) -> int:
    """Channels of the rendered audio (style_transfer.py:94-104; stito_chain_out_channels on the host, before a chain is
    compiled): a 2-channel plugin up-mixes a mono signal, except the dasp compressor, which never does."""
    c = int(in_channels)
    for plugin in plugins.values():
        if int(plugin["num_channels"]) == 2 and c == 1 and getattr(_instance_of(plugin), "KIND", -1) != _hip.FX_DASP_COMPRESSOR:
            c = 2
    return c


class Workspace:
    """Grow-only device scratch buffers keyed by name (torch owns the memory), one per evaluator; a call handed none: _hip.scratch."""

    def __init__(self):
        self._bufs: Dict[str, torch.Tensor] = {}

    def get(self, name: str, nbytes: int, device) -> torch.Tensor:
        b = self._bufs.get(name)
        if b is None or b.numel() < nbytes or b.device != device:
            b = self._bufs[name] = _hip.scratch(nbytes, device)
        return b

    def buffers(self) -> Tuple[torch.Tensor, ...]:
        """The buffers held at this moment: what a captured graph pins (a later, larger get() replaces the entry, not this object)."""
        return tuple(self._bufs.values())


def render_population(plugins: Dict[str, dict], x: torch.Tensor, W: torch.Tensor, sample_rate: float,
                      chain=None, out=None, ws: Optional[Workspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (C, L) float32 on the GPU -- or (B, C, L): B inputs, candidate p reads input p // (P // B) --
    W (P, D) float64 on the GPU -> (audio (P, C', L) before peak normalisation, peaks (P,)).
    out: (audio, peaks) to render into (contiguous slices of a larger population's buffers); ws: the evaluator's Workspace the
    render's scratch comes from (None: allocated for this call on the current stream)."""
    _hip.require_gpu()
    L = _hip.lib()
    descs, ndims = chain if chain is not None else compile_chain(plugins)
    n_fx = len(plugins)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 3)
    assert W.is_cuda and W.dtype == torch.float64 and W.dim() == 2
    x = x.contiguous()
    W = W.contiguous()
    if W.shape[1] != ndims:
        raise ValueError(f"parameter vector has {W.shape[1]} dims, chain consumes {ndims}")
    n_inputs = x.shape[0] if x.dim() == 3 else 1
    C, n = x.shape[-2:]
    P = W.shape[0]
    if P % n_inputs:
        raise ValueError(f"population {P} is not a multiple of the number of inputs {n_inputs}")
    c_out = L.stito_chain_out_channels(descs, n_fx, C)
    if out is None:
        audio = torch.empty((P, c_out, n), dtype=torch.float32, device=x.device)
        peaks = torch.empty((P,), dtype=torch.float32, device=x.device)
    else:
        audio, peaks = out
        assert audio.shape == (P, c_out, n) and audio.is_contiguous() and audio.dtype == torch.float32 and peaks.shape == (P,)
    for i in range(n_fx):  # the chorus stage reads its LFO from a table that has to cover this length
        if descs[i].kind == _hip.FX_CHORUS:
            # re-fetched on every call: the shared table belongs to one (sample rate, device) and is replaced when a longer render
            # grows it, so a descriptor compiled earlier may point at the old one (or at another rate's).  The descriptor keeps
            # every table it has pointed at alive (descs._keep): a launch already queued on the stream may still read it
            from .effects import chorus_lfo_device
            t = chorus_lfo_device(sample_rate, n, x.device)
            if descs[i].aux_dev != t.data_ptr() or descs[i].aux_len != t.numel():
                descs[i].aux_dev, descs[i].aux_len = t.data_ptr(), t.numel()
                if hasattr(descs, "_keep"):
                    descs._keep.append(t)
    need = L.stito_render_workspace_bytes(descs, n_fx, C, n, P)
    buf = _hip.scratch(need, x.device, ws, "render")
    _hip.check(L.stito_render_population_multi(descs, n_fx, _hip.ptr(x), n_inputs, C, n, _hip.ptr(W), P, ndims,
                                               float(sample_rate), _hip.ptr(audio), _hip.ptr(peaks), _hip.ptr(buf),
                                               buf.numel(), _hip.stream_ptr()))
    return audio, peaks


def normalize_audio_(audio: torch.Tensor, peaks: torch.Tensor) -> torch.Tensor:
    """In place: audio[p] /= clip(peaks[p], 1e-8)  (style_transfer.py:113)."""
    P, C, n = audio.shape
    _hip.check(_hip.lib().stito_normalize_audio(_hip.ptr(audio), P, C, n, _hip.ptr(peaks), _hip.stream_ptr()))
    return audio


def render_single(instance, x: np.ndarray, sample_rate: float) -> np.ndarray:
    """Basic*.process(x, sample_rate): one effect, current parameter values, (chs, n) -> (chs', n)."""
    dev = _current_device()
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("process expects a (chs, n) array")
    # .process() is called with exactly the channels the effect should see; a stereo effect
    # called with mono audio is fed the mono signal as in pedalboard (no up-mix here).
    nch = 2 if ((x.shape[0] == 2 and instance.NUM_CHANNELS == 2) or getattr(instance, "ALWAYS_STEREO", False)) else 1
    plugins = {"fx": {"class_path": type(instance), "instance": instance, "num_channels": nch,
                      "fixed_parameters": {}, "parameter_names": list(instance.parameters.keys()),
                      "num_params": len(instance.parameters)}}
    w = np.array([[p.raw_value for p in instance.parameters.values()]], dtype=np.float64)
    audio, _ = render_population(plugins, torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), sample_rate)
    return audio[0].cpu().numpy()


def process_audio_gpu(x: np.ndarray, w: np.ndarray, sr: int, plugins: Dict[str, dict],
                      normalize_stages: bool = False) -> np.ndarray:
    """process_audio for one parameter vector (style_transfer.py:45-115)."""
    dev = _current_device()
    xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)[None, :]).to(dev)
    audio, peaks = render_population(plugins, xt, wt, sr, chain=compile_chain(plugins, normalize_stages))
    normalize_audio_(audio, peaks)
    return audio[0].cpu().numpy()


# --------------------------------------------------------------------------------------------
# population evaluation
# --------------------------------------------------------------------------------------------
class _Evaluator:
    """What the evaluate step has in common under every objective: the inputs on the device, the compiled chain, the length
    policy and the checks of evaluate's arguments, each with its one text."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], device: Optional[torch.device],
                 normalize_stages: bool):
        _hip.require_gpu()
        self.device = device or _current_device()
        self.sample_rate = sample_rate
        self.plugins = plugins
        self.chain = compile_chain(plugins, normalize_stages)
        self.ndims = self.chain[1]
        self.n_inputs = x.shape[0]
        self.x_full = x.to(self.device, torch.float32).contiguous()
        self._x_padded = None  # cut_to_span's zero-padded copy of x_full
        self.ws = Workspace()  # the persistent scratch of this evaluator's launches: one evaluator, one stream at a time
        self.rendered_candidates = 0

    def _pairs(self, pairs, what: str = "inputs", once: bool = False) -> List[int]:
        """The listed pairs as ints; `once`: none of them twice."""
        pairs = [int(b) for b in pairs]
        if not pairs or (once and len(set(pairs)) != len(pairs)) or any(not 0 <= b < self.n_inputs for b in pairs):
            raise ValueError(f"pairs {pairs} do not name {what} 0 .. {self.n_inputs - 1}")
        return pairs

    @staticmethod
    def _ready_made(t: torch.Tensor, name: str, k: int) -> None:
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous() and t.shape[0] == k):
            raise ValueError(f"{name} must be a contiguous ({k}, chs, n) float32 tensor on the GPU")

    def _arguments(self, W, pairs, x, y=None):
        """The checks of evaluate(W, pairs=, x=, y=) -> (W as (P, ndims) float64, pairs as ints or None, number of inputs the
        call reads, candidates per input).  Nothing is drawn and nothing launched before they pass.  W as a torch tensor is a
        population that is already on the device (the device ES's): it is checked like any other, stays where it is and is
        returned as it is."""
        if isinstance(W, torch.Tensor):
            if not (W.is_cuda and W.dtype == torch.float64 and W.is_contiguous()):
                raise ValueError(f"parameter vectors given as a tensor must be a contiguous (P, {self.ndims}) float64 tensor on the GPU, "
                                 f"got {W.dtype} on {W.device}")
            Wn = W
        else:
            Wn = np.asarray(W, dtype=np.float64)
        if Wn.ndim != 2 or Wn.shape[1] != self.ndims:
            raise ValueError(f"parameter vectors must be (P, {self.ndims}), got {tuple(Wn.shape)}")
        if pairs is not None:
            pairs = self._pairs(pairs)
        k = self.n_inputs if pairs is None else len(pairs)
        if x is not None:
            self._ready_made(x, "x", k)
        elif y is not None:
            raise ValueError("y (ready-made target spans) needs x (the input spans they belong to)")
        P = Wn.shape[0]
        if P == 0 or P % k:
            raise ValueError(f"{P} candidates cannot be split over {k} inputs")
        return Wn, pairs, k, P // k

    def _on_device(self, Wn) -> torch.Tensor:
        """_arguments' W on the device: a numpy population is uploaded, a device population is used where it is."""
        return Wn.to(self.device) if isinstance(Wn, torch.Tensor) else torch.from_numpy(Wn).to(self.device)

    def nan_flags(self) -> Optional[torch.Tensor]:
        """The NaN flags of the last evaluate() as a device tensor, without a synchronisation (None: this objective has none).  A
        caller that does not fetch every fitness -- the device ES -- adds them up and hands the sum to nan_warning()."""
        return None

    def nan_warning(self, flags: Optional[torch.Tensor] = None) -> Optional[str]:
        return None


class PopulationEvaluator(_Evaluator):
    """GPU replacement of run_es.evaluate (style_transfer.py:474-573) for the AFx-Rep metric.

    One instance per run_es call: holds the (padded) input on the device, the compiled chain
    and the target embeddings.  evaluate(W) returns the fitness list; embeddings and (lazily)
    normalised audio are available for --savepop.

    Multi-pair batches (BASELINE.json configs[2]): x may hold B inputs (B, C, L) with B target
    embeddings (B, E); evaluate then takes the B populations stacked pair-major, (B * P, D), and
    scores the candidates of pair b against target b.  evaluate(W, pairs=[...], x=buffer) scores the populations of a SUBSET
    of the pairs, in the order listed, on a ready-made input buffer (len(pairs), C, L) -- the ragged batch, which gathers,
    renders and embeds its active pairs only.  `rendered_candidates` counts what went through the render."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], model, target_embeds: dict,
                 device: Optional[torch.device] = None, max_candidates_per_pass: Optional[int] = None,
                 embed_func=None, normalize_stages: bool = False, entry_weights: Optional[Dict[str, float]] = None,
                 use_graph: Optional[bool] = None, capture_after: Optional[int] = None):
        """embed_func: None or st_ito.utils.get_param_embeds -> the fused AFx-Rep path (render -> log-mel with the
        peak normalisations folded into the STFT loader -> Cnn14 -> loss).  Any other embed_func(x, model, sample_rate)
        -> dict of (P, E_k) embeddings (the MIR / MFCC metrics of st_ito.utils, or a user function working on GPU
        tensors) takes the generic path of style_transfer.py:531-571: the rendered population is peak-normalised in
        HBM, handed to embed_func as one (P, C, L) GPU tensor, and every entry of the returned dict is scored against
        the target's entry of the same name.  use_graph: None = STITO_GRAPH (default on), False = eager launches only
        (bench.py's per-launch event timing needs host-side launches)."""
        from . import utils as _utils

        assert x.dim() == 3, "input audio must be (batch, chs, seq_len)"
        super().__init__(x, sample_rate, plugins, device, normalize_stages)
        self.model = model
        self.embed_func = embed_func
        # the fused path embeds the rendered audio as 48 kHz audio; at any other rate the reference resamples inside
        # get_param_embeds (utils.py:462-463), on both sides of the distance: that goes through the generic path
        self.fused = (embed_func is None or embed_func is _utils.get_param_embeds) and int(sample_rate) == 48000
        if embed_func is None and not self.fused:
            self.embed_func = _utils.get_param_embeds
        self.targets = {k: v.detach().to(self.device, torch.float32).contiguous().view(-1, v.shape[-1])
                        for k, v in target_embeds.items()}
        for k, v in self.targets.items():
            if v.shape[0] != self.n_inputs:
                raise ValueError(f"{self.n_inputs} inputs but {v.shape[0]} target embeddings ({k})")
        if self.fused:
            self.tmid, self.tside = self.targets["mid"], self.targets["side"]
        # generic path: weight of every entry of the embedding dict inside the mean over entries (style_transfer.py:560-568
        # counts a content embedding's distance twice: dists.append(2 * dist)); default 1
        self.entry_weights = dict(entry_weights or {})
        self.max_cand = max_candidates_per_pass
        self.flags = torch.zeros((256, 2), dtype=torch.int32, device=self.device)  # NaN flags, one row per loss call
        # The plain fused call -- one population per pass, no crop, no dropout, no audio handed back: what run_es issues every
        # iteration -- is captured as ONE hipGraph (render -> log-mel -> Cnn14 -> loss: ~45 launches) and replayed; W travels
        # through a static device buffer.  STITO_GRAPH=0 keeps the eager launches.  On an idle host a replay buys little (the
        # eager launches already run ahead of the device: pop 32 6.56 against 6.60 ms per step, pop 256 43.0 against 43.1); what it
        # removes is the step's dependence on the host's launch rate: one launch per step and rank instead of ~45.
        # (Round 4 had this off: every replay after the first kept the previous replay's per-candidate peaks and stream maxima,
        # because the hipMemsetAsync nodes that zero those atomicMax targets were not ordered in front of their kernels on
        # replay.  The library now zeroes with a kernel -- csrc/common.h zero_async -- and tests/test_gpu_es.py replays the graph
        # in 50 fresh processes against the eager result, bit for bit.)
        self._graph_on = (os.environ.get("STITO_GRAPH", "1") != "0") if use_graph is None else bool(use_graph)
        # a graph is captured on the (capture_after + 1)-th eligible call with the same population size and input buffer.  The
        # capture costs ~10 ms at pop 32 and ~30 ms at pop 256 (private-pool allocations + hipGraphInstantiate of ~45 kernel nodes)
        # and a replay saves 0.2 - 1 % of a step on an idle host, so a short run never earns it back (the reference's CLI default
        # stops after ~25 iterations, its PST harness runs 32: 7.5 -> 7.9 ms per iteration with a capture at call 9, measured):
        # the first 32 calls launch eagerly, longer runs switch to replay.  STITO_GRAPH_AFTER overrides; 0 = capture on the first
        # call (bench.py: inside its warm-up)
        self.capture_after = int(os.environ.get("STITO_GRAPH_AFTER", "32")) if capture_after is None else int(capture_after)
        self._graph_calls = {}
        self._graph_evictions = 0
        self._n_flag_rows = 0  # rows of self.flags the last evaluate() wrote
        self._graphs = {}      # (P, input pointer, input shape) -> (graph, W buffer, loss, mid, side, n_calls, buffers kept alive)

    def _input(self, random_crop: bool, rng, parallel: bool = False) -> torch.Tensor:
        """The evaluator's own input under the length policy (eval_span), with one crop position for all inputs of a batch."""
        x, self._x_padded = cut_to_span(self.x_full, eval_span(self.x_full.shape[-1], random_crop, rng, parallel), self._x_padded)
        return x

    def _spans(self, p0, p1, per, pairs):
        """-> (inputs of x that candidates p0 .. p1 - 1 read, [(target index, first candidate, end) within the pass])"""
        B = self.n_inputs if pairs is None else len(pairs)
        tgt = (lambda b: b) if pairs is None else (lambda b: pairs[b])
        if B == 1:
            return (0, 1), [(tgt(0), 0, p1 - p0)]
        b0, b1 = p0 // per, (p1 + per - 1) // per
        return (b0, b1), [(tgt(b), (b - b0) * per, (b - b0 + 1) * per) for b in range(b0, b1)]

    def _fused_pass(self, Wc, x, p0, p1, per, n_calls, dropout, want_audio, pairs=None):
        """One pass of the fused AFx-Rep path over candidates p0 .. p1 - 1 on the current stream:
        render -> log-mel + Cnn14 -> loss.  -> (loss, mid, side, audio or None, peaks, n_calls)"""
        L = _hip.lib()
        (b0, b1), spans = self._spans(p0, p1, per, pairs)
        xin = x[0] if x.shape[0] == 1 else x[b0:b1]
        audio, peaks = render_population(self.plugins, xin, Wc, self.sample_rate, chain=self.chain, ws=self.ws)
        mid, side = self.model.embed_raw(audio, peaks, norm_passes=2, ws=self.ws)
        loss = torch.empty(mid.shape[0], dtype=torch.float32, device=self.device)
        # dropout (style_transfer.py:549-551) hits the embeddings only inside the distance; the cosine is
        # scale-invariant, so dropping the raw vectors and normalising afterwards is the same quantity.
        # The returned embeddings stay undropped, like the reference's output_embeds.
        md, sd = mid, side
        if dropout > 0.0:
            md = torch.nn.functional.dropout(mid, p=dropout, training=True).contiguous()
            sd = torch.nn.functional.dropout(side, p=dropout, training=True).contiguous()
        for b, q0, q1 in spans:  # candidates of pair b against target b
            _hip.check(L.stito_embed_loss(_hip.ptr(md[q0:q1]), _hip.ptr(sd[q0:q1]), q1 - q0, mid.shape[1],
                                          _hip.ptr(self.tmid[b]), _hip.ptr(self.tside[b]), _hip.ptr(loss[q0:q1]),
                                          _hip.ptr(self.flags[n_calls % 256]), _hip.stream_ptr()))
            n_calls += 1
        if dropout > 0.0:  # NaN scrub + L2 norm of the embeddings handed back
            _hip.check(L.stito_embed_loss(_hip.ptr(mid), _hip.ptr(side), mid.shape[0], mid.shape[1], None, None, None,
                                          _hip.ptr(self.flags[255]), _hip.stream_ptr()))
        return loss, mid, side, (normalize_audio_(audio, peaks) if want_audio else None), (audio, peaks), n_calls

    def _evaluate_graph(self, Wn, x, per):
        """The plain fused call as one hipGraph launch, or None while this (population size, input buffer) has been seen fewer than
        capture_after times.  W travels through a static device buffer; the outputs are copied out of the graph's buffers, so
        they stay valid across calls."""
        P = Wn.shape[0]
        key = (P, x.data_ptr(), tuple(x.shape))
        ent = self._graphs.get(key)
        if ent is None:
            seen = self._graph_calls.get(key, 0)
            self._graph_calls[key] = seen + 1
            if seen < self.capture_after:
                return None   # not yet: the caller launches eagerly
            if len(self._graphs) >= 4 and self._graph_evictions >= 8:
                return None   # more than four shapes keep rotating: every call would re-capture (10 - 30 ms each); stay eager
            Wbuf = torch.empty((P, self.ndims), dtype=torch.float64, device=self.device)
            Wbuf.copy_(Wn if isinstance(Wn, torch.Tensor) else torch.from_numpy(Wn))
            if seen == 0:
                # nothing of this shape has run yet: one eager pass first (not part of the graph), which builds everything lazy
                # -- packed weights, workspaces, LDS attributes -- outside the capture
                side_stream = torch.cuda.Stream(self.device)
                side_stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side_stream):
                    self._fused_pass(Wbuf, x, 0, P, per, 0, 0.0, False)
                torch.cuda.current_stream(self.device).wait_stream(side_stream)
            # capture by hand on a side stream: the torch.cuda.graph() context manager also runs gc.collect() and
            # torch.cuda.empty_cache(), i.e. it hands every cached block back to the driver (the CLI-default point: 8.2 ms per
            # iteration with it, 7.9 without, 7.5 - 7.6 eager)
            g = torch.cuda.CUDAGraph()
            cap_stream = torch.cuda.Stream(self.device)
            cap_stream.wait_stream(torch.cuda.current_stream(self.device))
            try:
                with torch.cuda.stream(cap_stream):
                    g.capture_begin(capture_error_mode="relaxed")
                    try:
                        loss, mid, side, _, keep, n_calls = self._fused_pass(Wbuf, x, 0, P, per, 0, 0.0, False)
                    finally:
                        g.capture_end()
            except Exception as e:  # noqa: BLE001 -- a capture-unsafe call on another ROCm build, an allocation failure, ...
                # the step must not die at call capture_after + 1 of a long run: drop the partial graph, switch replay off for
                # this evaluator and let the caller launch eagerly (the eager path is the one the first capture_after calls took)
                import warnings
                warnings.warn(f"st_ito: hipGraph capture of the evaluate step failed ({type(e).__name__}: {e}); continuing with eager launches")
                self._graph_on = False
                self._graphs.clear()
                del g
                torch.cuda.synchronize(self.device)
                return None
            torch.cuda.current_stream(self.device).wait_stream(cap_stream)
            # the graph holds raw pointers: everything it touches stays referenced here -- the outputs, the input and this
            # evaluator's scratch as it was at capture (a later, larger call replaces those buffers; the graph keeps its own)
            keep = (keep, self.ws.buffers(), x)
            ent = (g, Wbuf, loss, mid, side, n_calls, keep)
            if len(self._graphs) >= 4:   # a few shapes at most (find_w0 batch, population, last partial shard)
                old = next(iter(self._graphs))
                self._graphs.pop(old)
                self._graph_calls.pop(old, None)   # an evicted shape starts counting again instead of re-capturing on its next call
                self._graph_evictions += 1
            self._graphs[key] = ent
        g, Wbuf, loss, mid, side, n_calls, _ = ent
        Wbuf.copy_(Wn if isinstance(Wn, torch.Tensor) else torch.from_numpy(Wn))   # a device population: device to device
        g.replay()
        self.rendered_candidates += P
        self._n_flag_rows = min(n_calls, 255)
        return loss.clone(), {"mid": mid.clone(), "side": side.clone()}, None

    def evaluate(self, W, random_crop: bool = False, rng=np.random, want_audio: bool = False, dropout: float = 0.0,
                 parallel: bool = False, pairs=None, x: Optional[torch.Tensor] = None):
        """Fitness of every row of W -> (loss (P,), embeddings dict, normalised audio or None).  The population goes through in
        passes of at most `max_candidates_per_pass` candidates (whole pairs for a multi-pair batch), one after the other on the
        current stream; a candidate's result does not depend on how the population is cut.

        pairs: indices of the inputs / targets that the pair-major blocks of W belong to (default: all of them, in order).
        x: a ready-made evaluate-time input buffer (len(pairs), C, L) float32 on the device, used as it is -- no padding, no
        crop, nothing drawn from rng; without it the listed pairs are taken from the evaluator's own input by the length policy
        (one crop position for all).  Calls with `pairs` or `x` launch eagerly (no graph replay)."""
        subset = pairs is not None or x is not None
        Wn, pairs, B, per = self._arguments(W, pairs, x)
        if x is None:
            x = self._input(random_crop, rng, parallel)
            if pairs is not None:
                x = x[pairs].contiguous()
        P = Wn.shape[0]
        step = min(P, self.max_cand) if self.max_cand else P
        if B > 1:  # passes hold whole pairs
            step = max(per, step // per * per)
        bounds = [(p0, min(P, p0 + step)) for p0 in range(0, P, step)]
        n_full = self.x_full.shape[-1]
        cropped = not parallel and eval_length(n_full, random_crop) < n_full   # a new input buffer per call
        if (self._graph_on and self.fused and len(bounds) == 1 and dropout == 0.0 and not want_audio and not cropped and not subset and
                not torch.cuda.is_current_stream_capturing()):
            out = self._evaluate_graph(Wn, x, per)
            if out is not None:
                return out
        Wt = self._on_device(Wn)
        losses, mids, sides, audios, generic_embeds = [], [], [], [], []
        n_calls = 0
        for p0, p1 in bounds:
            Wc = Wt[p0:p1].contiguous()
            self.rendered_candidates += p1 - p0
            if self.fused:
                loss, mid, side, audio, _, n_calls = self._fused_pass(Wc, x, p0, p1, per, n_calls, dropout, want_audio, pairs)
                mids.append(mid); sides.append(side)
            else:
                (b0, b1), spans = self._spans(p0, p1, per, pairs)
                xin = x[0] if B == 1 else x[b0:b1]
                audio, peaks = render_population(self.plugins, xin, Wc, self.sample_rate, chain=self.chain, ws=self.ws)
                loss, emb = self._generic_loss(normalize_audio_(audio, peaks), spans, dropout)
                generic_embeds.append(emb)
            losses.append(loss)
            if want_audio:
                audios.append(audio)
        loss = torch.cat(losses) if len(losses) > 1 else losses[0]
        if self.fused:
            embeds = {"mid": torch.cat(mids), "side": torch.cat(sides)}
        else:
            embeds = {k: torch.cat([e[k] for e in generic_embeds]) for k in generic_embeds[0]}
        self._n_flag_rows = min(n_calls, 255)
        return loss, embeds, (torch.cat(audios) if want_audio else None)

    def _generic_loss(self, audio: torch.Tensor, spans, dropout: float):
        """style_transfer.py:531-571 for an arbitrary metric: embed_func on the normalised population (GPU tensor),
        then mean over the dict's entries of -cosine_similarity to the target entry (stito_neg_cosine)."""
        L = _hip.lib()
        embeds = self.embed_func(audio, self.model, self.sample_rate)
        if not isinstance(embeds, dict) or not embeds:
            raise ValueError("embed_func must return a non-empty dict of (batch, embed_dim) tensors")
        n = audio.shape[0]
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        out = {}
        for idx, (name, emb) in enumerate(embeds.items()):
            if name not in self.targets:
                raise KeyError(f"target embeddings have no entry {name!r}")
            emb = emb.detach().to(self.device, torch.float32).contiguous().view(n, -1)
            out[name] = emb
            tgt = self.targets[name]
            if tgt.shape[1] != emb.shape[1]:
                raise ValueError(f"{name}: candidate embeddings have {emb.shape[1]} dims, the target {tgt.shape[1]}")
            # dropout hits the style embeddings only: the reference scores the content embeddings undropped
            # (style_transfer.py:545-568: F.dropout on input_embeds[embed_name], then the content term on its own)
            drop = dropout > 0.0 and not name.startswith("__content__:")
            ed = torch.nn.functional.dropout(emb, p=dropout, training=True).contiguous() if drop else emb
            for b, q0, q1 in spans:
                _hip.check(L.stito_neg_cosine(_hip.ptr(ed[q0:q1]), q1 - q0, emb.shape[1], _hip.ptr(tgt[b]),
                                              self.entry_weights.get(name, 1.0) / len(embeds),
                                              0 if idx == 0 else 1, _hip.ptr(loss[q0:q1]), _hip.stream_ptr()))
        return loss, out

    def nan_flags(self) -> Optional[torch.Tensor]:
        return self.flags[: self._n_flag_rows].sum(dim=0)

    def nan_warning(self, flags: Optional[torch.Tensor] = None) -> Optional[str]:
        """The reference's "Warning: NaNs found in ..._embeddings" (utils.py:491-497) for the last evaluate() -- or for the
        evaluate() calls whose nan_flags() were added up into `flags`; reads the device flags, so call it after the fitness
        has been fetched (run_es does)."""
        fl = (self.nan_flags() if flags is None else flags).cpu()
        if fl.numel() and int(fl[0]):
            return "Warning: NaNs found in mid_embeddings"
        if fl.numel() and int(fl[1]):
            return "Warning: NaNs found in side_embeddings"
        return None


class MrstftEvaluator(_Evaluator):
    """The evaluate step with the multi-resolution STFT distance to the target AUDIO as the objective (auraloss's
    MultiResolutionSTFTLoss, the reference's second yardstick: scripts/eval/eval_synthetic.py:72, 368-369): render ->
    stito_mrstft_loss with process_audio's joint peak normalisation folded into the kernel's loader.  No model, no embeddings.

    x (B, C, n) and target_audio (B, C', n), C' the chain's output channels: candidates of pair b are scored against target b
    (evaluate takes the B populations stacked pair-major, like PopulationEvaluator).  The length policy is the embedding
    objective's (eval_span) and ONE span serves input and target alike: the same zero padding to 262144, the same crop, and
    under random_crop the same start.  evaluate(W, pairs=[...], x=buffer, y=buffer) scores the populations of a SUBSET of the
    pairs on ready-made buffers, the counterpart of PopulationEvaluator.evaluate(W, pairs=, x=) -- the ragged batch;
    `rendered_candidates` counts what went through the render.  Launches are eager.  stereo="sum-diff": the distance of the
    render's [L + R, L - R] to the target's (features.MrstftTarget's mode, every table is built in it); the chain must render 2
    channels.

    There are two kinds of target table.  The STATIC table of an evaluate-time length holds ALL the targets, for spans that
    never move: built once and read through a slot list.  A REFILLED table holds the targets of one call, for spans that move:
    one per (length, number of targets), rebuilt whenever the spans it holds are not the ones asked for."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], target_audio: torch.Tensor,
                 device: Optional[torch.device] = None, resolutions=None, normalize_stages: bool = False, stereo: str = "lr"):
        from . import features as _features

        if x.dim() != 3 or target_audio.dim() != 3:
            raise ValueError("input and target audio must be (batch, chs, seq_len)")
        _features._mrstft_stereo(stereo, 2)  # the name; the chain's channel count is checked below, once it is known
        if target_audio.shape[0] != x.shape[0] or target_audio.shape[-1] != x.shape[-1]:
            raise ValueError(f"target audio {tuple(target_audio.shape)} does not cover the input {tuple(x.shape)}: the MRSTFT "
                             "objective compares sample spans, so batch and length must be equal")
        _features._mrstft_res(resolutions)
        super().__init__(x, sample_rate, plugins, device, normalize_stages)
        self.resolutions = resolutions
        c_out = _hip.lib().stito_chain_out_channels(self.chain[0], len(plugins), x.shape[1])
        if stereo == "sum-diff" and c_out != 2:
            raise ValueError(f"the sum / difference distance needs 2 channels, the chain renders {c_out}")
        self.stereo = stereo
        if target_audio.shape[1] != c_out:
            raise ValueError(f"target audio has {target_audio.shape[1]} channels, the chain renders {c_out}")
        self.y_full = target_audio.to(self.device, torch.float32).contiguous()
        self._y_padded = None
        self._static = {}    # evaluate-time length -> (MrstftTarget of all targets, {pair: slot})
        self._refilled = {}  # (evaluate-time length, number of targets) -> [MrstftTarget, the spans it holds (None: a caller's y)]

    def _target_table(self, y: torch.Tensor):
        """The one place a target table is made, for y (targets, C', length) on the device: the kind of distance is the kind of
        table (MelMrstftEvaluator overrides this)."""
        from . import features as _features

        return _features.MrstftTarget(y, self.resolutions, self.stereo)

    def set_static_targets(self, length: int, pairs, y: torch.Tensor) -> None:
        """The static table of one evaluate-time length, for an evaluator whose own audio is a stand-in (the ragged batch): y
        (len(pairs), C', length) float32 on the device holds the target spans of the listed pairs, which never move.  Built
        once; evaluate(W, pairs=, x=) without y then scores any subset of these pairs through the slot list."""
        pairs = self._pairs(pairs, "targets", once=True)
        if y.dim() != 3 or y.shape[0] != len(pairs) or y.shape[-1] != int(length):
            raise ValueError(f"y must be ({len(pairs)}, chs, {int(length)}), got {tuple(y.shape)}")
        self._static[int(length)] = (self._target_table(y), {b: k for k, b in enumerate(pairs)})

    def _static_table(self, length: int):
        """-> (MrstftTarget, {pair: slot}) of ALL the targets at an evaluate-time length where no span moves: what
        set_static_targets registered, else the evaluator's own targets as they are or zero padded to 262144 (built once)."""
        ent = self._static.get(length)
        if ent is None:
            n = self.y_full.shape[-1]
            if not (length == n or n < length == CROP_LEN):
                raise ValueError(f"no static targets of {length} samples (the evaluator's own have {n}): pass y")
            y, self._y_padded = cut_to_span(self.y_full, (0, length), self._y_padded)
            ent = self._static[length] = (self._target_table(y), {b: b for b in range(self.n_inputs)})
        return ent

    def _input_and_target(self, random_crop: bool, rng, parallel: bool = False):
        """-> (x, y, span): the evaluator's own input and target under the length policy, ONE span (eval_span) for both."""
        span = eval_span(self.x_full.shape[-1], random_crop, rng, parallel)
        x, self._x_padded = cut_to_span(self.x_full, span, self._x_padded)
        y, self._y_padded = cut_to_span(self.y_full, span, self._y_padded)
        return x, y, span

    def _refilled_table(self, y: torch.Tensor, held):
        """-> the MrstftTarget of y's shape holding y.  held: what names y's spans from call to call (a table that already holds
        them is not refilled), or None for a caller's buffer, which always refills."""
        key = (y.shape[-1], y.shape[0])
        ent = self._refilled.get(key)
        if ent is None:
            ent = self._refilled[key] = [self._target_table(y), held]
        elif held is None or ent[1] != held:
            ent[0].update(y)
            ent[1] = held
        return ent[0]

    def evaluate(self, W, random_crop: bool = False, rng=np.random, want_audio: bool = False, dropout: float = 0.0,
                 parallel: bool = False, pairs=None, x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None):
        """Fitness of every row of W -> (loss (P,), {}, normalised audio or None).

        pairs / x: as PopulationEvaluator.evaluate -- the stacked populations of the listed pairs (default: all), in that order,
        on a ready-made input buffer (len(pairs), C, L) used as it is (nothing drawn from rng); without x the listed pairs are
        taken from the evaluator's own audio by the length policy.  The target side:
        y given -- (len(pairs), C', L), the target spans of exactly the listed pairs, for spans that move from call to call:
            a refilled table, and population k is scored against target k;
        x without y -- spans that never move: the static table of that length (_static_table), the listed pairs going through
            stito_mrstft_loss_slots, the slot list being the few int32 uploaded per call;
        neither -- the span of the evaluator's own targets that the length policy gave its inputs: a crop is a span that moves
            (a refilled table, which keeps the crop while the same start is drawn again), anything else is static."""
        if dropout > 0.0:
            raise ValueError("dropout acts on embeddings; the MRSTFT objective has none")
        subset = pairs is not None or x is not None or y is not None
        Wn, pairs, k, _ = self._arguments(W, pairs, x, y)
        held = None
        if x is None:
            x, own, span = self._input_and_target(random_crop, rng, parallel)
            if span[1] < self.y_full.shape[-1]:  # a crop
                y, held = own, (span, pairs)
            if pairs is not None:
                x = x[pairs].contiguous()
                y = None if y is None else y[pairs].contiguous()
        elif y is not None:
            self._ready_made(y, "y", k)
            if y.shape[-1] != x.shape[-1]:
                raise ValueError(f"y has {y.shape[-1]} samples, x {x.shape[-1]}")
        slots = None
        if y is not None:
            tgt = self._refilled_table(y, held)
        else:
            length = x.shape[-1]
            tgt, slot_of = self._static_table(length)
            if subset:
                pairs = list(range(self.n_inputs)) if pairs is None else pairs
                if any(b not in slot_of for b in pairs):
                    raise ValueError(f"pairs {pairs}: the static table of {length} samples holds the targets of {sorted(slot_of)}")
                slots = torch.tensor([slot_of[b] for b in pairs], dtype=torch.int32).to(self.device)
        Wt = self._on_device(Wn)
        audio, peaks = render_population(self.plugins, x[0] if x.shape[0] == 1 else x, Wt, self.sample_rate, self.chain, ws=self.ws)
        self.rendered_candidates += Wn.shape[0]
        loss = tgt.loss(audio, peaks, norm_passes=1, slots=slots, ws=self.ws, **self._loss_options)
        return loss, {}, (normalize_audio_(audio, peaks) if want_audio else None)

    _loss_options = {}  # what a subclass's tables take in `loss` beyond the above (WaveformEvaluator: its kind)

    def _uploaded_taps(self):
        """The prefilter taps of a subclass that has some (self.taps, host float32, or None) on the device: uploaded once, at the
        first table, and shared by all the evaluator's tables."""
        if self.taps is not None and self._taps_dev is None:
            self._taps_dev = torch.from_numpy(self.taps).to(self.device)
        return self._taps_dev


class MelMrstftEvaluator(MrstftEvaluator):
    """MrstftEvaluator with the mel-scaled distance (features.MelMrstftTarget; auraloss's scale="mel"): every table holds band sums
    of the target's magnitudes through the Slaney bank of the evaluator's sample rate with n_bins bands, channels compared L/R.
    The bank is built and checked on the host once, before the base class touches the device: a bank with an empty band is a
    ValueError naming the band, the resolution and the sample rate.  Everything else -- the length policy, static and refilled
    tables, the slot list, the folded peak -- is the base class's."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], target_audio: torch.Tensor,
                 device: Optional[torch.device] = None, resolutions=None, normalize_stages: bool = False, n_bins: int = 64):
        from . import features as _features

        self._bank = _features.mel_mrstft_bank(sample_rate, n_bins, resolutions)
        self.n_bins = int(n_bins)
        super().__init__(x, sample_rate, plugins, target_audio, device, resolutions, normalize_stages)

    def _target_table(self, y: torch.Tensor):
        from . import features as _features

        return _features.MelMrstftTarget(y, resolutions=self.resolutions, bank=self._bank)


class PrefilteredMrstftEvaluator(MrstftEvaluator):
    """MrstftEvaluator with a distance on prefiltered rows (features.PrefilteredMrstftTarget; with prefilter="aw", auraloss's
    perceptual_weighting=True at the evaluator's sample rate): render and target go through the FIR in the loss kernel's loader,
    after the folded peak normalisation (and after the sums and differences under kind "sum-diff"), before the STFT.  kind: "lr",
    "sum-diff" (the chain must render 2 channels) or "mel" (n_bins bands of the Slaney bank of the sample rate).  prefilter:
    features.mrstft_prefilter's argument.  Taps and bank are built and checked on the host, before the base class touches the
    device; the taps are uploaded once and stay on the device for the evaluator's lifetime, shared by all its tables.  Tables and
    workspace are sized by the prefiltered calls' own size functions.  Everything else is the base class's."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], target_audio: torch.Tensor,
                 device: Optional[torch.device] = None, resolutions=None, normalize_stages: bool = False, kind: str = "lr",
                 prefilter="aw", n_bins: int = 64):
        from . import features as _features

        if kind not in _features._PREFILTER_KINDS:
            raise ValueError(f"kind must be one of {sorted(_features._PREFILTER_KINDS)}, got {kind!r}")
        self.kind = kind
        self.taps = _features.mrstft_prefilter(prefilter, sample_rate)
        self._bank = _features.mel_mrstft_bank(sample_rate, n_bins, resolutions) if kind == "mel" else None
        self._taps_dev = None
        super().__init__(x, sample_rate, plugins, target_audio, device, resolutions, normalize_stages,
                         "sum-diff" if kind == "sum-diff" else "lr")

    def _target_table(self, y: torch.Tensor):
        from . import features as _features

        return _features.PrefilteredMrstftTarget(y, self.taps, kind=self.kind, resolutions=self.resolutions, bank=self._bank,
                                                 taps_dev=self._uploaded_taps())


class WaveformEvaluator(MrstftEvaluator):
    """MrstftEvaluator with a waveform distance as the objective (features.WaveformTarget, csrc/waveform.hip): kind "esr", "dc",
    "snr", "sisdr" or "logcosh" of the render, after process_audio's peak normalisation folded into the kernel, against the target
    audio -- sample against sample, so polarity, alignment and time of arrival count, which no magnitude-spectrogram distance
    sees.  prefilter: None, or features.mrstft_prefilter's argument ("aw": the A-weighting FIR of the evaluator's sample rate) --
    render and target go through it in the kernel.  Kind and taps are checked on the host, before the base class touches the
    device; the taps are uploaded once and shared by all the evaluator's tables.  A table is the target's filtered rows and their
    sums and serves every kind.  Everything else -- the length policy, static and refilled tables, pairs= / x= / y=, the slot list,
    a device-resident W, the workspace -- is the base class's."""

    def __init__(self, x: torch.Tensor, sample_rate: int, plugins: Dict[str, dict], target_audio: torch.Tensor, kind: str = "esr",
                 prefilter=None, device: Optional[torch.device] = None, normalize_stages: bool = False):
        from . import features as _features

        _features._waveform_kind(kind)
        self.kind = kind
        self.taps = _features._waveform_taps(prefilter, sample_rate)
        self._taps_dev = None
        self._loss_options = {"kind": kind}
        super().__init__(x, sample_rate, plugins, target_audio, device, None, normalize_stages)

    def _target_table(self, y: torch.Tensor):
        from . import features as _features

        return _features.WaveformTarget(y, self.taps, taps_dev=self._uploaded_taps())
