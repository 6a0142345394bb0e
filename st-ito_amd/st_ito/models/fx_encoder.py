"""FX-Encoder (Koo et al., "Music Mixing Style Transfer through Contrastive Learning"): the reference's second learned
audio-effects embedding (st_ito/models/fx_encoder.py there), written out from the published architecture.

Twelve residual blocks of one-dimensional convolutions on stereo audio at 44.1 kHz, then the mean over positions.  Block i:

    c1  = layer(x;  C_i -> C_i,     K_i, stride 1) + x        (the input is added AFTER the ReLU)
    out = layer(c1; C_i -> C_{i+1}, K_i, stride S_i)

and a layer is reflection padding of K - 1 samples (l_pad = (K - 1) // 2 left, the rest right: an even kernel pads one more on
the right), conv1d with bias, eval-mode batch norm (eps 1e-5), ReLU; its output has ceil(L / stride) positions.

The parameters live in torch modules under the reference checkpoint's key names; the forward runs on the GPU only, through
stito_fxenc_forward (csrc/fxenc.hip).  At the first forward after a load or a move the batch norm and the bias are folded to one
scale and shift per channel (float64, rounded once) and the weights are repacked into the kernel's operand layout; both are kept
until the parameters change."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import _hip

DEFAULT_CHANNELS = (16, 32, 64, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048)   # behind the stereo input's 2
DEFAULT_KERNELS = (25, 25, 15, 15, 10, 10, 10, 10, 5, 5, 5, 5)
DEFAULT_STRIDES = (4, 4, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1)
BN_EPS = 1e-5


# ------------------------------------------------ host rules (no GPU needed) ------------------------------------------------ #
def reflect_pads(kernel: int) -> Tuple[int, int]:
    """(l_pad, r_pad) of a layer: kernel - 1 samples in all, the odd one on the right."""
    pad = kernel - 1
    return pad // 2, pad - pad // 2


def out_len(n: int, stride: int) -> int:
    return -(-int(n) // int(stride))


def fold_batch_norm(bias, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv bias + eval-mode batch norm as one affine map per channel, in float64:
    scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale.  bias None: no bias."""
    f64 = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
    scale = f64(gamma) / torch.sqrt(f64(var) + eps)
    b = torch.zeros_like(scale) if bias is None else f64(bias)
    return scale, f64(beta) + (b - f64(mean)) * scale


def pack_conv1d_weights(w: torch.Tensor, bm: int, bk: int) -> torch.Tensor:
    """(cout, cin, K) -> the implicit GEMM's operand layout [ceil(cout / bm)][Rpad][bm]: element (mt, r, mi) is
    w[mt * bm + mi][r // K][r % K], zero where the channel or the reduction index r = ci * K + t runs past the end; Rpad =
    cin * K rounded up to bk.  One m tile's slab of bk reduction rows is then bk * bm consecutive floats.  bm == 0 (the
    layers with at most two input channels): the weights as they are."""
    cout, cin, k = w.shape
    if bm == 0:
        return w.detach().to(torch.float32).contiguous().reshape(-1)
    r, mt = cin * k, -(-cout // bm)
    rpad = -(-r // bk) * bk
    full = torch.zeros((mt * bm, rpad), dtype=torch.float32, device=w.device)
    full[:cout, :r] = w.detach().to(torch.float32).reshape(cout, r)
    return full.reshape(mt, bm, rpad).permute(0, 2, 1).contiguous().reshape(-1)


def unpack_conv1d_weights(packed: torch.Tensor, cout: int, cin: int, k: int, bm: int, bk: int) -> torch.Tensor:
    """The inverse of pack_conv1d_weights -> (cout, cin, K)."""
    if bm == 0:
        return packed.reshape(cout, cin, k)
    r, mt = cin * k, -(-cout // bm)
    rpad = -(-r // bk) * bk
    return packed.reshape(mt, rpad, bm).permute(0, 2, 1).reshape(mt * bm, rpad)[:cout, :r].reshape(cout, cin, k)


def layer_tiles(cout: int, cin: int, k: int, stride: int) -> Tuple[int, int]:
    """(bm, bk) of the kernel that runs this layer, from the library's one launch rule; bm == 0: the vector-ALU kernel."""
    L = _hip.lib()
    return int(L.stito_fxenc_tile_m(cout, cin, k, stride)), int(L.stito_fxenc_tile_k())


# ------------------------------------------------------- the modules -------------------------------------------------------- #
class _ConvBn(nn.Module):
    """Parameter holder named as in the checkpoint: .conv1d (weight, bias) and .batch_norm (weight, bias, running_*)."""

    def __init__(self, cin: int, cout: int, k: int, bias: bool):
        super().__init__()
        self.conv1d = nn.Conv1d(cin, cout, k, bias=bias)
        self.batch_norm = nn.BatchNorm1d(cout, eps=BN_EPS)


class _Layer(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, stride: int, bias: bool, residual: bool):
        super().__init__()
        self.conv1d = _ConvBn(cin, cout, k, bias)
        self.cin, self.cout, self.kernel, self.stride, self.residual = cin, cout, k, stride, residual


class _ResBlock(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, stride: int, bias: bool):
        super().__init__()
        self.conv1 = _Layer(cin, cin, k, 1, bias, residual=True)
        self.conv2 = _Layer(cin, cout, k, stride, bias, residual=False)


class FXencoder(nn.Module):
    """FXencoder(channels, kernels, strides, dilation): `channels` are the blocks' output widths (the stereo input's 2 is put in
    front of a copy; the arguments are never modified).  Built in eval mode; forward(x): (B, 2, L) -> (B, channels[-1]) on the GPU."""

    def __init__(self, channels: Optional[Sequence[int]] = None, kernels: Optional[Sequence[int]] = None,
                 strides: Optional[Sequence[int]] = None, dilation: Optional[Sequence[int]] = None, bias: bool = True,
                 norm: str = "batch", conv_block: str = "res", activation: str = "relu"):
        super().__init__()
        chans = [2] + [int(c) for c in (DEFAULT_CHANNELS if channels is None else channels)]
        kernels = [int(k) for k in (DEFAULT_KERNELS if kernels is None else kernels)]
        strides = [int(s) for s in (DEFAULT_STRIDES if strides is None else strides)]
        dilation = [1] * len(kernels) if dilation is None else [int(d) for d in dilation]
        if conv_block != "res":
            raise NotImplementedError(f'FXencoder(conv_block={conv_block!r}): only the residual blocks ("res") are built here')
        if norm != "batch":
            raise NotImplementedError(f'FXencoder(norm={norm!r}): only eval-mode batch norm ("batch") is built here')
        if activation != "relu":
            raise NotImplementedError(f'FXencoder(activation={activation!r}): only "relu" is built here')
        if any(d != 1 for d in dilation):
            raise NotImplementedError(f"FXencoder(dilation={dilation}): only dilation 1 is built here")
        if not (len(chans) - 1 == len(kernels) == len(strides) == len(dilation)) or not kernels:
            raise ValueError(f"FXencoder: {len(chans) - 1} channels, {len(kernels)} kernels, {len(strides)} strides, {len(dilation)} dilations")
        if min(chans) < 1 or min(kernels) < 1 or min(strides) < 1:
            raise ValueError("FXencoder: channels, kernels and strides must be positive")
        self.channels, self.kernels, self.strides = chans, kernels, strides
        self.encoder = nn.Sequential(*[_ResBlock(chans[i], chans[i + 1], kernels[i], strides[i], bias) for i in range(len(kernels))])
        self.embed_dim = chans[-1]
        self._prepared = None   # (device, _hip.FxencModel, tensors and arrays it points into)
        super().train(False)

    # ---- shapes ----
    def layers(self) -> List[Tuple[str, _Layer]]:
        return [(f"encoder.{i}.conv{j}", getattr(blk, f"conv{j}")) for i, blk in enumerate(self.encoder) for j in (1, 2)]

    def layer_lengths(self, n_samples: int) -> List[Tuple[str, int, int]]:
        """[(layer name, input length, output length)], the ceil(L / stride) rule; ValueError naming the first layer whose input
        is not longer than its right reflection."""
        out, n = [], int(n_samples)
        for name, ly in self.layers():
            r_pad = reflect_pads(ly.kernel)[1]
            if n <= r_pad:
                raise ValueError(f"FXencoder: an input of {n_samples} samples is too short: {name} (kernel {ly.kernel}) reflects "
                                 f"{r_pad} samples on the right and needs more than that, its input has {n}")
            out.append((name, n, out_len(n, ly.stride)))
            n = out[-1][2]
        return out

    def min_input_length(self) -> int:
        need = 1
        for _, ly in reversed(self.layers()):
            need = max(reflect_pads(ly.kernel)[1] + 1, (need - 1) * ly.stride + 1)
        return need

    # ---- torch plumbing ----
    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("FXencoder: training-mode batch norm is not built here (eval only)")
        return super().train(False)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts the reference checkpoint's keys; a leading `module.` (DistributedDataParallel) is stripped and
        num_batches_tracked is ignored."""
        sd = {}
        for k, v in state_dict.items():
            k = k[7:] if k.startswith("module.") else k
            if not k.endswith("num_batches_tracked"):
                sd[k] = v
        res = super().load_state_dict(sd, strict=False, **kw)
        missing = [k for k in res.missing_keys if not k.endswith("num_batches_tracked")]
        if strict and (missing or res.unexpected_keys):
            raise RuntimeError(f"FXencoder.load_state_dict: missing {missing}, unexpected {list(res.unexpected_keys)}")
        self._prepared = None
        return res

    def _apply(self, fn, *a, **k):
        self._prepared = None
        return super()._apply(fn, *a, **k)

    def _device(self) -> torch.device:
        d = next(self.parameters()).device
        return d if d.type == "cuda" else torch.device("cuda", torch.cuda.current_device())

    # ---- the GPU side ----
    def prepare(self):
        """Fold and pack once per (parameters, device)."""
        _hip.require_gpu()
        dev = self._device()
        if self._prepared is not None and self._prepared[0] == dev:
            return self._prepared
        descs = (_hip.FxencLayer * (2 * len(self.encoder)))()
        keep = []
        for d, (_, ly) in zip(descs, self.layers()):
            conv, bn = ly.conv1d.conv1d, ly.conv1d.batch_norm
            scale, shift = fold_batch_norm(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            bm, bk = layer_tiles(ly.cout, ly.cin, ly.kernel, ly.stride)
            wp = pack_conv1d_weights(conv.weight, bm, bk).to(dev)
            assert wp.numel() == _hip.lib().stito_fxenc_packed_floats(ly.cout, ly.cin, ly.kernel, ly.stride)
            sc, sh = scale.to(torch.float32).to(dev), shift.to(torch.float32).to(dev)
            keep += [wp, sc, sh]
            d.cin, d.cout, d.kernel, d.stride, d.dilation, d.residual = ly.cin, ly.cout, ly.kernel, ly.stride, 1, int(ly.residual)
            d.w_packed_dev, d.scale_dev, d.shift_dev = wp.data_ptr(), sc.data_ptr(), sh.data_ptr()
        M = _hip.FxencModel()
        M.n_layers, M.layers = len(descs), ctypes.cast(descs, ctypes.POINTER(_hip.FxencLayer))
        self._prepared = (dev, M, (descs, keep))
        return self._prepared

    def forward(self, x: torch.Tensor, ws=None) -> torch.Tensor:
        if x.dim() != 3 or x.shape[1] != self.channels[0]:
            raise ValueError(f"FXencoder: expected (batch, {self.channels[0]}, samples), got {tuple(x.shape)}")
        self.layer_lengths(x.shape[2])   # the length rule, before anything is launched
        dev, M, _ = self.prepare()
        L = _hip.lib()
        xin = x.detach().to(dev, torch.float32).contiguous()
        B, _, n = xin.shape
        nbytes = L.stito_fxenc_workspace_bytes(M, B, n)
        if nbytes == 0:
            raise ValueError(L.stito_last_error().decode("utf-8", "replace"))
        work = _hip.scratch(nbytes, dev, ws, "fxenc")
        out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=dev)
        _hip.check(L.stito_fxenc_forward(M, _hip.ptr(xin), B, n, _hip.ptr(work), work.numel(), _hip.ptr(out), _hip.stream_ptr()))
        return out


def conv1d_layer(x: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int,
                 residual: bool = False) -> torch.Tensor:
    """One fused layer on the GPU (stito_fxenc_conv1d), for tests and profiling: x (B, cin, L) float32 on the device, weight
    (cout, cin, K), scale / shift (cout) as fold_batch_norm gives them -> (B, cout, ceil(L / stride))."""
    _hip.require_gpu()
    L = _hip.lib()
    dev = x.device
    cout, cin, k = weight.shape
    bm, bk = layer_tiles(cout, cin, k, stride)
    wp = pack_conv1d_weights(weight, bm, bk).to(dev)
    sc, sh = scale.to(torch.float32).to(dev).contiguous(), shift.to(torch.float32).to(dev).contiguous()
    d = _hip.FxencLayer()
    d.cin, d.cout, d.kernel, d.stride, d.dilation, d.residual = cin, cout, k, int(stride), 1, int(residual)
    d.w_packed_dev, d.scale_dev, d.shift_dev = wp.data_ptr(), sc.data_ptr(), sh.data_ptr()
    xin = x.detach().to(torch.float32).contiguous()
    B, _, n = xin.shape
    y = torch.empty((B, cout, out_len(n, stride)), dtype=torch.float32, device=dev)
    _hip.check(L.stito_fxenc_conv1d(d, _hip.ptr(xin), B, n, _hip.ptr(y), _hip.stream_ptr()))
    return y
