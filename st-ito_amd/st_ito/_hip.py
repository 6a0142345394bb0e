"""ctypes binding of libstito_hip.so (include/stito_hip.h).

PyTorch owns device memory and streams; this module only passes raw pointers.  There is no
CPU fallback: if the library is missing or no HIP device is present, calls raise.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import torch  # noqa: F401  (must be imported first: brings in the process' libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STITO_LIB_PATH") or os.path.join(_HERE, "_lib", "libstito_hip.so")  # env: A/B builds of the library

FX_PARAMETRIC_EQ, FX_COMPRESSOR, FX_DISTORTION, FX_DELAY, FX_REVERB, FX_GAIN, FX_NOISE_REVERB, FX_CHORUS = range(8)
FX_DASP_EQ, FX_DASP_COMPRESSOR, FX_DASP_DISTORTION = 8, 9, 10  # the dasp-pytorch family of apply_* (ABI 10.2)
NORM_NONE, NORM_MINMAX, NORM_BATCHNORM = range(3)
FX_FLAG_NORMALIZE_AFTER = 1  # stito_fx_desc.flags bit 0
CONV_DIRECT, CONV_WINOGRAD, CONV_WINOGRAD_F4, CONV_WINOGRAD_F4_PRE, CONV_WINOGRAD_F4_SPLIT, CONV_WINOGRAD_F4_SPLIT2 = 0, 1, 2, 3, 4, 5
# 6, 7: retired in ABI version 9 (split-precision experiments that never beat the kernels they were meant to replace)
CONV_WINOGRAD_F2_REG = 8
CONV_WINOGRAD_F4_SPLIT3 = 9
MAX_FX_PARAMS = 32
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_HIP = -1, -2, -3, -4


class FxDesc(Structure):
    _fields_ = [
        ("kind", c_int32), ("num_channels", c_int32), ("w_offset", c_int32), ("has_bypass", c_int32),
        ("fixed_mask", c_uint32), ("flags", c_uint32), ("fixed_raw", c_double * MAX_FX_PARAMS),
        ("aux_dev", c_void_p), ("aux_len", c_int64),
    ]


class Frontend(Structure):
    _fields_ = [
        ("n_fft", c_int32), ("hop", c_int32), ("n_mels", c_int32), ("norm_mode", c_int32),
        ("window_dev", c_void_p), ("twiddle_dev", c_void_p), ("mel_start_dev", c_void_p),
        ("mel_len_dev", c_void_p), ("mel_off_dev", c_void_p), ("mel_w_dev", c_void_p),
        ("bn0_scale_dev", c_void_p), ("bn0_shift_dev", c_void_p),
        ("no_center", c_int32), ("mel_w_stride", c_int32),
    ]


class Cnn14Weights(Structure):
    _fields_ = [
        ("embed_dim", c_int32), ("n_mels", c_int32), ("channels", c_int32 * 7), ("reserved", c_int32),
        ("conv_w_dev", c_void_p * 12), ("conv_wino_dev", c_void_p * 12), ("conv_wino_algo", c_int32 * 12),
        ("bn_scale_dev", c_void_p * 12), ("bn_shift_dev", c_void_p * 12),
        ("fc_mid_wt_dev", c_void_p), ("fc_mid_b_dev", c_void_p),
        ("fc_side_wt_dev", c_void_p), ("fc_side_b_dev", c_void_p),
        ("reserved_ptr", c_void_p),
        ("conv1_f2reg_w_dev", c_void_p),
        ("conv_alt_dev", c_void_p * 12), ("conv_alt_algo", c_int32 * 12),
        ("chunk_streams", c_int32), ("chunk_first_conv", c_int32), ("chunk_last_conv", c_int32), ("reserved2", c_int32),
    ]


class MelBank(Structure):
    """stito_mel_bank: band_start / band_len on the host (checked by every call) and on the device (read by the kernel)."""
    _fields_ = [
        ("n_bins", c_int32), ("n_res", c_int32),
        ("band_start", POINTER(c_int32)), ("band_len", POINTER(c_int32)),
        ("band_start_dev", c_void_p), ("band_len_dev", c_void_p), ("weights_dev", c_void_p),
        ("w_offset", c_int64 * 8), ("w_stride", c_int32 * 8), ("w_rows", c_int32 * 8),
    ]


class FxencLayer(Structure):
    _fields_ = [
        ("cin", c_int32), ("cout", c_int32), ("kernel", c_int32), ("stride", c_int32), ("dilation", c_int32), ("residual", c_int32),
        ("w_packed_dev", c_void_p), ("scale_dev", c_void_p), ("shift_dev", c_void_p),
    ]


class FxencModel(Structure):
    _fields_ = [("n_layers", c_int32), ("reserved", c_int32), ("layers", POINTER(FxencLayer))]


class StitoError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); every symbol declared in include/stito_hip.h
SIGNATURES = {
    "stito_last_error": (c_char_p, []),
    "stito_version": (c_int, []),
    "stito_version_minor": (c_int, []),
    "stito_gather_crops": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int64, c_void_p,
                                   c_void_p]),
    "stito_fx_num_params": (c_int, [c_int]),
    "stito_chorus_lfo": (c_int, [ctypes.c_double, ctypes.c_double, c_int64, c_void_p, c_void_p]),
    "stito_dasp_compressor": (c_int, [c_void_p, c_int, c_int, c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, c_void_p, c_void_p]),
    "stito_chain_out_channels": (c_int, [POINTER(FxDesc), c_int, c_int]),
    "stito_chain_num_dims": (c_int, [POINTER(FxDesc), c_int]),
    "stito_render_workspace_bytes": (c_size_t, [POINTER(FxDesc), c_int, c_int, c_int64, c_int]),
    "stito_render_population": (c_int, [POINTER(FxDesc), c_int, c_void_p, c_int, c_int64, c_void_p, c_int, c_int,
                                        c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_render_population_multi": (c_int, [POINTER(FxDesc), c_int, c_void_p, c_int, c_int, c_int64, c_void_p, c_int,
                                              c_int, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_peak": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_normalize_audio": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_num_frames": (c_int64, [c_int64, c_int]),
    "stito_logmel": (c_int, [POINTER(Frontend), c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_cnn14_packed_conv_floats": (c_size_t, [c_int, c_int, c_int]),
    "stito_cnn14_pack_conv": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "stito_bn_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p]),
    "stito_transpose": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "stito_cnn14_workspace_bytes": (c_size_t, [POINTER(Cnn14Weights), c_int, c_int64]),
    "stito_cnn14_forward": (c_int, [POINTER(Cnn14Weights), c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "stito_debug_wino_trace": (c_int, [c_void_p]),
    "stito_conv_timing_enable": (c_int, [c_int]),
    "stito_conv_timing_read": (c_int, [POINTER(ctypes.c_double), POINTER(c_int)]),
    "stito_conv_timing_read_each": (c_int, [POINTER(ctypes.c_double), c_int, POINTER(c_int)]),
    "stito_conv_timing_read_tagged": (c_int, [POINTER(ctypes.c_double), POINTER(c_int), c_int, POINTER(c_int)]),
    "stito_cnn14_packed_conv1_f2reg_floats": (c_size_t, []),
    "stito_cnn14_pack_conv1_f2reg": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "stito_conv_block1_f2reg_supported": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "stito_conv_block1_f2reg_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "stito_conv_block1_f2reg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "stito_conv3x3_issued_flops": (c_double, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stito_conv3x3_supported": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stito_conv3x3_bn_relu": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_void_p]),
    "stito_conv3x3_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stito_conv3x3_bn_relu_ws": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "stito_num_frames_nocenter": (c_int64, [c_int64, c_int, c_int]),
    "stito_mfcc_stats": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]),
    "stito_rms_crest": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "stito_lufs_workspace_bytes": (c_size_t, [c_int, c_int64, c_int]),
    "stito_lufs": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_barkspectrum": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "stito_barkspectrum_mixed_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "stito_barkspectrum_mixed": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p,
                                         c_void_p, c_int64, c_void_p]),
    "stito_fft_mixed_plan": (c_int, [c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int]),
    "stito_mrstft_table_floats": (c_int64, [POINTER(c_int), c_int, c_int, c_int64]),
    "stito_mrstft_target": (c_int, [POINTER(c_int), c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "stito_mrstft_workspace_bytes": (c_size_t, [POINTER(c_int), c_int, c_int, c_int, c_int64]),
    "stito_mrstft_loss": (c_int, [POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "stito_mrstft_loss_slots": (c_int, [POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                        c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_mrstft_target_sd": (c_int, [POINTER(c_int), c_int, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_mrstft_loss_sd": (c_int, [POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "stito_mrstft_loss_slots_sd": (c_int, [POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                           c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the mel variants (ABI 10.8): the L/R calls with the bank after n_res; the workspace is stito_mrstft_workspace_bytes'
    "stito_mrstft_table_floats_mel": (c_int64, [POINTER(c_int), c_int, c_int, c_int, c_int64]),
    "stito_mrstft_target_mel": (c_int, [POINTER(c_int), c_int, POINTER(MelBank), c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "stito_mrstft_loss_mel": (c_int, [POINTER(c_int), c_int, POINTER(MelBank), c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                      c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_mrstft_loss_slots_mel": (c_int, [POINTER(c_int), c_int, POINTER(MelBank), c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                            c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the prefiltered variants (ABI 10.9): (kind, bank or None, taps_dev, n_taps) before the unfiltered calls' arguments; the target
    # call takes (n_targets, channels) like the _sd one; table and workspace have their own size functions
    "stito_mrstft_table_floats_pf": (c_int64, [c_int, c_int, c_int, POINTER(c_int), c_int, c_int, c_int64]),
    "stito_mrstft_workspace_bytes_pf": (c_size_t, [c_int, c_int, POINTER(c_int), c_int, c_int, c_int, c_int64]),
    "stito_mrstft_target_pf": (c_int, [c_int, POINTER(MelBank), c_void_p, c_int, POINTER(c_int), c_int, c_void_p, c_int, c_int, c_int64,
                                       c_void_p, c_void_p]),
    "stito_mrstft_loss_pf": (c_int, [c_int, POINTER(MelBank), c_void_p, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p,
                                     c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_mrstft_loss_slots_pf": (c_int, [c_int, POINTER(MelBank), c_void_p, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_int,
                                           c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the waveform distances (ABI 10.10): (kind, taps_dev, n_taps) before stito_mrstft_loss(_slots)'s arguments from audio_dev on
    "stito_waveform_tile_samples": (c_int, [c_int]),
    "stito_waveform_table_floats": (c_int64, [c_int, c_int, c_int64]),
    "stito_waveform_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int64]),
    "stito_waveform_target": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "stito_waveform_loss": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "stito_waveform_loss_slots": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                          c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "stito_spectral_centroid_workspace_bytes":(c_size_t, [c_int, c_int, c_int64]),
    "stito_spectral_centroid": (c_int, [c_void_p, c_int, c_int, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_size_t, c_void_p]),
    "stito_embed_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "stito_resample_num_samples": (c_int64, [c_int64, c_int, c_int]),
    "stito_resample_sinc": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "stito_neg_cosine": (c_int, [c_void_p, c_int, c_int, c_void_p, ctypes.c_float, c_int, c_void_p, c_void_p]),
    "stito_mean_spectrum": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "stito_savgol": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "stito_firwin2": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_void_p,
                              c_void_p, c_void_p]),
    "stito_fir": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "stito_peak_normalize": (c_int, [c_void_p, c_int, c_int, c_int64, c_float, c_float, c_void_p, c_void_p]),
    "stito_lufs_raw_workspace_bytes": (c_size_t, [c_int, c_int, c_int64, c_int]),
    "stito_lufs_raw": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                               c_size_t, c_void_p]),
    "stito_climb_init": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "stito_climb_workspace_bytes": (c_size_t, [c_int, c_int, c_int64, c_int]),
    "stito_climb_step": (c_int, [c_void_p, c_int, c_int, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the device-resident CMA-ES (ABI 10.6); every call takes (N, popsize, max_iters) after the state
    "stito_cmaes_state_bytes": (c_int64, [c_int, c_int, c_int64]),
    "stito_cmaes_state_offsets": (c_int, [c_int, c_int, c_int64, POINTER(c_int64), c_int]),
    "stito_cmaes_init": (c_int, [c_void_p, c_int, c_int, POINTER(c_double), c_double, c_double, c_double, c_uint64, c_int64, c_int, c_void_p]),
    "stito_cmaes_ask": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "stito_cmaes_tell": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_cmaes_eigen": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p]),
    "stito_cmaes_export": (c_int, [c_void_p, c_int, c_int, c_int64, POINTER(c_int64), POINTER(c_double), c_void_p]),
    "stito_cmaes_import": (c_int, [c_void_p, c_int, c_int, c_int64, POINTER(c_int64), POINTER(c_double), c_void_p]),
    "stito_cmaes_status": (c_int, [c_void_p, POINTER(c_int64), c_void_p]),
    "stito_cmaes_normals": (c_int, [c_uint64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    # the FX-Encoder (ABI 10.11)
    "stito_fxenc_out_len": (c_int64, [c_int64, c_int]),
    "stito_fxenc_tile_m": (c_int, [c_int, c_int, c_int, c_int]),
    "stito_fxenc_tile_k": (c_int, []),
    "stito_fxenc_packed_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stito_fxenc_conv1d": (c_int, [POINTER(FxencLayer), c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "stito_fxenc_pool": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "stito_fxenc_workspace_bytes": (c_size_t, [POINTER(FxencModel), c_int, c_int64]),
    "stito_fxenc_forward": (c_int, [POINTER(FxencModel), c_void_p, c_int, c_int64, c_void_p, c_size_t, c_void_p, c_void_p]),
}


def lib():
    """Load libstito_hip.so once.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StitoError(
                f"{LIB_PATH} not found: build it with `make -C st-ito_amd/csrc` "
                "(or __graft_entry__.build()).  There is no CPU fallback for this path."
            )
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int):
    if rc == 0:
        return
    msg = lib().stito_last_error().decode("utf-8", "replace")
    if rc in (E_INVALID,):
        raise ValueError(msg)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise StitoError(f"libstito_hip error {rc}: {msg}")


def require_gpu():
    if not torch.cuda.is_available():
        raise StitoError("st_ito (MI355X build): no HIP device visible; this path has no CPU fallback")


def ptr(t):
    """Device (or host) pointer of a contiguous tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor passed to libstito_hip must be contiguous"
    return c_void_p(t.data_ptr())


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def scratch(nbytes: int, device, ws=None, name: str = ""):
    """Scratch of one launch sequence: the engine.Workspace `ws`'s buffer of that name, else this call's own, in the stream's order."""
    return ws.get(name, nbytes, device) if ws is not None else torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def mel_tables(melW, dev):
    """Device tables of a (n_bins, n_mels) mel filterbank for stito_frontend: every band is one run of consecutive
    non-zero bins.  -> (mel_start, mel_len, mel_off, mel_w, mel_w_stride) in the interleaved layout: weight i of band m
    at mel_w[i * n_mels + m] (zero padded to the longest run), so that the lanes of a wave -- one band each -- read
    consecutive floats per step."""
    import numpy as np
    import torch
    melW = np.asarray(melW, dtype=np.float32)
    n_mels = melW.shape[1]
    starts, lens = [], []
    for m in range(n_mels):
        nz = np.nonzero(melW[:, m])[0]
        s, e = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        starts.append(s); lens.append(e - s)
    table = np.zeros((max(max(lens), 1), n_mels), np.float32)
    for m in range(n_mels):
        table[: lens[m], m] = melW[starts[m]: starts[m] + lens[m], m]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)  # noqa: E731
    return i32(starts), i32(lens), i32(list(range(n_mels))), torch.from_numpy(table).to(dev).contiguous(), n_mels
