/*
 * stito_hip.h -- C ABI of libstito_hip.so: the MI355X (gfx950) implementation of st-ito's
 * ES "evaluate-population" hot path.
 *
 * The reference (csteinmetz1/st-ito) is pure Python and has no FFI; the entry points below
 * are what a binding for this path replaces, one per stage of
 *     run_es.evaluate()                      st_ito/style_transfer.py:474-573
 * (file:line relative to the reference repository):
 *
 *   stito_render_population   <- the per-candidate loop over process_audio()
 *                                st_ito/style_transfer.py:45-115, 512-521 and the Basic*
 *                                plugin .process() methods st_ito/effects.py:784-959
 *   stito_normalize_audio     <- x /= clip(max|x|, 1e-8)   style_transfer.py:113
 *   stito_logmel              <- peak-normalise + mid/side + Spectrogram + LogmelFilterBank +
 *                                input_norm   st_ito/utils.py:473-474, models/panns.py:213-245
 *   stito_cnn14_*             <- Cnn14 conv stack / pooling head / fc_mid, fc_side
 *                                st_ito/models/panns.py:250-281
 *   stito_embed_loss          <- NaN scrub + F.normalize + -cosine_similarity + mean
 *                                st_ito/utils.py:491-501, style_transfer.py:544-571
 *
 * Conventions: every pointer named *_dev is a device pointer owned by the caller (PyTorch in
 * the Python host); `stream` is a hipStream_t passed as void*; all work is enqueued on that
 * stream -- or, for the streaming convolutions of stito_cnn14_forward / stito_conv3x3_bn_relu_ws
 * (ABI version 10), on library-owned side streams forked from and joined to it by events, so the
 * caller sees one stream's ordering and a hipGraph capture of `stream` captures them too -- and
 * nothing synchronises.  Functions return 0 on success and a negative STITO_E_*
 * code otherwise; stito_last_error() returns a thread-local message for the last failure.
 * No torch types appear here.  There is no CPU fallback: without a HIP device the calls fail.
 */
#ifndef STITO_HIP_H
#define STITO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STITO_OK 0
#define STITO_E_INVALID -1      /* bad argument (ValueError on the Python side) */
#define STITO_E_UNSUPPORTED -2  /* valid in the reference, not built here */
#define STITO_E_WORKSPACE -3    /* workspace too small */
#define STITO_E_HIP -4          /* a HIP runtime call failed */

/* Effect kinds; parameter order inside an effect is the reference's `parameters` dict order. */
enum {
    STITO_FX_PARAMETRIC_EQ = 0, /* effects.py:800-873, 18 params, 1-channel plugin */
    STITO_FX_COMPRESSOR = 1,    /* effects.py:876-897,  4 params, 1-channel */
    STITO_FX_DISTORTION = 2,    /* effects.py:900-916,  2 params, 1-channel */
    STITO_FX_DELAY = 3,         /* effects.py:919-934,  3 params, 2-channel in run_optim.py:395 */
    STITO_FX_REVERB = 4,        /* effects.py:937-959,  4 params, 2-channel */
    STITO_FX_GAIN = 5,          /* effects.py:532-542,  1 param  (BASELINE "gain" stage) */
    STITO_FX_NOISE_REVERB = 6,  /* effects.py:558-620 (apply_reverb -> dasp noise_shaped_reverberation), 25 params
                                   (12 band gains, 12 band decays, mix; raw values used as they are), 2-channel;
                                   convolution reverb of BASELINE.json configs[4].  Needs aux_dev / aux_len. */
    STITO_FX_CHORUS = 7,        /* effects.py:962-985 (pedalboard.Chorus = juce::dsp::Chorus<float>), 5 params (rate_hz is declared and,
                                   as in the reference's process(), not passed on: 1 Hz), 1-channel; aux_dev / aux_len: the LFO table
                                   of stito_chorus_lfo, at least n_samples long */
    /* The reference's second effect family, apply_parametric_eq / apply_compressor / apply_distortion (effects.py:545-706):
     * dasp_pytorch.functional.parametric_eq / compressor / distortion.  dasp-pytorch is an un-vendored, un-pinned dependency:
     * the three stages are restated from the library's published algorithm, PARITY UNPINNED (ABI 10.2). */
    STITO_FX_DASP_EQ = 8,       /* effects.py:651-706, 18 params (gain -18..18 dB, frequency 20..20 000 Hz, Q 0.1..10 for low shelf,
                                   four peaking sections, high shelf; RBJ, normalised by a0).  Applied as the library's sosfilt_via_fsm:
                                   H = prod rfft(b, N) / rfft(a, N), N = 2^ceil(log2(2 n - 1)), y = irfft(rfft(x, N) H)[:n], i.e.
                                   CIRCULAR filtering over N -- evaluated as the float64 recursion started from the periodic state
                                   (I - A^N)^-1 A^(N-n) s_n, coefficients in float64.  The library's own float32 evaluation is
                                   ill-conditioned at low cutoffs (0.3 of peak at 20 Hz / Q 10) and is not the target. */
    STITO_FX_DASP_COMPRESSOR = 9, /* effects.py:623-648, 6 params (threshold -60..0 dB, ratio 1..20, attack 0.1..250 ms, release
                                   10..2000 ms -- consumed and, as in the library, unused --, knee 1..24 dB, make-up 0..24 dB),
                                   lookahead_samples = 512: the signal path is delayed by 512 samples (zeros in front), the gain is
                                   not.  Side chain = sum of the channels the signal has at that point, one gain for all of them; the
                                   stage never up-mixes, whatever num_channels says.  The one-pole smoother is frequency-sampled
                                   like the EQ: started from a^(N-n) g_n / (1 - a^N). */
    STITO_FX_DASP_DISTORTION = 10, /* effects.py:545-555, 1 param (drive 0..48 dB): tanh(x 10^(drive/20)) */
    STITO_FX_NUM_KINDS = 11
};

#define STITO_MAX_FX_PARAMS 32
/* stito_fx_desc.flags bit 0: joint peak normalisation of every candidate after this stage --
 * process_audio(normalize_stages=True), style_transfer.py:106-107. */
#define STITO_FX_FLAG_NORMALIZE_AFTER 1u

/* One plugin of the chain == one entry of the reference's `plugins` dict
 * (run_optim.py:376-437, style_transfer.py:17-42). */
typedef struct {
    int32_t kind;         /* STITO_FX_* */
    int32_t num_channels; /* plugin["num_channels"]: 1 = run per channel, 2 = stereo (up-mixes mono) */
    int32_t w_offset;     /* index in w of this plugin's first slot */
    int32_t has_bypass;   /* 1: slot 0 is the dead "our_bypass" dimension (style_transfer.py:28, 89-92) */
    uint32_t fixed_mask;  /* bit p set: parameter p comes from fixed_raw[p], but still consumes a w slot
                             (style_transfer.py:79-84) */
    uint32_t flags;       /* STITO_FX_FLAG_* (ABI version 2 renamed this field from `reserved`; same offset) */
    double fixed_raw[STITO_MAX_FX_PARAMS]; /* raw [0,1] value = (v - min) / (max - min) */
    const float *aux_dev; /* STITO_FX_NOISE_REVERB: band-filtered noise bank (2, 12, aux_len) float32 on the device
                             (the library draws it afresh per call; here it is an input); NULL otherwise */
    int64_t aux_len;      /* STITO_FX_NOISE_REVERB: impulse-response length in taps (dasp default 65 536) */
} stito_fx_desc;

const char *stito_last_error(void);
/* ABI version: 10 (1 = first round; 2: stito_fx_desc.flags was `reserved`; 3: stito_cnn14_weights.conv_wino_algo;
 * 4: STITO_CONV_WINOGRAD_F4_PRE, stito_conv3x3_bn_relu_ws / stito_conv3x3_workspace_bytes; stito_frontend.mel_w_stride
 * was `reserved`: 0 keeps the packed-run layout of versions 1-3; 5: STITO_CONV_WINOGRAD_F4_SPLIT, _F4_SPLIT2,
 * _F4_SPLITK, stito_conv_timing_read_each; 6: STITO_CONV_DIRECT_SPLIT;
 * 7: STITO_CONV_WINOGRAD_F2_REG; 8: stito_conv_block1_f2reg + stito_cnn14_weights.conv1_f2reg_w_dev (appended);
 * 9: algorithms 6 and 7 and stito_conv_block1_fused / stito_cnn14_pack_conv1_fused retired;
 * STITO_CONV_WINOGRAD_F4_SPLIT3; 10: stito_cnn14_weights.chunk_* (appended), stito_conv_timing_read_tagged). */
int stito_version(void);
/* Additions since the last change of stito_version() that leave every existing symbol and struct as it is (a caller built against
 * 10.0 runs unchanged): 1 = stito_gather_crops; 2 = STITO_FX_DASP_EQ, _DASP_COMPRESSOR, _DASP_DISTORTION (kinds 8 - 10 of
 * stito_render_population(_multi); kinds 0 - 7 keep their numbers, parameter counts and bits); 3 = stito_barkspectrum_mixed,
 * stito_barkspectrum_mixed_workspace_bytes, stito_fft_mixed_plan; 4 = stito_mrstft_table_floats, stito_mrstft_target,
 * stito_mrstft_workspace_bytes, stito_mrstft_loss; 5 = stito_mrstft_loss_slots; 6 = the device-resident CMA-ES, stito_cmaes_*;
 * 7 = stito_mrstft_target_sd, stito_mrstft_loss_sd, stito_mrstft_loss_slots_sd; 8 = stito_mel_bank, stito_mrstft_table_floats_mel,
 * stito_mrstft_target_mel, stito_mrstft_loss_mel, stito_mrstft_loss_slots_mel; 9 = the prefiltered MR-STFT distances,
 * stito_mrstft_table_floats_pf, stito_mrstft_workspace_bytes_pf, stito_mrstft_target_pf, stito_mrstft_loss_pf,
 * stito_mrstft_loss_slots_pf; 10 = the waveform distances, stito_waveform_tile_samples, stito_waveform_table_floats,
 * stito_waveform_workspace_bytes, stito_waveform_target, stito_waveform_loss, stito_waveform_loss_slots; 11 = the FX-Encoder,
 * stito_fxenc_*. */
int stito_version_minor(void);

/* LFO of STITO_FX_CHORUS: lfo_dev[n] = sin(phase_n - pi) with juce::dsp::Oscillator's float phase recurrence (phase += 2 pi
 * rate / fs per sample, wrapped), n < n_samples.  The recurrence is walked on the host and copied (this call BLOCKS on `stream`
 * and must not be made while the stream is being captured); the sines are taken on the device.  Cache the table per (sample
 * rate, rate). */
int stito_chorus_lfo(double sample_rate, double rate_hz, int64_t n_samples, float *lfo_dev, void *stream);
/* dasp_pytorch.functional.compressor as st_ito/dsp.py:49-78 (apply_random_compressor) calls it: side chain = channel sum,
 * soft-knee gain computer, ONE one-pole smoothing filter with the attack constant (the library evaluates it by frequency
 * sampling on >= 2 n - 1 points = the causal recursion to FFT rounding; the release constant is unused there), make-up gain.
 * audio_dev / out_dev (n_items, channels, n_samples) float32. */
int stito_dasp_compressor(const float *audio_dev, int n_items, int channels, int64_t n_samples, double sample_rate,
                          double threshold_db, double ratio, double attack_ms, double knee_db, double makeup_gain_db,
                          float *out_dev, void *stream);
/* Number of real parameters of an effect kind (without the bypass slot), or <0. */
int stito_fx_num_params(int kind);
/* Channel count of the rendered audio for `in_channels` input channels (style_transfer.py:94-104). */
int stito_chain_out_channels(const stito_fx_desc *chain, int n_fx, int in_channels);
/* Total number of w slots the chain consumes. */
int stito_chain_num_dims(const stito_fx_desc *chain, int n_fx);

size_t stito_render_workspace_bytes(const stito_fx_desc *chain, int n_fx, int in_channels,
                                    int64_t n_samples, int pop);

/* Render every candidate of the population through the chain.
 *   x_dev        (in_channels, n_samples) float32, shared by all candidates
 *   w_dev        (pop, n_dims) float64, raw parameters in [0,1] (CMA-ES phenotypes)
 *   audio_dev    (pop, out_channels, n_samples) float32: chain output BEFORE peak normalisation
 *   peaks_dev    (pop) float32: max |audio| over channels and samples of each candidate
 * The final `x /= clip(peak, 1e-8)` of process_audio() is applied by stito_normalize_audio /
 * stito_logmel so that the audio tensor only has to be rewritten when the caller wants it. */
int stito_render_population(const stito_fx_desc *chain, int n_fx, const float *x_dev, int in_channels,
                            int64_t n_samples, const double *w_dev, int pop, int n_dims,
                            double sample_rate, float *audio_dev, float *peaks_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream);

/* Multi-pair batch (BASELINE.json configs[2]; an extension: the reference's evaluate assumes one
 * input, style_transfer.py:520, and eval_pst.py:691-765 walks its examples serially).
 *   x_dev  (n_inputs, in_channels, n_samples); pop % n_inputs == 0; candidate p reads input
 *   p / (pop / n_inputs).  Everything else as stito_render_population (= the n_inputs == 1 case). */
int stito_render_population_multi(const stito_fx_desc *chain, int n_fx, const float *x_dev, int n_inputs,
                                  int in_channels, int64_t n_samples, const double *w_dev, int pop, int n_dims,
                                  double sample_rate, float *audio_dev, float *peaks_dev, void *workspace_dev,
                                  size_t workspace_bytes, void *stream);

/* max|x| per candidate over (channels, n_samples). */
int stito_peak(const float *audio_dev, int pop, int channels, int64_t n_samples, float *peaks_dev,
               void *stream);
/* audio[p] /= clip(peaks[p], 1e-8)  (style_transfer.py:113). */
int stito_normalize_audio(float *audio_dev, int pop, int channels, int64_t n_samples,
                          const float *peaks_dev, void *stream);

/* ---- resampling in front of the path -------------------------------------------------------- */
/* torchaudio.functional.resample(x, orig_freq, new_freq) with the library defaults (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99) -- st_ito/utils.py:462-463, scripts/run_optim.py:446, 526.
 * orig / newf are the two rates divided by their gcd; width = ceil(6 * orig / (min(orig, newf) * 0.99));
 * kernel_t_dev (2 * width + orig, newf) float32: the library's kernel table transposed (host-built);
 * x_dev (rows, n_in) -> out_dev (rows, n_out), n_out = stito_resample_num_samples = ceil(newf * n_in / orig). */
int64_t stito_resample_num_samples(int64_t n_in, int orig, int newf);
int stito_resample_sinc(const float *x_dev, int rows, int64_t n_in, const float *kernel_t_dev, int orig, int newf,
                        int width, float *out_dev, int64_t n_out, void *stream);

/* ---- front end --------------------------------------------------------------------------- */
enum { STITO_NORM_NONE = 0, STITO_NORM_MINMAX = 1, STITO_NORM_BATCHNORM = 2 };

typedef struct {
    int32_t n_fft;        /* window_size (power of two, <= 4096) */
    int32_t hop;          /* hop_size */
    int32_t n_mels;       /* mel_bins (<= 256) */
    int32_t norm_mode;    /* STITO_NORM_* (Cnn14.input_norm, panns.py:233-245) */
    const float *window_dev;      /* (n_fft) analysis window (periodic Hann in the reference) */
    const float *twiddle_dev;     /* (n_fft/2, 2) cos/sin of exp(-2 pi i k / n_fft) */
    const int32_t *mel_start_dev; /* (n_mels) first FFT bin of each band */
    const int32_t *mel_len_dev;   /* (n_mels) number of consecutive bins */
    const int32_t *mel_off_dev;   /* (n_mels) offset of the band's first weight in mel_w_dev */
    const float *mel_w_dev;       /* the non-zero run of melW[:, m]: weight i of band m at mel_off[m] + i * mel_w_stride */
    const float *bn0_scale_dev;   /* (n_mels) gamma/sqrt(var+eps)        (BATCHNORM only) */
    const float *bn0_shift_dev;   /* (n_mels) beta - mean*scale          (BATCHNORM only) */
    int32_t no_center;    /* 0: frames centred with reflect padding (torchlibrosa, panns.py:147-155);
                             1: frame t starts at t*hop, no padding (torchaudio MelSpectrogram(center=False),
                             utils.py:104-113) */
    int32_t mel_w_stride; /* 0 / 1: runs packed back to back; n_mels with mel_off[m] = m: table (max run length, n_mels),
                             zero padded -- the lanes of a wave then read consecutive floats (ABI version 4; was `reserved`) */
} stito_frontend;

/* T = n_samples / hop + 1 frames (center=True, reflect padding). */
int64_t stito_num_frames(int64_t n_samples, int hop);
/* T = (n_samples - n_fft) / hop + 1 frames for no_center front ends. */
int64_t stito_num_frames_nocenter(int64_t n_samples, int n_fft, int hop);

/* audio_dev (pop, channels, n_samples) + peaks_dev (pop) = max|audio[p]|; norm_passes = how many
 * `x /= clip(max|x|, 1e-8)` the reference applies before the model: 2 for rendered candidates
 * (style_transfer.py:113 then utils.py:473-474), 1 for get_param_embeds() alone, 0 = none
 * -> logmel_dev (pop*channels, T, n_mels) float32, streams interleaved [p0_mid, p0_side, p1_mid, ...]
 * (panns.py:219-227).  channels == 1: one stream per candidate. */
int stito_logmel(const stito_frontend *fe, const float *audio_dev, const float *peaks_dev,
                 int norm_passes, int pop, int channels, int64_t n_samples, float *logmel_dev, void *stream);

/* ---- Cnn14 trunk -------------------------------------------------------------------------- */
#define STITO_CNN14_NUM_CONVS 12
/* 3x3 conv algorithm: direct implicit GEMM; Winograd F(2x2,3x3) (16 MACs per 2x2 outputs instead of 36);
 * Winograd F(4x4,3x3) (36 MACs per 4x4 outputs instead of 144: 4x fewer than direct, 1.78x fewer than F(2x2,3x3)).
 * Both Winograd forms need cin % 8 == 0, cout % 64 == 0 and a feature map whose halo patch fits LDS
 * (stito_conv3x3_supported). */
enum { STITO_CONV_DIRECT = 0, STITO_CONV_WINOGRAD = 1, STITO_CONV_WINOGRAD_F4 = 2,
       /* F(4x4,3x3) with the input transform hoisted out of the convolution: one pass writes the transformed input tiles
        * to a workspace, the convolution streams them like the weights.  Same packed weights as STITO_CONV_WINOGRAD_F4,
        * same arithmetic and results; pays off when cout >= 512 (the workgroups that share a pixel block and differ only
        * in their 64 output channels no longer repeat the transform).  Needs stito_conv3x3_bn_relu_ws (ABI version 4). */
       STITO_CONV_WINOGRAD_F4_PRE = 3,
       /* The hoisted form on the f16 matrix pipe with float32 accumulation: every float32 operand (transformed input,
        * transformed weight) travels as two f16 halves hi + lo of a power-of-two multiple of itself (22 significand bits;
        * the scale is per layer for the weights and per stream for the input, chosen from the data so that nothing
        * overflows), every product is hi hi' + hi lo' + lo hi'.  Results agree with the float32 forms to float32 rounding
        * level (not bitwise); own packing (stito_cnn14_packed_conv_floats), needs cin % 64 == 0, cout % 256 == 0 and
        * stito_conv3x3_bn_relu_ws (ABI version 5). */
       STITO_CONV_WINOGRAD_F4_SPLIT = 4,
       /* The same arithmetic per product on workgroup tiles twice as large (64 tiles x 64 channels), reached by going over the
        * input channels twice -- 18 of the 36 Winograd positions per sweep, the first sweep's share of the outputs parked in
        * the workspace: a third fewer bytes copied into LDS per MAC, which is what bounds _F4_SPLIT.  Own packing; sums in
        * a different order than _F4_SPLIT (same accuracy, not the same bits). */
       STITO_CONV_WINOGRAD_F4_SPLIT2 = 5,
       /* 6 (STITO_CONV_WINOGRAD_F4_SPLITK: split-precision products with the input transform inside the convolution) and
        * 7 (STITO_CONV_DIRECT_SPLIT: direct implicit GEMM with split operands) were experiments of rounds 3 - 4 that never beat
        * the kernels they were meant to replace; RETIRED in ABI version 9 (stito_conv3x3_supported returns 0 for them, packing
        * and launching fail with STITO_E_UNSUPPORTED).  The numbers stay reserved. */
       /* Winograd F(2x2,3x3) on the f16 matrix pipe with the same split operands, for the 64-input-channel layers (conv_block1.conv2,
        * conv_block2.conv1): the transformed WEIGHTS (16 positions x 64 x 64 as f16 hi + lo = 256 KB) stay in the registers of
        * persistent workgroups for the whole launch, the input transform is done in registers straight into the MFMA operand
        * layout (no transformed input in LDS or HBM), the raw halo patches arrive by LDS-DMA.  cin == 64, cout % 64 == 0; own
        * packing; workspace = one word per stream; stito_conv3x3_bn_relu_ws (ABI version 7).  gfx950 only by construction: a
        * workgroup needs 512 registers per wave and ~144 KB of dynamic LDS (153 KB with the first conv fused);
        * stito_conv3x3_supported / stito_conv_block1_f2reg_supported return 0 on a device whose LDS per workgroup is smaller,
        * and the trunk then takes the F(4x4,3x3) kernels for those layers. */
       STITO_CONV_WINOGRAD_F2_REG = 8,
       /* The split-precision streaming convolution on 128-tile x 128-channel workgroup tiles, in SIX sweeps over the input
        * channels (one Winograd position row per sweep; the rows' contributions to the 4 x 4 outputs accumulate in a workgroup-
        * private scratch area of the workspace): half the bytes copied into LDS per MAC of _F4_SPLIT2, which is what bounds these
        * kernels.  For the deep layers (long channel loops: the five extra passes over the outputs are + 13 % of the operand
        * stream at 2 048 input channels, + 27 % at 1 024).  cin % 64 == 0, cout % 512 == 0; own packing; the same arithmetic in the
        * same order as _F4_SPLIT2: identical results (ABI version 9). */
       STITO_CONV_WINOGRAD_F4_SPLIT3 = 9 };

typedef struct {
    int32_t embed_dim;
    int32_t n_mels;
    int32_t channels[7];   /* 1,64,128,256,512,1024,2048 */
    int32_t reserved;
    /* conv weights in the packed layout produced by stito_cnn14_pack_conv; BN folded to
     * per-channel scale/shift applied after the convolution (eval mode, panns.py:67-68) */
    const float *conv_w_dev[STITO_CNN14_NUM_CONVS];    /* STITO_CONV_DIRECT packing (required) */
    const float *conv_wino_dev[STITO_CNN14_NUM_CONVS]; /* Winograd packing of conv_wino_algo[i], or NULL: used per
                                                          layer whenever the feature map fits that kernel */
    int32_t conv_wino_algo[STITO_CNN14_NUM_CONVS];     /* STITO_CONV_WINOGRAD, _F4, _F4_PRE (these two share a packing), _F4_SPLIT, _F4_SPLIT2, _F4_SPLIT3 or STITO_CONV_WINOGRAD_F2_REG */
    const float *bn_scale_dev[STITO_CNN14_NUM_CONVS];
    const float *bn_shift_dev[STITO_CNN14_NUM_CONVS];
    const float *fc_mid_wt_dev;  /* (2048, embed_dim): fc_mid.weight transposed */
    const float *fc_mid_b_dev;   /* (embed_dim) */
    const float *fc_side_wt_dev; /* (2048, embed_dim) */
    const float *fc_side_b_dev;  /* (embed_dim) */
    const float *reserved_ptr;      /* was conv1_fused_w_dev (ABI 3 - 8: the F(4x4,3x3)-based fused block, retired in ABI 9); ignored */
    const float *conv1_f2reg_w_dev; /* stito_cnn14_pack_conv1_f2reg, or NULL (ABI v8).  With it and a
                                       STITO_CONV_WINOGRAD_F2_REG packing of conv index 1 the forward runs conv_block1 as ONE
                                       launch (stito_conv_block1_f2reg): the 64-channel full-resolution map is never stored */
    /* ABI v9: a second packing per conv (or NULL) for the calls in which the first one's kernel would not fill the device.
     * Today: conv_wino_algo[i] == STITO_CONV_WINOGRAD_F4_SPLIT3 with conv_alt_algo[i] == STITO_CONV_WINOGRAD_F4_SPLIT2 -- the
     * six-sweep kernel's workgroups are four times larger, so a small batch (fewer than 3/4 workgroup per CU) runs the
     * two-sweep kernel instead.  The two kernels do the same arithmetic in the same order: identical bits (tested), so the
     * choice cannot be seen in the results.  conv_alt_dev[i] is consulted on its own: a caller that wants conv i on the direct
     * kernel clears conv_wino_dev[i] AND conv_alt_dev[i] (with only the first one NULL a small batch still runs the alternative
     * packing). */
    const float *conv_alt_dev[STITO_CNN14_NUM_CONVS];
    int32_t conv_alt_algo[STITO_CNN14_NUM_CONVS];
    /* ABI v10: depth-first schedule of a run of convs over chunks of streams (replaces the layer-by-layer order of
     * panns.py:250-261 for that run; same results bit for bit, a stream never meets another one inside a kernel).
     * chunk_streams > 0: convs chunk_first_conv .. chunk_last_conv (indices 0 .. 11, conv_block<b>.conv<j> = 2 (b - 1) + (j - 1))
     * run on chunk_streams streams at a time with the maps between them in two chunk-sized scratch buffers that every chunk
     * reuses, so that the hand-offs of a chunk can stay in the 256 MiB Infinity Cache.  chunk_first_conv == chunk_last_conv:
     * one layer launched chunk by chunk (only its transformed input is reused).  0 = layer by layer.  Runs the forward cannot
     * schedule (they would overwrite their own input) fall back to layer by layer. */
    int32_t chunk_streams;
    int32_t chunk_first_conv;
    int32_t chunk_last_conv;
    int32_t reserved2;
} stito_cnn14_weights;

/* Number of floats of a packed conv weight for (cout, cin) and algorithm. */
size_t stito_cnn14_packed_conv_floats(int cout, int cin, int algo);
/* (cout, cin, 3, 3) PyTorch layout -> packed layout used by the MFMA kernel of `algo`
 * (Winograd: the weights are transformed, U = G g G^T, in float64, rounded once). */
int stito_cnn14_pack_conv(const float *w_oihw_dev, int cout, int cin, int algo, float *packed_dev, void *stream);
/* BN(eval) -> scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  gamma_dev == NULL:
 * identity (use_batchnorm=False). */
int stito_bn_fold(const float *gamma_dev, const float *beta_dev, const float *mean_dev,
                  const float *var_dev, double eps, int n, float *scale_dev, float *shift_dev,
                  void *stream);
/* (rows, cols) -> (cols, rows) float32 transpose (fc weights). */
int stito_transpose(const float *in_dev, int rows, int cols, float *out_dev, void *stream);

size_t stito_cnn14_workspace_bytes(const stito_cnn14_weights *w, int n_streams, int64_t n_frames);

/* logmel_dev (n_streams, T, n_mels) -> mid_dev / side_dev (n_cand, embed_dim), the raw fc outputs
 * (before L2 normalisation).  channels == 2: streams are [mid, side] pairs; channels == 1:
 * side := mid (panns.py:271-274). */
int stito_cnn14_forward(const stito_cnn14_weights *w, const float *logmel_dev, int n_cand, int channels,
                        int64_t n_frames, float *mid_dev, float *side_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);

/* Individual layers, exposed for parity tests and profiling.
 * Activations are channel-blocked: a map with C channels (C % 8 == 0) is (n, C/8, H, W, 8) float32;
 * the 1-channel input of the first conv is (n, H, W).
 * in (n, cin/8, H, W, 8) -> out (n, cout/8, H', W', 8), y = relu(conv3x3(x) * scale + shift),
 * pool != 0: 2x2 average pooling (floor). */
/* conv_block1 in one launch (panns.py:250, ConvBlock 65-80): y = pool?(relu(bn2(conv3x3(relu(bn1(conv3x3(x))))))) for a
 * 1-channel input x (n, H, W) -- the log-mel image -- on the register-resident F(2x2,3x3) kernel (STITO_CONV_WINOGRAD_F2_REG;
 * ABI v8; the F(4x4,3x3)-based stito_conv_block1_fused of ABI 3 - 8, 11.4 ms against this one's 5.4, was retired in ABI 9).
 * out_dev (n, cout/8, H', W', 8).  The first conv (c1 = 64 channels, bn1, ReLU) is evaluated on the f16 matrix pipe (4 x 4 window
 * x 32 channels x 32 pixels per product; operands split into f16 hi + lo like the second conv's, three products, f32
 * accumulate) straight into the LDS patch ring of the second conv, in the instruction slots where the unfused kernel issues
 * its patch copies.
 *   packed_w1_dev  stito_cnn14_pack_conv1_f2reg(w1 (c1,1,3,3), bn1 scale, bn1 shift): stito_cnn14_packed_conv1_f2reg_floats()
 *   packed_w2_dev  STITO_CONV_WINOGRAD_F2_REG packing of w2 (cout, c1, 3, 3);  scale2_dev / shift2_dev (cout)
 *   workspace      stito_conv_block1_f2reg_workspace_bytes (per-stream scales of the log-mel operand)
 *   amax_out_dev   NULL, or n zeroed words: per-stream maxima of the output (bit patterns) for a split-precision layer behind
 * |x| must stay below 2^29 (log-mel values do: dB); needs c1 == 64, cout % 64 == 0. */
size_t stito_cnn14_packed_conv1_f2reg_floats(void);
int stito_cnn14_pack_conv1_f2reg(const float *w_oihw_dev, const float *scale_dev, const float *shift_dev, int c1, float *packed_dev,
                                 void *stream);
int stito_conv_block1_f2reg_supported(int n, int H, int W, int c1, int cout, int pool);
size_t stito_conv_block1_f2reg_workspace_bytes(int n, int H, int W, int c1, int cout, int pool);
int stito_conv_block1_f2reg(const float *x_dev, const float *packed_w1_dev, const float *packed_w2_dev, const float *scale2_dev,
                            const float *shift2_dev, float *out_dev, int n, int H, int W, int c1, int cout, int pool,
                            void *workspace_dev, size_t workspace_bytes, void *stream, unsigned *amax_out_dev);
/* Profiling aid: with buf_dev != NULL the Winograd launches use an instrumented instantiation whose
 * workgroup 100 records s_memtime stamps of 32 chunks x 12 waves x 8 phases (int64) into buf_dev;
 * NULL (default) restores the plain kernel.  Thread-local.  See tools/wino_timeline.py. */
int stito_debug_wino_trace(long long *buf_dev);
/* Measurement aid (bench.py "roofline"): while enabled, stito_cnn14_forward brackets every f32-MFMA
 * conv launch (cin % 8 == 0: 11 of the 12 convs) with hipEventRecord on the launch stream.
 * stito_conv_timing_read waits for the recorded events, returns their summed elapsed time and the
 * number of launches, and clears the list.  The switch and the event list are thread-local (one host thread per
 * GPU, like stito_last_error): enable and read from the thread that calls stito_cnn14_forward. */
int stito_conv_timing_enable(int on);
int stito_conv_timing_read(double *total_ms, int *n_launches);
/* The same per launch, in launch order (bench.py attributes the launches to the matrix pipe they run on): fills
 * ms_each[0 .. min(cap, n) - 1], returns n in *n_launches and clears the list. */
int stito_conv_timing_read_each(double *ms_each, int cap, int *n_launches);
/* The same with the conv index (0 .. 11; 1 for conv_block1 in one launch) of every launch in conv_each (may be NULL): with a
 * chunked schedule a layer is several launches per pass (ABI v10). */
int stito_conv_timing_read_tagged(double *ms_each, int *conv_each, int cap, int *n_launches);
/* FLOPs of the MFMA instructions one launch of this shape issues with `algo`, tile padding included (0 if unsupported or
 * cin % 8 != 0; STITO_CONV_WINOGRAD_F4_SPLIT: the three f16 products per element, i.e. f16-pipe FLOPs).  Measurement aid: bench.py divides it by the launch time for `roofline.achieved`. */
double stito_conv3x3_issued_flops(int n, int H, int W, int cin, int cout, int pool, int algo);
/* 1 if stito_conv3x3_bn_relu can run this shape with `algo`, else 0. */
int stito_conv3x3_supported(int n, int H, int W, int cin, int cout, int pool, int algo);
int stito_conv3x3_bn_relu(const float *in_dev, const float *packed_w_dev, const float *scale_dev,
                          const float *shift_dev, float *out_dev, int n, int H, int W, int cin, int cout,
                          int pool, int algo, void *stream);
/* The same with a workspace, for the algorithms that need one (STITO_CONV_WINOGRAD_F4_PRE / _F4_SPLIT / _F4_SPLIT2 / _F4_SPLIT3: the transformed
 * input; STITO_CONV_WINOGRAD_F2_REG: per-stream maxima of the input; stito_conv3x3_workspace_bytes; 0 bytes / NULL for the others). */
size_t stito_conv3x3_workspace_bytes(int n, int H, int W, int cin, int cout, int pool, int algo);
int stito_conv3x3_bn_relu_ws(const float *in_dev, const float *packed_w_dev, const float *scale_dev,
                             const float *shift_dev, float *out_dev, int n, int H, int W, int cin, int cout,
                             int pool, int algo, void *workspace_dev, size_t workspace_bytes, void *stream);
/* Test hook, exported but NOT part of the declared ABI (so not in st_ito/_hip.py's SIGNATURES either: the bit fixtures of
 * tests/golden/make_w43_epilogue_sha.py are recorded with libraries from before it existed, which must still load):
 *     int stito_conv3x3_bn_relu_ws_amax(<the arguments of stito_conv3x3_bn_relu_ws>, unsigned *amax_out_dev);
 * the same launch, also reporting what the trunk hands from one layer to the next: amax_out_dev = n words the caller zeroed,
 * word s = the bit pattern of stream s's largest output (>= 0 after ReLU), or NULL.  STITO_E_INVALID for an algorithm that
 * does not report maxima (the F(4x4,3x3) family and STITO_CONV_WINOGRAD_F2_REG do). */

/* ---- hand-crafted features: st_ito/features.py (alternative metrics of the evaluation harness) ---- */
/* compute_rms_energy (features.py:235-245) and compute_crest_factor (248-264) of (n_items, channels, n) audio
 * -> rms_dev, crest_dev (n_items, channels). */
int stito_rms_crest(const float *audio_dev, int n_items, int channels, int64_t n_samples, float *rms_dev,
                    float *crest_dev, void *stream);
/* compute_lufs (features.py:267-299): the reference's per-sample cross-channel normalisation, mono duplicated, then
 * pyloudnorm.Meter(sr).integrated_loudness (ITU-R BS.1770-4; un-vendored: restated, parity unpinned): K-weighting in float64
 * (kweight_coef_dev: n_items rows of 32 doubles, six sections b0 b1 b2 a1 a2 -- the two K-weighting biquads, then identity
 * rows 1 0 0 0 0), 400 ms blocks at 75 % overlap with the HOST's integer block edges block_lo/hi_dev (n_blocks; they are
 * pyloudnorm's int() of float products), inv_block_len = 1 / (0.4 sr), absolute gate -70 LUFS, relative gate -10 LU.
 * lufs_dev (n_items) float32, -inf for silence. */
size_t stito_lufs_workspace_bytes(int n_items, int64_t n_samples, int n_blocks);
int stito_lufs(const float *audio_dev, int n_items, int channels, int64_t n_samples, const double *kweight_coef_dev,
               const int *block_lo_dev, const int *block_hi_dev, int n_blocks, double inv_block_len, float *lufs_dev,
               void *workspace_dev, size_t workspace_bytes, void *stream);
/* ---- rule-based style transfer: run_rule_based (style_transfer.py:163-278), csrc/matcheq.hip + features.hip ---------------- */
/* get_average_spectrum (style_transfer.py:168-181): mono mix (l + r) / 2 of a stereo item, torch.stft(n_fft, hop n_fft/4,
 * rectangular window, centred, reflect pad, normalized=True), |X| averaged over frames -> out_dev (n_items, n_fft/2 + 1).
 * n_fft a power of two in [2048, 32768]; n_samples > n_fft / 2.  twiddle_dev: n_fft/2 complex exp(-2 pi i k / n_fft) (float32). */
int stito_mean_spectrum(const float *audio_dev, int n_items, int channels, int64_t n_samples, int n_fft, const float *twiddle_dev,
                        float *out_dev, void *stream);
/* scipy.signal.savgol_filter(row, window, polyorder) with mode "interp" (smooth_spectrum, style_transfer.py:163-165) on every row
 * of in_dev (n_rows, n_cols) float32 -> out_dev float32, sums in float64.  coef_dev (window) doubles: savgol_coeffs in
 * correlation order (reversed); edge_dev (window, window) doubles: row r = the polynomial fit's value at point r as weights on
 * the window's inputs (the first / last window / 2 rows serve the two edges).  window odd, <= n_cols; not in place. */
int stito_savgol(const float *in_dev, int n_rows, int n_cols, const double *coef_dev, int window, const double *edge_dev,
                 float *out_dev, void *stream);
/* scipy.signal.firwin2(n_taps, freq, gain) (style_transfer.py:235-240) per item, float64, one workgroup each.
 *   gain = num / den in float32 with its last element set to 0 (the matched-EQ response), or num itself when den_dev is NULL;
 *   num_dev / den_dev (n_items, n_freq) float32; freq_dev (n_freq) doubles, ascending from 0 to nyq;
 *   grid_dev (n_grid) doubles: np.linspace(0, nyq, n_grid), n_grid = 1 + 2**ceil(log2(n_taps));
 *   phase_b = -(n_taps - 1) / 2 * pi, inv_nyq = 1 / nyq; window_dev (n_taps) doubles (symmetric Hamming);
 *   taps_dev (n_items, n_taps) doubles.  n_taps in [16, 4096]. */
int stito_firwin2(const float *num_dev, const float *den_dev, int n_items, int n_freq, const double *freq_dev, const double *grid_dev,
                  int n_grid, int n_taps, double phase_b, double inv_nyq, const double *window_dev, double *taps_dev, void *stream);
/* scipy.signal.lfilter(taps[item], [1.0], x) on every channel (style_transfer.py:243): causal FIR, zero initial state, float64
 * products and sums rounded to float32 once.  x_dev / y_dev (n_items, channels, n_samples), not in place; taps_dev
 * (n_items, n_taps) doubles, n_taps <= 4096. */
int stito_fir(const float *x_dev, int n_items, int channels, int64_t n_samples, const double *taps_dev, int n_taps, float *y_dev,
              void *stream);
/* In place: x = (x / d) * gain per item, d = max|x| over the item (NaN-propagating, like torch.max), clamped to clamp_min when
 * clamp_min > 0 (a NaN peak stays NaN, like torch.clamp).  peaks_dev (n_items) float32 receives the peaks. */
int stito_peak_normalize(float *audio_dev, int n_items, int channels, int64_t n_samples, float clamp_min, float gain,
                         float *peaks_dev, void *stream);
/* pyloudnorm.Meter(sr).integrated_loudness on the raw channels (style_transfer.py:250-252): like stito_lufs but without the
 * cross-channel normalisation and with a mono item measured as one channel; kweight_coef_dev: n_items rows as stito_lufs;
 * lufs_dev (n_items) float64, -inf for silence. */
size_t stito_lufs_raw_workspace_bytes(int n_items, int channels, int64_t n_samples, int n_blocks);
int stito_lufs_raw(const float *audio_dev, int n_items, int channels, int64_t n_samples, const double *kweight_coef_dev,
                   const int *block_lo_dev, const int *block_hi_dev, int n_blocks, double inv_block_len, double *lufs_dev,
                   void *workspace_dev, size_t workspace_bytes, void *stream);
/* The compressor hill-climb (style_transfer.py:254-268), every item in lockstep, state on the device: threshold_dev, delta_dev
 * (n_items) doubles, active_dev, steps_dev (n_items) ints.  stito_climb_init: threshold 0, delta = target - input loudness,
 * active = delta > 0.25.  stito_climb_step: for every item, Compressor(threshold, ratio 3, attack 1 ms, release 100 ms) of
 * audio_dev into a scratch copy, x / max|x| * 10^(-12/20) in float32, raw loudness; then, for active items only, the scratch
 * becomes audio_dev, delta = target - loudness, threshold -= 0.5, steps += 1, active = delta > 0.25 && threshold > -80.
 * The caller loops (at most 160 steps) and may read active_dev to stop early.  Meter arguments as stito_lufs_raw. */
int stito_climb_init(const double *input_lufs_dev, const double *target_lufs_dev, int n_items, double *threshold_dev,
                     double *delta_dev, int *active_dev, int *steps_dev, void *stream);
size_t stito_climb_workspace_bytes(int n_items, int channels, int64_t n_samples, int n_blocks);
int stito_climb_step(float *audio_dev, int n_items, int channels, int64_t n_samples, double sample_rate,
                     const double *kweight_coef_dev, const int *block_lo_dev, const int *block_hi_dev, int n_blocks,
                     double inv_block_len, const double *target_lufs_dev, double *threshold_dev, double *delta_dev,
                     int *active_dev, int *steps_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* compute_barkspectrum (features.py:166-232).  mode 0 mono / 1 stereo / 2 mid-side; fft_size a power of two
 * <= 32768 (hop fft_size/4, rectangular window, centred, reflect pad); twiddle_dev: fft_size/2 complex
 * exp(-2 pi i k / fft_size); fb_dev (n_bands, fft_size/2 + 1): barkscale_fbanks transposed;
 * out_dev (n_items, n_signals * n_bands), L2-normalised rows. */
int stito_barkspectrum(const float *audio_dev, int n_items, int channels, int64_t n_samples, int mode, int fft_size,
                       const float *twiddle_dev, const float *fb_dev, int n_bands, float *out_dev, void *stream);
/* compute_spectral_centroid (features.py:302-333): Hann 2048 / hop 1024 magnitude STFT, centroid per frame,
 * nan_to_num, adaptive average pooling to 10, / Nyquist -> out_dev (n_items, channels * 10).
 * window_dev: 2048 floats; twiddle_dev: 1024 complex exp(-2 pi i k / 2048). */
size_t stito_spectral_centroid_workspace_bytes(int n_items, int channels, int64_t n_samples);
int stito_spectral_centroid(const float *audio_dev, int n_items, int channels, int64_t n_samples, double sample_rate,
                            const float *window_dev, const float *twiddle_dev, float *out_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream);

/* ---- bark spectrum at any 7-smooth FFT size (ABI 10.3; csrc/fft_mixed.hip) -------------------------------------------------- */
/* The same quantity as stito_barkspectrum for an even fft_size in [128, 96000] whose prime factors all lie in {2, 3, 5, 7}
 * (44 100, 48 000, 22 050, 32 000, 88 200, 96 000, ...; powers of two included, though stito_barkspectrum keeps serving them).
 * The reference's MIR metric calls compute_barkspectrum(x, sample_rate, mode="mono") (utils.py:83), which binds the sample
 * rate to fft_size: this entry is what makes that binding computable.
 *
 * The real frame is packed as N2 = fft_size / 2 complex points and transformed by the four-step scheme over N2 = na * nb
 * (nb the largest divisor of N2 not above sqrt(N2), na = N2 / nb <= 512): nb Stockham transforms of length na in LDS, the
 * twiddle, a transposing store to a workgroup-private slab of N2 complex floats in the workspace, na transforms of length nb
 * in LDS written back over the slab in natural order, then the E/O unpacking of the real spectrum.  The time mean of |X| is
 * summed by one owner thread per bin, frames in order, in a private row of the workspace: the same input gives the same
 * bits on every launch and a row does not depend on the batch around it.
 *
 * stito_fft_mixed_plan (host only, touches no device): the factorisation the launch uses.  Returns the number of radices
 * written to radices[] -- first those of na, then those of nb, each in {2, 3, 4, 5, 7}, the product of each group equal to
 * *na and *nb, *na * *nb == fft_size / 2 -- or STITO_E_UNSUPPORTED (odd, outside [128, 96000], a prime factor above 7; the
 * message names the length) or STITO_E_INVALID (max_radices too small, NULL pointers).
 *
 * tables_dev: tables_len = na + nb + 2 * N2 complex float32 (re, im), every entry cos / sin taken in float64 and rounded:
 *   [0, na)                 exp(-2 pi i m / na)                       roots of the length-na transforms
 *   [na, na + nb)           exp(-2 pi i m / nb)                       roots of the length-nb transforms
 *   [na + nb, +N2)          exp(-2 pi i (n2 k1 mod N2) / N2) at n2 * na + k1     the four-step twiddle, in the slab's order
 *   [na + nb + N2, +N2)     exp(-2 pi i k / fft_size), k < N2         the unpacking twiddle
 * fb_dev, out_dev, mode: as stito_barkspectrum.  n_samples > fft_size / 2 (reflect padding).  The workspace holds, per
 * (item, signal), the slab and the row of sums; stito_barkspectrum_mixed_workspace_bytes returns 0 for arguments the launch
 * would refuse.  `stream` is a hipStream_t. */
int64_t stito_barkspectrum_mixed_workspace_bytes(int n_items, int n_sig, int fft_size);
int stito_barkspectrum_mixed(const float *audio_dev, int n_items, int channels, int64_t n_samples, int mode, int fft_size,
                             const void *tables_dev, int64_t tables_len, const float *fb_dev, int n_bands, float *out_dev,
                             void *ws_dev, int64_t ws_bytes, void *stream);
int stito_fft_mixed_plan(int fft_size, int *na, int *nb, int *radices, int max_radices);

/* MFCC statistics of get_mfcc_feature_embeds (utils.py:116-159) on top of stito_logmel's 10 log10(mel power):
 * logmel_dev (n_items * channels, T, n_mels); per item: clamp to (max over the item's channels, bands and
 * frames) - top_db (torchaudio amplitude_to_DB); per frame: DCT with dct_dev (n_mels, n_mfcc); over frames:
 * mean, unbiased std, max per coefficient -> out_dev (n_items, channels * 3 * n_mfcc) = per channel
 * [mean | std | max], rows L2-normalised.  n_mfcc <= 32; any number of frames T >= 2. */
int stito_mfcc_stats(const float *logmel_dev, int n_items, int channels, int64_t n_frames, int n_mels,
                     const float *dct_dev, int n_mfcc, float top_db, float *out_dev, void *stream);

/* ---- ragged multi-pair batches (ABI 10.1; an extension like stito_render_population_multi) ---- */
/* The evaluate-time inputs of pairs whose files differ in length (style_transfer.py:505-518: crop to, or zero-pad to, 262144 samples),
 * cut in ONE launch out of a buffer that holds every input once:
 *   packed_dev  (packed_floats) float32: input b is (channels, length[b]) row-major at packed_dev + offset[b]
 *   offset_dev, length_dev, start_dev  (n_pairs) int64 on the device; start[b] is this call's crop position of pair b
 *   slots_dev   (n_slots) int32 on the device: the pairs to gather, in output order (any subset, any order)
 *   out_dev     (n_slots, channels, crop_len) float32: out[s][c][i] = input slots[s], channel c, sample start + i, and 0 where
 *               start + i lies outside [0, length)
 * A slot that names no pair, and a pair whose (offset, length) does not lie inside packed_floats, give zeros: nothing outside
 * the packed buffer is read.  Rows whose source address is 16-byte aligned (offset + c * length + start a multiple of 4 floats
 * from an aligned base, crop_len % 4 == 0) move 16 bytes per lane, the others one dword per lane. */
int stito_gather_crops(const float *packed_dev, int64_t packed_floats, const int64_t *offset_dev, const int64_t *length_dev,
                       const int64_t *start_dev, int n_pairs, const int32_t *slots_dev, int n_slots, int channels,
                       int64_t crop_len, float *out_dev, void *stream);

/* ---- multi-resolution STFT distance as an objective (ABI 10.4; csrc/mrstft.hip) ---------------------------------------------- */
/* auraloss.freq.MultiResolutionSTFTLoss()(x, y) per item (scripts/eval/eval_synthetic.py:72, 368-369 of the reference; auraloss is
 * un-vendored: restated, PARITY UNPINNED), x the estimate and y the reference.  res: n_res (1 .. 8) triples (n_fft, hop, win) of
 * ints, n_fft a power of two in [256, 4096], 1 <= win <= n_fft, hop >= 1; the library's defaults are (1024, 120, 600), (2048, 240,
 * 1200), (512, 50, 240).  Per row of n_samples > max n_fft / 2 samples and resolution: torch.stft's framing -- reflect padding of
 * n_fft / 2, frame t = padded samples [t hop, t hop + n_fft), t < 1 + n_samples / hop, the periodic Hann of `win` points at offset
 * (n_fft - win) / 2, one-sided --, |X| = sqrt(max(re^2 + im^2, 1e-8)), sc = || |Y| - |X| ||_F / || |Y| ||_F, lm = mean |ln|X| - ln|Y||;
 * an item's loss = the mean over resolutions of the mean over its channel rows of sc + lm.  Not symmetric in x and y.
 *
 * stito_mrstft_target: y_dev (rows, n_samples) -> table_dev (stito_mrstft_table_floats floats, 16-byte aligned): the FFT twiddles
 * and windows of every resolution, per row and resolution the clamped magnitudes (frames x bins, bins contiguous), and sum |Y|^2
 * per (row, resolution) in float64 (tile sums added in a fixed order; the table holds their scratch too).
 *
 * stito_mrstft_loss: audio_dev (pop, channels, n_samples), channels <= 8, scored against a table of n_targets * channels rows built
 * with the SAME res and n_samples: candidate p against target p / (pop / n_targets), the convention of
 * stito_render_population_multi.  norm_passes 1 folds x / clip(peaks_dev[p], 1e-8) into the sample loader (stito_logmel's way: the
 * normalised population is never written); 0: audio as it is, peaks_dev may be NULL.  -> loss_dev (pop) float32.
 * Each (row, resolution) is cut into tiles of consecutive frames; a tile's sample span is loaded into LDS once, the spectra and the
 * candidate's magnitudes never leave the CU; per-tile sums (float64) go to the workspace (stito_mrstft_workspace_bytes, 8-byte
 * aligned) and a second launch adds them in a fixed order: no atomics, and a candidate's loss has the same bits at every position
 * of every batch, for every n_targets.  The table kernel and the candidate kernel share the FFT and magnitude code, so
 * loss(y, table(y)) with norm_passes 0 is exactly 0.  The size functions return 0 for arguments the launches refuse.
 *
 * stito_mrstft_loss_slots (ABI 10.5): stito_mrstft_loss for a SUBSET of the table's targets.  The population is n_slots stacked
 * populations of pop / n_slots candidates (pop % n_slots == 0); candidate p belongs to population k = p / (pop / n_slots) and is
 * scored against table target target_slot_dev[k] (n_slots int32 on the device): any subset of the n_targets targets, in any order,
 * repeats allowed -- the batch whose stopped pairs drop out without the table being rebuilt.  A slot outside [0, n_targets) gives
 * NaN for that population's losses, reads nothing from the table and leaves the other populations' bits as they are (the contract
 * of stito_gather_crops for a slot that names no pair).  Workspace: stito_mrstft_workspace_bytes(pop, ...), as before.  Same
 * kernels, same fixed-order sums: a candidate's loss has the same bits under every slot list as under stito_mrstft_loss on a table
 * that holds only its target, and stito_mrstft_loss is this call with the identity map (n_slots = n_targets, slot k = k).
 *
 * The sum / difference variants (ABI 10.7): auraloss.freq.SumAndDifferenceSTFTLoss with both weights 1 (restated, PARITY UNPINNED) --
 * the distance above of the 2-channel signal [ch0 + ch1, ch0 - ch1] of every item, no factor 1/2: an item's loss is the mean over
 * resolutions of the mean over the two rows {sum, difference} of sc + lm.  stito_mrstft_target_sd: y_dev (n_targets, 2, n_samples)
 * -> a table of 2 n_targets rows (stito_mrstft_table_floats(res, n_res, 2 * n_targets, n_samples) floats), row 2 t the sum row and
 * row 2 t + 1 the difference row of target t.  stito_mrstft_loss_sd / stito_mrstft_loss_slots_sd: stito_mrstft_loss /
 * stito_mrstft_loss_slots against such a table, every argument as there (workspace: stito_mrstft_workspace_bytes(pop, 2, ...)); the
 * loader reads both channels of a candidate and forms xL r + xR r, respectively xL r - xR r (r = 1 / clip(peaks_dev[p], 1e-8) under
 * norm_passes 1, else 1; two products and one add).  Everything behind the loader is the code above, so the same promises hold:
 * fixed-order sums, the same bits at every position of every batch and under every slot list, loss(y, table_sd(y)) exactly 0, NaN
 * for a slot that names no target.  channels must be 2: anything else is STITO_E_INVALID.  A table and the loss scored against it
 * must be of the same kind; the table does not record which. */
int64_t stito_mrstft_table_floats(const int *res, int n_res, int rows, int64_t n_samples);
int stito_mrstft_target(const int *res, int n_res, const float *y_dev, int rows, int64_t n_samples, float *table_dev, void *stream);
size_t stito_mrstft_workspace_bytes(const int *res, int n_res, int pop, int channels, int64_t n_samples);
int stito_mrstft_loss(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                      const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                      void *workspace_dev, size_t workspace_bytes, void *stream);
int stito_mrstft_loss_slots(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                            const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop,
                            int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                            void *stream);
int stito_mrstft_target_sd(const int *res, int n_res, const float *y_dev, int n_targets, int channels, int64_t n_samples,
                           float *table_dev, void *stream);
int stito_mrstft_loss_sd(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                         const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
int stito_mrstft_loss_slots_sd(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                               const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop,
                               int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                               void *stream);

/* The mel variants (ABI 10.8): auraloss.freq.MultiResolutionSTFTLoss(scale="mel", n_bins=, sample_rate=) (restated, PARITY UNPINNED).
 * Framing, window and clamped magnitude |X| are those above; per resolution M = F |X| with a bank F of n_bins bands over the n_fft / 2
 * + 1 bins, and sc = || M_y - M_x ||_F / || M_y ||_F, lm = mean | ln M_x - ln M_y | over frames x n_bins; an item's loss is the mean
 * over resolutions of the mean over its channel rows (L/R) of sc + lm.  The bank is the caller's: every band is ONE run of consecutive
 * bins, band m of resolution i covering bins [band_start[i n_bins + m], + band_len[i n_bins + m]) with weight j of the run at
 * weights_dev[w_offset[i] + j * w_stride[i] + m] -- the interleaved layout of stito_frontend.mel_w_dev: the lanes of a wave, one band
 * each, read consecutive floats per step; w_rows[i] rows (the longest run of the resolution, shorter runs zero padded) of w_stride[i]
 * >= n_bins floats.  band_start / band_len are given twice: on the HOST, where every call checks them before it asks the device
 * anything, and on the device, where the kernel reads them (it cuts a run to the bins and rows that exist, so tables that differ from
 * the checked ones cannot make it read outside).  STITO_E_INVALID: n_bins outside [1, 256], n_res other than the call's, a band longer
 * than the bins or than w_rows, a band that starts beyond the bins or runs past them, w_stride < n_bins, a null table.  A band of
 * length 0 is accepted here and gives M = 0, hence NaN, as in auraloss: the Python layer refuses such a bank.  A sum of magnitudes is
 * a chain of fmas in bin order, so with the identity bank (n_bins = n_fft / 2 + 1, band k = bin k, weight 1) every term is the
 * linear kernels' float32 value.
 * stito_mrstft_table_floats_mel: the floats of a table of `rows` rows, smaller than the linear one (frames x n_bins per row and
 * resolution).  stito_mrstft_target_mel / _loss_mel / _loss_slots_mel: stito_mrstft_target / _loss / _loss_slots with the bank after
 * n_res, every other argument and every promise as there: candidate p against target p / (pop / n_targets), norm_passes folds the
 * peak into the loader, a slot that names no target gives NaN and disturbs nobody else, the same bits at every position of every
 * batch and under every slot list, loss(y, table_mel(y)) exactly 0.  The workspace does not depend on the bank:
 * stito_mrstft_workspace_bytes holds.  The same bank must be given to the table and to the loss; the table does not record it. */
typedef struct stito_mel_bank {
    int32_t n_bins;                 /* bands per resolution, 1 .. 256 */
    int32_t n_res;                  /* resolutions the tables cover */
    const int32_t *band_start;      /* HOST  [n_res][n_bins] */
    const int32_t *band_len;        /* HOST  [n_res][n_bins] */
    const int32_t *band_start_dev;  /* the same two tables on the device */
    const int32_t *band_len_dev;
    const float *weights_dev;       /* device; resolution i at w_offset[i] */
    int64_t w_offset[8];
    int32_t w_stride[8];
    int32_t w_rows[8];
} stito_mel_bank;
int64_t stito_mrstft_table_floats_mel(const int *res, int n_res, int n_bins, int rows, int64_t n_samples);
int stito_mrstft_target_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *y_dev, int rows, int64_t n_samples,
                            float *table_dev, void *stream);
int stito_mrstft_loss_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *audio_dev, const float *peaks_dev,
                          int norm_passes, const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples,
                          float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int stito_mrstft_loss_slots_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *audio_dev, const float *peaks_dev,
                                int norm_passes, const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots,
                                int pop, int channels, int64_t n_samples, float *loss_dev, void *workspace_dev,
                                size_t workspace_bytes, void *stream);

/* The prefiltered variants (ABI 10.9): the three distances above on rows that went through an FIR first -- auraloss's
 * perceptual_weighting=True (its 101-tap A-weighting FIR; restated, PARITY UNPINNED) or any other pre-emphasis.  taps_dev: n_taps
 * float32 on the device, n_taps odd in [1, 255], centre c = n_taps / 2.  A row x of n samples becomes
 *     p[i] = sum_{k < n_taps} taps[k] x[i + k - c],  0 <= i < n,  x = 0 outside [0, n)
 * -- torch.nn.functional.conv1d(x, taps, padding=c): cross-correlation, zero padding, same length.  Order: the peak normalisation
 * of norm_passes, under kind 1 the rows [L + R, L - R], the prefilter, then everything the unfiltered call does, applied to p: the
 * STFT's reflect padding reflects the FILTERED row.  The table side goes through the same steps.  Every p[i] is a chain of fmaf in
 * tap order from 0.0f, in the table kernel and in the candidate kernel alike, so loss(y, table_pf(y)) is exactly 0 and a candidate's
 * loss has the same bits at every position of every batch and under every slot list.  The filter runs in the kernel's loader, on
 * the tile's samples in LDS: no filtered copy of the population exists in memory.
 * kind: 0 the L/R distance (stito_mrstft_loss), 1 sum / difference (stito_mrstft_loss_sd; channels must be 2), 2 mel
 * (stito_mrstft_loss_mel; `bank` as there).  bank must be NULL unless kind is 2.  After (kind, bank, taps_dev, n_taps) the arguments
 * are those of the unfiltered calls; stito_mrstft_target_pf takes (n_targets, channels) like stito_mrstft_target_sd and writes
 * n_targets * channels rows.  stito_mrstft_loss_pf is stito_mrstft_loss_slots_pf with the identity map.  The table does not record
 * the taps: the same taps (and bank) must be given to the table call and to the loss call.
 * The prefiltered kernels need more LDS and bound a tile's span, so their tiling may differ from the unfiltered kernels': table and
 * workspace have their OWN size functions, stito_mrstft_table_floats_pf (n_bins: the bank's under kind 2, else 0) and
 * stito_mrstft_workspace_bytes_pf, which return 0 for arguments the launches refuse.
 * STITO_E_INVALID, naming the value, before any device is asked: kind outside 0 .. 2, n_taps even or outside [1, 255], null
 * taps_dev, a missing bank under kind 2 or a bank under the other kinds, channels other than 2 under kind 1. */
int64_t stito_mrstft_table_floats_pf(int kind, int n_bins, int n_taps, const int *res, int n_res, int rows, int64_t n_samples);
size_t stito_mrstft_workspace_bytes_pf(int kind, int n_taps, const int *res, int n_res, int pop, int channels, int64_t n_samples);
int stito_mrstft_target_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                           const float *y_dev, int n_targets, int channels, int64_t n_samples, float *table_dev, void *stream);
int stito_mrstft_loss_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                         const float *audio_dev, const float *peaks_dev, int norm_passes, const float *table_dev, int n_targets, int pop,
                         int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int stito_mrstft_loss_slots_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                               const float *audio_dev, const float *peaks_dev, int norm_passes, const float *table_dev, int n_targets,
                               const int32_t *target_slot_dev, int n_slots, int pop, int channels, int64_t n_samples, float *loss_dev,
                               void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- waveform distances as objectives (ABI 10.10; csrc/waveform.hip) ----------------------------------------------------------- */
/* The time-domain yardsticks auraloss.time ships beside the MR-STFT ones (ESRLoss, DCLoss, SNRLoss, SISDRLoss, LogCoshLoss;
 * restated, PARITY UNPINNED), of a rendered population against target audio, in one pass over the rows.  A row is one channel of
 * one item: x the candidate's after the peak normalisation of norm_passes (x * (1 / clip(peak, 1e-8)), as stito_mrstft_loss folds
 * it), y the target's, n_samples float32 each.  With n_taps > 0 both first go through the FIR of the prefiltered MR-STFT calls,
 * p[i] = sum_k taps[k] row[i + k - n_taps / 2] with zero padding (n_taps odd, <= 255; taps_dev on the device); n_taps 0: p = row and
 * taps_dev is not read.  d = p_x - p_y, eps = 1e-8, and per row, `kind` being
 *     0 esr      sum d^2 / (sum p_y^2 + eps)
 *     1 dc       (sum d / n)^2 / (sum p_y^2 / n + eps)
 *     2 snr      -10 log10(sum p_y^2 / (sum d^2 + eps) + eps)
 *     3 sisdr    -10 log10(sum t^2 / (sum res^2 + eps) + eps): x', y' the rows minus their means, t = alpha y',
 *                alpha = sum x' y' / (sum y'^2 + eps), res = x' - t
 *     4 logcosh  (1 / n) sum ln(cosh d + eps), a sample with d == 0 adding exactly 0 (not ln(1 + eps) = 1e-8)
 * a candidate's value is the mean over its rows.  The sums are taken in float64 in a fixed order (per lane, per tile, tiles in
 * order), without atomics: a candidate's bits are the same at every position of every batch and under every slot list, a NaN stays
 * in its candidate, and esr, dc and logcosh of y against its own table are exactly 0 (norm_passes 0).
 * stito_waveform_target: y_dev (rows, n_samples) -> table_dev (stito_waveform_table_floats floats, 16-byte aligned): the filtered rows
 * and their float64 sums; written by the kernel that filters the candidates.  The table does not record the taps: the loss call
 * takes the same.  stito_waveform_loss_slots: audio_dev (pop, channels, n_samples), channels <= 8, against a table of n_targets *
 * channels rows; target_slot_dev / n_slots as in stito_mrstft_loss_slots (NaN for a slot that names no target); workspace of
 * stito_waveform_workspace_bytes bytes, 8-byte aligned.  stito_waveform_loss is that call with the identity map.
 * stito_waveform_tile_samples: the samples of a tile (where the order of the sums changes shape), for tests to aim at.  The three
 * size functions return 0 for arguments the launches refuse.  STITO_E_INVALID, naming the value, before any launch: kind outside
 * 0 .. 4, n_taps even or outside [0, 255], null taps_dev with n_taps > 0, n_samples < 1, channels outside 1 .. 8. */
int stito_waveform_tile_samples(int n_taps);
int64_t stito_waveform_table_floats(int n_taps, int rows, int64_t n_samples);
size_t stito_waveform_workspace_bytes(int n_taps, int pop, int channels, int64_t n_samples);
int stito_waveform_target(const float *taps_dev, int n_taps, const float *y_dev, int rows, int64_t n_samples, float *table_dev,
                          void *stream);
int stito_waveform_loss(int kind, const float *taps_dev, int n_taps, const float *audio_dev, const float *peaks_dev, int norm_passes,
                        const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);
int stito_waveform_loss_slots(int kind, const float *taps_dev, int n_taps, const float *audio_dev, const float *peaks_dev, int norm_passes,
                              const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop, int channels,
                              int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- embeddings -> fitness ----------------------------------------------------------------- */
/* In place: NaN scrub (utils.py:491-497), L2-normalise mid/side (n_cand, E).  If target_mid_dev
 * is not NULL also writes loss_dev (n_cand) = mean(-cos(mid, target_mid), -cos(side, target_side))
 * (style_transfer.py:544-571); targets are (1, E). */
int stito_embed_loss(float *mid_dev, float *side_dev, int n_cand, int embed_dim,
                     const float *target_mid_dev, const float *target_side_dev, float *loss_dev,
                     int32_t *flags_dev /* (2) scratch */, void *stream);

/* Generic-metric form of the loss (any embed_func returning a dict of (n_cand, E_k) embeddings,
 * style_transfer.py:544-571): loss[c] (+)= weight * -cosine_similarity(embed[c], target), eps 1e-8.
 * The host walks the dict: first entry with accumulate = 0, the others with 1, weight = 1 / n_entries
 * (the reference's mean over the stacked distances).  embed (n_cand, embed_dim), target (embed_dim). */
int stito_neg_cosine(const float *embed_dev, int n_cand, int embed_dim, const float *target_dev, float weight,
                     int accumulate, float *loss_dev, void *stream);

/* ---- Device-resident CMA-ES (ABI 10.6): st_ito/cmaes.py's CMAEvolutionStrategy, and the run bookkeeping of run_es around it, with
 * the state on the device.  Same update rule as the host class -- from the same state and the same deviates the two agree to float64
 * summation order -- but its own random stream, so not the host's trajectory.  2 <= N <= 128, 2 <= popsize <= 1024, anything else
 * STITO_E_UNSUPPORTED naming the value; 1 <= max_iters <= 2^20.  Every call takes the (N, popsize, max_iters) the state was sized
 * with: the library keeps nothing per state.
 *
 * The state is ONE device allocation of stito_cmaes_state_bytes() bytes, 8-byte words, laid out by one function that the size query,
 * the kernels and import / export share.  stito_cmaes_state_offsets() writes the word offsets of its fields (18 values, returned count):
 *   ints, reals, mean, pc, ps, D, best_x, weights, C, B, invsqrtC, genotypes, log_f, log_x, log_disp, persist, n_ints, disp_row
 * Words [0, persist) are the state proper -- what import and export move -- and the rest is scratch.
 *   ints   (int64 x n_ints = 17): iterations done, stale, stopped, counteval | countiter, eigeneval, best_evals, N, popsize, mu,
 *          max_iters, early_stop, seed, told, need_eig, sweeps of the last decomposition, asked (an ask is pending: set by ask,
 *          cleared by tell; a tell without one returns without storing anything)
 *   reals  (double x 16): sigma, best_f, cc, cs, c1, cmu, damps, mueff, chiN, lb, ub, al, au, sum of the weights, hsig of the last
 *          tell, sigma0
 *   mean, pc, ps, D, best_x (N each), weights (popsize, negative ones included), C, B, invsqrtC (N x N, row-major), the genotypes of
 *   the last ask (popsize x N; spent by tell), then the per-iteration logs of max_iters rows: log_f / log_x = best-so-far value /
 *   vector BEFORE the iteration's tell (run_es's fval_history / wopt_history; the vector is meaningless while the value is inf),
 *   log_disp = disp_row = 8 doubles: countiter, counteval, best f of the iteration, axis ratio, sigma, min std, max std, hsig.
 * A state whose `stopped` is set (early stop: stale > 10) or that has logged max_iters iterations is FROZEN: ask, tell and eigen return
 * without storing anything (ask leaves W_dev as it is; stito_cmaes_eigen, the forced decomposition, too), so a run's result does
 * not depend on how many iterations were enqueued after the freeze.
 *
 * ask, tell, eigen and normals enqueue on `stream`, never synchronise and can be captured into a hipGraph once an eager tell (or
 * eigen) at that N has run -- the first one sets the decomposition kernel's LDS attribute, once per device; init, import, export and status BLOCK on
 * `stream` (a host copy) and must not be called while it is being captured.  The random deviates of iteration i are a pure function of
 * (seed, the state's countiter, element index): output `element` of the splitmix64 stream started at mix(mix(seed) ^ iteration), the
 * two 32-bit halves through the cosine branch of Box-Muller.  The iteration number is read from the state, not passed: a captured
 * ask / evaluate / tell sequence replays unchanged. */
int64_t stito_cmaes_state_bytes(int N, int popsize, int64_t max_iters);   /* host only; negative STITO_E_* for unsupported sizes */
int stito_cmaes_state_offsets(int N, int popsize, int64_t max_iters, int64_t *offsets, int n_offsets);   /* host only */
/* Weights and constants of CMAEvolutionStrategy.__init__ in float64 on the host, mean = BoundTransform.inverse(x0), C = B = I. */
int stito_cmaes_init(void *state_dev, int N, int popsize, const double *x0_host, double sigma0, double lb, double ub, uint64_t seed,
                     int64_t max_iters, int early_stop, void *stream);
/* z_dev: (popsize, N) standard normals used as they are, or NULL for the state's own stream.  W_dev (popsize, N) float64: the
 * phenotypes, the layout stito_render_population reads. */
int stito_cmaes_ask(void *state_dev, int N, int popsize, int64_t max_iters, const double *z_dev, double *W_dev, void *stream);
/* fitness_dev (popsize,) float32; ranks as np.argsort(kind="stable"): ascending, NaN last, ties in index order.  Two launches: the
 * update, then the lazy decomposition (which returns at once when the update did not ask for it). */
int stito_cmaes_tell(void *state_dev, int N, int popsize, int64_t max_iters, const float *fitness_dev, void *stream);
/* The decomposition of the state's C now, whatever the lazy rule says: cyclic Jacobi warm-started from B; counters untouched. */
int stito_cmaes_eigen(void *state_dev, int N, int popsize, int64_t max_iters, void *stream);
int stito_cmaes_export(const void *state_dev, int N, int popsize, int64_t max_iters, int64_t *ints_host, double *reals_host, void *stream);
int stito_cmaes_import(void *state_dev, int N, int popsize, int64_t max_iters, const int64_t *ints_host, const double *reals_host, void *stream);
/* status_host[4] = iterations done, stale, stopped, counteval */
int stito_cmaes_status(const void *state_dev, int64_t *status_host, void *stream);
/* count deviates of (seed, iteration) from element `first` on: z_dev (doubles) and / or bits_dev (the 64-bit integer stage), either NULL */
int stito_cmaes_normals(uint64_t seed, int64_t iteration, int64_t first, int64_t count, double *z_dev, uint64_t *bits_dev, void *stream);

/* ---- FX-Encoder (ABI 10.11; csrc/fxenc.hip): the reference's second learned embedding, st_ito/models/fx_encoder.py --------------
 * A stack of one-dimensional convolution layers on (n_items, channels, positions) float32 maps as torch lays them out, then the
 * mean over positions.  One layer:
 *     y[b][co][p] = relu(scale[co] * sum_{ci, t} w[co][ci][t] * x[b][ci][reflect(p * stride + t - l_pad)] + shift[co])  (+ x[b][co][p])
 * p < stito_fxenc_out_len(L, stride) = ceil(L / stride); reflection padding of kernel - 1 samples, l_pad = (kernel - 1) / 2 on
 * the left and r_pad = kernel - 1 - l_pad on the right (an even kernel pads one more on the right); L > r_pad, else STITO_E_INVALID
 * naming the layer, before anything is launched.  scale / shift: the eval-mode batch norm and the convolution's bias folded by the
 * caller in float64, scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale.  dilation must be 1 (STITO_E_UNSUPPORTED).
 *
 * Layers with more than two input channels (or a kernel / stride outside {25, 15, 10, 5} x {1, 2, 4}) run as an implicit GEMM on
 * the f32 matrix pipe, M = cout, N = n_items * out_len, reduction over r = ci * kernel + t in ascending order; the others on the
 * vector ALU.  Either way every output element is one fixed sequence of operations: an item's results do not depend on the batch
 * around it, bit for bit.  No atomics, no graph capture, eager launches on `stream`.
 *
 * w_packed_dev holds stito_fxenc_packed_floats(cout, cin, kernel, stride) floats.  With bm = stito_fxenc_tile_m(...) > 0 and
 * bk = stito_fxenc_tile_k(): [ceil(cout / bm)][Rpad][bm], Rpad = cin * kernel rounded up to bk, element (mt, r, mi) =
 * w[mt * bm + mi][r / kernel][r % kernel], zero where mt * bm + mi >= cout or r >= cin * kernel; 16-byte aligned.  bm == 0: the
 * plain (cout, cin, kernel) weights.  The packing itself is host code of the caller (st_ito/models/fx_encoder.py), done once per model. */
typedef struct {
    int32_t cin, cout, kernel, stride;
    int32_t dilation;          /* 1 */
    int32_t residual;          /* 1: + x after the ReLU (cin == cout, stride 1) */
    const float *w_packed_dev;
    const float *scale_dev;    /* (cout) */
    const float *shift_dev;    /* (cout) */
} stito_fxenc_layer;
typedef struct {
    int32_t n_layers;
    int32_t reserved;
    const stito_fxenc_layer *layers;   /* host array; layer i + 1 takes layer i's cout channels */
} stito_fxenc_model;
int64_t stito_fxenc_out_len(int64_t n_positions, int stride);              /* host only */
int stito_fxenc_tile_m(int cout, int cin, int kernel, int stride);         /* host only */
int stito_fxenc_tile_k(void);                                              /* host only */
size_t stito_fxenc_packed_floats(int cout, int cin, int kernel, int stride); /* host only */
/* one layer: x_dev (n_items, cin, n_positions) -> y_dev (n_items, cout, out_len); not in place */
int stito_fxenc_conv1d(const stito_fxenc_layer *layer, const float *x_dev, int n_items, int64_t n_positions, float *y_dev, void *stream);
/* y_dev (n_items, channels, n_positions) -> out_dev (n_items, channels): the mean over positions, one fixed summation order per row */
int stito_fxenc_pool(const float *y_dev, int n_items, int channels, int64_t n_positions, float *out_dev, void *stream);
/* The stack: x_dev (n_items, layers[0].cin, n_samples) -> out_dev (n_items, layers[n - 1].cout).  The workspace holds two buffers of
 * the largest map any layer writes; stito_fxenc_workspace_bytes returns 0 for arguments the forward would refuse. */
size_t stito_fxenc_workspace_bytes(const stito_fxenc_model *model, int n_items, int64_t n_samples);
int stito_fxenc_forward(const stito_fxenc_model *model, const float *x_dev, int n_items, int64_t n_samples, void *workspace_dev,
                        size_t workspace_bytes, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STITO_HIP_H */
