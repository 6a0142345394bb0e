// audio_distance.h -- what mrstft.hip and waveform.hip share: which target a candidate is scored against, the folded peak, the FIR
// prefilter's register window, the tile's fixed-order sums, the host checks of a loss call.  Both files are built without fp
// contraction; every multiply-add here is explicit.
#pragma once
#include "common.h"

namespace stito {

// a prefilter's taps are taken in blocks of four: a raw run reaches AD_TAP_REACH past its last whole float4
static constexpr int AD_MAX_TAPS = 255, AD_TAP_REACH = 256;

// Table target of candidate `cand`: population k = cand / per_target reads target slots[k], or target k when there is no slot
// list.  -1 for a slot that names no target: such a candidate reads nothing, writes no partial, and the final kernel gives it NaN.
__device__ __forceinline__ int ad_target_of(int64_t cand, int per_target, const int32_t *__restrict__ slots, int n_targets) {
    const int k = (int)(cand / per_target);
    const int t = slots != nullptr ? slots[k] : k;
    return (t >= 0 && t < n_targets) ? t : -1;
}

// The folded peak normalisation: the loaders score x * (1 / clip(peak, 1e-8)), as stito_logmel's does.
__device__ __forceinline__ float ad_peak_scale(const float *__restrict__ peaks, int norm_passes, int64_t cand) {
    return (peaks != nullptr && norm_passes > 0) ? 1.0f / fmaxf(peaks[cand], 1e-8f) : 1.0f;
}

// The prefilter on four consecutive outputs: p[o] = sum_k taps[k] raw[o + k], o = 4 g .. 4 g + 3, of the staged raw run (16-byte aligned,
// readable up to raw[4 g + 4 (n_taps / 4) + 7]; n_taps odd).  A sliding register window; each output's chain is fmaf in tap order from 0.0f.
__device__ __forceinline__ float4 ad_fir_run(const float *raw, int g, const float *__restrict__ taps, int n_taps) {
    // the same taps for every lane, written by nobody: through the constant address space they are scalar loads into SGPRs
    typedef const __attribute__((address_space(4))) float *ctaps_t;
    ctaps_t ctaps = (ctaps_t)(uintptr_t)taps;
    const int kb_full = n_taps >> 2, tail = n_taps & 3;           // n_taps is odd: 1 or 3 taps behind the whole blocks
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float4 *rp = (const float4 *)raw + g;
    float4 lo = rp[0];
    for (int kb = 0; kb < kb_full; ++kb) {
        const float4 hi = rp[kb + 1];
        const float4 t = make_float4(ctaps[4 * kb], ctaps[4 * kb + 1], ctaps[4 * kb + 2], ctaps[4 * kb + 3]);
        a0 = fmaf(t.x, lo.x, a0); a1 = fmaf(t.x, lo.y, a1); a2 = fmaf(t.x, lo.z, a2); a3 = fmaf(t.x, lo.w, a3);
        a0 = fmaf(t.y, lo.y, a0); a1 = fmaf(t.y, lo.z, a1); a2 = fmaf(t.y, lo.w, a2); a3 = fmaf(t.y, hi.x, a3);
        a0 = fmaf(t.z, lo.z, a0); a1 = fmaf(t.z, lo.w, a1); a2 = fmaf(t.z, hi.x, a2); a3 = fmaf(t.z, hi.y, a3);
        a0 = fmaf(t.w, lo.w, a0); a1 = fmaf(t.w, hi.x, a1); a2 = fmaf(t.w, hi.y, a2); a3 = fmaf(t.w, hi.z, a3);
        lo = hi;
    }
    const float4 hi = rp[kb_full + 1];
    const float t0 = ctaps[4 * kb_full];                          // no read behind the last tap
    a0 = fmaf(t0, lo.x, a0); a1 = fmaf(t0, lo.y, a1); a2 = fmaf(t0, lo.z, a2); a3 = fmaf(t0, lo.w, a3);
    if (tail == 3) {
        const float t1 = ctaps[4 * kb_full + 1], t2 = ctaps[4 * kb_full + 2];
        a0 = fmaf(t1, lo.y, a0); a1 = fmaf(t1, lo.z, a1); a2 = fmaf(t1, lo.w, a2); a3 = fmaf(t1, hi.x, a3);
        a0 = fmaf(t2, lo.z, a0); a1 = fmaf(t2, lo.w, a1); a2 = fmaf(t2, hi.x, a2); a3 = fmaf(t2, hi.y, a3);
    }
    return make_float4(a0, a1, a2, a3);
}

// The tile's K sums over its THREADS threads, float64: a fixed tree in LDS, so the order of the adds is a property of the tile.
// All threads of the workgroup; on return red[k][0] is sum k.
template <int K, int THREADS>
__device__ __forceinline__ void ad_tile_tree(double (*red)[THREADS], const double (&acc)[K], int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + s];
        }
        __syncthreads();
    }
}

// The taps of a call.  zero_is_none: 0 taps stands for "no prefilter" (then taps_dev is not looked at).
static int ad_taps_check(const char *who, const float *taps_dev, int n_taps, bool zero_is_none) {
    STITO_REQUIRE(n_taps >= (zero_is_none ? 0 : 1) && n_taps <= AD_MAX_TAPS, STITO_E_INVALID,
                  zero_is_none ? "%s: n_taps %d, 0 (no prefilter) .. %d are supported" : "%s: n_taps %d, 1 .. %d are supported", who, n_taps, AD_MAX_TAPS);
    STITO_REQUIRE(n_taps == 0 || (n_taps & 1) == 1, STITO_E_INVALID, "%s: n_taps %d must be odd (the filter is centred on tap n_taps / 2)", who,
                  n_taps);
    STITO_REQUIRE(n_taps == 0 || taps_dev != nullptr, STITO_E_INVALID, "%s: null taps_dev", who);
    return STITO_OK;
}

// What a loss call checks of its arguments, in the order the calls report them: populations of pop / n_slots candidates against
// n_targets targets, the caller's own rule for the channel count (channels_check() -> status), the folded peaks, the pointers.
template <class ChannelsCheck>
static int ad_loss_args_check(const char *who, int pop, int n_targets, int n_slots, ChannelsCheck channels_check, int norm_passes,
                              const float *peaks_dev, const float *audio_dev, const float *table_dev, const float *loss_dev) {
    STITO_REQUIRE(pop >= 1 && n_targets >= 1, STITO_E_INVALID, "%s: pop %d, n_targets %d", who, pop, n_targets);
    STITO_REQUIRE(n_slots >= 1, STITO_E_INVALID, "%s: %d target slots", who, n_slots);
    STITO_REQUIRE(pop % n_slots == 0, STITO_E_INVALID, "%s: population %d is not a multiple of the number of targets %d", who, pop, n_slots);
    STITO_TRY(channels_check());
    STITO_REQUIRE(norm_passes == 0 || norm_passes == 1, STITO_E_INVALID, "%s: norm_passes %d must be 0 or 1", who, norm_passes);
    STITO_REQUIRE(norm_passes == 0 || peaks_dev != nullptr, STITO_E_INVALID, "%s: norm_passes 1 needs the peaks", who);
    STITO_REQUIRE(audio_dev != nullptr && table_dev != nullptr && loss_dev != nullptr, STITO_E_INVALID, "%s: null pointer", who);
    STITO_REQUIRE(((uintptr_t)table_dev & 15) == 0, STITO_E_INVALID, "%s: the table must be 16-byte aligned", who);
    return STITO_OK;
}

// ... and of its workspace.  ("too many tiles" stays in each file: behind this in mrstft.hip, in front of it in waveform.hip.)
static int ad_workspace_check(const char *who, const void *workspace_dev, size_t workspace_bytes, size_t need) {
    STITO_REQUIRE(workspace_dev != nullptr && workspace_bytes >= need, STITO_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
                  workspace_bytes, need);
    STITO_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, STITO_E_INVALID, "%s: the workspace must be 8-byte aligned", who);
    return STITO_OK;
}

}  // namespace stito
