// juce::dsp::Compressor<float>::update + BallisticsFilter coefficients, shared by the effect chain's compressor (dsp.hip,
// k_prepare) and the rule-based hill-climb (matcheq.hip, k_climb_coef): one restatement of the JUCE arithmetic.
#pragma once
#include "common.h"

namespace stito {

// juce::Decibels::decibelsToGain<float>
__device__ __forceinline__ float db_to_gain(float db, float minus_inf) {
    return db > minus_inf ? powf(10.0f, db * 0.05f) : 0.0f;
}

// o[0..4] = threshold gain, its inverse, 1/ratio - 1, attack and release one-pole constants (the row k_comp_* read)
__device__ __forceinline__ void juce_compressor_coef(double threshold_db, double ratio, double attack_ms, double release_ms,
                                                     double sr, double *o) {
    const float thr = db_to_gain((float)threshold_db, -200.0f);
    const float expf_ = (float)(-2.0 * M_PI * 1000.0 / sr);
    const float at = (float)attack_ms, rl = (float)release_ms;
    o[0] = thr;
    o[1] = 1.0f / thr;
    o[2] = 1.0f / (float)ratio - 1.0f;
    // the one-pole coefficients sit next to 1 and the envelope only sees 1 - c: one ulp of c is up to 3e-5 of
    // (1 - c).  exp in double of the float32 argument, rounded once, is the correctly rounded expf the host libm
    // returns (ocml's expf is allowed 1 ulp)
    o[3] = at < 1.0e-3f ? 0.0f : (float)exp((double)(expf_ / at));
    o[4] = rl < 1.0e-3f ? 0.0f : (float)exp((double)(expf_ / rl));
}

}  // namespace stito
